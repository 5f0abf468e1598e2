"""Test-side driver of matlab/admm_mex.cpp linked with the MEX stand-in of tests/mex_shim (no MATLAB anywhere): MATLAB values
as plain Python data, a ctypes front end to the bridge (mex_bridge.cpp), a writer of the same calls as a script for the
stand-alone replay program (mex_replay.cpp), and the catalogue of accepted problem forms and refusals both of them run.

A MATLAB value is: MX (numeric / logical array), str (char row), dict (1 x 1 struct), Ref (an output saved by an earlier step).
A step is (nlhs, args, expect, save): expect is "ok" or the identifier of the error the call must raise."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "mex_shim")
GATEWAY = os.path.join(ROOT, "matlab", "admm_mex.cpp")

# matrix.h
CLASS = {"logical": 3, "char": 4, "double": 6, "single": 7, "int32": 12, "uint64": 15, "struct": 2}
DTYPE = {3: np.uint8, 4: np.uint16, 6: np.float64, 7: np.float32, 12: np.int32, 15: np.uint64}


@dataclasses.dataclass
class MX:
    """A numeric / logical MATLAB array: class id, the dimensions AS GIVEN to the creation call (the stand-in drops trailing
    singletons as MATLAB does) and the column-major data."""
    cls: int
    dims: tuple
    data: np.ndarray
    complex: bool = False
    sparse: bool = False


def mx(a, cls="double", dims=None, **kw):
    """MX of an array indexed as MATLAB indexes it (shape = MATLAB dimensions); a scalar becomes 1 x 1."""
    a = np.asarray(a)
    if a.ndim == 0:
        a = a.reshape(1, 1)
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    return MX(CLASS[cls], tuple(dims or a.shape), np.ascontiguousarray(a.flatten(order="F"), DTYPE[CLASS[cls]]), **kw)


def raw(buf, dims, cls="double"):
    """MX over a buffer that is already column-major (what _abi.marshal_problem lays out for the C ABI)."""
    return MX(CLASS[cls], tuple(dims), np.ascontiguousarray(np.asarray(buf).reshape(-1), DTYPE[CLASS[cls]]))


EMPTY = MX(6, (0, 0), np.zeros(0))


@dataclasses.dataclass
class Ref:
    name: str


@dataclasses.dataclass
class Out:
    cls: int
    dims: tuple
    data: object          # np array (column-major, flat) or dict for a struct
    ptr: int = 0

    def array(self):
        return self.data.reshape(self.dims, order="F")


@dataclasses.dataclass
class Result:
    rc: int
    error_id: str
    error_text: str
    warnings: list
    outputs: list
    orphans: int
    ptrs: dict            # data pointer of every input array: "arg<i>" or "arg<i>.<field>"


def compile_shared(out, extra_sources=(), extra_flags=()):
    """gateway + stand-in + bridge (+ extra) into one shared object."""
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I", SHIM, "-I",
           os.path.join(ROOT, "include"), GATEWAY, os.path.join(SHIM, "mex_standin.cpp"), os.path.join(SHIM, "mex_bridge.cpp"),
           *extra_sources, *extra_flags, "-o", str(out)]
    subprocess.run(cmd, check=True)
    return str(out)


class Bridge:
    def __init__(self, path):
        self.lib = lib = C.CDLL(path)
        vp, cp, i, u64 = C.c_void_p, C.c_char_p, C.c_int, C.c_uint64
        sig = {"msb_numeric": (vp, [i, i, i, i, C.POINTER(u64), vp, u64]), "msb_string": (vp, [cp]),
               "msb_struct": (vp, [i, C.POINTER(cp)]), "msb_set_field": (None, [vp, cp, vp]), "msb_destroy": (None, [vp]),
               "msb_call": (i, [i, i, C.POINTER(vp)]), "msb_output": (vp, [i]), "msb_orphans": (i, []),
               "msb_class": (i, [vp]), "msb_ndim": (i, [vp]), "msb_dim": (u64, [vp, i]), "msb_numel": (u64, [vp]),
               "msb_element_size": (u64, [vp]), "msb_data": (vp, [vp]), "msb_nfields": (i, [vp]),
               "msb_field_name": (cp, [vp, i]), "msb_field": (vp, [vp, cp]), "msb_live": (i, []),
               "msb_warning_count": (i, []), "msb_warning_id": (cp, [i]), "msb_warning_text": (cp, [i]),
               "msb_error_id": (cp, []), "msb_error_text": (cp, []), "msb_at_exit_registrations": (i, []),
               "msb_fire_at_exit": (i, [])}
        for name, (res, args) in sig.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        self.saved = {}

    # -- Python value -> mxArray* ------------------------------------------------------------------------------------
    def _make(self, v, ptrs, key):
        lib = self.lib
        if isinstance(v, Ref):
            v = self.saved[v.name]
        if isinstance(v, Out):
            v = MX(v.cls, v.dims, v.data)
        if isinstance(v, str):
            return lib.msb_string(v.encode())
        if isinstance(v, dict):
            names = (C.c_char_p * len(v))(*[k.encode() for k in v])
            s = lib.msb_struct(len(v), names)
            for k, f in v.items():
                lib.msb_set_field(s, k.encode(), self._make(f, ptrs, f"{key}.{k}"))
            return s
        dims = (C.c_uint64 * len(v.dims))(*v.dims)
        a = lib.msb_numeric(v.cls, int(v.complex), int(v.sparse), len(v.dims), dims, v.data.ctypes.data_as(C.c_void_p),
                            v.data.nbytes)
        assert a, "data do not fill the dimensions"
        ptrs[key] = lib.msb_data(a) or 0
        return a

    # -- mxArray* -> Python value ------------------------------------------------------------------------------------
    def _read(self, a):
        lib = self.lib
        cls = lib.msb_class(a)
        dims = tuple(lib.msb_dim(a, k) for k in range(lib.msb_ndim(a)))
        if cls == CLASS["struct"]:
            names = [lib.msb_field_name(a, k).decode() for k in range(lib.msb_nfields(a))]
            return Out(cls, dims, {k: self._read(lib.msb_field(a, k.encode())) for k in names})
        n, p = lib.msb_numel(a), lib.msb_data(a) or 0
        data = np.frombuffer(C.string_at(p, n * lib.msb_element_size(a)), DTYPE[cls]).copy() if n else np.zeros(0, DTYPE[cls])
        return Out(cls, dims, data, p)

    def call(self, nlhs, *args, save=None):
        """mexFunction(nlhs, plhs, len(args), args) as MATLAB calls it; inputs and outputs are destroyed afterwards (the outputs
        after they were read; `save` keeps output 0 for Ref(save))."""
        lib = self.lib
        ptrs = {}
        made = [self._make(v, ptrs, f"arg{k}") for k, v in enumerate(args)]
        prhs = (C.c_void_p * max(len(made), 1))(*made)
        rc = lib.msb_call(nlhs, len(made), prhs)
        outs = []
        if rc == 0:
            for k in range(max(nlhs, 1)):
                o = lib.msb_output(k)
                outs.append(self._read(o) if o else None)
                if o:
                    lib.msb_destroy(o)
            if save:
                self.saved[save] = outs[0]
        for a in made:
            lib.msb_destroy(a)
        warns = [(lib.msb_warning_id(k).decode(), lib.msb_warning_text(k).decode()) for k in range(lib.msb_warning_count())]
        return Result(rc, lib.msb_error_id().decode(), lib.msb_error_text().decode(), warns, outs, lib.msb_orphans(), ptrs)

    def run(self, steps):
        """Run steps; assert each one's expectation; return the results."""
        res = []
        for nlhs, args, expect, save in steps:
            r = self.call(nlhs, *args, save=save)
            assert (r.error_id or "ok") == expect and r.rc == (expect != "ok"), (expect, r.rc, r.error_id, r.error_text, args[:1])
            res.append(r)
        return res

    def live(self):
        return self.lib.msb_live()

    def fire_at_exit(self):
        return self.lib.msb_fire_at_exit()


class StubControl:
    """ctypes front end of admm_stub.cpp's control surface."""

    def __init__(self, lib):
        self.lib = lib
        cp, i = C.c_char_p, C.c_int
        sig = {"stub_reset": (None, []), "stub_fail": (None, [cp, i, cp]), "stub_warn": (None, [cp, cp]),
               "stub_clear_faults": (None, []), "stub_set_history": (None, [i]), "stub_calls": (i, [cp]),
               "stub_total_calls": (i, []), "stub_has": (i, [cp]), "stub_num": (C.c_double, [cp]),
               "stub_ptr": (C.c_uint64, [cp]), "stub_handles": (i, []), "stub_frees": (i, [i]), "stub_handle": (C.c_uint64, [i])}
        for name, (res, args) in sig.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args

    def reset(self):
        self.lib.stub_reset()

    def fail(self, sym, code, text):
        self.lib.stub_fail(sym.encode(), code, text.encode())

    def warn(self, sym, text):
        self.lib.stub_warn(sym.encode(), text.encode())

    def clear_faults(self):
        self.lib.stub_clear_faults()

    def set_history(self, k):
        self.lib.stub_set_history(k)

    def calls(self, sym=None):
        return self.lib.stub_total_calls() if sym is None else self.lib.stub_calls(sym.encode())

    def num(self, key):
        assert self.lib.stub_has(key.encode()), key
        return self.lib.stub_num(key.encode())

    def ptr(self, key):
        return self.lib.stub_ptr(key.encode())

    def frees(self):
        return [self.lib.stub_frees(k) for k in range(self.lib.stub_handles())]

    def handles(self):
        return [self.lib.stub_handle(k) for k in range(self.lib.stub_handles())]


# ---- the same steps as a script for the stand-alone replay program (mex_replay.cpp) -----------------------------------------
class Script:
    def __init__(self):
        self.lines = []
        self.k = 0

    def _emit(self, v):
        if isinstance(v, Ref):
            return "@" + v.name
        self.k += 1
        name = f"v{self.k}"
        if isinstance(v, str):
            assert v and " " not in v
            self.lines.append(f"S {name} {v}")
        elif isinstance(v, dict):
            ids = [(k, self._emit(f)) for k, f in v.items()]
            self.lines.append(f"T {name} {len(ids)} " + " ".join(f"{k} {i}" for k, i in ids))
        else:
            vals = " ".join(repr(float(x)) for x in v.data)
            self.lines.append(f"N {name} {v.cls} {int(v.complex)} {int(v.sparse)} {len(v.dims)} " + " ".join(str(d) for d in v.dims) +
                              f" {len(v.data)} {vals}".rstrip())
        return name

    def steps(self, steps):
        for nlhs, args, expect, save in steps:
            ids = [self._emit(a) for a in args]
            self.lines.append(f"C {nlhs} {expect} {save or '-'} {len(ids)} " + " ".join(ids))

    def fail(self, sym, code, text):
        self.lines.append(f"F {sym} {code} {text}")

    def reset(self):
        self.lines.append("R")

    def text(self):
        return "\n".join(self.lines) + "\n"


# ---- the catalogue: accepted forms and refusals -------------------------------------------------------------------------------
def ints(rng, *shape):
    """Small integer-valued doubles: their sum is exact in any order, so the stub's sum equals NumPy's bit for bit."""
    return rng.integers(-9, 10, size=shape).astype(np.float64)


def make_problem(N=4, n=3, m=2, batch=5, dyn="lti", box="shared", q=False, unorm=None, fuel=None, seed=0):
    """A problem struct (dict of MX) in the form asked for, with the dimensions MATLAB would give the arrays.
    dyn: lti | ltv | per_instance;  box: shared | stage | per_instance;  unorm / fuel: None | 1 | "N"."""
    rng = np.random.default_rng(seed)
    nb = n + m
    ashape = {"lti": (n, n), "ltv": (n, n, N), "per_instance": (n, n, N, batch)}[dyn]
    bshape = {"lti": (n, m), "ltv": (n, m, N), "per_instance": (n, m, N, batch)}[dyn]
    boxshape = {"shared": (nb, 1), "stage": (nb, N), "per_instance": (nb, N, batch)}[box]
    lo = -1.0 - np.abs(ints(rng, *boxshape))
    p = {"N": mx(float(N)), "A": mx(ints(rng, *ashape)), "B": mx(ints(rng, *bshape)), "Q": mx(ints(rng, n, n)),
         "R": mx(ints(rng, m, m)), "QN": mx(ints(rng, n, n)), "x0": mx(ints(rng, n, batch)), "lo": mx(lo),
         "hi": mx(1.0 + np.abs(ints(rng, *boxshape)))}
    if dyn == "per_instance":
        p["per_instance"] = mx(1, "logical")
    if box == "per_instance":
        p["per_instance_bounds"] = mx(1, "logical")
    if q:
        p["q"] = mx(ints(rng, N * nb, batch))
    for name, v in (("unorm", unorm), ("fuel", fuel)):
        if v is not None:
            p[name] = mx(1.0 + np.abs(ints(rng, N if v == "N" else 1, 1)))
    return p


def expected_form(N, n, m, batch, dyn, box):
    """(time_varying, stage_bounds) the library must be told: a singleton the array cannot carry degenerates harmlessly."""
    tv = 2 if dyn == "per_instance" else (1 if dyn == "ltv" and N > 1 else 0)
    sb = 2 if box == "per_instance" else (1 if box == "stage" and N > 1 else 0)
    return tv, sb


ACCEPTED = [
    # every form of dynamics and of the box
    dict(dyn="lti", box="shared"), dict(dyn="ltv", box="shared"), dict(dyn="ltv", box="stage"), dict(dyn="lti", box="stage"),
    dict(dyn="per_instance", box="shared"), dict(dyn="per_instance", box="stage"), dict(dyn="per_instance", box="per_instance"),
    # q, unorm and fuel with 1 and with N entries
    dict(q=True), dict(dyn="ltv", q=True), dict(unorm=1), dict(box="stage", unorm="N"), dict(fuel=1), dict(box="stage", fuel="N"),
    dict(box="stage", unorm="N", fuel="N", q=True),
    # MATLAB's dimension edges: trailing singletons are gone before the gateway sees the array
    dict(batch=1), dict(m=1), dict(n=1), dict(n=1, m=1, batch=1),
    dict(N=1, dyn="ltv", box="stage"),                         # 3-D inputs arrive 2-D
    dict(N=1, dyn="ltv", box="stage", unorm="N", fuel="N"),
    dict(batch=1, dyn="per_instance", box="per_instance"),     # 4-D arrives 3-D
    dict(batch=1, N=1, dyn="per_instance", box="per_instance"),  # ... and 2-D
    dict(batch=1, dyn="ltv", box="stage", q=True), dict(m=1, dyn="ltv"), dict(n=1, dyn="per_instance"),
]


def accepted_id(kw):
    return "-".join(f"{k}={v}" for k, v in kw.items()) or "default"


def _with(p, **repl):
    out = dict(p)
    for k, v in repl.items():
        if v is None:
            out.pop(k)
        else:
            out[k] = v
    return out


def refusals():
    """label -> steps.  The last step of each must be refused with admm:input; the steps before it set the scene."""
    N, n, m, batch = 4, 3, 2, 5
    nb, L = n + m, N * (n + m)
    rng = np.random.default_rng(5)
    lti, ltv = make_problem(), make_problem(dyn="ltv", box="stage")
    pin = make_problem(dyn="per_instance", box="per_instance")
    setup = lambda p, *o: [(1, ("setup", p, *o), "admm:input", None)]          # noqa: E731
    ok = (1, ("setup", lti), "ok", "h")
    on_handle = lambda *args, nlhs=0: [ok, (nlhs, args, "admm:input", None)]    # noqa: E731
    r = {
        # the pages of B against those of A (the out-of-bounds read this catalogue was written for)
        "B-2d-with-A-3d": setup(_with(ltv, B=lti["B"])),
        "B-short-pages": setup(_with(ltv, B=mx(ints(rng, n, m, N - 1)))),
        "B-3d-with-A-2d": setup(_with(lti, B=ltv["B"])),
        "A-pages": setup(_with(ltv, A=mx(ints(rng, n, n, N + 1)))),
        "A-not-square": setup(_with(lti, A=mx(ints(rng, n, n - 1)))),
        "A-rows": setup(_with(lti, A=mx(ints(rng, n - 1, n)))),
        "A-smaller": setup(_with(lti, A=mx(ints(rng, n - 1, n - 1)))),
        "A-4d-without-flag": setup(_with(pin, per_instance=None, per_instance_bounds=None, lo=lti["lo"], hi=lti["hi"])),
        "A-per-instance-short": setup(_with(pin, A=mx(ints(rng, n, n, N, batch - 1)))),
        "B-per-instance-short": setup(_with(pin, B=mx(ints(rng, n, m, N, batch - 1)))),
        "A-per-instance-swapped": setup(_with(pin, A=mx(ints(rng, n, n, batch, N)))),
        "Q-size": setup(_with(lti, Q=mx(ints(rng, n - 1, n - 1)))),
        "Q-3d": setup(_with(lti, Q=mx(ints(rng, n, n, 2)))),
        "R-size": setup(_with(lti, R=mx(ints(rng, m - 1, m - 1)))),
        "R-as-n-by-n": setup(_with(lti, R=mx(ints(rng, n, n)))),
        "QN-size": setup(_with(lti, QN=mx(ints(rng, n, n - 1)))),
        "hi-columns": setup(_with(ltv, hi=lti["hi"])),
        "hi-columns-more": setup(_with(lti, hi=ltv["hi"])),
        "lo-rows": setup(_with(lti, lo=mx(-np.ones((nb - 1, 1))), hi=mx(np.ones((nb - 1, 1))))),
        "lo-columns": setup(_with(lti, lo=mx(-np.ones((nb, N - 1))), hi=mx(np.ones((nb, N - 1))))),
        "box-per-instance-short": setup(_with(pin, lo=mx(-np.ones((nb, N, batch - 1))), hi=mx(np.ones((nb, N, batch - 1))))),
        "box-per-instance-without-dynamics": setup(_with(lti, per_instance_bounds=mx(1, "logical"))),
        "x0-rows": setup(_with(lti, x0=mx(ints(rng, n + 1, batch)))),
        "x0-3d": setup(_with(lti, x0=mx(ints(rng, n, batch, 2)))),
        "q-rows": setup(_with(lti, q=mx(ints(rng, L - 1, batch)))),
        "q-columns": setup(_with(lti, q=mx(ints(rng, L, batch + 1)))),
        "q-transposed": setup(_with(lti, q=mx(ints(rng, batch, L)))),
        "unorm-N-with-shared-box": setup(_with(lti, unorm=mx(np.ones((N, 1))))),
        "unorm-1-with-stage-box": setup(_with(ltv, unorm=mx(1.0))),
        "fuel-N-with-shared-box": setup(_with(lti, fuel=mx(np.ones((N, 1))))),
        "fuel-2": setup(_with(ltv, fuel=mx(np.ones((2, 1))))),
        # classes
        "A-int32": setup(_with(lti, A=mx(np.ones((n, n)), "int32"))),
        "A-single": setup(_with(lti, A=mx(np.ones((n, n)), "single"))),
        "A-logical": setup(_with(lti, A=mx(np.ones((n, n)), "logical"))),
        "A-complex": setup(_with(lti, A=mx(np.ones((n, n)), complex=True))),
        "x0-sparse": setup(_with(lti, x0=mx(np.ones((n, batch)), sparse=True))),
        "q-single": setup(_with(lti, q=mx(np.ones((L, batch)), "single"))),
        "A-empty": setup(_with(lti, A=EMPTY)),
        "B-empty": setup(_with(lti, B=EMPTY)),
        "N-empty": setup(_with(lti, N=EMPTY)),
        "N-vector": setup(_with(lti, N=mx(np.array([4.0, 4.0])))),
        "N-zero": setup(_with(lti, N=mx(0.0))),
        "N-fraction": setup(_with(lti, N=mx(4.5))),
        "N-string": setup(_with(lti, N="4")),
        "problem-not-a-struct": setup(mx(np.ones((3, 3)))),
        "problem-absent": [(1, ("setup",), "admm:input", None)],
        "options-not-a-struct": setup(lti, mx(0.5)),
        # the command
        "no-arguments": [(0, (), "admm:input", None)],
        "command-not-a-string": [(0, (mx(1.0),), "admm:input", None)],
        "command-unknown": [(0, ("frobnicate",), "admm:input", None)],
        "command-unknown-with-handle": on_handle("frobnicate", Ref("h")),
        "command-too-long": on_handle("get" + "x" * 40, Ref("h")),
        # the handle
        "handle-absent": [(0, ("get",), "admm:input", None)],
        "handle-double": on_handle("get", mx(12345.0)),
        "handle-two": on_handle("get", mx(np.array([1, 2]), "uint64")),
        "handle-null": on_handle("get", mx(0, "uint64")),
        "handle-unknown": on_handle("get", mx(0x1234560, "uint64")),
        "handle-freed": [ok, (0, ("free", Ref("h")), "ok", None), (1, ("get", Ref("h")), "admm:input", None)],
        "handle-freed-twice": [ok, (0, ("free", Ref("h")), "ok", None), (0, ("free", Ref("h")), "admm:input", None)],
        # arguments of the commands on a handle
        "z0-count": on_handle("solve", Ref("h"), mx(ints(rng, L - 1, batch)), nlhs=1),
        "y0-count": on_handle("solve", Ref("h"), EMPTY, mx(ints(rng, L, batch + 1)), nlhs=1),
        "z0-single": on_handle("solve", Ref("h"), mx(np.ones((L, batch)), "single"), nlhs=1),
        "iterate-without-count": on_handle("iterate", Ref("h")),
        "iterate-empty-count": on_handle("iterate", Ref("h"), EMPTY),
        "update-not-a-struct": on_handle("update", Ref("h"), mx(1.0)),
        "update-wrong-B": [ok, (0, ("update", Ref("h"), _with(ltv, B=lti["B"])), "admm:input", None)],
        "update-other-batch": [ok, (0, ("update", Ref("h"), make_problem(batch=batch + 1)), "admm:input", None)],
    }
    for name in ("A", "B", "Q", "R", "QN", "x0", "lo", "hi", "N"):
        r[f"missing-{name}"] = setup(_with(lti, **{name: None}))
    return r


def setup_steps(kw, options=None):
    """setup of an accepted form, then every command on the handle, then free."""
    p = make_problem(**kw)
    d = dict(N=4, n=3, m=2, batch=5)
    d.update({k: v for k, v in kw.items() if k in d})
    L = d["N"] * (d["n"] + d["m"])
    z0 = mx(np.arange(L * d["batch"], dtype=np.float64).reshape(L, d["batch"]))
    return [(1, ("setup", p) + ((options,) if options is not None else ()), "ok", "h"),
            (0, ("iterate", Ref("h"), mx(3.0)), "ok", None), (3, ("get", Ref("h")), "ok", None),
            (1, ("solve", Ref("h")), "ok", None), (1, ("solve", Ref("h"), z0, z0), "ok", None),
            (1, ("solve", Ref("h"), EMPTY, z0), "ok", None), (0, ("update", Ref("h"), p), "ok", None),
            (1, ("history", Ref("h")), "ok", None), (1, ("path", Ref("h")), "ok", None), (0, ("get", Ref("h")), "ok", None),
            (0, ("free", Ref("h")), "ok", None)]
