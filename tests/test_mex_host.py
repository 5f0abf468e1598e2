"""matlab/admm_mex.cpp, executed: the gateway is linked with a functional stand-in for the MEX API (tests/mex_shim: it restates
MathWorks' documented behaviour, it is not MATLAB) and a stub of the C ABI that records what it is given, reads every element
the header entitles the library to read and writes every element it may write.  No GPU, no HIP: what is tested is the
marshalling -- sizes, classes, pointers, options, errors, warnings, the handle table -- which is all the gateway does."""
import os
import re
import subprocess

import numpy as np
import pytest

import _mex
from _mex import EMPTY, Ref, mx

SHIM = _mex.SHIM
STUB = os.path.join(SHIM, "admm_stub.cpp")
N, n, m, batch = 4, 3, 2, 5          # the catalogue's default shape
L = N * (n + m)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """gateway + stand-in + bridge + stub in one shared object, compiled once."""
    so = _mex.compile_shared(tmp_path_factory.mktemp("mex") / "admm_mex_host.so", [STUB])
    b = _mex.Bridge(so)
    return b, _mex.StubControl(b.lib)


@pytest.fixture
def mexf(host):
    """A clean gateway for one test: no handle in its table, a fresh stub; afterwards nothing may be left alive."""
    b, stub = host
    b.fire_at_exit()
    stub.reset()
    b.saved.clear()
    yield b, stub
    b.fire_at_exit()
    stub.reset()
    assert b.live() == 0


def dims_of(kw):
    d = dict(N=N, n=n, m=m, batch=batch)
    d.update({k: v for k, v in kw.items() if k in d})
    return d


# ---- marshalling of every accepted form ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", _mex.ACCEPTED, ids=_mex.accepted_id)
@pytest.mark.parametrize("command", ["setup", "update"])
def test_accepted_forms_arrive_as_given(mexf, kw, command):
    """Sizes and forms as expected, every pointer the input's own (no copies), every element readable: the stub's sum over what
    admm_hip.h lets it read is NumPy's sum (integer data: exact in any order)."""
    b, stub = mexf
    d = dims_of(kw)
    p = _mex.make_problem(**kw)
    if command == "setup":
        r = b.call(1, "setup", p, save="h")
        key, sym = "arg1", "admm_setup_fuel"
    else:
        b.run([(1, ("setup", _mex.make_problem(seed=9, **kw)), "ok", "h")])
        r = b.call(0, "update", Ref("h"), p)
        key, sym = "arg2", "admm_update_problem"
    assert r.rc == 0, (r.error_id, r.error_text)
    assert r.warnings == [] and r.orphans == 0 and stub.calls(sym) == 1
    tv, sb = _mex.expected_form(d["N"], d["n"], d["m"], d["batch"], kw.get("dyn", "lti"), kw.get("box", "shared"))
    got = {k: stub.num(k) for k in ("N", "n", "m", "batch", "time_varying", "stage_bounds")}
    assert got == dict(N=d["N"], n=d["n"], m=d["m"], batch=d["batch"], time_varying=tv, stage_bounds=sb)
    names = ["A", "B", "Q", "R", "QN", "x0", "lo", "hi", "q", "unorm"] + (["fuel"] if command == "setup" else [])
    for name in names:
        if name in p:
            assert stub.ptr(name) == r.ptrs[f"{key}.{name}"] != 0, name
            assert stub.num("count_" + name) == p[name].data.size, name
            assert stub.num("sum_" + name) == p[name].data.sum(), name
        else:
            assert stub.ptr(name) == 0, name
    if command == "setup":
        h = r.outputs[0]
        assert h.cls == _mex.CLASS["uint64"] and h.dims == (1, 1) and int(h.data[0]) == stub.handles()[0]


def test_every_command_on_every_form_leaves_nothing_behind(mexf):
    b, stub = mexf
    for kw in _mex.ACCEPTED:
        for r in b.run(_mex.setup_steps(kw)):
            assert r.orphans == 0
        assert b.live() == 0
    assert stub.frees() == [1] * len(_mex.ACCEPTED)


# ---- options --------------------------------------------------------------------------------------------------------------------
OPTION_VALUES = dict(rho=0.625, alpha=1.5, eps_abs=2e-7, eps_rel=3e-8, max_iter=77, check_interval=11, segments=6, device=1,
                     flags=72, adapt_interval=22, adapt_max=5, adapt_mu=12.5, adapt_tau=3.5, precision_mode=1)
STUB_DEFAULTS = dict(rho=0.375, alpha=1.25, eps_abs=3e-5, eps_rel=7e-4, max_iter=123, check_interval=7, segments=3, device=2,
                     zrows=11, flags=5, adapt_interval=21, adapt_max=9, adapt_mu=4.5, adapt_tau=1.75, precision_mode=2, reserved=0)


def test_every_option_field_arrives(mexf):
    b, stub = mexf
    b.run([(1, ("setup", _mex.make_problem(), {k: mx(float(v)) for k, v in OPTION_VALUES.items()}), "ok", "h")])
    want = dict(STUB_DEFAULTS, **OPTION_VALUES)          # zrows and reserved are not the gateway's to set
    assert {k: stub.num(k) for k in want} == want


@pytest.mark.parametrize("one", sorted(OPTION_VALUES))
def test_an_absent_option_field_keeps_the_librarys_default(mexf, one):
    """The stub's admm_default_options differs from the library's in every field: a default hard-coded in the gateway shows."""
    b, stub = mexf
    b.run([(1, ("setup", _mex.make_problem(), {one: mx(float(OPTION_VALUES[one])), "segments_typo": mx(1.0)}), "ok", "h")])
    want = dict(STUB_DEFAULTS, **{one: OPTION_VALUES[one]})
    assert {k: stub.num(k) for k in want} == want


@pytest.mark.parametrize("form", ["absent", "empty", "empty-struct", "empty-fields"])
def test_no_options_give_admm_default_options(mexf, form):
    b, stub = mexf
    opts = {"absent": (), "empty": (EMPTY,), "empty-struct": ({},), "empty-fields": ({"rho": EMPTY, "flags": EMPTY},)}[form]
    b.run([(1, ("setup", _mex.make_problem()) + opts, "ok", "h")])
    assert {k: stub.num(k) for k in STUB_DEFAULTS} == STUB_DEFAULTS
    assert stub.calls("admm_default_options") == 1


def test_option_classes(mexf):
    """Integer-class and logical scalars are numbers too; a string, a vector or a fraction for an integer field is refused."""
    b, stub = mexf
    b.run([(1, ("setup", _mex.make_problem(), {"max_iter": mx(9, "int32"), "flags": mx(1, "logical"), "rho": mx(0.5, "single")}),
            "ok", "h")])
    assert (stub.num("max_iter"), stub.num("flags"), stub.num("rho")) == (9, 1, 0.5)
    for bad in ({"max_iter": mx(7.5)}, {"rho": "0.1"}, {"rho": mx(np.ones(2))}, {"flags": mx(1.0, complex=True)}):
        r = b.call(1, "setup", _mex.make_problem(), bad)
        assert (r.rc, r.error_id) == (1, "admm:input")
    assert stub.calls("admm_setup_fuel") == 1 and b.live() == 0


# ---- refusals -------------------------------------------------------------------------------------------------------------------
REFUSALS = _mex.refusals()


@pytest.mark.parametrize("label", sorted(REFUSALS))
def test_refusals(mexf, label):
    """admm:input, before the library is called, and nothing leaked.  The size checks mirror Problem.validate of the Python host:
    the C ABI takes raw pointers, so what the gateway lets through is read past its end."""
    b, stub = mexf
    steps = REFUSALS[label]
    b.run(steps[:-1])
    calls, live = stub.calls(), b.live()
    (r,) = b.run(steps[-1:])
    assert r.error_id == "admm:input" and r.error_text
    assert stub.calls() == calls, "the library was called"
    assert b.live() == live == 0 and r.outputs == []


def test_refused_shapes_are_those_the_python_host_refuses():
    """The catalogue's size refusals, as Problem arrays: Problem.validate refuses each one too."""
    import admm_library_amd as pkg
    g = np.random.default_rng(0)
    base = dict(N=N, A=g.random((n, n)), B=g.random((n, m)), Q=np.eye(n), R=np.eye(m), QN=np.eye(n), x0=g.random((batch, n)),
                lo=-np.ones(n + m), hi=np.ones(n + m))
    pkg.Problem(**base).validate()
    ltv = dict(base, A=g.random((N, n, n)), B=g.random((N, n, m)))
    pkg.Problem(**ltv).validate()
    for bad in (dict(ltv, B=base["B"]), dict(ltv, B=g.random((N - 1, n, m))), dict(base, A=g.random((n, n - 1))),
                dict(base, Q=np.eye(n - 1)), dict(base, R=np.eye(n)), dict(base, QN=np.ones((n, n - 1))),
                dict(base, hi=np.ones((N, n + m))), dict(base, x0=g.random((batch, n + 1))), dict(base, q=g.random((batch, L - 1))),
                dict(base, unorm=np.ones(N)), dict(base, fuel=np.ones(N))):
        with pytest.raises(ValueError):
            pkg.Problem(**bad).validate()


# ---- library errors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("command,sym,args,nlhs", [
    ("setup", "admm_setup_fuel", (), 1), ("solve", "admm_solve", (), 1), ("solve", "admm_get_rho", (), 1),
    ("solve", "admm_get_info", (), 1), ("get", "admm_get", (), 3), ("history", "admm_get_history", (), 1),
    ("path", "admm_get_path", (), 1), ("iterate", "admm_iterate", (mx(2.0),), 0), ("iterate", "admm_sync", (mx(2.0),), 0),
    ("update", "admm_update_problem", (_mex.make_problem(),), 0)])
def test_a_library_error_becomes_admm_library(mexf, command, sym, args, nlhs):
    b, stub = mexf
    if command != "setup":
        b.run([(1, ("setup", _mex.make_problem()), "ok", "h")])
    stub.fail(sym, 2, f"text of {sym}: (n, m) = (7, 5) is not compiled")
    r = b.call(nlhs, *(("setup", _mex.make_problem()) if command == "setup" else (command, Ref("h")) + args))
    assert (r.rc, r.error_id) == (1, "admm:library")
    assert f"text of {sym}: (n, m) = (7, 5) is not compiled" in r.error_text and "2" in r.error_text
    assert r.outputs == [] and r.warnings == [] and b.live() == 0
    stub.clear_faults()
    if command == "setup":                      # a failed setup remembers no handle: nothing to free at exit
        b.fire_at_exit()
        assert stub.calls("admm_free") == 0 and stub.handles() == []
    else:                                       # the handle survives the error
        assert b.call(1, "get", Ref("h")).rc == 0


# ---- warnings -------------------------------------------------------------------------------------------------------------------
def test_a_warning_is_emitted_once_by_the_call_that_can_set_it(mexf):
    """admm_last_warning() is cleared by setup, update_problem and solve only: forwarding it after any other call repeats it."""
    b, stub = mexf
    stub.warn("admm_setup_fuel", "setup fell back")
    r = b.call(1, "setup", _mex.make_problem(), save="h")
    assert r.warnings == [("admm:path", "setup fell back")]
    stub.clear_faults()
    seen = []
    for nlhs, args in ((0, ("iterate", Ref("h"), mx(2.0))), (3, ("get", Ref("h"))), (1, ("path", Ref("h"))),
                       (1, ("history", Ref("h"))), (0, ("iterate", Ref("h"), mx(1.0))), (0, ("iterate", Ref("h"), mx(1.0)))):
        r = b.call(nlhs, *args)
        assert r.rc == 0
        seen += r.warnings
    assert seen == []
    assert b.call(1, "solve", Ref("h")).warnings == []          # admm_solve cleared the text and left none


@pytest.mark.parametrize("command,sym", [("solve", "admm_solve"), ("update", "admm_update_problem")])
def test_solve_and_update_emit_their_warning_once(mexf, command, sym):
    b, stub = mexf
    b.run([(1, ("setup", _mex.make_problem()), "ok", "h")])
    stub.warn(sym, "rho refused")
    args = ("solve", Ref("h")) if command == "solve" else ("update", Ref("h"), _mex.make_problem())
    assert b.call(1 if command == "solve" else 0, *args).warnings == [("admm:path", "rho refused")]      # not three times
    assert b.call(3, "get", Ref("h")).warnings == [] and b.call(0, "iterate", Ref("h"), mx(1.0)).warnings == []


# ---- handle table ---------------------------------------------------------------------------------------------------------------
def test_handle_table(mexf):
    b, stub = mexf
    shapes = [dict(N=2), dict(N=3), dict(N=5), dict(batch=2)]
    for k, kw in enumerate(shapes):
        b.run([(1, ("setup", _mex.make_problem(**kw)), "ok", f"h{k}")])
    assert b.lib.msb_at_exit_registrations() == 1                  # registered once, by the first setup ever
    Ls = [b.call(1, "get", Ref(f"h{k}")).outputs[0].dims for k in range(4)]
    assert Ls == [(10, 5), (15, 5), (25, 5), (20, 2)]               # each handle kept its own sizes
    b.run([(0, ("free", Ref("h1")), "ok", None), (0, ("free", Ref("h1")), "admm:input", None)])      # a double free is refused
    assert stub.frees() == [0, 1, 0, 0]
    b.run([(1, ("setup", _mex.make_problem(N=6)), "ok", "h4")])    # reuses the freed slot: the others are untouched
    assert [b.call(1, "get", Ref(f"h{k}")).outputs[0].dims for k in (0, 2, 3, 4)] == [(10, 5), (25, 5), (20, 2), (30, 5)]
    assert b.fire_at_exit() == 1
    assert stub.frees() == [1, 1, 1, 1, 1]                          # every live handle exactly once
    b.fire_at_exit()
    assert stub.frees() == [1, 1, 1, 1, 1]
    b.run([(1, ("get", Ref("h0")), "admm:input", None)])            # the table is empty afterwards
    assert b.lib.msb_at_exit_registrations() == 1


# ---- outputs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlhs", [0, 1, 2, 3])
def test_get_passes_null_for_what_is_not_asked(mexf, nlhs):
    b, stub = mexf
    b.run([(1, ("setup", _mex.make_problem()), "ok", "h")])
    r = b.call(nlhs, "get", Ref("h"))
    k = max(nlhs, 1)
    assert len(r.outputs) == k and r.orphans == 0
    for o, name, base in zip(r.outputs, ("get_w", "get_z", "get_y"), (1e6, 2e6, 3e6)):
        assert o.cls == _mex.CLASS["double"] and o.dims == (L, batch) and stub.ptr(name) == o.ptr
        assert np.array_equal(o.data, base + np.arange(L * batch))
    for name in ("get_w", "get_z", "get_y")[k:]:
        assert stub.ptr(name) == 0


def test_solve_output(mexf):
    b, stub = mexf
    b.run([(1, ("setup", _mex.make_problem()), "ok", "h")])
    z0, y0 = mx(np.arange(L * batch, dtype=float).reshape(L, batch)), mx(np.ones((L, batch)))
    r = b.call(1, "solve", Ref("h"), z0, y0)
    assert (stub.ptr("z0"), stub.ptr("y0")) == (r.ptrs["arg2"], r.ptrs["arg3"])
    assert (stub.num("sum_z0"), stub.num("sum_y0")) == (z0.data.sum(), L * batch)
    info = r.outputs[0]
    assert info.dims == (1, 1) and list(info.data) == ["iters_run", "n_converged", "max_r", "max_s", "solve_ms", "iters", "status",
                                                       "r", "s", "rho", "rho_updates", "mixed_iters", "rho_per_qp"]
    scalars = dict(iters_run=41, n_converged=42, max_r=43.5, max_s=44.5, solve_ms=45.5, rho=46.5, rho_updates=47, mixed_iters=48)
    for k, v in scalars.items():
        f = info.data[k]
        assert (f.cls, f.dims, f.data[0]) == (_mex.CLASS["double"], (1, 1), v), k
    for k, cls, base in (("iters", "int32", 600), ("status", "int32", 700), ("r", "double", 800), ("s", "double", 900),
                         ("rho_per_qp", "double", 500)):
        f = info.data[k]
        assert (f.cls, f.dims) == (_mex.CLASS[cls], (batch, 1)), k
        assert np.array_equal(f.data, base + np.arange(batch)), k
    r = b.call(1, "solve", Ref("h"), EMPTY, y0)                       # [] = continue from the handle's state
    assert stub.ptr("z0") == 0 and stub.ptr("y0") == r.ptrs["arg3"]
    r = b.call(1, "solve", Ref("h"))
    assert stub.ptr("z0") == 0 and stub.ptr("y0") == 0
    # batch = 1: the per-QP fields are 1 x 1
    b.run([(1, ("setup", _mex.make_problem(batch=1)), "ok", "h1")])
    info = b.call(1, "solve", Ref("h1")).outputs[0]
    assert all(info.data[k].dims == (1, 1) for k in ("iters", "status", "r", "s", "rho_per_qp"))


@pytest.mark.parametrize("k", [0, 1, 7])
def test_history_output(mexf, k):
    b, stub = mexf
    b.run([(1, ("setup", _mex.make_problem()), "ok", "h")])
    stub.set_history(k)
    h = b.call(1, "history", Ref("h")).outputs[0]
    assert list(h.data) == ["iteration", "n_converged", "max_r", "max_s", "rho"]
    assert stub.calls("admm_get_history") == 2 and stub.num("history_capacity") == k
    for name, cls, base in (("iteration", "int32", 10), ("n_converged", "int32", 20), ("max_r", "double", 30), ("max_s", "double", 40),
                            ("rho", "double", 50)):
        f = h.data[name]
        assert (f.cls, f.dims) == (_mex.CLASS[cls], (k, 1)), name
        assert np.array_equal(f.data, base + np.arange(k)), name


def test_path_output(mexf):
    b, stub = mexf
    b.run([(1, ("setup", _mex.make_problem()), "ok", "h")])
    p = b.call(1, "path", Ref("h")).outputs[0]
    want = dict(alternating=1, alt_requested=2, mfma=3, xfree=4, segments=5, auto_segments=6, scan_form=7, per_instance=8,
                alt_check=9.5, alt_gate=10.5, scan_growth=11.5)
    assert list(p.data) == list(want) and len(want) == 11
    for k, v in want.items():
        assert (p.data[k].cls, p.data[k].dims, p.data[k].data[0]) == (_mex.CLASS["double"], (1, 1), v)


def test_iterate_passes_its_count(mexf):
    b, stub = mexf
    b.run([(1, ("setup", _mex.make_problem()), "ok", "h"), (0, ("iterate", Ref("h"), mx(17, "int32")), "ok", None)])
    assert stub.num("iterate_iters") == 17 and stub.calls("admm_sync") == 1 and stub.ptr("handle") == stub.handles()[0]


# ---- the stand-in's own rules -----------------------------------------------------------------------------------------------------
def test_stand_in_restates_matlabs_array_rules(mexf):
    """Trailing singletons are dropped, at least two dimensions remain, and each output reports them so."""
    b, _ = mexf
    lib = b.lib
    for given, stored in (((3, 3, 4, 1), (3, 3, 4)), ((3, 3, 1), (3, 3)), ((3, 3, 1, 1), (3, 3)), ((5, 1), (5, 1)), ((1, 1, 1), (1, 1)),
                          ((1, 5, 1, 2), (1, 5, 1, 2)), ((0, 0), (0, 0)), ((3, 0, 1), (3, 0))):
        ptrs = {}
        a = b._make(_mex.MX(6, given, np.zeros(int(np.prod(given)))), ptrs, "a")
        assert tuple(lib.msb_dim(a, k) for k in range(lib.msb_ndim(a))) == stored
        assert (ptrs["a"] == 0) == (int(np.prod(given)) == 0)          # no data: no pointer
        lib.msb_destroy(a)


# ---- the .m files, as text --------------------------------------------------------------------------------------------------------
MATLAB = os.path.join(_mex.ROOT, "matlab")
GATEWAY_TEXT = open(_mex.GATEWAY).read()


def m_files():
    return sorted(f for f in os.listdir(MATLAB) if f.endswith(".m"))


def test_m_files_call_commands_the_gateway_implements():
    commands = set(re.findall(r'const char\* commands\[\] = \{([^}]*)\}', GATEWAY_TEXT)[0].replace('"', "").replace(" ", "").split(","))
    assert commands == set(re.findall(r'!std::strcmp\(cmd, "(\w+)"\)', GATEWAY_TEXT))        # each listed command has a branch
    used = set()
    for f in m_files():
        used |= set(re.findall(r"admm_mex\('(\w+)'", open(os.path.join(MATLAB, f)).read()))
    assert {"setup", "solve", "get", "free", "update"} <= used <= commands
    # the header comment of the gateway names only files that exist
    for name in re.findall(r"\b(admm_\w+\.m)\b", GATEWAY_TEXT):
        assert os.path.exists(os.path.join(MATLAB, name)), name


def default_options_m():
    text = open(os.path.join(MATLAB, "admm_default_options.m")).read()
    body = re.search(r"opts = struct\((.*?)\);", text, re.S).group(1).replace("...", " ")
    return {k: float(v) for k, v in re.findall(r"'(\w+)'\s*,\s*([-+0-9.eE]+)", body)}


def test_default_options_m_names_the_fields_the_gateway_reads():
    read = set(re.findall(r'(?:scalar_or|integer_or)\(O, "(\w+)"', GATEWAY_TEXT))
    assert set(default_options_m()) == read == set(OPTION_VALUES)


def test_default_options_m_equals_the_librarys_defaults(lib):
    from admm_library_amd import _abi
    o = _abi.COptions()
    lib.admm_default_options(o)
    assert default_options_m() == {k: float(getattr(o, k)) for k in OPTION_VALUES}


def test_admm_solve_help_lists_every_info_field():
    names = re.search(r'const char\* names\[\] = \{("iters_run".*?)\};', GATEWAY_TEXT, re.S).group(1)
    fields = re.findall(r'"(\w+)"', names)
    assert len(fields) == 13
    help_text = "\n".join(l for l in open(os.path.join(MATLAB, "admm_solve.m")).read().splitlines() if l.startswith("%"))
    for f in fields:
        assert re.search(rf"\b{f}\b", help_text), f


# ---- one sanitizer run, of a stand-alone program ----------------------------------------------------------------------------------
def replay_script():
    s = _mex.Script()
    for kw in _mex.ACCEPTED:
        s.steps(_mex.setup_steps(kw))
        s.steps(_mex.setup_steps(kw, {"rho": mx(0.5), "max_iter": mx(9, "int32")})[:2])
        s.reset()
    for label, steps in REFUSALS.items():          # (the catalogue's order: the short B that started it comes first)
        s.steps(steps)
        s.reset()
    for sym in ("admm_setup_fuel", "admm_solve", "admm_get_info", "admm_get", "admm_get_history", "admm_update_problem"):
        s.steps([(1, ("setup", _mex.make_problem()), "ok", "h")] if sym != "admm_setup_fuel" else [])
        s.fail(sym, 2, "refused")
        s.steps([_library_error_step(sym)])
        s.reset()
    return s.text()


def _library_error_step(sym):
    return {"admm_setup_fuel": (1, ("setup", _mex.make_problem()), "admm:library", None),
            "admm_solve": (1, ("solve", Ref("h")), "admm:library", None),
            "admm_get_info": (1, ("solve", Ref("h")), "admm:library", None),
            "admm_get": (3, ("get", Ref("h")), "admm:library", None),
            "admm_get_history": (1, ("history", Ref("h")), "admm:library", None),
            "admm_update_problem": (0, ("update", Ref("h"), _mex.make_problem()), "admm:library", None)}[sym]


def test_replay_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """Every accepted form (every command on it), every refusal and the library errors, replayed by a stand-alone program built
    with -fsanitize=address,undefined: each array is its own allocation, so a read or write past an input or output traps; leak
    detection is on.  (The code loaded into this process is the plain build.)"""
    exe, script = str(tmp_path / "mex_replay"), tmp_path / "script.txt"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-Wall", "-Wextra", "-Werror", "-I", SHIM, "-I", os.path.join(_mex.ROOT, "include"), _mex.GATEWAY,
                    os.path.join(SHIM, "mex_standin.cpp"), os.path.join(SHIM, "mex_bridge.cpp"), STUB,
                    os.path.join(SHIM, "mex_replay.cpp"), "-o", exe], check=True)
    script.write_text(replay_script())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, str(script)], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-6000:]
    assert re.search(r"mex_replay: \d{3,} calls replayed, 0 ended otherwise", out.stdout), out.stdout
