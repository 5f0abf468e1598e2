"""One half-space per stage without a GPU: the reference the GPU tests compare against (tests/_halfspace_ref.py) is
the oracle's loop and its prox is the projection; csrc/admm_prox.hpp's halfspace_project, compiled on the host, gives the
specified bits; Problem.validate and the C set-up refuse what the interface says they refuse, before a device is looked for; and
the cases tests/test_gpu_halfspace.py runs have, in the reference alone, stages of every kind in every QP."""
import ctypes as C
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import admm_library_amd as pkg
import _fuel_ref as fr
import _halfspace_ref as hr
import _readout_cases as rc
import admm_ref
from admm_library_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 2
INF = np.inf
SYMBOLS = ("admm_setup_halfspace", "admm_set_halfspace", "admm_set_halfspace_device", "admm_get_halfspace",
           "admm_get_halfspace_report", "admm_get_halfspace_report_device")
RHO = 0.3


# ---- the cases the GPU tests share (tests/test_gpu_halfspace.py imports them) ----

def random_planes(p, nh, per_qp, seed=11, free=4, pin=False):
    """Planes for a random_ltv problem: every `free`-th stage (from stage 2) has a = 0; elsewhere a is standard normal with a
    zero entry here and there (never all), b = 0.15 |a| times a standard normal -- planes that cut close to the origin, so that
    about half of them bind.  pin: the plane of stage 0 lies 50 |a| away (never reached: t = 0) and that of stage 1 at -5 |a|
    (out of the dynamics' reach within a step: always binding), so that every QP has a stage of either kind whatever the rest
    does.  The box of the rows under a plane is opened; returns the problem with hs_a / hs_b."""
    rng = np.random.default_rng(seed)
    cnt = p.batch if per_qp else 1
    a = rng.standard_normal((cnt, p.N, nh))
    if nh > 1:
        zero = rng.random((cnt, p.N, nh)) < 0.2
        zero[:, :, 0] = False
        a[zero] = 0.0
    na = np.sqrt(np.sum(a * a, axis=2))
    b = 0.15 * na * rng.standard_normal((cnt, p.N))
    if pin:
        b[:, 0] = 50.0 * na[:, 0]
        b[:, 1] = -5.0 * na[:, 1]
    off = np.zeros(p.N, bool)
    off[2::free] = True
    a[:, off] = 0.0
    b[:, off] = 0.0
    lo, hi = np.array(np.broadcast_to(p.lo, (p.N, p.nb))), np.array(np.broadcast_to(p.hi, (p.N, p.nb)))
    lo[~off, p.m:p.m + nh] = -INF
    hi[~off, p.m:p.m + nh] = INF
    q = dataclasses.replace(p, lo=lo, hi=hi, hs_a=a if per_qp else a[0], hs_b=b if per_qp else b[0])
    q.validate()
    return q


# (n, m, nh, N, batch, per_qp, kind, alpha, residual_every, zrows): every shape, batch, form, alpha, kind and residual spacing the
# walk distinguishes appears; zrows = L is a single chunk, a smaller number several, the last one shorter where it does not divide L
ITER_CASES = [
    (6, 3, 3, 9, 3, True, "box", 1.0, 1, 18),
    (6, 3, 3, 9, 70, False, "box", 1.6, 3, 18),
    (6, 3, 1, 8, 514, True, "thrust", 1.0, 1, 27),
    (6, 3, 1, 8, 1, False, "fuel", 1.6, 1, 72),
    (4, 2, 4, 9, 70, True, "fuel", 1.6, 3, 12),
    (4, 2, 4, 9, 3, False, "thrust", 1.0, 1, 54),
    (2, 1, 1, 12, 514, False, "box", 1.0, 3, 9),
    (2, 1, 1, 12, 1, True, "box", 1.6, 1, 36),
    (12, 6, 3, 8, 70, True, "thrust", 1.0, 3, 36),
    (12, 6, 3, 8, 3, False, "box", 1.6, 1, 144),
]
ITER_IDS = ["%dx%d_nh%d_N%d_b%d_%s_%s_a%g_e%d_z%d" % (c[0], c[1], c[2], c[3], c[4], "perqp" if c[5] else "shared", c[6], c[7], c[8], c[9])
            for c in ITER_CASES]
ITER_STEPS = (1, 2, 9, 30)


def iter_case(n, m, nh, N, batch, per_qp, kind, alpha, every, zrows):
    """(problem, options) of a row of ITER_CASES."""
    p = pkg.random_ltv(N=N, n=n, m=m, batch=batch, seed=5000 + 16 * n + m, thrust_norm=kind != "box")
    if kind == "fuel":
        p = rc.stage_fuel(p)
    p = random_planes(p, nh, per_qp, seed=100 * n + nh, pin=True)
    kw = dict(rho=RHO, alpha=alpha)
    if zrows:
        kw["zrows"] = zrows
    return p, kw


def ref_iterates(p, kw, k, every, **more):
    return hr.solve(p, rho=kw["rho"], alpha=kw.get("alpha", 1.0), max_iter=k, check_interval=max(every, 1), eps_abs=0, eps_rel=0,
                    stop=False, **more)


SOLVE_OPTS = dict(rho=0.5, eps_abs=1e-7, eps_rel=1e-7, max_iter=4000, check_interval=10, adapt_interval=50, adapt_max=8)


def solve_problem():
    return pkg.cw_keepout(N=40, batch=6)


# ---- interface ----

def test_header_announces_the_symbols_and_keeps_the_abi_version():
    h = open(os.path.join(ROOT, "include", "admm_hip.h")).read()
    assert re.search(r"^#define ADMM_HIP_HAS_HALFSPACE 1$", h, re.M)
    assert re.search(r"^#define ADMM_HIP_ABI_VERSION 9$", h, re.M)
    for name in SYMBOLS:
        assert re.search(r"^int " + name + r"\(", h, re.M), name


def test_nm_lists_the_symbols(built):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.library_path()], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in SYMBOLS:
        assert name in names, name
    from admm_library_amd import solver
    assert set(SYMBOLS) <= set(solver._SIGNATURES)


def test_setup_halfspace_validates_before_the_device(lib):
    """Every refusal of admm_setup_halfspace comes back with its own status -- never ADMM_ERR_NO_DEVICE, which is what any call that
    got as far as looking for a GPU returns on a machine without one -- and leaves no handle."""
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.admm_abi_version() == 9
    out = np.zeros(8)
    cnt = np.zeros(4, np.int32)
    assert lib.admm_set_halfspace(None, _abi.dptr(out), _abi.dptr(out)) == INVALID and b"NULL" in lib.admm_last_error()
    assert lib.admm_set_halfspace_device(None, _abi.dptr(out), _abi.dptr(out), None) == INVALID
    assert lib.admm_get_halfspace(None, _abi.dptr(out), _abi.dptr(out)) == INVALID and b"NULL" in lib.admm_last_error()
    assert lib.admm_get_halfspace_report(None, _abi.dptr(out), None, None) == INVALID and b"NULL" in lib.admm_last_error()
    assert lib.admm_get_halfspace_report_device(None, _abi.dptr(out), _abi.iptr(cnt), None, None) == INVALID
    h = C.c_void_p()
    p = random_planes(pkg.random_ltv(N=6, n=4, m=2, batch=5, seed=2), 2, True)
    cp, keep = _abi.marshal_problem(p)
    a, b, nh, per_qp = _abi.marshal_halfspace(p)
    assert (nh, per_qp) == (2, True) and a.shape == (5, 6, 2) and b.shape == (5, 6)

    def setup(c, a_, b_, nh_=nh, per=1, opt=None, fuel=None):
        rc_ = lib.admm_setup_halfspace(C.byref(h), C.byref(c), None if opt is None else C.byref(opt), _abi.dptr(fuel), _abi.dptr(a_),
                                       _abi.dptr(b_), nh_, per)
        assert not h.value
        return rc_, lib.admm_last_error().decode()

    assert lib.admm_setup_halfspace(C.byref(h), None, None, None, _abi.dptr(a), _abi.dptr(b), nh, 1) == INVALID and not h.value
    for args in ((None, b), (a, None)):
        rc_, msg = setup(cp, *args)
        assert rc_ == INVALID and "must not be NULL" in msg
    for bad_nh in (0, -1, 5):
        rc_, msg = setup(cp, a, b, nh_=bad_nh)
        assert rc_ == INVALID and "nh" in msg, (bad_nh, msg)
    for bad in (np.nan, INF, -INF):
        for which in (0, 1):
            aa, bb = a.copy(), b.copy()
            (aa if which == 0 else bb).reshape(-1)[7] = bad
            rc_, msg = setup(cp, aa, bb)
            assert rc_ == INVALID and "non-finite" in msg, (bad, which, msg)
    aa = a.copy()
    aa[3, 1] = (1e-170, 0.0)                    # a'a underflows: the projection would divide by it
    rc_, msg = setup(cp, aa, b)
    assert rc_ == INVALID and "normal number" in msg
    # a closed box under a plane: of one QP only, and in the shared form
    closed = dataclasses.replace(p, lo=p.lo.copy())
    closed.lo[1, p.m + 1] = -2.0
    cc, keep_c = _abi.marshal_problem(dataclasses.replace(closed, hs_a=None, hs_b=None))
    rc_, msg = setup(cc, a, b)
    assert rc_ == INVALID and "unbounded" in msg and "stage 1" in msg
    one = np.zeros_like(a)
    one[4, 1] = a[4, 1]
    rc_, msg = setup(cc, one, b)
    assert rc_ == INVALID and "unbounded" in msg
    rc_, msg = setup(cc, np.ascontiguousarray(a[0]), np.ascontiguousarray(b[0]), per=0)
    assert rc_ == INVALID and "unbounded" in msg
    # ... and with stage_bounds = 0 the rule applies to the one block
    lti = rc.lti(pkg.random_ltv(N=6, n=4, m=2, batch=5, seed=2))
    cl, keep_l = _abi.marshal_problem(lti)
    rc_, msg = setup(cl, a, b)
    assert rc_ == INVALID and "unbounded" in msg
    inst = pkg.random_instances(N=6, n=4, m=2, batch=5, seed=2)
    ci, keep_i = _abi.marshal_problem(inst)
    rc_, msg = setup(ci, a, b)
    assert rc_ == UNSUPPORTED and "batch-shared" in msg
    for mode in (_abi.PRECISION_MIXED, _abi.PRECISION_FP64_MFMA):
        opt = pkg.Options(rho=0.3, precision_mode=mode).to_c()
        rc_, msg = setup(cp, a, b, opt=opt)
        assert rc_ == UNSUPPORTED and "precision_mode" in msg and "half-spaces" in msg
    # a valid request gets as far as the device
    rc_, msg = setup(cp, a, b)
    assert rc_ == 3 or pkg.device_count() > 0, (rc_, msg)
    if h.value:
        lib.admm_free(h)


def test_problem_validate_checks_the_planes():
    base = pkg.random_ltv(N=6, n=4, m=2, batch=5, seed=2)
    for nh in (1, 4):
        for per_qp in (False, True):
            random_planes(base, nh, per_qp).validate()
    p = random_planes(base, 2, True)
    with pytest.raises(ValueError, match="together"):
        dataclasses.replace(p, hs_b=None).validate()
    for field, bad in (("hs_a", np.nan), ("hs_b", INF)):
        arr = getattr(p, field).copy()
        arr.reshape(-1)[3] = bad
        with pytest.raises(ValueError, match="finite"):
            dataclasses.replace(p, **{field: arr}).validate()
    with pytest.raises(ValueError, match="hs_a / hs_b must be"):
        dataclasses.replace(p, hs_b=p.hs_b[:, :5]).validate()
    with pytest.raises(ValueError, match="hs_a / hs_b must be"):
        dataclasses.replace(p, hs_a=p.hs_a[:4], hs_b=p.hs_b[:4]).validate()
    with pytest.raises(ValueError, match="nh"):
        dataclasses.replace(p, hs_a=np.zeros((5, 6, 5))).validate()
    closed = dataclasses.replace(p, hi=p.hi.copy())
    closed.hi[0, p.m] = 1.0
    with pytest.raises(ValueError, match="unbounded"):
        closed.validate()
    a = p.hs_a.copy()
    a[:, 0] = 0.0                                # no plane at stage 0 for any QP: its box may be closed
    dataclasses.replace(closed, hs_a=a).validate()
    tiny = p.hs_a.copy()
    tiny[2, 1] = (1e-170, 0.0)
    with pytest.raises(ValueError, match="normal"):
        dataclasses.replace(p, hs_a=tiny).validate()
    with pytest.raises(ValueError, match="soft or consensus"):
        dataclasses.replace(p, soft=np.full((6, 6), INF)).validate()
    with pytest.raises(ValueError, match="soft or consensus"):
        dataclasses.replace(p, consensus=5).validate()
    inst = pkg.random_instances(N=6, n=4, m=2, batch=5, seed=2)
    with pytest.raises(ValueError, match="batch-shared"):
        dataclasses.replace(inst, hs_a=p.hs_a, hs_b=p.hs_b).validate()
    with pytest.raises(ValueError, match="device-memory"):
        dataclasses.replace(pkg.DeviceProblem(**{f.name: getattr(base, f.name) for f in dataclasses.fields(pkg.DeviceProblem)}),
                            hs_a=p.hs_a, hs_b=p.hs_b).validate()
    # the fields sit before fuel, which stays last
    names = [f.name for f in dataclasses.fields(pkg.Problem)]
    assert names[-3:] == ["hs_a", "hs_b", "fuel"]


def test_the_generators():
    X = np.random.default_rng(0).standard_normal((3, 7, 3))
    X[1, 2] = 0.0
    c = np.array([0.1, -0.2, 0.3])
    a, b = pkg.keepout_halfspaces(X, 0.4, c)
    assert a.shape == (3, 7, 3) and b.shape == (3, 7)
    nhat = (X - c) / np.linalg.norm(X - c, axis=2, keepdims=True)
    assert np.allclose(a, -nhat) and np.allclose(b, -(0.4 + nhat @ c))
    # a point at distance r from the centre along n satisfies a.x <= b iff r >= R
    for r, ok in ((0.5, True), (0.3, False)):
        pt = c + r * nhat
        assert np.all((np.sum(a * pt, axis=2) <= b + 1e-15) == ok)
    a0, b0 = pkg.keepout_halfspaces(X, 0.4)
    assert not a0[1, 2].any() and b0[1, 2] == 0.0                 # no direction at the centre: no plane
    p = solve_problem()
    p.validate()
    assert p.hs_a.shape == (6, 40, 3) and p.hs_b.shape == (6, 40) and not p.hs_a[:, 35:].any() and p.hs_a[:, :35].any(axis=2).all()
    R = 0.5 * np.linalg.norm(p.x0[:, :3], axis=1).min()
    assert np.allclose(p.hs_b[:, :35], -R) and np.allclose(np.linalg.norm(p.hs_a[:, :35], axis=2), 1.0)
    pf = pkg.cw_keepout(N=20, batch=2, radius=0.2, free_tail=3, fuel=0.05)
    pf.validate()
    assert pf.unorm is not None and pf.fuel == 0.05 and np.allclose(pf.hs_b[:, :17], -0.2) and not pf.hs_a[:, 17:].any()
    assert pkg.cw_keepout(N=20, batch=2, thrust_norm=True).unorm is not None


def test_the_unit_is_built_checked_and_does_not_spill(tmp_path):
    """csrc/admm_halfspace.hip compiled on its own with the library's flags and the compiler's resource report: exactly the sixteen
    forms of zdual_halfspace_kernel and the two read-outs carry `halfspace` in their names, and none uses scratch memory or spills
    a VGPR (DESIGN.md §2.14 records the registers this prints)."""
    import __graft_entry__ as ge
    assert "admm_halfspace.hip" in ge.RUNTIME_UNITS and "admm_halfspace_kernels.hpp" in ge.HEADERS and "admm_halfspace.hpp" in ge.HEADERS
    assert "admm_halfspace.hip" in ge.NO_SCRATCH_UNITS            # the build itself refuses scratch in this unit
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-Rpass-analysis=kernel-resource-usage"] + ge.HIPCC_FLAGS +
                       ["-c", os.path.join(ge.CSRC, "admm_halfspace.hip"), "-o", str(tmp_path / "admm_halfspace.o")],
                       cwd=ge.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = ge.parse_resource_usage(r.stderr)
    mine = [x for x in rows if "halfspace" in x["name"]]
    for x in mine:
        print(f'{x["name"]}: {x["vgpr"]} VGPRs, {x["agpr"]} AGPRs, {x["sgpr"]} SGPRs, scratch {x["scratch"]} B, occupancy {x["occupancy"]}')
    forms = sorted(x["name"].split("<")[1] for x in mine if "zdual_halfspace_kernel" in x["name"])
    tf = ("false", "true")
    assert forms == sorted(f"{a}, {b}, {c}, {d}>" for a in tf for b in tf for c in tf for d in tf)
    assert sorted(x["name"].split("::")[-1] for x in mine if "zdual_halfspace_kernel" not in x["name"]) == \
        ["halfspace_report_kernel", "halfspace_scan_kernel"]
    assert all(x["scratch"] == 0 and x["vgpr_spill"] == 0 for x in mine), mine
    assert all(x["scratch"] == 0 for x in rows), [x["name"] for x in rows if x["scratch"]]


# ---- the prox ----

@pytest.fixture(scope="module")
def prox_host(tmp_path_factory):
    """tests/halfspace_prox.cpp + csrc/admm_prox.hpp as a shared object (host compiler, no contraction): prox(a, b, v) ->
    (z, y, active) for stacks of stages, a and v (count, nh), b (count,)."""
    return build_prox_host(tmp_path_factory.mktemp("halfspace"))


def build_prox_host(tmp):
    import __graft_entry__ as ge
    assert "admm_prox.hpp" in ge.HEADERS
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    so = tmp / "halfspace_prox.so"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", ge.CSRC,
                    os.path.join(os.path.dirname(os.path.abspath(__file__)), "halfspace_prox.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    dp = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
    lib.halfspace_stages.argtypes = [C.c_int, C.c_int] + [dp] * 5 + [np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")]
    lib.halfspace_stages.restype = None

    def prox(a, b, v):
        a, b, v = (np.ascontiguousarray(x, np.float64) for x in (a, b, v))
        z, y, act = np.empty_like(v), np.empty_like(v), np.empty(a.shape[0], np.int32)
        lib.halfspace_stages(a.shape[0], a.shape[1], a, b, v, z, y, act)
        return z, y, act
    return prox


def up(x):
    return np.nextafter(x, INF)


def dn(x):
    return np.nextafter(x, -INF)


def edge_stages(nh, rng):
    """Stages (a, b, v) on the edges of the prox: d = 0 exactly, d the smallest positive value and its negative, d one rounding
    either side of a plane through a generic point, a with zero entries, a = 0 with b of either sign."""
    rows = []
    for trial in range(6):
        a = rng.standard_normal(nh)
        if nh > 1 and trial % 2:
            a[rng.integers(1, nh)] = 0.0
        v = rng.standard_normal(nh)
        d0 = 0.0
        for ai, vi in zip(a, v):
            d0 = hr._fma(ai, vi, d0)
        # b = a.v as the chain computes it from -b: d = fma(.., -b) ends at exactly 0 when the chain without b is exact in b
        a2 = np.round(a * 8) / 8
        v2 = np.round(v * 8) / 8
        b2 = float(np.dot(a2, v2))                                  # exact: multiples of 1/64
        rows += [(a2, b2, v2), (a2, b2 - 5e-324, v2), (a2, b2 + 5e-324, v2), (a2, dn(b2), v2), (a2, up(b2), v2)]
        rows += [(a, d0, v), (a, up(d0), v), (a, dn(d0), v), (a, d0 - 1.0, v), (a, d0 + 1.0, v)]
    z = np.zeros(nh)
    rows += [(z, 1.0, rng.standard_normal(nh)), (z, -1.0, rng.standard_normal(nh)), (z, 0.0, rng.standard_normal(nh))]
    a1 = np.zeros(nh)
    a1[0] = 1.0                                                     # d = v_0 - b with v_0 = 5e-324, b = 0: the smallest positive d
    v1 = np.zeros(nh)
    v1[0] = 5e-324
    rows += [(a1, 0.0, v1), (a1, 0.0, -v1), (a1, 0.0, np.zeros(nh))]
    return [np.array(x) for x in zip(*rows)]


@pytest.mark.parametrize("nh", [1, 2, 3, 6])
def test_the_header_prox_equals_the_exact_chain(prox_host, nh):
    """halfspace_project of csrc/admm_prox.hpp against tests/_halfspace_ref.project -- every fma in exact rationals, rounded once --
    bit for bit, on random stages and on the edges."""
    rng = np.random.default_rng(40 + nh)
    a, b, v = edge_stages(nh, rng)
    ar = rng.standard_normal((200, nh))
    ar[rng.random((200, nh)) < 0.15] = 0.0
    a, b, v = np.vstack([a, ar]), np.concatenate([b, rng.standard_normal(200)]), np.vstack([v, 2.0 * rng.standard_normal((200, nh))])
    z, y, act = prox_host(a, b, v)
    kinds = set()
    for s in range(a.shape[0]):
        want = hr.project(a[s], b[s], v[s])
        if want is None:
            assert act[s] == 0 and not a[s].any() and np.array_equal(z[s], v[s]) and not y[s].any()
            kinds.add("off")
            continue
        assert act[s] == 1
        assert np.array_equal(z[s], want[0]) and np.array_equal(y[s], want[1]), (s, a[s], b[s], v[s], z[s], want[0])
        kinds.add("moved" if y[s].any() else "kept")
        if not y[s].any():
            assert np.array_equal(z[s], v[s])
    assert kinds == {"off", "moved", "kept"}
    # d = 0 exactly and the smallest positive d, by construction
    a2, b2, v2 = a[0], b[0], v[0]
    assert float(np.dot(a2, v2)) - b2 == 0.0 and not y[0].any()
    zs, ys, _ = prox_host(np.eye(1, nh), np.zeros(1), 5e-324 * np.eye(1, nh))
    assert zs[0, 0] == 0.0 and ys[0, 0] == 5e-324                   # t = 5e-324 / 1: the row is moved onto the plane


def test_the_numpy_prox_is_the_exact_chain_to_rounding():
    """tests/_halfspace_ref.prox (NumPy sums instead of fma chains) against project on a whole iterate: a few ulps."""
    p = iter_case(*ITER_CASES[0])[0]
    rng = np.random.default_rng(3)
    v = rng.standard_normal((p.batch, p.L))
    lo, hi = admm_ref.expand_bounds(p.lo, p.hi, p.N, p.nb)
    A, Bv = hr.planes(p)
    zn = hr.prox(v, lo, hi, admm_ref.expand_unorm(p.unorm, p.N), np.zeros(p.N), p.m, A, Bv).reshape(p.batch, p.N, p.nb)
    box = fr.prox(v, lo, hi, admm_ref.expand_unorm(p.unorm, p.N), np.zeros(p.N), p.m).reshape(p.batch, p.N, p.nb)
    vb = v.reshape(p.batch, p.N, p.nb)
    nh = A.shape[2]
    for b in range(p.batch):
        for k in range(p.N):
            want = hr.project(A[b, k], Bv[b, k], vb[b, k, p.m:p.m + nh])
            got = zn[b, k, p.m:p.m + nh]
            if want is None:
                assert np.array_equal(got, box[b, k, p.m:p.m + nh])
            else:
                assert np.abs(got - want[0]).max() <= 8 * np.finfo(float).eps * max(1.0, np.abs(vb[b, k]).max())
            other = np.r_[0:p.m, p.m + nh:p.nb]
            assert np.array_equal(zn[b, k, other], box[b, k, other])


@pytest.mark.parametrize("nh", [1, 3, 6])
def test_prox_is_the_euclidean_projection(prox_host, nh):
    """z = P(v) onto C = {x: a.x <= b} iff z in C and (v - z).(x - z) <= 0 for every x in C (the variational inequality)."""
    rng = np.random.default_rng(7 + nh)
    a = rng.standard_normal((300, nh))
    b = rng.standard_normal(300)
    v = 2.0 * rng.standard_normal((300, nh))
    z, y, act = prox_host(a, b, v)
    assert act.all()
    na = np.linalg.norm(a, axis=1)
    assert np.all(np.sum(a * z, axis=1) - b <= 4e-16 * (np.abs(b) + na * np.linalg.norm(v, axis=1)))
    inside = np.sum(a * v, axis=1) <= b
    assert np.array_equal(z[inside], v[inside]) and inside.any() and (~inside).any()
    for trial in range(20):
        x = 3.0 * rng.standard_normal((300, nh))
        x = x - np.maximum(np.sum(a * x, axis=1) - b, 0.0)[:, None] * a / (na * na)[:, None]       # into C
        x = x - 1e-12 * a
        assert np.all(np.sum(a * x, axis=1) <= b)
        assert np.all(np.sum(y * (x - z), axis=1) <= 1e-13 * (1.0 + np.linalg.norm(y, axis=1) * np.linalg.norm(x - z, axis=1)))


# ---- the reference loop ----

@pytest.mark.parametrize("kind", ["box", "thrust"])
def test_zero_planes_are_the_oracle_bit_for_bit(kind):
    p = pkg.random_ltv(N=9, n=6, m=3, batch=5, seed=77, thrust_norm=kind == "thrust")
    ph = dataclasses.replace(p, hs_a=np.zeros((5, 9, 3)), hs_b=np.random.default_rng(1).standard_normal((5, 9)))
    ph.validate()
    for alpha in (1.0, 1.6):
        a = hr.solve(ph, rho=RHO, alpha=alpha, max_iter=40, check_interval=10, adapt_interval=10, stop=False)
        b = admm_ref.solve(p.A, p.B, p.Q, p.R, p.QN, p.x0, p.lo, p.hi, p.N, q=p.q, rho=RHO, alpha=alpha, max_iter=40, check_interval=10,
                           adapt_interval=10, stop=False, unorm=p.unorm)
        for name in ("w", "z", "y", "r", "s"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), (alpha, name)
        assert a.rho == b.rho and a.rho_updates == b.rho_updates


def dense_with_planes(p, b):
    """(P, q, G, rhs, Ah, bh) of QP b of p: admm_ref.dense_qp and the inequalities Ah w <= bh of the stages with a plane."""
    P, q, G, rhs = admm_ref.dense_qp(p.A, p.B, p.Q, p.R, p.QN, p.x0[b], p.N, None if p.q is None else p.q[b])
    A, Bv = hr.planes(p)
    nh = A.shape[2]
    rows, rh = [], []
    for k in range(p.N):
        if A[b, k].any():
            row = np.zeros(p.L)
            row[k * p.nb + p.m:k * p.nb + p.m + nh] = A[b, k]
            rows.append(row)
            rh.append(Bv[b, k])
    return P, q, G, rhs, np.array(rows), np.array(rh)


def test_a_small_instance_equals_slsqp_on_the_dense_qp():
    """N = 6, (4, 2), nh = 2, per-QP planes and the input box (a seed at which all three QPs are feasible): the ADMM fixed point
    against SciPy's SLSQP on the dense QP with the dynamics as equalities, the planes as inequalities and the box as bounds."""
    from scipy.optimize import minimize
    p = random_planes(pkg.random_ltv(N=6, n=4, m=2, batch=3, seed=8, state_bounds=False), 2, True, seed=7, free=3)
    res = hr.solve(p, rho=1.0, alpha=1.6, eps_abs=1e-11, eps_rel=1e-11, max_iter=40000, check_interval=10)
    assert res.status.all()
    lo, hi = admm_ref.expand_bounds(p.lo, p.hi, p.N, p.nb)
    n_act = 0
    for b in range(p.batch):
        P, q, G, rhs, Ah, bh = dense_with_planes(p, b)
        sol = minimize(lambda w: 0.5 * w @ P @ w + q @ w, res.z[b] * 0.0, jac=lambda w: P @ w + q, method="SLSQP",
                       bounds=list(zip(np.where(np.isfinite(lo), lo, None), np.where(np.isfinite(hi), hi, None))),
                       constraints=[dict(type="eq", fun=lambda w: G @ w - rhs, jac=lambda w: G),
                                    dict(type="ineq", fun=lambda w: bh - Ah @ w, jac=lambda w: -Ah)],
                       options=dict(ftol=1e-14, maxiter=2000))
        assert sol.success, sol.message
        assert np.abs(sol.x - res.z[b]).max() <= 2e-6, (b, np.abs(sol.x - res.z[b]).max())
        f_admm = 0.5 * res.z[b] @ P @ res.z[b] + q @ res.z[b]
        assert abs(f_admm - sol.fun) <= 1e-8 * max(1.0, abs(sol.fun))
        n_act += int((np.abs(Ah @ res.z[b] - bh) <= 1e-8).sum())
    assert n_act >= 3                                               # the planes matter in this instance
    c = hr.conditions(p, res.z, res.y, res.rho)
    for name in ("feas_dyn", "stat", "feas_plane", "normal", "sign", "comp"):
        assert c[name].max() <= 1e-8, (name, c[name])


# ---- the precondition of the GPU cases ----

def _assert_kinds(p, v, what):
    on, off, none = hr.stage_kinds(p, v)
    assert (on >= 1).all() and (off >= 1).all() and (none >= 1).all(), (what, on, off, none)


@pytest.mark.parametrize("case", ITER_CASES, ids=ITER_IDS)
def test_the_iterate_cases_have_every_kind_of_stage(case):
    """In the reference run of each GPU iterate case, at its last step, every QP has a stage that is moved onto its plane, a stage
    whose plane is satisfied with t = 0 and a stage with a = 0."""
    p, kw = iter_case(*case)
    lv = []
    ref_iterates(p, kw, ITER_STEPS[-1], case[8], last_v=lv)
    _assert_kinds(p, lv[0], case)


def test_the_solve_case_has_every_kind_of_stage_and_converges():
    p = solve_problem()
    lv, dec = [], []
    res = hr.solve(p, last_v=lv, decisions=dec, **SOLVE_OPTS)
    assert res.status.all() and res.iters_run < SOLVE_OPTS["max_iter"]
    _assert_kinds(p, lv[0], "solve")
    c = hr.conditions(p, res.z, res.y, res.rho)
    print({k: float(np.max(v)) for k, v in c.items()}, res.iters_run, res.rho, dec)
    assert c["feas_plane"].max() <= 1e-12 and (c["n_active"] >= 1).all()
