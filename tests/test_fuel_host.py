"""Minimum-fuel cost  + sum_k f_k ||u_k||_2  (DESIGN.md §2.7), the part that needs no GPU: the reference the GPU tests compare
against (tests/_fuel_ref.py) is checked here against admm_ref (fuel = 0), against brute force (the prox) and against the
optimality conditions of the fuel problem; then Problem.validate and the validation step of admm_setup_fuel, which runs
before a device is looked for."""
import ctypes as C
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import admm_library_amd as pkg
import admm_ref as ar
import _fuel_ref as fr
from admm_library_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1


def _ref_solve(p, **kw):
    return ar.solve(p.A, p.B, p.Q, p.R, p.QN, p.x0, p.lo, p.hi, p.N, q=p.q, unorm=p.unorm, **kw)


@pytest.mark.parametrize("make,kw", [
    (lambda: pkg.random_ltv(N=23, n=6, m=3, batch=5, seed=3, thrust_norm=True), dict(rho=0.4, alpha=1.5, max_iter=40, stop=False)),
    (lambda: pkg.cw_rendezvous(N=60, batch=3, thrust_norm=True), dict(rho=0.05, max_iter=400, adapt_interval=20)),
    (lambda: pkg.random_ltv(N=15, n=4, m=2, batch=4, seed=8), dict(rho=0.3, max_iter=300, adapt_interval=10, check_interval=5)),
    (lambda: pkg.double_integrator(N=30, batch=3), dict(rho=1.0, alpha=1.2, max_iter=200)),
], ids=["soc_ltv", "soc_cw_adaptive", "box_ltv_adaptive", "box_di"])
def test_helper_without_fuel_is_admm_ref_bit_for_bit(make, kw):
    p = make()
    ref = _ref_solve(p, **kw)
    for fuel in (None, 0.0, np.zeros(p.N)):
        got = fr.solve(p, fuel=fuel, **kw)
        assert got.iters_run == ref.iters_run and got.rho == ref.rho and got.rho_updates == ref.rho_updates
        for name in ("w", "z", "y", "r", "s", "iters", "status"):
            assert np.array_equal(getattr(got, name), getattr(ref, name)), name


def _ball_sample(m, ub, rng):
    """A fine sample of the ball ||z|| <= ub in R^m (ub = inf: of a ball that contains every candidate minimiser, |z| <= |v|)."""
    if m == 1:
        return np.linspace(-ub, ub, 20001)[:, None]
    if m == 2:
        r, th = np.meshgrid(np.linspace(0, ub, 301), np.linspace(0, 2 * np.pi, 721), indexing="ij")
        return np.stack([r * np.cos(th), r * np.sin(th)], axis=-1).reshape(-1, 2)
    r = np.linspace(0, ub, 61)
    th = np.linspace(0, np.pi, 91)
    ph = np.linspace(0, 2 * np.pi, 181)
    R, T, P = np.meshgrid(r, th, ph, indexing="ij")
    return np.stack([R * np.sin(T) * np.cos(P), R * np.sin(T) * np.sin(P), R * np.cos(T)], axis=-1).reshape(-1, 3)


@pytest.mark.parametrize("m", [1, 2, 3])
def test_prox_against_brute_force(m):
    """z = prox(v) minimises  kappa ||z|| + 1/2 ||z - v||^2  over the ball: no point of a fine sample of the ball (plus the
    radial candidates, where the minimiser lies) has a lower value."""
    rng = np.random.default_rng(100 + m)
    n = 2
    seen = set()
    for trial in range(40):
        v_u = rng.standard_normal(m) * rng.choice([0.05, 0.5, 2.0])
        kap = float(rng.choice([0.0, 0.02, 0.3, 1.0, 5.0]))
        ub = float(rng.choice([0.1, 0.7, 3.0, np.inf]))
        v = np.concatenate([v_u, rng.standard_normal(n)])[None]
        lo, hi = np.full(m + n, -np.inf), np.full(m + n, np.inf)
        z = fr.prox(v, lo, hi, np.array([ub]), np.array([kap]), m)
        zu = z[0, :m]
        assert np.array_equal(z[0, m:], v[0, m:])                       # state rows: their (open) box
        assert np.linalg.norm(zu) <= ub * (1 + 1e-15)
        nv = np.linalg.norm(v_u)
        radius = ub if np.isfinite(ub) else nv
        cand = _ball_sample(m, radius, rng)
        if nv > 0:          # the ray through v, finely: the minimiser is on it
            cand = np.concatenate([cand, np.linspace(0, min(radius, nv), 4001)[:, None] * (v_u / nv)[None]])

        def cost(zz):
            return kap * np.linalg.norm(zz, axis=-1) + 0.5 * np.sum((zz - v_u) ** 2, axis=-1)
        assert cost(zu) <= cost(cand).min() + 1e-13 * max(1.0, cost(zu)), (trial, v_u, kap, ub)
        seen.add("coast" if not zu.any() else "bound" if np.linalg.norm(zu) >= ub * (1 - 1e-12) else "mid")
        if nv <= kap:
            assert not zu.any()                                          # a coast stage is exactly zero
    assert seen == {"coast", "bound", "mid"}


def _case(name):
    if name == "cw_scalar":
        return pkg.cw_rendezvous_fuel(N=50, batch=4), 1.0
    if name == "cw_no_bound":
        p = pkg.cw_rendezvous_fuel(N=50, batch=4)
        return dataclasses.replace(p, unorm=None), 1.0
    p = pkg.random_ltv(N=23, n=6, m=3, batch=5, seed=3, thrust_norm=True)       # per-stage: zeros among the weights, inf among the bounds
    rng = np.random.default_rng(5)
    fuel = rng.uniform(0.05, 0.4, p.N)
    fuel[::4] = 0.0                       # the stages whose control rows keep their box
    fuel[1::5] = 0.0
    un = p.unorm.copy()
    free = np.where(np.isfinite(un))[0][::3]
    un[free] = np.inf                     # weight without a bound on some stages
    fuel[free] = np.maximum(fuel[free], 0.1)
    return dataclasses.replace(p, unorm=un, fuel=fuel), 0.4


@pytest.mark.parametrize("name", ["cw_scalar", "cw_no_bound", "ltv_per_stage"])
def test_optimality_certificate_at_the_helpers_converged_point(name):
    p, rho = _case(name)
    eps = 1e-9
    r = fr.solve(p, rho=rho, eps_abs=eps, eps_rel=eps, max_iter=20000, check_interval=10)
    assert r.status.all(), (r.iters_run, r.r.max(), r.s.max())
    c = fr.certificate(p, r.z, r.y, rho)
    scale = max(1.0, np.abs(r.z).max(), rho * np.abs(r.y).max())
    # the prox relations hold to rounding at every iterate; feasibility of the dynamics and stationarity hold at convergence:
    # |w - z| <= eps-level primal residual, rho |z+ - z| the dual one (sqrt(L) eps_abs + eps_rel |.|, L <= 450)
    assert c["fuel"].max() <= 1e-12 * scale and c["comp_x"].max() <= 1e-12 * scale
    assert c["feas_ball"].max() <= 1e-14 and c["feas_box"].max() == 0.0
    bound = 50 * np.sqrt(p.L) * eps * scale
    assert c["feas_dyn"].max() <= bound and c["stat"].max() <= bound, (c["feas_dyn"].max(), c["stat"].max(), bound)
    if name.startswith("cw"):
        assert c["n_coast"].sum() > 0 and c["n_mid"].sum() > 0
    if name == "cw_scalar":
        assert c["n_bound"].sum() > 0
    # a stronger weight never burns more: total ||u|| is monotone in the weight
    if name == "cw_scalar":
        burn = [np.linalg.norm(fr.solve(dataclasses.replace(p, fuel=np.float64(f)), rho=rho, max_iter=3000).z
                               .reshape(p.batch, p.N, p.nb)[:, :, :p.m], axis=2).sum() for f in (0.0, float(p.fuel), 4 * float(p.fuel))]
        assert burn[0] > burn[1] > burn[2]


def test_problem_validate_and_slice():
    p = pkg.cw_rendezvous_fuel(N=12, batch=6)
    p.validate()
    assert float(p.fuel) == pytest.approx(2 * np.pi / 12) and p.unorm is not None
    assert pkg.cw_rendezvous_fuel(N=12, batch=6, fuel=0.3).fuel == 0.3
    assert [f.name for f in dataclasses.fields(pkg.Problem)][-1] == "fuel"
    sl = pkg.shard_problem(p, 3, 1)
    assert sl.batch == 2 and sl.fuel == p.fuel
    for bad in (-0.1, np.nan, np.inf, np.zeros(12), np.zeros((1, 1))):          # (N,) needs per-stage bounds
        with pytest.raises(ValueError, match="fuel"):
            dataclasses.replace(p, fuel=np.asarray(bad)).validate()
    ps = dataclasses.replace(p, lo=np.tile(p.lo, (12, 1)), hi=np.tile(p.hi, (12, 1)), unorm=np.full(12, 0.2))
    dataclasses.replace(ps, fuel=np.linspace(0, 1, 12)).validate()
    with pytest.raises(ValueError, match="fuel"):
        dataclasses.replace(ps, fuel=np.ones(11)).validate()                    # wrong length
    box = pkg.cw_rendezvous(N=12, batch=2)                                      # bounded control rows
    dataclasses.replace(box, fuel=np.float64(0.0)).validate()                   # weight 0: the box may stay
    with pytest.raises(ValueError, match="unbounded.*fuel"):
        dataclasses.replace(box, fuel=np.float64(0.1)).validate()
    inst = pkg.random_instances(N=6, n=4, m=2, batch=3, seed=2, thrust_norm=True)
    with pytest.raises(ValueError, match="fuel"):
        dataclasses.replace(inst, fuel=np.zeros(6)).validate()
    assert np.array_equal(_abi.marshal_fuel(p), [float(p.fuel)])
    assert _abi.marshal_fuel(dataclasses.replace(ps, fuel=np.float64(0.5))).shape == (12,)


def test_header_and_library_announce_the_feature(lib):
    hdr = open(os.path.join(ROOT, "include", "admm_hip.h")).read()
    assert re.search(r"^#define ADMM_HIP_HAS_FUEL 1\s*$", hdr, re.M)
    assert re.search(r"^#define ADMM_HIP_ABI_VERSION 9\s*$", hdr, re.M) and lib.admm_abi_version() == 9
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for decl in (r"int admm_setup_fuel\(admm_handle\*\* out, const admm_problem\* p, const admm_options\* o, const double\* fuel\);",
                 r"int admm_set_fuel\(admm_handle\* h, const double\* fuel\);", r"int admm_get_fuel\(admm_handle\* h, double\* fuel\);"):
        assert re.search(decl, code), decl
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.library_path()], capture_output=True, text=True, check=True).stdout
    assert {"admm_setup_fuel", "admm_set_fuel", "admm_get_fuel"} <= set(re.findall(r"\bT (admm_[a-z_]+)\b", nm))


def test_setup_fuel_validates_before_the_device(lib):
    """Through ctypes, past Problem.validate: the checks of admm_setup_fuel come before the device look-up, so a bad weight is
    ADMM_ERR_INVALID with a message naming `fuel` on a machine without a GPU too."""
    h = C.c_void_p()

    def rc(cp, fuel):
        code = lib.admm_setup_fuel(C.byref(h), C.byref(cp), None, _abi.dptr(fuel))
        assert not h.value or code == 0
        if h.value:                       # (a GPU is present: valid input sets a handle up)
            lib.admm_free(h)
            h.value = None
        return code, lib.admm_last_error().decode()

    cp, keep = _abi.marshal_problem(pkg.cw_rendezvous(N=10, batch=2, thrust_norm=True))
    for bad in (-1.0, np.nan, np.inf):
        code, msg = rc(cp, np.array([bad]))
        assert code == INVALID and "fuel" in msg, (bad, code, msg)
    # per-stage box: N entries are read
    ps = pkg.random_ltv(N=9, n=4, m=2, batch=2, seed=1, thrust_norm=True)
    cps, keeps = _abi.marshal_problem(ps)
    fuel = np.zeros(9)
    fuel[8] = -0.5
    code, msg = rc(cps, fuel)
    assert code == INVALID and "fuel" in msg
    # a positive weight on a stage whose control rows are bounded (stages 0, 4, 8 of this generator keep their box)
    assert np.isfinite(ps.lo[4, 0])
    fuel[:] = 0.0
    fuel[4] = 0.1
    code, msg = rc(cps, fuel)
    assert code == INVALID and "unbounded (-inf, inf) where fuel" in msg
    cpb, keepb = _abi.marshal_problem(pkg.cw_rendezvous(N=10, batch=2))
    code, msg = rc(cpb, np.array([0.1]))
    assert code == INVALID and "unbounded (-inf, inf) where fuel" in msg
    # valid weights pass the validation step: what comes back is the device's answer, not ADMM_ERR_INVALID
    fuel[4] = 0.0
    fuel[1] = 0.2
    assert rc(cps, fuel)[0] in (0, 3)
    assert rc(cpb, np.array([0.0]))[0] in (0, 3)
    # the refusals come before the device too
    inst = pkg.random_instances(N=6, n=4, m=2, batch=3, seed=2, thrust_norm=True)
    cpi, keepi = _abi.marshal_problem(inst)
    code, msg = rc(cpi, np.zeros(6))
    assert code == 2 and "fuel" in msg
    o = _abi.make_options(precision_mode=_abi.PRECISION_MIXED)
    assert lib.admm_setup_fuel(C.byref(h), C.byref(cp), C.byref(o), _abi.dptr(np.array([0.1]))) == 2 and b"fuel" in lib.admm_last_error()
    # NULL handle
    assert lib.admm_set_fuel(None, _abi.dptr(np.zeros(1))) == INVALID and lib.admm_get_fuel(None, _abi.dptr(np.zeros(1))) == INVALID
