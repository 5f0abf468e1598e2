"""Minimum-fuel cost  + sum_k f_k ||u_k||_2  on the GPU against tests/_fuel_ref.py -- admm_ref's batch loop with the
shrink-then-scale prox (tests/test_fuel_host.py checks that helper on the CPU).  Every test asserts the kernel path it names
through s.path(); the problems pass the forward-elimination probe (tests/_shapes.py ALT_TABLE: the probe depends on dynamics,
weights, rho and segments only), and its fallback warning is an error in this module."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded, as in tests/test_gpu_device_io.py: test_refusals builds a DeviceProblem)

import admm_library_amd as pkg
import _fuel_ref as fr
from admm_library_amd import _abi
from _shapes import ALT_TABLE, SWEEP_N, SWEEP_SEGMENTS

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error:.*forward-elimination form failed:RuntimeWarning")]
TOL = 1e-10            # relative, as tests/test_gpu_parity.py::test_thrust_magnitude_constraint; residuals 1e-10
UNSUPPORTED, INVALID = 2, 1
PATHS = {"default": 0, "plain": _abi.FLAG_NO_ALTERNATE, "unfused": _abi.FLAG_UNFUSED}
# the shapes of SOC_CASES (tests/test_gpu_parity.py): (6, 3) at batches on both sides of 64 and 128, (4, 2), (12, 6), (3, 1)
SHAPES = [((6, 3), 5), ((6, 3), 70), ((6, 3), 130), ((4, 2), 66), ((12, 6), 3), ((3, 1), 4)]
VARIANTS = ["scalar_bounded", "per_stage", "no_bound"]


def make_case(shape, batch, variant, with_q):
    """random_ltv of the shape sweep (passes the probe at ALT_TABLE's rho with SWEEP_SEGMENTS segments) with a fuel term:
      scalar_bounded  one weight, a finite thrust bound at every stage
      per_stage       per-stage weights with zeros among them (those stages: ball only, or their box), unorm = inf on some
                      stages that carry a weight
      no_bound        a weight and no thrust bound at all; state rows unbounded (the XFREE kernel forms)"""
    (n, m), (seed, rho) = shape, ALT_TABLE[shape]
    p = pkg.random_ltv(N=SWEEP_N, n=n, m=m, batch=batch, seed=seed, with_q=with_q, state_bounds=variant != "no_bound", thrust_norm=True)
    rng = np.random.default_rng(seed + 17)
    lo, hi, un = p.lo.copy(), p.hi.copy(), p.unorm.copy()
    if variant == "per_stage":
        fuel = rng.uniform(0.05, 0.5, p.N)
        fuel[~np.isfinite(un)] = 0.0          # the stages whose control rows keep their box
        fuel[1::5] = 0.0                      # ball only
        free = np.where(np.isfinite(un))[0][::3]
        un[free] = np.inf                     # weight, no bound
        fuel[free] = np.maximum(fuel[free], 0.1)
        assert (fuel == 0).any() and (fuel[free] > 0).all()
    else:
        lo[:, :m], hi[:, :m] = -np.inf, np.inf
        fuel = np.float64(0.25)
        un = np.where(np.isfinite(un), un, 0.4) if variant == "scalar_bounded" else None
    return dataclasses.replace(p, lo=lo, hi=hi, unorm=un, fuel=fuel), rho


def _solver(p, opts, batch_rule=True):
    s = pkg.Solver(p, opts)
    path = s.path()
    want_alt = not opts.flags & (_abi.FLAG_NO_ALTERNATE | _abi.FLAG_UNFUSED)
    assert path["alternating"] == want_alt and path["kernel_family"] == "one_lane_fp64", path
    return s


def _close(a, b, tol=TOL):
    return np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("with_q", [False, True], ids=["noq", "q"])
@pytest.mark.parametrize("alpha", [1.0, 1.5])
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape,batch", SHAPES, ids=[f"n{s[0]}m{s[1]}b{b}" for s, b in SHAPES])
def test_iterates_and_residuals_match_the_helper(gpu, shape, batch, variant, path, alpha, with_q):
    p, rho = make_case(shape, batch, variant, with_q)
    opts = pkg.Options(rho=rho, alpha=alpha, segments=SWEEP_SEGMENTS, flags=PATHS[path])
    with _solver(p, opts) as s:
        assert s.path()["segments"] == SWEEP_SEGMENTS and s.path()["xfree"] == (variant == "no_bound")
        assert np.array_equal(s.fuel(), fr.expand_fuel(p.fuel, p.N))
        done = 0
        for upto in (1, 2, 9, 30):
            s.run(upto - done, residual_every=3)
            done = upto
            w, z, y = s.get()
            ref = fr.solve(p, rho=rho, alpha=alpha, max_iter=upto, check_interval=3, eps_abs=0, eps_rel=0, stop=False)
            for name, a, b in (("w", w, ref.w), ("z", z, ref.z), ("y", y, ref.y)):
                assert _close(a, b), (upto, name, np.abs(a - b).max())
        r, sd, *_ = s.residuals()
        assert np.abs(r - ref.r).max() <= 1e-10 and np.abs(sd - ref.s).max() <= 1e-10
    nr = np.linalg.norm(z.reshape(p.batch, p.N, p.nb)[:, :, :p.m], axis=2)
    assert (nr <= fr.expand_unorm(p.unorm, p.N)[None] * (1 + 1e-14)).all()


# full solves: (case, rho, adaptive) with the helper converging inside max_iter for every QP (checked on the CPU when they were fixed;
# asserted below, so that no case passes by hitting max_iter on both sides)
SOLVES = [
    # helper on the CPU: iterations (all QPs converged), rho updates
    (lambda: pkg.cw_rendezvous_fuel(N=50, batch=70, u_max=0.5), 1.0, 0),        # 160
    (lambda: pkg.cw_rendezvous_fuel(N=50, batch=70, u_max=0.5), 0.1, 20),       # 410, 2 updates: a poor rho, the adaptive rule moves it
    (lambda: make_case((6, 3), 130, "no_bound", True)[0], 0.3, 0),              # 700
    (lambda: make_case((6, 3), 70, "scalar_bounded", True)[0], 0.3, 10),        # 490, 2 updates
    (lambda: make_case((6, 3), 5, "per_stage", True)[0], 0.03, 10),             # 240, 5 updates
    (lambda: make_case((4, 2), 66, "no_bound", False)[0], 0.03, 10),            # 260, 5 updates
    (lambda: make_case((12, 6), 3, "scalar_bounded", True)[0], 0.03, 10),       # 370, 5 updates
    (lambda: make_case((12, 6), 3, "no_bound", True)[0], 0.3, 0),               # 230
    (lambda: make_case((3, 1), 4, "per_stage", False)[0], 3.0, 10),             # 60, 1 update
    # (u_max = 0.2 at N = 50, and the state-bounded random cases at the larger batches, hold QPs that need more than the suite's
    #  1500 iterations at any rho tried: not used here)
]


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("idx", range(len(SOLVES)))
def test_full_solve_fixed_and_adaptive_rho(gpu, idx, path):
    """iters_run, n_converged, rho_updates and the final rho equal the helper's: a kappa = f / rho left stale by a rho change
    would shift the iteration count and z."""
    make, rho, adapt = SOLVES[idx]
    p = make()
    kw = dict(rho=rho, eps_abs=1e-6, eps_rel=1e-6, max_iter=1500, check_interval=10, adapt_interval=adapt)
    ref = fr.solve(p, **kw)
    assert ref.status.all() and ref.iters_run < 1500, (ref.iters_run, int(ref.status.sum()))
    if adapt:
        assert ref.rho_updates > 0
    segs = dict(segments=SWEEP_SEGMENTS) if p.N == SWEEP_N else {}
    with _solver(p, pkg.Options(flags=PATHS[path], **segs, **kw)) as s:
        info = s.solve()
        w, z, y = s.get()
    print(f"case {idx} {path}: iters {info.iters_run} / {ref.iters_run}, rho {info.rho} / {ref.rho}, updates {info.rho_updates} / {ref.rho_updates}, "
          f"|z - ref| {np.abs(z - ref.z).max():.3e}")
    assert (info.iters_run, info.n_converged, info.rho_updates, info.rho) == (ref.iters_run, int(ref.status.sum()), ref.rho_updates, ref.rho)
    assert _close(z, ref.z) and _close(y, ref.y)


@pytest.mark.parametrize("path", list(PATHS))
def test_set_rho_and_set_fuel_in_mid_run(gpu, path):
    p, rho = make_case((6, 3), 70, "per_stage", True)
    f0 = fr.expand_fuel(p.fuel, p.N)
    with _solver(p, pkg.Options(rho=rho, segments=SWEEP_SEGMENTS, flags=PATHS[path])) as s:
        s.run(12, residual_every=4)
        _, z, y = s.get()
        ref = fr.solve(p, rho=rho, max_iter=12, stop=False)
        assert _close(z, ref.z) and _close(y, ref.y)
        # rho change: the helper continued from the same (z, y) with y rescaled, kappa = f / rho_new
        rho2 = 0.75
        s.set_rho(rho2)
        s.run(7, residual_every=3)
        w, z, y = s.get()
        ref = fr.solve(p, rho=rho2, max_iter=7, stop=False, z0=ref.z, y0=ref.y * (rho / rho2))
        assert _close(w, ref.w) and _close(z, ref.z) and _close(y, ref.y)
        # new weights (continuation): same state, new prox
        f1 = np.where(f0 > 0, 2.5 * f0, 0.0)
        s.set_fuel(f1)
        assert np.array_equal(s.fuel(), f1)
        _, zk, yk = s.get()
        assert np.array_equal(zk, z) and np.array_equal(yk, y)            # the state is kept as the (z, y) pair
        s.run(9, residual_every=2)
        w, z, y = s.get()
        ref = fr.solve(p, rho=rho2, max_iter=9, stop=False, z0=ref.z, y0=ref.y, fuel=f1)
        assert _close(w, ref.w) and _close(z, ref.z) and _close(y, ref.y)
        # refused changes leave the handle as it was
        before = s.get()
        bad = f1.copy()
        bad[3] = -1.0
        with pytest.raises(ValueError, match="fuel"):
            s.set_fuel(bad)
        assert s._lib.admm_set_fuel(s._h, _abi.dptr(bad)) == INVALID and b"fuel" in s._lib.admm_last_error()
        boxed = np.where(~np.isfinite(fr.expand_unorm(p.unorm, p.N)) & (f1 == 0))[0]        # stages whose control rows are bounded
        assert np.isfinite(p.lo[boxed[0], 0])
        bad = f1.copy()
        bad[boxed[0]] = 0.1
        assert s._lib.admm_set_fuel(s._h, _abi.dptr(bad)) == INVALID and b"unbounded" in s._lib.admm_last_error()
        lo2 = p.lo.copy()
        k = int(np.where(f1 > 0)[0][0])
        lo2[k, 0] = -0.3                                                   # a bounded control row under a positive weight
        cp, keep = _abi.marshal_problem(dataclasses.replace(p, lo=lo2, fuel=None))
        assert s._lib.admm_update_problem(s._h, C.byref(cp)) == INVALID and b"fuel" in s._lib.admm_last_error()
        with pytest.raises(ValueError, match="unbounded.*fuel"):
            s.update_problem(dataclasses.replace(p, lo=lo2, fuel=None))
        with pytest.raises(ValueError, match="set_fuel"):
            s.update_problem(p)                                            # (p carries the weights the handle had at setup)
        assert np.array_equal(s.fuel(), f1) and all(np.array_equal(a, b) for a, b in zip(s.get(), before))
        # an accepted update keeps the weights: new x0 and q, the helper continued
        p2 = dataclasses.replace(p, x0=0.5 * p.x0, q=-p.q, fuel=None)
        s.update_problem(p2)
        assert np.array_equal(s.fuel(), f1)
        s.update_instances(x0=p2.x0)
        s.run(6, residual_every=3)
        _, z, y = s.get()
        ref = fr.solve(p2, rho=rho2, max_iter=6, stop=False, z0=ref.z, y0=ref.y, fuel=f1)
        assert _close(z, ref.z) and _close(y, ref.y)
    # on a handle without the term
    with pkg.Solver(dataclasses.replace(p, fuel=None), pkg.Options(rho=rho, segments=SWEEP_SEGMENTS)) as s:
        assert s._lib.admm_set_fuel(s._h, _abi.dptr(f0)) == INVALID and b"cannot be added" in s._lib.admm_last_error()
        assert not s.fuel().any()


@pytest.mark.parametrize("path", ["default", "plain"])
@pytest.mark.parametrize("kind", ["thrust_bound", "box_only"])
def test_zero_weights_are_the_handle_without_the_term_bit_for_bit(gpu, kind, path):
    """fuel = zeros runs the SOC forms; with kappa = 0 they compute what the handle of admm_setup computes, to the last bit."""
    seed, rho = ALT_TABLE[(6, 3)]
    p = pkg.random_ltv(N=SWEEP_N, n=6, m=3, batch=70, seed=seed, thrust_norm=kind == "thrust_bound")
    opts = pkg.Options(rho=rho, alpha=1.5, segments=SWEEP_SEGMENTS, flags=PATHS[path] | _abi.FLAG_NO_MFMA)
    out = []
    for fuel in (None, np.zeros(p.N)):
        with _solver(dataclasses.replace(p, fuel=fuel), opts) as s:
            s.run(30, residual_every=3)
            out.append(s.get() + tuple(s.residuals()))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_refusals(gpu):
    inst = pkg.random_instances(N=6, n=4, m=2, batch=3, seed=2, thrust_norm=True)
    cp, keep = _abi.marshal_problem(inst)
    lib, h = pkg.load_library(), C.c_void_p()
    assert lib.admm_setup_fuel(C.byref(h), C.byref(cp), None, _abi.dptr(np.zeros(6))) == UNSUPPORTED and not h.value
    assert b"fuel" in lib.admm_last_error()
    p = pkg.cw_rendezvous_fuel(N=150, batch=8)
    for mode in (_abi.PRECISION_MIXED, _abi.PRECISION_FP64_MFMA):
        with pytest.raises(pkg.AdmmError) as e:
            pkg.Solver(p, pkg.Options(rho=0.1, precision_mode=mode))
        assert e.value.code == UNSUPPORTED and "fuel" in str(e.value)
    with pytest.raises(pkg.AdmmError) as e:
        pkg.Solver(p, pkg.Options(rho=0.1, segments=4), timeshard=(0, 1, None))
    assert e.value.code == UNSUPPORTED and "time-sharded" in str(e.value)
    d = pkg.DeviceProblem.from_problem(p)
    assert d.fuel is not None
    with pytest.raises(ValueError, match="fuel"):
        pkg.Solver(d, pkg.Options(rho=0.1))
    # small batches at (6, 3) without q: the MFMA form is the default there -- not with a fuel term, zero weights included
    for fuel, family in ((None, "mfma_fp64"), (np.float64(0.0), "one_lane_fp64"), (p.fuel, "one_lane_fp64")):
        q = pkg.cw_rendezvous(N=150, batch=8) if fuel is None else dataclasses.replace(p, unorm=None, fuel=fuel)
        with pkg.Solver(q, pkg.Options(rho=0.05)) as s:
            assert s.path()["kernel_family"] == family and s.path()["alternating"], s.path()


def test_sharded_batch_carries_the_weights(gpu):
    p = pkg.cw_rendezvous_fuel(N=50, batch=9)
    full = fr.solve(p, rho=1.0, max_iter=25, stop=False)
    for rank in range(2):
        lo, hi = pkg.shard_bounds(p.batch, 2, rank)
        with _solver(pkg.shard_problem(p, 2, rank), pkg.Options(rho=1.0)) as s:
            s.iterate(25)
            _, z, _ = s.get()
        assert _close(z, full.z[lo:hi])


# Certificate tolerances of the at-size test: the helper's own residuals on the 64-QP slice at the same eps, rho and
# stopping rule on the CPU -- feas_dyn 1.6e-8, stat 1.1e-5 -- times 10 (another summation order, 4096 QPs instead of 64).
AT_SIZE_FEAS_DYN, AT_SIZE_STAT = 1.6e-7, 1.1e-4


def test_structure_at_size(gpu):
    """N = 1000, n = 6, m = 3, batch 4096 (cw_rendezvous_fuel): a 64-QP slice against the helper, the coast / burn structure, and
    the optimality certificate of the fuel problem over all QPs."""
    p = pkg.cw_rendezvous_fuel(N=1000, batch=4096)
    rho, umax = 1.0, float(p.unorm)
    kw = dict(rho=rho, eps_abs=1e-6, eps_rel=1e-6, check_interval=10)
    sl = p.slice(0, 64)
    with _solver(p, pkg.Options(max_iter=6000, **kw)) as s:
        # the slice alone on the CPU, iterate for iterate (QPs are independent)
        s.run(200, residual_every=10)
        w, z, y = s.get()
        ref = fr.solve(sl, max_iter=200, stop=False, **kw)
        assert _close(z[:64], ref.z) and _close(w[:64], ref.w) and _close(y[:64], ref.y)
        info = s.solve(z0=np.zeros_like(z), y0=np.zeros_like(y))
        w, z, y = s.get()
    nr = np.linalg.norm(z.reshape(p.batch, p.N, p.nb)[:, :, :p.m], axis=2)
    coast, bound = nr == 0, nr >= umax * (1 - 1e-9)
    print(f"at size: iters {info.iters_run}, converged {info.n_converged} / 4096, {info.solve_ms:.1f} ms; coast share {coast.mean():.3f}, "
          f"on the bound {bound.mean():.3f}")
    assert (nr <= umax * (1 + 1e-14)).all()
    assert coast.any() and bound.any()
    # per QP, where the helper's converged solution of the slice shows it (the helper converges for every QP of the slice: 1060
    # iterations on the CPU when this case was fixed)
    ref = fr.solve(sl, max_iter=1500, **kw)
    assert ref.status.all() and ref.iters_run < 1500
    rnr = np.linalg.norm(ref.z.reshape(64, p.N, p.nb)[:, :, :p.m], axis=2)
    rcoast, rbound = (rnr == 0).any(axis=1), (rnr >= umax * (1 - 1e-9)).any(axis=1)
    assert rcoast.any() and rbound.any()
    assert coast[:64][rcoast].any(axis=1).all() and bound[:64][rbound].any(axis=1).all()
    assert info.iters_run >= ref.iters_run
    c = fr.certificate(p, z, y, rho)
    print(f"at size: certificate feas_dyn {c['feas_dyn'].max():.3e} stat {c['stat'].max():.3e} fuel {c['fuel'].max():.3e} "
          f"feas_ball {c['feas_ball'].max():.3e}; unconverged {4096 - info.n_converged}")
    assert info.n_converged == 4096
    assert c["fuel"].max() <= 1e-12 and c["feas_ball"].max() <= 1e-14 and c["comp_x"].max() == 0.0
    assert c["feas_dyn"].max() <= AT_SIZE_FEAS_DYN and c["stat"].max() <= AT_SIZE_STAT
