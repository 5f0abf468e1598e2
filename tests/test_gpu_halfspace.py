"""One half-space per stage on the GPU (csrc/admm_halfspace_kernels.hpp) against tests/_halfspace_ref.py -- the
oracle's loop with the projection (tests/test_halfspace_host.py checks that reference on the CPU, holds the cases, and asserts that
every QP of every case has an active stage, a satisfied one and one without a plane).

Shapes are chosen for the kernel's geometry (one lane = two adjacent QPs, 512 columns per workgroup, chunks of whole blocks):
batches 1 and 3 (odd: a pad column beside the last QP), 70 (pad columns) and 514 (two workgroups along the batch); chunks of one,
two or three blocks with a shorter last one, and a single chunk."""
import ctypes as C
import dataclasses
import importlib.util
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded, as in tests/test_gpu_device_io.py)

import admm_library_amd as pkg
import _halfspace_ref as hr
import _readout_cases as rc
import test_halfspace_host as host
from admm_library_amd import _abi

pytestmark = pytest.mark.gpu
TOL = 1e-10            # x max(1, |.|): the project's iterate tolerance
INVALID, UNSUPPORTED = 1, 2
INF = np.inf
DEV = "cuda:0"
RHO = host.RHO


def _close(a, b, tol=TOL):
    return np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


def _solver(p, **kw):
    s = pkg.Solver(p, pkg.Options(**kw))
    path = s.path()
    assert not path["alternating"] and not path["alt_requested"] and path["kernel_family"] == "one_lane_fp64", path
    return s


def _state(s):
    return s.get() + tuple(s.residuals())


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. iterates and residuals against the reference ----

@pytest.mark.parametrize("case", host.ITER_CASES, ids=host.ITER_IDS)
def test_iterates_match_the_reference(gpu, case):
    n, m, nh, N, batch, per_qp, kind, alpha, every, zrows = case
    p, kw = host.iter_case(*case)
    with _solver(p, **kw) as s:
        geo = s.geometry()
        assert geo["zrows"] % p.nb == 0
        assert geo["zrows"] == zrows and (geo["zchunks"] == 1 if zrows == p.L else geo["zchunks"] > 1), geo
        a, b = s.halfspace()
        assert np.array_equal(a, p.hs_a) and np.array_equal(b, p.hs_b) and a.ndim == (3 if per_qp else 2)
        done = 0
        for k in host.ITER_STEPS:
            # the spacing within the call (iterations with and without the residual sums), then one iteration that has them:
            # r and s are the last iteration's, as the reference's are
            if k - done > 1:
                s.run(k - done - 1, residual_every=every)
            s.run(1, residual_every=1)
            done = k
            w, z, y = s.get()
            ref = host.ref_iterates(p, kw, k, every)
            for name, got, want in (("w", w, ref.w), ("z", z, ref.z), ("y", y, ref.y)):
                print(case, k, name, np.abs(got - want).max())
                assert _close(got, want), (k, name, np.abs(got - want).max())
            r, sd, *_ = s.residuals()
            print(case, k, "r, s", np.abs(r - ref.r).max(), np.abs(sd - ref.s).max())
            assert np.abs(r - ref.r).max() <= TOL and np.abs(sd - ref.s).max() <= TOL, (k, np.abs(r - ref.r).max(), np.abs(sd - ref.s).max())
    # the planes matter: the problem without them iterates elsewhere
    plain = host.ref_iterates(dataclasses.replace(p, hs_a=np.zeros_like(p.hs_a)), kw, host.ITER_STEPS[-1], every)
    assert np.abs(plain.z - ref.z).max() > 1e-3


# ---- 2. all-zero planes are the unfused path, bit for bit ----

@pytest.mark.parametrize("per_qp", [False, True], ids=["shared", "perqp"])
@pytest.mark.parametrize("alpha", [1.0, 1.6])
@pytest.mark.parametrize("kind", ["box", "thrust", "fuel"])
def test_zero_planes_are_the_unfused_handle_bit_for_bit(gpu, kind, alpha, per_qp):
    """zdual_kernel (box) / zdual_soc_kernel (thrust, fuel) against zdual_halfspace_kernel with a = 0 everywhere (and b of either
    sign), residuals included.  Both handles get two blocks per chunk: the residual sums are added chunk by chunk."""
    batch = 70
    p = pkg.random_ltv(N=9, n=6, m=3, batch=batch, seed=77, thrust_norm=kind != "box")
    if kind == "fuel":
        p = rc.stage_fuel(p)
    cnt = (batch,) if per_qp else ()
    ph = dataclasses.replace(p, hs_a=np.zeros(cnt + (p.N, 3)), hs_b=np.random.default_rng(3).standard_normal(cnt + (p.N,)))
    kw = dict(rho=RHO, alpha=alpha, zrows=2 * p.nb)
    out = []
    with pkg.Solver(p, pkg.Options(flags=_abi.FLAG_UNFUSED, **kw)) as plain, _solver(ph, **kw) as s:
        assert plain.geometry() == s.geometry()
        for h in (plain, s):
            h.run(9, residual_every=3)
            out.append(_state(h))
        rep = s.halfspace_report(multipliers=True)
    assert _same(*out)
    assert not rep.max_violation.any() and not rep.n_active.any() and not rep.lam.any()


# ---- 3. the edges, bit for bit ----

@pytest.fixture(scope="module")
def prox_host(tmp_path_factory):
    return host.build_prox_host(tmp_path_factory.mktemp("halfspace_gpu"))


@pytest.mark.parametrize("n,m,nh,per_qp", [(6, 3, 3, True), (6, 3, 6, False), (4, 2, 4, True), (2, 1, 1, True), (6, 3, 1, False)])
def test_edges_bit_for_bit(gpu, prox_host, n, m, nh, per_qp):
    """The state is set so that v = w + y is exactly the wanted point (y = 0, alpha = 1), then one step_z: the rows under a plane
    get the bits of csrc/admm_prox.hpp compiled on the host -- rows exactly on the plane (d = 0), one ulp of b either side, the
    smallest d, a with zero entries, nh = n, a = 0 -- and every other row its box."""
    rng = np.random.default_rng(60 + nh)
    a_e, b_e, v_e = host.edge_stages(nh, rng)
    E = a_e.shape[0]
    batch = 67 if per_qp else 3
    N = E if not per_qp else 7
    p = pkg.random_ltv(N=N, n=n, m=m, batch=batch, seed=9, state_bounds=True)
    lo, hi = p.lo.copy(), p.hi.copy()
    lo[:, m:m + nh], hi[:, m:m + nh] = -INF, INF
    if per_qp:                       # QP b, stage k carries edge (b + 3 k) % E
        idx = (np.arange(batch)[:, None] + 3 * np.arange(N)[None]) % E
        a, b, vx = a_e[idx], b_e[idx], v_e[idx]
    else:                            # stage k carries edge k, every QP a different point: QP 0 the edge's, the others random
        a, b = a_e, b_e
        vx = np.stack([v_e] + [v_e + rng.standard_normal(v_e.shape) for _ in range(batch - 1)])
    ph = dataclasses.replace(p, lo=lo, hi=hi, hs_a=a, hs_b=b)
    ph.validate()
    v = rng.uniform(-4.0, 4.0, (batch, N, p.nb))
    v[:, :, m:m + nh] = vx
    A, Bv = hr.planes(ph)
    zx, yx, act = prox_host(A.reshape(-1, nh), Bv.reshape(-1), np.ascontiguousarray(v[:, :, m:m + nh]).reshape(-1, nh))
    assert act.any() and not act.all()
    want = np.minimum(np.maximum(v, lo[None]), hi[None])
    want[:, :, m:m + nh] = zx.reshape(batch, N, nh)
    v = v.reshape(batch, -1)
    want = want.reshape(batch, -1)
    with _solver(ph, rho=RHO, zrows=2 * p.nb) as s:
        s.set_state(w=v, z=np.zeros_like(v), y=np.zeros_like(v))
        s.step_z()
        _, z, y = s.get(w=False)
    assert np.array_equal(z, want)
    assert np.array_equal(y, v - want)
    moved = (y.reshape(batch, N, p.nb)[:, :, m:m + nh] != 0).any(axis=2)
    assert moved.any() and (~moved & act.reshape(batch, N).astype(bool)).any()


# ---- 4. a solve with adaptive rho ----

def test_solve_follows_the_reference_and_meets_the_optimality_conditions(gpu):
    """cw_keepout(N = 40, batch 6) to eps = 1e-7 with the adaptive rule (2980 iterations, rho 0.5 -> 1 -> 2 -> 4).  Every quantity
    of the optimality conditions is bounded by ten times what the reference's own solution of the same case has:
        reference   feas_dyn 3.338e-6   stat 1.731e-6   feas_plane 3.33e-16   normal 4.44e-16   sign 0   comp 4.03e-15
        handle      feas_dyn 3.338e-6   stat 1.731e-6   feas_plane 2.78e-16   normal 3.55e-15   sign 0   comp 2.69e-15
    (sign is exactly 0 on either path: a . y is a sum of terms t a_i^2 (1 + eps) with t >= 0, never negative)."""
    p = host.solve_problem()
    dec = []
    ref = hr.solve(p, decisions=dec, **host.SOLVE_OPTS)
    cref = hr.conditions(p, ref.z, ref.y, ref.rho)
    bounds = {name: 10.0 * float(cref[name].max()) for name in ("feas_dyn", "stat", "feas_plane", "normal", "sign", "comp")}
    assert bounds["feas_dyn"] <= 3.4e-5 and bounds["stat"] <= 1.8e-5 and max(bounds["feas_plane"], bounds["normal"], bounds["comp"]) <= 1e-13
    with _solver(p, flags=_abi.FLAG_HISTORY, **host.SOLVE_OPTS) as s:
        info = s.solve()
        _, z, y = s.get(w=False)
        hist = s.history()
        rep = s.halfspace_report()
    assert info.iters_run == ref.iters_run and info.rho == ref.rho and info.rho_updates == ref.rho_updates
    assert np.array_equal(info.status, ref.status) and np.array_equal(info.iters, ref.iters)
    assert len(hist["iteration"]) == ref.iters_run // host.SOLVE_OPTS["check_interval"]
    for it, rho in zip(hist["iteration"], hist["rho"]):       # rho in force at a test = the last decision before it
        prev = [r for i, r in dec if i < it]
        assert rho == (prev[-1] if prev else host.SOLVE_OPTS["rho"]), (it, rho)
    c = hr.conditions(p, z, y, info.rho)
    for name, bnd in bounds.items():
        print(name, c[name].max(), "reference", cref[name].max(), "bound", bnd)
        assert c[name].max() <= bnd, (name, c[name].max())
    assert np.array_equal(c["n_active"], cref["n_active"]) and np.array_equal(rep.n_active, cref["n_active"])
    assert _close(z, ref.z, 1e-8)


# ---- 5. the report ----

@pytest.mark.parametrize("per_qp", [False, True], ids=["shared", "perqp"])
def test_report_matches_numpy_on_the_handles_state(gpu, per_qp):
    case = (6, 3, 3, 9, 70, per_qp, "thrust", 1.6, 1, 18)
    p, kw = host.iter_case(*case)
    with _solver(p, **kw) as s, _solver(p, **kw) as twin:
        s.run(12)
        twin.run(12)
        w, _, y = s.get()
        rep = s.halfspace_report(multipliers=True)
        dev = s.halfspace_report(multipliers=True, device=True)
        torch.cuda.synchronize()
        mx, cnt, lam = hr.report(p, w, y, RHO)
        assert (mx > 0).any() and (cnt > 0).all() and (cnt < p.N).all() and (lam == 0).any() and (lam < 0).sum() == 0
        assert rep.n_active.dtype == np.int32 and np.array_equal(rep.n_active, cnt)
        assert np.abs(rep.max_violation - mx).max() <= 1e-12 * np.abs(mx).max()
        assert np.abs(rep.lam - lam).max() <= 1e-12 * np.abs(lam).max()
        assert rep.lam.shape == (p.batch, p.N)
        for name in ("max_violation", "n_active", "lam"):
            assert np.array_equal(getattr(dev, name).cpu().numpy(), getattr(rep, name)), name
        assert dev.n_active.dtype == torch.int32
        # any pointer may be NULL, and repeating the call gives the same bits
        lib, one = pkg.load_library(), np.zeros(p.batch)
        assert lib.admm_get_halfspace_report(s._h, _abi.dptr(one), None, None) == 0 and np.array_equal(one, rep.max_violation)
        again = s.halfspace_report(multipliers=True)
        assert np.array_equal(again.lam, rep.lam) and np.array_equal(again.max_violation, rep.max_violation)
        # reading changes nothing
        s.run(3, residual_every=1)
        twin.run(3, residual_every=1)
        assert _same(_state(s), _state(twin))


def test_device_form_of_the_report_checks_its_pointers(gpu):
    lib = pkg.load_library()
    p, kw = host.iter_case(6, 3, 3, 9, 70, True, "box", 1.0, 1, 18)

    def dp(t, typ=_abi.c_double_p, off=0):
        return C.cast(C.c_void_p(t.data_ptr() + off), typ)
    with _solver(p, **kw) as s:
        s.run(5)
        ref = s.halfspace_report(multipliers=True)
        t = torch.zeros(p.batch + 1, dtype=torch.float64, device=DEV)
        ti = torch.zeros(p.batch + 1, dtype=torch.int32, device=DEV)
        tl = torch.zeros(p.batch * p.N, dtype=torch.float64, device=DEV)
        st = pkg.solver._stream(DEV)
        assert lib.admm_get_halfspace_report_device(s._h, dp(t[1:]), dp(ti[1:], _abi.c_int32_p), dp(tl), st) == 0
        torch.cuda.synchronize()
        assert np.array_equal(t[1:].cpu().numpy(), ref.max_violation) and t[0] == 0
        assert np.array_equal(ti[1:].cpu().numpy(), ref.n_active) and ti[0] == 0
        assert np.array_equal(tl.cpu().numpy().reshape(p.batch, p.N), ref.lam)
        hostv = np.zeros(p.batch)
        assert lib.admm_get_halfspace_report_device(s._h, _abi.dptr(hostv), None, None, None) == INVALID
        assert "admm_get_halfspace_report_device: max_violation is not device memory" in lib.admm_last_error().decode()
        assert lib.admm_get_halfspace_report_device(s._h, dp(t, off=4), None, None, None) == INVALID
        assert "max_violation is not 8-byte aligned" in lib.admm_last_error().decode()
        assert lib.admm_get_halfspace_report_device(s._h, None, dp(ti, _abi.c_int32_p, off=2), None, None) == INVALID
        assert "n_active is not 4-byte aligned" in lib.admm_last_error().decode()
        big = torch.zeros(3 * 2 ** 20, dtype=torch.float64, device=DEV)      # a block of its own in torch's allocator: its true end is known
        short = big[big.numel() - (p.batch * p.N - 1):]
        assert lib.admm_get_halfspace_report_device(s._h, None, None, dp(short), None) == INVALID
        assert f"lam ends before its {p.batch * p.N} doubles" in lib.admm_last_error().decode()
        assert lib.admm_get_halfspace_report_device(s._h, None, None, None, None) == INVALID and b"at least one" in lib.admm_last_error()
        assert lib.admm_get_halfspace_report(s._h, None, None, None) == INVALID and b"at least one" in lib.admm_last_error()
        assert not hostv.any()
        # ... and of set_halfspace_device
        a = torch.as_tensor(p.hs_a, device=DEV)
        b = torch.as_tensor(p.hs_b, device=DEV)
        assert lib.admm_set_halfspace_device(s._h, _abi.dptr(np.ascontiguousarray(p.hs_a)), dp(b), None) == INVALID
        assert "admm_set_halfspace_device: a is not device memory" in lib.admm_last_error().decode()
        assert lib.admm_set_halfspace_device(s._h, dp(a), dp(short), None) == INVALID and "b ends before" in lib.admm_last_error().decode()
        assert lib.admm_set_halfspace_device(s._h, dp(a), dp(b, off=4), None) == INVALID and "b is not 8-byte aligned" in lib.admm_last_error().decode()
        ha, hb = s.halfspace()
        assert np.array_equal(ha, p.hs_a) and np.array_equal(hb, p.hs_b)
    with pkg.Solver(dataclasses.replace(p, hs_a=None, hs_b=None), pkg.Options(rho=RHO)) as plain:
        assert lib.admm_get_halfspace_report(plain._h, _abi.dptr(hostv), None, None) == INVALID and b"no half-spaces" in lib.admm_last_error()
        assert lib.admm_set_halfspace(plain._h, _abi.dptr(hostv), _abi.dptr(hostv)) == INVALID and b"cannot be added" in lib.admm_last_error()
        with pytest.raises(pkg.AdmmError):
            plain.halfspace()


# ---- 6. set_halfspace ----

def _new_planes(p, seed):
    q = host.random_planes(dataclasses.replace(p, hs_a=None, hs_b=None), p.hs_a.shape[-1], p.hs_a.ndim == 3, seed=seed, pin=True)
    assert np.array_equal(q.lo, p.lo)                # the same stages carry planes: the box is the same
    return q.hs_a, q.hs_b


@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "cuda"])
@pytest.mark.parametrize("per_qp", [False, True], ids=["shared", "perqp"])
def test_set_halfspace_continues_as_the_reference_does(gpu, per_qp, on_device):
    case = (6, 3, 3, 9, 70, per_qp, "fuel", 1.6, 1, 18)
    p, kw = host.iter_case(*case)
    a2, b2 = _new_planes(p, 321)
    assert np.abs(a2 - p.hs_a).max() > 0.1
    with _solver(p, **kw) as s:
        s.run(6)
        _, z0, y0 = s.get(w=False)
        if on_device:
            s.set_halfspace(torch.as_tensor(a2, device=DEV), torch.as_tensor(b2, device=DEV))
        else:
            s.set_halfspace(a2, b2)
        a, b = s.halfspace()
        assert np.array_equal(a, a2) and np.array_equal(b, b2)
        _, z1, y1 = s.get(w=False)
        assert np.array_equal(z1, z0) and np.array_equal(y1, y0)         # the state is kept
        s.run(7, residual_every=1)
        w, z, y = s.get()
        r, sd, *_ = s.residuals()
    ref = host.ref_iterates(p, kw, 7, 1, z0=z0, y0=y0, hs=(a2, b2))
    for name, got, want in (("w", w, ref.w), ("z", z, ref.z), ("y", y, ref.y)):
        assert _close(got, want), (name, np.abs(got - want).max())
    assert np.abs(r - ref.r).max() <= TOL and np.abs(sd - ref.s).max() <= TOL
    old = host.ref_iterates(p, kw, 7, 1, z0=z0, y0=y0)
    assert np.abs(old.z - ref.z).max() > 1e-3


@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "cuda"])
@pytest.mark.parametrize("per_qp", [False, True], ids=["shared", "perqp"])
def test_a_refused_set_halfspace_changes_nothing(gpu, per_qp, on_device):
    """A closed box under a newly active stage, a NaN, a wrong form: each is refused, and the handle then gives the bits of a twin
    that never saw the calls."""
    case = (6, 3, 3, 9, 70, per_qp, "box", 1.0, 1, 18)
    p, kw = host.iter_case(*case)
    lib = pkg.load_library()
    conv = (lambda x: torch.as_tensor(np.ascontiguousarray(x), device=DEV)) if on_device else (lambda x: x)
    with _solver(p, **kw) as s, _solver(p, **kw) as twin:
        s.run(4, residual_every=1)
        twin.run(4, residual_every=1)
        # stage 2 has no plane and a closed box: a plane there, for one QP only in the per-QP form
        assert not p.hs_a[..., 2, :].any() and np.isfinite(p.lo[2, p.m:p.m + 3]).any()
        a = p.hs_a.copy()
        a[(-1, 2, 1) if per_qp else (2, 1)] = 0.5
        for bad_a, bad_b, exc, msg in ((a, p.hs_b, (ValueError, pkg.AdmmError), "unbounded"),):
            with pytest.raises(exc, match=msg):
                s.set_halfspace(conv(bad_a), conv(bad_b))
        nan_a, nan_b = p.hs_a.copy(), p.hs_b.copy()
        nan_a[..., 3, 0] = np.nan
        nan_b[..., 4] = INF
        for bad_a, bad_b in ((nan_a, p.hs_b), (p.hs_a, nan_b)):
            with pytest.raises((ValueError, pkg.AdmmError), match="finite"):
                s.set_halfspace(conv(bad_a), conv(bad_b))
        other_a = np.array(np.broadcast_to(p.hs_a, (p.batch, p.N, 3))) if not per_qp else p.hs_a[0]
        other_b = np.array(np.broadcast_to(p.hs_b, (p.batch, p.N))) if not per_qp else p.hs_b[0]
        with pytest.raises(ValueError, match="shape"):
            s.set_halfspace(conv(other_a), conv(other_b))
        with pytest.raises(ValueError, match="shape"):
            s.set_halfspace(conv(p.hs_a[..., :2]), conv(p.hs_b))             # another nh
        # the library itself refuses the first two (the wrapper's checks aside), before anything is written
        if on_device:
            ta, tb = conv(a), conv(p.hs_b)
            rc_ = lib.admm_set_halfspace_device(s._h, C.cast(C.c_void_p(ta.data_ptr()), _abi.c_double_p),
                                                C.cast(C.c_void_p(tb.data_ptr()), _abi.c_double_p), pkg.solver._stream(DEV))
        else:
            rc_ = lib.admm_set_halfspace(s._h, _abi.dptr(np.ascontiguousarray(a)), _abi.dptr(np.ascontiguousarray(p.hs_b)))
        assert rc_ == INVALID and "unbounded" in lib.admm_last_error().decode() and "stage 2" in lib.admm_last_error().decode()
        if not on_device:
            assert lib.admm_set_halfspace(s._h, _abi.dptr(np.ascontiguousarray(nan_a)), _abi.dptr(np.ascontiguousarray(p.hs_b))) == INVALID
            assert "non-finite" in lib.admm_last_error().decode()
        ha, hb = s.halfspace()
        assert np.array_equal(ha, p.hs_a) and np.array_equal(hb, p.hs_b)
        assert _same(_state(s), _state(twin))
        s.iterate(5)
        twin.iterate(5)
        assert _same(s.get(), twin.get())


# ---- 7. update_problem ----

def test_update_problem_keeps_the_planes_and_rechecks_the_rule(gpu):
    case = (6, 3, 3, 9, 70, True, "thrust", 1.0, 1, 18)
    p, kw = host.iter_case(*case)
    p2 = dataclasses.replace(p, Q=1.5 * p.Q, x0=0.5 * p.x0, hs_a=None, hs_b=None)
    with _solver(p, **kw) as s, _solver(p, **kw) as twin:
        s.run(5)
        twin.run(5)
        _, z0, y0 = s.get(w=False)
        closed = dataclasses.replace(p2, lo=p2.lo.copy())
        closed.lo[0, p.m + 2] = -3.0                     # stage 0 carries a plane for every QP
        with pytest.raises((ValueError, pkg.AdmmError), match="unbounded"):
            s.update_problem(closed)
        lib = pkg.load_library()
        cp, keep = _abi.marshal_problem(closed)
        assert lib.admm_update_problem(s._h, C.byref(cp)) == INVALID and "unbounded" in lib.admm_last_error().decode()
        s.iterate(2)
        twin.iterate(2)
        assert _same(s.get(), twin.get())                # the refused update changed nothing
        _, z0, y0 = s.get(w=False)
        s.update_problem(p2)
        a, b = s.halfspace()
        assert np.array_equal(a, p.hs_a) and np.array_equal(b, p.hs_b) and np.array_equal(s.problem.hs_a, p.hs_a)
        s.run(6, residual_every=1)
        w, z, y = s.get()
    ref = host.ref_iterates(dataclasses.replace(p2, hs_a=p.hs_a, hs_b=p.hs_b), kw, 6, 1, z0=z0, y0=y0)
    for name, got, want in (("w", w, ref.w), ("z", z, ref.z), ("y", y, ref.y)):
        assert _close(got, want), (name, np.abs(got - want).max())


# ---- 8. set_rho and graph replay ----

@pytest.mark.parametrize("per_qp", [False, True], ids=["shared", "perqp"])
def test_set_rho_and_graph_replay_give_the_bits_of_direct_launches(gpu, per_qp):
    case = (6, 3, 3, 9, 70, per_qp, "fuel", 1.6, 1, 18)
    p, kw = host.iter_case(*case)
    a2, b2 = _new_planes(p, 99)
    out = []
    for flags in (0, _abi.FLAG_GRAPH):
        with _solver(p, flags=flags, **kw) as s:
            s.run(7, residual_every=2)
            s.set_halfspace(a2, b2)                      # the planes change under the captured graph, at the same addresses
            s.run(5, residual_every=2)
            s.set_rho(2 * RHO)
            s.run(6, residual_every=3)
            out.append(_state(s) + (s.halfspace_report(multipliers=True).lam,))
    assert _same(*out)
    # ... and set_rho is the reference's rescale: y (rho / rho_new), a new factor, the planes untouched
    ref = host.ref_iterates(p, kw, 7, 2)
    ref = host.ref_iterates(p, kw, 5, 2, z0=ref.z, y0=ref.y, hs=(a2, b2))
    kw2 = dict(kw, rho=2 * RHO)
    ref = host.ref_iterates(p, kw2, 6, 3, z0=ref.z, y0=ref.y * 0.5, hs=(a2, b2))
    for got, want in zip(out[0][:3], (ref.w, ref.z, ref.y)):
        assert _close(got, want), np.abs(got - want).max()


# ---- 9. refusals on such a handle ----

def test_calls_without_a_halfspace_form_are_refused_with_a_reason(gpu):
    p, kw = host.iter_case(6, 3, 3, 9, 3, True, "box", 1.0, 1, 18)
    lib = pkg.load_library()
    with _solver(p, **kw) as s, _solver(p, **kw) as twin:
        s.run(3)
        twin.run(3)
        with pytest.raises(pkg.AdmmError, match="window-relative") as e:
            s.mpc_advance()
        assert e.value.code == UNSUPPORTED
        with pytest.raises(pkg.AdmmError, match="window-relative") as e:
            s.mpc_advance(dx=torch.zeros((p.batch, p.n), dtype=torch.float64, device=DEV))
        assert e.value.code == UNSUPPORTED
        with pytest.raises(pkg.AdmmError, match="Farkas") as e:
            s.infeasibility()
        assert e.value.code == UNSUPPORTED
        out = np.zeros(16)
        assert lib.admm_profile(s._h, 2, 1, 1, _abi.dptr(out)) == UNSUPPORTED and b"unfused path only" in lib.admm_last_error()
        assert lib.admm_profile(s._h, 2, 1, 0, _abi.dptr(out)) == 0
        twin.run(2, residual_every=1)                    # (profile mode 0 runs its iterations on the handle)
        cert = s.certificate()
        assert np.isfinite(cert.obj).all() and np.isfinite(cert.stat).all()
    with pytest.raises(ValueError, match="device-memory"):
        pkg.Solver(pkg.DeviceProblem.from_problem(p, DEV), pkg.Options(**kw))


# ---- 10. the example ----

def test_the_example_keeps_out_after_four_passes(gpu):
    spec = importlib.util.spec_from_file_location("keepout_rendezvous", os.path.join(host.ROOT, "examples", "keepout_rendezvous.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    for fuel in (None, 2.0 * np.pi / 40):
        radius, rows = ex.run(N=40, batch=6, passes=4, fuel=fuel, verbose=False)
        closest, n_active, iters, nconv, ms = rows[-1]
        print(fuel, closest / radius, n_active, [r[2] for r in rows])
        assert (closest >= radius * (1.0 - 1e-3)).all(), closest / radius
        assert (rows[0][0] / radius).min() < 1.5 and (n_active >= 1).all()
