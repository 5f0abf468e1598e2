"""One approach cone per stage on the GPU (csrc/admm_cone_kernels.hpp) against tests/_cone_ref.py -- the oracle's loop
with the projection onto the cone (tests/test_cone_host.py checks that reference on the CPU, holds the cases, and asserts that every
case meets, over its batch and its 30 iterations, every branch of the projection that can occur at its nh).

Shapes are chosen for the kernel's geometry (one lane = two adjacent QPs, 512 columns per workgroup, chunks of whole blocks):
batches 1 and 3 (odd: a pad column beside the last QP), 70 (pad columns) and 514 (two workgroups along the batch); chunks of two to
ten blocks with a shorter last one, and a single chunk."""
import ctypes as C
import dataclasses
import importlib.util
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded, as in tests/test_gpu_device_io.py)

import admm_library_amd as pkg
import _cone_ref as cr
import _readout_cases as rc
import test_cone_host as host
from admm_library_amd import _abi

pytestmark = pytest.mark.gpu
TOL = 1e-10            # x max(1, |.|): the project's iterate tolerance
INVALID, UNSUPPORTED = 1, 2
INF = np.inf
DEV = "cuda:0"
RHO = host.RHO
FIELDS = host.FIELDS


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


def _payload(p):
    return tuple(getattr(p, f) for f in FIELDS)


def _no_cones(p):
    return dataclasses.replace(p, cone_c=None, cone_p=None, cone_g=None)


# ---- 1. iterates and residuals against the reference ----

@pytest.mark.parametrize("case", host.ITER_CASES, ids=host.ITER_IDS)
def test_iterates_match_the_reference(gpu, case):
    n, m, nh, N, batch, per_qp, kind, alpha, every, zrows = case
    p, kw = host.iter_case(*case)
    with _solver(p, **kw) as s:
        geo = s.geometry()
        assert geo["zrows"] % p.nb == 0
        assert geo["zrows"] == zrows and (geo["zchunks"] == 1 if zrows == p.L else geo["zchunks"] > 1), geo
        got = s.cone()
        assert all(np.array_equal(a, b) for a, b in zip(got, _payload(p))) and got[0].ndim == (3 if per_qp else 2)
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
    # the cones matter: the problem without them iterates elsewhere
    plain = host.ref_iterates(dataclasses.replace(p, cone_c=np.zeros_like(p.cone_c)), kw, host.ITER_STEPS[-1], every)
    assert np.abs(plain.z - ref.z).max() > 1e-3


# ---- 2. all-zero axes are the unfused path, bit for bit ----

@pytest.mark.parametrize("per_qp", [False, True], ids=["shared", "perqp"])
@pytest.mark.parametrize("alpha", [1.0, 1.6])
@pytest.mark.parametrize("kind", ["box", "thrust", "fuel"])
def test_zero_axes_are_the_unfused_handle_bit_for_bit(gpu, kind, alpha, per_qp):
    """zdual_kernel (box) / zdual_soc_kernel (thrust, fuel) against zdual_cone_kernel with c = 0 everywhere (apex and slope
    arbitrary), residuals included.  Both handles get two blocks per chunk: the residual sums are added chunk by chunk."""
    batch = 70
    p = pkg.random_ltv(N=9, n=6, m=3, batch=batch, seed=77, thrust_norm=kind != "box")
    if kind == "fuel":
        p = rc.stage_fuel(p)
    cnt = (batch,) if per_qp else ()
    rng = np.random.default_rng(3)
    pc = dataclasses.replace(p, cone_c=np.zeros(cnt + (p.N, 3)), cone_p=rng.standard_normal(cnt + (p.N, 3)),
                             cone_g=rng.uniform(0.2, 3.0, cnt + (p.N,)))
    kw = dict(rho=RHO, alpha=alpha, zrows=2 * p.nb)
    out = []
    with pkg.Solver(p, pkg.Options(flags=_abi.FLAG_UNFUSED, **kw)) as plain, _solver(pc, **kw) as s:
        assert plain.geometry() == s.geometry()
        for h in (plain, s):
            h.run(9, residual_every=3)
            out.append(_state(h))
        rep = s.cone_report(multipliers=True)
    assert _same(*out)
    assert not rep.max_violation.any() and not rep.n_active.any() and not rep.lam.any()


# ---- 3. the edges, bit for bit ----

@pytest.fixture(scope="module")
def prox_host(tmp_path_factory):
    return host.build_prox_host(tmp_path_factory.mktemp("cone_gpu"))


@pytest.mark.parametrize("n,m,nh,per_qp", [(6, 3, 3, True), (6, 3, 6, False), (4, 2, 2, True), (2, 1, 1, True), (6, 3, 2, False)])
def test_edges_bit_for_bit(gpu, prox_host, n, m, nh, per_qp):
    """The state is set so that v = w + y is exactly the wanted point (y = 0, alpha = 1), then one step_z: the rows under a cone
    get the bits of csrc/admm_prox.hpp compiled on the host -- v on the axis, v = apex, r = g s and g r = -s exactly and one
    rounding of g either side, c with zero entries, nh = n, c = 0 -- and every other row its box."""
    rng = np.random.default_rng(60 + nh)
    c_e, a_e, g_e, v_e = host.edge_stages(nh, rng)
    g_e = np.where(c_e.any(axis=1), g_e, 1.0)
    E = c_e.shape[0]
    batch = 67 if per_qp else 3
    N = E if not per_qp else 7
    p = pkg.random_ltv(N=N, n=n, m=m, batch=batch, seed=9, state_bounds=True)
    lo, hi = p.lo.copy(), p.hi.copy()
    lo[:, m:m + nh], hi[:, m:m + nh] = -INF, INF
    if per_qp:                       # QP b, stage k carries edge (5 b + 3 k) % E: every edge occurs
        idx = (5 * np.arange(batch)[:, None] + 3 * np.arange(N)[None]) % E
        assert len(set(idx.ravel())) == E
        c, a, g, vx = c_e[idx], a_e[idx], g_e[idx], v_e[idx]
    else:                            # stage k carries edge k, every QP a different point: QP 0 the edge's, the others random
        c, a, g = c_e, a_e, g_e
        vx = np.stack([v_e] + [v_e + rng.standard_normal(v_e.shape) for _ in range(batch - 1)])
    pc = dataclasses.replace(p, lo=lo, hi=hi, cone_c=c, cone_p=a, cone_g=g)
    pc.validate()
    v = rng.uniform(-4.0, 4.0, (batch, N, p.nb))
    v[:, :, m:m + nh] = vx
    C_, Pa, G = cr.cones(pc)
    zx, yx, br = prox_host(C_.reshape(-1, nh), Pa.reshape(-1, nh), G.reshape(-1), np.ascontiguousarray(v[:, :, m:m + nh]).reshape(-1, nh))
    assert set(br) == ({-1, 0, 1} if nh == 1 else {-1, 0, 1, 2})
    want = np.minimum(np.maximum(v, lo[None]), hi[None])
    want[:, :, m:m + nh] = zx.reshape(batch, N, nh)
    v = v.reshape(batch, -1)
    want = want.reshape(batch, -1)
    with _solver(pc, rho=RHO, zrows=2 * p.nb) as s:
        s.set_state(w=v, z=np.zeros_like(v), y=np.zeros_like(v))
        s.step_z()
        _, z, y = s.get(w=False)
    assert np.array_equal(z, want)
    assert np.array_equal(y, v - want)
    inside = (br == 0).reshape(batch, N)
    yb = y.reshape(batch, N, p.nb)[:, :, m:m + nh]
    assert not yb[inside].any() and not np.signbit(yb[inside]).any()          # inside: the bits of v, y = +0


# ---- 4. a solve with adaptive rho ----

def test_solve_follows_the_reference_and_meets_the_optimality_conditions(gpu):
    """cw_approach(N = 40, batch 6) to eps = 1e-7 with the adaptive rule (720 iterations in the reference, rho 0.5 -> 1).  Every
    quantity of the optimality conditions is bounded by ten times what the reference's own solution of the same case has
    (a bound of ten times a quantity that is a few roundings in the reference is a bound of a few tens of roundings):
        reference   feas_dyn 2.767e-6   stat 1.544e-7   feas_cone 1.9e-17   polar 4.9e-17   comp 1.4e-17
        handle      feas_dyn 2.767e-6   stat 1.544e-7   feas_cone 7.5e-17   polar 6.0e-18   comp 4.2e-17"""
    p = host.solve_problem()
    dec = []
    ref = cr.solve(p, decisions=dec, **host.SOLVE_OPTS)
    cref = cr.conditions(p, ref.z, ref.y, ref.rho)
    names = ("feas_dyn", "stat", "feas_cone", "polar", "comp")
    bounds = {name: 10.0 * float(cref[name].max()) for name in names}
    with _solver(p, flags=_abi.FLAG_HISTORY, **host.SOLVE_OPTS) as s:
        info = s.solve()
        _, z, y = s.get(w=False)
        hist = s.history()
        rep = s.cone_report()
    assert info.iters_run == ref.iters_run and info.rho == ref.rho and info.rho_updates == ref.rho_updates
    assert np.array_equal(info.status, ref.status) and np.array_equal(info.iters, ref.iters) and info.status.all()
    assert len(hist["iteration"]) == ref.iters_run // host.SOLVE_OPTS["check_interval"]
    for it, rho in zip(hist["iteration"], hist["rho"]):       # rho in force at a test = the last decision before it
        prev = [r for i, r in dec if i < it]
        assert rho == (prev[-1] if prev else host.SOLVE_OPTS["rho"]), (it, rho)
    c = cr.conditions(p, z, y, info.rho)
    for name, bnd in bounds.items():
        print(name, c[name].max(), "reference", cref[name].max(), "bound", bnd)
    for name, bnd in bounds.items():
        assert c[name].max() <= bnd, (name, c[name].max(), bnd)
    assert np.array_equal(c["n_active"], cref["n_active"]) and np.array_equal(rep.n_active, cref["n_active"])
    assert _close(z, ref.z, 1e-8)


# ---- 5. the report ----

@pytest.mark.parametrize("per_qp", [False, True], ids=["shared", "perqp"])
def test_report_matches_numpy_on_the_handles_state(gpu, per_qp):
    case = (6, 3, 3, 12, 70, per_qp, "thrust", 1.6, 1, 18)
    p, kw = host.iter_case(*case)
    with _solver(p, **kw) as s, _solver(p, **kw) as twin:
        s.run(12)
        twin.run(12)
        w, _, y = s.get()
        rep = s.cone_report(multipliers=True)
        dev = s.cone_report(multipliers=True, device=True)
        torch.cuda.synchronize()
        mx, cnt, lam = cr.report(p, w, y, RHO)
        assert (mx > 0).any() and (cnt > 0).all() and (cnt < p.N).all() and (lam == 0).any() and (lam > 0).any()
        assert rep.n_active.dtype == np.int32 and np.array_equal(rep.n_active, cnt)
        assert np.abs(rep.max_violation - mx).max() <= 1e-12 * max(1.0, np.abs(mx).max())
        assert np.abs(rep.lam - lam).max() <= 1e-12 * np.abs(lam).max()
        assert rep.lam.shape == (p.batch, p.N)
        for name in ("max_violation", "n_active", "lam"):
            assert np.array_equal(getattr(dev, name).cpu().numpy(), getattr(rep, name)), name
        assert dev.n_active.dtype == torch.int32
        # any pointer may be NULL, and repeating the call gives the same bits
        lib, one = pkg.load_library(), np.zeros(p.batch)
        assert lib.admm_get_cone_report(s._h, _abi.dptr(one), None, None) == 0 and np.array_equal(one, rep.max_violation)
        again = s.cone_report(multipliers=True)
        assert np.array_equal(again.lam, rep.lam) and np.array_equal(again.max_violation, rep.max_violation)
        assert lib.admm_get_cone_report(s._h, None, None, None) == INVALID and b"at least one" in lib.admm_last_error()
        # reading changes nothing
        s.run(3, residual_every=1)
        twin.run(3, residual_every=1)
        assert _same(_state(s), _state(twin))
    with pkg.Solver(_no_cones(p), pkg.Options(rho=RHO)) as plain:
        hostv = np.zeros(p.batch * p.N * 3)
        assert lib.admm_get_cone_report(plain._h, _abi.dptr(hostv), None, None) == INVALID and b"no approach cones" in lib.admm_last_error()
        assert lib.admm_set_cone(plain._h, _abi.dptr(hostv), _abi.dptr(hostv), _abi.dptr(hostv)) == INVALID
        assert b"cannot be added" in lib.admm_last_error()
        with pytest.raises(pkg.AdmmError):
            plain.cone()


# ---- 6. set_cone ----

def _new_cones(p, seed):
    q = host.random_cones(_no_cones(p), p.cone_c.shape[-1], p.cone_c.ndim == 3, seed=seed)
    assert np.array_equal(q.lo, p.lo)                # the same stages carry cones: the box is the same
    return _payload(q)


@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "cuda"])
@pytest.mark.parametrize("per_qp", [False, True], ids=["shared", "perqp"])
def test_set_cone_continues_as_the_reference_does(gpu, per_qp, on_device):
    case = (6, 3, 3, 12, 70, per_qp, "fuel", 1.6, 1, 18)
    p, kw = host.iter_case(*case)
    new = _new_cones(p, 321)
    assert np.abs(new[0] - p.cone_c).max() > 0.1
    with _solver(p, **kw) as s:
        s.run(6)
        _, z0, y0 = s.get(w=False)
        if on_device:
            s.set_cone(*(torch.as_tensor(x, device=DEV) for x in new))
        else:
            s.set_cone(*new)
        assert all(np.array_equal(a, b) for a, b in zip(s.cone(), new))
        _, z1, y1 = s.get(w=False)
        assert np.array_equal(z1, z0) and np.array_equal(y1, y0)         # the state is kept
        s.run(7, residual_every=1)
        w, z, y = s.get()
        r, sd, *_ = s.residuals()
    ref = host.ref_iterates(p, kw, 7, 1, z0=z0, y0=y0, cone=new)
    for name, got, want in (("w", w, ref.w), ("z", z, ref.z), ("y", y, ref.y)):
        assert _close(got, want), (name, np.abs(got - want).max())
    assert np.abs(r - ref.r).max() <= TOL and np.abs(sd - ref.s).max() <= TOL
    old = host.ref_iterates(p, kw, 7, 1, z0=z0, y0=y0)
    assert np.abs(old.z - ref.z).max() > 1e-3


@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "cuda"])
@pytest.mark.parametrize("per_qp", [False, True], ids=["shared", "perqp"])
def test_a_refused_set_cone_changes_nothing(gpu, per_qp, on_device):
    """A closed box under a newly coned stage, a NaN, a slope <= 0, a wrong form: each is refused, and the handle then gives the bits
    of a twin that never saw the calls."""
    case = (6, 3, 3, 12, 70, per_qp, "box", 1.0, 1, 18)
    p, kw = host.iter_case(*case)
    lib = pkg.load_library()
    conv = (lambda x: torch.as_tensor(np.ascontiguousarray(x), device=DEV)) if on_device else (lambda x: x)
    c0, a0, g0 = _payload(p)

    def raw(c, a, g):
        if on_device:
            t = [conv(x) for x in (c, a, g)]
            return lib.admm_set_cone_device(s._h, *(C.cast(C.c_void_p(x.data_ptr()), _abi.c_double_p) for x in t), pkg.solver._stream(DEV))
        return lib.admm_set_cone(s._h, *(_abi.dptr(np.ascontiguousarray(x)) for x in (c, a, g)))
    with _solver(p, **kw) as s, _solver(p, **kw) as twin:
        s.run(4, residual_every=1)
        twin.run(4, residual_every=1)
        # stage 2 has no cone and a closed box: a cone there, for one QP only in the per-QP form
        assert not c0[..., 2, :].any() and np.isfinite(p.lo[2, p.m:p.m + 3]).any()
        c = c0.copy()
        c[(-1, 2, 1) if per_qp else (2, 1)] = 0.5
        with pytest.raises((ValueError, pkg.AdmmError), match="unbounded"):
            s.set_cone(conv(c), conv(a0), conv(g0))
        nan_c, nan_a, nan_g = c0.copy(), a0.copy(), g0.copy()
        nan_c[..., 3, 0] = np.nan
        nan_a[..., 4, 1] = INF
        nan_g[..., 5] = np.nan
        for bad in ((nan_c, a0, g0), (c0, nan_a, g0), (c0, a0, nan_g)):
            with pytest.raises((ValueError, pkg.AdmmError), match="finite"):
                s.set_cone(*(conv(x) for x in bad))
        for slope in (0.0, -1.0):
            g = g0.copy()
            g[(-1, 3) if per_qp else (3,)] = slope           # stage 3 carries a cone
            with pytest.raises((ValueError, pkg.AdmmError), match="slope|gamma"):
                s.set_cone(conv(c0), conv(a0), conv(g))
            assert raw(c0, a0, g) == INVALID and "gamma of stage 3 must be a positive normal number" in lib.admm_last_error().decode()
        other = [np.array(np.broadcast_to(x, (p.batch,) + x.shape)) if not per_qp else x[0] for x in (c0, a0, g0)]
        with pytest.raises(ValueError, match="shape"):
            s.set_cone(*(conv(x) for x in other))
        with pytest.raises(ValueError, match="shape"):
            s.set_cone(conv(c0[..., :2]), conv(a0[..., :2]), conv(g0))           # another nh
        # the library itself refuses them (the wrapper's checks aside), before anything is written
        assert raw(c, a0, g0) == INVALID
        assert "unbounded" in lib.admm_last_error().decode() and "stage 2" in lib.admm_last_error().decode()
        assert raw(nan_c, a0, g0) == INVALID and "non-finite" in lib.admm_last_error().decode()
        assert raw(c0, a0, nan_g) == INVALID and "non-finite" in lib.admm_last_error().decode()
        tiny = c0.copy()
        tiny[(-1, 3) if per_qp else (3,)] = (1e-170, 0.0, 0.0)
        assert raw(tiny, a0, g0) == INVALID and "c'c of stage 3 is not a normal number" in lib.admm_last_error().decode()
        assert all(np.array_equal(a, b) for a, b in zip(s.cone(), (c0, a0, g0)))
        assert _same(_state(s), _state(twin))
        s.iterate(5)
        twin.iterate(5)
        assert _same(s.get(), twin.get())


def test_device_form_checks_its_pointers(gpu):
    lib = pkg.load_library()
    p, kw = host.iter_case(6, 3, 3, 12, 70, True, "box", 1.0, 1, 18)

    def dp(t, typ=_abi.c_double_p, off=0):
        return C.cast(C.c_void_p(t.data_ptr() + off), typ)
    with _solver(p, **kw) as s:
        s.run(5)
        ref = s.cone_report(multipliers=True)
        t = torch.zeros(p.batch + 1, dtype=torch.float64, device=DEV)
        ti = torch.zeros(p.batch + 1, dtype=torch.int32, device=DEV)
        tl = torch.zeros(p.batch * p.N, dtype=torch.float64, device=DEV)
        st = pkg.solver._stream(DEV)
        assert lib.admm_get_cone_report_device(s._h, dp(t[1:]), dp(ti[1:], _abi.c_int32_p), dp(tl), st) == 0
        torch.cuda.synchronize()
        assert np.array_equal(t[1:].cpu().numpy(), ref.max_violation) and t[0] == 0
        assert np.array_equal(ti[1:].cpu().numpy(), ref.n_active) and ti[0] == 0
        assert np.array_equal(tl.cpu().numpy().reshape(p.batch, p.N), ref.lam)
        hostv = np.zeros(p.batch)
        assert lib.admm_get_cone_report_device(s._h, _abi.dptr(hostv), None, None, None) == INVALID
        assert "admm_get_cone_report_device: max_violation is not device memory" in lib.admm_last_error().decode()
        assert lib.admm_get_cone_report_device(s._h, None, dp(ti, _abi.c_int32_p, off=2), None, None) == INVALID
        assert "n_active is not 4-byte aligned" in lib.admm_last_error().decode()
        assert lib.admm_get_cone_report_device(s._h, None, None, None, None) == INVALID and b"at least one" in lib.admm_last_error()
        c, a, g = (torch.as_tensor(x, device=DEV) for x in _payload(p))
        assert lib.admm_set_cone_device(s._h, _abi.dptr(np.ascontiguousarray(p.cone_c)), dp(a), dp(g), None) == INVALID
        assert "admm_set_cone_device: c is not device memory" in lib.admm_last_error().decode()
        assert lib.admm_set_cone_device(s._h, dp(c), dp(a), dp(g, off=4), None) == INVALID
        assert "gamma is not 8-byte aligned" in lib.admm_last_error().decode()
        big = torch.zeros(3 * 2 ** 20, dtype=torch.float64, device=DEV)      # a block of its own in torch's allocator: its true end is known
        short = big[big.numel() - (p.batch * p.N * 3 - 1):]
        assert lib.admm_set_cone_device(s._h, dp(c), dp(short), dp(g), None) == INVALID and "apex ends before" in lib.admm_last_error().decode()
        assert all(np.array_equal(x, y) for x, y in zip(s.cone(), _payload(p)))


# ---- 7. update_problem ----

def test_update_problem_keeps_the_cones_and_rechecks_the_rule(gpu):
    case = (6, 3, 3, 12, 70, True, "thrust", 1.0, 1, 18)
    p, kw = host.iter_case(*case)
    p2 = _no_cones(dataclasses.replace(p, Q=1.5 * p.Q, x0=0.5 * p.x0))
    with _solver(p, **kw) as s, _solver(p, **kw) as twin:
        s.run(5)
        twin.run(5)
        closed = dataclasses.replace(p2, lo=p2.lo.copy())
        closed.lo[0, p.m + 2] = -3.0                     # stage 0 carries a cone for every QP
        with pytest.raises((ValueError, pkg.AdmmError), match="unbounded"):
            s.update_problem(closed)
        lib = pkg.load_library()
        cp, keep = _abi.marshal_problem(closed)
        assert lib.admm_update_problem(s._h, C.byref(cp)) == INVALID
        assert "at a stage with a cone (stage 0)" in lib.admm_last_error().decode()
        s.iterate(2)
        twin.iterate(2)
        assert _same(s.get(), twin.get())                # the refused update changed nothing
        _, z0, y0 = s.get(w=False)
        s.update_problem(p2)
        assert all(np.array_equal(a, b) for a, b in zip(s.cone(), _payload(p))) and np.array_equal(s.problem.cone_c, p.cone_c)
        s.run(6, residual_every=1)
        w, z, y = s.get()
    ref = host.ref_iterates(dataclasses.replace(p2, cone_c=p.cone_c, cone_p=p.cone_p, cone_g=p.cone_g), kw, 6, 1, z0=z0, y0=y0)
    for name, got, want in (("w", w, ref.w), ("z", z, ref.z), ("y", y, ref.y)):
        assert _close(got, want), (name, np.abs(got - want).max())


# ---- 8. set_rho and graph replay ----

@pytest.mark.parametrize("per_qp", [False, True], ids=["shared", "perqp"])
def test_set_rho_and_graph_replay_give_the_bits_of_direct_launches(gpu, per_qp):
    case = (6, 3, 3, 12, 70, per_qp, "fuel", 1.6, 1, 18)
    p, kw = host.iter_case(*case)
    new = _new_cones(p, 99)
    out = []
    for flags in (0, _abi.FLAG_GRAPH):
        with _solver(p, flags=flags, **kw) as s:
            s.run(7, residual_every=2)
            s.set_cone(*new)                             # the cones change under the captured graph, at the same addresses
            s.run(5, residual_every=2)
            s.set_rho(2 * RHO)
            s.run(6, residual_every=3)
            out.append(_state(s) + (s.cone_report(multipliers=True).lam,))
    assert _same(*out)
    # ... and set_rho is the reference's rescale: y (rho / rho_new), a new factor, the cones untouched
    ref = host.ref_iterates(p, kw, 7, 2)
    ref = host.ref_iterates(p, kw, 5, 2, z0=ref.z, y0=ref.y, cone=new)
    kw2 = dict(kw, rho=2 * RHO)
    ref = host.ref_iterates(p, kw2, 6, 3, z0=ref.z, y0=ref.y * 0.5, cone=new)
    for got, want in zip(out[0][:3], (ref.w, ref.z, ref.y)):
        assert _close(got, want), np.abs(got - want).max()


# ---- 9. refusals on such a handle ----

def test_calls_without_a_cone_form_are_refused_with_their_table_sentences(gpu):
    p, kw = host.iter_case(6, 3, 3, 12, 3, True, "box", 1.0, 1, 27)
    lib = pkg.load_library()
    on = "not available on a handle with approach cones ("
    step_why = on + "a per-QP cone is not window-relative: it would have to shift with the horizon)"
    probe_why = on + "the Farkas certificate is written for boxes and the thrust ball)"

    def refused(rc_, status, message):
        assert (rc_, lib.admm_last_error().decode()) == (status, message)

    def tptr(t, ctype=_abi.c_double_p):
        return C.cast(C.c_void_p(t.data_ptr()), ctype)
    with _solver(p, **kw) as s, _solver(p, **kw) as twin:
        s.run(3)
        twin.run(3)
        h = s._h
        with pytest.raises(pkg.AdmmError, match="window-relative") as e:
            s.mpc_advance()
        assert e.value.code == UNSUPPORTED
        with pytest.raises(pkg.AdmmError, match="Farkas") as e:
            s.infeasibility()
        assert e.value.code == UNSUPPORTED
        step = _abi.CMpcStep(tail=_abi.MPC_TAILS["copy"], reserved=0)
        u, x = np.zeros((p.batch, p.m)), np.zeros((p.batch, p.n))
        tu, tx = (torch.zeros(v.shape, dtype=torch.float64, device=DEV) for v in (u, x))
        refused(lib.admm_mpc_advance(h, C.byref(step), _abi.dptr(u), _abi.dptr(x)), UNSUPPORTED, "admm_mpc_advance: " + step_why)
        refused(lib.admm_mpc_advance_device(h, C.byref(step), tptr(tu), tptr(tx), None), UNSUPPORTED, "admm_mpc_advance_device: " + step_why)
        sep, drift, defect, flag = np.zeros(p.batch), np.zeros(p.batch), np.zeros(p.batch), np.zeros(p.batch, np.int32)
        refused(lib.admm_probe_infeasibility(h, 4, 1e-6, _abi.dptr(sep), _abi.dptr(drift), _abi.dptr(defect), _abi.iptr(flag), None),
                UNSUPPORTED, "admm_probe_infeasibility: " + probe_why)
        ta, tb, tc = (torch.zeros(p.batch, dtype=torch.float64, device=DEV) for _ in range(3))
        tf = torch.zeros(p.batch, dtype=torch.int32, device=DEV)
        refused(lib.admm_probe_infeasibility_device(h, 4, 1e-6, tptr(ta), tptr(tb), tptr(tc), tptr(tf, _abi.c_int32_p), None, None),
                UNSUPPORTED, "admm_probe_infeasibility_device: " + probe_why)
        out = np.zeros(16)
        for fused_path in (1, 2, 3, 4):
            refused(lib.admm_profile(h, 2, 1, fused_path, _abi.dptr(out)), UNSUPPORTED,
                    "admm_profile: a handle with approach cones runs the unfused path only (fused_path = 0)")
        assert _same(s.get(), twin.get())                # the refusals changed nothing
        assert lib.admm_profile(h, 2, 1, 0, _abi.dptr(out)) == 0
        cert = s.certificate()
        assert np.isfinite(cert.obj).all() and np.isfinite(cert.stat).all()
    with pytest.raises(ValueError, match="device-memory"):
        pkg.Solver(pkg.DeviceProblem.from_problem(p, DEV), pkg.Options(**kw))


# ---- 10. the example ----

def test_the_example_stays_inside_its_cones(gpu):
    spec = importlib.util.spec_from_file_location("approach_cone_rendezvous", os.path.join(host.ROOT, "examples", "approach_cone_rendezvous.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    rows = ex.run(N=40, batch=6, verbose=False)
    assert [r["workload"] for r in rows] == ["box", "fuel"]
    for r in rows:
        print(r["workload"], r["iters"], r["n_active"], r["max_violation"], r["angle"], r["half_angle"])
        assert r["status"].all() and (r["max_violation"] <= 1e-12).all()
        assert (r["angle"] <= r["half_angle"] * (1.0 + 1e-9)).all()
    assert (rows[0]["n_active"] >= 1).all()
