"""Receding-horizon step on the device (ADMM_HIP_HAS_MPC) against its defining property: admm_mpc_advance on one
handle equals, bit for bit in the state and in every later iterate, the host route -- get, a NumPy shift, update_instances,
set_state -- on a twin handle built from the same problem and options, given the same x+.  The shapes sit where the chunking and
the lanes can go wrong: N = 1, 2, 3 and horizons a forced chunk count does not divide (ADMM_MPC_CHUNKS), batches around the wave
of 64, the three headline (n, m)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import admm_library_amd as pkg
from admm_library_amd import _abi
from admm_library_amd.mpc import plant_step, shift_horizon

import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CODE = {v: k for k, v in _abi.STATUS_NAMES.items()}
U = 2.0 ** -53


def _pre(s, how):
    if how == "run7":
        s.run(7, 0)
    elif how == "run8":
        s.run(8, 1)
    elif how == "solve":
        s.solve()
    else:
        assert how == "fresh"


def _host_route(s, q, xn, tail, q_tail=None):
    """The defining sequence on handle s; q: the problem's current linear term (or None).  Returns (w, z, y) before the shift and q'."""
    nb = s.problem.nb
    w, z, y = s.get()
    q2 = None if q is None else shift_horizon(q, nb, tail, q_tail)
    s.update_instances(xn, q2)
    s.set_state(shift_horizon(w, nb, tail), shift_horizon(z, nb, tail), shift_horizon(y, nb, tail))
    return (w, z, y), q2


def _same(a, b, what):
    for name, x, y in zip("wzy", a.get(), b.get()):
        assert np.array_equal(x, y), (what, name, float(np.abs(x - y).max()))


def _noise(p, seed):
    rng = np.random.default_rng(seed)
    return 1e-2 * rng.standard_normal((p.batch, p.m)), 1e-2 * rng.standard_normal((p.batch, p.n))


def _step_against_twin(p, opt, pre, tail="copy", chunks=None, q_tail=None, monkeypatch=None, runs=(5, 1)):
    du, dx = _noise(p, 5)
    with pkg.Solver(p, pkg.Options(**opt)) as s, pkg.Solver(p, pkg.Options(**opt)) as twin:
        _pre(s, pre)
        _pre(twin, pre)
        if chunks is not None:
            monkeypatch.setenv("ADMM_MPC_CHUNKS", str(chunks))
        u, xn = s.mpc_advance(du=du, dx=dx, q_tail=q_tail, tail=tail)
        if chunks is not None:
            monkeypatch.delenv("ADMM_MPC_CHUNKS")
        before, _ = _host_route(twin, p.q, xn, tail, q_tail)
        assert np.array_equal(u, before[1][:, :p.m] + du)
        got = s.get()
        for name, a, b in zip("wzy", got, before):          # ... and directly against the helper
            assert np.array_equal(a, shift_horizon(b, p.nb, tail)), name
        _same(s, twin, "after the step")
        s.run(*runs)
        twin.run(*runs)
        _same(s, twin, "after run")
        for a, b in zip(s.residuals(), twin.residuals()):
            assert np.array_equal(a, b)
        return before


F = _abi
CASES = [
    # name, problem, options, state before the step, tail, forced chunk count
    ("di_N1_b1", lambda: pkg.double_integrator(N=1, batch=1), dict(rho=1.0), "run7", "copy", None),
    ("ltv_6x3_N2_b63_q_chunks2", lambda: pkg.random_ltv(2, 6, 3, 63, seed=11), dict(rho=0.3), "run8", "zero", 2),
    ("ltv_12x6_N3_b64_chunks3", lambda: pkg.random_ltv(3, 12, 6, 64, seed=12, with_q=False), dict(rho=0.3), "run7", "copy", 3),
    ("cw_N7_seg3_b65_solve_chunks3", lambda: pkg.cw_rendezvous(N=7, batch=65), dict(rho=0.05, segments=3, max_iter=200), "solve", "copy", 3),
    ("cw_N40_seg8_b257_run8", lambda: pkg.cw_rendezvous(N=40, batch=257), dict(rho=0.05, segments=8), "run8", "copy", None),
    ("formation_N40_seg8_b65_chunks7", lambda: pkg.cw_formation(N=40, batch=65), dict(rho=0.05, segments=8), "run7", "zero", 7),
    ("di_N40_seg8_b64_fresh", lambda: pkg.double_integrator(N=40, batch=64), dict(rho=1.0, segments=8), "fresh", "copy", None),
    ("di_N7_seg3_b257_chunks7", lambda: pkg.double_integrator(N=7, batch=257), dict(rho=1.0, segments=3), "run8", "zero", 7),
    ("cw_N7_b63_unfused", lambda: pkg.cw_rendezvous(N=7, batch=63), dict(rho=0.05, segments=3, flags=F.FLAG_UNFUSED), "run7", "copy", 2),
    ("cw_N40_b65_no_alternate", lambda: pkg.cw_rendezvous(N=40, batch=65), dict(rho=0.05, segments=8, flags=F.FLAG_NO_ALTERNATE), "run8", "copy", None),
    ("cw_N40_b65_graph", lambda: pkg.cw_rendezvous(N=40, batch=65), dict(rho=0.05, segments=8, flags=F.FLAG_GRAPH), "run8", "zero", None),
    ("cw_N40_b65_thrust_bound_chunks7", lambda: pkg.cw_rendezvous(N=40, batch=65, thrust_norm=True), dict(rho=0.05, segments=8), "run7", "copy", 7),
    ("cw_N40_b3_fuel", lambda: pkg.cw_rendezvous_fuel(N=40, batch=3), dict(rho=0.05), "run8", "copy", None),
    ("cw_N40_b16_fp64_mfma", lambda: pkg.cw_rendezvous(N=40, batch=16), dict(rho=0.05, precision_mode=F.PRECISION_FP64_MFMA), "run8", "copy", 3),
    ("ltv_6x3_N7_b65_tv_stage_bounds_relaxed", lambda: pkg.random_ltv(7, 6, 3, 65, seed=13), dict(rho=0.3, alpha=1.6, segments=3), "run7", "copy", 3),
    ("cw_N40_b1_solve", lambda: pkg.cw_rendezvous(N=40, batch=1), dict(rho=0.05, segments=8, max_iter=300), "solve", "zero", None),
]


@pytest.mark.parametrize("name,make,opt,pre,tail,chunks", CASES, ids=[c[0] for c in CASES])
def test_equals_the_host_route(gpu, monkeypatch, name, make, opt, pre, tail, chunks):
    """1. State after the step, and state and residuals after run(5, 1) on both handles: np.array_equal."""
    _step_against_twin(make(), opt, pre, tail, chunks, monkeypatch=monkeypatch)


def test_outputs(gpu):
    """2. u_applied = z_u,0 + du bit for bit; x_next within the dot-product bound of dx + Ap x0 + Bp u, with the model's plant
    (Ap = Bp = NULL: A_0, B_0 of time-varying dynamics) and with another one; x_meas comes back unchanged."""
    p = pkg.random_ltv(7, 6, 3, 65, seed=21)
    n, m = p.n, p.m
    rng = np.random.default_rng(22)
    other = (np.eye(n) + 0.1 * rng.standard_normal((n, n)), rng.standard_normal((n, m)))
    du, dx = _noise(p, 23)
    for plant, (Ap, Bp) in ((None, (p.A[0], p.B[0])), (other, other)):
        with pkg.Solver(p, pkg.Options(rho=0.3, segments=3)) as s:
            s.run(7, 0)
            z = s.get()[1]
            u, xn = s.mpc_advance(plant=plant, du=du, dx=dx)
            assert np.array_equal(u, z[:, :m] + du)
            ref = plant_step(p.x0, u, Ap, Bp, dx)
            bound = 2 * (n + m + 1) * U * (np.abs(dx) + np.abs(p.x0) @ np.abs(Ap).T + np.abs(u) @ np.abs(Bp).T)
            err = np.abs(xn - ref)
            print("x_next: max err / bound", float((err / bound).max()))
            assert (err <= bound).all()
            u2, _ = s.mpc_advance(plant=plant)                 # no du: the control itself; no dx: the plant alone
            assert np.array_equal(u2, shift_horizon(z, p.nb)[:, :m])
    with pkg.Solver(p, pkg.Options(rho=0.3, segments=3)) as s:
        s.run(7, 0)
        z = s.get()[1]
        xm = rng.standard_normal((p.batch, n))
        u, xn = s.mpc_advance(du=du, x_meas=xm)
        assert np.array_equal(xn, xm) and np.array_equal(u, z[:, :m] + du)


@pytest.mark.parametrize("tail", ["copy", "zero"])
@pytest.mark.parametrize("with_tail", [False, True])
def test_tails_and_q(gpu, monkeypatch, tail, with_tail):
    """3. A handle with q under both tails, with q_tail and without (q's last block then follows the tail): the twin gets the host
    helper's q'; states and later iterates equal bitwise.  Two steps in a row, so that the first step's q is what the second moves."""
    p = pkg.random_ltv(7, 6, 3, 65, seed=31)
    qt = np.random.default_rng(32).standard_normal((p.batch, p.nb)) if with_tail else None
    _step_against_twin(p, dict(rho=0.3, segments=3), "run8", tail, 3, q_tail=qt, monkeypatch=monkeypatch)
    with pkg.Solver(p, pkg.Options(rho=0.3, segments=3)) as s, pkg.Solver(p, pkg.Options(rho=0.3, segments=3)) as twin:
        q = p.q
        for step in range(2):
            s.run(4, 0)
            twin.run(4, 0)
            _, xn = s.mpc_advance(q_tail=qt, tail=tail)
            _, q = _host_route(twin, q, xn, tail, qt)
        s.run(6, 1)
        twin.run(6, 1)
        _same(s, twin, "two steps")


def _raw(lib, h, **fields):
    keep = {k: np.ascontiguousarray(v, np.float64) for k, v in fields.items() if isinstance(v, np.ndarray)}
    step = _abi.CMpcStep(**{k: (_abi.dptr(keep[k]) if k in keep else v) for k, v in fields.items()})
    return lib.admm_mpc_advance(h, C.byref(step), None, None), lib.admm_last_error().decode()


def test_refusals_leave_the_handle_alone(gpu):
    """4. ADMM_ERR_UNSUPPORTED on per-instance and time-sharded handles, every ADMM_ERR_INVALID case; after each refusal a following
    run matches a twin that never saw the call."""
    lib = pkg.load_library()
    cases = [(pkg.random_instances(N=6, n=4, m=2, batch=3), dict(rho=0.3), None, "per-instance"),
             (pkg.cw_rendezvous(N=40, batch=4), dict(rho=0.05, segments=2), (0, 1, None), "time-sharded")]
    for p, kw, ts, word in cases:
        with pkg.Solver(p, pkg.Options(**kw), timeshard=ts) as s, pkg.Solver(p, pkg.Options(**kw), timeshard=ts) as twin:
            s.run(5)
            twin.run(5)
            with pytest.raises(pkg.AdmmError) as e:
                s.mpc_advance()
            assert e.value.code == CODE["ADMM_ERR_UNSUPPORTED"] and word in str(e.value)
            step = _abi.CMpcStep()
            assert lib.admm_mpc_advance_device(s._h, C.byref(step), None, None, None) == CODE["ADMM_ERR_UNSUPPORTED"]
            assert word in lib.admm_last_error().decode()
            s.run(4)
            twin.run(4)
            _same(s, twin, word)
    p = pkg.cw_rendezvous(N=7, batch=5)
    pq = pkg.random_ltv(7, 6, 3, 5, seed=41)
    n, m, b = p.n, p.m, p.batch
    ok_x, ok_u, ok_q = np.ones((b, n)), np.ones((b, m)), np.ones((b, n + m))
    def nan(a):
        a = a.copy()
        a[-1, -1] = np.nan
        return a
    def inf(a):
        a = a.copy()
        a[0, 0] = np.inf
        return a
    invalid = [(p, dict(tail=2), "tail"), (p, dict(tail=-1), "tail"), (p, dict(reserved=1), "reserved"),
               (p, dict(x_meas=ok_x, Ap=np.eye(n)), "x_meas"), (p, dict(x_meas=ok_x, Bp=np.ones((n, m))), "x_meas"),
               (p, dict(x_meas=ok_x, dx=ok_x), "x_meas"), (p, dict(q_tail=ok_q), "q_tail"),
               (p, dict(du=nan(ok_u)), "du"), (p, dict(dx=inf(ok_x)), "dx"), (p, dict(x_meas=nan(ok_x)), "x_meas"),
               (pq, dict(q_tail=inf(ok_q)), "q_tail"), (p, dict(Ap=nan(np.eye(n))), "Ap"), (p, dict(Bp=inf(np.ones((n, m)))), "Bp")]
    for prob, fields, word in invalid:
        with pkg.Solver(prob, pkg.Options(rho=0.3, segments=3)) as s, pkg.Solver(prob, pkg.Options(rho=0.3, segments=3)) as twin:
            s.run(5)
            twin.run(5)
            rc, msg = _raw(lib, s._h, **fields)
            assert rc == CODE["ADMM_ERR_INVALID"] and word in msg, (fields.keys(), rc, msg)
            if word in ("du", "dx", "x_meas", "q_tail") and "non-finite" in msg:      # the device form finds the same entry
                t = torch.from_numpy(fields[word]).to(DEV)
                torch.cuda.synchronize()
                step = _abi.CMpcStep(**{word: pkg.solver._tptr(t)})
                assert lib.admm_mpc_advance_device(s._h, C.byref(step), None, None, None) == CODE["ADMM_ERR_INVALID"]
                assert lib.admm_last_error().decode() == f"admm_mpc_advance_device: non-finite entry in {word}"
            assert lib.admm_mpc_advance(s._h, None, None, None) == CODE["ADMM_ERR_INVALID"] and "step is NULL" in lib.admm_last_error().decode()
            s.run(4)
            twin.run(4)
            _same(s, twin, word)


def test_device_form(gpu):
    """5. Torch inputs (views at an 8-byte offset) give the host form's results bit for bit; a host pointer or a too-short allocation
    is refused with the argument named; work queued on the caller's stream afterwards sees x_next."""
    lib = pkg.load_library()
    p = pkg.random_ltv(7, 6, 3, 65, seed=51)
    n, m, b = p.n, p.m, p.batch
    du, dx = _noise(p, 52)
    qt = np.random.default_rng(53).standard_normal((b, p.nb))
    def view(a):                      # a contiguous view one element into its storage: 8-byte, not 16-byte aligned
        buf = torch.empty(a.size + 1, dtype=torch.float64, device=DEV)
        buf[1:] = torch.from_numpy(a.reshape(-1)).to(DEV)
        return buf[1:].view(a.shape)
    opt = pkg.Options(rho=0.3, segments=3)
    with pkg.Solver(p, opt) as sh, pkg.Solver(p, opt) as sd:
        sh.run(8, 1)
        sd.run(8, 1)
        uh, xh = sh.mpc_advance(du=du, dx=dx, q_tail=qt, tail="zero")
        st = torch.cuda.Stream(device=DEV)
        tdu, tdx, tqt = view(du), view(dx), view(qt)
        assert tdu.data_ptr() % 16 == 8
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            ud, xd = sd.mpc_advance(du=tdu, dx=tdx, q_tail=tqt, tail="zero")
            seen = xd * 1.0                # queued on the caller's stream after the call, without a host synchronisation
        st.synchronize()
        assert ud.is_cuda and xd.is_cuda
        assert np.array_equal(ud.cpu().numpy(), uh) and np.array_equal(xd.cpu().numpy(), xh) and np.array_equal(seen.cpu().numpy(), xh)
        _same(sh, sd, "device form")
        # x_meas from the device, outputs into views at an offset, no outputs at all
        xm = np.random.default_rng(54).standard_normal((b, n))
        uh, xh = sh.mpc_advance(x_meas=xm)
        out_u, out_x = view(np.zeros((b, m))), view(np.zeros((b, n)))
        txm = view(xm)
        step = _abi.CMpcStep(x_meas=pkg.solver._tptr(txm))
        torch.cuda.synchronize()         # (hip_stream = NULL: the caller vouches that its data are ready)
        assert lib.admm_mpc_advance_device(sd._h, C.byref(step), pkg.solver._tptr(out_u), pkg.solver._tptr(out_x), None) == 0
        assert np.array_equal(out_u.cpu().numpy(), uh) and np.array_equal(out_x.cpu().numpy(), xm)
        sh.mpc_advance()
        assert lib.admm_mpc_advance_device(sd._h, C.byref(_abi.CMpcStep()), None, None, None) == 0
        _same(sh, sd, "x_meas, then no arrays")
        # host and pinned pointers, too-short allocations: refused by name, nothing changed
        hostv = np.zeros(b * p.nb)
        pinned = torch.zeros(b * p.nb, dtype=torch.float64).pin_memory()
        big = torch.zeros(3 * 2 ** 20, dtype=torch.float64, device=DEV)
        sizes = {"du": b * m, "dx": b * n, "x_meas": b * n, "q_tail": b * p.nb, "u_applied": b * m, "x_next": b * n}
        def call(name, ptr):
            step = _abi.CMpcStep(**({name: ptr} if name not in ("u_applied", "x_next") else {}))
            return lib.admm_mpc_advance_device(sd._h, C.byref(step), ptr if name == "u_applied" else None,
                                               ptr if name == "x_next" else None, None)
        for name, need in sizes.items():
            for host in (_abi.dptr(hostv), pkg.solver._tptr(pinned)):
                assert call(name, host) == CODE["ADMM_ERR_INVALID"]
                assert f"admm_mpc_advance_device: {name} is not device memory" in lib.admm_last_error().decode()
            assert call(name, pkg.solver._tptr(big[big.numel() - (need - 1):])) == CODE["ADMM_ERR_INVALID"]
            msg = lib.admm_last_error().decode()
            assert f"admm_mpc_advance_device: {name} ends before its {need} doubles" in msg, msg
        torch.cuda.synchronize()
        assert (big == 0).all() and (hostv == 0).all() and (pinned == 0).all()
        sh.run(3, 1)
        sd.run(3, 1)
        _same(sh, sd, "after the refusals")


def test_closed_loop(gpu):
    """6. mpc_batch(on_device=True) on double_integrator(N=30, batch=65), 6 steps with process noise; the host route replayed on the
    recorded x+: U and the iteration counts equal, X equal bitwise; every warm solve takes fewer iterations than step 0's cold one."""
    p = pkg.double_integrator(N=30, batch=65)
    opt = pkg.Options(rho=1.0, check_interval=5, max_iter=2000)
    dev = pkg.mpc_batch(p, 6, opt, noise=1e-3, on_device=True)
    host = pkg.mpc_batch(p, 6, opt, noise=1e-3, on_device=False, replay=dev.X)
    print("iterations per step:", dev.iterations.tolist(), "converged:", dev.converged.tolist())
    assert np.array_equal(dev.U, host.U) and np.array_equal(dev.X, host.X)
    assert np.array_equal(dev.iterations, host.iterations) and np.array_equal(dev.converged, host.converged)
    assert (dev.converged == p.batch).all()
    assert (dev.iterations[1:] < dev.iterations[0]).all()
    # the device's plant arithmetic against NumPy's: within the dot-product bound, step by step
    dx = 1e-3 * np.random.default_rng(0).standard_normal((6, p.batch, p.n))
    for t in range(6):
        ref = plant_step(dev.X[t], dev.U[t], p.A, p.B, dx[t])
        bound = 2 * (p.nb + 1) * U * (np.abs(dx[t]) + np.abs(dev.X[t]) @ np.abs(p.A).T + np.abs(dev.U[t]) @ np.abs(p.B).T)
        assert (np.abs(dev.X[t + 1] - ref) <= bound).all()
