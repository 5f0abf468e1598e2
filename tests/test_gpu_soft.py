"""Soft box constraints on the GPU (csrc/admm_soft_kernels.hpp) against tests/_soft_ref.py -- the fuel helper's
loop with the soft prox (tests/test_soft_host.py checks that reference on the CPU and holds the solve cases).

Shapes are chosen for the kernel's geometry (one lane = two adjacent QPs, 512 columns per workgroup, four rows in flight, chunks of
Options.zrows rows): batches 1 and 3 (odd: a pad column beside the last QP), 70 and 129 (pad columns, a pitch of 128 / 192), 600
(two workgroups along the batch); N = 5, 7, 13 with 6, 9 or 18 rows per stage (L no multiple of 4) and chunks of 8 rows, whose last
one is shorter and leaves a remainder to the row-at-a-time loop; whole blocks per chunk in the block-structured form."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded, as in tests/test_gpu_device_io.py)

import admm_library_amd as pkg
import _infeas_cases as ic
import _infeas_ref as ir
import _prox_cases as pc
import _readout_cases as rc
import _soft_ref as sr
import test_soft_host as host
from admm_library_amd import _abi
from admm_library_amd.mpc import shift_horizon

pytestmark = pytest.mark.gpu
TOL = 1e-10            # x max(1, |.|): the project's iterate tolerance, as tests/test_gpu_consensus.py
INVALID, UNSUPPORTED = 1, 2
INF = np.inf
DEV = "cuda:0"
PAIRS = [(4, 2), (6, 3), (12, 6)]
BATCHES = [1, 3, 70, 129, 600]
FORMS = ["noresid", "relax", "lti_box", "thrust", "fuel", "seg1", "seg4"]
STAGES = dict(noresid=5, relax=7, lti_box=7, thrust=5, fuel=7, seg1=13, seg4=13)
RHO = 0.3


def make_problem(form, n, m, batch, with_q, seed=None):
    """(problem, options, residual_every) of a form."""
    N = STAGES[form]
    p = pkg.random_ltv(N=N, n=n, m=m, batch=batch, seed=2000 + 16 * n + m if seed is None else seed, with_q=with_q,
                       thrust_norm=form in ("thrust", "fuel"))
    if form == "fuel":
        p = rc.stage_fuel(p)
    sw = host.random_soft(p)
    if form == "lti_box":
        p, sw = rc.lti(p), sw[1].copy()
    kw = dict(rho=RHO)
    if form == "relax":
        kw["alpha"] = 1.6
    if form in ("seg1", "seg4"):
        kw["segments"] = int(form[3:])
    if form in ("noresid", "relax", "seg4"):
        kw["zrows"] = 8                    # chunks of 8 rows: the last one is shorter, and not a multiple of 4
    if form == "fuel":
        kw["zrows"] = 2 * p.nb             # two blocks per chunk, one in the last
    return dataclasses.replace(p, soft=sw), kw, (0 if form == "noresid" else 1)


def _close(a, b, tol=TOL):
    return np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


def _ref(p, kw, k, every, **more):
    return sr.solve(p, rho=kw["rho"], alpha=kw.get("alpha", 1.0), max_iter=k, check_interval=max(every, 1), eps_abs=0, eps_rel=0,
                    stop=False, **more)


def _solver(p, **kw):
    s = pkg.Solver(p, pkg.Options(**kw))
    path = s.path()
    assert not path["alternating"] and not path["alt_requested"] and path["kernel_family"] == "one_lane_fp64", path
    return s


# ---- 1. iterates and residuals against the reference ----

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("batch", BATCHES)
def test_iterates_match_the_reference(gpu, batch, form):
    for n, m in PAIRS:
        for with_q in (False, True):
            p, kw, every = make_problem(form, n, m, batch, with_q)
            with _solver(p, **kw) as s:
                geo = s.geometry()
                if form in ("seg1", "seg4"):
                    assert geo["segments"] == kw["segments"]
                if form in ("noresid", "relax", "seg4"):
                    assert geo["zrows"] == 8 and p.L % 8 != 0 and (p.L % 8) % 4 != 0
                if form in ("thrust", "fuel"):
                    assert geo["zrows"] % p.nb == 0
                assert np.array_equal(s.soft(), np.broadcast_to(p.soft, (p.N, p.nb)))
                done = 0
                for k in (1, 2, 7):
                    s.run(k - done, residual_every=every)
                    done = k
                    w, z, y = s.get()
                    ref = _ref(p, kw, k, every)
                    for name, a, b in (("w", w, ref.w), ("z", z, ref.z), ("y", y, ref.y)):
                        assert _close(a, b), (n, m, with_q, k, name, np.abs(a - b).max())
                    if every:
                        r, sd, *_ = s.residuals()
                        assert _close(r, ref.r) and _close(sd, ref.s), (n, m, with_q, k, np.abs(r - ref.r).max(), np.abs(sd - ref.s).max())
            # the weights matter: the hard problem's iterates are elsewhere
            if with_q and batch == 70:
                hard = _ref(dataclasses.replace(p, soft=None), kw, 7, every)
                assert np.abs(hard.z - ref.z).max() > 1e-3


# ---- 2. infinite weights are the unfused path, bit for bit ----

@pytest.mark.parametrize("alpha", [1.0, 1.6])
@pytest.mark.parametrize("kind", ["box", "thrust", "fuel"])
@pytest.mark.parametrize("batch", [70, 195])
def test_infinite_weights_are_the_unfused_handle_bit_for_bit(gpu, batch, kind, alpha):
    """zdual_kernel (box) / zdual_soc_kernel (thrust, fuel) against zdual_soft_kernel with every weight +inf, residuals included.
    Both handles get two blocks per chunk: the residual sums are added chunk by chunk."""
    p = pkg.random_ltv(N=9, n=6, m=3, batch=batch, seed=77, thrust_norm=kind != "box")
    if kind == "fuel":
        p = rc.stage_fuel(p)
    kw = dict(rho=RHO, alpha=alpha, zrows=2 * p.nb)
    out = []
    with pkg.Solver(p, pkg.Options(flags=_abi.FLAG_UNFUSED, **kw)) as plain, \
            _solver(dataclasses.replace(p, soft=np.full((p.N, p.nb), INF)), **kw) as s:
        assert plain.geometry() == s.geometry()
        for h in (plain, s):
            h.run(9, residual_every=3)
            out.append(h.get() + tuple(h.residuals()))
        rep = s.soft_report()
    for i, (a, b) in enumerate(zip(*out)):
        assert np.array_equal(a, b), i
    assert not rep.penalty.any() and not rep.max_violation.any() and not rep.n_violated.any()      # no row has a finite weight


# ---- 3. the edges, bit for bit ----

def edge_case(n, m, batch, form, rho):
    """The decoupled problem of tests/_prox_cases.py with weights and a state (z0, y0) that puts v on the soft prox's edges in the
    first iteration.  Row r = k nb + j carries the weight rho * KAPS[r % 5]; QP b's v on it is variant (b + r) % 9 of: hi + kap and
    one ulp either side, lo - kap and one ulp either side, a point inside, a point 2 kap beyond hi, lo itself (a row without that
    bound takes the other one; a free row 0.1).  The control rows of a stage with a thrust bound keep _prox_cases' own table."""
    case = pc.make(n, m, batch, form, rho=rho)
    p = case.p
    nb = p.nb
    kaps = (0.125, 0.0, INF, 2.0 ** -30, 0.375)
    sw = np.array([[rho * kaps[(k * nb + j) % 5] for j in range(nb)] for k in range(pc.N)])
    sw[case.soc, :m] = INF
    z0, y0 = case.z0.reshape(batch, pc.N, nb).copy(), case.y0.reshape(batch, pc.N, nb).copy()
    for b in range(batch):
        for k in range(pc.N):
            for j in range(nb):
                if j < m and case.soc[k]:
                    continue
                r = k * nb + j
                lo, hi = case.lo[b, k, j], case.hi[b, k, j]
                kap = kaps[r % 5]
                kk = kap if np.isfinite(kap) and kap > 0 else 0.125
                var = (b + r) % 9
                if not np.isfinite(lo) and not np.isfinite(hi):
                    v = 0.1
                else:
                    use_hi = np.isfinite(hi) and (var in (0, 1, 2, 7) or not np.isfinite(lo))
                    edge = hi + kk if use_hi else lo - kk
                    v = {0: edge, 1: pc.up(edge), 2: pc.dn(edge), 3: edge, 4: pc.dn(edge), 5: pc.up(edge),
                         6: 0.5 * (max(lo, -1.0) + min(hi, 1.0)), 7: hi + 2 * kk if use_hi else lo - 2 * kk, 8: lo if np.isfinite(lo) else hi}[var]
                if j < m:
                    z0[b, k, j], y0[b, k, j] = v, 0.0
                else:
                    z0[b, k, j] = case.wx[b, k, j - m]
                    y0[b, k, j] = v - case.wx[b, k, j - m]
    ps = dataclasses.replace(p, soft=sw)
    ps.validate()
    return case, ps, z0.reshape(batch, -1), y0.reshape(batch, -1)


def edge_model(case, ps, z, y):
    """One iteration of the decoupled model in NumPy fp64, one rounding per operation: w, v of _prox_cases.iterate (exact rationals
    rounded once: the same values), the soft prox on v, the thrust stages' control rows from _prox_cases."""
    w, v, zh, _ = pc.iterate(case, z, y)
    batch, nb = ps.batch, ps.nb
    skap = (np.broadcast_to(ps.soft, (pc.N, nb)) / case.rho)[None]
    zn = sr.soft_clip(v.reshape(batch, pc.N, nb), case.lo, case.hi, skap)
    zn[:, case.soc, :ps.m] = zh.reshape(batch, pc.N, nb)[:, case.soc, :ps.m]
    zn = zn.reshape(batch, -1)
    return w, v, zn, v - zn


@pytest.mark.parametrize("rho", pc.RHOS)
@pytest.mark.parametrize("form", ["box", "ball"])
@pytest.mark.parametrize("shape", [(4, 2), (6, 3)], ids=["4x2", "6x3"])
def test_edges_bit_for_bit(gpu, shape, form, rho):
    n, m = shape
    batch = 67
    case, ps, z, y = edge_case(n, m, batch, form, rho)
    nb = ps.nb
    skap = np.broadcast_to(np.broadcast_to(ps.soft, (pc.N, nb)) / rho, (batch, pc.N, nb)).reshape(batch, -1)
    lo, hi = case.lo.reshape(batch, -1), case.hi.reshape(batch, -1)
    with _solver(ps, rho=rho) as s:
        s.set_state(z=z, y=y)
        for it in range(3):
            w, v, zn, yn = edge_model(case, ps, z, y)
            if it == 0:                    # the table is what it claims to be
                c = np.minimum(np.maximum(v, lo), hi)
                e = v - c
                fin = np.isfinite(skap) & (skap > 0)
                assert (e[fin] == skap[fin]).any() and (e[fin] == -skap[fin]).any()
                for sgn in (1.0, -1.0):
                    assert ((sgn * e[fin] > skap[fin]) & (sgn * e[fin] < skap[fin] * (1 + 1e-9))).any()
                    assert ((sgn * e[fin] < skap[fin]) & (sgn * e[fin] > skap[fin] * (1 - 1e-9))).any()
                assert ((skap == 0) & (e != 0)).any() and (np.isinf(skap) & (e != 0)).any()
                pinned = (lo == hi) & fin
                assert (pinned & (np.abs(e) > skap)).any() and (pinned & (np.abs(e) <= skap) & (e != 0)).any()
                one_sided = (np.isinf(lo) != np.isinf(hi)) & fin
                assert (one_sided & (np.abs(e) > skap)).any() and (one_sided & (e == 0)).any()
                negz = (((lo == 0) & np.signbit(lo)) | ((hi == 0) & np.signbit(hi))) & fin
                assert negz.any() and (negz & (e != 0)).any()
                assert np.array_equal(zn[skap == 0], v[skap == 0]) and not yn[skap == 0].any()
                assert np.array_equal(zn[np.isinf(skap)], c[np.isinf(skap)]) or form == "ball"
            s.run(1, residual_every=1)
            gw, gz, gy = s.get()
            for name, a, b in (("w", gw, w), ("z", gz, zn), ("y", gy, yn)):
                assert np.isfinite(a).all()
                if not np.array_equal(a, b):
                    i = np.argwhere(a != b)[0]
                    raise AssertionError((it, name, "QP %d row %d" % tuple(i), a[tuple(i)], b[tuple(i)], v[tuple(i)], skap[tuple(i)]))
            z, y = zn, yn


# ---- 4. the report ----

@pytest.mark.parametrize("form,batch", [("relax", 70), ("fuel", 129), ("lti_box", 3)])
def test_report_against_numpy(gpu, form, batch):
    """Penalty within 4 ulps of the fma chain in row order (the kernel runs that very chain), the largest violation and the count
    exact; host and device forms agree bit for bit."""
    p, kw, _ = make_problem(form, 6, 3, batch, True)
    with _solver(p, **kw) as s, _solver(p, **kw) as twin:
        s.run(6)
        twin.run(6)
        _, z, _ = s.get()
        rep = s.soft_report()
        dev = s.soft_report(device=True)
        torch.cuda.synchronize()
        pen, mx, cnt = sr.report(p, z)
        assert (pen > 0).sum() >= (batch + 1) // 2 and not pen[cnt == 0].any() and (mx[cnt > 0] > 0).all()
        assert rep.n_violated.dtype == np.int32 and np.array_equal(rep.n_violated, cnt) and np.array_equal(rep.max_violation, mx)
        assert (np.abs(rep.penalty - pen) <= 4 * np.spacing(pen)).all(), np.abs(rep.penalty - pen).max()
        assert np.array_equal(dev.penalty.cpu().numpy(), rep.penalty) and np.array_equal(dev.max_violation.cpu().numpy(), rep.max_violation)
        assert dev.n_violated.dtype == torch.int32 and np.array_equal(dev.n_violated.cpu().numpy(), cnt)
        # any pointer may be NULL
        lib, one = pkg.load_library(), np.zeros(batch)
        assert lib.admm_get_soft_report(s._h, None, _abi.dptr(one), None) == 0 and np.array_equal(one, mx)
        # the objective of the certificate leaves the penalty out
        cert = s.certificate()
        assert np.isfinite(cert.obj).all()
        # reading changes nothing
        s.run(3, residual_every=1)
        twin.run(3, residual_every=1)
        for a, b in zip(s.get() + tuple(s.residuals()), twin.get() + tuple(twin.residuals())):
            assert np.array_equal(a, b)


def test_device_form_of_the_report_checks_its_pointers(gpu):
    lib = pkg.load_library()
    p, kw, _ = make_problem("relax", 6, 3, 70, True)

    def dp(t, typ=_abi.c_double_p):
        return C.cast(C.c_void_p(t.data_ptr()), typ)
    with _solver(p, **kw) as s:
        s.run(5)
        ref = s.soft_report()
        t = torch.zeros(p.batch + 1, dtype=torch.float64, device=DEV)
        ti = torch.zeros(p.batch + 1, dtype=torch.int32, device=DEV)
        assert lib.admm_get_soft_report_device(s._h, dp(t[1:]), None, dp(ti[1:], _abi.c_int32_p), pkg.solver._stream(DEV)) == 0
        torch.cuda.synchronize()
        assert np.array_equal(t[1:].cpu().numpy(), ref.penalty) and t[0] == 0
        assert np.array_equal(ti[1:].cpu().numpy(), ref.n_violated) and ti[0] == 0
        hostv = np.zeros(p.batch)
        assert lib.admm_get_soft_report_device(s._h, _abi.dptr(hostv), None, None, None) == INVALID
        assert "admm_get_soft_report_device: penalty is not device memory" in lib.admm_last_error().decode()
        assert lib.admm_get_soft_report_device(s._h, None, None, None, None) == INVALID and b"at least one" in lib.admm_last_error()
        assert lib.admm_get_soft_report(s._h, None, None, None) == INVALID and b"at least one" in lib.admm_last_error()
        assert not hostv.any()


# ---- 5. solves ----

def test_a_soft_corridor_converges_to_its_optimality_conditions(gpu):
    """The host test's case and conditions on the GPU's (z, y); iteration count and iterates follow the reference."""
    p = host.kkt_problem()
    ref = sr.solve(p, **host.KKT_OPTS)
    with _solver(p, **host.KKT_OPTS) as s:
        info = s.solve()
        w, z, y = s.get()
        rep = s.soft_report()
    assert info.status.all() and info.iters_run == ref.iters_run and np.array_equal(info.iters, ref.iters)
    assert _close(w, ref.w) and _close(z, ref.z) and _close(y, ref.y)
    c = sr.conditions(p, z, y, float(info.rho))
    worst = {k: float(np.max(v)) for k, v in c.items()}
    assert c["feas_dyn"].max() < 1e-6 and c["stat"].max() < 1e-6, worst
    assert c["inside"].max() < 1e-6 and c["on_bound"].max() < 1e-6 and c["outside"].max() < 1e-6 and c["feas_hard"].max() == 0.0, worst
    assert rep.n_violated.tolist() == [0, 0, 0, 7, 5] and c["n_outside"].tolist() == [0, 0, 0, 7, 5]


def test_adaptive_rho_follows_the_reference(gpu):
    """The case whose decisions tests/test_soft_host.py shows to be clear of the thresholds: 150 iterations, the rho of every
    stopping test equals the reference's, the iterates agree."""
    p = host.kkt_problem()
    dec = []
    ref = sr.solve(p, stop=False, decisions=dec, **host.ADAPT_OPTS)
    trajectory = [host.ADAPT_OPTS["rho"]] + [d[3] for d in dec]
    with _solver(p, flags=_abi.FLAG_HISTORY, **host.ADAPT_OPTS) as s:
        info = s.solve()
        w, z, y = s.get()
        hist = s.history()
    assert (info.iters_run, info.rho_updates, info.rho) == (ref.iters_run, ref.rho_updates, ref.rho)
    assert hist["iteration"].tolist() == list(range(10, 151, 10)) and hist["rho"].tolist() == trajectory
    assert _close(w, ref.w) and _close(z, ref.z) and _close(y, ref.y)


# ---- 6. changes in mid-run ----

@pytest.mark.parametrize("form", ["relax", "fuel"])
def test_set_soft_set_rho_and_update_problem(gpu, form):
    p, kw, _ = make_problem(form, 6, 3, 70, True)
    with _solver(p, **kw) as s:
        s.run(4, residual_every=2)
        _, z, y = s.get()
        ref = _ref(p, kw, 4, 2)
        assert _close(z, ref.z) and _close(y, ref.y)
        # new weights: continuation from the warm start
        sw2 = np.where(np.isfinite(p.soft), 0.25 * p.soft + 0.01, INF)
        sw2[2, p.m:] = INF                                   # a stage's state rows become hard
        s.set_soft(sw2)
        assert np.array_equal(s.soft(), sw2) and np.array_equal(s.problem.soft, sw2)
        p2 = dataclasses.replace(p, soft=sw2)
        s.run(3, residual_every=3)
        w, z, y = s.get()
        ref = _ref(p2, kw, 3, 3, z0=ref.z, y0=ref.y)
        assert _close(w, ref.w) and _close(z, ref.z) and _close(y, ref.y) and _close(s.residuals()[0], ref.r)
        # new rho: y is rescaled, the factor rebuilt, kappa = s / rho refreshed
        rho2 = 0.8
        s.set_rho(rho2)
        s.run(3, residual_every=3)
        w, z, y = s.get()
        kw2 = dict(kw, rho=rho2)
        ref = _ref(p2, kw2, 3, 3, z0=ref.z, y0=ref.y * (kw["rho"] / rho2))
        assert _close(w, ref.w) and _close(z, ref.z) and _close(y, ref.y) and _close(s.residuals()[0], ref.r)
        # new problem data: the weights stay
        q3 = pkg.random_ltv(N=p.N, n=6, m=3, batch=70, seed=4242, with_q=True, thrust_norm=form == "fuel")
        p3 = dataclasses.replace(p2, A=q3.A, B=q3.B, Q=q3.Q, R=q3.R, QN=q3.QN, x0=q3.x0, q=q3.q,
                                 lo=np.where(np.isfinite(p2.lo), 0.9 * p2.lo, p2.lo), hi=np.where(np.isfinite(p2.hi), 1.1 * p2.hi, p2.hi))
        s.update_problem(dataclasses.replace(p3, soft=None))
        assert np.array_equal(s.soft(), sw2) and np.array_equal(s.problem.soft, sw2)
        s.run(2, residual_every=2)
        w, z, y = s.get()
        ref = _ref(p3, kw2, 2, 2, z0=ref.z, y0=ref.y)
        assert _close(w, ref.w) and _close(z, ref.z) and _close(y, ref.y) and _close(s.residuals()[0], ref.r)
        with pytest.raises(ValueError, match="set_soft"):
            s.update_problem(dataclasses.replace(p3, soft=np.where(np.isfinite(sw2), 2.0 * sw2, INF)))


@pytest.mark.parametrize("form,batch", [("relax", 129), ("fuel", 600)])
def test_graph_replay_gives_the_bits_of_direct_launches(gpu, form, batch):
    p, kw, _ = make_problem(form, 6, 3, batch, True)
    out = []
    for flags in (0, _abi.FLAG_GRAPH):
        with _solver(p, flags=flags, **kw) as s:
            s.run(7, residual_every=2)
            s.set_soft(np.where(np.isfinite(p.soft), 0.5 * p.soft, INF))      # kappa changes under the captured graph
            s.run(5, residual_every=2)
            out.append(s.get() + tuple(s.residuals()))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("tail", ["copy", "zero"])
def test_mpc_advance_equals_the_host_route(gpu, tail):
    """admm_mpc_advance on a soft handle against get, a NumPy shift, update_instances, set_state, bit for bit: the weights are
    window-relative, nothing of them shifts."""
    p, kw, _ = make_problem("relax", 6, 3, 70, False)
    with _solver(p, **kw) as a, _solver(p, **kw) as b:
        for step in range(3):
            a.run(5, residual_every=5)
            b.run(5, residual_every=5)
            u, xn = a.mpc_advance(tail=tail)
            w, z, y = b.get()
            assert np.array_equal(u, z[:, :p.m])
            b.update_instances(xn)
            b.set_state(shift_horizon(w, p.nb, tail), shift_horizon(z, p.nb, tail), shift_horizon(y, p.nb, tail))
            assert np.array_equal(a.soft(), b.soft())
        a.run(4, residual_every=2)
        b.run(4, residual_every=2)
        for x, yv in zip(a.get() + tuple(a.residuals()) + (a.soft_report().penalty,), b.get() + tuple(b.residuals()) + (b.soft_report().penalty,)):
            assert np.array_equal(x, yv)


# ---- 7. the probe ----

def _opened(p):
    """p with the box of every row with a finite weight removed: the feasibility problem of a soft handle."""
    sw = np.broadcast_to(p.soft, p.lo.shape)
    return dataclasses.replace(p, lo=np.where(np.isfinite(sw), -INF, p.lo), hi=np.where(np.isfinite(sw), INF, p.hi), soft=None)


def test_probe_on_hard_soft_and_pinned_corridors(gpu):
    """di_position_box of tests/_infeas_cases.py.  Hard: QPs 1, 2, 3 flagged.  The corridor soft: none flagged, every QP solves.
    Soft corridor with the terminal state pinned hard at the origin: the QPs that cannot stop are flagged.  The flags are those
    of the NumPy probe on the reference's iterates of the opened problem."""
    base = ic.di_position_box()
    opt = dict(rho=ic.RHO)
    with pkg.Solver(base, pkg.Options(**opt)) as s:
        s.run(100)
        assert s.infeasibility(span=10, eps=ic.EPS).infeasible.tolist() == [0, 1, 1, 1]
    soft = dataclasses.replace(base, soft=host.corridor_weights(base, 5.0))
    pinned = ic.pin_terminal(base)
    swp = host.corridor_weights(base, 5.0)
    swp[-1, base.m] = INF
    pinned = dataclasses.replace(pinned, soft=swp)
    for p, flags in ((soft, [0, 0, 0, 0]), (pinned, [0, 1, 1, 1])):
        r = sr.solve(p, rho=ic.RHO, max_iter=110, stop=False, record={100, 110}, eps_abs=0, eps_rel=0)
        (_, _, _, ya), (_, _, _, yb) = r.history
        want = ir.probe(_opened(p), ya, yb, 10, ic.EPS)
        assert want["infeasible"].tolist() == flags
        with _solver(p, **opt) as s:
            s.run(100)
            got = s.infeasibility(span=10, eps=ic.EPS)
            assert got.infeasible.tolist() == flags, (got.sep, want["sep"])
            fin = np.isfinite(want["sep"])
            assert np.array_equal(np.isfinite(got.sep), fin) and np.allclose(got.sep[fin], want["sep"][fin], rtol=1e-6)
            if p is soft:
                info = s.solve()
                assert info.status.all()
                rep = s.soft_report()
                assert rep.max_violation[0] == 0.0 and (rep.max_violation[1:] > 1.0).all()


# ---- 8. refusals ----

def test_setup_refusals(gpu):
    p, kw, _ = make_problem("relax", 4, 2, 6, True)
    for mode in (_abi.PRECISION_MIXED, _abi.PRECISION_FP64_MFMA):
        with pytest.raises(pkg.AdmmError) as e:
            pkg.Solver(p, pkg.Options(rho=RHO, precision_mode=mode))
        assert e.value.code == UNSUPPORTED and "precision_mode" in str(e.value) and "soft" in str(e.value)
    with pytest.raises(ValueError, match="time-sharded"):
        pkg.Solver(p, pkg.Options(rho=RHO, segments=2), timeshard=(0, 1, None))
    with pytest.raises(ValueError, match="consensus"):
        pkg.Solver(dataclasses.replace(p, consensus=3), pkg.Options(rho=RHO))
    d = pkg.DeviceProblem.from_problem(p, DEV)
    assert d.soft is not None
    with pytest.raises(ValueError, match="soft"):
        pkg.Solver(d, pkg.Options(rho=RHO))
    # a handle without weights
    lib = pkg.load_library()
    plain = dataclasses.replace(p, soft=None)
    with pkg.Solver(plain, pkg.Options(rho=RHO)) as s:
        out, cnt = np.zeros(p.batch), np.zeros(p.batch, np.int32)
        sw = np.ascontiguousarray(np.broadcast_to(p.soft, (p.N, p.nb)))
        assert lib.admm_set_soft(s._h, _abi.dptr(sw)) == INVALID and b"cannot be added" in lib.admm_last_error()
        assert lib.admm_get_soft_report(s._h, _abi.dptr(out), None, _abi.iptr(cnt)) == INVALID and b"no soft weights" in lib.admm_last_error()
        assert lib.admm_get_soft_report_device(s._h, _abi.dptr(out), None, None, None) == INVALID and b"no soft weights" in lib.admm_last_error()
        assert np.isinf(s.soft()).all() and not out.any() and not cnt.any()
        with pytest.raises(pkg.AdmmError):
            s.set_soft(sw)
        with pytest.raises(ValueError, match="cannot be added"):
            s.update_problem(p)


def test_refusals_leave_the_handle_alone(gpu):
    lib = pkg.load_library()
    p, kw, _ = make_problem("thrust", 6, 3, 70, True)
    sw = np.ascontiguousarray(p.soft)
    with _solver(p, **kw) as s, _solver(p, **kw) as twin:
        s.run(5)
        twin.run(5)
        for bad in (-1.0, np.nan):
            cand = sw.copy()
            cand[3, 5] = bad
            assert lib.admm_set_soft(s._h, _abi.dptr(cand)) == INVALID and b">= 0" in lib.admm_last_error()
            with pytest.raises(ValueError):
                s.set_soft(cand)
        cand = sw.copy()
        cand[int(np.nonzero(np.isfinite(p.unorm))[0][0]), 0] = 1.0
        assert lib.admm_set_soft(s._h, _abi.dptr(cand)) == INVALID and b"control rows" in lib.admm_last_error()
        assert lib.admm_set_soft(s._h, None) == INVALID
        assert np.array_equal(s.soft(), sw)
        # a new problem whose thrust stages meet a finite weight on a control row: refused, nothing changed
        k_free = int(np.nonzero(~np.isfinite(p.unorm) & np.isfinite(sw[:, :p.m]).any(axis=1))[0][0])
        un = p.unorm.copy()
        un[k_free] = 0.4
        lo, hi = p.lo.copy(), p.hi.copy()
        lo[k_free, :p.m], hi[k_free, :p.m] = -INF, INF
        cp, keep = _abi.marshal_problem(dataclasses.replace(p, unorm=un, lo=lo, hi=hi, soft=None))
        assert lib.admm_update_problem(s._h, C.byref(cp)) == INVALID and b"control rows" in lib.admm_last_error()
        # the fused modes of admm_profile carry the hard z-update
        for mode_kw in (dict(), dict(fused=True), dict(alternating=True), dict(alternating=True, back_to_back=True), dict(alternating=True, lean=True)):
            with pytest.raises(pkg.AdmmError) as e:
                s.profile(3, **mode_kw)
            assert e.value.code == UNSUPPORTED and "unfused path only" in str(e.value), (mode_kw, str(e.value))
        s.run(4, residual_every=2)
        twin.run(4, residual_every=2)
        for a, b in zip(s.get() + tuple(s.residuals()), twin.get() + tuple(twin.residuals())):
            assert np.array_equal(a, b)
        # ... and the unfused mode is four plain iterations of the handle's own kernels
        ms = s.profile(4, residuals=True, fused=False)
        assert ms["zdual_ms"] > 0
        twin.run(4, residual_every=1)
        for a, b in zip(s.get(), twin.get()):
            assert np.array_equal(a, b)


def test_set_fuel_respects_the_soft_weights(gpu):
    """A stage with open control rows, no thrust bound and no fuel weight carries a finite soft weight on a control row: a fuel
    weight on that stage would hand the row to the shrink-and-scale projection -- admm_set_fuel refuses, the handle is unchanged."""
    lib = pkg.load_library()
    p, kw, _ = make_problem("fuel", 6, 3, 70, True)
    k0 = int(np.nonzero(~np.isfinite(p.unorm))[0][0])
    lo, hi, sw = p.lo.copy(), p.hi.copy(), p.soft.copy()
    lo[k0, :p.m], hi[k0, :p.m] = -INF, INF
    sw[k0, 0] = 0.3
    p = dataclasses.replace(p, lo=lo, hi=hi, soft=sw)
    with _solver(p, **kw) as s, _solver(p, **kw) as twin:
        s.run(5)
        twin.run(5)
        fuel = np.ascontiguousarray(s.fuel())
        assert fuel[k0] == 0.0
        fuel[k0] = 0.2
        assert lib.admm_set_fuel(s._h, _abi.dptr(fuel)) == INVALID and b"soft entries of the control rows" in lib.admm_last_error()
        with pytest.raises(ValueError, match="soft"):
            s.set_fuel(fuel)
        assert s.fuel()[k0] == 0.0
        # ... and a change that leaves that stage alone goes through
        ok = np.where(s.fuel() > 0, 0.5 * s.fuel(), 0.0)
        s.set_fuel(ok)
        twin.set_fuel(ok)
        s.run(4, residual_every=2)
        twin.run(4, residual_every=2)
        for a, b in zip(s.get() + tuple(s.residuals()), twin.get() + tuple(twin.residuals())):
            assert np.array_equal(a, b)
