"""Time-sharded handles (admm_setup_timeshard) on INTERIOR ranks and through the state changes include/admm_hip.h
promises for them: three and four ranks as threads of one process (tests/_timeshard.py), windows of unequal length, warm starts,
new instance data, rho changes, problem updates, the adaptive solve, the full-array twin, the refusals.  An interior rank has
stage_lo > 0 and stage_hi < N: both of its boundary exchanges are live and every windowed pointer and row offset is non-trivial.

The reference is the oracle (oracle_c.solve), warm-started through z0 / y0 where a handle's state is carried over a change; the
tolerance is the suite's own for fp64 paths, 1e-10 max(1, |ref|_inf) on w, z, y and 1e-10 on r, s (tests/test_shapes.py keeps
every case inside the conditioning bound of the segment scan).  Residuals are compared bit for bit across the ranks."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch  # (before libadmm_hip.so is loaded: the exchange runs torch and the library on ONE HIP runtime, torch's)

import admm_library_amd as pkg
import oracle_c as oc
from admm_library_amd import _abi
from admm_library_amd.solver import AdmmError, Options, Solver
from _timeshard import (ADAPT, ALPHAS, CASES, RHO_FACTOR, SENTINEL, UPDATE_CASES, OracleChain, assemble, inside_window, outside_window,
                        read_into, run_ranks, second_problem)

pytestmark = pytest.mark.gpu
TOL = 1e-10
UPTO = (1, 2, 3, 4, 8, 24)
INVALID, UNSUPPORTED, HIP_ERROR = 1, 2, 4


def _err(got, ref):
    return max(np.abs(a - ref[k]).max() / max(1.0, np.abs(ref[k]).max()) for a, k in zip(got, "wzy"))


def _opts(case, alpha, **more):
    return dict(CASES[case].opts, alpha=alpha, **more)


def _check_setup(case, run, p):
    """The windows tile [0, N) in rank order, hold the same number of segments, differ in length where the table says so, and one
    rank at least is interior; every rank takes the path the table records."""
    c, wins = CASES[case], run.wins
    assert wins[0]["stage_lo"] == 0 and wins[-1]["stage_hi"] == p.N
    assert all(a["stage_hi"] == b["stage_lo"] for a, b in zip(wins, wins[1:]))
    assert all(w["stage_lo"] < w["stage_hi"] for w in wins)
    sl = wins[0]["segs_local"]
    assert all(w["segs_local"] == sl and w["segs_total"] == sl * c.world and w["seg_lo"] == r * sl for r, w in enumerate(wins))
    assert any(0 < w["stage_lo"] and w["stage_hi"] < p.N for w in wins)
    assert (len({w["stage_hi"] - w["stage_lo"] for w in wins}) > 1) == c.uneven, wins
    if c.opts["segments"]:
        assert wins[0]["segs_total"] == c.opts["segments"]
    assert all(pt["alternating"] == c.alternating for pt in run.paths), run.paths
    assert all(pt["scan_form"] == ("matrix_vector" if p.batch <= 4 else "mfma_gemm") for pt in run.paths)
    assert len({tuple(sorted(pt.items())) for pt in run.paths}) == 1


def _check_state(run, p, got, ref, what):
    """got[r] = (w, z, y[, r, s]) of rank r: the assembled iterates equal the chain's, every rank's residuals do, and the ranks hold
    the same residuals bit for bit."""
    full = assemble([g[:3] for g in got], run.wins, p.nb)
    e = _err(full, ref)
    assert e <= TOL, (what, e)
    if len(got[0]) > 3:
        for g in got:
            assert np.abs(g[3] - ref["r"]).max() <= TOL and np.abs(g[4] - ref["s"]).max() <= TOL, what
        for g in got[1:]:
            np.testing.assert_array_equal(g[3], got[0][3])
            np.testing.assert_array_equal(g[4], got[0][4])


def _ref_of(chain):
    return dict(w=chain.w, z=chain.z, y=chain.y, r=chain.r, s=chain.s)


def _snap(s, resid=True):
    return s.get() + (s.residuals()[:2] if resid else ())


@functools.lru_cache(maxsize=None)
def _cold(case, alpha, iters):
    """The oracle's state after `iters` iterations from the cold start, residuals at the multiples of 4 (computed once per case)."""
    return oc.solve(CASES[case].make(), rho=CASES[case].opts["rho"], alpha=alpha, max_iter=iters, check_interval=4, stop=False)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("case", CASES)
def test_iterates_and_residuals_on_three_and_four_ranks(gpu, case, alpha):
    """After 1, 2, 3, 4, 8 and 24 iterations, residuals every 4th: the assembled iterates and every rank's r, s equal the oracle's,
    the ranks hold the same residuals, and every iteration exchanged at least once."""
    p = CASES[case].make()

    def script(s, r):
        out, done = {}, 0
        for upto in UPTO:
            every = 0 if upto < 4 else (1 if upto == 4 else 4)
            s.run(upto - done, residual_every=every)
            done = upto
            out[upto] = _snap(s, upto >= 4)
        return out

    run = run_ranks(p, _opts(case, alpha), CASES[case].world, script)
    _check_setup(case, run, p)
    if case == "I":
        assert run.wins[0]["segs_total"] % 3 == 0 and len({w["segs_total"] for w in run.wins}) == 1
        assert all(pt["auto_segments"] for pt in run.paths)
    assert run.calls > 24
    for upto in UPTO:
        _check_state(run, p, [o[upto] for o in run.outs], _cold(case, alpha, upto), (case, alpha, upto))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["A", "C"])
def test_get_writes_only_the_window(gpu, case):
    """admm_get on every rank, into arrays pre-filled with a sentinel: the rows outside the rank's window keep it, the rows inside
    are the oracle's."""
    p, alpha, iters = CASES[case].make(), 1.6, 8
    run = run_ranks(p, _opts(case, alpha), CASES[case].world, lambda s, r: (s.run(iters), read_into(s))[1])
    _check_setup(case, run, p)
    ref = _cold(case, alpha, iters)
    for got, win in zip(run.outs, run.wins):
        for a, k in zip(got, "wzy"):
            assert (outside_window(a, win, p.nb) == SENTINEL).all(), (case, win, k)
            e = np.abs(inside_window(a, win, p.nb) - inside_window(ref[k], win, p.nb)).max()
            assert e <= TOL * max(1.0, np.abs(ref[k]).max()), (case, win, k, e)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["A", "C1", "E", "F2"])
def test_warm_start_uses_the_window_rows(gpu, case):
    """Every rank is given the same full random (z, y) by admm_set_state and uses its own rows of them: 7 iterations equal the
    oracle's from that start.  admm_set_state(w) is then read back bit for bit inside the window and not at all outside it.  On
    case A admm_solve(z0, y0) follows, against the oracle's warm-started solve."""
    p, alpha = CASES[case].make(), 1.6
    rng = np.random.default_rng(11)
    Z, Y, W, Z2, Y2 = (0.3 * rng.standard_normal((p.batch, p.L)) for _ in range(5))
    kw = dict(eps_abs=1e-6, eps_rel=1e-6, check_interval=10, max_iter=120)
    with_solve = case == "A"

    def script(s, r):
        s.set_state(z=Z, y=Y)
        s.run(7, residual_every=7)
        first = _snap(s)
        s.set_state(w=W)
        back = read_into(s)
        if not with_solve:
            return first, back
        info = s.solve(z0=Z2, y0=Y2)
        return first, back, info, _snap(s)

    run = run_ranks(p, _opts(case, alpha, **kw), CASES[case].world, script)
    _check_setup(case, run, p)
    chain = OracleChain(p, CASES[case].opts["rho"], alpha).set_state(Z, Y).run(7)
    _check_state(run, p, [o[0] for o in run.outs], _ref_of(chain), (case, "set_state"))
    for o, win in zip(run.outs, run.wins):
        first, back = o[0], o[1]
        np.testing.assert_array_equal(inside_window(back[0], win, p.nb), inside_window(W, win, p.nb))
        for a, b in zip(back[1:], first[1:3]):                       # z, y are untouched by set_state(w)
            np.testing.assert_array_equal(inside_window(a, win, p.nb), inside_window(b, win, p.nb))
        for a in back:
            assert (outside_window(a, win, p.nb) == SENTINEL).all(), (case, win)
    if with_solve:
        ref = chain.set_state(Z2, Y2).solve(**kw)
        for o in run.outs:
            info = o[2]
            assert info.iters_run == ref["iters_run"] and (info.status == ref["status"]).all()
            assert (np.abs(info.iters - ref["iters"]) <= kw["check_interval"]).all()
            np.testing.assert_array_equal(info.iters, run.outs[0][2].iters)
        _check_state(run, p, [o[3] for o in run.outs], ref, (case, "solve(z0, y0)"))


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", [6, 7])
@pytest.mark.parametrize("case", ["A", "C", "C1"])
def test_update_instances_mid_run(gpu, case, first):
    """admm_update_instances between two legs (x0 alone on A; x0 and q, then q alone, on C and C'): a rank takes its own rows of q.
    The reference is the oracle on the new instance data from the state the first leg left; the first leg has an even or an odd
    count, the alternating state is reset either way."""
    p, alpha = CASES[case].make(), 1.6 if case != "A" else 1.0
    rng = np.random.default_rng(12)
    x0n = p.x0 * rng.uniform(0.6, 1.1, p.x0.shape)
    qs = [None, None] if p.q is None else [0.1 * rng.standard_normal(p.q.shape) for _ in range(2)]

    def script(s, r):
        s.run(first, residual_every=first)
        out = [_snap(s)]
        s.update_instances(x0=x0n, q=qs[0])
        s.run(6, residual_every=6)
        out.append(_snap(s))
        if qs[1] is not None:
            s.update_instances(q=qs[1])
            s.run(6, residual_every=6)
            out.append(_snap(s))
        return out

    run = run_ranks(p, _opts(case, alpha), CASES[case].world, script)
    _check_setup(case, run, p)
    chain = OracleChain(p, CASES[case].opts["rho"], alpha).run(first)
    _check_state(run, p, [o[0] for o in run.outs], _ref_of(chain), (case, first, "before"))
    chain.set_problem(dataclasses.replace(p, x0=x0n, q=qs[0])).run(6)
    _check_state(run, p, [o[1] for o in run.outs], _ref_of(chain), (case, first, "x0" if qs[0] is None else "x0, q"))
    if qs[1] is not None:
        chain.set_problem(dataclasses.replace(p, x0=x0n, q=qs[1])).run(6)
        _check_state(run, p, [o[2] for o in run.outs], _ref_of(chain), (case, first, "q"))


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["v", "zy"])
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("case", ["A", "B", "C1", "D", "E", "F3"])
def test_set_rho_mid_run(gpu, case, alpha, form):
    """admm_set_rho on every rank after 9 iterations (refactor in the rank-by-rank scan layout, y of the window rescaled), 8
    iterations, back to the first rho, 4 more.  form "v": the change meets the state as the fused kernels left it (v; z, y and w
    are rebuilt inside the call); "zy": admm_get has materialised (w, z, y) before.  (F3's three QPs saturate their thrust box
    in rank 0's window only, so y vanishes on the other ranks there: F3 checks the refactor of the matrix-vector scan, the
    rescale on interior ranks is what the other cases check.)"""
    p, rho = CASES[case].make(), CASES[case].opts["rho"]

    def script(s, r):
        if form == "v":
            s.run(9, residual_every=0)
        else:
            s.iterate(9)
            s.get()
        s.set_rho(RHO_FACTOR * rho)
        out = [s.get()]                                  # right after the change: w of the old records, y rescaled
        s.run(8, residual_every=4)
        out.append(_snap(s))
        s.set_rho(rho)
        s.run(4, residual_every=4)
        out.append(_snap(s))
        return out, s.path()["alternating"]

    run = run_ranks(p, _opts(case, alpha), CASES[case].world, script)
    _check_setup(case, run, p)
    assert all(o[1] == CASES[case].alternating for o in run.outs)        # the refactors kept the path
    chain = OracleChain(p, rho, alpha).run(9)
    w9 = chain.w
    chain.set_rho(RHO_FACTOR * rho)
    _check_state(run, p, [o[0][0] for o in run.outs], dict(w=w9, z=chain.z, y=chain.y), (case, alpha, form, "at the change"))
    chain.run(8)
    _check_state(run, p, [o[0][1] for o in run.outs], _ref_of(chain), (case, alpha, form, "after the change"))
    chain.set_rho(rho).run(4)
    _check_state(run, p, [o[0][2] for o in run.outs], _ref_of(chain), (case, alpha, form, "back"))


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", UPDATE_CASES)
def test_update_problem_mid_run(gpu, case):
    """admm_update_problem on every rank after 8 iterations: new dynamics, box, thrust bounds (per stage from then on), x0 and q;
    10 iterations equal the oracle's on the new problem from the state before.  An update with another N is then refused by every
    rank and leaves no trace: 4 further iterations continue the chain."""
    p, alpha = CASES[case].make(), 1.6
    p2 = second_problem(p)
    other = _other_horizon(p)

    def script(s, r):
        s.run(8)
        out = [_snap(s, False)]
        s.update_problem(p2)
        s.run(10, residual_every=5)
        out.append(_snap(s))
        code = 0
        try:
            s.update_problem(other)
        except AdmmError as e:
            code = e.code
        s.run(4, residual_every=4)
        out.append(_snap(s))
        return out, code

    run = run_ranks(p, _opts(case, alpha), CASES[case].world, script)
    _check_setup(case, run, p)
    assert [o[1] for o in run.outs] == [INVALID] * CASES[case].world
    chain = OracleChain(p, CASES[case].opts["rho"], alpha).run(8)
    _check_state(run, p, [o[0][0] for o in run.outs], _ref_of(chain), (case, "before"))
    chain.set_problem(p2).run(10)
    _check_state(run, p, [o[0][1] for o in run.outs], _ref_of(chain), (case, "updated"))
    chain.run(4)
    _check_state(run, p, [o[0][2] for o in run.outs], _ref_of(chain), (case, "after the refused update"))


def _other_horizon(p):
    """p's kind of problem with one stage more (what admm_update_problem refuses)."""
    if p.q is not None:
        return pkg.random_ltv(N=p.N + 1, n=p.n, m=p.m, batch=p.batch, seed=1)
    return pkg.cw_rendezvous(N=p.N + 1, batch=p.batch, thrust_norm=p.unorm is not None)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ADAPT)
def test_adaptive_solve_on_three_ranks(gpu, case):
    """admm_solve with the adaptive rho rule and over-relaxation: every rank runs the oracle's iteration count, ends at its rho
    after as many changes (two at least), reports its statuses, and the ranks agree bit for bit on r, s and the per-QP counts."""
    p = CASES[case].make()
    kw = dict(rho=ADAPT[case]["rho"], alpha=1.6, eps_abs=1e-6, eps_rel=1e-6, max_iter=ADAPT[case]["max_iter"], check_interval=10,
              adapt_interval=20)
    ref = oc.solve(p, **kw)
    assert ref["rho_updates"] >= 2 and ref["rho"] != kw["rho"]

    def script(s, r):
        info = s.solve()
        return _snap(s, False), info

    run = run_ranks(p, dict(CASES[case].opts, **kw), CASES[case].world, script)
    _check_setup(case, run, p)
    assert run.calls >= ref["iters_run"]
    first = run.outs[0][1]
    for got, info in run.outs:
        assert (info.iters_run, info.rho, info.rho_updates) == (ref["iters_run"], ref["rho"], ref["rho_updates"])
        assert (info.status == ref["status"]).all() and info.n_converged == int(ref["status"].sum())
        assert (np.abs(info.iters - ref["iters"]) <= kw["check_interval"]).all()
        assert np.abs(info.r - ref["r"]).max() <= TOL and np.abs(info.s - ref["s"]).max() <= TOL
        for a, b in ((info.r, first.r), (info.s, first.s), (info.iters, first.iters), (info.status, first.status)):
            np.testing.assert_array_equal(a, b)
    _check_state(run, p, [o[0] for o in run.outs], ref, case)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------

def test_full_arrays_twin(gpu, monkeypatch):
    """ADMM_TS_FULL_ARRAYS=1 (every rank allocates the whole horizon, no pointer is biased) against the windowed handles on case A:
    the window rows are the same bit for bit after 10 iterations, a rho change and 6 more."""
    p, rho, alpha = CASES["A"].make(), CASES["A"].opts["rho"], 1.6

    def script(s, r):
        s.run(10, residual_every=5)
        s.set_rho(RHO_FACTOR * rho)
        s.run(6, residual_every=3)
        return read_into(s) + s.residuals()[:2]

    windowed = run_ranks(p, _opts("A", alpha), CASES["A"].world, script)
    monkeypatch.setenv("ADMM_TS_FULL_ARRAYS", "1")
    full = run_ranks(p, _opts("A", alpha), CASES["A"].world, script)
    monkeypatch.delenv("ADMM_TS_FULL_ARRAYS")
    _check_setup("A", windowed, p)
    assert full.wins == windowed.wins
    for a, b, win in zip(windowed.outs, full.outs, windowed.wins):
        for x, y in zip(a[:3], b[:3]):
            np.testing.assert_array_equal(inside_window(x, win, p.nb), inside_window(y, win, p.nb))
            assert (outside_window(x, win, p.nb) == SENTINEL).all()
            assert not (y == SENTINEL).any()                        # the twin holds, and writes, every row
        np.testing.assert_array_equal(a[3], b[3])
        np.testing.assert_array_equal(a[4], b[4])


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------

def _refused_calls(s, dev):
    """Every call include/admm_hip.h refuses on a time shard, made on handle s: [(name, status)].  dev: (DeviceProblem, zeros)."""
    lib, out = s._lib, []
    for name, call in (("step_z", lambda: s.step_z()), ("profile", lambda: s.profile(1)), ("mpc_advance", lambda: s.mpc_advance()),
                       ("certificate", lambda: s.certificate()), ("probe_infeasibility", lambda: s.infeasibility(span=2))):
        try:
            call()
            out.append((name, 0))
        except AdmmError as e:
            out.append((name, e.code))
    dp, zero = dev
    cp, keep = _abi.marshal_device_problem(dp)
    stream = C.c_void_p(torch.cuda.current_stream("cuda:0").cuda_stream)
    ptr = lambda t: C.cast(C.c_void_p(t.data_ptr()), _abi.c_double_p)
    out += [("update_problem_device", lib.admm_update_problem_device(s._h, C.byref(cp), stream)),
            ("update_instances_device", lib.admm_update_instances_device(s._h, ptr(dp.x0), None, stream)),
            ("set_state_device", lib.admm_set_state_device(s._h, None, ptr(zero), None, stream)),
            ("get_device", lib.admm_get_device(s._h, None, ptr(zero), None, stream))]
    del keep
    return out


def test_lifecycle_on_an_interior_rank(gpu):
    """One chain on case C', four ranks: run, set_state, run, update_instances, run, set_rho, run, update_problem, solve -- compared
    with the oracle chain after every step.  Between the steps rank 1 (interior) makes every call the header refuses on a time
    shard; each is ADMM_ERR_UNSUPPORTED and none leaves a trace in what follows."""
    case, alpha = "C1", 1.6
    p, rho = CASES[case].make(), CASES[case].opts["rho"]
    p2 = second_problem(p)
    rng = np.random.default_rng(13)
    Z, Y = (0.3 * rng.standard_normal((p.batch, p.L)) for _ in range(2))
    x0n, qn = p.x0 * 0.8, 0.1 * rng.standard_normal(p.q.shape)
    kw = dict(eps_abs=1e-6, eps_rel=1e-6, check_interval=10, max_iter=80)
    dev = (pkg.DeviceProblem.from_problem(p, "cuda:0"), torch.zeros((p.batch, p.L), dtype=torch.float64, device="cuda:0"))

    def script(s, r):
        out, refused = [], []

        def step(fn, iters):
            fn()
            if iters:
                s.run(iters, residual_every=iters)
            out.append(_snap(s, bool(iters)))
            if r == 1:
                refused.extend(_refused_calls(s, dev))

        step(lambda: None, 5)
        step(lambda: s.set_state(z=Z, y=Y), 4)
        step(lambda: s.update_instances(x0=x0n, q=qn), 5)
        step(lambda: s.set_rho(RHO_FACTOR * rho), 6)
        step(lambda: s.update_problem(p2), 3)
        info = s.solve()
        out.append(_snap(s, False))
        return out, refused, info

    run = run_ranks(p, _opts(case, alpha, **kw), CASES[case].world, script)
    _check_setup(case, run, p)
    assert 0 < run.wins[1]["stage_lo"] and run.wins[1]["stage_hi"] < p.N
    refused = run.outs[1][1]
    assert len(refused) == 5 * 9 and all(code == UNSUPPORTED for _, code in refused), refused
    got = lambda i: [o[0][i] for o in run.outs]
    chain = OracleChain(p, rho, alpha).run(5)
    _check_state(run, p, got(0), _ref_of(chain), "run")
    chain.set_state(Z, Y).run(4)
    _check_state(run, p, got(1), _ref_of(chain), "set_state")
    chain.set_problem(dataclasses.replace(p, x0=x0n, q=qn)).run(5)
    _check_state(run, p, got(2), _ref_of(chain), "update_instances")
    chain.set_rho(RHO_FACTOR * rho).run(6)
    _check_state(run, p, got(3), _ref_of(chain), "set_rho")
    chain.set_problem(p2).run(3)
    _check_state(run, p, got(4), _ref_of(chain), "update_problem")
    ref = chain.solve(**kw)
    for o in run.outs:
        assert o[2].iters_run == ref["iters_run"] and (o[2].status == ref["status"]).all()
        assert (np.abs(o[2].iters - ref["iters"]) <= kw["check_interval"]).all()
    _check_state(run, p, got(5), ref, "solve")


# ---- 10 -----------------------------------------------------------------------------------------------------------------------------

def test_setup_refusals_and_failing_exchange(gpu):
    """What admm_setup_timeshard refuses, and an exchange callback that fails: the collective call fails with ADMM_ERR_HIP naming
    the callback, and the handle can still be freed.  One handle, one rank: nothing here can wait for a peer."""
    p = CASES["A"].make()
    never = _abi.EXCHANGE_FN(lambda ctx, stream, op, buf, count: 1)

    def code_of(problem, rank, world, fn, **opts):
        with pytest.raises(AdmmError) as e:
            Solver(problem, Options(rho=0.05, **opts), timeshard=(rank, world, fn))
        return e.value.code

    assert code_of(p, 0, 3, never, segments=7) == INVALID
    assert code_of(pkg.cw_rendezvous(N=2, batch=4), 0, 3, never) == INVALID
    assert code_of(p, 3, 3, never, segments=6) == INVALID
    assert code_of(p, 0, 2, None, segments=6) == INVALID
    assert code_of(p, 0, 3, never, segments=6, flags=_abi.FLAG_UNFUSED) == UNSUPPORTED
    assert code_of(p, 0, 3, never, segments=6, flags=_abi.FLAG_GRAPH) == UNSUPPORTED
    assert code_of(pkg.random_instances(N=12, n=6, m=3, batch=4, seed=1), 0, 3, never, segments=6) == UNSUPPORTED

    calls = []

    def failing(ctx, stream, op, buf, count):
        calls.append((op, count))
        return 1

    fn = _abi.EXCHANGE_FN(failing)
    s = Solver(p, Options(rho=0.05, segments=6), timeshard=(0, 2, fn))
    try:
        with pytest.raises(AdmmError) as e:
            s.run(1)
        assert e.value.code == HIP_ERROR and "exchange callback" in str(e.value)
        assert calls and calls[0][0] == _abi.EXCHANGE_ALLGATHER
    finally:
        s.close()
    assert not s._h.value
