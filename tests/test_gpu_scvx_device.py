"""The outer step of the batched successive-convexification loop on the device (ADMM_HIP_HAS_SCVX) against the
host code it mirrors: scvx.rollout, scvx.linearise, scvx.correction_qp_batch, scvx.outer_update and scvx_batch itself; under a
general parameter set (dense weights, a per-axis asymmetric box, other model settings) against a long-double restatement of the
model; across the shape edges of the advance kernel; over whole loops in lockstep with a host model; and on a caller's stream.
Inputs and host references: tests/_scvx_device_case.py (built once, shared, read-only)."""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch          # before libadmm_hip.so is loaded (the `gpu` fixture): both then share one HIP runtime, as in test_gpu_device_io.py

from admm_library_amd import _abi
from admm_library_amd import scvx as sc

import _scvx_case as case
import _scvx_device_case as dc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = 1


def _loop(x0, N, **kw):
    kw = dict(dict(device=DEV, tol=dc.TOL, rho_reject=dc.RHO_REJECT, rho_expand=dc.RHO_EXPAND), **kw)
    return sc.DeviceOuterStep(x0, N, dc.DT, case.Q, case.R, case.QN, -case.U_MAX, case.U_MAX, **kw)


def _loop_p(x0, N, p, **kw):
    """The loop object under a parameter set of tests/_scvx_device_case.py."""
    kw = dict(dict(device=DEV, tol=dc.TOL, rho_reject=dc.RHO_REJECT, rho_expand=dc.RHO_EXPAND, substeps=p.substeps, rc=p.rc, eps=p.fd_eps), **kw)
    return sc.DeviceOuterStep(x0, N, p.dt, *(np.array(a) for a in (p.Q, p.R, p.QN, p.u_lo, p.u_hi)), **kw)     # copies: the sets are read-only


def _t(a, dtype=None):
    return torch.as_tensor(np.array(a, dtype), device=DEV)


def _prepared(B, N):
    """prepare() about the scattered reference of (B, N): the loop object, its tensors copied to the host."""
    x0, u, x, tru, trx, active = dc.scattered(B, N)
    loop = _loop(x0, N)
    for k, a in (("ub", u), ("xb", x), ("tr_u", tru), ("tr_x", trx)):
        loop.t[k].copy_(_t(a))
    loop.t["active"].copy_(_t(active, np.int32))
    loop.prepare()
    return {k: getattr(loop, k).cpu().numpy().reshape((B, N, 9) if k == "q" else tuple(getattr(loop, k).shape)) for k in ("A", "B", "lo", "hi", "q")}


@pytest.mark.parametrize("B,N", dc.SHAPES)
def test_rollout_matches_the_host_rollout(gpu, B, N):
    """admm_scvx_rollout_device vs scvx.rollout: max abs <= 5e-11 -- 10x what NumPy fp64 itself differs from an 80-bit evaluation of
    the same formulas on these inputs (4.0 - 4.4e-12, states up to 165 km); the r2 sqrt(r2) form differs from NumPy by 2.7 - 3.3e-12."""
    x0, u, x, *_ = dc.scattered(B, N)
    got = _loop(x0, N).rollout(_t(u)).cpu().numpy()
    err = np.abs(got - x).max()
    print(f"rollout B={B} N={N}: max abs err {err:.3e}")
    assert got.shape == x.shape and err <= 5e-11


@pytest.mark.parametrize("B,N", dc.SHAPES)
def test_linearisation_matches_the_host_central_differences(gpu, B, N):
    """A, B of admm_scvx_prepare_device vs scvx.linearise: max abs <= 5e-7 (central differences at eps = 1e-6 amplify the rollout's
    rounding by 5e5; NumPy vs longdouble is 4 - 6e-8, entries are O(1)); and each A block is its own, not its transpose."""
    A, Bm = dc.linearised(B, N)[:2]
    got = _prepared(B, N)
    eA, eB = np.abs(got["A"] - A).max(), np.abs(got["B"] - Bm).max()
    print(f"linearise B={B} N={N}: max abs err A {eA:.3e}, B {eB:.3e}")
    assert eA <= 5e-7 and eB <= 5e-7
    own = np.abs(got["A"] - A).max(axis=(2, 3))
    swapped = np.abs(got["A"] - np.swapaxes(A, -1, -2)).max(axis=(2, 3))
    assert (swapped - own >= 1e-3).all()


@pytest.mark.parametrize("B,N", dc.SHAPES)
def test_assembly_matches_the_host_qp(gpu, B, N):
    """lo, hi of prepare equal correction_qp_batch's exactly (only subtract, min, max), q within 1e-13 relative; the radii differ
    per trajectory and every fifth trajectory is inactive (zero-width box)."""
    _, _, lo, hi, q = dc.linearised(B, N)
    active = dc.scattered(B, N)[5]
    got = _prepared(B, N)
    np.testing.assert_array_equal(got["lo"], lo)
    np.testing.assert_array_equal(got["hi"], hi)
    off = ~active
    assert (got["lo"][off] == 0).all() and (got["hi"][off] == 0).all() and (B == 1 or off.any())
    err = np.abs(got["q"] - q).max() / np.abs(q).max()
    print(f"assembly B={B} N={N}: q max rel err {err:.3e}")
    assert np.abs(got["q"] - q).max() <= 1e-13 * np.abs(q).max()


def _prepared_general(B, N, substeps):
    """prepare() about scattered_general(B, N, substeps) under GENERAL[substeps]: A, B, lo, hi, q copied to the host."""
    x0, u, x, tru, trx, active = dc.scattered_general(B, N, substeps)
    loop = _loop_p(x0, N, dc.GENERAL[substeps])
    for k, a in (("ub", u), ("xb", x), ("tr_u", tru), ("tr_x", trx)):
        loop.t[k].copy_(_t(a))
    loop.t["active"].copy_(_t(active, np.int32))
    loop.prepare()
    return {k: getattr(loop, k).cpu().numpy().reshape((B, N, 9) if k == "q" else tuple(getattr(loop, k).shape)) for k in ("A", "B", "lo", "hi", "q")}


def _ld_err(got, ref):
    return float(np.abs(got.astype(np.longdouble) - ref).max())


@pytest.mark.parametrize("substeps", [1, 3])
@pytest.mark.parametrize("B,N", dc.SHAPES)
def test_general_rollout_matches_the_long_double_rollout(gpu, B, N, substeps):
    """admm_scvx_rollout_device under GENERAL[substeps] (substeps 1 | 3, rc 7000, dt 2 pi / 60) vs the long-double rollout: max abs
    <= 10 x what NumPy fp64 differs from it on these inputs (_scvx_device_case.FP64_VS_LD)."""
    x0, u, *_ = dc.scattered_general(B, N, substeps)
    got = _loop_p(x0, N, dc.GENERAL[substeps]).rollout(_t(u)).cpu().numpy()
    ref = dc.reference_general(B, N, substeps)["ld"]["x"]
    err, c = _ld_err(got, ref), dc.FP64_VS_LD[substeps, B, N]["x"]
    print(f"general rollout substeps={substeps} B={B} N={N}: max abs err {err:.3e} (NumPy {c:.1e}, bound {dc.GPU_MARGIN * c:.1e})")
    assert got.shape == ref.shape and err <= dc.GPU_MARGIN * c


@pytest.mark.parametrize("substeps", [1, 3])
@pytest.mark.parametrize("B,N", dc.SHAPES)
def test_general_linearisation_matches_the_long_double_central_differences(gpu, B, N, substeps):
    """A, B of prepare under GENERAL[substeps] (fd_eps = 1e-5) vs long-double central differences of the long-double step: max abs
    <= 10 x NumPy's own distance (which contains the 1 / (2 fd_eps) amplification); each A block is its own, not its transpose."""
    ref, c = dc.reference_general(B, N, substeps)["ld"], dc.FP64_VS_LD[substeps, B, N]
    got = _prepared_general(B, N, substeps)
    eA, eB = _ld_err(got["A"], ref["A"]), _ld_err(got["B"], ref["B"])
    print(f"general linearise substeps={substeps} B={B} N={N}: max abs err A {eA:.3e} (NumPy {c['A']:.1e}, bound {dc.GPU_MARGIN * c['A']:.1e}), "
          f"B {eB:.3e} (NumPy {c['B']:.1e}, bound {dc.GPU_MARGIN * c['B']:.1e})")
    assert eA <= dc.GPU_MARGIN * c["A"] and eB <= dc.GPU_MARGIN * c["B"]
    A = np.asarray(ref["A"], np.float64)
    own = np.abs(got["A"] - A).max(axis=(2, 3))
    swapped = np.abs(got["A"] - np.swapaxes(A, -1, -2)).max(axis=(2, 3))
    assert (swapped - own >= 1e-3).all()


@pytest.mark.parametrize("substeps", [1, 3])
@pytest.mark.parametrize("B,N", dc.SHAPES)
def test_general_assembly_matches_the_long_double_linear_term(gpu, B, N, substeps):
    """lo, hi of prepare under the per-axis asymmetric box equal correction_qp_batch's exactly; q vs the long-double (R ub, Q xb),
    QN at the last stage: max abs <= 10 x NumPy's own distance.  And q is built from the whole of Q, R, QN and from QN at the last
    stage: per block of rows (R's, Q's, QN's) the device is farther, by >= 1e-3 of the block's largest entry, from the q of the
    diagonals alone and from the q with Q at the last stage than from the reference."""
    r = dc.reference_general(B, N, substeps)
    active = dc.scattered_general(B, N, substeps)[5]
    got = _prepared_general(B, N, substeps)
    np.testing.assert_array_equal(got["lo"], r["lo"])
    np.testing.assert_array_equal(got["hi"], r["hi"])
    off = ~active
    assert (got["lo"][off] == 0).all() and (got["hi"][off] == 0).all() and (B == 1 or off.any())
    err, c = _ld_err(got["q"], r["ld"]["q"]), dc.FP64_VS_LD[substeps, B, N]["q"]
    print(f"general assembly substeps={substeps} B={B} N={N}: q max abs err {err:.3e} (NumPy {c:.1e}, bound {dc.GPU_MARGIN * c:.1e})")
    assert err <= dc.GPU_MARGIN * c
    q = np.asarray(r["ld"]["q"], np.float64)
    blocks = {"R": (slice(None), slice(0, 3)), "QN": (slice(N - 1, N), slice(3, 9))}
    if N > 1:
        blocks["Q"] = (slice(0, N - 1), slice(3, 9))
    for name, (ks, rows) in blocks.items():
        own = np.abs(got["q"][:, ks, rows] - q[:, ks, rows]).max()
        scale = np.abs(q[:, ks, rows]).max()
        for wrong in ("q_diag",) + (("q_qlast",) if name == "QN" else ()):
            other = np.abs(got["q"][:, ks, rows] - r[wrong][:, ks, rows]).max()
            assert other - own >= 1e-3 * scale, (name, wrong, other, own, scale)


def _record_matches(row, rec, where):
    """One history record of the device (the 9 doubles) against outer_update's: flags, radii and du_max equal; doubles within 1e-12
    relative, where the scale of a DIFFERENCE of costs (predicted, actual) is that of the costs it is formed from, |J|, and the
    ratio's bound is that of its operands propagated: 1e-12 |J| (1 + |ratio|) / |predicted|.  Returns |device - host| / |J| per field."""
    row = dict(zip(_abi.SCVX_HISTORY_FIELDS, row))
    assert bool(row["accepted"]) == rec["accepted"] and row["accepted"] in (0.0, 1.0), where
    assert row["tr_u"] == rec["tr_u"] and row["tr_x"] == rec["tr_x"], where
    assert row["du_max"] == rec["du_max"], where                   # a maximum of |du|: exact
    J = abs(rec["cost"])
    bounds = dict(cost=1e-12 * J, cost_candidate=1e-12 * J, predicted=1e-12 * J, actual=1e-12 * J)
    for k, bound in bounds.items():
        assert abs(row[k] - rec[k]) <= bound, (where, k, row[k], rec[k])
    if abs(rec["predicted"]) <= 1e-12 * J:
        # predicted is a rounding residue of J - J (0 on the host): its sign, and so ratio = -inf or actual / predicted, is noise
        assert abs(row["predicted"]) <= 1e-12 * J, where
    elif rec["predicted"] < 0:
        assert row["ratio"] == rec["ratio"] == -np.inf, (where, row, rec)
    else:
        assert abs(row["ratio"] - rec["ratio"]) <= 1e-12 * J * (1.0 + abs(rec["ratio"])) / abs(rec["predicted"]), (where, row, rec)
    return {k: abs(row[k] - rec[k]) / J for k in bounds}


def _check_decisions(state, ref, taken, p):
    """One advance call on `state` under the parameter set p against the host reference `ref` (tests/_scvx_device_case.
    decision_inputs).  Flags, counts and radii are equal; doubles agree within 1e-12 relative (_record_matches); the candidate's
    controls are equal, its states within 5e-11; what the call has no business with -- inactive trajectories, the other history rows
    -- holds the bits it held."""
    B, N = state["ub"].shape[:2]
    cap = int(ref["outer"].max()) + 1
    loop = _loop_p(state["x0"], N, p, max_outer=cap)
    junk = dc.decision_junk(B, N, cap)
    assert {k: tuple(loop.t[k].shape) for k in junk} == {k: v.shape for k, v in junk.items()}
    for k in ("ub", "xb", "J", "tr_u", "tr_x"):
        loop.t[k].copy_(_t(state[k]))
    for k in ("active", "converged", "accepted", "outer"):
        loop.t[k].copy_(_t(state[k], np.int32))
    for k, a in junk.items():
        loop.t[k].copy_(_t(a))
    loop.t["take"].fill_(7)
    n_active = loop.advance(_t(state["z"].reshape(B, N * 9)))
    got = {k: v.cpu().numpy() for k, v in loop.t.items()}

    assert n_active == int(ref["active"].sum())
    for k in ("active", "converged", "accepted", "outer", "take"):
        np.testing.assert_array_equal(got[k], ref[k].astype(np.int32), err_msg=k)
    np.testing.assert_array_equal(got["tr_u"], ref["tr_u"])
    np.testing.assert_array_equal(got["tr_x"], ref["tr_x"])
    scale = np.abs(state["J"])
    assert (np.abs(got["J"] - ref["J"]) <= 1e-12 * scale).all()
    worst = {}
    for b in range(B):
        it = int(state["outer"][b])
        if not state["active"][b]:        # untouched, bit for bit: reference, cost, candidates, every history row
            for k in ("ub", "xb", "J"):
                np.testing.assert_array_equal(got[k][b], state[k][b])
            for k in junk:
                np.testing.assert_array_equal(got[k][:, b] if k == "history" else got[k][b], junk[k][:, b] if k == "history" else junk[k][b])
            continue
        others = np.delete(np.arange(cap), it)
        np.testing.assert_array_equal(got["history"][others, b], junk["history"][others, b])
        for k, v in _record_matches(got["history"][it, b], ref["records"][b], b).items():
            worst[k] = max(worst.get(k, 0.0), v)
        # the candidate; the reference takes it where accepted
        assert np.abs(got["u_cand"][b] - ref["u_new"][b]).max() == 0.0
        assert np.abs(got["x_cand"][b] - ref["x_new"][b]).max() <= dc.ROLLOUT_BOUND
        if ref["take"][b]:
            np.testing.assert_array_equal(got["ub"][b], got["u_cand"][b])
            np.testing.assert_array_equal(got["xb"][b], got["x_cand"][b])
        else:
            np.testing.assert_array_equal(got["ub"][b], state["ub"][b])
            np.testing.assert_array_equal(got["xb"][b], state["xb"][b])
    print(f"decisions B={B} N={N} {p.name}: worst |device - host| / |J| per field:", {k: f"{v:.2e}" for k, v in worst.items()})


def test_decisions_match_outer_update_on_every_branch(gpu):
    """One advance call, B = 66, N = 9, against scvx.outer_update on the same inputs (tests/_scvx_device_case.decision_inputs: the
    HOST reference takes every branch, 11 trajectories each -- asserted first).  Flags, counts and radii are equal; doubles agree
    within 1e-12 relative, where the scale of a DIFFERENCE of costs (predicted, actual) is that of the costs it is formed from, |J|,
    and the ratio's bound is that of its operands propagated: 1e-12 |J| (1 + |ratio|) / |predicted|."""
    state, ref = dc.decision_inputs()
    B, N = state["ub"].shape[:2]
    taken = [dc.branch_of(b, state, ref) for b in range(B)]
    assert {t: taken.count(t) for t in dc.BRANCHES} == {t: 11 for t in dc.BRANCHES}
    ratios = np.array([r["ratio"] for r in ref["records"].values() if np.isfinite(r["ratio"])])
    assert min(np.abs(ratios - dc.RHO_REJECT).min(), np.abs(ratios - dc.RHO_EXPAND).min()) > 1e-3       # no decision on a knife's edge
    _check_decisions(state, ref, taken, dc.ORIGINAL)


@pytest.mark.parametrize("B,N,params", [(B, N, name) for B, N in dc.DECISION_SHAPES for name in dc.DECISION_PARAMS
                                        if (B, N, name) != (66, 9, "original")])      # that one: the test above
def test_decisions_across_the_shape_edges_of_the_advance_kernel(gpu, B, N, params):
    """The comparison of test_decisions_match_outer_update_on_every_branch at the edges of scvx_advance_kernel -- a lone lane with
    one stage; N below one LDS chunk of 4 stages; an exact wave with an exact chunk; a wave + 1 with two exact chunks; four waves
    (the per-wave atomicAdd into n_active, the row_on masking of the chunk stores past the first wave) with one stage left over;
    today's shape -- under the scenario's parameters and under GENERAL at both substeps (dense weights in both costs, the candidate
    clipped to a per-axis asymmetric box).  Asserted on the HOST reference first: every branch is taken >= B // 6 times (the lone
    trajectory is accepted), no ratio within 1e-3 of a threshold, and under GENERAL the reversed step of the rejected branch is
    clipped to u_lo and to u_hi on every axis."""
    p = dc.PARAMS[params]
    state, ref = dc.decision_inputs(B, N, params)
    taken = [dc.branch_of(b, state, ref) for b in range(B)]
    counts = {t: taken.count(t) for t in dc.BRANCHES}
    if B == 1:
        assert taken == ["accepted"], f"precondition (branch counts) failed: {counts}"
    else:
        assert all(c >= B // 6 for c in counts.values()), f"precondition (branch counts) failed: {counts}"
    margin = dc.ratio_margin(ref["records"].values())
    assert margin > 1e-3, f"precondition (knife-edge margin) failed: a ratio lies within {margin:.3e} of a threshold"
    if params != "original" and B >= 6:
        below, above, exact = dc.clip_activity(state, ref, p)
        assert (below >= 1).all() and (above >= 1).all() and exact, f"precondition (clip activity) failed: {below} below u_lo, {above} above u_hi"
    if B >= 66:
        assert (np.flatnonzero(~state["active"]) > 63).any(), "precondition failed: no inactive trajectory past the first wave"
    _check_decisions(state, ref, taken, p)


def test_end_to_end_matches_the_host_outer_loop(gpu):
    """scvx_batch(outer_on_device=True) vs scvx_batch(qp_data_on_device=True) (the host outer loop), both on the GPU solver, 66
    trajectories of the shared scenario: every trajectory converges, outer_iterations and accepted agree per trajectory, cost within
    1e-6 relative and |u| within 1e-2 (the criteria tests/test_gpu_scvx.py applies between two QP solvers), x is the nonlinear
    trajectory under u within 5e-11.
    Equal decision counts are safe to ask for: with the host loop and the CPU oracle as QP solver, trajectories 0, 17, 33, 49, 65 of
    this batch have every finite ratio in [0.9993, 1.2148] -- 0.299 from rho_expand = 0.7 and 0.899 from rho_reject = 0.1, against
    the 1e-3 asked for -- and stop on predicted <= tol |J| with |predicted| ~ 3e-5 against a threshold of 1e-3."""
    rng = np.random.default_rng(11)
    B = 66
    x0s = case.X0[None] * (1.0 + 0.05 * rng.standard_normal((B, 6)))
    args = (x0s, case.N, case.DT, case.Q, case.R, case.QN, -case.U_MAX, case.U_MAX)
    ref = sc.scvx_batch(*args, qp_options=case.QP, linearise_on=DEV, qp_data_on_device=True, **case.SCVX)
    res = sc.scvx_batch(*args, qp_options=case.QP, linearise_on=DEV, outer_on_device=True, **case.SCVX)
    assert len(res) == B and all(r.converged for r in res) and all(r.converged for r in ref)
    worst_cost = worst_u = worst_x = 0.0
    for r, o, x0 in zip(res, ref, x0s):
        assert r.outer_iterations == o.outer_iterations == len(r.history) and r.accepted == o.accepted
        assert [h["accepted"] for h in r.history] == [h["accepted"] for h in o.history]
        assert [h["iteration"] for h in r.history] == list(range(1, r.outer_iterations + 1))
        worst_cost = max(worst_cost, abs(r.cost - o.cost) / abs(o.cost))
        worst_u = max(worst_u, np.abs(r.u - o.u).max())
        worst_x = max(worst_x, np.abs(r.x - sc.rollout(x0, r.u, case.DT)).max())
        assert (np.abs(r.u) <= case.U_MAX).all()
    print(f"end to end: cost rel {worst_cost:.3e}, |u| {worst_u:.3e}, x vs host rollout {worst_x:.3e}")
    assert worst_cost <= 1e-6 and worst_u <= 1e-2 and worst_x <= 5e-11


def test_whole_loops_in_lockstep_with_a_host_model(gpu):
    """The real device loop -- init, then max_outer = 8 rounds of prepare -> GPU QP solve -> advance -- on 70 trajectories of 13 stages
    whose x0 are the scenario's scaled 1x .. 8x (tests/_scvx_device_case.LOCKSTEP: GENERAL[3] with a ten times wider box and longer
    stages, so that the linear model errs), and a host model (HostLoop) that repeats every outer iteration in the host formulas
    from the same z and from nothing else of the device's.  The run is made first and everything downloaded; then the preconditions
    are asserted on the HOST model's records (lockstep_preconditions: accept + expand, accept + keep, reject, model-converged stop
    and still-active-at-the-cap all occur; a reject is followed by an accept; trajectories stop at two different iterations or more;
    no deciding ratio within 1e-3 of a threshold, no predicted decrease within a factor 2 of the stop threshold -- all of which
    tests/test_scvx_device_host.py has at ten times the margin with the CPU oracle); then, per outer iteration:
      prepare   lo, hi equal correction_qp_batch's about the host's own state; A, B within 10 x LOCKSTEP_FP64_VS_LD (what NumPy
                differs from long double on this run's inputs, ten times larger than part 1's); q within 10 x its constant plus what
                the weights make of the 5e-11 the two references xb may differ by (max row sum of |QN| x 5e-11)
      advance   flags, counts, take, radii, ub and n_active equal; xb within 5e-11, J within 1e-12 |J|, the new history row as in the
                decision test; every other history row, and the candidate of a trajectory that was inactive, hold their bits.
    At the end a trajectory still active has outer = history_capacity: one more advance is refused and touches nothing."""
    c = dc.LOCKSTEP
    p, host = dc.lockstep_params(), dc.lockstep_host()
    B, N, cap = c["B"], c["N"], c["max_outer"]
    loop = _loop_p(host.x0, N, p, tol=c["tol"], max_outer=cap)
    rng = np.random.default_rng(5)
    for k in ("u_cand", "x_cand", "history"):
        loop.t[k].copy_(_t(rng.standard_normal(tuple(loop.t[k].shape))))
    loop.init(c["tr_u"], c["tr_x"])
    solve = sc.gpu_qp_solver(True, z_on_device=True, **dc.LOCKSTEP_QP)

    def state_of(h):
        return {k: np.array(getattr(h, k)) for k in ("ub", "xb", "J", "tr_u", "tr_x", "active", "converged", "accepted", "outer")}
    dev = [{k: v.cpu().numpy() for k, v in loop.t.items()}]        # the device's tensors after init and after each advance ...
    hst = [state_of(host)]                                          # ... and the host model's state at the same points
    qps, outs, counts = [], [], []
    t0 = time.perf_counter()
    for it in range(cap):
        prob = loop.prepare()
        qps.append(({k: getattr(loop, k).cpu().numpy().reshape((B, N, 9) if k == "q" else tuple(getattr(loop, k).shape))
                     for k in ("A", "B", "lo", "hi", "q")}, host.qp()))
        z, _ = solve(prob)
        counts.append(loop.advance(z))
        outs.append(host.advance(z.cpu().numpy(), it))
        dev.append({k: v.cpu().numpy() for k, v in loop.t.items()})
        hst.append(state_of(host))
    print(f"lockstep: {cap} outer iterations of B={B} N={N} in {time.perf_counter() - t0:.2f} s")

    seen = dc.lockstep_preconditions(host)                          # on the host model's records; names what failed
    print("lockstep:", {k: v for k, v in seen.items() if k != "mixed"}, f"{len(seen['mixed'])} trajectories with mixed sequences")

    def same_state(d, h, what):
        for k in ("active", "converged", "accepted", "outer"):
            np.testing.assert_array_equal(d[k], h[k].astype(np.int32), err_msg=f"{what}: {k}")
        for k in ("tr_u", "tr_x", "ub"):
            np.testing.assert_array_equal(d[k], h[k], err_msg=f"{what}: {k}")
        ex, eJ = np.abs(d["xb"] - h["xb"]).max(), (np.abs(d["J"] - h["J"]) / np.abs(h["J"])).max()
        assert ex <= dc.ROLLOUT_BOUND and eJ <= 1e-12, (what, ex, eJ)
        return ex, eJ
    worst = dict(zip(("xb", "J"), same_state(dev[0], hst[0], "after init")))
    worst.update(A=0.0, B=0.0, q=0.0, x_cand=0.0)
    assert (dev[0]["take"] == 0).all()
    bound = {k: dc.GPU_MARGIN * v for k, v in dc.LOCKSTEP_FP64_VS_LD.items()}
    bound["q"] += max(np.abs(M).sum(axis=1).max() for M in (p.Q, p.QN)) * dc.ROLLOUT_BOUND
    for it in range(cap):
        got, want = qps[it]
        np.testing.assert_array_equal(got["lo"], want.lo, err_msg=f"iteration {it}: lo")
        np.testing.assert_array_equal(got["hi"], want.hi, err_msg=f"iteration {it}: hi")
        off = ~hst[it]["active"]
        assert (got["lo"][off] == 0).all() and (got["hi"][off] == 0).all()
        for k, w in (("A", want.A), ("B", want.B), ("q", want.q.reshape(B, N, 9))):
            e = np.abs(got[k] - w).max()
            worst[k] = max(worst[k], e)
            assert e <= bound[k], (it, k, e, bound[k])
        d, d0, out, was = dev[it + 1], dev[it], outs[it], outs[it]["was_active"]
        assert counts[it] == int(hst[it + 1]["active"].sum()), it
        np.testing.assert_array_equal(d["take"], out["take"].astype(np.int32), err_msg=f"iteration {it}: take")
        ex, eJ = same_state(d, hst[it + 1], f"iteration {it}")
        worst["xb"], worst["J"] = max(worst["xb"], ex), max(worst["J"], eJ)
        for b in range(B):
            row = int(hst[it]["outer"][b])
            rows = np.arange(cap) != row if was[b] else np.ones(cap, bool)
            np.testing.assert_array_equal(d["history"][rows, b], d0["history"][rows, b], err_msg=f"iteration {it}, trajectory {b}: older history rows")
            if not was[b]:
                np.testing.assert_array_equal(d["u_cand"][b], d0["u_cand"][b])
                np.testing.assert_array_equal(d["x_cand"][b], d0["x_cand"][b])
                continue
            assert row == it                                         # active so far: one record per outer iteration
            rec = out["records"][b]
            for k, v in _record_matches(d["history"][row, b], rec, (it, b)).items():
                worst[k] = max(worst.get(k, 0.0), v)
            np.testing.assert_array_equal(d["u_cand"][b], out["u_new"][b])
            e = np.abs(d["x_cand"][b] - out["x_new"][b]).max()
            worst["x_cand"] = max(worst["x_cand"], e)
            assert e <= dc.ROLLOUT_BOUND, (it, b, e)
    print("lockstep: worst |device - host|:", {k: f"{v:.2e}" for k, v in worst.items()}, "; bounds", {k: f"{v:.1e}" for k, v in bound.items()})

    # the cap: a trajectory still active would write record 8 of 8
    still = np.flatnonzero(hst[-1]["active"])
    assert still.size and (dev[-1]["outer"][still] == cap).all() and loop.t["history"].shape[0] == cap
    before = {k: v.clone() for k, v in loop.t.items()}
    with pytest.raises(RuntimeError, match=rf"history_capacity \({cap}\) exhausted: trajectory {still[0]} "):
        loop.advance(z)
    torch.cuda.synchronize()
    for k, v in loop.t.items():
        assert torch.equal(v, before[k]), k


def _same_results(a, b, what):
    assert len(a) == len(b)
    for i, (r, o) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(r.u, o.u, err_msg=f"{what}: u of trajectory {i}")
        np.testing.assert_array_equal(r.x, o.x, err_msg=f"{what}: x of trajectory {i}")
        assert r.cost == o.cost and r.accepted == o.accepted and r.converged == o.converged and r.outer_iterations == o.outer_iterations, (what, i)
        assert r.history == o.history, (what, i)


def test_the_loop_on_a_callers_stream(gpu):
    """scvx_batch(outer_on_device=True) on 9 trajectories of the shared scenario: twice on torch's default stream (hip_stream = NULL)
    with the same bits -- u, x, cost, every history field: the loop is deterministic --, then inside torch.cuda.stream(side), where
    admm_update_problem_device, admm_set_state_device, admm_get_device and the four SCvx entry points are ordered against each other
    by nothing but the caller's non-NULL stream: the same bits again.
    And the rollout behind a busy stream: `side` is given a chain of fp64 matmuls (their number from one timed matmul, for >= 200
    ms of work) that ends by writing u into its tensor; the rollout is queued while that chain is still running (side.query() is
    False just before -- the test fails as vacuous otherwise), and only then is the stream waited for."""
    rng = np.random.default_rng(11)
    B = 9
    x0s = case.X0[None] * (1.0 + 0.05 * rng.standard_normal((B, 6)))
    args = (x0s, case.N, case.DT, case.Q, case.R, case.QN, -case.U_MAX, case.U_MAX)
    kw = dict(qp_options=case.QP, linearise_on=DEV, outer_on_device=True, **case.SCVX)
    t0 = time.perf_counter()
    first = sc.scvx_batch(*args, **kw)
    t1 = time.perf_counter()
    assert all(r.converged for r in first)
    _same_results(sc.scvx_batch(*args, **kw), first, "second run on the default stream")
    side = torch.cuda.Stream(device=DEV)
    assert side.cuda_stream != 0
    with torch.cuda.stream(side):
        on_side = sc.scvx_batch(*args, **kw)
    side.synchronize()
    _same_results(on_side, first, "on the caller's stream")
    print(f"stream: one loop of B={B} N={case.N} takes {t1 - t0:.2f} s, {first[0].outer_iterations} outer iterations")

    x0, u, x, *_ = dc.scattered(65, 64)
    loop = _loop(x0, 64)
    src = _t(u)
    u_dev = torch.full_like(src, 7.0)                              # what a rollout that did not wait would read
    a = torch.eye(2048, dtype=torch.float64, device=DEV).roll(1, 0)
    bufs = [a.clone(), torch.empty_like(a)]
    torch.mm(a, bufs[0], out=bufs[1])                              # warm-up (library initialisation), then one timed product
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    torch.mm(a, bufs[1], out=bufs[0])
    torch.cuda.synchronize()
    count = max(16, math.ceil(0.2 / max(time.perf_counter() - t0, 1e-6)))
    try:
        with torch.cuda.stream(side):
            for i in range(count):
                torch.mm(a, bufs[i % 2], out=bufs[(i + 1) % 2])
            u_dev.copy_(src)
            busy = not side.query()
            got = loop.rollout(u_dev)
        side.synchronize()
    finally:
        del a, bufs
        torch.cuda.empty_cache()                                   # the 32 MB blocks go back: later tests expect fresh blocks for large tensors
    assert busy, f"vacuous: the stream had already finished its {count} matmuls when the rollout was queued"
    err = np.abs(got.cpu().numpy() - x).max()
    print(f"stream: rollout behind {count} matmuls, max abs err {err:.3e}")
    assert err <= dc.ROLLOUT_BOUND


def test_refusals_name_the_argument_and_touch_nothing(gpu, lib):
    """Every argument case of the entry points gives ADMM_ERR_INVALID with the argument's name in admm_last_error, before anything
    is launched: afterwards every tensor of the state (and the outputs) holds the bits it held."""
    state, _ = dc.decision_inputs()
    B, N = state["ub"].shape[:2]
    loop = _loop(state["x0"], N, max_outer=4)
    loop.init(1.0, 100.0)
    z = _t(state["z"].reshape(B, N * 9))
    u = _t(state["ub"])
    xout = torch.full((B, N, 6), 3.0, dtype=torch.float64, device=DEV)
    outs = {k: getattr(loop, k) for k in ("A", "B", "lo", "hi", "q")}
    for v in outs.values():
        v.fill_(3.0)
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in {**loop.t, **outs, "xout": xout}.items()}
    P, S = loop.ptr, None
    nact = C.c_int32(-5)

    def call(name, model=None, params=None, st=None, **ptrs):
        """One entry point with the loop's own (valid) arguments, some replaced."""
        model = C.byref(model or loop.model)
        params = C.byref(params or loop.params)
        st = C.byref(st or loop.state)
        a = {k: P(v) for k, v in dict(x0=loop.x0, u=u, x=xout, z=z, **outs).items()}
        a.update(ptrs)
        fn = getattr(lib, name)
        if name == "admm_scvx_rollout_device":
            return fn(0, model, a["x0"], a["u"], a["x"], S)
        if name == "admm_scvx_init_device":
            return fn(0, model, params, a["x0"], st, 1.0, 100.0, S)
        if name == "admm_scvx_prepare_device":
            return fn(0, model, params, a["x0"], st, a["A"], a["B"], a["lo"], a["hi"], a["q"], S)
        return fn(0, model, params, a["x0"], a["z"], st, ptrs.get("n_active", C.byref(nact)), S)

    def refused(name, word, **kw):
        assert call(name, **kw) == INVALID, (name, word)
        msg = lib.admm_last_error().decode()
        assert msg.startswith(name + ": ") and word in msg, (name, word, msg)

    def model(**kw):
        return _abi.CScvxModel(**dict(dict(N=N, batch=B, substeps=4, dt=dc.DT, rc=sc.RC_KM), **kw))

    def params(**kw):
        p = _abi.CScvxParams.from_buffer_copy(loop.params)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    ALL = ("admm_scvx_rollout_device", "admm_scvx_init_device", "admm_scvx_prepare_device", "admm_scvx_advance_device")
    for name in ALL:
        for field in ("N", "batch", "substeps"):
            for bad in (0, -1):
                refused(name, "model." + field, model=model(**{field: bad}))
        for field in ("dt", "rc"):
            for bad in (0.0, -1.0, np.inf, np.nan):
                refused(name, "model." + field, model=model(**{field: bad}))
        if name != ALL[0]:
            for bad in (0.0, -1e-6, np.inf, np.nan):
                refused(name, "params.fd_eps", params=params(fd_eps=bad))
    # NULL, host memory (pageable and pinned), an allocation that ends too early: every pointer argument
    hostv = np.zeros(B * N * 36)
    pinned = torch.zeros(B * N * 36, dtype=torch.float64).pin_memory()
    big = torch.zeros(3 * 2 ** 20, dtype=torch.float64, device=DEV)      # a block of its own in torch's allocator: its true end is known

    def wrong(count):
        yield "is NULL", _abi.c_double_p()
        yield "is not device memory", _abi.dptr(hostv)
        yield "is not device memory", P(pinned)
        yield f"ends before its {count} doubles", P(big[big.numel() - (count - 1):])
    direct = {"admm_scvx_rollout_device": dict(x0=B * 6, u=B * N * 3, x=B * N * 6),
              "admm_scvx_init_device": dict(x0=B * 6),
              "admm_scvx_prepare_device": dict(x0=B * 6, A=B * N * 36, B=B * N * 18, lo=B * N * 9, hi=B * N * 9, q=B * N * 9),
              "admm_scvx_advance_device": dict(x0=B * 6, z=B * N * 9)}
    for name, argsz in direct.items():
        for arg, count in argsz.items():
            for word, p in wrong(count):
                refused(name, f"{arg} {word}", **{arg: p})
    sizes = dict(ub=B * N * 3, xb=B * N * 6, u_cand=B * N * 3, x_cand=B * N * 6, J=B, tr_u=B, tr_x=B, history=4 * B * 9)
    used = {"admm_scvx_init_device": tuple(sizes), "admm_scvx_prepare_device": ("ub", "xb", "tr_u", "tr_x"),
            "admm_scvx_advance_device": tuple(sizes)}
    for name, fields in used.items():
        for f in fields:
            for word, p in wrong(sizes[f]):
                st = _abi.CScvxState.from_buffer_copy(loop.state)
                setattr(st, f, p)
                refused(name, f"state.{f} {word}", st=st)
        for f in ("active",) if name == ALL[2] else loop.STATE_I32:
            bigi = big.view(torch.int32)
            for word, p in (("is NULL", _abi.c_int32_p()), ("is not device memory", _abi.iptr(np.zeros(B, np.int32))),
                            (f"ends before its {B} int32 entries", P(bigi[bigi.numel() - (B - 1):]))):
                st = _abi.CScvxState.from_buffer_copy(loop.state)
                setattr(st, f, p)
                refused(name, f"state.{f} {word}", st=st)
    assert lib.admm_scvx_advance_device(0, C.byref(loop.model), C.byref(loop.params), P(loop.x0), P(z), C.byref(loop.state), None, S) == INVALID
    assert "n_active is NULL" in lib.admm_last_error().decode()
    # history exhausted: an ACTIVE trajectory whose next record is past the capacity (an inactive one may sit there)
    st = _abi.CScvxState.from_buffer_copy(loop.state)
    st.history_capacity = 0
    refused(ALL[3], "history_capacity", st=st)
    loop.t["outer"][3] = 4
    torch.cuda.synchronize()
    before["outer"] = loop.t["outer"].clone()
    refused(ALL[3], "history_capacity (4) exhausted: trajectory 3")
    torch.cuda.synchronize()
    for k, v in {**loop.t, **outs, "xout": xout}.items():
        assert torch.equal(v, before[k]), k
    assert nact.value == -5 and (big == 0).all() and (hostv == 0).all() and (pinned == 0).all()
    # ... and with that trajectory inactive the same call goes through
    loop.t["active"][3] = 0
    assert 0 <= loop.advance(z) <= B - 1
    assert int(loop.t["outer"][3]) == 4 and int(loop.t["outer"].min()) == 1
