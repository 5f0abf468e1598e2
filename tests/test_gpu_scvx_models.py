"""The model interface of the device SCvx outer step on the GPU (ADMM_HIP_HAS_SCVX_MODELS): the CR3BP kernels
against a long-double restatement of the model (the yardstick: NumPy fp64's own distance from it, tests/_scvx_models_case.py), the
decisions on every branch, kind 0 through the new entry points against the old entry points, whole loops in lockstep with a host
model and against the host loop, a caller's stream, and the refusals that need a device.  Inputs and references are built once on
the CPU, shared and read-only; tests/test_scvx_models_host.py asserts their preconditions."""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch          # before libadmm_hip.so is loaded (the `gpu` fixture): both then share one HIP runtime

from admm_library_amd import _abi
from admm_library_amd import scvx as sc

import _scvx_device_case as dc
import _scvx_models_case as mc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = 1
NAMES = sorted(mc.PARAMS)


def _loop(x0, N, p, **kw):
    """The loop object under a parameter set of tests/_scvx_models_case.py, with its CR3BP model."""
    kw = dict(dict(device=DEV, tol=mc.TOL, rho_reject=mc.RHO_REJECT, rho_expand=mc.RHO_EXPAND, substeps=p.substeps, eps=p.fd_eps,
                   model=mc.model_of(p)), **kw)
    return sc.DeviceOuterStep(x0, N, p.dt, *(np.array(a) for a in (p.Q, p.R, p.QN, p.u_lo, p.u_hi)), **kw)


def _t(a, dtype=None):
    return torch.as_tensor(np.array(a, dtype), device=DEV)


def _ld_err(got, ref):
    return float(np.abs(got.astype(np.longdouble) - ref).max())


def _qp_of(loop, B, N):
    return {k: getattr(loop, k).cpu().numpy().reshape((B, N, 9) if k == "q" else tuple(getattr(loop, k).shape)) for k in ("A", "B", "lo", "hi", "q")}


# ---- 8. rollout, linearisation, assembly
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("B,N", mc.SHAPES)
def test_rollout_linearisation_and_assembly_match_long_double(gpu, B, N, name):
    """admm_scvx_rollout_model_device and admm_scvx_prepare_model_device of the CR3BP about scattered(B, N, name): x, A, B and q
    within GPU_MARGIN = 10 x what NumPy fp64 itself differs from the long-double evaluation of the same formulas on these inputs
    (FP64_VS_LD); lo, hi equal correction_qp_batch's exactly, the zero-width box for inactive trajectories; each A block is its own
    and not its transpose."""
    p = mc.PARAMS[name]
    x0, u, x, tru, trx, active = mc.scattered(B, N, name)
    r, c = mc.reference(B, N, name), mc.FP64_VS_LD[name, B, N]
    loop = _loop(x0, N, p)
    got_x = loop.rollout(_t(u)).cpu().numpy()
    for k, a in (("ub", u), ("xb", x), ("tr_u", tru), ("tr_x", trx)):
        loop.t[k].copy_(_t(a))
    loop.t["active"].copy_(_t(active, np.int32))
    loop.prepare()
    got = _qp_of(loop, B, N)
    err = dict(x=_ld_err(got_x, r["ld"]["x"]), A=_ld_err(got["A"], r["ld"]["A"]), B=_ld_err(got["B"], r["ld"]["B"]), q=_ld_err(got["q"], r["ld"]["q"]))
    print(f"{name} B={B} N={N}: device vs long double / NumPy vs long double:",
          {k: f"{err[k]:.2e} / {c[k]:.1e} = {err[k] / c[k]:.2f}" for k in err})
    assert got_x.shape == x.shape
    for k in err:
        assert err[k] <= mc.GPU_MARGIN * c[k], (k, err[k], c[k])
    np.testing.assert_array_equal(got["lo"], r["lo"])
    np.testing.assert_array_equal(got["hi"], r["hi"])
    off = ~active
    assert (got["lo"][off] == 0).all() and (got["hi"][off] == 0).all() and (B == 1 or off.any())
    A = np.asarray(r["ld"]["A"], np.float64)
    own = np.abs(got["A"] - A).max(axis=(2, 3))
    swapped = np.abs(got["A"] - np.swapaxes(A, -1, -2)).max(axis=(2, 3))
    assert (swapped - own >= 1e-3).all()
    # and the device is the right model, not one with the primaries' masses or offsets exchanged
    for wrong in ("x_mu_swapped", "x_d_swapped"):
        assert _ld_err(got_x, r[wrong]) >= 1e-3 - err["x"]


# ---- 9. decisions
def _record_matches(row, rec, where, slack=0.0):
    """One history record of the device (the 9 doubles) against outer_update's: flags, radii and du_max equal; costs and their
    differences within 1e-12 |J| + slack (slack: what the bound on the candidate's states makes of the cost, where the states carry
    an amplified rounding); the ratio within that bound propagated through its operands."""
    row = dict(zip(_abi.SCVX_HISTORY_FIELDS, row))
    assert bool(row["accepted"]) == rec["accepted"] and row["accepted"] in (0.0, 1.0), where
    assert row["tr_u"] == rec["tr_u"] and row["tr_x"] == rec["tr_x"], where
    assert row["du_max"] == rec["du_max"], where
    bound = 1e-12 * abs(rec["cost"]) + slack
    for k in ("cost", "cost_candidate", "predicted", "actual"):
        assert abs(row[k] - rec[k]) <= bound, (where, k, row[k], rec[k], bound)
    if abs(rec["predicted"]) <= bound:
        assert abs(row["predicted"]) <= 2.0 * bound, where
    elif rec["predicted"] < 0:
        assert row["ratio"] == rec["ratio"] == -np.inf, (where, row, rec)
    else:
        assert abs(row["ratio"] - rec["ratio"]) <= 2.0 * bound * (1.0 + abs(rec["ratio"])) / abs(rec["predicted"]), (where, row, rec)
    return max(abs(row[k] - rec[k]) for k in ("cost", "cost_candidate", "predicted", "actual")) / abs(rec["cost"])


@pytest.mark.parametrize("params", mc.DECISION_PARAMS)
@pytest.mark.parametrize("B,N", mc.DECISION_SHAPES)
def test_decisions_match_outer_update_on_every_branch(gpu, B, N, params):
    """One admm_scvx_advance_model_device call at the shape edges of scvx_advance_kernel against scvx.outer_update on the same inputs
    (decision_inputs: the oracle's z steers the branches; asserted first: every branch B // 6 times, no ratio within 1e-3 of a
    threshold).  Flags, radii, take, n_active and accepted counts are equal; the history records within the cost bounds; the
    candidate's controls equal, its states within GPU_MARGIN x CANDIDATE_FP64_VS_LD of the long-double rollout; candidates and
    history of inactive rows, and every other history row, hold the junk they were filled with."""
    p = mc.PARAMS[params]
    state, ref = mc.decision_inputs(B, N, params)
    taken = [dc.branch_of(b, state, ref) for b in range(B)]
    counts = {t: taken.count(t) for t in mc.BRANCHES}
    if B == 1:
        assert taken == ["accepted"], f"precondition (branch counts) failed: {counts}"
    else:
        assert all(c >= B // 6 for c in counts.values()), f"precondition (branch counts) failed: {counts}"
    margin = dc.ratio_margin(ref["records"].values())
    assert margin > 1e-3, f"precondition (knife-edge margin) failed: a ratio lies within {margin:.3e} of a threshold"
    if B >= 66:
        assert (np.flatnonzero(~state["active"]) > 63).any(), "precondition failed: no inactive trajectory past the first wave"

    cap = int(ref["outer"].max()) + 1
    loop = _loop(state["x0"], N, p, max_outer=cap)
    junk = dc.decision_junk(B, N, cap)
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
    assert (np.abs(got["J"] - ref["J"]) <= 1e-12 * np.abs(state["J"])).all()
    xbound = mc.GPU_MARGIN * mc.CANDIDATE_FP64_VS_LD[params]
    worst, worst_x = 0.0, 0.0
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
        worst = max(worst, _record_matches(got["history"][it, b], ref["records"][b], b))
        assert np.abs(got["u_cand"][b] - ref["u_new"][b]).max() == 0.0
        ex = _ld_err(got["x_cand"][b], ref["x_new_ld"][b])
        worst_x = max(worst_x, ex)
        assert ex <= xbound, (b, ex, xbound)
        if ref["take"][b]:
            np.testing.assert_array_equal(got["ub"][b], got["u_cand"][b])
            np.testing.assert_array_equal(got["xb"][b], got["x_cand"][b])
        else:
            np.testing.assert_array_equal(got["ub"][b], state["ub"][b])
            np.testing.assert_array_equal(got["xb"][b], state["xb"][b])
    print(f"decisions B={B} N={N} {params}: worst |device - host| / |J| over the cost fields {worst:.2e}; x_cand vs long double "
          f"{worst_x:.2e} = {worst_x / mc.CANDIDATE_FP64_VS_LD[params]:.2f} x NumPy's")


def test_a_candidate_with_a_non_finite_cost_is_rejected_as_outer_update_rejects_it(gpu):
    """Candidates rolled out from ON a primary (k d = inf 0: a NaN cost) and with a velocity that overflows the cost, next to
    ordinary ones (tests/_scvx_models_case.nonfinite_inputs), against scvx.outer_update: every flag, count, take and radius equal
    -- rejected, radii halved, still active, J, ub and xb untouched; the record carries the NaN.  A second call rejects them
    again: no trajectory ends converged with a NaN cost.  (Device code is compiled with -fno-honor-nans; the decision tests the
    bits before it compares.)"""
    p, state, ref = mc.nonfinite_inputs()
    B, N = state["ub"].shape[:2]
    loop = _loop(state["x0"], N, p, max_outer=3)
    for k in ("ub", "xb", "J", "tr_u", "tr_x"):
        loop.t[k].copy_(_t(state[k]))
    for k in ("active", "converged", "accepted", "outer"):
        loop.t[k].copy_(_t(state[k], np.int32))
    z = _t(state["z"].reshape(B, N * 9))
    n_active = loop.advance(z)
    got = {k: v.cpu().numpy() for k, v in loop.t.items()}
    assert n_active == int(ref["active"].sum())
    for k in ("active", "converged", "accepted", "outer", "take"):
        np.testing.assert_array_equal(got[k], ref[k].astype(np.int32), err_msg=k)
    np.testing.assert_array_equal(got["tr_u"], ref["tr_u"])
    np.testing.assert_array_equal(got["tr_x"], ref["tr_x"])
    for b in range(B):
        rec, row = ref["records"][b], dict(zip(_abi.SCVX_HISTORY_FIELDS, got["history"][0, b]))
        if b not in mc.NONFINITE_ROWS:
            _record_matches(got["history"][0, b], rec, b)
            assert abs(got["J"][b] - ref["J"][b]) <= 1e-12 * abs(ref["J"][b])
            continue
        print(f"trajectory {b} ({mc.NONFINITE_ROWS[b]}): device cost_candidate {row['cost_candidate']}, ratio {row['ratio']}; host "
              f"{rec['cost_candidate']}, {rec['ratio']}")
        assert row["accepted"] == 0.0 and row["cost"] == rec["cost"] and abs(row["predicted"] - rec["predicted"]) <= 1e-12 * rec["cost"]
        assert not np.isfinite(row["cost_candidate"]) and not np.isfinite(row["actual"])
        if mc.NONFINITE_ROWS[b] == "nan":
            assert np.isnan(row["cost_candidate"]) and np.isnan(row["actual"]) and np.isnan(row["ratio"]) and np.isnan(rec["ratio"])
        assert got["J"][b] == state["J"][b]
        np.testing.assert_array_equal(got["ub"][b], state["ub"][b])
        np.testing.assert_array_equal(got["xb"][b], state["xb"][b])
    assert loop.advance(z) >= len(mc.NONFINITE_ROWS)
    again = {k: v.cpu().numpy() for k, v in loop.t.items()}
    rows = sorted(mc.NONFINITE_ROWS)
    assert np.isfinite(again["J"]).all() and (again["converged"][rows] == 0).all() and (again["active"][rows] == 1).all()
    assert (again["accepted"][rows] == 0).all() and (again["tr_u"][rows] == 0.25 * state["tr_u"][rows]).all()


# ---- 10. kind 0 through the new entry points
def test_kind_0_through_the_model_calls_equals_the_old_calls(gpu):
    """rollout, init, prepare and advance on _scvx_device_case.scattered(65, 64), once through admm_scvx_*_device and once through
    admm_scvx_*_model_device with kind ADMM_SCVX_RELATIVE_CIRCULAR: every output array and n_active are equal, bit for bit."""
    B, N = 65, 64
    x0, u, x, tru, trx, active = dc.scattered(B, N)
    rng = np.random.default_rng(7)
    z = (-0.02 * np.concatenate([u, x], axis=-1) * rng.uniform(0.5, 1.5, (B, 1, 1))).reshape(B, N * 9)      # towards the origin: a gain is predicted
    c = dc.ORIGINAL
    outs = []
    for model in (None, sc.relative_circular()):
        loop = sc.DeviceOuterStep(x0, N, c.dt, c.Q, c.R, c.QN, c.u_lo, c.u_hi, device=DEV, tol=dc.TOL, max_outer=3, model=model)
        assert type(loop.model) is (_abi.CScvxModel if model is None else _abi.CScvxDynamics)
        out = {"rollout": loop.rollout(_t(u)).cpu().numpy()}
        loop.init(1.0, 100.0)
        out.update({"init_" + k: v.cpu().numpy() for k, v in loop.t.items() if k not in ("u_cand", "x_cand", "history")})
        for k, a in (("ub", u), ("xb", x), ("tr_u", tru), ("tr_x", trx)):
            loop.t[k].copy_(_t(a))
        loop.t["active"].copy_(_t(active, np.int32))
        for k in ("u_cand", "x_cand", "history"):
            loop.t[k].fill_(3.0)
        loop.prepare()
        out.update({"prepare_" + k: v for k, v in _qp_of(loop, B, N).items()})
        out["n_active"] = loop.advance(_t(z))
        out.update({"advance_" + k: v.cpu().numpy() for k, v in loop.t.items()})
        outs.append(out)
    old, new = outs
    print("kind 0:", old["n_active"], "still active,", int(old["advance_take"].sum()), "candidates taken")
    assert old["n_active"] == new["n_active"] < B and np.abs(old["rollout"] - x).max() <= dc.ROLLOUT_BOUND
    for k in old:
        np.testing.assert_array_equal(new[k], old[k], err_msg=k)


# ---- 11. whole loops
def test_whole_loops_in_lockstep_with_a_host_model(gpu):
    """The device loop of the CR3BP -- init, then max_outer = 8 rounds of prepare -> GPU QP solve -> advance -- on the 70 trajectories
    of 13 stages of tests/_scvx_models_case.LOCKSTEP, and a host model (HostLoop) that repeats every outer iteration in the host
    formulas from the same z and from nothing else of the device's, so that the QP tolerance does not enter.  The preconditions are
    asserted on the host model's records (lockstep_preconditions; tests/test_scvx_models_host.py has them at ten times the margin
    with the CPU oracle).  Per outer iteration: lo, hi equal; A, B, q and the candidates within GPU_MARGIN x LOCKSTEP_FP64_VS_LD of the
    long-double formulas on the device's own inputs, the references within that of the host model's; every flag, count, take, radius, ub and n_active equal; costs and history rows within 1e-12 |J| plus what
    the bound on the states makes of a cost (sum_k |Q_k x_k|_1 x the bound); older history rows and the candidates of inactive
    trajectories hold their bits."""
    c = mc.LOCKSTEP
    p, host = mc.lockstep_params(), mc.lockstep_host()
    B, N, cap = c["B"], c["N"], c["max_outer"]
    loop = _loop(host.x0, N, p, tol=c["tol"], max_outer=cap)
    rng = np.random.default_rng(5)
    for k in ("u_cand", "x_cand", "history"):
        loop.t[k].copy_(_t(rng.standard_normal(tuple(loop.t[k].shape))))
    loop.init(c["tr_u"], c["tr_x"])
    solve = sc.gpu_qp_solver(True, z_on_device=True, **mc.LOCKSTEP_QP)

    def state_of(h):
        return {k: np.array(getattr(h, k)) for k in ("ub", "xb", "J", "tr_u", "tr_x", "active", "converged", "accepted", "outer")}
    dev = [{k: v.cpu().numpy() for k, v in loop.t.items()}]
    hst = [state_of(host)]
    qps, outs, counts = [], [], []
    t0 = time.perf_counter()
    for it in range(cap):
        prob = loop.prepare()
        qps.append((_qp_of(loop, B, N), host.qp()))
        z, _ = solve(prob)
        counts.append(loop.advance(z))
        outs.append(host.advance(z.cpu().numpy(), it))
        dev.append({k: v.cpu().numpy() for k, v in loop.t.items()})
        hst.append(state_of(host))
    print(f"lockstep: {cap} outer iterations of B={B} N={N} in {time.perf_counter() - t0:.2f} s")
    seen = dc.lockstep_preconditions(host)
    print("lockstep:", {k: v for k, v in seen.items() if k != "mixed"}, f"{len(seen['mixed'])} trajectories with mixed sequences")

    bound = {k: mc.GPU_MARGIN * v for k, v in mc.LOCKSTEP_FP64_VS_LD.items()}
    weight = lambda x: (np.abs(x[:, :-1] @ p.Q.T).sum(axis=(1, 2)) + np.abs(x[:, -1] @ p.QN.T).sum(axis=1))      # noqa: E731

    def same_state(d, h, what):
        for k in ("active", "converged", "accepted", "outer"):
            np.testing.assert_array_equal(d[k], h[k].astype(np.int32), err_msg=f"{what}: {k}")
        for k in ("tr_u", "tr_x", "ub"):
            np.testing.assert_array_equal(d[k], h[k], err_msg=f"{what}: {k}")
        ex = np.abs(d["xb"] - h["xb"]).max()                       # both within their bounds of the long-double rollout: 10 + 1
        eJ = (np.abs(d["J"] - h["J"]) / (1e-12 * np.abs(h["J"]) + 1.1 * bound["x"] * weight(h["xb"]))).max()
        assert ex <= 1.1 * bound["x"] and eJ <= 1.0, (what, ex, eJ)
        return ex, eJ
    worst = dict(zip(("xb", "J / its bound"), same_state(dev[0], hst[0], "after init")))
    worst.update(A=0.0, B=0.0, q=0.0, x_cand=0.0)
    assert (dev[0]["take"] == 0).all()
    qbound = bound["q"] + max(np.abs(M).sum(axis=1).max() for M in (p.Q, p.QN)) * bound["x"]
    for it in range(cap):
        got, want = qps[it]
        np.testing.assert_array_equal(got["lo"], want.lo, err_msg=f"iteration {it}: lo")
        np.testing.assert_array_equal(got["hi"], want.hi, err_msg=f"iteration {it}: hi")
        off = ~hst[it]["active"]
        assert (got["lo"][off] == 0).all() and (got["hi"][off] == 0).all()
        # A, B, q against the long-double formulas about the DEVICE's own reference (the same inputs: where a reference passes a
        # primary closely, A about the host's reference differs by the propagated 1e-10 of the two references, not by rounding)
        xprev = np.concatenate([host.x0[:, None, :], dev[it]["xb"][:, :-1, :]], axis=1)
        A_ld, B_ld = mc.ld_linearise(xprev, dev[it]["ub"], p)
        q_ld = dc.linear_term(dev[it]["xb"], dev[it]["ub"], p.Q, p.R, p.QN, mc.LD)
        for k, w in (("A", A_ld), ("B", B_ld), ("q", q_ld)):
            e = _ld_err(got[k], w)
            worst[k] = max(worst[k], e)
            assert e <= bound[k], (it, k, e, bound[k])
        assert np.abs(got["q"] - want.q.reshape(B, N, 9)).max() <= qbound
        d, d0, out, was = dev[it + 1], dev[it], outs[it], outs[it]["was_active"]
        assert counts[it] == int(hst[it + 1]["active"].sum()), it
        np.testing.assert_array_equal(d["take"], out["take"].astype(np.int32), err_msg=f"iteration {it}: take")
        ex, eJ = same_state(d, hst[it + 1], f"iteration {it}")
        worst["xb"], worst["J / its bound"] = max(worst["xb"], ex), max(worst["J / its bound"], eJ)
        slack = 1.1 * bound["x"] * (weight(hst[it]["xb"]) + weight(out["x_new"]))
        x_ld = mc.ld_rollout(host.x0, out["u_new"], p)              # the candidates' controls are equal (asserted below)
        for b in range(B):
            row = int(hst[it]["outer"][b])
            rows = np.arange(cap) != row if was[b] else np.ones(cap, bool)
            np.testing.assert_array_equal(d["history"][rows, b], d0["history"][rows, b], err_msg=f"iteration {it}, trajectory {b}: older history rows")
            if not was[b]:
                np.testing.assert_array_equal(d["u_cand"][b], d0["u_cand"][b])
                np.testing.assert_array_equal(d["x_cand"][b], d0["x_cand"][b])
                continue
            assert row == it
            _record_matches(d["history"][row, b], out["records"][b], (it, b), slack[b])
            np.testing.assert_array_equal(d["u_cand"][b], out["u_new"][b])
            e = _ld_err(d["x_cand"][b], x_ld[b])
            worst["x_cand"] = max(worst["x_cand"], e)
            assert e <= bound["x"], (it, b, e)
    print("lockstep: worst |device - host|:", {k: f"{v:.2e}" for k, v in worst.items()}, "; bounds", {k: f"{v:.1e}" for k, v in bound.items()},
          "; as multiples of NumPy's distance from long double:",
          {k: f"{worst[w] / mc.LOCKSTEP_FP64_VS_LD[k]:.2f}" for k, w in (("x", "x_cand"), ("A", "A"), ("B", "B"), ("q", "q"))})


def test_the_device_loop_agrees_with_the_host_loop_about_l2(gpu):
    """scvx_batch(model=crtbp(Earth-Moon, L2), outer_on_device=True) against the same call with outer_on_device=False (the host loop
    over the torch linearisation), both on the GPU solver, on the em_l2 Monte-Carlo set (B = 66, N = 40) under EM_MC_SCVX (a state
    trust radius inside which the linear model holds; tests/_scvx_models_case.py says why): the number of outer iterations, the
    accepted counts and the converged flags agree for every trajectory -- those that converge and any that is cut at max_outer
    alike --, and the device's x is the nonlinear trajectory under its u."""
    B = 66
    x0 = mc.em_l2_x0(B)
    m = mc.model_of(mc.EM_L2)
    kw = dict(linearise_on=DEV, model=m, **mc.EM_MC_SCVX)
    t0 = time.perf_counter()
    ref = sc.scvx_batch(*mc.em_l2_args(x0), qp_data_on_device=True, **kw)
    t1 = time.perf_counter()
    res = sc.scvx_batch(*mc.em_l2_args(x0), outer_on_device=True, **kw)
    t2 = time.perf_counter()
    worst_cost = worst_x = 0.0
    for b, (r, o) in enumerate(zip(res, ref)):
        assert (r.outer_iterations, r.accepted, r.converged) == (o.outer_iterations, o.accepted, o.converged), (b, r.history, o.history)
        assert [h["accepted"] for h in r.history] == [h["accepted"] for h in o.history], b
        worst_cost = max(worst_cost, abs(r.cost - o.cost) / abs(o.cost))
        worst_x = max(worst_x, np.abs(r.x - sc.rollout(x0[b], r.u, mc.EM_DT, m.step)).max())
        assert (np.abs(r.u) <= mc.EM_U_MAX).all()
    kinds = {(h["accepted"], bool(h["ratio"] >= 0.7)) for r in res for h in r.history}
    print(f"L2 acquisition, B={B}: host loop {t1 - t0:.2f} s, device loop {t2 - t1:.2f} s; outer iterations "
          f"{min(r.outer_iterations for r in res)}..{max(r.outer_iterations for r in res)}, {sum(r.converged for r in res)} converged; "
          f"cost rel {worst_cost:.2e}, x vs host rollout {worst_x:.2e}")
    assert len(res) == B and (True, True) in kinds and sum(r.converged for r in res) >= B // 2
    assert worst_cost <= 1e-5 and worst_x <= 1e-12


# ---- 12. a caller's stream, the device ordinal, pointer refusals
def _same_results(a, b, what):
    assert len(a) == len(b)
    for i, (r, o) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(r.u, o.u, err_msg=f"{what}: u of trajectory {i}")
        np.testing.assert_array_equal(r.x, o.x, err_msg=f"{what}: x of trajectory {i}")
        assert r.cost == o.cost and r.accepted == o.accepted and r.converged == o.converged and r.outer_iterations == o.outer_iterations, (what, i)
        assert r.history == o.history, (what, i)


def test_the_model_loop_on_a_callers_stream(gpu):
    """scvx_batch(model=..., outer_on_device=True) on 9 trajectories of the em_l2 set: twice on torch's default stream with the same
    bits, then inside torch.cuda.stream(side), where the solver's device calls and the four model calls are ordered by nothing but
    the caller's stream: the same bits again.  And the CR3BP rollout behind a busy stream (a chain of fp64 matmuls that ends by
    writing u; the test fails as vacuous if the chain had finished before the rollout was queued)."""
    x0 = mc.em_l2_x0(9)
    kw = dict(linearise_on=DEV, outer_on_device=True, model=mc.model_of(mc.EM_L2), **mc.EM_SCVX)
    first = sc.scvx_batch(*mc.em_l2_args(x0), **kw)
    _same_results(sc.scvx_batch(*mc.em_l2_args(x0), **kw), first, "second run on the default stream")
    side = torch.cuda.Stream(device=DEV)
    assert side.cuda_stream != 0
    with torch.cuda.stream(side):
        on_side = sc.scvx_batch(*mc.em_l2_args(x0), **kw)
    side.synchronize()
    _same_results(on_side, first, "on the caller's stream")

    name, B, N = "general3", 65, 64
    p = mc.PARAMS[name]
    x0, u, *_ = mc.scattered(B, N, name)
    loop = _loop(x0, N, p)
    src = _t(u)
    u_dev = torch.full_like(src, 0.4)                              # what a rollout that did not wait would read
    a = torch.eye(2048, dtype=torch.float64, device=DEV).roll(1, 0)
    bufs = [a.clone(), torch.empty_like(a)]
    torch.mm(a, bufs[0], out=bufs[1])
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
        torch.cuda.empty_cache()
    assert busy, f"vacuous: the stream had already finished its {count} matmuls when the rollout was queued"
    err = _ld_err(got.cpu().numpy(), mc.reference(B, N, name)["ld"]["x"])
    print(f"stream: rollout behind {count} matmuls, max abs err {err:.3e}")
    assert err <= mc.GPU_MARGIN * mc.FP64_VS_LD[name, B, N]["x"]


def test_model_call_refusals_name_the_argument_and_launch_nothing(gpu, lib):
    """A device ordinal that does not exist, and every pointer argument as NULL, host memory (pageable and pinned), an allocation that
    ends too early and -- with a second GPU visible -- memory of another device: ADMM_ERR_INVALID naming the argument, and every
    tensor of the state and the outputs holds the bits it held."""
    p = mc.PARAMS["general3"]
    state, _ = mc.decision_inputs(66, 9, "general3")
    B, N = state["ub"].shape[:2]
    loop = _loop(state["x0"], N, p, max_outer=4)
    loop.init(1.0, 2.0)
    z = _t(state["z"].reshape(B, N * 9))
    u = _t(state["ub"])
    xout = torch.full((B, N, 6), 3.0, dtype=torch.float64, device=DEV)
    outs = {k: getattr(loop, k) for k in ("A", "B", "lo", "hi", "q")}
    for v in outs.values():
        v.fill_(3.0)
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in {**loop.t, **outs, "xout": xout}.items()}
    P = loop.ptr
    nact = C.c_int32(-5)
    ALL = ("admm_scvx_rollout_model_device", "admm_scvx_init_model_device", "admm_scvx_prepare_model_device", "admm_scvx_advance_model_device")

    def call(name, device=0, st=None, **ptrs):
        dyn, params = C.byref(loop.model), C.byref(loop.params)
        st = C.byref(st or loop.state)
        a = {k: P(v) for k, v in dict(x0=loop.x0, u=u, x=xout, z=z, **outs).items()}
        a.update(ptrs)
        fn = getattr(lib, name)
        if name == ALL[0]:
            return fn(device, dyn, a["x0"], a["u"], a["x"], None)
        if name == ALL[1]:
            return fn(device, dyn, params, a["x0"], st, 1.0, 2.0, None)
        if name == ALL[2]:
            return fn(device, dyn, params, a["x0"], st, a["A"], a["B"], a["lo"], a["hi"], a["q"], None)
        return fn(device, dyn, params, a["x0"], a["z"], st, C.byref(nact), None)

    def refused(name, word, **kw):
        assert call(name, **kw) == INVALID, (name, word)
        msg = lib.admm_last_error().decode()
        assert msg.startswith(name + ": ") and word in msg, (name, word, msg)

    ndev = torch.cuda.device_count()
    for name in ALL:
        for device in (ndev, -1, 64):
            refused(name, "device must be a device ordinal", device=device)
    hostv = np.zeros(B * N * 36)
    pinned = torch.zeros(B * N * 36, dtype=torch.float64).pin_memory()
    big = torch.zeros(3 * 2 ** 20, dtype=torch.float64, device=DEV)
    other = torch.zeros(B * N * 36, dtype=torch.float64, device="cuda:1") if ndev >= 2 else None

    def wrong(count):
        yield "is NULL", _abi.c_double_p()
        yield "is not device memory", _abi.dptr(hostv)
        yield "is not device memory", P(pinned)
        yield f"ends before its {count} doubles", P(big[big.numel() - (count - 1):])
        if other is not None:
            yield "is not device memory", P(other)
    direct = {ALL[0]: dict(x0=B * 6, u=B * N * 3, x=B * N * 6), ALL[1]: dict(x0=B * 6),
              ALL[2]: dict(x0=B * 6, A=B * N * 36, B=B * N * 18, lo=B * N * 9, hi=B * N * 9, q=B * N * 9), ALL[3]: dict(x0=B * 6, z=B * N * 9)}
    for name, argsz in direct.items():
        for arg, count in argsz.items():
            for word, ptr in wrong(count):
                refused(name, f"{arg} {word}", **{arg: ptr})
    sizes = dict(ub=B * N * 3, xb=B * N * 6, u_cand=B * N * 3, x_cand=B * N * 6, J=B, tr_u=B, tr_x=B, history=4 * B * 9)
    used = {ALL[1]: tuple(sizes), ALL[2]: ("ub", "xb", "tr_u", "tr_x"), ALL[3]: tuple(sizes)}
    for name, fields in used.items():
        for f in fields:
            for word, ptr in wrong(sizes[f]):
                st = _abi.CScvxState.from_buffer_copy(loop.state)
                setattr(st, f, ptr)
                refused(name, f"state.{f} {word}", st=st)
        for f in ("active",) if name == ALL[2] else loop.STATE_I32:
            bigi = big.view(torch.int32)
            for word, ptr in (("is NULL", _abi.c_int32_p()), ("is not device memory", _abi.iptr(np.zeros(B, np.int32))),
                              (f"ends before its {B} int32 entries", P(bigi[bigi.numel() - (B - 1):]))):
                st = _abi.CScvxState.from_buffer_copy(loop.state)
                setattr(st, f, ptr)
                refused(name, f"state.{f} {word}", st=st)
    torch.cuda.synchronize()
    for k, v in {**loop.t, **outs, "xout": xout}.items():
        assert torch.equal(v, before[k]), k
    assert nact.value == -5 and (big == 0).all() and (hostv == 0).all() and (pinned == 0).all()
    # and the same calls with their own arguments go through
    assert call(ALL[2]) == 0 and 0 <= loop.advance(z) <= B
