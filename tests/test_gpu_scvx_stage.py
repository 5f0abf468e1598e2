"""Time-dependent models of the device SCvx outer step on the GPU (ADMM_HIP_HAS_SCVX_STAGE_MODELS): the
ScvxRelativeTabulated kernels against a long-double restatement of the model fed the same fp64 node table (the yardstick: NumPy
fp64's own distance from it, tests/_scvx_stage_case.py) -- about an eccentric chief and under tables whose rows are independent per
node, which a node index that is wrong by one cannot survive --, the decisions on every branch, a whole loop in lockstep with a host
model, the e = 0 table against the circular model's kernels, the pointer checks of the table, and the loop end to end.  Inputs and
references are built once on the CPU, shared and read-only; tests/test_scvx_stage_host.py asserts their preconditions."""
import ctypes as C
import time

import numpy as np
import pytest
import torch          # before libadmm_hip.so is loaded (the `gpu` fixture): both then share one HIP runtime

from admm_library_amd import _abi
from admm_library_amd import scvx as sc

import _scvx_device_case as dc
import _scvx_stage_case as st

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = 1


def _loop(x0, N, p, **kw):
    """The loop object under a parameter set of tests/_scvx_stage_case.py, with its time-dependent model."""
    kw = dict(dict(device=DEV, tol=st.TOL, rho_reject=st.RHO_REJECT, rho_expand=st.RHO_EXPAND, substeps=p.substeps, eps=p.fd_eps,
                   model=st.model_of(p)), **kw)
    return sc.DeviceOuterStep(x0, N, p.dt, *(np.array(a) for a in (p.Q, p.R, p.QN, p.u_lo, p.u_hi)), **kw)


def _t(a, dtype=None):
    return torch.as_tensor(np.array(a, dtype), device=DEV)


def _ld_err(got, ref):
    return float(np.abs(got.astype(np.longdouble) - ref).max())


def _qp_of(loop, B, N):
    return {k: getattr(loop, k).cpu().numpy().reshape((B, N, 9) if k == "q" else tuple(getattr(loop, k).shape)) for k in ("A", "B", "lo", "hi", "q")}


def _load_scatter(loop, u, x, tru, trx, active):
    for k, a in (("ub", u), ("xb", x), ("tr_u", tru), ("tr_x", trx)):
        loop.t[k].copy_(_t(a))
    loop.t["active"].copy_(_t(active, np.int32))


# ---- rollout, linearisation, assembly
@pytest.mark.parametrize("name", st.GPU_PARAMS)
@pytest.mark.parametrize("B,N", st.SHAPES)
def test_rollout_linearisation_and_assembly_match_long_double(gpu, B, N, name):
    """admm_scvx_rollout_stage_device and admm_scvx_prepare_stage_device about scattered(B, N, name): x, A, B and q within
    GPU_MARGIN = 10 x what NumPy fp64 itself differs from the long-double evaluation of the same formulas on the same fp64 table
    (FP64_VS_LD); lo, hi equal correction_qp_batch's exactly, the zero-width box for inactive trajectories.  The device is far from
    the restatement with its node indices shifted by one stage, one sub-interval or one RK4 point (random tables: by >= 0.1)."""
    p = st.PARAMS[name]
    x0, u, x, tru, trx, active = st.scattered(B, N, name)
    r, c = st.reference(B, N, name), st.FP64_VS_LD[name, B, N]
    loop = _loop(x0, N, p)
    assert type(loop.model) is _abi.CScvxStageDynamics and loop.model.n_nodes == 2 * p.substeps * N + 1
    np.testing.assert_array_equal(loop.nodes.cpu().numpy(), st.table_of(p, N))
    got_x = loop.rollout(_t(u)).cpu().numpy()
    _load_scatter(loop, u, x, tru, trx, active)
    loop.prepare()
    got = _qp_of(loop, B, N)
    err = dict(x=_ld_err(got_x, r["ld"]["x"]), A=_ld_err(got["A"], r["ld"]["A"]), B=_ld_err(got["B"], r["ld"]["B"]), q=_ld_err(got["q"], r["ld"]["q"]))
    print(f"{name} B={B} N={N}: device vs long double / NumPy vs long double:",
          {k: f"{err[k]:.2e} / {c[k]:.1e} = {err[k] / c[k]:.2f}" for k in err})
    assert got_x.shape == x.shape
    for k in err:
        assert err[k] <= st.GPU_MARGIN * c[k], (k, err[k], c[k])
    np.testing.assert_array_equal(got["lo"], r["lo"])
    np.testing.assert_array_equal(got["hi"], r["hi"])
    off = ~active
    assert (got["lo"][off] == 0).all() and (got["hi"][off] == 0).all() and (B == 1 or off.any())
    if name.startswith("random"):
        for s in st.SHIFTS:
            assert _ld_err(got_x, r["x_" + s]) >= 0.1 - err["x"], s


# ---- decisions
def _record_matches(row, rec, where, slack=0.0):
    """One history record of the device (the 9 doubles) against outer_update's: flags, radii and du_max equal; costs and their
    differences within 1e-12 |J| + slack (slack: what the bound on the candidate's states makes of the cost); the ratio within that
    bound propagated through its operands."""
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


@pytest.mark.parametrize("B,N", st.DECISION_SHAPES)
def test_decisions_match_outer_update_on_every_branch(gpu, B, N):
    """One admm_scvx_advance_stage_device call at the shape edges of scvx_advance_kernel against scvx.outer_update on the same inputs
    about the eccentric chief (decision_inputs: the oracle's z steers the branches; asserted first: every branch B // 6 times, no
    ratio within 1e-3 of a threshold).  Flags, radii, take, n_active and accepted counts are equal; the history records within the
    cost bounds; the candidate's controls equal, its states within GPU_MARGIN x CANDIDATE_FP64_VS_LD of the long-double rollout;
    candidates and history of inactive rows, and every other history row, hold the junk they were filled with."""
    params = "elliptic"
    p = st.PARAMS[params]
    state, ref = st.decision_inputs(B, N, params)
    taken = [dc.branch_of(b, state, ref) for b in range(B)]
    counts = {t: taken.count(t) for t in st.BRANCHES}
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
    xbound = st.GPU_MARGIN * st.CANDIDATE_FP64_VS_LD[params]
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
          f"{worst_x:.2e} = {worst_x / st.CANDIDATE_FP64_VS_LD[params]:.2f} x NumPy's")


# ---- the whole loop in lockstep
def test_the_whole_loop_in_lockstep_with_a_host_model(gpu):
    """The device loop about the eccentric chief -- init, then max_outer = 8 rounds of prepare -> GPU QP solve -> advance -- on the 70
    trajectories of 13 stages of tests/_scvx_stage_case.LOCKSTEP, and a host model (HostLoop) that repeats every outer iteration in
    the host formulas from the same z and from nothing else of the device's, so that the QP tolerance does not enter.  The
    preconditions are asserted on the host model's records (lockstep_preconditions; tests/test_scvx_stage_host.py has them at ten
    times the margin with the CPU oracle).  Per outer iteration: lo, hi equal; A, B, q and the candidates within GPU_MARGIN x
    LOCKSTEP_FP64_VS_LD of the long-double formulas on the device's own inputs; every flag, count, take, radius, ub and n_active
    equal; costs and history rows within 1e-12 |J| plus what the bound on the states makes of a cost; older history rows and the
    candidates of inactive trajectories hold their bits."""
    c = st.LOCKSTEP
    p, host = st.lockstep_params(), st.lockstep_host()
    B, N, cap = c["B"], c["N"], c["max_outer"]
    table = st.table_of(p, N)
    loop = _loop(host.x0, N, p, tol=c["tol"], max_outer=cap)
    rng = np.random.default_rng(5)
    for k in ("u_cand", "x_cand", "history"):
        loop.t[k].copy_(_t(rng.standard_normal(tuple(loop.t[k].shape))))
    loop.init(c["tr_u"], c["tr_x"])
    solve = sc.gpu_qp_solver(True, z_on_device=True, **st.LOCKSTEP_QP)

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

    bound = {k: st.GPU_MARGIN * v for k, v in st.LOCKSTEP_FP64_VS_LD.items()}
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
        # A, B, q against the long-double formulas about the DEVICE's own reference (the same inputs)
        xprev = np.concatenate([host.x0[:, None, :], dev[it]["xb"][:, :-1, :]], axis=1)
        A_ld, B_ld = st.ld_linearise(xprev, dev[it]["ub"], p, table)
        q_ld = dc.linear_term(dev[it]["xb"], dev[it]["ub"], p.Q, p.R, p.QN, st.LD)
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
        x_ld = st.ld_rollout(host.x0, out["u_new"], p, table)       # the candidates' controls are equal (asserted below)
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
          {k: f"{worst[w] / st.LOCKSTEP_FP64_VS_LD[k]:.2f}" for k, w in (("x", "x_cand"), ("A", "A"), ("B", "B"), ("q", "q"))})


# ---- the two doors at e = 0
def test_the_e_0_table_through_the_stage_calls_agrees_with_the_circular_model(gpu):
    """rollout and prepare on scattered(65, 64, "circular"), once through admm_scvx_*_stage_device with the e = 0 table and once
    through admm_scvx_*_model_device with relative_circular(a): x, A, B and q of both lie within GPU_MARGIN x FP64_VS_LD of the
    long-double restatement, and of each other; lo and hi are equal."""
    name, B, N = "circular", 65, 64
    p = st.PARAMS[name]
    x0, u, x, tru, trx, active = st.scattered(B, N, name)
    r, c = st.reference(B, N, name), st.FP64_VS_LD[name, B, N]
    outs = []
    for model in (st.model_of(p), sc.relative_circular(st.A_KM)):
        loop = _loop(x0, N, p, model=model)
        got_x = loop.rollout(_t(u)).cpu().numpy()
        _load_scatter(loop, u, x, tru, trx, active)
        loop.prepare()
        outs.append(dict(_qp_of(loop, B, N), x=got_x, struct=type(loop.model)))
    stage, circ = outs
    assert (stage["struct"], circ["struct"]) == (_abi.CScvxStageDynamics, _abi.CScvxDynamics)
    for k in ("x", "A", "B", "q"):
        es, ec, d = _ld_err(stage[k], r["ld"][k]), _ld_err(circ[k], r["ld"][k]), float(np.abs(stage[k] - circ[k]).max())
        print(f"e = 0, {k}: stage door vs long double {es:.2e}, circular door {ec:.2e}, the two doors {d:.2e}; NumPy {c[k]:.1e}")
        assert es <= st.GPU_MARGIN * c[k] and ec <= st.GPU_MARGIN * c[k] and d <= st.GPU_MARGIN * c[k], k
    for k in ("lo", "hi"):
        np.testing.assert_array_equal(stage[k], circ[k])
        np.testing.assert_array_equal(stage[k], r[k])


# ---- pointer checks of the table
def test_the_table_pointer_is_checked_like_every_other_array(gpu, lib):
    """`nodes` as host memory (pageable and pinned) and as a device allocation that ends one double before its 4 n_nodes: each of
    the four calls gives ADMM_ERR_INVALID naming `nodes`, and every tensor of the state and the outputs holds the bits it held.
    The same calls with the loop's own table then give what a fresh loop gives."""
    p = st.PARAMS["random3"]
    state, _ = st.decision_inputs(66, 9, "elliptic")
    B, N = state["ub"].shape[:2]

    def fresh():
        loop = _loop(state["x0"], N, p, max_outer=4)
        loop.init(1.0, 2.0)
        return loop
    loop = fresh()
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
    count = 4 * (2 * p.substeps * N + 1)
    assert loop.nodes.numel() == count
    ALL = ("admm_scvx_rollout_stage_device", "admm_scvx_init_stage_device", "admm_scvx_prepare_stage_device", "admm_scvx_advance_stage_device")

    def call(name, nodes=None):
        dyn = _abi.CScvxStageDynamics.from_buffer_copy(loop.model)
        if nodes is not None:
            dyn.nodes = nodes
        dyn, params, s = C.byref(dyn), C.byref(loop.params), C.byref(loop.state)
        fn = getattr(lib, name)
        if name == ALL[0]:
            return fn(0, dyn, P(loop.x0), P(u), P(xout), None)
        if name == ALL[1]:
            return fn(0, dyn, params, P(loop.x0), s, 1.0, 2.0, None)
        if name == ALL[2]:
            return fn(0, dyn, params, P(loop.x0), s, *(P(outs[k]) for k in ("A", "B", "lo", "hi", "q")), None)
        return fn(0, dyn, params, P(loop.x0), P(z), s, C.byref(nact), None)

    hostv = np.zeros(count)
    pinned = torch.zeros(count, dtype=torch.float64).pin_memory()
    big = torch.zeros(3 * 2 ** 20, dtype=torch.float64, device=DEV)     # a block of its own in torch's allocator: its true end is known
    for name in ALL:
        for word, ptr in (("nodes is not device memory", _abi.dptr(hostv)), ("nodes is not device memory", P(pinned)),
                          (f"nodes ends before its {count} doubles", P(big[big.numel() - (count - 1):]))):
            assert call(name, ptr) == INVALID, (name, word)
            msg = lib.admm_last_error().decode()
            assert msg.startswith(name + ": ") and word in msg, (name, word, msg)
    torch.cuda.synchronize()
    for k, v in {**loop.t, **outs, "xout": xout}.items():
        assert torch.equal(v, before[k]), k
    assert nact.value == -5 and (big == 0).all() and (hostv == 0).all() and (pinned == 0).all()
    # and the same calls with their own table go through, with the results of a loop that saw no refusal
    other = fresh()
    for lp in (loop, other):
        lp.prepare()
    assert call(ALL[0]) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(xout.cpu().numpy(), other.rollout(u).cpu().numpy())
    for k in ("A", "B", "lo", "hi", "q"):
        assert torch.equal(getattr(loop, k), getattr(other, k)), k
    assert loop.advance(z) == other.advance(z)
    for k in loop.t:
        assert torch.equal(loop.t[k], other.t[k]), k


# ---- end to end
def test_the_device_loop_agrees_with_the_host_loop_about_an_eccentric_chief(gpu):
    """scvx_batch(model=relative_elliptic(7000, 0.3, 0.4), linearise_on="cuda:0", outer_on_device=True) on 8 trajectories with
    N = 40 against the host loop (NumPy outer step) and the torch route, all on the GPU solver: the same outer iterations and the
    same accept pattern for every trajectory, costs within the QP tolerance (1e-5 relative), and the device's x is the nonlinear
    trajectory under its u -- within GPU_MARGIN x NumPy's own distance from the long-double rollout of that u."""
    B = 8
    x0 = st.elliptic_x0(B)
    m = st.model_of(st.ELLIPTIC)
    args = st.elliptic_args(x0)
    t0 = time.perf_counter()
    host = sc.scvx_batch(*args, model=m, **st.EL_SCVX)
    t1 = time.perf_counter()
    torch_route = sc.scvx_batch(*args, model=m, linearise_on=DEV, qp_data_on_device=True, **st.EL_SCVX)
    t2 = time.perf_counter()
    res = sc.scvx_batch(*args, model=m, linearise_on=DEV, outer_on_device=True, **st.EL_SCVX)
    t3 = time.perf_counter()
    p = st.ELLIPTIC._replace(dt=st.EL_DT)
    table = st.table_of(p, st.EL_N)
    worst_cost = worst_x = yard = 0.0
    for b, r in enumerate(res):
        for o in (host[b], torch_route[b]):
            assert (r.outer_iterations, r.accepted, r.converged) == (o.outer_iterations, o.accepted, o.converged), (b, r.history, o.history)
            assert [h["accepted"] for h in r.history] == [h["accepted"] for h in o.history], b
            worst_cost = max(worst_cost, abs(r.cost - o.cost) / abs(o.cost))
        x_ld = st.ld_rollout(x0[b], r.u, p, table)
        worst_x = max(worst_x, _ld_err(r.x, x_ld))
        yard = max(yard, _ld_err(sc.rollout(x0[b], r.u, st.EL_DT, model=m), x_ld))
        assert (np.abs(r.u) <= st.EL_U_MAX).all() and np.linalg.norm(r.x[-1, :3]) < 0.5
    print(f"eccentric rendezvous, B={B}: host loop {t1 - t0:.2f} s, torch route {t2 - t1:.2f} s, device loop {t3 - t2:.2f} s; outer iterations "
          f"{min(r.outer_iterations for r in res)}..{max(r.outer_iterations for r in res)}, {sum(r.converged for r in res)} converged; "
          f"cost rel {worst_cost:.2e}, x vs long double {worst_x:.2e} (NumPy: {yard:.2e})")
    assert len(res) == B and all(r.converged for r in res)
    assert worst_cost <= 1e-5 and worst_x <= st.GPU_MARGIN * yard
