"""The outer step of the batched successive-convexification loop on the device (ADMM_HIP_HAS_SCVX) against the
host code it mirrors: scvx.rollout, scvx.linearise, scvx.correction_qp_batch, scvx.outer_update and scvx_batch itself.  Inputs and
host references: tests/_scvx_device_case.py (built once, shared, read-only)."""
import ctypes as C

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

    cap = int(ref["outer"].max()) + 1
    loop = _loop(state["x0"], N, max_outer=cap)
    rng = np.random.default_rng(5)
    junk = {k: rng.standard_normal(tuple(loop.t[k].shape)) for k in ("u_cand", "x_cand", "history")}
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
        rec = ref["records"][b]
        row = dict(zip(_abi.SCVX_HISTORY_FIELDS, got["history"][it, b]))
        others = np.delete(np.arange(cap), it)
        np.testing.assert_array_equal(got["history"][others, b], junk["history"][others, b])
        assert bool(row["accepted"]) == rec["accepted"] and row["accepted"] in (0.0, 1.0)
        assert row["tr_u"] == rec["tr_u"] and row["tr_x"] == rec["tr_x"]
        assert row["du_max"] == rec["du_max"]                       # a maximum of |du|: exact
        J = abs(rec["cost"])
        bounds = dict(cost=1e-12 * J, cost_candidate=1e-12 * J, predicted=1e-12 * J, actual=1e-12 * J)
        for k, bound in bounds.items():
            worst[k] = max(worst.get(k, 0.0), abs(row[k] - rec[k]) / J)
            assert abs(row[k] - rec[k]) <= bound, (b, k, row[k], rec[k])
        if taken[b] == "model_converged":
            # predicted is a rounding residue of J - J (0 on the host): its sign, and so ratio = -inf or actual / predicted, is noise
            assert abs(row["predicted"]) <= 1e-12 * J
        else:
            assert abs(row["ratio"] - rec["ratio"]) <= 1e-12 * J * (1.0 + abs(rec["ratio"])) / abs(rec["predicted"]), (b, row, rec)
        # the candidate; the reference takes it where accepted
        assert np.abs(got["u_cand"][b] - ref["u_new"][b]).max() == 0.0
        assert np.abs(got["x_cand"][b] - ref["x_new"][b]).max() <= 5e-11
        if ref["take"][b]:
            np.testing.assert_array_equal(got["ub"][b], got["u_cand"][b])
            np.testing.assert_array_equal(got["xb"][b], got["x_cand"][b])
        else:
            np.testing.assert_array_equal(got["ub"][b], state["ub"][b])
            np.testing.assert_array_equal(got["xb"][b], state["xb"][b])
    print("decisions: worst |device - host| / |J| per field:", {k: f"{v:.2e}" for k, v in worst.items()})


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
