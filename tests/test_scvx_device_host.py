"""Device outer step of the batched SCvx loop (ADMM_HIP_HAS_SCVX), host side: the ABI surface, the ctypes mirror
of its structs, the refusals that need no GPU, the refactored decision block against the loop it was taken from, and the register
report of the new kernels; and the inputs of tests/test_gpu_scvx_device.py themselves (tests/_scvx_device_case.py): that the
long-double reference is extended precision, that the recorded NumPy-vs-long-double constants are current, that every precondition
of the GPU tests holds on the host reference, and that each input tells a wrong kernel from a right one.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import admm_library_amd as pkg
from admm_library_amd import _abi
from admm_library_amd import scvx as sc

import _scvx_case as case
import _scvx_device_case as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("admm_scvx_rollout_device", "admm_scvx_init_device", "admm_scvx_prepare_device", "admm_scvx_advance_device")


def test_abi_surface(lib):
    hdr = open(os.path.join(ROOT, "include", "admm_hip.h")).read()
    assert "#define ADMM_HIP_HAS_SCVX 1" in hdr
    assert "#define ADMM_HIP_ABI_VERSION 9" in hdr and lib.admm_abi_version() == 9
    for name in SYMBOLS:
        assert name in pkg.solver._SIGNATURES and hasattr(lib, name)


def test_ctypes_structs_have_the_c_sizes(tmp_path):
    """sizeof and the offset of the last field of each struct, from a C program compiled against the header."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "admm_hip.h"\n'
                   "int main(void) { printf(\"%zu %zu %zu %zu %zu %zu\\n\", sizeof(admm_scvx_model), offsetof(admm_scvx_model, rc),\n"
                   "  sizeof(admm_scvx_params), offsetof(admm_scvx_params, rho_expand), sizeof(admm_scvx_state),\n"
                   "  offsetof(admm_scvx_state, history_capacity)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_abi.CScvxModel), _abi.CScvxModel.rc.offset, C.sizeof(_abi.CScvxParams), _abi.CScvxParams.rho_expand.offset,
                   C.sizeof(_abi.CScvxState), _abi.CScvxState.history_capacity.offset]
    assert C.sizeof(_abi.CScvxParams) == 8 * (36 + 9 + 36 + 3 + 3 + 4)


def test_outer_on_device_needs_the_device_linearisation():
    x0 = case.X0[None]
    args = (x0, 5, case.DT, case.Q, case.R, case.QN, -case.U_MAX, case.U_MAX)
    with pytest.raises(ValueError, match="outer_on_device"):
        sc.scvx_batch(*args, outer_on_device=True)
    with pytest.raises(ValueError, match="outer_on_device"):
        sc.scvx_batch(*args, outer_on_device=True, linearise_on="cuda:0", step=lambda s, u, dt: sc.rk4_step(s, u, dt))


def test_argument_checks_come_before_any_hip_call(lib):
    """batch = 0 and NULL pointers are refused with the argument's name -- on a machine without a GPU too (ADMM_ERR_INVALID, not
    ADMM_ERR_NO_DEVICE or ADMM_ERR_HIP): these checks precede the first HIP call."""
    model = _abi.CScvxModel(N=4, batch=0, substeps=4, dt=0.1, rc=sc.RC_KM)
    params = _abi.CScvxParams(fd_eps=1e-6, tol=1e-6, rho_reject=0.1, rho_expand=0.7)
    state = _abi.CScvxState(history_capacity=4)
    n = C.c_int32(-1)
    null = _abi.c_double_p()
    calls = {"admm_scvx_rollout_device": lambda m: lib.admm_scvx_rollout_device(0, m, null, null, null, None),
             "admm_scvx_init_device": lambda m: lib.admm_scvx_init_device(0, m, C.byref(params), null, C.byref(state), 1.0, 1.0, None),
             "admm_scvx_prepare_device": lambda m: lib.admm_scvx_prepare_device(0, m, C.byref(params), null, C.byref(state), null, null,
                                                                                null, null, null, None),
             "admm_scvx_advance_device": lambda m: lib.admm_scvx_advance_device(0, m, C.byref(params), null, null, C.byref(state),
                                                                                C.byref(n), None)}
    for name, fn in calls.items():
        assert fn(C.byref(model)) == 1
        assert lib.admm_last_error().decode() == name + ": model.batch must be >= 1"
        assert fn(None) == 1 and "model is NULL" in lib.admm_last_error().decode()
    model.batch = 3
    for name, fn in calls.items():
        assert fn(C.byref(model)) == 1
        msg = lib.admm_last_error().decode()
        assert msg.startswith(name + ": ") and msg.endswith(" is NULL"), msg
    assert n.value == -1


def _scvx_batch_before(x0, N, dt, Q, R, QN, u_lo, u_hi, qp_solver, tr_u, tr_x, max_outer, tol, rho_reject=0.1, rho_expand=0.7):
    """scvx_batch as it stood before its decision block became outer_update (host linearisation), kept here as the recorded run's
    source: the loop over trajectories is written out."""
    x0 = np.atleast_2d(np.asarray(x0, np.float64))
    Bn = x0.shape[0]
    n, m = 6, 3
    u_lo = np.broadcast_to(np.asarray(u_lo, np.float64), (m,))
    u_hi = np.broadcast_to(np.asarray(u_hi, np.float64), (m,))
    ub = np.zeros((Bn, N, m))
    xb = sc.rollout(x0, ub, dt)
    J = sc.trajectory_cost(xb, ub, Q, R, QN)
    tru, trx = np.full(Bn, float(tr_u)), np.full(Bn, float(tr_x))
    active, converged, accepted = np.ones(Bn, bool), np.zeros(Bn, bool), np.zeros(Bn, int)
    hist = [[] for _ in range(Bn)]
    for it in range(1, max_outer + 1):
        if not active.any():
            break
        p = sc.correction_qp_batch(xb, ub, x0, dt, Q, R, QN, u_lo, u_hi, np.where(active, tru, 0.0), np.where(active, trx, 0.0))
        z, admm_iters = qp_solver(p)
        d = np.asarray(z, np.float64).reshape(Bn, N, m + n)
        du, dx = d[..., :m], d[..., m:]
        J_lin = sc.trajectory_cost(xb + dx, ub + du, Q, R, QN)
        u_new = np.clip(ub + du, u_lo, u_hi)
        x_new = sc.rollout(x0, u_new, dt)
        J_new = sc.trajectory_cost(x_new, u_new, Q, R, QN)
        predicted, actual = J - J_lin, J - J_new
        for b in np.flatnonzero(active):
            ratio = actual[b] / predicted[b] if predicted[b] > 0 else -np.inf
            step_norm = float(np.abs(du[b]).max())
            rec = dict(iteration=it, cost=float(J[b]), cost_candidate=float(J_new[b]), predicted=float(predicted[b]),
                       actual=float(actual[b]), ratio=float(ratio), tr_u=float(tru[b]), tr_x=float(trx[b]), du_max=step_norm,
                       admm_iterations=admm_iters, accepted=False)
            if predicted[b] <= tol * max(1.0, abs(J[b])):
                hist[b].append(rec)
                converged[b], active[b] = True, False
                continue
            if ratio >= rho_reject:
                ub[b], xb[b], J[b] = u_new[b], x_new[b], J_new[b]
                accepted[b] += 1
                rec["accepted"] = True
                if ratio >= rho_expand:
                    tru[b], trx[b] = 2.0 * tru[b], 2.0 * trx[b]
            else:
                tru[b], trx[b] = 0.5 * tru[b], 0.5 * trx[b]
            hist[b].append(rec)
            if rec["accepted"] and step_norm <= tol:
                converged[b], active[b] = True, False
    return ub, xb, J, accepted, converged, hist


def test_outer_update_reproduces_the_loop_it_was_taken_from():
    """A 3-trajectory, N = 20 run with the CPU oracle as QP solver, recorded by the loop as it stood (above) and repeated by
    scvx_batch over outer_update: the same bits -- controls, states, costs, counts, every history record.  Stages of a fifth of an orbit under wide
    initial radii make the linear model poor: the run rejects and shrinks, accepts with and without expansion, stops on both rules
    or runs into max_outer (asserted below)."""
    rng = np.random.default_rng(11)
    N, dt = 20, 2 * np.pi / 5
    x0s = case.X0[None] * (1.0 + 0.05 * rng.standard_normal((3, 6)))
    kw = dict(tr_u=8.0, tr_x=800.0, max_outer=12, tol=1e-7)
    args = (x0s, N, dt, case.Q * 4, case.R * 4, case.QN, -case.U_MAX, case.U_MAX)
    ub, xb, J, accepted, converged, hist = _scvx_batch_before(*args, qp_solver=case.oracle_qp_solver(**case.QP), **kw)
    res = sc.scvx_batch(*args, qp_solver=case.oracle_qp_solver(**case.QP), **kw)
    for b, r in enumerate(res):
        np.testing.assert_array_equal(r.u, ub[b])
        np.testing.assert_array_equal(r.x, xb[b])
        assert r.cost == J[b] and r.accepted == accepted[b] and r.converged == converged[b] and r.outer_iterations == len(hist[b])
        assert r.history == hist[b]
    kinds = {(h["accepted"], bool(h["ratio"] >= 0.7)) for h in sum(hist, [])}
    print("recorded run:", [(len(h), int(a), bool(c)) for h, a, c in zip(hist, accepted, converged)], sorted(kinds))
    assert kinds >= {(True, True), (True, False), (False, False)} and converged.any() and not converged.all()


def test_the_new_kernels_do_not_spill(tmp_path):
    """csrc/admm_scvx.hip compiled on its own with the library's flags and the compiler's resource report: the four kernels (the
    rollout in both forms) are there and no kernel of the unit uses scratch memory."""
    import __graft_entry__ as ge
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-Rpass-analysis=kernel-resource-usage"] + ge.HIPCC_FLAGS +
                       ["-c", os.path.join(ge.CSRC, "admm_scvx.hip"), "-o", str(tmp_path / "admm_scvx.o")],
                       cwd=ge.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = ge.parse_resource_usage(r.stderr)
    mine = [x for x in rows if "scvx_" in x["name"]]
    for x in mine:
        print(f'{x["name"]}: {x["vgpr"]} VGPRs, {x["agpr"]} AGPRs, {x["sgpr"]} SGPRs, LDS {x["lds"]} B, scratch {x["scratch"]} B, '
              f'occupancy {x["occupancy"]}')
    names = sorted(x["name"].split("<")[0].split("::")[-1] for x in mine)
    assert names == ["scvx_advance_kernel", "scvx_commit_kernel", "scvx_linearise_kernel", "scvx_rollout_kernel", "scvx_rollout_kernel"]
    assert all(x["scratch"] == 0 and x["vgpr_spill"] == 0 for x in rows), [x["name"] for x in rows if x["scratch"]]
    assert all(x["lds"] <= 65536 for x in rows)


# ---- the inputs of the GPU tests (tests/_scvx_device_case.py)
def test_long_double_is_extended_precision():
    """The reference of the GENERAL tests must be finer than fp64 where the suite runs (x86: 80-bit, eps = 2^-63)."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    x0, u, x, *_ = dc.scattered_general(63, 7, 3)
    p = dc.GENERAL[3]
    ld = dc.ld_rollout(x0, u, p.dt, p.substeps, p.rc)
    assert ld.dtype == np.longdouble and 0 < np.abs(ld - x).max() < 1e-11
    J = sc.trajectory_cost(x, u, p.Q, p.R, p.QN)
    assert (np.abs(dc.ld_trajectory_cost(x, u, p.Q, p.R, p.QN) - J) <= 1e-14 * np.abs(J)).all()


def test_general_is_general():
    """GENERAL: dense SPD weights with the scenario's diagonals and every off-diagonal entry >= 0.1 of the geometric mean of its two
    diagonal entries; six box values of distinct magnitudes; substeps 1 and 3, another rc, another dt, fd_eps 1e-5."""
    assert sorted(dc.GENERAL) == [1, 3]
    for s, p in dc.GENERAL.items():
        for M, M0 in ((p.Q, case.Q), (p.R, case.R), (p.QN, case.QN)):
            d = np.sqrt(np.diag(M))
            off = ~np.eye(len(d), dtype=bool)
            np.testing.assert_array_equal(M, M.T)
            np.testing.assert_allclose(np.diag(M), np.diag(M0), rtol=1e-15)
            assert np.linalg.eigvalsh(M).min() > 0 and (np.abs(M)[off] >= 0.1 * np.outer(d, d)[off]).all()
        mags = np.abs(np.concatenate([p.u_lo, p.u_hi]))
        assert len(set(mags.tolist())) == 6 and (p.u_lo < 0).all() and (p.u_hi > 0).all()
        assert p.substeps == s != 4 and p.rc != sc.RC_KM and p.dt != dc.DT and p.fd_eps == 1e-5


def test_the_original_inputs_are_what_they_were():
    """SHAPES, scattered, linearised and decision_inputs() with its defaults: sums recorded before decision_inputs took parameters."""
    assert dc.SHAPES == [(1, 1), (63, 7), (65, 64), (130, 65)]
    sums = {(1, 1): (476.8583430225166, 9709.60962294856), (63, 7): (90106.26605024634, 527614.3064976961),
            (65, 64): (295673.44036039966, 133883.97141898965), (130, 65): (603357.0756154201, 293780.9925621709)}
    for shape, want in sums.items():
        got = (float(sum(np.asarray(a, float).sum() for a in dc.scattered(*shape))), float(sum(a.sum() for a in dc.linearised(*shape))))
        assert got == want, shape
    st, ref = dc.decision_inputs()
    assert float(sum(np.asarray(v, float).sum() for v in st.values())) == 33462908.17951297
    assert float(ref["J"].sum() + ref["x_new"].sum() + ref["tr_u"].sum()) == 33437912.884325143
    assert dc.decision_inputs() is dc.decision_inputs(66, 9, "original") or dc.decision_inputs()[0]["z"].tobytes() == dc.decision_inputs(66, 9, "original")[0]["z"].tobytes()


@pytest.mark.parametrize("substeps", [1, 3])
@pytest.mark.parametrize("B,N", dc.SHAPES)
def test_recorded_fp64_vs_long_double_constants_are_current(B, N, substeps):
    """FP64_VS_LD[substeps, B, N] bounds max |NumPy fp64 - long double| per quantity on scattered_general(B, N, substeps) today,
    and is no more than twice it: the GPU bounds (GPU_MARGIN x the constant) are neither stale nor padded."""
    got = dc.fp64_vs_ld(B, N, substeps)
    print(f"fp64 vs long double, substeps {substeps}, B={B} N={N}:", {k: f"{v:.3e}" for k, v in got.items()})
    for k, v in got.items():
        c = dc.FP64_VS_LD[substeps, B, N][k]
        assert v <= c <= 2.0 * v, (k, v, c)


def _decision_case(B, N, params):
    state, ref = dc.decision_inputs(B, N, params)
    return state, ref, [dc.branch_of(b, state, ref) for b in range(B)]


@pytest.mark.parametrize("params", dc.DECISION_PARAMS)
@pytest.mark.parametrize("B,N", dc.DECISION_SHAPES)
def test_decision_inputs_meet_their_preconditions_with_margin(B, N, params):
    """What tests/test_gpu_scvx_device.py asserts first, at ten times the knife-edge margin: every branch is taken B // 6 times (the
    lone trajectory of B = 1 is accepted), no ratio within 1e-2 of a threshold, and under the asymmetric box the reversed step of the
    rejected branch is clipped on both sides of every axis."""
    state, ref, taken = _decision_case(B, N, params)
    if B == 1:
        assert taken == ["accepted"]
    else:
        assert all(taken.count(t) >= B // 6 for t in dc.BRANCHES), {t: taken.count(t) for t in dc.BRANCHES}
        assert [t == "inactive" for t in taken] == (ref["kind"] == 5).tolist()
    assert dc.ratio_margin(ref["records"].values()) > 1e-2
    if params != "original" and B >= 6:
        below, above, exact = dc.clip_activity(state, ref, dc.PARAMS[params])
        assert (below >= 1).all() and (above >= 1).all() and exact, (below, above, exact)
    p = dc.PARAMS[params]
    assert (state["ub"] >= p.u_lo).all() and (state["ub"] <= p.u_hi).all()


def test_lockstep_preconditions_hold_with_ten_times_the_margin():
    """The host model of the lockstep test with the CPU oracle as QP solver: every precondition of
    test_gpu_scvx_device.py::test_whole_loops_in_lockstep_with_a_host_model holds at ten times the margin it asks for there; and
    LOCKSTEP_FP64_VS_LD, from which that test takes its bounds on A, B, q and x, is what NumPy differs from long double over this
    run (states up to 1.7e3 km, ten times part 1's)."""
    host = dc.lockstep_host()
    solve = case.oracle_qp_solver(**dc.LOCKSTEP_QP)
    p = host.p
    worst = dict(x=0.0, A=0.0, B=0.0, q=0.0)
    for it in range(dc.LOCKSTEP["max_outer"]):
        assert host.active.any()
        qp = host.qp()
        xprev = np.concatenate([host.x0[:, None, :], host.xb[:, :-1, :]], axis=1)
        A, Bm = dc.ld_linearise(xprev, host.ub, p.dt, p.substeps, p.rc, p.fd_eps)
        q = dc.linear_term(host.xb, host.ub, p.Q, p.R, p.QN, dc.LD)
        out = host.advance(solve(qp)[0], it)
        x = dc.ld_rollout(host.x0, out["u_new"], p.dt, p.substeps, p.rc)
        for k, a, b in (("A", qp.A, A), ("B", qp.B, Bm), ("q", qp.q.reshape(q.shape), q), ("x", out["x_new"], x)):
            worst[k] = max(worst[k], float(np.abs(a - b).max()))
    seen = dc.lockstep_preconditions(host, margin=10.0)
    print("lockstep with the oracle:", {k: v for k, v in seen.items() if k != "mixed"}, len(seen["mixed"]), "mixed; fp64 vs long double",
          {k: f"{v:.3e}" for k, v in worst.items()}, f"; |x| up to {np.abs(host.xb).max():.0f}")
    assert (host.outer[host.active] == dc.LOCKSTEP["max_outer"]).all()
    for k in worst:
        assert worst[k] <= dc.LOCKSTEP_FP64_VS_LD[k] <= 2.0 * worst[k], (k, worst[k])


def _box(p, u, tu, u_lo, u_hi):
    return np.maximum(u_lo - u, -tu[:, None, None]), np.minimum(u_hi - u, tu[:, None, None])


ERRORS = ("diagonal_weights", "Q_at_the_last_stage", "axis_0_bounds_everywhere", "bounds_swapped_and_negated", "substeps_4", "rc_RC_KM",
          "divisor_2e-6", "inactive_candidate_stored")


@pytest.mark.parametrize("error", ERRORS)
def test_the_inputs_tell_a_wrong_kernel_from_a_right_one(error):
    """One deliberate error in the HOST formulas at a time.  On the new inputs (GENERAL, the decision shapes) the erroneous result is
    at least 100 x the GPU test's tolerance for that quantity away from the true one -- or different at all where the GPU test asks
    for equality.  On the old inputs (the scenario; B = 66, N = 9) it is identical wherever the old inputs could not see the error:
    that is the gap the new input closes.  (Q at the last stage and a stored inactive candidate the old inputs do see -- at one
    shape and with one wave past the first.)"""
    for B, N in dc.SHAPES:
        x0o, uo, xo, truo, trxo, acto = dc.scattered(B, N)
        Ao, Bo, loo, hio, qo = dc.linearised(B, N)
        for s in (1, 3):
            p = dc.GENERAL[s]
            tol = {k: 100.0 * dc.GPU_MARGIN * v for k, v in dc.FP64_VS_LD[s, B, N].items()}
            x0, u, x, tru, trx, active = dc.scattered_general(B, N, s)
            r = dc.reference_general(B, N, s)
            q, A, Bm = r["np"]["q"], r["np"]["A"], r["np"]["B"]
            tu = np.where(active, tru, 0.0)
            xprev = np.concatenate([x0[:, None, :], x[:, :-1, :]], axis=1)
            if error == "diagonal_weights":
                d = np.abs(r["q_diag"] - q)
                assert d[..., :3].max() >= tol["q"] and d[:, -1, 3:].max() >= tol["q"] and (N == 1 or d[:, :-1, 3:].max() >= tol["q"])
                np.testing.assert_array_equal(dc.linear_term(xo, uo, *(np.diag(np.diag(M)) for M in (case.Q, case.R, case.QN))), qo)
            elif error == "Q_at_the_last_stage":
                assert np.abs(r["q_qlast"] - q)[:, -1, 3:].max() >= tol["q"]
                assert np.abs(dc.linear_term(xo, uo, case.Q, case.R, case.Q) - qo).max() > 1e-13 * np.abs(qo).max()    # seen before too
            elif error in ("axis_0_bounds_everywhere", "bounds_swapped_and_negated"):
                wrong = (lambda lo, hi: (np.full(3, lo[0]), np.full(3, hi[0]))) if error[0] == "a" else (lambda lo, hi: (-hi, -lo))
                lo, hi = _box(p, u, tu, *wrong(p.u_lo, p.u_hi))
                assert not np.array_equal(lo, r["lo"][..., :3]) and not np.array_equal(hi, r["hi"][..., :3])
                lo, hi = _box(p, uo, np.where(acto, truo, 0.0), *wrong(dc.ORIGINAL.u_lo, dc.ORIGINAL.u_hi))
                np.testing.assert_array_equal(lo, loo[..., :3])
                np.testing.assert_array_equal(hi, hio[..., :3])
            elif error in ("substeps_4", "rc_RC_KM"):
                step = dc.functools.partial(sc.rk4_step, substeps=4, rc=p.rc) if error == "substeps_4" else dc.functools.partial(sc.rk4_step, substeps=s, rc=sc.RC_KM)
                assert np.abs(sc.rollout(x0, u, p.dt, step) - x).max() >= tol["x"]
                Aw, Bw = sc.linearise(xprev, u, p.dt, step, p.fd_eps)
                # the Jacobians of so short a stage feel the substeps less: 1 for 4 moves A by a few times its GPU bound (asserted: more
                # than the bound), 3 for 4 by less than the bound -- it is the rollout that shows a wrong substeps 100-fold.  A wrong
                # rc shows 100-fold in A as well
                dA = np.abs(Aw - A).max()
                assert dA >= tol["A"] if error == "rc_RC_KM" else (s == 3 or dA >= tol["A"] / 100.0), (B, N, s, dA)
                np.testing.assert_array_equal(sc.rollout(x0o, uo, dc.DT, dc.functools.partial(sc.rk4_step, substeps=4, rc=sc.RC_KM)), xo)
            elif error == "divisor_2e-6":
                assert np.abs(A * (2 * p.fd_eps) / 2e-6 - A).max() >= tol["A"] and np.abs(Bm * (2 * p.fd_eps) / 2e-6 - Bm).max() >= tol["B"]
                np.testing.assert_array_equal(Ao * (2 * dc.ORIGINAL.fd_eps) / 2e-6, Ao)
    # the decision inputs: costs, the candidate's clip, what an inactive trajectory leaves alone
    for B, N in dc.DECISION_SHAPES:
        for params in dc.DECISION_PARAMS:
            p = dc.PARAMS[params]
            state, ref = dc.decision_inputs(B, N, params)
            raw = state["ub"] + state["z"][..., :3]
            on = state["active"]
            if error == "diagonal_weights":
                J = sc.trajectory_cost(ref["x_new"], ref["u_new"], p.Q, p.R, p.QN)
                Jd = sc.trajectory_cost(ref["x_new"], ref["u_new"], *(np.diag(np.diag(M)) for M in (p.Q, p.R, p.QN)))
                if params == "original":
                    np.testing.assert_array_equal(Jd, J)
                else:
                    assert (np.abs(Jd - J) >= 100.0 * 1e-12 * np.abs(J)).all()
            elif error in ("axis_0_bounds_everywhere", "bounds_swapped_and_negated") and B >= 6:
                lo, hi = (np.full(3, p.u_lo[0]), np.full(3, p.u_hi[0])) if error[0] == "a" else (-p.u_hi, -p.u_lo)
                same = np.array_equal(np.clip(raw, lo, hi)[on], ref["u_new"][on])
                assert same == (params == "original"), (B, N, params)
            elif error == "inactive_candidate_stored" and B >= 6:
                junk = dc.decision_junk(B, N, int(ref["outer"].max()) + 1)
                off = np.flatnonzero(~on)
                assert all((ref["u_new"][b] != junk["u_cand"][b]).any() and (ref["x_new"][b] != junk["x_cand"][b]).any() for b in off)
                if B >= 66:
                    assert (off > 63).any()                       # ... and past the first wave
                if B == 200:
                    assert set((off // 64).tolist()) == {0, 1, 2, 3}
