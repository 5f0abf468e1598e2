"""Device outer step of the batched SCvx loop (ADMM_HIP_HAS_SCVX), host side: the ABI surface, the ctypes mirror
of its structs, the refusals that need no GPU, the refactored decision block against the loop it was taken from, and the register
report of the new kernels.  No GPU."""
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
