"""Inputs and host references of the device outer-step tests (tests/test_gpu_scvx_device.py), built on the CPU:
the scatter of tests/_scvx_case.py (X0 (1 + 0.05 randn), default_rng(11), controls uniform in +-3) and, for the decision test, one
outer iteration's inputs on which the HOST reference scvx.outer_update takes every branch."""
import functools

import numpy as np

from admm_library_amd import scvx as sc

import _scvx_case as case

SHAPES = [(1, 1), (63, 7), (65, 64), (130, 65)]      # lone lane; partial wave; the wave boundary in B and N; several workgroups
DT = 2 * np.pi / 80
TOL, RHO_REJECT, RHO_EXPAND = 1e-7, 0.1, 0.7
BRANCHES = ("model_converged", "accepted_expanded", "accepted", "rejected", "step_converged", "inactive")


@functools.lru_cache(maxsize=None)
def scattered(B, N):
    """x0 (B, 6), u (B, N, 3), the host rollout x (B, N, 6), per-trajectory radii and an active mask with some trajectories off."""
    rng = np.random.default_rng(11)
    x0 = case.X0[None] * (1.0 + 0.05 * rng.standard_normal((B, 6)))
    u = rng.uniform(-case.U_MAX, case.U_MAX, (B, N, 3))
    x = sc.rollout(x0, u, DT)
    tru = rng.uniform(0.5, 2.0, B)
    trx = rng.uniform(50.0, 200.0, B)
    active = np.ones(B, bool)
    active[::5] = False
    if B == 1:
        active[:] = True
    for a in (x0, u, x, tru, trx, active):
        a.setflags(write=False)
    return x0, u, x, tru, trx, active


@functools.lru_cache(maxsize=None)
def linearised(B, N):
    """scvx.linearise and scvx.correction_qp_batch (host) about scattered(B, N): A, B, lo, hi, q."""
    x0, u, x, tru, trx, active = scattered(B, N)
    p = sc.correction_qp_batch(x, u, x0, DT, case.Q, case.R, case.QN, -case.U_MAX, case.U_MAX, np.where(active, tru, 0.0),
                               np.where(active, trx, 0.0))
    out = (p.A, p.B, p.lo, p.hi, p.q.reshape(B, N, 9))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def decision_inputs(B=66, N=9):
    """One advance call's inputs, six trajectories apart per branch (b % 6 -> BRANCHES), and what scvx.outer_update makes of them.
    The correction du, dx of the QP about (ub, xb) comes from the CPU oracle; the branches are steered by what z is made of it:
      0  z = 0: the model predicts no decrease                     -> stops
      1  z = the QP's solution: the model is accurate              -> accepted, radii doubled
      2  du halved but dx kept: the model promises too much        -> accepted, radii kept
      3  du reversed but dx kept                                   -> rejected, radii halved
      4  du ~ 1e-8 and a reference cost J above the true one       -> accepted (a decrease the step did not earn), stops: |du| <= tol
      5  inactive on entry, z arbitrary                            -> untouched
    J is an INPUT of the decision (the cost the loop carries), so 4 is a legitimate state of the interface."""
    rng = np.random.default_rng(11)
    x0 = case.X0[None] * (1.0 + 0.05 * rng.standard_normal((B, 6)))
    ub = rng.uniform(-case.U_MAX, case.U_MAX, (B, N, 3))
    xb = sc.rollout(x0, ub, DT)
    J = sc.trajectory_cost(xb, ub, case.Q, case.R, case.QN)
    tru = rng.uniform(0.05, 0.2, B)
    trx = rng.uniform(50.0, 200.0, B)
    kind = np.arange(B) % 6
    active = kind != 5
    p = sc.correction_qp_batch(xb, ub, x0, DT, case.Q, case.R, case.QN, -case.U_MAX, case.U_MAX, np.where(active, tru, 0.0),
                               np.where(active, trx, 0.0))
    zq = case.oracle_qp_solver(**case.QP)(p)[0].reshape(B, N, 9)
    z = zq.copy()
    z[kind == 0] = 0.0
    z[kind == 2, :, :3] *= 0.5
    z[kind == 3, :, :3] *= -1.0
    z[kind == 4] = 0.0
    z[kind == 4, :, :3] = rng.uniform(-1e-8, 1e-8, (int((kind == 4).sum()), N, 3))
    z[kind == 5] = rng.uniform(-1.0, 1.0, (int((kind == 5).sum()), N, 9))
    J = J.copy()
    J[kind == 4] += 5.0
    converged = np.zeros(B, bool)
    converged[kind == 5] = rng.integers(0, 2, int((kind == 5).sum())).astype(bool)
    accepted = rng.integers(0, 3, B)
    outer = accepted + rng.integers(0, 2, B)
    state = dict(x0=x0, ub=ub, xb=xb, J=J, tr_u=tru, tr_x=trx, active=active, converged=converged, accepted=accepted, outer=outer, z=z)
    # the host reference: the candidate as scvx_batch builds it, then outer_update on copies
    du, dx = z[..., :3], z[..., 3:]
    J_lin = sc.trajectory_cost(xb + dx, ub + du, case.Q, case.R, case.QN)
    u_new = np.clip(ub + du, -case.U_MAX, case.U_MAX)
    x_new = sc.rollout(x0, u_new, DT)
    J_new = sc.trajectory_cost(x_new, u_new, case.Q, case.R, case.QN)
    ref = dict(J=J.copy(), tr_u=tru.copy(), tr_x=trx.copy(), active=active.copy(), converged=converged.copy(), accepted=accepted.copy())
    take, records = sc.outer_update(ref["J"], J_lin, J_new, np.abs(du).max(axis=(1, 2)), ref["tr_u"], ref["tr_x"], ref["active"],
                                    ref["converged"], ref["accepted"], TOL, RHO_REJECT, RHO_EXPAND)
    ref.update(take=take, records=records, u_new=u_new, x_new=x_new, outer=outer + active, kind=kind)
    return state, ref


def branch_of(b, state, ref):
    """Which branch the reference took for trajectory b."""
    if not state["active"][b]:
        return "inactive"
    rec = ref["records"][b]
    stopped = not ref["active"][b]
    if not rec["accepted"]:
        return "model_converged" if stopped else "rejected"
    if stopped:
        return "step_converged"
    return "accepted_expanded" if ref["tr_u"][b] == 2.0 * state["tr_u"][b] else "accepted"
