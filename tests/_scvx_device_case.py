"""Inputs and host references of the device outer-step tests (tests/test_gpu_scvx_device.py), built on the CPU:
the scatter of tests/_scvx_case.py (X0 (1 + 0.05 randn), default_rng(11), controls uniform in +-3) and, for the decision test, one
outer iteration's inputs on which the HOST reference scvx.outer_update takes every branch.
Next to that scenario (ORIGINAL: diagonal weights, one scalar box, substeps 4, RC_KM, eps 1e-6) stands a second parameter set, GENERAL
(dense weights, a per-axis asymmetric box, other model settings), with an extended-precision (np.longdouble) restatement of the
model as its reference, and a host model of the whole outer loop (HostLoop) that the device loop is replayed against."""
import collections
import dataclasses
import functools

import numpy as np

from admm_library_amd import scvx as sc

import _scvx_case as case

SHAPES = [(1, 1), (63, 7), (65, 64), (130, 65)]      # lone lane; partial wave; the wave boundary in B and N; several workgroups
DT = 2 * np.pi / 80
TOL, RHO_REJECT, RHO_EXPAND = 1e-7, 0.1, 0.7
BRANCHES = ("model_converged", "accepted_expanded", "accepted", "rejected", "step_converged", "inactive")


Params = collections.namedtuple("Params", "name Q R QN u_lo u_hi dt substeps rc fd_eps")


def _dense_spd(diag, rng):
    """Symmetric, diagonal `diag`, every off-diagonal entry +-(0.10 .. 0.18) sqrt(d_i d_j): the scaled matrix is strictly diagonally
    dominant (at most 5 x 0.18 < 1 off the diagonal of a row), hence positive definite."""
    n = len(diag)
    c = np.triu(rng.uniform(0.10, 0.18, (n, n)) * rng.choice([-1.0, 1.0], (n, n)), 1)
    d = np.sqrt(np.asarray(diag, np.float64))
    return (c + c.T + np.eye(n)) * np.outer(d, d)


def _general(substeps):
    rng = np.random.default_rng(2024)
    Q, R, QN = (_dense_spd(np.diag(a), rng) for a in (case.Q, case.R, case.QN))
    return Params(f"general{substeps}", Q, R, QN, np.array([-3.0, -1.5, -2.5]), np.array([2.0, 2.75, 0.75]), 2 * np.pi / 60, substeps,
                  7000.0, 1e-5)


ORIGINAL = Params("original", case.Q, case.R, case.QN, np.full(3, -case.U_MAX), np.full(3, case.U_MAX), DT, 4, sc.RC_KM, 1e-6)
GENERAL = {s: _general(s) for s in (1, 3)}                  # by substeps; everything else is shared
PARAMS = {p.name: p for p in (ORIGINAL, GENERAL[1], GENERAL[3])}
for _p in PARAMS.values():
    for _a in _p[1:6]:
        _a.setflags(write=False)


def step_of(p):
    """scvx.rk4_step at the parameter set's substeps and rc, as the `step` of scvx.rollout / linearise / correction_qp_batch."""
    return functools.partial(sc.rk4_step, substeps=p.substeps, rc=p.rc)


def host_qp(p, xb, ub, x0, tr_u, tr_x):
    """scvx.correction_qp_batch under the parameter set p: box and linear term are its own; its A, B (central differences at the
    default eps) are replaced by scvx.linearise at p.fd_eps."""
    step = step_of(p)
    qp = sc.correction_qp_batch(xb, ub, x0, p.dt, p.Q, p.R, p.QN, p.u_lo, p.u_hi, tr_u, tr_x, step)
    if p.fd_eps == 1e-6:
        return qp
    xprev = np.concatenate([x0[:, None, :], xb[:, :-1, :]], axis=1)
    A, B = sc.linearise(xprev, ub, p.dt, step, p.fd_eps)
    return dataclasses.replace(qp, A=A, B=B)


# ---- the model in extended precision: the formulas of scvx.relative_motion_rhs, rk4_step, rollout, linearise, trajectory_cost in
# the same order, every operand np.longdouble (80-bit on x86: eps = 2^-63; tests/test_scvx_device_host.py asserts eps < 2^-60)
LD = np.longdouble


def ld_rhs(s, u, rc):
    rc = LD(rc)
    x, y, z, vx, vy, vz = (s[..., i] for i in range(6))
    rd3 = ((rc + x) ** 2 + y ** 2 + z ** 2) ** LD(1.5)
    k = rc ** 3 / rd3
    ax = LD(2) * vy + x + rc - k * (rc + x) + u[..., 0]
    ay = -LD(2) * vx + y - k * y + u[..., 1]
    az = -k * z + u[..., 2]
    return np.stack([vx, vy, vz, ax, ay, az], axis=-1)


def ld_rk4_step(s, u, dt, substeps, rc):
    s, u = np.asarray(s, LD), np.asarray(u, LD)
    h = LD(dt) / LD(substeps)
    for _ in range(substeps):
        k1 = ld_rhs(s, u, rc)
        k2 = ld_rhs(s + LD(0.5) * h * k1, u, rc)
        k3 = ld_rhs(s + LD(0.5) * h * k2, u, rc)
        k4 = ld_rhs(s + h * k3, u, rc)
        s = s + (h / LD(6)) * (k1 + LD(2) * k2 + LD(2) * k3 + k4)
    return s


def ld_rollout(x0, u, dt, substeps, rc):
    u = np.asarray(u, LD)
    s = np.asarray(x0, LD)
    xs = np.empty(u.shape[:-1] + (6,), LD)
    for k in range(u.shape[-2]):
        s = ld_rk4_step(s, u[..., k, :], dt, substeps, rc)
        xs[..., k, :] = s
    return xs


def ld_linearise(xprev, u, dt, substeps, rc, eps):
    xprev, u, eps = np.asarray(xprev, LD), np.asarray(u, LD), LD(eps)
    A = np.empty(xprev.shape[:-1] + (6, 6), LD)
    B = np.empty(xprev.shape[:-1] + (6, 3), LD)
    for j in range(6):
        d = np.zeros(6, LD); d[j] = eps
        A[..., :, j] = (ld_rk4_step(xprev + d, u, dt, substeps, rc) - ld_rk4_step(xprev - d, u, dt, substeps, rc)) / (LD(2) * eps)
    for j in range(3):
        d = np.zeros(3, LD); d[j] = eps
        B[..., :, j] = (ld_rk4_step(xprev, u + d, dt, substeps, rc) - ld_rk4_step(xprev, u - d, dt, substeps, rc)) / (LD(2) * eps)
    return A, B


def _ld_quad(v, M):
    return ((v @ np.asarray(M, LD)) * v).sum(axis=(-1, -2) if v.ndim > 1 else -1)


def ld_trajectory_cost(x, u, Q, R, QN):
    x, u = np.asarray(x, LD), np.asarray(u, LD)
    return LD(0.5) * _ld_quad(u, R) + LD(0.5) * _ld_quad(x[..., :-1, :], Q) + LD(0.5) * _ld_quad(x[..., -1:, :], QN)


def linear_term(xb, ub, Q, R, QN, dtype=np.float64):
    """q (B, N, 9) of scvx.correction_qp_batch: (R ub_k, Q xb_k), QN at the last stage."""
    xb, ub, Q, R, QN = (np.asarray(a, dtype) for a in (xb, ub, Q, R, QN))
    q = np.empty(ub.shape[:-1] + (9,), dtype)
    q[..., :3] = ub @ R.T
    q[:, :-1, 3:] = xb[:, :-1, :] @ Q.T
    q[:, -1, 3:] = xb[:, -1, :] @ QN.T
    return q


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
def decision_inputs(B=66, N=9, params="original"):
    """One advance call's inputs, six trajectories apart per branch (b % 6 -> BRANCHES; the lone trajectory of B = 1 takes branch 2),
    and what scvx.outer_update makes of them, under the parameter set PARAMS[params].
    The correction du, dx of the QP about (ub, xb) comes from the CPU oracle; the branches are steered by what z is made of it:
      0  z = 0: the model predicts no decrease                     -> stops
      1  z = the QP's solution: the model is accurate              -> accepted, radii doubled
      2  du halved but dx kept: the model promises too much        -> accepted, radii kept
      3  du reversed but dx kept                                   -> rejected, radii halved
      4  du ~ 1e-8 and a reference cost J above the true one       -> accepted (a decrease the step did not earn), stops: |du| <= tol
      5  inactive on entry, z arbitrary                            -> untouched
    J is an INPUT of the decision (the cost the loop carries), so 4 is a legitimate state of the interface.
    Under a GENERAL set every control of a branch-3 trajectory sits ON the box, on the side the QP moves it away from (found by a
    probe solve): the reversed step then leaves the box and the candidate's clip is active.  For it to be active on both sides of
    every axis within ONE trajectory (B = 6 has only one), those trajectories start from an x0 that makes the QP's push change sign
    along the horizon (below; clip_activity counts what came of it)."""
    p = PARAMS[params]
    step = step_of(p)
    rng = np.random.default_rng(DECISION_SEEDS.get((B, N, params), 11))
    x0 = case.X0[None] * (1.0 + 0.05 * rng.standard_normal((B, 6)))
    ub = rng.uniform(p.u_lo, p.u_hi, (B, N, 3))
    kind = np.arange(B) % 6 if B > 1 else np.array([2])
    if params != "original" and N >= 2:
        k3 = kind == 3
        # an x0 for the branch-3 trajectories under which the QP's push changes sign along the horizon (a push to one side only
        # clips on one side only).  The terminal cost dominates, so the push on u_k is about
        # -B_k' Phi' QN x_N ~ -dt ((N - k - 1/2) dt a + b), a | b the position | velocity rows of QN x_N: with b = -(N dt / 2) a it
        # changes sign half way.  That fixes v_N for the scattered p_N; x0 is x_N integrated backwards under ub
        tau = 0.5 * N * p.dt
        vN = -np.linalg.solve(p.QN[3:, 3:] + tau * p.QN[:3, 3:], (p.QN[3:, :3] + tau * p.QN[:3, :3]) @ x0[k3, :3].T).T
        s = np.concatenate([x0[k3, :3], vN], axis=1)
        for k in reversed(range(N)):
            s = step(s, ub[k3, k], -p.dt)
        x0[k3] = s
        xb = sc.rollout(x0, ub, p.dt, step)
        probe = case.oracle_qp_solver(**case.QP)(host_qp(p, xb, ub, x0, np.full(B, 0.1), np.full(B, 100.0)))[0].reshape(B, N, 9)
        ub[k3] = np.where(probe[k3][..., :3] > 0, p.u_lo, p.u_hi)
    xb = sc.rollout(x0, ub, p.dt, step)
    J = sc.trajectory_cost(xb, ub, p.Q, p.R, p.QN)
    tru = rng.uniform(0.05, 0.2, B)
    trx = rng.uniform(50.0, 200.0, B)
    active = kind != 5
    qp = host_qp(p, xb, ub, x0, np.where(active, tru, 0.0), np.where(active, trx, 0.0))
    zq = case.oracle_qp_solver(**case.QP)(qp)[0].reshape(B, N, 9)
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
    J_lin = sc.trajectory_cost(xb + dx, ub + du, p.Q, p.R, p.QN)
    u_new = np.clip(ub + du, p.u_lo, p.u_hi)
    x_new = sc.rollout(x0, u_new, p.dt, step)
    J_new = sc.trajectory_cost(x_new, u_new, p.Q, p.R, p.QN)
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


# ---- GENERAL: the scatter and its references
@functools.lru_cache(maxsize=None)
def scattered_general(B, N, substeps):
    """scattered(B, N) under GENERAL[substeps]: the controls fill the asymmetric box per axis, x is the host rollout."""
    p = GENERAL[substeps]
    rng = np.random.default_rng(11)
    x0 = case.X0[None] * (1.0 + 0.05 * rng.standard_normal((B, 6)))
    u = rng.uniform(p.u_lo, p.u_hi, (B, N, 3))
    x = sc.rollout(x0, u, p.dt, step_of(p))
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
def reference_general(B, N, substeps):
    """About scattered_general(B, N, substeps): the long-double rollout x, central differences A, B and linear term q ("ld"), what
    NumPy fp64 gives for the same ("np"), lo and hi of correction_qp_batch, and two WRONG linear terms the device must be far from:
    q_diag (Q, R, QN reduced to their diagonals) and q_qlast (Q at the last stage instead of QN)."""
    p = GENERAL[substeps]
    x0, u, x, tru, trx, active = scattered_general(B, N, substeps)
    xprev = np.concatenate([x0[:, None, :], x[:, :-1, :]], axis=1)
    qp = host_qp(p, x, u, x0, np.where(active, tru, 0.0), np.where(active, trx, 0.0))
    A, Bm = ld_linearise(xprev, u, p.dt, p.substeps, p.rc, p.fd_eps)
    ld = dict(x=ld_rollout(x0, u, p.dt, p.substeps, p.rc), A=A, B=Bm, q=linear_term(x, u, p.Q, p.R, p.QN, LD))
    out = dict(ld=ld, np=dict(x=x, A=qp.A, B=qp.B, q=qp.q.reshape(B, N, 9)), lo=qp.lo, hi=qp.hi,
               q_diag=linear_term(x, u, *(np.diag(np.diag(M)) for M in (p.Q, p.R, p.QN))), q_qlast=linear_term(x, u, p.Q, p.R, p.Q))
    for a in list(ld.values()) + list(out["np"].values()) + [out["lo"], out["hi"], out["q_diag"], out["q_qlast"]]:
        a.setflags(write=False)
    return out


def fp64_vs_ld(B, N, substeps):
    """max |NumPy fp64 - long double| per quantity on the inputs of scattered_general(B, N, substeps)."""
    r = reference_general(B, N, substeps)
    return {k: float(np.abs(r["np"][k] - r["ld"][k]).max()) for k in ("x", "A", "B", "q")}


# max |NumPy fp64 - long double| per quantity on scattered_general(B, N, substeps), by (substeps, B, N), as
# tests/test_scvx_device_host.py printed it (rounded up to two digits; that test keeps the table current).  The GPU tests allow
# GPU_MARGIN times as much: the device differs from NumPy by fma contraction and r2 sqrt(r2) for pow, which is of the order of
# NumPy's own rounding.  x and q are absolute, at states up to 166 km and |q| up to 8.4e3; A, B contain the 1 / (2 fd_eps) = 5e4
# amplification of the step's rounding (entries O(1)).
FP64_VS_LD = {
    (1, 1, 1): dict(x=6.3e-14, A=5.8e-09, B=4.8e-09, q=1.4e-12),
    (1, 63, 7): dict(x=4.3e-13, A=1.6e-08, B=7.6e-09, q=1.5e-12),
    (1, 65, 64): dict(x=4.7e-12, A=1.5e-08, B=9.2e-09, q=9.1e-13),
    (1, 130, 65): dict(x=4.0e-12, A=1.7e-08, B=1.1e-08, q=1.2e-12),
    (3, 1, 1): dict(x=2.5e-14, A=2.7e-09, B=1.9e-09, q=8.9e-13),
    (3, 63, 7): dict(x=2.4e-13, A=8.2e-09, B=6.2e-09, q=1.4e-12),
    (3, 65, 64): dict(x=2.6e-12, A=8.4e-09, B=7.6e-09, q=6.8e-13),
    (3, 130, 65): dict(x=3.3e-12, A=1.1e-08, B=9.1e-09, q=8.2e-13),
}
GPU_MARGIN = 10.0
ROLLOUT_BOUND = 5e-11                                       # the bound of the ORIGINAL rollout (tests/test_gpu_scvx_device.py)


# ---- the decision test across the advance kernel's shape edges (SCVX_ADV_CH = 4 stages per chunk, 64 trajectories per wave)
DECISION_SHAPES = [(1, 1), (6, 3), (64, 4), (65, 8), (200, 5), (66, 9)]
DECISION_PARAMS = ("original", "general1", "general3")
DECISION_SEEDS = {}                                         # (B, N, params) -> seed where 11 leaves a ratio too near a threshold


def decision_junk(B, N, cap):
    """What the candidates and the history hold before the advance call (the call must leave it where it has nothing to write)."""
    rng = np.random.default_rng(5)
    return {k: rng.standard_normal(shape) for k, shape in (("u_cand", (B, N, 3)), ("x_cand", (B, N, 6)), ("history", (cap, B, 9)))}


def clip_activity(state, ref, p):
    """For the trajectories of branch 3 (du reversed): per axis, how many components of ub + du lie strictly below u_lo and strictly
    above u_hi -- where np.clip changes the value -- and whether the candidate is then exactly the bound."""
    rows = ref["kind"] == 3
    raw = state["ub"][rows] + state["z"][rows][..., :3]
    below, above = raw < p.u_lo, raw > p.u_hi
    u_new = ref["u_new"][rows]
    exact = (u_new[below] == np.broadcast_to(p.u_lo, raw.shape)[below]).all() and (u_new[above] == np.broadcast_to(p.u_hi, raw.shape)[above]).all()
    return below.sum(axis=(0, 1)), above.sum(axis=(0, 1)), bool(exact)


def ratio_margin(records):
    """The distance of the nearest finite ratio from rho_reject and rho_expand."""
    ratios = np.array([r["ratio"] for r in records if np.isfinite(r["ratio"])])
    if ratios.size == 0:
        return np.inf
    return float(min(np.abs(ratios - RHO_REJECT).min(), np.abs(ratios - RHO_EXPAND).min()))


# ---- whole loops: a host model of scvx_batch's outer loop that is fed the QP solutions z from outside
class HostLoop:
    """The state of scvx_batch between two QP solves and its two halves of one outer iteration, in the host formulas: qp() is
    correction_qp_batch about the current reference, advance(z) the candidate, the costs, outer_update and the take."""

    def __init__(self, x0, N, p, tr_u, tr_x, tol, rho_reject=RHO_REJECT, rho_expand=RHO_EXPAND):
        self.p, self.step, self.x0, self.N = p, step_of(p), np.array(x0, np.float64), N
        Bn = self.x0.shape[0]
        self.tol, self.rho_reject, self.rho_expand = tol, rho_reject, rho_expand
        self.ub = np.zeros((Bn, N, 3))
        self.xb = sc.rollout(self.x0, self.ub, p.dt, self.step)
        self.J = sc.trajectory_cost(self.xb, self.ub, p.Q, p.R, p.QN)
        self.tr_u, self.tr_x = np.full(Bn, float(tr_u)), np.full(Bn, float(tr_x))
        self.active, self.converged = np.ones(Bn, bool), np.zeros(Bn, bool)
        self.accepted, self.outer = np.zeros(Bn, int), np.zeros(Bn, int)
        self.history = [[] for _ in range(Bn)]              # per trajectory: its records, in order
        self.stopped_at = np.full(Bn, -1)                   # the outer iteration (0-based) at which the trajectory went inactive

    def qp(self):
        return host_qp(self.p, self.xb, self.ub, self.x0, np.where(self.active, self.tr_u, 0.0), np.where(self.active, self.tr_x, 0.0))

    def advance(self, z, iteration):
        p = self.p
        d = np.asarray(z, np.float64).reshape(self.x0.shape[0], self.N, 9)
        du, dx = d[..., :3], d[..., 3:]
        J_lin = sc.trajectory_cost(self.xb + dx, self.ub + du, p.Q, p.R, p.QN)
        u_new = np.clip(self.ub + du, p.u_lo, p.u_hi)
        x_new = sc.rollout(self.x0, u_new, p.dt, self.step)
        J_new = sc.trajectory_cost(x_new, u_new, p.Q, p.R, p.QN)
        was = self.active.copy()
        take, records = sc.outer_update(self.J, J_lin, J_new, np.abs(du).max(axis=(1, 2)), self.tr_u, self.tr_x, self.active,
                                        self.converged, self.accepted, self.tol, self.rho_reject, self.rho_expand)
        self.ub[take], self.xb[take] = u_new[take], x_new[take]
        self.outer += was
        self.stopped_at[was & ~self.active] = iteration
        for b, rec in records.items():
            self.history[b].append(rec)
        return dict(take=take, records=records, u_new=u_new, x_new=x_new, was_active=was)


# B = 70 trajectories of N = 13 stages under GENERAL[3], with two departures that make the steps move and the model err: the box is
# 10 times as wide (its asymmetry stays) and a stage three times as long.  (With GENERAL's own dt and box the linear model is almost
# exact: with the oracle as QP solver every decision of every trajectory was accept + expand, ratio 1.000.)  Seed, tol and the
# number of scale levels were chosen on the CPU (oracle as QP solver, LOCKSTEP_QP) so that lockstep_preconditions holds at ten times
# its margins: no deciding ratio within 1.46e-2 of a threshold, no predicted decrease within a factor 23 of tol max(1, |J|); the run
# takes accept + expand 138, accept + keep 42, reject 170 and model-converged 40 times, 30 trajectories are active at the cap.
LOCKSTEP = dict(B=70, N=13, params="general3", seed=22, scale=(1.0, 8.0), levels=7, scatter=0.005, box=10.0, dt=2 * np.pi / 20,
                tr_u=16.0, tr_x=1600.0, tol=1.3e-7, max_outer=8)
# max |NumPy fp64 - long double| over that run: the candidates' rollouts x, and A, B, q of every outer iteration (states up to
# 1.7e3 km, ten times those of FP64_VS_LD), as tests/test_scvx_device_host.py printed it and keeps it current
LOCKSTEP_FP64_VS_LD = dict(x=4.5e-12, A=2.9e-08, B=2.8e-08, q=2.3e-11)
LOCKSTEP_QP = dict(rho=0.5, eps_abs=1e-6, eps_rel=1e-6, max_iter=1000, check_interval=25)


def lockstep_x0():
    """The scenario's X0 scaled per trajectory by one of LOCKSTEP["levels"] factors spread geometrically over LOCKSTEP["scale"]
    (shuffled over the batch) and scattered by LOCKSTEP["scatter"]."""
    c = LOCKSTEP
    rng = np.random.default_rng(c["seed"])
    f = np.resize(np.geomspace(*c["scale"], c["levels"]), c["B"])
    rng.shuffle(f)
    return case.X0[None] * f[:, None] * (1.0 + c["scatter"] * rng.standard_normal((c["B"], 6)))


def lockstep_params():
    """GENERAL[3] with its box widened by LOCKSTEP["box"] and stages of LOCKSTEP["dt"]."""
    c = LOCKSTEP
    p = PARAMS[c["params"]]
    return p._replace(name="lockstep", u_lo=c["box"] * p.u_lo, u_hi=c["box"] * p.u_hi, dt=c["dt"])


def lockstep_host():
    c = LOCKSTEP
    return HostLoop(lockstep_x0(), c["N"], lockstep_params(), c["tr_u"], c["tr_x"], c["tol"])


def kind_of(rec, tol, rho_expand=RHO_EXPAND):
    """What outer_update did with a record: model_converged | accepted_expanded | accepted | rejected."""
    if rec["predicted"] <= tol * max(1.0, abs(rec["cost"])):
        return "model_converged"
    if not rec["accepted"]:
        return "rejected"
    return "accepted_expanded" if rec["ratio"] >= rho_expand else "accepted"


def lockstep_preconditions(host, margin=1.0):
    """What a finished HostLoop run must have been through for the lockstep test to mean anything; AssertionError names the
    precondition (a failure here is one of the test's inputs, not of the kernels).  margin: the multiple of the knife-edge margins
    (1e-3 about the ratio thresholds, a factor 2 about the stop threshold) that is asked for."""
    pre = "precondition of the lockstep test failed (its inputs, not the kernels): "
    tol = host.tol
    kinds = [[kind_of(r, tol, host.rho_expand) for r in h] for h in host.history]
    seen = collections.Counter(k for ks in kinds for k in ks)
    for k in ("accepted_expanded", "accepted", "rejected", "model_converged"):
        assert seen[k] >= 1, pre + f"no trajectory took the branch {k}: {dict(seen)}"
    assert host.active.any(), pre + "no trajectory is still active at the cap"
    acc = [["accepted" in k for k in ks if k != "model_converged"] for ks in kinds]
    mixed = [b for b, a in enumerate(acc) if any((not a[i]) and any(a[i + 1:]) for i in range(len(a))) or
             any(a[i] and not a[i + 1] for i in range(len(a) - 1))]
    assert mixed, pre + "no trajectory has a reject followed by an accept, or a reject directly after an accept"
    stops = sorted(set(host.stopped_at[host.stopped_at >= 0].tolist()))
    assert len(stops) >= 2, pre + f"trajectories go inactive at fewer than two different iterations: {stops}"
    worst_ratio, worst_pred = np.inf, np.inf
    for h, ks in zip(host.history, kinds):
        for r, k in zip(h, ks):
            thr = tol * max(1.0, abs(r["cost"]))
            if r["predicted"] > 0:
                worst_pred = min(worst_pred, abs(np.log(r["predicted"] / thr)))
            if k != "model_converged":                      # the ratio decides only where the model still sees a gain
                worst_ratio = min(worst_ratio, abs(r["ratio"] - host.rho_reject), abs(r["ratio"] - host.rho_expand))
    assert worst_ratio > 1e-3 * margin, pre + f"a deciding ratio lies within {worst_ratio:.3e} of a threshold (asked: {1e-3 * margin:.0e})"
    assert worst_pred > np.log(2.0 * margin), pre + (f"a predicted decrease lies within a factor {np.exp(worst_pred):.3f} of tol max(1, |J|) "
                                                     f"(asked: {2.0 * margin:.0f})")
    return dict(branches=dict(seen), mixed=mixed, stops=stops, ratio_margin=float(worst_ratio), predicted_factor=float(np.exp(worst_pred)),
                still_active=int(host.active.sum()))
