"""Inputs and host references of the tests of the time-dependent models of the device SCvx outer step (tests/test_scvx_stage_host.py,
tests/test_gpu_scvx_stage.py), built on the CPU by the method of tests/_scvx_models_case.py: a scatter of
trajectories per parameter set, an extended-precision (np.longdouble) restatement of the model -- right-hand side, RK4 with its node
indexing, rollout, central differences, linear term -- fed the SAME fp64 node table as the reference, NumPy fp64's own distance from
it as the yardstick (recorded below, kept current by the CPU tests), one advance call's inputs on which scvx.outer_update takes every
branch, and a host model of the whole loop.

Parameter sets: `elliptic` (a chief with e = 0.3, 4 sub-intervals, the scenario of tests/_scvx_case.py), `circular` (the same with
e = 0: the model then is scvx.relative_motion_rhs) and `random1`, `random3`: tables whose rows are INDEPENDENT per node at 1 and 3
sub-intervals, so that a node index that is wrong by one stage, one sub-interval or one RK4 point moves x far beyond the bound
(ld_rollout's `shift` states such wrong indexings; tests/test_scvx_stage_host.py checks that each is told from the right one)."""
import collections
import dataclasses
import functools

import numpy as np

from admm_library_amd import scvx as sc

import _scvx_case as case
import _scvx_device_case as dc

LD = np.longdouble
SHAPES = [(1, 1), (63, 7), (65, 64), (130, 65)]      # lone lane; partial wave; the wave boundary in B and N; several workgroups
TOL, RHO_REJECT, RHO_EXPAND = dc.TOL, dc.RHO_REJECT, dc.RHO_EXPAND
BRANCHES = dc.BRANCHES
GPU_MARGIN = dc.GPU_MARGIN

A_KM, ECC, M0 = 7000.0, 0.3, 0.4                     # the chief of the eccentric sets: semi-major axis, eccentricity, mean anomaly at t0
MU = A_KM ** 3                                       # time in units of 1 / mean motion

Params = collections.namedtuple("Params", "name Q R QN u_lo u_hi dt substeps mu fd_eps table")


def random_nodes(mu, seed, N, dt, substeps):
    """A table whose rows are independent per node: rc in [6000, 8000], w in [0.5, 1.5], wd in [-0.5, 0.5], g = mu / rc^2."""
    rng = np.random.default_rng(seed)
    n = 2 * substeps * N + 1
    rc = rng.uniform(6000.0, 8000.0, n)
    return np.stack([rc, rng.uniform(0.5, 1.5, n), rng.uniform(-0.5, 0.5, n), mu / rc ** 2], axis=-1)


def _random(substeps):
    g = dc._general(substeps)                        # dense SPD Q, R, QN; the per-axis asymmetric box; dt = 2 pi / 60; fd_eps 1e-5
    return Params(f"random{substeps}", g.Q, g.R, g.QN, g.u_lo, g.u_hi, g.dt, substeps, MU, g.fd_eps, ("random", 31 + substeps))


def _kepler(name, e):
    o = dc.ORIGINAL                                  # the scenario of tests/_scvx_case.py: diagonal weights, one scalar box, dt = 2 pi / 80
    return Params(name, o.Q, o.R, o.QN, o.u_lo, o.u_hi, o.dt, 4, MU, 1e-6, ("elliptic", A_KM, e, M0))


ELLIPTIC = _kepler("elliptic", ECC)
CIRCULAR = _kepler("circular", 0.0)
PARAMS = {p.name: p for p in (ELLIPTIC, _random(1), _random(3), CIRCULAR)}
GPU_PARAMS = ("elliptic", "random1", "random3")      # the sets of the accuracy test; `circular` is the set of the two-doors test
for _p in PARAMS.values():
    for _a in _p[1:6]:
        _a.setflags(write=False)


def model_of(p):
    if p.table[0] == "elliptic":
        return sc.relative_elliptic(*p.table[1:])
    return sc.relative_tabulated(functools.partial(random_nodes, p.mu, p.table[1]), p.mu)


def table_of(p, N):
    """The fp64 node table of the parameter set on a horizon of N stages (read-only)."""
    t = model_of(p).nodes(N, p.dt, p.substeps)
    t.setflags(write=False)
    return t


def host_rollout(p, x0, u):
    return sc.rollout(x0, u, p.dt, model=model_of(p), substeps=p.substeps)


def host_qp(p, xb, ub, x0, tr_u, tr_x):
    """scvx.correction_qp_batch under the parameter set p with A, B by scvx.linearise at p.fd_eps."""
    m = model_of(p)
    qp = sc.correction_qp_batch(xb, ub, x0, p.dt, p.Q, p.R, p.QN, p.u_lo, p.u_hi, tr_u, tr_x, model=m, substeps=p.substeps)
    if p.fd_eps == 1e-6:
        return qp
    xprev = np.concatenate([x0[:, None, :], xb[:, :-1, :]], axis=1)
    A, B = sc.linearise(xprev, ub, p.dt, eps=p.fd_eps, model=m, substeps=p.substeps)
    return dataclasses.replace(qp, A=A, B=B)


# ---- the model in extended precision: the formulas of scvx.relative_tabulated_rhs and StageModel.step in the same order, every
# operand np.longdouble; the node rows are the fp64 table's
def ld_rhs(s, u, e, mu):
    mu = LD(mu)
    x, y, z, vx, vy, vz = (s[..., i] for i in range(6))
    rc, w, wd, g = (e[..., i] for i in range(4))
    xr = rc + x
    r2 = xr ** 2 + y ** 2 + z ** 2
    k = mu / (r2 * np.sqrt(r2))
    ax = LD(2) * w * vy + wd * y + w * w * x + g - k * xr + u[..., 0]
    ay = -LD(2) * w * vx - wd * x + w * w * y - k * y + u[..., 1]
    az = -k * z + u[..., 2]
    return np.stack([vx, vy, vz, ax, ay, az], axis=-1)


SHIFTS = ("stage", "sub", "point")                   # wrong node indexings: off by one stage, one sub-interval, one RK4 point


def stage_rows(p, N, shift=None):
    """(N, 2 substeps + 1) global node indices, stage k holding 2 substeps k .. 2 substeps (k + 1); `shift`: one of SHIFTS, the
    indices moved on by 2 substeps, 2 or 1 (wrapped at the table's end)."""
    idx = 2 * p.substeps * np.arange(N)[:, None] + np.arange(2 * p.substeps + 1)[None, :]
    if shift is not None:
        idx = (idx + {"stage": 2 * p.substeps, "sub": 2, "point": 1}[shift]) % (2 * p.substeps * N + 1)
    return idx


def ld_step(s, u, p, e):
    """One stage; e (..., 2 substeps + 1, 4): the stage's node rows."""
    s, u, e = np.asarray(s, LD), np.asarray(u, LD), np.asarray(e, LD)
    h = LD(p.dt) / LD(p.substeps)
    for i in range(p.substeps):
        e0, e1, e2 = e[..., 2 * i, :], e[..., 2 * i + 1, :], e[..., 2 * i + 2, :]
        k1 = ld_rhs(s, u, e0, p.mu)
        k2 = ld_rhs(s + LD(0.5) * h * k1, u, e1, p.mu)
        k3 = ld_rhs(s + LD(0.5) * h * k2, u, e1, p.mu)
        k4 = ld_rhs(s + h * k3, u, e2, p.mu)
        s = s + (h / LD(6)) * (k1 + LD(2) * k2 + LD(2) * k3 + k4)
    return s


def ld_rollout(x0, u, p, table, shift=None):
    u = np.asarray(u, LD)
    s = np.asarray(x0, LD)
    N = u.shape[-2]
    e = np.asarray(table, LD)[stage_rows(p, N, shift)]
    xs = np.empty(u.shape[:-1] + (6,), LD)
    for k in range(N):
        s = ld_step(s, u[..., k, :], p, e[k])
        xs[..., k, :] = s
    return xs


def ld_linearise(xprev, u, p, table):
    xprev, u, eps = np.asarray(xprev, LD), np.asarray(u, LD), LD(p.fd_eps)
    e = np.asarray(table, LD)[stage_rows(p, xprev.shape[-2])]
    A = np.empty(xprev.shape[:-1] + (6, 6), LD)
    B = np.empty(xprev.shape[:-1] + (6, 3), LD)
    for j in range(6):
        d = np.zeros(6, LD); d[j] = eps
        A[..., :, j] = (ld_step(xprev + d, u, p, e) - ld_step(xprev - d, u, p, e)) / (LD(2) * eps)
    for j in range(3):
        d = np.zeros(3, LD); d[j] = eps
        B[..., :, j] = (ld_step(xprev, u + d, p, e) - ld_step(xprev, u - d, p, e)) / (LD(2) * eps)
    return A, B


# ---- the scatter and its references
@functools.lru_cache(maxsize=None)
def scattered(B, N, name):
    """x0 (B, 6) = the scenario's X0 (1 + 0.05 randn), u (B, N, 3) filling the box per axis, the host rollout x, per-trajectory
    radii and an active mask with every fifth trajectory off (the scatter of _scvx_device_case.scattered_general)."""
    p = PARAMS[name]
    rng = np.random.default_rng(11)
    x0 = case.X0[None] * (1.0 + 0.05 * rng.standard_normal((B, 6)))
    u = rng.uniform(p.u_lo, p.u_hi, (B, N, 3))
    x = host_rollout(p, x0, u)
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
def reference(B, N, name):
    """About scattered(B, N, name): the long-double rollout x, central differences A, B and linear term q ("ld"), what NumPy fp64
    gives for the same ("np"), lo and hi of correction_qp_batch, and the long-double rollouts under the wrong node indexings of
    SHIFTS ("x_<shift>")."""
    p = PARAMS[name]
    x0, u, x, tru, trx, active = scattered(B, N, name)
    table = table_of(p, N)
    xprev = np.concatenate([x0[:, None, :], x[:, :-1, :]], axis=1)
    qp = host_qp(p, x, u, x0, np.where(active, tru, 0.0), np.where(active, trx, 0.0))
    A, Bm = ld_linearise(xprev, u, p, table)
    ld = dict(x=ld_rollout(x0, u, p, table), A=A, B=Bm, q=dc.linear_term(x, u, p.Q, p.R, p.QN, LD))
    out = dict(ld=ld, np=dict(x=x, A=qp.A, B=qp.B, q=qp.q.reshape(B, N, 9)), lo=qp.lo, hi=qp.hi,
               **{"x_" + s: ld_rollout(x0, u, p, table, s) for s in SHIFTS})
    for a in list(ld.values()) + list(out["np"].values()) + [out["lo"], out["hi"]] + [out["x_" + s] for s in SHIFTS]:
        a.setflags(write=False)
    return out


def fp64_vs_ld(B, N, name):
    """max |NumPy fp64 - long double| per quantity on the inputs of scattered(B, N, name)."""
    r = reference(B, N, name)
    return {k: float(np.abs(r["np"][k] - r["ld"][k]).max()) for k in ("x", "A", "B", "q")}


# max |NumPy fp64 - long double| per quantity on scattered(B, N, name), as tests/test_scvx_stage_host.py printed it (rounded up to
# two digits; that test keeps the table current).  The GPU tests allow GPU_MARGIN times as much: the device differs from NumPy by
# fma contraction and in the order of a few additions, which is of the order of NumPy's own rounding; both cancel the 7000-sized
# terms g and k xr alike.  A, B contain the 1 / (2 fd_eps) amplification of the step's rounding.
FP64_VS_LD = {
    ('elliptic', 1, 1): dict(x=8.3e-15, A=7.2e-08, B=2e-08, q=5.3e-13),
    ('elliptic', 63, 7): dict(x=3.4e-13, A=1.3e-07, B=9.5e-08, q=9.9e-13),
    ('elliptic', 65, 64): dict(x=5.6e-12, A=2e-07, B=1.8e-07, q=4.2e-12),
    ('elliptic', 130, 65): dict(x=3.8e-12, A=2.2e-07, B=2e-07, q=4.2e-12),
    ('random1', 1, 1): dict(x=9e-14, A=7.7e-09, B=4.6e-09, q=1e-12),
    ('random1', 63, 7): dict(x=5.3e-13, A=1.7e-08, B=1.1e-08, q=1.7e-12),
    ('random1', 65, 64): dict(x=1.6e-11, A=2.5e-08, B=1.6e-08, q=7.1e-12),
    ('random1', 130, 65): dict(x=1.7e-11, A=2.4e-08, B=1.5e-08, q=1.3e-11),
    ('random3', 1, 1): dict(x=5.9e-14, A=3.3e-09, B=3.4e-09, q=2.7e-13),
    ('random3', 63, 7): dict(x=2.8e-13, A=1.1e-08, B=9.1e-09, q=1.6e-12),
    ('random3', 65, 64): dict(x=4.9e-12, A=1.4e-08, B=1.2e-08, q=6e-12),
    ('random3', 130, 65): dict(x=5.1e-12, A=1.6e-08, B=1.4e-08, q=8.5e-12),
    ('circular', 1, 1): dict(x=4.5e-14, A=4.5e-08, B=1.9e-08, q=2e-13),
    ('circular', 63, 7): dict(x=1.8e-13, A=7.1e-08, B=7.5e-08, q=5.3e-13),
    ('circular', 65, 64): dict(x=1.8e-12, A=6.9e-08, B=6.3e-08, q=2.5e-13),
    ('circular', 130, 65): dict(x=2.3e-12, A=7.4e-08, B=7.1e-08, q=2.7e-13),
}


# ---- one advance call's inputs on which scvx.outer_update takes every branch (the construction of _scvx_device_case.decision_inputs)
DECISION_SHAPES = dc.DECISION_SHAPES
DECISION_PARAMS = ("elliptic",)
DECISION_SEEDS = {}                                  # (B, N, params) -> seed where 11 leaves a ratio too near a threshold
DECISION_QP = case.QP


@functools.lru_cache(maxsize=None)
def decision_inputs(B, N, params="elliptic"):
    """Six trajectories apart per branch (b % 6 -> BRANCHES; the lone trajectory of B = 1 takes branch 2): the correction of the QP
    about (ub, xb) comes from the CPU oracle, and z is made of it as _scvx_device_case.decision_inputs makes it (0: z = 0; 1: the
    solution; 2: du halved, dx kept; 3: du reversed, dx kept; 4: du ~ 1e-8 and J above the true cost; 5: inactive, z arbitrary)."""
    p = PARAMS[params]
    rng = np.random.default_rng(DECISION_SEEDS.get((B, N, params), 11))
    x0 = case.X0[None] * (1.0 + 0.05 * rng.standard_normal((B, 6)))
    ub = rng.uniform(p.u_lo, p.u_hi, (B, N, 3))
    kind = np.arange(B) % 6 if B > 1 else np.array([2])
    xb = host_rollout(p, x0, ub)
    J = sc.trajectory_cost(xb, ub, p.Q, p.R, p.QN)
    tru = rng.uniform(0.05, 0.2, B)
    trx = rng.uniform(50.0, 200.0, B)
    active = kind != 5
    qp = host_qp(p, xb, ub, x0, np.where(active, tru, 0.0), np.where(active, trx, 0.0))
    zq = case.oracle_qp_solver(**DECISION_QP)(qp)[0].reshape(B, N, 9)
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
    du, dx = z[..., :3], z[..., 3:]
    J_lin = sc.trajectory_cost(xb + dx, ub + du, p.Q, p.R, p.QN)
    u_new = np.clip(ub + du, p.u_lo, p.u_hi)
    x_new = host_rollout(p, x0, u_new)
    J_new = sc.trajectory_cost(x_new, u_new, p.Q, p.R, p.QN)
    ref = dict(J=J.copy(), tr_u=tru.copy(), tr_x=trx.copy(), active=active.copy(), converged=converged.copy(), accepted=accepted.copy())
    take, records = sc.outer_update(ref["J"], J_lin, J_new, np.abs(du).max(axis=(1, 2)), ref["tr_u"], ref["tr_x"], ref["active"],
                                    ref["converged"], ref["accepted"], TOL, RHO_REJECT, RHO_EXPAND)
    ref.update(take=take, records=records, u_new=u_new, x_new=x_new, outer=outer + active, kind=kind,
               x_new_ld=ld_rollout(x0, u_new, p, table_of(p, N)))
    return state, ref


def candidate_fp64_vs_ld(params):
    """max |NumPy fp64 - long double| of the candidates' rollouts over the decision shapes."""
    return max(float(np.abs(ref["x_new"] - ref["x_new_ld"]).max()) for ref in (decision_inputs(B, N, params)[1] for B, N in DECISION_SHAPES))


# ... as tests/test_scvx_stage_host.py printed it; the bound of x_cand in the decision tests is GPU_MARGIN times it
CANDIDATE_FP64_VS_LD = dict(elliptic=3.8e-13)


# ---- whole loops: _scvx_device_case.HostLoop over a parameter set of this module
class HostLoop(dc.HostLoop):
    def __init__(self, x0, N, p, tr_u, tr_x, tol, rho_reject=RHO_REJECT, rho_expand=RHO_EXPAND):
        self.p, self.x0, self.N = p, np.array(x0, np.float64), N
        Bn = self.x0.shape[0]
        self.tol, self.rho_reject, self.rho_expand = tol, rho_reject, rho_expand
        self.ub = np.zeros((Bn, N, 3))
        self.xb = host_rollout(p, self.x0, self.ub)
        self.J = sc.trajectory_cost(self.xb, self.ub, p.Q, p.R, p.QN)
        self.tr_u, self.tr_x = np.full(Bn, float(tr_u)), np.full(Bn, float(tr_x))
        self.active, self.converged = np.ones(Bn, bool), np.zeros(Bn, bool)
        self.accepted, self.outer = np.zeros(Bn, int), np.zeros(Bn, int)
        self.history = [[] for _ in range(Bn)]
        self.stopped_at = np.full(Bn, -1)

    def qp(self):
        return host_qp(self.p, self.xb, self.ub, self.x0, np.where(self.active, self.tr_u, 0.0), np.where(self.active, self.tr_x, 0.0))

    def advance(self, z, iteration):
        """dc.HostLoop.advance with the candidate rolled out by the time-dependent model (a `step` sees no stage index)."""
        p = self.p
        d = np.asarray(z, np.float64).reshape(self.x0.shape[0], self.N, 9)
        du, dx = d[..., :3], d[..., 3:]
        J_lin = sc.trajectory_cost(self.xb + dx, self.ub + du, p.Q, p.R, p.QN)
        u_new = np.clip(self.ub + du, p.u_lo, p.u_hi)
        x_new = host_rollout(p, self.x0, u_new)
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


# B = 70 trajectories of N = 13 stages about the eccentric chief: random3's dense weights, its box 10 times as wide (the asymmetry
# kept), 3 sub-intervals, fd_eps 1e-5, and stages of 0.3 (3.9 time units: 0.6 of a chief orbit, through apogee) from 0.3 times the
# scenario's X0, so that the steps move and the linear model errs.  Scale, stage length, radii and tol were chosen on the CPU (oracle
# as QP solver, LOCKSTEP_QP) so that every branch occurs; the candidates kept are those of lockstep_select().
LOCKSTEP = dict(B=70, N=13, seed=22, scale=(0.02, 8.0), levels=7, scatter=0.005, x0_scale=0.3, box=10.0, dt=0.3, tr_u=8.0, tr_x=200.0,
                tol=1e-6, max_outer=8, candidates=240)
LOCKSTEP_KEEP = (
                 6, 7, 17, 20, 23, 25, 31, 35, 36, 38, 42, 43, 44, 47, 57, 60, 63, 64, 66, 67, 68, 74, 79, 84, 88, 89, 93, 95,
                 96, 99, 103, 105, 109, 110, 111, 112, 113, 116, 120, 127, 131, 132, 133, 135, 138, 141, 151, 158, 163, 168,
                 170, 171, 184, 188, 190, 196, 201, 203, 204, 206, 207, 209, 210, 214, 215, 217, 223, 226, 230, 231)
LOCKSTEP_FP64_VS_LD = dict(x=6.4e-12, A=4.4e-08, B=4.7e-08, q=5.3e-12)
LOCKSTEP_QP = dict(rho=0.5, eps_abs=1e-6, eps_rel=1e-6, max_iter=1000, check_interval=25)
LOCKSTEP_CLEAR = dict(ratio=1.5e-2, predicted=30.0)         # the criterion of LOCKSTEP_KEEP


def lockstep_params():
    c = LOCKSTEP
    p = PARAMS["random3"]
    return p._replace(name="lockstep", u_lo=c["box"] * p.u_lo, u_hi=c["box"] * p.u_hi, dt=c["dt"], table=ELLIPTIC.table)


def lockstep_candidates():
    """LOCKSTEP["candidates"] starts: the scenario's X0 scaled per trajectory by one of LOCKSTEP["levels"] factors spread
    geometrically over LOCKSTEP["scale"] (shuffled) and scattered by LOCKSTEP["scatter"]."""
    c = LOCKSTEP
    rng = np.random.default_rng(c["seed"])
    f = np.resize(np.geomspace(*c["scale"], c["levels"]), c["candidates"])
    rng.shuffle(f)
    return c["x0_scale"] * case.X0[None] * f[:, None] * (1.0 + c["scatter"] * rng.standard_normal((c["candidates"], 6)))


def lockstep_select():
    """LOCKSTEP_KEEP from its criterion (tests/test_scvx_stage_host.py asserts that the recorded list is this one; to regenerate
    after a change of the inputs, paste what this returns): the CPU rehearsal of all candidates with the oracle as QP solver, then
    the first LOCKSTEP["B"] of those with no deciding ratio within LOCKSTEP_CLEAR["ratio"] of rho_reject or rho_expand and no
    predicted decrease within a factor LOCKSTEP_CLEAR["predicted"] of tol max(1, |J|)."""
    c = LOCKSTEP
    host = HostLoop(lockstep_candidates(), c["N"], lockstep_params(), c["tr_u"], c["tr_x"], c["tol"])
    solve = case.oracle_qp_solver(**LOCKSTEP_QP)
    for it in range(c["max_outer"]):
        host.advance(solve(host.qp())[0], it)
    keep = []
    for b, h in enumerate(host.history):
        ratio, pred = np.inf, np.inf
        for r in h:
            if r["predicted"] > 0:
                pred = min(pred, abs(np.log(r["predicted"] / (host.tol * max(1.0, abs(r["cost"]))))))
            if dc.kind_of(r, host.tol) != "model_converged":
                ratio = min(ratio, abs(r["ratio"] - host.rho_reject), abs(r["ratio"] - host.rho_expand))
        if ratio >= LOCKSTEP_CLEAR["ratio"] and pred >= np.log(LOCKSTEP_CLEAR["predicted"]):
            keep.append(b)
    return tuple(keep[:c["B"]])


def lockstep_x0():
    """The candidates of LOCKSTEP_KEEP (each trajectory has its own QP: they do not interact)."""
    assert len(LOCKSTEP_KEEP) == LOCKSTEP["B"]
    return lockstep_candidates()[list(LOCKSTEP_KEEP)]


def lockstep_host():
    c = LOCKSTEP
    return HostLoop(lockstep_x0(), c["N"], lockstep_params(), c["tr_u"], c["tr_x"], c["tol"])


# ---- the eccentric rendezvous of the loop tests: 0.3 times the insertion error of tests/_scvx_case.py (45 km along-track, 9 km
# cross-track) about the chief of ELLIPTIC, N = 40 stages of 0.05 (a third of a chief orbit from M0 = 0.4), a box of +-60 and radii
# under which the loop takes five accepted steps and stops on the model's verdict (CPU rehearsal with the oracle as QP solver).  The
# design of the circular model, flown on this plant, misses by 59 km; this model's by 0.12 km
EL_N, EL_DT, EL_U_MAX = 40, 0.05, 60.0
EL_X0 = 0.3 * case.X0
EL_Q = np.diag([1.0, 1.0, 1.0, 0.1, 0.1, 0.1]) * EL_DT
EL_R = np.eye(3) * EL_DT * 0.05
EL_QN = np.diag([50.0, 50.0, 50.0, 20.0, 20.0, 20.0])
EL_SCVX = dict(tr_u=5.0, tr_x=20.0, max_outer=20, tol=1e-6)


def elliptic_x0(B, seed=11):
    rng = np.random.default_rng(seed)
    return EL_X0[None] * (1.0 + 0.1 * rng.standard_normal((B, 6)))


def elliptic_args(x0):
    return (x0, EL_N, EL_DT, EL_Q, EL_R, EL_QN, -EL_U_MAX, EL_U_MAX)


# ---- the scenario of the fourth-order check (tests/test_scvx_stage_host.py): an uncontrolled deputy about the chief of ELLIPTIC
TWO_BODY = dict(a=A_KM, e=ECC, M0=M0, dt=0.05, N=40, s0=(3.0, -5.0, 2.0, 0.01, -0.02, 0.015))
