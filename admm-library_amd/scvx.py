"""Successive-convexification outer loop over the batched ADMM solver.

The caller that generates the hot path's QPs in practice: a NONLINEAR trajectory problem is solved
by repeatedly linearising the dynamics about the current trajectory, solving the resulting
box-constrained optimal-control QP (libadmm_hip.so) for a correction, and re-propagating the
nonlinear dynamics.  Host-side NumPy; the QP solve is the only device work.  No reference
counterpart exists (README.md:1-2 only); the scheme is the standard trust-region successive
linearisation (Mao, Szmuk, Acikmese 2016) without virtual control: the reference trajectory is
always re-propagated through the nonlinear dynamics, so the linearised model has no defect term.

Model shipped here: exact nonlinear relative motion about a circular reference orbit in the
rotating (LVLH) frame, in the units of problems.cw_matrices (time 1/mean-motion, length 1 km) --
its linearisation at the origin is the Clohessy-Wiltshire system of the benchmark workload:

    x'' =  2 y' + x + rc - rc^3 (rc + x) / rd^3 + u_x
    y'' = -2 x' + y      - rc^3 y        / rd^3 + u_y          rd = |(rc + x, y, z)|,  rc = a / 1 km
    z'' =                - rc^3 z        / rd^3 + u_z

The QP of one outer iteration, in the correction (du, dx) about the reference (ub, xb):

    minimise   1/2 sum_k [(ub_k + du_k)' R (ub_k + du_k) + (xb_{k+1} + dx_{k+1})' Q_{k+1} (xb_{k+1} + dx_{k+1})]
    subject to dx_{k+1} = A_k dx_k + B_k du_k,  dx_0 = 0,
               max(u_lo - ub_k, -tr_u) <= du_k <= min(u_hi - ub_k, tr_u),   |dx| <= tr_x

i.e. the hot path's QP with time-varying (A_k, B_k), per-stage bounds and the linear term
q = (R ub_k, Q_{k+1} xb_{k+1}).  scvx() drives ONE trajectory (batch-shared dynamics, batch = 1);
scvx_batch() drives MANY at once -- a Monte-Carlo set of initial conditions, say: every trajectory
has its own linearisation, box and linear term, i.e. one QP batch with per-instance dynamics
(admm_problem.time_varying = 2, stage_bounds = 2) per outer iteration.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import Callable, List, Optional, Tuple

import numpy as np

from .problems import A_REF, Problem

RC_KM = A_REF / 1000.0        # reference orbit radius in the length unit of cw_matrices (1 km)


def relative_motion_rhs(s: np.ndarray, u: np.ndarray, rc: float = RC_KM) -> np.ndarray:
    """Time derivative of s = (x, y, z, vx, vy, vz) (..., 6) under thrust acceleration u (..., 3)."""
    x, y, z, vx, vy, vz = (s[..., i] for i in range(6))
    rd3 = ((rc + x) ** 2 + y ** 2 + z ** 2) ** 1.5
    k = rc ** 3 / rd3
    ax = 2.0 * vy + x + rc - k * (rc + x) + u[..., 0]
    ay = -2.0 * vx + y - k * y + u[..., 1]
    az = -k * z + u[..., 2]
    return np.stack([vx, vy, vz, ax, ay, az], axis=-1)


def rk4_step(s: np.ndarray, u: np.ndarray, dt: float, substeps: int = 4, rc: float = RC_KM) -> np.ndarray:
    """Zero-order-hold propagation of one stage (classical RK4, `substeps` sub-intervals)."""
    h = dt / substeps
    for _ in range(substeps):
        k1 = relative_motion_rhs(s, u, rc)
        k2 = relative_motion_rhs(s + 0.5 * h * k1, u, rc)
        k3 = relative_motion_rhs(s + 0.5 * h * k2, u, rc)
        k4 = relative_motion_rhs(s + h * k3, u, rc)
        s = s + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    return s


MU_EARTH_MOON = 0.012150585    # mass ratio m2 / (m1 + m2) of the Earth-Moon system


def crtbp_rhs(s, u, mu: float, x_ref: float = 0.0):
    """Circular restricted three-body problem in the nondimensional rotating frame (primaries at X = -mu and X = 1 - mu): time
    derivative of s = (x, y, z, vx, vy, vz) (..., 6), the position measured from the point (x_ref, 0, 0), under the thrust
    acceleration u (..., 3).  The normative statement of the device model ScvxCrtbp; NumPy arrays or torch
    tensors.  Nothing is special near a primary: inf / NaN propagate."""
    if isinstance(s, np.ndarray):
        sqrt, stack = np.sqrt, functools.partial(np.stack, axis=-1)
    else:
        import torch
        sqrt, stack = torch.sqrt, functools.partial(torch.stack, dim=-1)
    x, y, z, vx, vy, vz = (s[..., i] for i in range(6))
    ux, uy, uz = (u[..., i] for i in range(3))
    X = x_ref + x;  d1 = X + mu;  d2 = X - 1 + mu;  yz = y**2 + z**2
    r1 = d1**2 + yz;  r2 = d2**2 + yz
    k1 = (1 - mu) / (r1 * sqrt(r1));  k2 = mu / (r2 * sqrt(r2))
    ax = 2*vy + X - k1*d1 - k2*d2 + ux
    ay = -2*vx + y - (k1 + k2)*y + uy
    az = -(k1 + k2)*z + uz
    return stack((vx, vy, vz, ax, ay, az))


def _relative_motion_rhs_torch(s, uu, rc):
    """relative_motion_rhs on torch tensors: the same formulas in the same order."""
    import torch
    x, y, z, vx, vy, vz = (s[..., i] for i in range(6))
    rd3 = ((rc + x) ** 2 + y ** 2 + z ** 2) ** 1.5
    k = rc ** 3 / rd3
    ax = 2.0 * vy + x + rc - k * (rc + x) + uu[..., 0]
    ay = -2.0 * vx + y - k * y + uu[..., 1]
    az = -k * z + uu[..., 2]
    return torch.stack([vx, vy, vz, ax, ay, az], dim=-1)


def _rk4(rhs, s, u, dt, substeps):
    h = dt / substeps
    for _ in range(substeps):
        k1 = rhs(s, u)
        k2 = rhs(s + 0.5 * h * k1, u)
        k3 = rhs(s + 0.5 * h * k2, u)
        k4 = rhs(s + h * k3, u)
        s = s + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    return s


@dataclasses.dataclass(frozen=True)
class Model:
    """A nonlinear model the loop can be run for, on the host and -- by `kind`, one of the models compiled into the library
    (admm_scvx_dynamics) -- in the device outer step: n = 6, m = 3, time-invariant."""
    name: str                     # admm_scvx_model_name(kind)
    kind: int                     # ADMM_SCVX_RELATIVE_CIRCULAR | ADMM_SCVX_CRTBP
    par: Tuple[float, ...]        # admm_scvx_dynamics.par, the entries in use
    rhs: Callable                 # rhs(s, u) on NumPy arrays
    rhs_torch: Callable           # ... on torch tensors: the same formulas in the same order

    def step(self, s, u, dt: float, substeps: int = 4):
        """Zero-order-hold propagation of one stage (classical RK4 over rhs, `substeps` sub-intervals): the `step` of rollout,
        linearise, scvx and scvx_batch."""
        return _rk4(self.rhs, s, u, dt, substeps)


def relative_circular(rc: float = RC_KM) -> Model:
    """The shipped model: relative_motion_rhs about a circular orbit of radius rc."""
    return Model("relative_circular", 0, (float(rc),), functools.partial(relative_motion_rhs, rc=rc),
                 functools.partial(_relative_motion_rhs_torch, rc=rc))


def crtbp(mu: float, x_ref: float = 0.0) -> Model:
    """The circular restricted three-body problem of mass ratio mu, the state relative to (x_ref, 0, 0) (crtbp_rhs).  With x_ref a
    collinear libration point (crtbp_collinear_point) the origin is an equilibrium and the loop's quadratic cost means "acquire
    or keep the point"."""
    if not (np.isfinite(mu) and 0.0 < mu < 1.0) or not np.isfinite(x_ref):
        raise ValueError("crtbp: mu must lie in (0, 1) and x_ref be finite")
    f = functools.partial(crtbp_rhs, mu=float(mu), x_ref=float(x_ref))
    return Model("crtbp", 1, (float(mu), float(x_ref)), f, f)


def crtbp_collinear_point(mu: float, which: int) -> float:
    """X of the collinear libration point L1, L2 or L3 (which = 1, 2, 3) of the CR3BP of mass ratio mu: the root of the x-axis
    equilibrium equation X - (1 - mu) (X + mu) / |X + mu|^3 - mu (X - 1 + mu) / |X - 1 + mu|^3 = 0 in the point's interval, by
    Newton's method in extended precision from Hill's estimate, then the fp64 neighbour at which crtbp_rhs at rest is smallest."""
    if which not in (1, 2, 3):
        raise ValueError("which must be 1, 2 or 3")
    LD = np.longdouble
    m = LD(mu)
    rh = (m / LD(3)) ** (LD(1) / LD(3))
    X = {1: LD(1) - m - rh, 2: LD(1) - m + rh, 3: -LD(1) - LD(5) * m / LD(12)}[which]

    def f(X):
        d1, d2 = X + m, X - LD(1) + m
        return X - (LD(1) - m) * d1 / abs(d1) ** 3 - m * d2 / abs(d2) ** 3

    def df(X):
        d1, d2 = X + m, X - LD(1) + m
        return LD(1) + LD(2) * (LD(1) - m) / abs(d1) ** 3 + LD(2) * m / abs(d2) ** 3
    for _ in range(60):
        step = f(X) / df(X)
        X = X - step
        if abs(step) <= LD(4) * np.finfo(LD).eps * abs(X):
            break
    x = float(X)
    rest, zero = np.zeros(6), np.zeros(3)
    cands = [x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)]
    return min(cands, key=lambda c: float(np.abs(crtbp_rhs(rest, zero, mu, c)).max()))


def relative_tabulated_rhs(s, u, e, mu: float):
    """Exact nonlinear relative motion in the rotating frame of a chief that moves in a plane (x radial, y along-track, z
    cross-track): time derivative of s = (x, y, z, vx, vy, vz) (..., 6) under the thrust acceleration u (..., 3) at a node whose
    row e (..., 4) = (rc, w, wd, g) holds the chief's radius, angular rate, angular acceleration and radial gravity mu / rc^2.
    The normative statement of the device model ScvxRelativeTabulated; NumPy arrays or torch tensors.  With
    rc = a, w = 1, wd = 0, g = a, mu = a^3 it is relative_motion_rhs."""
    if isinstance(s, np.ndarray):
        sqrt, stack = np.sqrt, functools.partial(np.stack, axis=-1)
    else:
        import torch
        sqrt, stack = torch.sqrt, functools.partial(torch.stack, dim=-1)
    x, y, z, vx, vy, vz = (s[..., i] for i in range(6))
    rc, w, wd, g = (e[..., i] for i in range(4))
    xr = rc + x
    r2 = xr**2 + y**2 + z**2
    k = mu / (r2 * sqrt(r2))
    ax = 2*w*vy + wd*y + w*w*x + g - k*xr + u[..., 0]
    ay = -2*w*vx - wd*x + w*w*y - k*y + u[..., 1]
    az = -k*z + u[..., 2]
    return stack((vx, vy, vz, ax, ay, az))


def _rk4_nodes(rhs, s, u, dt, e, substeps):
    """_rk4 for a right-hand side that reads node rows: e (..., 2 substeps + 1, 4) holds the stage's rows -- sub-interval i uses
    row 2 i (k1), 2 i + 1 (k2, k3) and 2 i + 2 (k4)."""
    h = dt / substeps
    for i in range(substeps):
        e0, e1, e2 = e[..., 2 * i, :], e[..., 2 * i + 1, :], e[..., 2 * i + 2, :]
        k1 = rhs(s, u, e0)
        k2 = rhs(s + 0.5 * h * k1, u, e1)
        k3 = rhs(s + 0.5 * h * k2, u, e1)
        k4 = rhs(s + h * k3, u, e2)
        s = s + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    return s


@dataclasses.dataclass(frozen=True)
class StageModel:
    """A TIME-DEPENDENT model the loop can be run for (n = 6, m = 3): its right-hand side reads ADMM_SCVX_NODE_PAR = 4 values per
    RK4 node from a table shared by all trajectories (admm_scvx_stage_dynamics).  The nodes of a grid
    (N, dt, substeps) lie at the times t0 + g h / 2, h = dt / substeps, g = 0 .. 2 substeps N; all time dependence is in the table."""
    name: str                     # admm_scvx_stage_model_name(kind)
    kind: int                     # ADMM_SCVX_STAGE_RELATIVE_TABULATED
    par: Tuple[float, ...]        # admm_scvx_stage_dynamics.par, the entries in use
    rhs: Callable                 # rhs(s, u, e) on NumPy arrays, e the node's row (..., 4)
    rhs_torch: Callable           # ... on torch tensors: the same formulas in the same order
    nodes_fn: Callable            # nodes_fn(N, dt, substeps) -> the table (2 substeps N + 1, 4)

    def nodes(self, N: int, dt: float, substeps: int = 4) -> np.ndarray:
        """The table of the grid (N, dt, substeps): (2 substeps N + 1, 4) fp64, C order."""
        t = np.ascontiguousarray(self.nodes_fn(int(N), float(dt), int(substeps)), np.float64)
        if t.shape != (2 * int(substeps) * int(N) + 1, 4):
            raise ValueError(f"{self.name}: the node table has shape {t.shape}, expected {(2 * int(substeps) * int(N) + 1, 4)}")
        return t

    def stage_nodes(self, N: int, dt: float, substeps: int = 4) -> np.ndarray:
        """The table by stage: (N, 2 substeps + 1, 4), stage k holding the rows 2 substeps k .. 2 substeps (k + 1)."""
        idx = 2 * substeps * np.arange(N)[:, None] + np.arange(2 * substeps + 1)[None, :]
        return self.nodes(N, dt, substeps)[idx]

    def step(self, s, u, dt: float, e, substeps: int = 4):
        """Zero-order-hold propagation of one stage whose node rows are e (..., 2 substeps + 1, 4)."""
        return _rk4_nodes(self.rhs, s, u, dt, e, substeps)


def kepler_E(M, e: float):
    """The eccentric anomaly E of Kepler's equation E - e sin E = M, by Newton's method in np.longdouble (M: array)."""
    LD = np.longdouble
    M, e = np.asarray(M, LD), LD(e)
    E = M + e * np.sin(M)
    for _ in range(60):
        d = (E - e * np.sin(E) - M) / (LD(1) - e * np.cos(E))
        E = E - d
        if np.all(np.abs(d) <= LD(4) * np.finfo(LD).eps * np.maximum(LD(1), np.abs(E))):
            break
    return E


def elliptic_nodes(a: float, e: float, M0: float, N: int, dt: float, substeps: int = 4) -> np.ndarray:
    """The node table (2 substeps N + 1, 4) of relative_tabulated_rhs for a chief on a Kepler orbit of semi-major axis a and
    eccentricity e that is at mean anomaly M0 at the first node.  The time unit is 1 / mean motion (mu = a^3, as the circular model
    has it), so node g lies at mean anomaly M0 + g h / 2, h = dt / substeps.  Evaluated in np.longdouble and rounded to fp64 once:
    rc = a (1 - e cos E), w = a^2 sqrt(1 - e^2) / rc^2, wd = -2 w rdot / rc with rdot = a e sin E / (1 - e cos E), g = a^3 / rc^2."""
    if not (np.isfinite(a) and a > 0.0) or not (np.isfinite(e) and 0.0 <= e < 1.0):
        raise ValueError("elliptic_nodes: a must be positive and e lie in [0, 1)")
    LD = np.longdouble
    a_, e_ = LD(a), LD(e)
    hh = LD(dt) / LD(substeps) / LD(2)
    E = kepler_E(LD(M0) + np.arange(2 * int(substeps) * int(N) + 1).astype(LD) * hh, e)
    den = LD(1) - e_ * np.cos(E)
    rc = a_ * den
    w = a_ * a_ * np.sqrt(LD(1) - e_ * e_) / (rc * rc)
    rdot = a_ * e_ * np.sin(E) / den
    wd = -LD(2) * w * rdot / rc
    g = a_ * a_ * a_ / (rc * rc)
    return np.ascontiguousarray(np.stack([rc, w, wd, g], axis=-1).astype(np.float64))


def relative_tabulated(nodes_fn: Callable, mu: float) -> StageModel:
    """relative_tabulated_rhs about a chief whose motion the caller tabulates: nodes_fn(N, dt, substeps) -> (2 substeps N + 1, 4)
    rows (rc, w, wd, mu / rc^2)."""
    if not (np.isfinite(mu) and mu > 0.0):
        raise ValueError("relative_tabulated: mu must be finite and positive")
    f = functools.partial(relative_tabulated_rhs, mu=float(mu))
    return StageModel("relative_tabulated", 0, (float(mu),), f, f, nodes_fn)


def relative_elliptic(a: float = RC_KM, e: float = 0.0, M0: float = 0.0) -> StageModel:
    """Relative motion about a chief on a Kepler orbit (elliptic_nodes): semi-major axis a, eccentricity e, mean anomaly M0 at the
    start of the horizon; time in units of 1 / mean motion."""
    if not (np.isfinite(a) and a > 0.0) or not (np.isfinite(e) and 0.0 <= e < 1.0):
        raise ValueError("relative_elliptic: a must be positive and e lie in [0, 1)")
    return relative_tabulated(functools.partial(elliptic_nodes, float(a), float(e), float(M0)), float(a) ** 3)


def _resolve(model, step):
    """The `step` of a call that may name a model instead: model.step (a StageModel: `step` itself -- the callee is handed the model
    as well, _timed); both: ValueError."""
    if model is None:
        return step
    if step is not rk4_step:
        raise ValueError("model and step cannot both be given" if not isinstance(model, StageModel) else
                         "a time-dependent model and step cannot both be given")
    return step if isinstance(model, StageModel) else model.step


def _timed(model):
    """model if it is time-dependent, else None."""
    return model if isinstance(model, StageModel) else None


def _model_step(model, step, substeps):
    """rollout's and linearise's `step` under their keywords model and substeps (a Model: its step, at `substeps` if given)."""
    if model is None:
        if substeps is not None:
            raise ValueError("substeps goes with model (a foreign step carries its own)")
        return step
    step = _resolve(model, step)
    return step if substeps is None or isinstance(model, StageModel) else functools.partial(step, substeps=substeps)


def rollout(x0: np.ndarray, u: np.ndarray, dt: float, step=rk4_step, model=None, substeps: Optional[int] = None) -> np.ndarray:
    """States x_1..x_N (N, n) of the nonlinear dynamics from x0 under controls u (N, m); with a leading
    batch axis on both ((B, n), (B, N, m)) the B trajectories are propagated together -> (B, N, n).
    model: a Model or StageModel in place of `step` (not both), at `substeps` sub-intervals (default 4); stage k of a StageModel
    reads the rows 2 substeps k .. 2 substeps (k + 1) of model.nodes(N, dt, substeps)."""
    step = _model_step(model, step, substeps)
    u = np.asarray(u, np.float64)
    s = np.asarray(x0, np.float64)
    N = u.shape[-2]
    xs = np.empty(u.shape[:-1] + (s.shape[-1],))
    if _timed(model):
        sub = 4 if substeps is None else int(substeps)
        e = model.stage_nodes(N, dt, sub)
        for k in range(N):
            s = model.step(s, u[..., k, :], dt, e[k], sub)
            xs[..., k, :] = s
        return xs
    for k in range(N):
        s = step(s, u[..., k, :], dt)
        xs[..., k, :] = s
    return xs


def linearise(xprev: np.ndarray, u: np.ndarray, dt: float, step=rk4_step, eps: float = 1e-6, model=None,
              substeps: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """A_k = dF/dx, B_k = dF/du of the stage map F at (xprev_k, u_k), k = 0..N-1, by central
    differences (vectorised over stages and perturbation directions).
    model, substeps: as in rollout; with a StageModel the stage axis (the last but one of xprev) is the whole horizon 0..N-1."""
    step = _model_step(model, step, substeps)
    if _timed(model):
        sub = 4 if substeps is None else int(substeps)
        e = model.stage_nodes(xprev.shape[-2], dt, sub)

        def step(s, uu, dt):      # noqa: F811
            return model.step(s, uu, dt, e, sub)
    lead, n = xprev.shape[:-1], xprev.shape[-1]          # (N,) or (B, N)
    m = u.shape[-1]
    A = np.empty(lead + (n, n))
    B = np.empty(lead + (n, m))
    for j in range(n):
        d = np.zeros(n); d[j] = eps
        A[..., :, j] = (step(xprev + d, u, dt) - step(xprev - d, u, dt)) / (2.0 * eps)
    for j in range(m):
        d = np.zeros(m); d[j] = eps
        B[..., :, j] = (step(xprev, u + d, dt) - step(xprev, u - d, dt)) / (2.0 * eps)
    return A, B


def linearise_device(xprev: np.ndarray, u: np.ndarray, dt: float, device: str = "cuda:0", eps: float = 1e-6,
                     substeps: int = 4, rc: float = RC_KM, keep_on_device: bool = False, model=None):
    """linearise() of the shipped model (rk4_step of relative_motion_rhs) with the n + m central differences evaluated as ONE
    batch of torch tensors on `device`: the same formulas in the same order, fp64.  The NumPy version makes 2 (n + m) x 16
    passes over (B, N, 6) arrays -- 10 s per outer iteration of a 4096-trajectory batch, most of the wall time of
    examples/scvx_batch_rendezvous.py; this is host plumbing, not the solver.
    keep_on_device: return A, B as the torch tensors on `device` (for a DeviceProblem) instead of NumPy copies.
    model: the right-hand side is model.rhs_torch instead of the shipped one (rc is then not used); a StageModel: its node rows are
    uploaded once and broadcast along the stage axis (the last but one of xprev: the whole horizon)."""
    import torch
    xp = torch.as_tensor(np.ascontiguousarray(xprev), dtype=torch.float64, device=device)
    up = torch.as_tensor(np.ascontiguousarray(u), dtype=torch.float64, device=device)
    n, m = xp.shape[-1], up.shape[-1]

    rhs = functools.partial(_relative_motion_rhs_torch, rc=rc) if model is None else model.rhs_torch

    def step(s, uu):
        return _rk4(rhs, s, uu, dt, substeps)

    if _timed(model):
        e = torch.as_tensor(model.stage_nodes(xp.shape[-2], dt, substeps), device=device)

        def step(s, uu):      # noqa: F811
            return _rk4_nodes(rhs, s, uu, dt, e, substeps)

    ex = eps * torch.eye(n, dtype=torch.float64, device=device).reshape((n,) + (1,) * (xp.dim() - 1) + (n,))
    eu = eps * torch.eye(m, dtype=torch.float64, device=device).reshape((m,) + (1,) * (up.dim() - 1) + (m,))
    A = (step(xp[None] + ex, up[None]) - step(xp[None] - ex, up[None])) / (2.0 * eps)        # (n, ..., n): [j, ..., i] = dF_i / dx_j
    B = (step(xp[None].expand((m,) + xp.shape), up[None] + eu) - step(xp[None].expand((m,) + xp.shape), up[None] - eu)) / (2.0 * eps)
    A, B = torch.movedim(A, 0, -1).contiguous(), torch.movedim(B, 0, -1).contiguous()
    if keep_on_device:
        return A, B
    return A.cpu().numpy(), B.cpu().numpy()


@dataclasses.dataclass
class ScvxCertificate:
    """Costates and the first-order optimality measure of the NONLINEAR problem at a trajectory (adjoint()).  NumPy
    arrays from adjoint(), torch tensors from DeviceOuterStep.certify(); with a leading batch axis where the trajectory had one."""
    nu: object                    # (N, 6): nu[k] = nu_{k+1}, the costate of stage k's dynamics (sign and indexing of DESIGN.md §2.9)
    primer: object                # (N, 3): B_k' nu_{k+1}
    grad: object                  # (N, 3): dJ/du_k at fixed x0 = R u_k - primer_k
    dJdx0: object                 # (6,): dJ/dx_0 at fixed u = -A_0' nu_1
    stat: object                  # the largest violation of first-order optimality over the components of u in their box
    n_bound: object               # the number of components of u on a bound


@dataclasses.dataclass
class ScvxResult:
    u: np.ndarray                 # (N, m) controls
    x: np.ndarray                 # (N, n) states x_1..x_N of the NONLINEAR dynamics under u
    cost: float                   # nonlinear cost of (x, u)
    outer_iterations: int
    accepted: int
    converged: bool
    history: List[dict]           # per outer iteration: cost, predicted / actual decrease, ratio, trust radius, |du|, ADMM iterations
    certificate: Optional[ScvxCertificate] = None      # with certify=True: adjoint() at (x, u)


def trajectory_cost(x: np.ndarray, u: np.ndarray, Q, R, QN):
    """Nonlinear cost of one trajectory (float), or of B trajectories with a leading batch axis ((B,) array)."""
    c = 0.5 * np.einsum("...ki,ij,...kj->...", u, R, u)
    c = c + 0.5 * np.einsum("...ki,ij,...kj->...", x[..., :-1, :], Q, x[..., :-1, :])
    c = c + 0.5 * np.einsum("...i,ij,...j->...", x[..., -1, :], QN, x[..., -1, :])
    return float(c) if np.ndim(c) == 0 else c


def stationarity(grad: np.ndarray, u: np.ndarray, u_lo, u_hi) -> Tuple[np.ndarray, np.ndarray]:
    """(stat, n_bound) of ScvxCertificate from the reduced gradient grad (..., N, 3) at the controls u in the box [u_lo, u_hi]
    (per axis), comparisons exact: a component violates first-order optimality by 0 if u_lo == u_hi, by max(-g, 0) on its lower
    bound, max(g, 0) on its upper bound and |g| elsewhere; stat is the maximum over (k, j) -- NaN if any entry of grad is a NaN."""
    grad, u = np.asarray(grad, np.float64), np.asarray(u, np.float64)
    lo = np.broadcast_to(np.asarray(u_lo, np.float64), (u.shape[-1],))
    hi = np.broadcast_to(np.asarray(u_hi, np.float64), (u.shape[-1],))
    at_lo, at_hi = u == lo, u == hi
    v = np.where(at_lo, np.maximum(-grad, 0.0), np.where(at_hi, np.maximum(grad, 0.0), np.abs(grad)))
    v = np.where(lo == hi, 0.0, v)
    stat = np.where(np.isnan(grad).any(axis=(-1, -2)), np.nan, np.nan_to_num(v, nan=0.0).max(axis=(-1, -2)))
    return stat, (at_lo | at_hi).sum(axis=(-1, -2)).astype(np.int32)


def adjoint(x0: np.ndarray, u: np.ndarray, x: np.ndarray, dt: float, Q, R, QN, u_lo, u_hi, step=rk4_step, model=None,
            eps: float = 1e-6, A: Optional[np.ndarray] = None, B: Optional[np.ndarray] = None) -> ScvxCertificate:
    """The discrete adjoint of trajectory_cost(rollout(x0, u), u) at the trajectory (x0, u, x = x_1 .. x_N), with or without a
    leading batch axis: costates, primer vector, reduced gradient dJ/du at fixed x0, dJ/dx0 at fixed u, and the first-order
    optimality measure of u in its box (stationarity) -- the host reference of admm_scvx_adjoint_device.

        nu_N = -QN x_N,    nu_{k+1} = A_{k+1}' nu_{k+2} - Q x_{k+1}  (k = N-2 .. 0),    primer_k = B_k' nu_{k+1},
        grad_k = R u_k - primer_k,    dJdx0 = -A_0' nu_1                                (Q, R, QN symmetric)

    A (..., N, 6, 6), B (..., N, 6, 3): the stage Jacobians at (x_k, u_k); by default linearise(...) of step / model at `eps`
    (model, step: as in rollout)."""
    u, x = np.asarray(u, np.float64), np.asarray(x, np.float64)
    x0 = np.asarray(x0, np.float64)
    Q, R, QN = (np.asarray(a, np.float64) for a in (Q, R, QN))
    single = u.ndim == 2
    if single:
        u, x, x0 = u[None], x[None], x0[None]
        A, B = (None if a is None else np.asarray(a)[None] for a in (A, B))
    if (A is None) != (B is None):
        raise ValueError("adjoint: A and B go together")
    if A is None:
        xprev = np.concatenate([x0[:, None, :], x[:, :-1, :]], axis=1)
        A, B = linearise(xprev, u, dt, step, eps, model=model)
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    Bn, N, m = u.shape
    n = x.shape[-1]
    qu = u @ R.T
    qx = x @ Q.T
    qx[:, -1] = x[:, -1] @ QN.T
    nu = np.empty((Bn, N, n))
    nu[:, -1] = -qx[:, -1]
    for k in range(N - 2, -1, -1):
        nu[:, k] = np.einsum("bji,bj->bi", A[:, k + 1], nu[:, k + 1]) - qx[:, k]
    primer = np.einsum("bkij,bki->bkj", B, nu)
    grad = qu - primer
    dJdx0 = -np.einsum("bji,bj->bi", A[:, 0], nu[:, 0])
    stat, n_bound = stationarity(grad, u, u_lo, u_hi)
    if single:
        return ScvxCertificate(nu[0], primer[0], grad[0], dJdx0[0], float(stat[0]), int(n_bound[0]))
    return ScvxCertificate(nu, primer, grad, dJdx0, stat, n_bound)


def correction_qp(xb: np.ndarray, ub: np.ndarray, x0: np.ndarray, dt: float, Q, R, QN, u_lo, u_hi,
                  tr_u: float, tr_x: float, step=rk4_step, model=None, substeps: Optional[int] = None) -> Problem:
    """The QP of one outer iteration (module docstring) as a hot-path Problem (batch = 1).
    model, substeps: as in linearise (scvx passes a StageModel on; a Model arrives as its step)."""
    N, n = xb.shape
    m = ub.shape[1]
    xprev = np.vstack([x0[None], xb[:-1]])
    A, B = linearise(xprev, ub, dt, step, model=model, substeps=substeps)
    q = np.empty((N, m + n))
    q[:, :m] = ub @ R.T
    q[:-1, m:] = xb[:-1] @ Q.T
    q[-1, m:] = QN @ xb[-1]
    lo = np.empty((N, m + n))
    hi = np.empty((N, m + n))
    lo[:, :m] = np.maximum(u_lo - ub, -tr_u)
    hi[:, :m] = np.minimum(u_hi - ub, tr_u)
    lo[:, m:] = -tr_x
    hi[:, m:] = tr_x
    return Problem(N=N, A=A, B=B, Q=np.asarray(Q, np.float64), R=np.asarray(R, np.float64),
                   QN=np.asarray(QN, np.float64), x0=np.zeros((1, n)), lo=lo, hi=hi, q=q.reshape(1, -1),
                   name=f"scvx_correction_N{N}")


def gpu_qp_solver(qp_data_on_device: bool = False, z_on_device: bool = False, **options
                  ) -> Callable[[Problem], Tuple[np.ndarray, int]]:
    """QP solver for scvx(): the HIP solver (raises without a device: no CPU fallback).  One handle
    serves every outer iteration: admm_update_problem refactors in place (same N, n, m, batch), each
    solve starts cold (z = y = 0), like a fresh handle.  A DeviceProblem (correction_qp_batch(..., qp_data_on_device=True))
    goes in through the device-memory entry points; qp_data_on_device: z comes back through admm_get_device as well.
    z_on_device (DeviceProblems only; scvx_batch(outer_on_device=True)): z is returned as the CUDA tensor admm_get_device wrote,
    and the cold start is set from a zero tensor on the device (admm_set_state_device) -- nothing of size batch x L crosses PCIe."""
    from .solver import Options, Solver
    state = {"solver": None, "shape": None, "zero": None}

    def solve(p: Problem):
        shape = (p.N, p.n, p.m, p.batch, p.q is not None, p.unorm is not None)
        if state["solver"] is None or state["shape"] != shape:
            if state["solver"] is not None:
                state["solver"].close()
            state["solver"], state["shape"] = Solver(p, Options(**options)), shape
        else:
            state["solver"].update_problem(p)
        s = state["solver"]
        if z_on_device:
            import torch
            if state["zero"] is None or tuple(state["zero"].shape) != (p.batch, p.L):
                state["zero"] = torch.zeros((p.batch, p.L), dtype=torch.float64, device=p.device)
            s.set_state(z=state["zero"], y=state["zero"])
            info = s.solve()
            return s.get_device(w=False, y=False)[1], int(info.iters_run)
        zero = np.zeros((p.batch, p.L))
        info = s.solve(z0=zero, y0=zero)
        if qp_data_on_device:
            _, z, _ = s.get_device(w=False, y=False)
            z = z.cpu().numpy()
        else:
            _, z, _ = s.get(w=False)
        return z, int(info.iters_run)      # z: the feasible (projected) iterate
    return solve


def scvx(x0: np.ndarray, N: int, dt: float, Q, R, QN, u_lo, u_hi,
         qp_solver: Optional[Callable[[Problem], Tuple[np.ndarray, int]]] = None,
         u_init: Optional[np.ndarray] = None, tr_u: float = 0.1, tr_x: float = 20.0,
         max_outer: int = 20, tol: float = 1e-6, rho_reject: float = 0.1, rho_expand: float = 0.7,
         step=rk4_step, qp_options: Optional[dict] = None, model=None, certify: bool = False) -> ScvxResult:
    """Trust-region successive convexification of

        minimise 1/2 sum_k [u_k' R u_k + x_{k+1}' Q_{k+1} x_{k+1}]   s.t.  x_{k+1} = F(x_k, u_k),  u_lo <= u_k <= u_hi.

    qp_solver(problem) -> (z of shape (1, L), ADMM iterations); default = the HIP solver.
    A step is accepted when actual / predicted cost decrease >= rho_reject (trust radii halve
    otherwise, double above rho_expand); stops when the accepted correction is below `tol`.
    model: a Model (relative_circular(), crtbp(...)) whose step replaces `step`; not both.  Or a StageModel (relative_elliptic(...),
    relative_tabulated(...)): a time-dependent model, whose stages read the node table of the grid (N, dt, 4 sub-intervals).
    certify: the result carries adjoint() at the returned trajectory (ScvxResult.certificate); nothing else changes."""
    step = _resolve(model, step)
    tm = _timed(model)
    x0 = np.asarray(x0, np.float64)
    Q, R, QN = (np.asarray(a, np.float64) for a in (Q, R, QN))
    n, m = Q.shape[0], R.shape[0]
    u_lo = np.broadcast_to(np.asarray(u_lo, np.float64), (m,))
    u_hi = np.broadcast_to(np.asarray(u_hi, np.float64), (m,))
    if qp_solver is None:
        qp_solver = gpu_qp_solver(**(qp_options or dict(rho=0.5, eps_abs=1e-8, eps_rel=1e-8, max_iter=20000,
                                                        check_interval=25)))
    ub = np.zeros((N, m)) if u_init is None else np.clip(np.asarray(u_init, np.float64), u_lo, u_hi)
    xb = rollout(x0, ub, dt, step, model=tm)
    J = trajectory_cost(xb, ub, Q, R, QN)
    hist: List[dict] = []
    accepted, converged = 0, False
    for it in range(1, max_outer + 1):
        p = correction_qp(xb, ub, x0, dt, Q, R, QN, u_lo, u_hi, tr_u, tr_x, step, model=tm)
        z, admm_iters = qp_solver(p)
        d = np.asarray(z, np.float64).reshape(N, m + n)
        du, dx = d[:, :m], d[:, m:]
        # cost the QP's model predicts for (xb + dx, ub + du)
        J_lin = trajectory_cost(xb + dx, ub + du, Q, R, QN)
        u_new = np.clip(ub + du, u_lo, u_hi)
        x_new = rollout(x0, u_new, dt, step, model=tm)
        J_new = trajectory_cost(x_new, u_new, Q, R, QN)
        predicted, actual = J - J_lin, J - J_new
        ratio = actual / predicted if predicted > 0 else -np.inf
        step_norm = float(np.abs(du).max())
        rec = dict(iteration=it, cost=J, cost_candidate=J_new, predicted=predicted, actual=actual, ratio=ratio,
                   tr_u=tr_u, tr_x=tr_x, du_max=step_norm, admm_iterations=admm_iters, accepted=False)
        if predicted <= tol * max(1.0, abs(J)):          # the model sees nothing left to gain
            hist.append(rec)
            converged = True
            break
        if ratio >= rho_reject:
            ub, xb, J = u_new, x_new, J_new
            accepted += 1
            rec["accepted"] = True
            if ratio >= rho_expand:
                tr_u, tr_x = 2.0 * tr_u, 2.0 * tr_x
        else:
            tr_u, tr_x = 0.5 * tr_u, 0.5 * tr_x
        hist.append(rec)
        if rec["accepted"] and step_norm <= tol:
            converged = True
            break
    cert = adjoint(x0, ub, xb, dt, Q, R, QN, u_lo, u_hi, step, model=tm) if certify else None
    return ScvxResult(u=ub, x=xb, cost=J, outer_iterations=len(hist), accepted=accepted, converged=converged,
                      history=hist, certificate=cert)


def correction_qp_batch(xb: np.ndarray, ub: np.ndarray, x0: np.ndarray, dt: float, Q, R, QN, u_lo, u_hi,
                        tr_u: np.ndarray, tr_x: np.ndarray, step=rk4_step, device: Optional[str] = None,
                        qp_data_on_device: bool = False, model=None, substeps: Optional[int] = None):
    """The correction QPs of B trajectories as ONE batch with per-instance dynamics, box and linear term
    (xb (B, N, n), ub (B, N, m), x0 (B, n), trust radii (B,)).
    qp_data_on_device (with device): a DeviceProblem -- A, B stay where linearise_device made them, the rest is built here
    exactly as for the Problem and copied to the device.
    model (scvx_batch passes it with step = model.step): the device linearisation evaluates model.rhs_torch.  A StageModel: the
    host linearisation reads its node table too, at `substeps` sub-intervals (default 4; with a StageModel only)."""
    tm = _timed(model)
    if tm is not None and step is not rk4_step:
        raise ValueError("a time-dependent model and step cannot both be given")
    if substeps is not None and tm is None:
        raise ValueError("substeps goes with a time-dependent model (a step carries its own)")
    Bn, N, n = xb.shape
    m = ub.shape[-1]
    xprev = np.concatenate([x0[:, None, :], xb[:, :-1, :]], axis=1)
    if qp_data_on_device and (device is None or (step is not rk4_step and model is None)):
        raise ValueError("qp_data_on_device needs the device linearisation (device = 'cuda:k', the shipped rk4_step)")
    if device is not None and model is not None:
        A, B = linearise_device(xprev, ub, dt, device, keep_on_device=qp_data_on_device, model=model,
                                **({} if substeps is None else dict(substeps=substeps)))
    elif device is not None and step is rk4_step:
        A, B = linearise_device(xprev, ub, dt, device, keep_on_device=qp_data_on_device)
    else:
        A, B = linearise(xprev, ub, dt, step, model=tm, substeps=substeps)
    q = np.empty((Bn, N, m + n))
    q[..., :m] = ub @ R.T
    q[:, :-1, m:] = xb[:, :-1, :] @ Q.T
    q[:, -1, m:] = xb[:, -1, :] @ QN.T
    lo = np.empty((Bn, N, m + n))
    hi = np.empty((Bn, N, m + n))
    lo[..., :m] = np.maximum(u_lo - ub, -tr_u[:, None, None])
    hi[..., :m] = np.minimum(u_hi - ub, tr_u[:, None, None])
    lo[..., m:] = -tr_x[:, None, None]
    hi[..., m:] = tr_x[:, None, None]
    p = Problem(N=N, A=A, B=B, Q=np.asarray(Q, np.float64), R=np.asarray(R, np.float64),
                QN=np.asarray(QN, np.float64), x0=np.zeros((Bn, n)), lo=lo, hi=hi, q=q.reshape(Bn, -1),
                name=f"scvx_correction_batch{Bn}_N{N}")
    if not qp_data_on_device:
        return p
    import torch
    from .problems import DeviceProblem

    def t(a):
        return torch.as_tensor(np.ascontiguousarray(a, np.float64), device=device)
    return DeviceProblem(N=N, A=A, B=B, Q=t(p.Q), R=t(p.R), QN=t(p.QN), x0=t(p.x0), lo=t(lo), hi=t(hi), q=t(p.q), name=p.name)


def outer_update(J: np.ndarray, J_lin: np.ndarray, J_new: np.ndarray, du_max: np.ndarray, tru: np.ndarray, trx: np.ndarray,
                 active: np.ndarray, converged: np.ndarray, accepted: np.ndarray, tol: float, rho_reject: float, rho_expand: float):
    """The decision of one outer iteration of scvx_batch for every ACTIVE trajectory, from the reference cost J, the cost J_lin the
    QP's model predicts for its solution, the cost J_new of the re-propagated candidate and du_max = |du|_inf (all (B,)): stop if
    the model sees nothing left to gain; otherwise accept when actual / predicted >= rho_reject (radii doubled above rho_expand),
    else halve the radii; stop after an accepted step below tol.  J, tru, trx, active, converged, accepted are UPDATED IN PLACE.
    Returns (take, records): take (B,) bool -- the candidate replaces the reference --, records {b: history record of b} for the
    trajectories that were active (the caller adds `iteration` and `admm_iterations`).  The host reference of the device kernel
    scvx_advance_kernel."""
    take = np.zeros(J.shape[0], bool)
    records = {}
    predicted, actual = J - J_lin, J - J_new
    for b in np.flatnonzero(active):
        ratio = actual[b] / predicted[b] if predicted[b] > 0 else -np.inf
        step_norm = float(du_max[b])
        rec = dict(cost=float(J[b]), cost_candidate=float(J_new[b]), predicted=float(predicted[b]),
                   actual=float(actual[b]), ratio=float(ratio), tr_u=float(tru[b]), tr_x=float(trx[b]), du_max=step_norm,
                   accepted=False)
        records[int(b)] = rec
        if predicted[b] <= tol * max(1.0, abs(J[b])):
            converged[b], active[b] = True, False
            continue
        if ratio >= rho_reject:
            take[b] = True
            J[b] = J_new[b]
            accepted[b] += 1
            rec["accepted"] = True
            if ratio >= rho_expand:
                tru[b], trx[b] = 2.0 * tru[b], 2.0 * trx[b]
        else:
            tru[b], trx[b] = 0.5 * tru[b], 0.5 * trx[b]
        if rec["accepted"] and step_norm <= tol:
            converged[b], active[b] = True, False
    return take, records


def scvx_batch(x0: np.ndarray, N: int, dt: float, Q, R, QN, u_lo, u_hi,
               qp_solver: Optional[Callable[[Problem], Tuple[np.ndarray, int]]] = None,
               tr_u: float = 0.1, tr_x: float = 20.0, max_outer: int = 20, tol: float = 1e-6,
               rho_reject: float = 0.1, rho_expand: float = 0.7, step=rk4_step,
               qp_options: Optional[dict] = None, linearise_on: Optional[str] = None,
               qp_data_on_device: bool = False, outer_on_device: bool = False, model=None,
               certify: bool = False) -> List[ScvxResult]:
    """scvx() for B initial conditions x0 (B, n) at once: the same trust-region loop per trajectory (own trust radii,
    own accept / reject decisions, own stop), but ONE batched QP solve per outer iteration -- per-instance dynamics,
    bounds and linear term (correction_qp_batch).  A trajectory that has stopped keeps its place in the batch with a
    zero-width box (its correction is then exactly zero) until the last one stops.
    linearise_on = "cuda:0": the central differences of the shipped model run as torch tensors on that device (linearise_device).
    qp_data_on_device (with linearise_on): the QP data go to the solver as a DeviceProblem -- A, B never leave the GPU -- and z
    comes back through admm_get_device; the QPs, and so every decision, are those of the default path bit for bit.
    outer_on_device (with linearise_on, the shipped rk4_step): everything between two QP solves -- rollout, linearisation, QP
    assembly, costs, decisions -- runs in the HIP kernels of DeviceOuterStep on the tensors the solver reads and writes; the host
    reads one integer per outer iteration.  Same scheme, same formulas; the roundings differ (device sqrt / fma), so the result
    agrees with the host loop to the QP tolerance, not bit for bit.
    model: a Model whose step replaces `step` (not both); linearise_on then evaluates model.rhs_torch, and outer_on_device runs the
    kernels of that model (DeviceOuterStep(model=...), the admm_scvx_*_model_device entry points).  Or a StageModel, a
    time-dependent model (4 sub-intervals per stage): the same three routes, the device one through admm_scvx_*_stage_device.
    certify: every result carries its trajectory's ScvxCertificate -- adjoint() on the host routes; with outer_on_device
    DeviceOuterStep.certify() (one more device call after the loop, one more host copy); nothing else changes."""
    step = _resolve(model, step)
    tm = _timed(model)
    x0 = np.atleast_2d(np.asarray(x0, np.float64))
    Bn = x0.shape[0]
    Q, R, QN = (np.asarray(a, np.float64) for a in (Q, R, QN))
    n, m = Q.shape[0], R.shape[0]
    u_lo = np.broadcast_to(np.asarray(u_lo, np.float64), (m,))
    u_hi = np.broadcast_to(np.asarray(u_hi, np.float64), (m,))
    if outer_on_device:
        if linearise_on is None or (step is not rk4_step and model is None):
            raise ValueError("outer_on_device needs linearise_on = 'cuda:k' and the shipped rk4_step")
        if qp_solver is None:
            qp_solver = gpu_qp_solver(True, z_on_device=True, **(qp_options or dict(rho=0.5, eps_abs=1e-8, eps_rel=1e-8,
                                                                                    max_iter=20000, check_interval=25)))
        loop = DeviceOuterStep(x0, N, dt, Q, R, QN, u_lo, u_hi, device=linearise_on, tol=tol, rho_reject=rho_reject,
                               rho_expand=rho_expand, max_outer=max_outer, model=model)
        loop.init(tr_u, tr_x)
        admm_iters: List[int] = []
        n_active = Bn
        for _ in range(max_outer):
            if n_active == 0:
                break
            z, iters = qp_solver(loop.prepare())
            admm_iters.append(iters)
            n_active = loop.advance(z)
        return loop.results(admm_iters, loop.certify() if certify else None)
    if qp_solver is None:
        qp_solver = gpu_qp_solver(qp_data_on_device, **(qp_options or dict(rho=0.5, eps_abs=1e-8, eps_rel=1e-8, max_iter=20000,
                                                                           check_interval=25)))
    ub = np.zeros((Bn, N, m))
    xb = rollout(x0, ub, dt, step, model=tm)
    J = trajectory_cost(xb, ub, Q, R, QN)
    tru = np.full(Bn, float(tr_u))
    trx = np.full(Bn, float(tr_x))
    active = np.ones(Bn, bool)
    converged = np.zeros(Bn, bool)
    accepted = np.zeros(Bn, int)
    hist: List[List[dict]] = [[] for _ in range(Bn)]
    for it in range(1, max_outer + 1):
        if not active.any():
            break
        p = correction_qp_batch(xb, ub, x0, dt, Q, R, QN, u_lo, u_hi, np.where(active, tru, 0.0), np.where(active, trx, 0.0), step,
                                device=linearise_on, qp_data_on_device=qp_data_on_device, model=model)
        z, admm_iters = qp_solver(p)
        d = np.asarray(z, np.float64).reshape(Bn, N, m + n)
        du, dx = d[..., :m], d[..., m:]
        J_lin = trajectory_cost(xb + dx, ub + du, Q, R, QN)
        u_new = np.clip(ub + du, u_lo, u_hi)
        x_new = rollout(x0, u_new, dt, step, model=tm)
        J_new = trajectory_cost(x_new, u_new, Q, R, QN)
        take, records = outer_update(J, J_lin, J_new, np.abs(du).max(axis=(1, 2)), tru, trx, active, converged, accepted,
                                     tol, rho_reject, rho_expand)
        ub[take], xb[take] = u_new[take], x_new[take]
        for b, rec in records.items():
            hist[b].append(dict(iteration=it, admm_iterations=admm_iters, **rec))
    cert = adjoint(x0, ub, xb, dt, Q, R, QN, u_lo, u_hi, step, model=tm) if certify else None
    return [ScvxResult(u=ub[b], x=xb[b], cost=float(J[b]), outer_iterations=len(hist[b]), accepted=int(accepted[b]),
                       converged=bool(converged[b]), history=hist[b], certificate=_certificate_row(cert, b)) for b in range(Bn)]


def _certificate_row(cert: Optional[ScvxCertificate], b: int) -> Optional[ScvxCertificate]:
    """Trajectory b of a batched certificate of NumPy arrays (None: None)."""
    if cert is None:
        return None
    return ScvxCertificate(*(None if a is None else a[b] for a in (cert.nu, cert.primer, cert.grad, cert.dJdx0)), float(cert.stat[b]),
                           int(cert.n_bound[b]))


class DeviceOuterStep:
    """The state of scvx_batch(outer_on_device=True) as torch tensors on one GPU, and the four device entry points on it
    (ADMM_HIP_HAS_SCVX): rollout / init / prepare / advance.  Without `model`: the shipped model (relative_motion_rhs,
    rk4_step) through admm_scvx_*_device; with a Model: its kind and parameters in an admm_scvx_dynamics, through
    admm_scvx_*_model_device (ADMM_HIP_HAS_SCVX_MODELS; rc is then not used); with a StageModel: its node table
    of the grid (N, dt, substeps), uploaded once, in an admm_scvx_stage_dynamics, through admm_scvx_*_stage_device (§2.8.3).
    certify() adds the costates and the optimality certificate of the nonlinear problem at the current reference
    (admm_scvx_adjoint_device; ADMM_HIP_HAS_SCVX_ADJOINT; §2.8.4), whatever the model.
    Every call is queued on torch's current stream; advance() alone waits -- for the count of trajectories still active."""

    STATE_F64 = ("ub", "xb", "u_cand", "x_cand", "J", "tr_u", "tr_x")
    STATE_I32 = ("active", "converged", "accepted", "outer", "take")

    def __init__(self, x0, N: int, dt: float, Q, R, QN, u_lo, u_hi, device: str = "cuda:0", substeps: int = 4, rc: float = RC_KM,
                 eps: float = 1e-6, tol: float = 1e-6, rho_reject: float = 0.1, rho_expand: float = 0.7, max_outer: int = 20,
                 model=None):
        import torch

        from . import _abi
        from .solver import load_library
        self._lib = load_library()
        self.device = torch.device(device)
        x0 = np.atleast_2d(np.asarray(x0, np.float64))
        Bn = x0.shape[0]
        self.batch, self.N = Bn, int(N)
        if isinstance(model, StageModel):
            # the table of the grid, uploaded once; the struct holds its device pointer
            self.nodes = torch.as_tensor(model.nodes(int(N), float(dt), int(substeps)), device=self.device)
            self.model, self._suffix = _abi.CScvxStageDynamics(N=int(N), batch=Bn, substeps=int(substeps), kind=int(model.kind), dt=float(dt),
                                                               nodes=self.ptr(self.nodes), n_nodes=int(self.nodes.shape[0])), "_stage_device"
            self.model.par[:len(model.par)] = [float(v) for v in model.par]
        elif model is None:
            self.model, self._suffix = _abi.CScvxModel(N=int(N), batch=Bn, substeps=int(substeps), dt=float(dt), rc=float(rc)), "_device"
        else:
            self.model, self._suffix = _abi.CScvxDynamics(N=int(N), batch=Bn, substeps=int(substeps), kind=int(model.kind), dt=float(dt)), "_model_device"
            self.model.par[:len(model.par)] = [float(v) for v in model.par]
        self.params = _abi.CScvxParams(fd_eps=float(eps), tol=float(tol), rho_reject=float(rho_reject), rho_expand=float(rho_expand))
        for name, a, shape in (("Q", Q, (6, 6)), ("R", R, (3, 3)), ("QN", QN, (6, 6)), ("u_lo", np.broadcast_to(u_lo, (3,)), (3,)),
                               ("u_hi", np.broadcast_to(u_hi, (3,)), (3,))):
            a = np.ascontiguousarray(a, np.float64)
            if a.shape != shape:
                raise ValueError(f"{name}: shape {a.shape}, expected {shape} (the shipped model has n = 6, m = 3)")
            getattr(self.params, name)[:] = a.reshape(-1).tolist()

        def f64(*shape):
            return torch.zeros(shape, dtype=torch.float64, device=self.device)
        self.x0 = torch.as_tensor(np.array(x0), device=self.device)
        self.t = {"ub": f64(Bn, N, 3), "xb": f64(Bn, N, 6), "u_cand": f64(Bn, N, 3), "x_cand": f64(Bn, N, 6),
                  "J": f64(Bn), "tr_u": f64(Bn), "tr_x": f64(Bn), "history": f64(max(int(max_outer), 1), Bn, 9)}
        for k in self.STATE_I32:
            self.t[k] = torch.zeros(Bn, dtype=torch.int32, device=self.device)
        # the QP of one outer iteration, filled by prepare(): A, B row-major blocks, box and linear term; its x0 is zero (dx_0 = 0)
        self.A, self.B = f64(Bn, N, 6, 6), f64(Bn, N, 6, 3)
        self.lo, self.hi, self.q = f64(Bn, N, 9), f64(Bn, N, 9), f64(Bn, N * 9)
        self.Qt, self.Rt, self.QNt = (torch.as_tensor(np.ascontiguousarray(a, np.float64), device=self.device) for a in (Q, R, QN))
        self.dx0 = f64(Bn, 6)
        self.state = self.c_state()

    @staticmethod
    def ptr(t):
        """double* / int32_t* of a CUDA tensor."""
        import ctypes as C

        import torch

        from ._abi import c_double_p, c_int32_p
        return C.cast(C.c_void_p(t.data_ptr()), c_int32_p if t.dtype == torch.int32 else c_double_p)

    def c_state(self, **override):
        """admm_scvx_state over the tensors (override: other tensors by field name, or history_capacity)."""
        from . import _abi
        t = dict(self.t, **{k: v for k, v in override.items() if k != "history_capacity"})
        return _abi.CScvxState(history_capacity=override.get("history_capacity", self.t["history"].shape[0]),
                               **{k: self.ptr(t[k]) for k in self.STATE_F64 + self.STATE_I32 + ("history",)})

    def _call(self, name, *args):
        import ctypes as C

        from .solver import _check, _stream
        fn = getattr(self._lib, name + self._suffix)
        _check(self._lib, fn(self.device.index or 0, C.byref(self.model), *args, _stream(self.device)))

    def rollout(self, u):
        """x_1 .. x_N (B, N, 6) of the nonlinear dynamics under the controls u (B, N, 3), a CUDA tensor."""
        import torch
        x = torch.empty((self.batch, self.N, 6), dtype=torch.float64, device=self.device)
        self._call("admm_scvx_rollout", self.ptr(self.x0), self.ptr(u), self.ptr(x))
        return x

    def init(self, tr_u: float, tr_x: float):
        import ctypes as C
        self._call("admm_scvx_init", C.byref(self.params), self.ptr(self.x0), C.byref(self.state), float(tr_u), float(tr_x))

    def prepare(self):
        """The correction QPs about the current reference as a DeviceProblem over this object's tensors (rewritten by each call)."""
        import ctypes as C

        from .problems import DeviceProblem
        self._call("admm_scvx_prepare", C.byref(self.params), self.ptr(self.x0), C.byref(self.state), self.ptr(self.A),
                   self.ptr(self.B), self.ptr(self.lo), self.ptr(self.hi), self.ptr(self.q))
        return DeviceProblem(N=self.N, A=self.A, B=self.B, Q=self.Qt, R=self.Rt, QN=self.QNt, x0=self.dx0, lo=self.lo, hi=self.hi,
                             q=self.q, name=f"scvx_correction_batch{self.batch}_N{self.N}")

    def certify(self, costates: bool = True) -> ScvxCertificate:
        """The ScvxCertificate of the current reference (ub, xb) as CUDA tensors (batch axis first): prepare() about it, then
        admm_scvx_adjoint_device on what prepare wrote -- so A, B, lo, hi, q are REWRITTEN, as by prepare().  costates=False: nu and
        primer are not written (None).  Queued on torch's current stream; nothing waits."""
        import ctypes as C

        import torch

        from . import _abi
        from .solver import _check, _stream
        self.prepare()
        Bn, N = self.batch, self.N

        def f64(*shape):
            return torch.empty(shape, dtype=torch.float64, device=self.device)
        t = dict(nu=f64(Bn, N, 6) if costates else None, primer=f64(Bn, N, 3) if costates else None, grad=f64(Bn, N, 3),
                 dJdx0=f64(Bn, 6), stat=f64(Bn), n_bound=torch.empty(Bn, dtype=torch.int32, device=self.device))
        out = _abi.CScvxAdjointOut(**{k: self.ptr(v) for k, v in t.items() if v is not None})
        _check(self._lib, self._lib.admm_scvx_adjoint_device(self.device.index or 0, N, Bn, C.byref(self.params), self.ptr(self.t["ub"]),
                                                             self.ptr(self.A), self.ptr(self.B), self.ptr(self.q), C.byref(out),
                                                             _stream(self.device)))
        return ScvxCertificate(**t)

    def advance(self, z) -> int:
        """Candidate, costs and decisions from the QP solutions z (B, N * 9): a CUDA tensor (or a NumPy array, uploaded).  Returns the
        number of trajectories still active."""
        import ctypes as C

        import torch
        if not torch.is_tensor(z):
            z = torch.as_tensor(np.ascontiguousarray(z, np.float64), device=self.device)
        if tuple(z.shape) != (self.batch, self.N * 9) or z.dtype != torch.float64 or not z.is_contiguous() or z.device != self.x0.device:
            raise ValueError(f"z: expected a contiguous fp64 ({self.batch}, {self.N * 9}) tensor on {self.x0.device}")
        n_active = C.c_int32(-1)
        self._call("admm_scvx_advance", C.byref(self.params), self.ptr(self.x0), self.ptr(z), C.byref(self.state),
                   C.byref(n_active))
        return int(n_active.value)

    def results(self, admm_iterations, certificate: Optional[ScvxCertificate] = None) -> List[ScvxResult]:
        """The loop's state as scvx_batch returns it (one copy of each tensor to the host).  certificate: what certify() returned;
        each result then carries its trajectory's part (one more copy to the host)."""
        from ._abi import SCVX_HISTORY_FIELDS
        h = {k: v.cpu().numpy() for k, v in self.t.items()}
        if certificate is not None:
            certificate = ScvxCertificate(*(None if v is None else v.cpu().numpy() for v in (certificate.nu, certificate.primer, certificate.grad, certificate.dJdx0, certificate.stat,
                                                                                                   certificate.n_bound)))
        out = []
        for b in range(self.batch):
            hist = []
            for it in range(int(h["outer"][b])):
                rec = dict(zip(SCVX_HISTORY_FIELDS, (float(v) for v in h["history"][it, b])))
                rec["accepted"] = bool(rec["accepted"])
                hist.append(dict(iteration=it + 1, admm_iterations=int(admm_iterations[it]), **rec))
            out.append(ScvxResult(u=h["ub"][b], x=h["xb"][b], cost=float(h["J"][b]), outer_iterations=len(hist),
                                  accepted=int(h["accepted"][b]), converged=bool(h["converged"][b]), history=hist,
                                  certificate=_certificate_row(certificate, b)))
        return out
