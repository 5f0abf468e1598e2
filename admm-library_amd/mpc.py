"""Receding-horizon (MPC) loops on one persistent solver handle.

One step: solve the QP from a warm start, apply the first control u_0 (+ actuation error) to the plant, take the state it
reaches (+ process noise) as the next x0, move the horizon one stage.  With on_device=True everything between two solves is
one call, Solver.mpc_advance (admm_mpc_advance: two kernels on the state where it lies).  on_device=False is the same step
written out on the host from calls that existed before it -- get, a NumPy shift, update_instances, set_state: the defining
property of admm_mpc_advance, the reference of its tests and the "before" of its timing.
"""
from __future__ import annotations

import dataclasses
import time
from typing import Optional

import numpy as np

from .problems import Problem

TAILS = ("copy", "zero")


def shift_horizon(a: np.ndarray, nb: int, tail: str = "copy", fill: Optional[np.ndarray] = None) -> np.ndarray:
    """(batch, L) stacked array moved one stage: block k <- block k + 1 (blocks of nb entries); the last block keeps its content
    (tail "copy": the old last block appears twice), becomes 0 ("zero"), or is `fill` (batch, nb) where that is given."""
    if tail not in TAILS:
        raise ValueError(f"tail must be one of {TAILS}, got {tail!r}")
    a = np.asarray(a, np.float64)
    if a.ndim != 2 or a.shape[1] % nb or a.shape[1] < nb:
        raise ValueError(f"expected (batch, N * {nb}), got {a.shape}")
    out = np.empty_like(a)
    out[:, :-nb] = a[:, nb:]
    if fill is not None:
        out[:, -nb:] = fill
    elif tail == "zero":
        out[:, -nb:] = 0.0
    else:
        out[:, -nb:] = a[:, -nb:]
    return out


def plant_step(x0, u, Ap, Bp, dx=None) -> np.ndarray:
    """x+ = dx + Ap x0 + Bp u for a batch: x0 (batch, n), u (batch, m)."""
    xn = x0 @ np.asarray(Ap, np.float64).T + u @ np.asarray(Bp, np.float64).T
    return xn if dx is None else dx + xn


def model_plant(problem: Problem):
    """(A_0, B_0): the plant admm_mpc_advance uses when none is given -- stage 0 of the handle's own (batch-shared) dynamics."""
    if problem.per_instance:
        raise ValueError("per-instance dynamics have no receding-horizon step (admm_mpc_advance refuses them)")
    return (problem.A[0], problem.B[0]) if problem.time_varying else (problem.A, problem.B)


@dataclasses.dataclass
class MpcResult:
    X: np.ndarray             # (steps + 1, batch, n): X[t] is the x0 of step t's QP, X[t + 1] the state its control led to
    U: np.ndarray             # (steps, batch, m): the controls applied (first control of each solve + du)
    iterations: np.ndarray    # (steps,) ADMM iterations of each solve
    converged: np.ndarray     # (steps,) QPs that met the stopping rule
    solve_ms: np.ndarray      # (steps,) wall time of each solve
    step_ms: np.ndarray       # (steps,) wall time between two solves: apply, propagate, shift


def _noise(noise, steps, batch, n, m):
    """noise = None; a float sigma (process noise dx ~ sigma N(0, 1), default_rng(0)); or (du, dx) with du (steps, batch, m), dx
    (steps, batch, n), either None."""
    if noise is None:
        return None, None
    if np.isscalar(noise):
        return None, float(noise) * np.random.default_rng(0).standard_normal((steps, batch, n))
    du, dx = noise
    du = None if du is None else np.ascontiguousarray(du, np.float64)
    dx = None if dx is None else np.ascontiguousarray(dx, np.float64)
    if (du is not None and du.shape != (steps, batch, m)) or (dx is not None and dx.shape != (steps, batch, n)):
        raise ValueError(f"noise: expected du {(steps, batch, m)} and dx {(steps, batch, n)}")
    return du, dx


def mpc_batch(problem: Problem, steps: int, options=None, plant=None, noise=None, tail: str = "copy", on_device: bool = True,
              qp_solver=None, replay=None, on_step=None) -> MpcResult:
    """The closed loop over `steps` steps for a batch of QPs on one handle.

    plant = (Ap, Bp): the true plant (None: the model's A_0, B_0).  noise: see _noise.  tail: what the new last stage of the
    warm start holds ("copy" / "zero"); a problem with q keeps q's last block under "copy" and zeroes it under "zero".
    on_device: the step between two solves is Solver.mpc_advance; False: the host route (get, NumPy shift, update_instances,
    set_state).  replay = X of an earlier run: the recorded x+ are fed back (as x_meas on the device route) instead of
    evaluating the plant, so that two routes whose plant arithmetic rounds differently walk through the same QPs.
    qp_solver(problem, z0, y0) -> (w, z, y, iterations, converged): a stand-in for the handle (CPU tests drive the loop with
    the oracle); it implies the host route, and z0 = y0 = None asks for a cold start.
    on_step(t, solver, info): called after the solve of step t, before the step is taken, on the handle itself -- read-outs of the
    window's solution (Solver.soft_report(), .certificate(), .infeasibility(), ...).  Not with qp_solver."""
    if tail not in TAILS:
        raise ValueError(f"tail must be one of {TAILS}, got {tail!r}")
    if steps < 1:
        raise ValueError("steps must be >= 1")
    n, m, nb, batch = problem.n, problem.m, problem.nb, problem.batch
    Ap, Bp = model_plant(problem) if plant is None else (np.asarray(a, np.float64) for a in plant)
    du, dx = _noise(noise, steps, batch, n, m)
    if replay is not None:
        replay = np.asarray(replay, np.float64)
        if replay.shape != (steps + 1, batch, n):
            raise ValueError(f"replay: expected {(steps + 1, batch, n)}, got {replay.shape}")
    X = np.empty((steps + 1, batch, n))
    U = np.empty((steps, batch, m))
    X[0] = problem.x0
    iters, nconv = np.zeros(steps, np.int64), np.zeros(steps, np.int64)
    solve_ms, step_ms = np.zeros(steps), np.zeros(steps)
    q = None if problem.q is None else np.ascontiguousarray(problem.q, np.float64)

    def host_step(t, z):
        u = z[:, :m] if du is None else z[:, :m] + du[t]
        xn = replay[t + 1] if replay is not None else plant_step(X[t], u, Ap, Bp, None if dx is None else dx[t])
        return u, np.ascontiguousarray(xn)

    if qp_solver is not None:
        z = y = None
        cur = problem
        for t in range(steps):
            t0 = time.perf_counter()
            w, z, y, iters[t], nconv[t] = qp_solver(cur, z, y)
            t1 = time.perf_counter()
            U[t], X[t + 1] = host_step(t, z)
            z, y = shift_horizon(z, nb, tail), shift_horizon(y, nb, tail)
            if q is not None:
                q = shift_horizon(q, nb, tail)
            cur = dataclasses.replace(cur, x0=X[t + 1].copy(), q=q)
            solve_ms[t], step_ms[t] = (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3
        return MpcResult(X, U, iters, nconv, solve_ms, step_ms)

    from .solver import Solver
    with Solver(problem, options) as s:
        for t in range(steps):
            t0 = time.perf_counter()
            info = s.solve()                        # (from the handle's state: zeros at step 0, the shifted solution afterwards)
            t1 = time.perf_counter()
            iters[t], nconv[t] = info.iters_run, info.n_converged
            t2 = t1
            if on_step is not None:
                on_step(t, s, info)
                t2 = time.perf_counter()            # (the read-outs belong to neither figure)
            if on_device:
                kw = dict(x_meas=np.ascontiguousarray(replay[t + 1])) if replay is not None else \
                    dict(plant=None if plant is None else (Ap, Bp), dx=None if dx is None else dx[t])
                U[t], X[t + 1] = s.mpc_advance(du=None if du is None else du[t], tail=tail, **kw)
            else:
                w, z, y = s.get()
                U[t], X[t + 1] = host_step(t, z)
                if q is not None:
                    q = shift_horizon(q, nb, tail)
                s.update_instances(X[t + 1], q)
                s.set_state(shift_horizon(w, nb, tail), shift_horizon(z, nb, tail), shift_horizon(y, nb, tail))
            solve_ms[t], step_ms[t] = (t1 - t0) * 1e3, (time.perf_counter() - t2) * 1e3
    return MpcResult(X, U, iters, nconv, solve_ms, step_ms)
