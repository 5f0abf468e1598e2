#!/usr/bin/env python3
"""Cislunar station acquisition by BATCHED successive convexification (needs an MI355X).

A Monte-Carlo set of B insertion errors about the Earth-Moon L2 point is driven to the point: the dynamics are the circular
restricted three-body problem in the rotating frame, the state measured from L2 (scvx.crtbp(mu, x_ref)), so the
origin is an (unstable) equilibrium and the loop's quadratic cost means "acquire the libration point".  Nondimensional units:
length = the Earth-Moon distance, time = 1 / mean motion (the horizon of 2 is 8.7 days), thrust acceleration box +-0.5; the state
trust radius 0.02 keeps the corrections where the linear model holds about an unstable point.

    python examples/scvx_cislunar.py [B=64] [N=40] [--outer-on-device] [--repeat=1]

Three routes through scvx_batch(model=crtbp(...)), in one process:
  host loop          everything between two QP solves in NumPy (model.step)
  torch route        linearise_on + qp_data_on_device: the central differences of model.rhs_torch as torch tensors, the QP data
                     handed to the solver in GPU memory; rollout, costs and decisions in NumPy
  --outer-on-device  rollout, linearisation, QP assembly, costs and decisions in the HIP kernels of the CR3BP model
                     (admm_scvx_*_model_device) on the tensors the solver reads and writes
and prints, per route, the wall time, the time in the solver calls and the remainder -- what the outer loop itself costs --, the
outer iterations, and how the routes agree.  --repeat=K runs the routes K times interleaved and prints the medians."""
import os
import sys
import time

import numpy as np
import torch          # noqa: F401  -- before libadmm_hip.so is loaded (by the first solve): both then share one HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from admm_library_amd import scvx as sc               # noqa: E402

outer_on_device = "--outer-on-device" in sys.argv[1:]
repeat = max([int(a.split("=")[1]) for a in sys.argv[1:] if a.startswith("--repeat=")] + [1])
args = [a for a in sys.argv[1:] if not a.startswith("--")]
B = int(args[0]) if len(args) > 0 else 64
N = int(args[1]) if len(args) > 1 else 40
dt = 2.0 / N                                           # a horizon of 2 time units (8.7 days): 0.05 per stage at N = 40
Q = np.diag([1, 1, 1, .1, .1, .1]) * dt
R = np.eye(3) * dt * 0.05
QN = np.diag([50., 50, 50, 20, 20, 20])
U_MAX = 0.5
mu = sc.MU_EARTH_MOON
model = sc.crtbp(mu, sc.crtbp_collinear_point(mu, 2))
rng = np.random.default_rng(11)
x0 = np.array([0.03, -0.03, 0.015, 0.0, 0.0, 0.0]) * (1.0 + 0.1 * rng.standard_normal((B, 6)))
x0[:, 3:] += 0.005 * rng.standard_normal((B, 3))


def timed_solver(solves, on_device=False, z_on_device=False):
    inner = sc.gpu_qp_solver(on_device, z_on_device=z_on_device, rho=0.5, eps_abs=1e-8, eps_rel=1e-8, max_iter=20000, check_interval=25)

    def solve(p):
        t = time.perf_counter()
        z, iters = inner(p)
        solves.append((time.perf_counter() - t, iters))
        return z, iters
    return solve


def run(route):
    solves = []
    kw = {"host": dict(), "torch": dict(linearise_on="cuda:0", qp_data_on_device=True),
          "device": dict(linearise_on="cuda:0", outer_on_device=True)}[route]
    t0 = time.perf_counter()
    res = sc.scvx_batch(x0, N, dt, Q, R, QN, -U_MAX, U_MAX, qp_solver=timed_solver(solves, route != "host", route == "device"),
                        model=model, tr_u=0.1, tr_x=0.02, max_outer=20, tol=1e-6, **kw)
    return res, solves, time.perf_counter() - t0


ROUTES = [("host", "host loop"), ("torch", "torch route")] + ([("device", "--outer-on-device")] if outer_on_device else [])
runs = {r: [] for r, _ in ROUTES}
for _ in range(repeat):
    for r, _name in ROUTES:
        runs[r].append(run(r))
        print(f"[{_name}: {runs[r][-1][2]:.1f} s]", flush=True)      # a sign of life: the large sizes take minutes per route

res = runs["host"][0][0]
free = sc.rollout(x0, np.zeros((B, N, 3)), dt, model.step)
err = np.array([np.linalg.norm(r.x[-1, :3]) for r in res])
print(f"{B} insertion errors about Earth-Moon L2 (X = {model.par[1]:.6f}), N = {N} stages of {dt}: "
      f"{sum(r.converged for r in res)} converged in at most {max(r.outer_iterations for r in res)} outer iterations")
print(f"  distance from L2 at the end of the horizon: uncontrolled median {np.median(np.linalg.norm(free[:, -1, :3], axis=1)):.3f}, "
      f"controlled median {np.median(err):.2e}, max {err.max():.2e}; largest |u| {max(np.abs(r.u).max() for r in res):.3f}")
for r, name in ROUTES:
    wall = float(np.median([w for _, _, w in runs[r]]))
    t = float(np.median([sum(s[0] for s in solves) for _, solves, _ in runs[r]]))
    rr, solves, _ = runs[r][0]
    print(f"  {name:<18} {wall:7.2f} s wall = {t:6.2f} s in the solver calls + {wall - t:6.2f} s outside them; {len(solves)} QP batches, "
          f"{sum(s[1] for s in solves)} ADMM batch-iterations, at most {max(x.outer_iterations for x in rr)} outer iterations")
for r, name in ROUTES[1:]:
    other = runs[r][0][0]
    same_outer = sum(a.outer_iterations == b.outer_iterations for a, b in zip(res, other))
    same_acc = sum(a.accepted == b.accepted for a, b in zip(res, other))
    dcost = max(abs(a.cost - b.cost) / abs(a.cost) for a, b in zip(res, other))
    print(f"  {name} vs host loop: outer_iterations agree on {same_outer} of {B} trajectories, accepted on {same_acc} of {B}, "
          f"{sum(x.converged for x in other)} converged; largest relative cost difference {dcost:.2e}")
