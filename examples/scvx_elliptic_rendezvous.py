#!/usr/bin/env python3
"""Rendezvous with a chief on an ECCENTRIC orbit by BATCHED successive convexification (needs an MI355X).

A Monte-Carlo set of B insertion errors (45 km along-track, 9 km cross-track, scattered by 10 %) is driven to a chief on a Kepler
orbit with a = 7000 km and e = 0.3, starting at mean anomaly 0.4: the dynamics are the exact nonlinear relative motion in the
chief's rotating frame, whose coefficients -- the chief's radius, angular rate and angular acceleration -- change along the orbit
(scvx.relative_elliptic(a, e, M0)).  Units: length 1 km, time 1 / mean motion (the horizon of 2 is a third of the
chief's orbit), thrust acceleration box +-60.

    python examples/scvx_elliptic_rendezvous.py [B=64] [N=40] [--outer-on-device] [--repeat=1] [--only=ROUTE] [--model=circular]
                                                [--max-outer=20]

First the design a caller without this model would make: the same loop with the circular model (scvx.relative_circular(a)), on
the first 8 insertion errors with the host loop, flown open loop on the eccentric plant -- and the miss it leaves.  Then three routes
through scvx_batch(model=relative_elliptic(...)), in one process:
  host loop          everything between two QP solves in NumPy
  torch route        linearise_on + qp_data_on_device: the central differences of model.rhs_torch as torch tensors (node rows broadcast
                     along the stage axis), the QP data handed to the solver in GPU memory; rollout, costs and decisions in NumPy
  --outer-on-device  rollout, linearisation, QP assembly, costs and decisions in the HIP kernels of the tabulated model
                     (admm_scvx_*_stage_device) on the tensors the solver reads and writes; the node table is uploaded once
and prints, per route, the wall time, the time in the solver calls and the remainder -- what the outer loop itself costs --, the
outer iterations, and how the routes agree.  --repeat=K runs the routes K times interleaved and prints the medians.
--only=host|torch|device runs that route alone (for a profiler); --model=circular runs the routes with the circular model instead
(the same sizes through the kernels of admm_scvx_*_model_device, for a comparison of the kernels); --max-outer=K cuts the loop
after K outer iterations."""
import os
import sys
import time

import numpy as np
import torch          # noqa: F401  -- before libadmm_hip.so is loaded (by the first solve): both then share one HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from admm_library_amd import scvx as sc               # noqa: E402

flags = [a for a in sys.argv[1:] if a.startswith("--")]
outer_on_device = "--outer-on-device" in flags
repeat = max([int(a.split("=")[1]) for a in flags if a.startswith("--repeat=")] + [1])
only = ([a.split("=")[1] for a in flags if a.startswith("--only=")] + [None])[0]
circular = "--model=circular" in flags
args = [a for a in sys.argv[1:] if not a.startswith("--")]
B = int(args[0]) if len(args) > 0 else 64
N = int(args[1]) if len(args) > 1 else 40
dt = 2.0 / N                                           # a horizon of 2 time units: 0.05 per stage at N = 40
Q = np.diag([1, 1, 1, .1, .1, .1]) * dt
R = np.eye(3) * dt * 0.05
QN = np.diag([50., 50, 50, 20, 20, 20])
U_MAX = 60.0
A_KM, ECC, M0 = 7000.0, 0.3, 0.4
plant = sc.relative_elliptic(A_KM, ECC, M0)
design = sc.relative_circular(A_KM)
model = design if circular else plant
max_outer = max([int(a.split("=")[1]) for a in flags if a.startswith("--max-outer=")] + [0]) or 20
SCVX = dict(tr_u=5.0, tr_x=20.0, max_outer=max_outer, tol=1e-6)
rng = np.random.default_rng(11)
x0 = 0.3 * np.array([10.0, 150.0, 30.0, 0.0, -15.0, 0.0]) * (1.0 + 0.1 * rng.standard_normal((B, 6)))


def timed_solver(solves, on_device=False, z_on_device=False):
    inner = sc.gpu_qp_solver(on_device, z_on_device=z_on_device, rho=0.5, eps_abs=1e-8, eps_rel=1e-8, max_iter=20000, check_interval=25)

    def solve(p):
        t = time.perf_counter()
        z, iters = inner(p)
        solves.append((time.perf_counter() - t, iters))
        return z, iters
    return solve


def run(route, x0=x0, model=model):
    solves = []
    kw = {"host": dict(), "torch": dict(linearise_on="cuda:0", qp_data_on_device=True),
          "device": dict(linearise_on="cuda:0", outer_on_device=True)}[route]
    t0 = time.perf_counter()
    res = sc.scvx_batch(x0, N, dt, Q, R, QN, -U_MAX, U_MAX, qp_solver=timed_solver(solves, route != "host", route == "device"),
                        model=model, **SCVX, **kw)
    return res, solves, time.perf_counter() - t0


ROUTES = [("host", "host loop"), ("torch", "torch route")] + ([("device", "--outer-on-device")] if outer_on_device else [])
if only is not None:
    ROUTES = [(r, name) for r, name in ROUTES + [("device", "--outer-on-device")] if r == only][:1]

if only is None and not circular:
    nb = min(B, 8)
    circ, _, _ = run("host", x0[:nb], design)
    flown = sc.rollout(x0[:nb], np.stack([r.u for r in circ]), dt, model=plant)
    miss = np.linalg.norm(flown[:, -1, :3], axis=1)
    own = np.array([np.linalg.norm(r.x[-1, :3]) for r in circ])
    print(f"the circular model's design on the eccentric plant (e = {ECC}), first {nb} insertion errors: it believes it arrives within "
          f"{own.max():.3f} km; flown, it misses by {np.median(miss):.1f} km (median), {miss.max():.1f} km (max)", flush=True)

runs = {r: [] for r, _ in ROUTES}
for _ in range(repeat):
    for r, _name in ROUTES:
        runs[r].append(run(r))
        print(f"[{_name}: {runs[r][-1][2]:.1f} s]", flush=True)      # a sign of life: the large sizes take minutes per route

first = ROUTES[0][0]
res = runs[first][0][0]
free = sc.rollout(x0, np.zeros((B, N, 3)), dt, model=model)
err = np.array([np.linalg.norm(r.x[-1, :3]) for r in res])
print(f"{B} insertion errors about a chief with a = {A_KM:.0f} km, e = {0.0 if circular else ECC} ({model.name}), N = {N} stages of {dt}: "
      f"{sum(r.converged for r in res)} converged in at most {max(r.outer_iterations for r in res)} outer iterations")
print(f"  distance from the chief at the end of the horizon: uncontrolled median {np.median(np.linalg.norm(free[:, -1, :3], axis=1)):.1f} km, "
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
