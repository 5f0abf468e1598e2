#!/usr/bin/env python3
"""A Monte-Carlo set of nonlinear rendezvous problems by BATCHED successive convexification (needs an MI355X).

B chasers start from scattered relative states; every outer iteration linearises the exact relative-motion dynamics about
each chaser's own trajectory and solves ALL correction QPs as one batch with per-instance dynamics, box and linear term
(admm_problem.time_varying = 2: device factorisation, per-QP segments in time).

    python examples/scvx_batch_rendezvous.py [B=64] [N=200] [--device-data] [--outer-on-device]

--device-data: run the batch a second time with the QP data handed to the solver in GPU memory (a DeviceProblem: A, B stay
where the linearisation made them; admm_update_problem_device, admm_get_device) and print its solver-call time next to the
default path's; the two runs must agree exactly.
--outer-on-device: run the batch again with the whole outer step on the GPU (scvx_batch(outer_on_device=True): rollout,
linearisation, QP assembly, costs and decisions in HIP kernels on the tensors the solver reads and writes) and
print, per mode, the wall time, the time in the solver calls and the remainder -- what the outer loop itself costs -- and how
the result compares with the default mode's: decision counts per trajectory, largest relative cost difference."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_library_amd as pkg                        # noqa: E402
from admm_library_amd import scvx as sc               # noqa: E402

device_data = "--device-data" in sys.argv[1:]
outer_on_device = "--outer-on-device" in sys.argv[1:]
args = [a for a in sys.argv[1:] if not a.startswith("--")]
B = int(args[0]) if len(args) > 0 else 64
N = int(args[1]) if len(args) > 1 else 200
dt = 2 * np.pi / N
Q = np.diag([1, 1, 1, .1, .1, .1]) * dt * 1e-3
R = np.eye(3) * dt * 0.05
QN = np.diag([50., 50, 50, 20, 20, 20])
rng = np.random.default_rng(11)
x0 = np.array([10.0, 150.0, 30.0, 0.0, -15.0, 0.0]) * (1.0 + 0.05 * rng.standard_normal((B, 6)))

def timed_solver(solves, on_device=False, z_on_device=False):
    # per-QP residual balancing on the device; SCVX_ADAPT=0 for fixed rho
    every = int(os.environ.get("SCVX_ADAPT", "100"))
    adapt = dict(adapt_interval=every, adapt_mu=5.0) if every > 0 else {}
    inner = sc.gpu_qp_solver(on_device, z_on_device=z_on_device, rho=0.5, eps_abs=1e-8, eps_rel=1e-8, max_iter=20000,
                             check_interval=25, **adapt)

    def solve(p):
        t = time.perf_counter()
        z, iters = inner(p)
        solves.append((time.perf_counter() - t, iters))
        return z, iters
    return solve


def run(on_device=False, outer=False):
    solves = []
    t0 = time.perf_counter()
    res = sc.scvx_batch(x0, N, dt, Q, R, QN, -3.0, 3.0, qp_solver=timed_solver(solves, on_device or outer, outer), tr_u=1.0, tr_x=100.0,
                        max_outer=25, tol=1e-7,
                        linearise_on="cuda:0" if on_device or outer or not os.environ.get("SCVX_HOST_LINEARISE") else None,
                        qp_data_on_device=on_device, outer_on_device=outer)
    return res, solves, time.perf_counter() - t0


def split(name, solves, wall, res):
    t = sum(s[0] for s in solves)
    print(f"  {name:<16} {wall:7.2f} s wall = {t:6.2f} s in the solver calls + {wall - t:6.2f} s outside them; "
          f"at most {max(r.outer_iterations for r in res)} outer iterations")


res, solves, wall = run()
outer = max(r.outer_iterations for r in res)
print(f"{B} trajectories, N = {N}: {sum(r.converged for r in res)} converged in at most {outer} outer iterations, {wall:.2f} s wall")
print(f"  QP batches: {len(solves)} solves, {sum(s[1] for s in solves)} ADMM batch-iterations, "
      f"{sum(s[0] for s in solves):.2f} s in the solver calls (upload + device refactor + iterations + read-out)")
print(f"  first / last QP batch: {solves[0][1]} iterations in {solves[0][0] * 1e3:.0f} ms, {solves[-1][1]} in {solves[-1][0] * 1e3:.0f} ms")
err = np.array([np.linalg.norm(r.x[-1, :3]) for r in res])
print(f"  terminal position error [km]: median {np.median(err):.3f}, max {err.max():.3f}; cost median {np.median([r.cost for r in res]):.3f}")
if device_data:
    res_d, solves_d, wall_d = run(on_device=True)
    same = all(np.array_equal(a.u, b.u) and np.array_equal(a.x, b.x) and a.cost == b.cost and a.outer_iterations == b.outer_iterations
               for a, b in zip(res, res_d))
    print(f"  solver calls: {sum(s[0] for s in solves):.2f} s host arrays, {sum(s[0] for s in solves_d):.2f} s device data "
          f"(--device-data; {wall_d:.2f} s wall); results identical: {same}")
if outer_on_device:
    res_o, solves_o, wall_o = run(outer=True)
    split("default", solves, wall, res)
    if device_data:
        split("--device-data", solves_d, wall_d, res_d)
    split("--outer-on-device", solves_o, wall_o, res_o)
    same_outer = sum(a.outer_iterations == b.outer_iterations for a, b in zip(res, res_o))
    same_acc = sum(a.accepted == b.accepted for a, b in zip(res, res_o))
    dcost = max(abs(a.cost - b.cost) / abs(a.cost) for a, b in zip(res, res_o))
    print(f"  --outer-on-device vs default: outer_iterations agree on {same_outer} of {B} trajectories, accepted on {same_acc} of {B}, "
          f"{sum(r.converged for r in res_o)} converged; largest relative cost difference {dcost:.2e}")
