#!/usr/bin/env python3
"""Fuel-optimal Clohessy-Wiltshire rendezvous: minimise  1/2 (quadratic cost) + f sum_k ||u_k||_2  under the thrust bound
||u_k||_2 <= u_max for a batch of initial states, and print how the stages split into coast / intermediate / saturated.

    python examples/min_fuel_rendezvous.py [batch] [horizon] [weight / dt]

Needs an MI355X and the built library (python -c "import __graft_entry__ as g; g.build()")."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_library_amd as pkg   # noqa: E402

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
c = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0
u_max = 0.2
problem = pkg.cw_rendezvous_fuel(N=N, batch=batch, u_max=u_max, fuel=c * 2.0 * np.pi / N)
options = pkg.Options(rho=1.0, eps_abs=1e-6, eps_rel=1e-6, max_iter=6000, check_interval=10)
with pkg.Solver(problem, options) as s:
    info = s.solve()
    _, z, _ = s.get()
    thrust = np.linalg.norm(z.reshape(batch, N, 9)[:, :, :3], axis=2)
    coast, full = thrust == 0.0, thrust >= u_max * (1 - 1e-9)
    print(f"{batch} QPs, horizon {N}, weight {float(problem.fuel):.4g}: {info.iters_run} iterations in {info.solve_ms:.1f} ms, "
          f"{info.n_converged}/{batch} converged")
    print(f"stages: {100 * coast.mean():.1f} % coast (u = 0 exactly), {100 * (~coast & ~full).mean():.1f} % intermediate, "
          f"{100 * full.mean():.1f} % at the thrust bound;  propellant sum ||u|| dt per QP: median "
          f"{np.median(thrust.sum(axis=1)) * 2 * np.pi / N:.4f}")
    # continuation in the weight: a heavier fuel term from this solution as a warm start
    s.set_fuel(4.0 * float(problem.fuel))
    info = s.solve()
    _, z, _ = s.get()
    thrust = np.linalg.norm(z.reshape(batch, N, 9)[:, :, :3], axis=2)
    print(f"weight x 4 (warm start): {info.iters_run} iterations, {info.n_converged}/{batch} converged, {100 * (thrust == 0).mean():.1f} % coast")
