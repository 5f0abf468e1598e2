#!/usr/bin/env python3
"""Primer vector of a fuel-optimal Clohessy-Wiltshire rendezvous, from the on-device certificate.

Solves cw_rendezvous_fuel, asks the handle for the objective, the stationarity defect and the costates nu of every QP
(Solver.certificate: nothing but these cross PCIe), and checks Lawden's condition on the primer vector p_k = B_k' nu_{k+1}:
    coast  (u_k = 0):              ||p_k||_2 <= f
    burn, inside the thrust bound: ||p_k - R u_k||_2 = f

    python examples/primer_vector.py [batch] [horizon]

Needs an MI355X and the built library (python -c "import __graft_entry__ as g; g.build()")."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_library_amd as pkg   # noqa: E402

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 8
N = int(sys.argv[2]) if len(sys.argv) > 2 else 300
u_max = 0.2
problem = pkg.cw_rendezvous_fuel(N=N, batch=batch, u_max=u_max)
f = float(problem.fuel)
options = pkg.Options(rho=1.0, eps_abs=1e-8, eps_rel=1e-8, max_iter=20000, check_interval=10)
with pkg.Solver(problem, options) as s:
    info = s.solve()
    cert = s.certificate(costates=True)
    _, z, _ = s.get()
print(f"{batch} QPs, horizon {N}, weight {f:.4g}: {info.iters_run} iterations, {info.n_converged}/{batch} converged")
for b in range(min(batch, 8)):
    print(f"  QP {b}: objective {cert.obj[b]:.6f}   stat {cert.stat[b]:.2e}   dynamics defect {cert.feas_dyn[b]:.2e}")
u = z.reshape(batch, N, 9)[:, :, :3]
primer = cert.nu @ problem.B                            # (batch, N, 3): B' nu_{k+1} (LTI: one B)
thrust = np.linalg.norm(u, axis=2)
coast = thrust == 0.0
interior = ~coast & (thrust < u_max * (1 - 1e-9))
tol = np.sqrt(3.0) * cert.stat[:, None] + 1e-12
ok_coast = np.linalg.norm(primer, axis=2) <= f + tol
ok_burn = np.abs(np.linalg.norm(primer - u @ problem.R, axis=2) - f) <= tol
print(f"coast stages: {100 * coast.mean():.1f} % of all; ||B' nu|| <= f holds at {100 * ok_coast[coast].mean():.1f} % of them")
if interior.any():
    print(f"interior burn stages: {100 * interior.mean():.1f} % of all; ||B' nu - R u|| = f holds at "
          f"{100 * ok_burn[interior].mean():.1f} % of them")
else:
    print("interior burn stages: none (every burn is at the thrust bound)")
