#!/usr/bin/env python3
"""Receding-horizon control of a Clohessy-Wiltshire station approach under process noise.

One persistent handle per route: solve the window's QP from the shifted previous solution, fly the first control, take the state
the (noisy) plant reaches as the next x0, move the window one stage.  The loop runs twice on the same noise --

  device route   the step between two solves is Solver.mpc_advance (admm_mpc_advance: two kernels on the state where it lies)
  host route     get, NumPy shift, update_instances, set_state, fed the device route's recorded states (replay=), so that both
                 routes walk through the same QPs

-- and a third handle solves every step's QP cold.  Per step: warm and cold iteration counts, and the wall time between two
solves on both routes.

    python examples/mpc_rendezvous.py [batch] [horizon] [steps] [rho]

A warm start is not always a win here: cw_rendezvous weighs the terminal state heavily, and when the window moves, the stage
that was terminal becomes an ordinary one -- the shifted solution is a poor guess for exactly the rows the cost cares most about.
On the CPU oracle at horizon 40, rho = 1, batch 8, the warm solves take 95, 155, 145, 155, 120 iterations over steps 1 .. 5
against 210, 195, 165, 145, 100 cold: ahead over the first steps, behind at steps 4 and 5.  The table shows what it shows.

Needs an MI355X and the built library (python -c "import __graft_entry__ as g; g.build()")."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_library_amd as pkg   # noqa: E402

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 8
N = int(sys.argv[2]) if len(sys.argv) > 2 else 40
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 8
rho = float(sys.argv[4]) if len(sys.argv) > 4 else 1.0
SIGMA = 1e-3

p = pkg.cw_rendezvous(N=N, batch=batch)
opt = pkg.Options(rho=rho, check_interval=5)
dev = pkg.mpc_batch(p, steps, opt, noise=SIGMA, on_device=True)
host = pkg.mpc_batch(p, steps, opt, noise=SIGMA, on_device=False, replay=dev.X)
same = np.array_equal(dev.U, host.U) and np.array_equal(dev.iterations, host.iterations)

cold = np.zeros(steps, np.int64)
zero = np.zeros((batch, p.L))
with pkg.Solver(p, opt) as s:
    for t in range(steps):
        s.update_instances(dev.X[t])
        cold[t] = s.solve(z0=zero, y0=zero).iters_run

print(f"cw_rendezvous, batch {batch}, horizon {N}, process noise {SIGMA:g}; both routes apply the same controls: {same}")
print(" step   warm   cold   converged   solve ms   step ms (device)   step ms (host)   |x|_max")
for t in range(steps):
    print(f"{t:5d} {dev.iterations[t]:6d} {cold[t]:6d} {dev.converged[t]:7d}/{batch:<4d} {dev.solve_ms[t]:9.2f} "
          f"{dev.step_ms[t]:15.3f} {host.step_ms[t]:16.3f} {np.abs(dev.X[t + 1]).max():10.4f}")
worse = [t for t in range(1, steps) if dev.iterations[t] >= cold[t]]
print(f"warm iterations, steps 1..: {int(dev.iterations[1:].sum())}; cold: {int(cold[1:].sum())}"
      + (f"; the warm start did NOT win at step(s) {worse}" if worse else "; the warm start won at every step"))
print(f"between two solves, median over the steps: device route {np.median(dev.step_ms):.3f} ms, host route {np.median(host.step_ms):.3f} ms")
