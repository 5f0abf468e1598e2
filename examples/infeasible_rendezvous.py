#!/usr/bin/env python3
"""Telling "has no solution" from "not converged yet": the on-device infeasibility probe.

A batch of Clohessy-Wiltshire rendezvous QPs with the terminal state pinned to the origin and the thrust box |u_i| <= u_max; the
initial states are one draw scaled from easy to hopeless, so the far ones cannot reach the origin within the horizon.  Every 200
iterations the handle is asked for a Farkas certificate per QP (Solver.infeasibility: 190 plain iterations, then 10 inside the
probe); a flagged QP is PROVEN infeasible -- whatever the state of the iteration -- and is dropped.  The rest is solved.

    python examples/infeasible_rendezvous.py [batch] [horizon]

Needs an MI355X and the built library (python -c "import __graft_entry__ as g; g.build()")."""
import dataclasses
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import admm_library_amd as pkg   # noqa: E402

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 16
N = int(sys.argv[2]) if len(sys.argv) > 2 else 16
EVERY, SPAN, ROUNDS = 200, 10, 10

p = pkg.cw_rendezvous(N=N, batch=batch)
scale = np.geomspace(0.01, 30.0, batch)
lo, hi = np.tile(p.lo, (N, 1)), np.tile(p.hi, (N, 1))
lo[-1, p.m:] = hi[-1, p.m:] = 0.0                         # x_N = 0
problem = dataclasses.replace(p, x0=p.x0[:1] * scale[:, None], lo=lo, hi=hi)

proven = np.zeros(batch, np.int64)                        # iteration at which a QP was proven infeasible (0: not)
with pkg.Solver(problem, pkg.Options(rho=1.0)) as s:
    for r in range(1, ROUNDS + 1):
        s.run(EVERY - SPAN)
        probe = s.infeasibility(span=SPAN, eps=1e-6)
        new = (probe.infeasible == 1) & (proven == 0)
        proven[new] = r * EVERY
        print(f"iteration {r * EVERY}: {int((proven > 0).sum())} of {batch} QPs proven infeasible"
              + (f" (new: {np.flatnonzero(new).tolist()})" if new.any() else ""))
        if not new.any() and r > 1:
            break
for b in range(batch):
    tag = f"proven infeasible after {proven[b]} iterations" if proven[b] else "no certificate: kept"
    print(f"  QP {b:2d}: |x0| scaled by {scale[b]:7.3f}   sep {probe.sep[b]:+9.3g}   drift {probe.drift[b]:.2e}   {tag}")

keep = proven == 0
if keep.any():
    rest = dataclasses.replace(problem, x0=np.ascontiguousarray(problem.x0[keep]))
    with pkg.Solver(rest, pkg.Options(rho=1.0, max_iter=20000, check_interval=10)) as s:
        info = s.solve()
    print(f"the other {int(keep.sum())} QPs: {info.n_converged} converged in {info.iters_run} iterations "
          f"(max r {info.max_r:.2e}, max s {info.max_s:.2e})")
