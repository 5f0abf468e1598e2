#!/usr/bin/env python3
"""Costates, primer vector and the optimality certificate of a NONLINEAR trajectory (needs an MI355X).

The scenario of examples/scvx_rendezvous.py (a chaser 150 km behind and 30 km out of plane of its target, one orbit, a 3 km n^2
thrust box) is solved by successive convexification with certify=True.  The loop's own `converged` is a trust-region heuristic;
the certificate is the discrete adjoint of the nonlinear cost at the returned trajectory:
  * stat, the largest violation of first-order optimality over the control components in their box, at the start (u = 0) and at
    the end, and how many components sit on a bound;
  * Lawden's condition on the nonlinear solution: interior components satisfy R u = primer to within stat, bounded ones carry the
    primer's sign;
  * dJ/dx0, the reaction of the cost to the insertion error, against a central difference over one component.

    python examples/scvx_primer_vector.py [--outer-on-device] [--model crtbp|elliptic] [N]

--outer-on-device: the loop runs in the HIP kernels of DeviceOuterStep and the certificate comes from admm_scvx_adjoint_device.
--model: the Earth-Moon L2 acquisition of examples/scvx_cislunar.py, or the eccentric chief of examples/scvx_elliptic_rendezvous.py."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from admm_library_amd import scvx as sc               # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("N", type=int, nargs="?", default=None)
ap.add_argument("--outer-on-device", action="store_true")
ap.add_argument("--model", choices=("crtbp", "elliptic"), default=None)
args = ap.parse_args()

if args.model is None:
    N = args.N or 200
    dt = 2 * np.pi / N
    Q = np.diag([1, 1, 1, .1, .1, .1]) * dt * 1e-3
    model, u_max = None, 3.0
    x0 = np.array([10.0, 150.0, 30.0, 0.0, -15.0, 0.0])    # km, km * mean motion
    kw = dict(tr_u=1.0, tr_x=100.0, max_outer=25, tol=1e-7)
else:
    N = args.N or 40
    dt = 2.0 / N
    Q = np.diag([1, 1, 1, .1, .1, .1]) * dt
    if args.model == "crtbp":
        mu = sc.MU_EARTH_MOON
        model, u_max = sc.crtbp(mu, sc.crtbp_collinear_point(mu, 2)), 0.5
        x0 = np.array([0.03, -0.03, 0.015, 0.0, 0.0, 0.0])
    else:
        model, u_max = sc.relative_elliptic(7000.0, 0.3, 0.4), 60.0
        x0 = 0.3 * np.array([10.0, 150.0, 30.0, 0.0, -15.0, 0.0])
    kw = dict(max_outer=20, tol=1e-6)
R = np.eye(3) * dt * 0.05
QN = np.diag([50., 50, 50, 20, 20, 20])
problem = (dt, Q, R, QN, -u_max, u_max)


def cost(x0_, u):
    return sc.trajectory_cost(sc.rollout(x0_, u, dt, model=model), u, Q, R, QN)


u0 = np.zeros((N, 3))
start = sc.adjoint(x0, u0, sc.rollout(x0, u0, dt, model=model), *problem, model=model)
if args.outer_on_device:
    res = sc.scvx_batch(x0[None], N, *problem, linearise_on="cuda:0", outer_on_device=True, model=model, certify=True, **kw)[0]
else:
    res = sc.scvx(x0, N, *problem, model=model, certify=True, **kw)
c = res.certificate
print(f"scvx ({'device' if args.outer_on_device else 'host'} loop, model {args.model or 'relative_circular'}): {res.outer_iterations} outer "
      f"iterations, converged={res.converged}, cost {res.cost:.6g}")
print(f"stat: {start.stat:.4g} at u = 0  ->  {c.stat:.3e} at the solution ({c.stat / start.stat:.1e} of the start); "
      f"{c.n_bound} of {3 * N} control components on a bound")

inside = np.abs(res.u) < u_max
lawden = np.abs((res.u @ R.T - c.primer)[inside]).max() if inside.any() else 0.0
bounded = ~inside & (np.abs(c.grad) > c.stat)
agree = int((np.sign(res.u[bounded]) == np.sign(c.primer[bounded])).sum())
print(f"Lawden: max |R u - primer| over the {int(inside.sum())} interior components {lawden:.3e} (<= stat: {lawden <= c.stat}); "
      f"{agree} of {int(bounded.sum())} bounded components with |grad| > stat carry the primer's sign")
k = int(np.abs(c.primer).sum(axis=1).argmax())
print(f"primer vector: largest at stage {k}: {np.array2string(c.primer[k], precision=4)}, u there {np.array2string(res.u[k], precision=4)}")

j = int(np.abs(c.dJdx0).argmax())
h = 1e-6 * max(1.0, abs(x0[j]))
e = np.zeros(6)
e[j] = h
fd = (cost(x0 + e, res.u) - cost(x0 - e, res.u)) / (2 * h)
print(f"dJ/dx0: {np.array2string(c.dJdx0, precision=5)}")
print(f"  component {j}: adjoint {c.dJdx0[j]:.8g}, central difference (h = {h:.1e}) {fd:.8g}, relative difference "
      f"{abs(fd - c.dJdx0[j]) / abs(fd):.1e}")
