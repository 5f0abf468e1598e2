#!/usr/bin/env python3
"""Rendezvous inside an approach cone: one second-order cone per stage on the position rows.

The chaser must stay inside a cone in front of the docking port: with the axis e along the initial line of sight and the apex p a
little behind the target, r <= gamma s for s = e . (x - p) along the axis and r the distance from it.  The cone is convex and its
projection is closed-form, so the handle needs no re-linearisation: only its z-update differs from a plain handle's.

problems.cw_approach builds the workload feasible by construction (the cone holds the plain problem's trajectory with 5 % to spare)
and adds a linear cost across the axis that pulls the trajectory into the cone's surface.  The example solves two workloads on ONE
handle -- the input box, then the thrust ball with the minimum-fuel term: update_problem for the box and the linear cost, set_fuel
for the weight, set_cone for the cones, each between solves -- and prints per QP the iterations, the stages on the surface
(Solver.cone_report), the largest violation of a cone by z and the wall time, then the trajectory's largest off-axis angle against
the half-angle of its cone.

    python examples/approach_cone_rendezvous.py [N] [batch]

Needs the built library and a GPU (python -c "import __graft_entry__ as g; g.build()")."""
import dataclasses
import os
import sys
import time

import numpy as np
import torch   # noqa: F401  (before the library is loaded)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import admm_library_amd as pkg   # noqa: E402

OPTS = dict(rho=0.5, alpha=1.6, eps_abs=1e-7, eps_rel=1e-7, max_iter=4000, check_interval=10, adapt_interval=50, adapt_max=8)
FREE_TAIL = 3


def cone_coordinates(p, z):
    """(coned, s, r): per QP and stage whether it carries a cone, and the coordinates of z's positions along and off the axis."""
    x = z.reshape(p.batch, p.N, p.nb)[:, :, p.m:p.m + 3] - p.cone_p
    nrm = np.linalg.norm(p.cone_c, axis=2)
    coned = nrm > 0
    e = p.cone_c / np.where(coned, nrm, 1.0)[:, :, None]
    s = np.sum(x * e, axis=2)
    r = np.sqrt(np.maximum(np.sum(x * x, axis=2) - s * s, 0.0))
    return coned, s, r


def measure(p, s, verbose):
    """One cold solve of the handle's problem; the row of results."""
    zero = np.zeros((p.batch, p.L))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    info = s.solve(zero, zero)
    rep = s.cone_report()
    _, z, _ = s.get(w=False, y=False)
    ms = (time.perf_counter() - t0) * 1e3
    coned, along, off = cone_coordinates(p, z)
    viol = np.where(coned, np.maximum(off - p.cone_g * along, 0.0) / np.sqrt(1.0 + p.cone_g ** 2), 0.0).max(axis=1)
    angle = np.where(coned, np.arctan2(off, along), 0.0).max(axis=1)
    half = np.arctan(p.cone_g[:, 0])
    row = dict(iters=info.iters.copy(), status=info.status.copy(), n_active=rep.n_active.copy(), max_violation=viol, ms=ms,
               angle=angle, half_angle=half, rho=info.rho)
    if verbose:
        for b in range(p.batch):
            print(f"  QP {b}: {info.iters[b]:5d} iterations{'' if info.status[b] else ' (not converged)'} | {rep.n_active[b]} stages on the "
                  f"surface | largest cone violation of z {viol[b]:.2e}")
        print(f"  {info.iters_run} iterations of the batch, final rho {info.rho:g}, {ms:.1f} ms")
        print(f"  largest off-axis angle / half-angle: " + "  ".join(f"{np.degrees(a):.2f}/{np.degrees(h):.2f}" for a, h in zip(angle, half)) +
              " degrees")
    return row


def run(N=40, batch=6, verbose=True):
    """Both workloads on one handle; returns one dict per workload (per-QP arrays: iters, status, n_active, max_violation, angle,
    half_angle; ms, rho)."""
    box = pkg.cw_approach(N=N, batch=batch, pull=0.05, free_tail=FREE_TAIL)
    fuel = pkg.cw_approach(N=N, batch=batch, pull=0.2, free_tail=FREE_TAIL, fuel=2.0 * np.pi / N)
    rows = []
    # a fuel handle from the start, with weight 0: the weight can be changed on a handle, not added to one
    with pkg.Solver(dataclasses.replace(box, fuel=np.float64(0.0)), pkg.Options(**OPTS)) as s:
        if verbose:
            print(f"N = {N}, batch = {batch}, input box, pull 0.05, last {FREE_TAIL} stages free")
        rows.append(dict(measure(box, s, verbose), workload="box"))
        # the second workload on the same handle: thrust ball and linear cost, the fuel weight, the cones, the first rho
        s.update_problem(dataclasses.replace(fuel, fuel=None, cone_c=None, cone_p=None, cone_g=None))
        s.set_fuel(fuel.fuel)
        s.set_cone(fuel.cone_c, fuel.cone_p, fuel.cone_g)
        s.set_rho(OPTS["rho"])
        if verbose:
            print(f"N = {N}, batch = {batch}, thrust ball and fuel weight {float(fuel.fuel):.4f}, pull 0.2, last {FREE_TAIL} stages free")
        rows.append(dict(measure(fuel, s, verbose), workload="fuel"))
    return rows


if __name__ == "__main__":
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    batch = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    if pkg.device_count() < 1:
        sys.exit("approach_cone_rendezvous.py needs a GPU: the library has no CPU fallback")
    run(N, batch)
