#!/usr/bin/env python3
"""One thrust profile for a cloud of initial conditions: scenario consensus.

Clohessy-Wiltshire rendezvous from `groups` nominal starts, each dispersed into `group_size` scenarios (insertion errors), under
a radial corridor |x| <= 0.15 km that every scenario must respect.  The burn plan is uplinked once, so all scenarios of a group
fly the SAME controls (Problem.consensus = group_size).  Two comparisons:

  1. with the corridor: the profile planned for the nominal start alone, flown from the dispersed starts, leaves the corridor on
     some scenarios; the consensus profile on none -- the state box holds for each x0, not for their mean;
  2. with the states open: the consensus profile IS the solution for the group's mean x0 (linear dynamics, quadratic cost).

    python examples/robust_rendezvous.py [groups] [group_size]

Runs on the GPU where one is visible (built library: python -c "import __graft_entry__ as g; g.build()"), else on the CPU with
the NumPy reference of the tests (tests/_consensus_ref.py) -- same iteration, same stopping rule."""
import dataclasses
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, d)
import admm_library_amd as pkg   # noqa: E402

groups = int(sys.argv[1]) if len(sys.argv) > 1 else 2
G = int(sys.argv[2]) if len(sys.argv) > 2 else 4
N, SPREAD, CORRIDOR = 12, 0.05, (0.15, np.inf, np.inf)
# consensus wants a larger rho than a single QP: the scenarios' deviations from the shared profile converge at rate
# lambda / (lambda + rho) over the eigenvalues lambda of the condensed Hessian
OPTS = dict(rho=100.0, alpha=1.6, eps_abs=1e-8, eps_rel=1e-8, max_iter=20000, check_interval=10)

try:
    on_gpu = pkg.device_count() > 0
except (OSError, FileNotFoundError):
    on_gpu = False
print("running on", "the GPU" if on_gpu else "the CPU reference (no GPU visible)")


def solve(p):
    """(z, iterations) of the converged batch; consensus groups where p.consensus is set."""
    if on_gpu:
        with pkg.Solver(p, pkg.Options(**OPTS)) as s:
            info = s.solve()
            assert info.status.all(), "not converged"
            return s.get()[1], info.iters_run
    import _consensus_ref as cr
    ref = cr.solve(p, group=p.consensus or 1, **OPTS)
    assert ref.status.all(), "not converged"
    return ref.z, ref.iters_run


def controls(p, z, every=1):
    return z.reshape(p.batch, p.N, p.nb)[::every, :, :p.m]


def fly(p, x0, u):
    """Positions (scenarios, N, 3) of the linear dynamics from x0 under the profile u (N, m)."""
    x, out = x0.copy(), []
    for k in range(p.N):
        x = x @ p.A.T + u[k] @ p.B.T
        out.append(x[:, :3])
    return np.stack(out, axis=1)


def outside(pos):
    """Scenarios that leave the corridor by more than the accuracy of the solve (dynamics defect of the iterate: below 1e-6)."""
    return (np.abs(pos) > np.asarray(CORRIDOR) + 1e-6).any(axis=(1, 2))


cloud = pkg.cw_rendezvous_scenarios(N=N, groups=groups, group_size=G, spread=SPREAD, pos_box=CORRIDOR)
nominal = dataclasses.replace(pkg.cw_rendezvous_scenarios(N=N, groups=groups, group_size=1, spread=0.0, pos_box=CORRIDOR), consensus=None)

print(f"\n1. radial corridor |x| <= {CORRIDOR[0]} km, {groups} groups of {G} scenarios, N = {N}")
z_nom, it_nom = solve(nominal)
z_con, it_con = solve(cloud)
u_nom, u_con = controls(nominal, z_nom), controls(cloud, z_con, every=G)
for g in range(groups):
    x0 = cloud.x0[g * G:(g + 1) * G]
    bad_nom, bad_con = outside(fly(cloud, x0, u_nom[g])), outside(fly(cloud, x0, u_con[g]))
    worst_nom, worst_con = (np.abs(fly(cloud, x0, u)[:, :, 0]).max() for u in (u_nom[g], u_con[g]))
    print(f"   group {g}: nominal profile leaves the corridor on {int(bad_nom.sum())} of {G} scenarios (worst |x| {worst_nom:.4f} km); "
          f"consensus profile on {int(bad_con.sum())} (worst |x| {worst_con:.7f} km)")
print(f"   iterations: nominal {it_nom}, consensus {it_con}; the profiles differ by {np.abs(u_nom - u_con).max():.3e}")

print("\n2. states open: consensus against the solution for the group's mean x0")
open_cloud = pkg.cw_rendezvous_scenarios(N=N, groups=groups, group_size=G, spread=SPREAD)
means = dataclasses.replace(open_cloud, x0=open_cloud.x0.reshape(groups, G, -1).mean(axis=1), consensus=None)
z_open, _ = solve(open_cloud)
z_mean, _ = solve(means)
diff = np.abs(controls(open_cloud, z_open, every=G) - controls(means, z_mean)).max()
print(f"   max |consensus profile - mean-x0 profile| = {diff:.3e}  (both converged to eps = {OPTS['eps_abs']:g})")
