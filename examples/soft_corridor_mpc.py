#!/usr/bin/env python3
"""A receding-horizon loop that survives an infeasible window: soft constraints.

Clohessy-Wiltshire station keeping inside a radial corridor |x| <= 0.25 km, a window of N steps solved again at every step from
the shifted solution (admm_library_amd.mpc_batch on one persistent handle), under a radial push at every step that the thrusters
cannot take back.  After a few steps the measured state lies outside the corridor, and the window's QP has no solution:

  hard corridor   the infeasibility probe (Solver.infeasibility) flags the window's QP; the iterate the loop goes on flying is
                  not a solution of anything
  soft corridor   Problem.soft puts the price `weight` per km on leaving the corridor; the same loop flies on, every window
                  converges, and Solver.soft_report() gives the violation and the penalty paid at every step

    python examples/soft_corridor_mpc.py [steps] [batch] [weight]

Runs on the GPU where one is visible (built library: python -c "import __graft_entry__ as g; g.build()"), else on the CPU with
the NumPy references of the tests (tests/_soft_ref.py, tests/_infeas_ref.py) -- same iteration, same stopping rule, same probe."""
import dataclasses
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, d)
import admm_library_amd as pkg   # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 12
batch = int(sys.argv[2]) if len(sys.argv) > 2 else 8
weight = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0
N, SPAN, EPS = 20, 10, 1e-6
OPTS = dict(rho=0.5, alpha=1.6, eps_abs=1e-6, eps_rel=1e-6, max_iter=4000, check_interval=10)

try:
    on_gpu = pkg.device_count() > 0
except (OSError, FileNotFoundError):
    on_gpu = False
print("running on", "the GPU" if on_gpu else "the CPU references (no GPU visible)")

hard, dx = pkg.cw_corridor_mpc(N=N, batch=batch)
soft, _ = pkg.cw_corridor_mpc(N=N, batch=batch, soft=weight)
dx = dx[:steps]
rows = {"hard": [], "soft": []}


def loop(name, p):
    """The closed loop on p; per step: QPs converged, QPs the probe flags (hard) or violation and penalty (soft)."""
    if on_gpu:
        def on_step(t, s, info):
            if name == "hard":
                rows[name].append((info.iters_run, info.n_converged, int(s.infeasibility(span=SPAN, eps=EPS).infeasible.sum())))
            else:
                rep = s.soft_report()
                rows[name].append((info.iters_run, info.n_converged, float(rep.max_violation.max()), float(rep.penalty.max()), int(rep.n_violated.max())))
        return pkg.mpc_batch(p, steps, pkg.Options(**OPTS), noise=(None, dx), on_step=on_step)
    import _infeas_ref as ir
    import _soft_ref as sr

    def qp(cur, z0, y0):
        r = sr.solve(cur, z0=z0, y0=y0, **OPTS)
        if name == "hard":      # the probe: SPAN more iterations from the iterate, the drift of the dual over them
            more = sr.solve(cur, z0=r.z, y0=r.y, **dict(OPTS, max_iter=SPAN, eps_abs=0, eps_rel=0), stop=False)
            flags = ir.probe(cur, r.y, more.y, SPAN, EPS)["infeasible"]
            rows[name].append((r.iters_run, int(r.status.sum()), int(flags.sum())))
            r = more
        else:
            pen, mx, cnt = sr.report(cur, r.z)
            rows[name].append((r.iters_run, int(r.status.sum()), float(mx.max()), float(pen.max()), int(cnt.max())))
        return r.w, r.z, r.y, r.iters_run, int(r.status.sum())
    return pkg.mpc_batch(p, steps, noise=(None, dx), qp_solver=qp)


res_h, res_s = loop("hard", hard), loop("soft", soft)
print(f"\nradial corridor |x| <= {hard.hi[3]} km, window N = {N}, {batch} scenarios, weight {weight} per km, {steps} steps")
print(" step | worst |x0| (km) | hard: iterations converged flagged | soft: iterations converged  violation (km)  penalty  rows")
for t in range(steps):
    h, s = rows["hard"][t], rows["soft"][t]
    print(f"  {t:3d} |     {np.abs(res_s.X[t, :, 0]).max():8.4f}    |      {h[0]:6d}     {h[1]:3d}/{batch}   {h[2]:3d}/{batch}    |"
          f"      {s[0]:6d}     {s[1]:3d}/{batch}      {s[2]:9.5f}  {s[3]:9.5f}  {s[4]:3d}")
first = next((t for t in range(steps) if rows["hard"][t][2] > 0), None)
print("\nhard corridor:", "never flagged" if first is None else f"the probe flags a window at step {first}; from there on the loop has nothing to fly")
print(f"soft corridor: {sum(r[1] == batch for r in rows['soft'])} of {steps} windows converged on every scenario; "
      f"largest violation {max(r[2] for r in rows['soft']):.4f} km")
if on_gpu:
    # the same loop with the step written out on the host (get, NumPy shift, update_instances, set_state): the "before" of mpc_advance
    res_host = pkg.mpc_batch(soft, steps, pkg.Options(**OPTS), noise=(None, dx), on_device=False)
    print(f"per step, soft handle (medians): solve {np.median(res_s.solve_ms):.2f} ms; apply + propagate + shift on the device "
          f"{np.median(res_s.step_ms):.3f} ms, on the host route {np.median(res_host.step_ms):.3f} ms; "
          f"the two routes' states differ by {np.abs(res_host.X - res_s.X).max():.1e}")
