#!/usr/bin/env python3
"""Rendezvous around a keep-out sphere: one tangent half-space per stage, re-linearised on one handle.

A keep-out sphere |r| >= R about the target is not convex.  Its standard convexification is, per stage, the half-space tangent to
the sphere at the point below the previous trajectory, n_k . r_{k+1} >= R with n_k = r_prev / |r_prev|.  The Clohessy-Wiltshire
dynamics are linear, so the loop needs no new dynamics and no new factor: one persistent handle, and per pass

    solve            Solver.solve from the handle's state, the previous pass' (z, y): a warm start
    get_device       the positions of the solution, as a tensor on the GPU
    planes           a = -n, b = -R, by torch on the GPU; the last `free_tail` stages carry none (the final approach)
    set_halfspace    the new planes into the handle, from GPU memory

The first pass' planes are about the unconstrained trajectory, which runs straight through the target (problems.cw_keepout).
Per pass the example prints the closest approach of the worst QP over the constrained stages, relative to R, the active stages
(Solver.halfspace_report: stages with a positive multiplier), the iterations and the wall time.  It runs the loop twice: with
the input box, and with the thrust ball and the minimum-fuel term.

    python examples/keepout_rendezvous.py [N] [batch] [passes]

On an MI355X at N = 40, batch 6, 4 passes: 4000 / 2100 / 1750 / 1290 iterations with the input box, closest approach 1.00001 -
1.0007 R; 4000 / 1520 / 950 / 4000 with the thrust ball and the fuel term, 1.00002 - 1.0013 R (the run
at N = 1000, batch 4096 has not been measured).

Needs the built library and a GPU (python -c "import __graft_entry__ as g; g.build()")."""
import os
import sys
import time

import numpy as np
import torch   # (before the library is loaded)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import admm_library_amd as pkg   # noqa: E402

OPTS = dict(rho=0.5, eps_abs=1e-7, eps_rel=1e-7, max_iter=4000, check_interval=10)
FREE_TAIL = 5


def planes_on_device(z, N, nb, m, radius, free_tail):
    """(a, b) of the tangent half-spaces about the positions in z (batch, L), a CUDA tensor: a = -r / |r|, b = -R; a = 0, b = 0 on
    the last free_tail stages and wherever r = 0."""
    r = z.view(z.shape[0], N, nb)[:, :, m:m + 3]
    nrm = torch.linalg.vector_norm(r, dim=2, keepdim=True)
    ok = nrm > 0
    a = torch.where(ok, -r / torch.where(ok, nrm, torch.ones_like(nrm)), torch.zeros_like(r))
    b = torch.where(ok[:, :, 0], torch.full_like(nrm[:, :, 0], -radius), torch.zeros_like(nrm[:, :, 0]))
    if free_tail > 0:
        a[:, N - free_tail:] = 0.0
        b[:, N - free_tail:] = 0.0
    return a.contiguous(), b.contiguous()


def run(N=40, batch=6, passes=4, fuel=None, verbose=True):
    """The re-linearisation loop; returns (radius, rows) with one row per pass: closest approach over the constrained stages per QP
    (NumPy, batch), active stages per QP, iterations, QPs converged, wall time in ms."""
    p = pkg.cw_keepout(N=N, batch=batch, free_tail=FREE_TAIL, fuel=fuel)
    radius = float(-p.hs_b[0, 0])
    rows = []
    with pkg.Solver(p, pkg.Options(**OPTS)) as s:
        for ps in range(passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = s.solve()                           # from the handle's state: zero at first, then the previous pass' (z, y)
            _, z, _ = s.get_device(w=False, y=False)
            a, b = planes_on_device(z, N, p.nb, p.m, radius, FREE_TAIL)
            rep = s.halfspace_report()
            if ps + 1 < passes:
                s.set_halfspace(a, b)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            r = z.view(batch, N, p.nb)[:, :N - FREE_TAIL, p.m:p.m + 3]
            closest = torch.linalg.vector_norm(r, dim=2).min(dim=1).values.cpu().numpy()
            rows.append((closest, rep.n_active.copy(), info.iters_run, info.n_converged, ms))
            if verbose:
                print(f"  pass {ps}: closest approach / R  min {closest.min() / radius:.6f}  max {closest.max() / radius:.6f} | "
                      f"active stages {rep.n_active.min()} .. {rep.n_active.max()} | {info.iters_run} iterations, "
                      f"{info.n_converged}/{batch} converged | {ms:.1f} ms")
    return radius, rows


if __name__ == "__main__":
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    batch = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    passes = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    if pkg.device_count() < 1:
        sys.exit("keepout_rendezvous.py needs a GPU: the library has no CPU fallback")
    for fuel in (None, 2.0 * np.pi / N):
        print(f"N = {N}, batch = {batch}, keep-out sphere of half the smallest initial range, last {FREE_TAIL} stages free, " +
              ("input box" if fuel is None else f"thrust ball and fuel weight {fuel:.4f}"))
        run(N, batch, passes, fuel)
