"""zdual_cone_kernel against the per-QP z kernels it is modelled on: HIP-event time of the standalone z-update
(admm_profile, unfused mode, residual form) at N = 1000, (6, 3), batch 4096 for
    zdual_kernel, zdual_kernel_2       two plain ADMM_FLAG_UNFUSED handles on the box problem: the control, against itself
    zdual_soc_kernel                   ... on the thrust-ball problem
    hs_shared                          zdual_halfspace_kernel<true, false, false, false> on problems.cw_keepout, the planes of QP 0
    cone_shared, cone_perqp            zdual_cone_kernel<true, false, false, PERQP>: the cones of QP 0 shared by the batch / every
                                       QP its own
    cone_soc_shared, cone_soc_perqp    zdual_cone_kernel<true, false, true, PERQP> on the thrust-ball problem
The cones are cw_approach's recipe about the unconstrained trajectory (problems.lqr_rollout) instead of the plain problem's solution,
which a CPU does not produce at this size: axis along the initial position, apex behind the target, slope 1.05 x the largest r / s of
that trajectory, the last three stages free -- a workload to time the kernel on, not one to solve.
The handles are timed in turn, ROUNDS times over (alternated: a drift of the clocks hits every kernel alike); the figure of a
kernel is the median of its rounds, reported with its minimum and maximum.  One JSON line.  --report also times
Solver.cone_report(multipliers=True) and Solver.set_cone from GPU tensors."""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before the library is loaded, as in tests/test_gpu_device_io.py)
import admm_library_amd as pkg  # noqa: E402
from admm_library_amd import _abi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=1000)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warm", type=int, default=30)
ap.add_argument("--free-tail", type=int, default=3)
ap.add_argument("--report", action="store_true")
a = ap.parse_args()


def with_cones(p, free_tail):
    """p with per-QP cones about its unconstrained trajectory, by cw_approach's recipe."""
    N = p.N
    X = pkg.problems.lqr_rollout(p)[:, :, :3]
    rng0 = np.linalg.norm(p.x0[:, :3], axis=1)
    e = p.x0[:, :3] / rng0[:, None]
    along = np.einsum("bki,bi->bk", X, e)
    apex = -(1.5 * np.maximum(-along.min(axis=1), 0.0) + 0.1 * rng0)[:, None] * e
    dl = X - apex[:, None, :]
    s = np.einsum("bki,bi->bk", dl, e)
    r = np.sqrt(np.maximum(np.sum(dl * dl, axis=2) - s * s, 0.0))
    g = np.repeat((1.05 * (r / s)[:, :N - free_tail].max(axis=1))[:, None], N, axis=1)
    c, ap_ = np.repeat(e[:, None, :], N, axis=1), np.repeat(apex[:, None, :], N, axis=1)
    c[:, N - free_tail:], ap_[:, N - free_tail:], g[:, N - free_tail:] = 0.0, 0.0, 1.0
    return dataclasses.replace(p, cone_c=c, cone_p=ap_, cone_g=g)


box0 = pkg.cw_rendezvous(N=a.N, batch=a.batch)
soc0 = pkg.cw_rendezvous(N=a.N, batch=a.batch, thrust_norm=True)
box, soc = with_cones(box0, a.free_tail), with_cones(soc0, a.free_tail)
keepout = pkg.cw_keepout(N=a.N, batch=a.batch)
shared = lambda p: dict(cone_c=p.cone_c[0].copy(), cone_p=p.cone_p[0].copy(), cone_g=p.cone_g[0].copy())
cases = [("zdual_kernel", box0), ("zdual_kernel_2", box0), ("zdual_soc_kernel", soc0),
         ("hs_shared", dataclasses.replace(keepout, hs_a=keepout.hs_a[0].copy(), hs_b=keepout.hs_b[0].copy())),
         ("cone_shared", dataclasses.replace(box, **shared(box))), ("cone_perqp", box),
         ("cone_soc_shared", dataclasses.replace(soc, **shared(soc))), ("cone_soc_perqp", soc)]
solvers, geometry, active = {}, {}, {}
for name, p in cases:
    s = pkg.Solver(p, pkg.Options(rho=0.5, flags=_abi.FLAG_UNFUSED if p.z_kind is None else 0))
    s.run(a.warm, 1)                      # off the zero state: some cones bind, some do not
    solvers[name], geometry[name] = s, s.geometry()
    if p.z_kind == "cone":
        active[name] = float(s.cone_report().n_active.mean())
times = {name: [] for name in solvers}
for _ in range(a.rounds):
    for name, s in solvers.items():
        times[name].append(1e3 * s.profile(a.iters, residuals=True, fused=False)["zdual_ms"])
extra = {}
if a.report:
    s = solvers["cone_perqp"]
    s.cone_report(multipliers=True)
    t0 = time.perf_counter()
    for _ in range(10):
        s.cone_report(multipliers=True)
    extra["cone_report_call_ms"] = round((time.perf_counter() - t0) * 100.0, 3)
    tc, tp, tg = (torch.as_tensor(x, device="cuda:0") for x in (box.cone_c, box.cone_p, box.cone_g))
    s.set_cone(tc, tp, tg)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        s.set_cone(tc, tp, tg)
    torch.cuda.synchronize()
    extra["set_cone_device_call_ms"] = round((time.perf_counter() - t0) * 100.0, 3)
for s in solvers.values():
    s.close()
med = {k: float(np.median(v)) for k, v in times.items()}
elements = a.N * 9 * a.batch
out = {"N": a.N, "batch": a.batch, "rounds": a.rounds, "zdual_us": {k: round(v, 2) for k, v in med.items()},
       "min_us": {k: round(min(v), 2) for k, v in times.items()}, "max_us": {k: round(max(v), 2) for k, v in times.items()},
       "TBps_at_40B": {k: round(40.0 * elements / (v * 1e-6) / 1e12, 3) for k, v in med.items()},
       "ratio_to_zdual_kernel": {k: round(v / med["zdual_kernel"], 3) for k, v in med.items()},
       "ratio_to_zdual_soc_kernel": {k: round(v / med["zdual_soc_kernel"], 3) for k, v in med.items()},
       "mean_active_stages": active, "geometry": geometry}
out.update(extra)
print(json.dumps(out))
