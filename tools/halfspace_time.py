"""zdual_halfspace_kernel against the two per-QP z kernels it is modelled on: HIP-event time of the standalone
z-update (admm_profile, unfused mode, residual form) at N = 1000, (6, 3), batch 4096 for
    zdual_kernel, zdual_kernel_2     two plain ADMM_FLAG_UNFUSED handles on the box problem: the control, against itself
    zdual_soc_kernel                 ... on the thrust-ball problem
    hs_shared, hs_perqp              zdual_halfspace_kernel<true, false, false, PERQP> on problems.cw_keepout, the planes of QP 0
                                     shared by the batch / every QP its own
    hs_soc_shared, hs_soc_perqp      zdual_halfspace_kernel<true, false, true, PERQP> on cw_keepout(thrust_norm=True)
The handles are timed in turn, ROUNDS times over (alternated: a drift of the clocks hits every kernel alike); the figure of a
kernel is the median of its rounds, reported with its minimum and maximum.  One JSON line.  --report also times
Solver.halfspace_report(multipliers=True) and Solver.set_halfspace from GPU tensors."""
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
ap.add_argument("--report", action="store_true")
a = ap.parse_args()

box = pkg.cw_keepout(N=a.N, batch=a.batch)
soc = pkg.cw_keepout(N=a.N, batch=a.batch, thrust_norm=True)
plain = dict(hs_a=None, hs_b=None)
shared = lambda p: dict(hs_a=p.hs_a[0].copy(), hs_b=p.hs_b[0].copy())
cases = [("zdual_kernel", dataclasses.replace(box, **plain)), ("zdual_kernel_2", dataclasses.replace(box, **plain)),
         ("zdual_soc_kernel", dataclasses.replace(soc, **plain)),
         ("hs_shared", dataclasses.replace(box, **shared(box))), ("hs_perqp", box),
         ("hs_soc_shared", dataclasses.replace(soc, **shared(soc))), ("hs_soc_perqp", soc)]
solvers, geometry, active = {}, {}, {}
for name, p in cases:
    s = pkg.Solver(p, pkg.Options(rho=0.5, flags=_abi.FLAG_UNFUSED if p.hs_a is None else 0))
    s.run(a.warm, 1)                      # off the zero state: some planes bind, some do not
    solvers[name], geometry[name] = s, s.geometry()
    if p.hs_a is not None:
        active[name] = float(s.halfspace_report().n_active.mean())
times = {name: [] for name in solvers}
for _ in range(a.rounds):
    for name, s in solvers.items():
        times[name].append(1e3 * s.profile(a.iters, residuals=True, fused=False)["zdual_ms"])
extra = {}
if a.report:
    s = solvers["hs_perqp"]
    s.halfspace_report(multipliers=True)
    t0 = time.perf_counter()
    for _ in range(10):
        s.halfspace_report(multipliers=True)
    extra["halfspace_report_call_ms"] = round((time.perf_counter() - t0) * 100.0, 3)
    ta, tb = torch.as_tensor(box.hs_a, device="cuda:0"), torch.as_tensor(box.hs_b, device="cuda:0")
    s.set_halfspace(ta, tb)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        s.set_halfspace(ta, tb)
    torch.cuda.synchronize()
    extra["set_halfspace_device_call_ms"] = round((time.perf_counter() - t0) * 100.0, 3)
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
