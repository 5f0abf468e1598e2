"""zdual_soft_kernel against the two per-QP z kernels it is modelled on: HIP-event time of the standalone
z-update (admm_profile, unfused mode, residual form) at N = 1000, (6, 3), batch 4096 for
    zdual_kernel       a plain ADMM_FLAG_UNFUSED handle on the box problem
    zdual_soc_kernel   ... on the thrust-bound problem
    soft               zdual_soft_kernel<true, false, false>: the box problem with a finite weight on the position rows
    soft_soc           zdual_soft_kernel<true, false, true>: the thrust-bound problem with the same weights
    soft_inf, soft_soc_inf   the same kernels with every weight +inf (the select always takes the clip)
The handles are timed in turn, ROUNDS times over (alternated: a drift of the box's clocks hits every kernel alike); the figure of a
kernel is the median of its rounds, reported with its minimum and maximum.  One JSON line.  --once runs every kernel a few times
only (for a rocprofv3 --kernel-trace pass, which times the kernels itself).  --report also times Solver.soft_report()."""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import admm_library_amd as pkg  # noqa: E402
from admm_library_amd import _abi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=1000)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--weight", type=float, default=0.5)
ap.add_argument("--once", action="store_true")
ap.add_argument("--report", action="store_true")
a = ap.parse_args()

box = pkg.cw_rendezvous(N=a.N, batch=a.batch)
soc = pkg.cw_rendezvous(N=a.N, batch=a.batch, thrust_norm=True)
# a position corridor inside the open solution's excursion, soft: rows on both sides of the select
lo, hi = box.lo.copy(), box.hi.copy()
lo[3:6], hi[3:6] = -0.15, 0.15
sw = np.full(9, np.inf)
sw[3:6] = a.weight
cases = [("zdual_kernel", dataclasses.replace(box, lo=lo, hi=hi), None), ("zdual_soc_kernel", dataclasses.replace(soc, lo=np.r_[soc.lo[:3], lo[3:]], hi=np.r_[soc.hi[:3], hi[3:]]), None)]
cases += [("soft", cases[0][1], sw), ("soft_soc", cases[1][1], sw), ("soft_inf", cases[0][1], np.full(9, np.inf)), ("soft_soc_inf", cases[1][1], np.full(9, np.inf))]
solvers, geometry = {}, {}
for name, p, w in cases:
    if w is None:
        s = pkg.Solver(p, pkg.Options(rho=0.05, flags=_abi.FLAG_UNFUSED))
    else:
        s = pkg.Solver(dataclasses.replace(p, soft=w), pkg.Options(rho=0.05))
    s.run(3, 1)
    solvers[name], geometry[name] = s, s.geometry()
rounds = 1 if a.once else a.rounds
times = {name: [] for name in solvers}
for _ in range(rounds):
    for name, s in solvers.items():
        times[name].append(1e3 * s.profile(3 if a.once else a.iters, residuals=True, fused=False)["zdual_ms"])
report_ms = None
if a.report:
    s = solvers["soft"]
    s.soft_report()
    t0 = time.perf_counter()
    for _ in range(10):
        rep = s.soft_report()
    report_ms = (time.perf_counter() - t0) * 100.0
    violated = int((rep.n_violated > 0).sum())
for s in solvers.values():
    s.close()
med = {k: float(np.median(v)) for k, v in times.items()}
elements = a.N * 9 * a.batch
out = {"N": a.N, "batch": a.batch, "rounds": rounds, "weight": a.weight, "zdual_us": {k: round(v, 2) for k, v in med.items()},
       "min_us": {k: round(min(v), 2) for k, v in times.items()}, "max_us": {k: round(max(v), 2) for k, v in times.items()},
       "TBps_at_40B": {k: round(40.0 * elements / (v * 1e-6) / 1e12, 3) for k, v in med.items()},
       "ratio_to_zdual_kernel": {k: round(v / med["zdual_kernel"], 3) for k, v in med.items()},
       "ratio_to_zdual_soc_kernel": {k: round(v / med["zdual_soc_kernel"], 3) for k, v in med.items()},
       "geometry": geometry}
if report_ms is not None:
    out["soft_report_call_ms"] = round(report_ms, 3)
    out["qps_with_a_violation"] = violated
print(json.dumps(out))
