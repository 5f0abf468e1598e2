"""zdual_consensus_kernel against the two per-QP z kernels it is modelled on: HIP-event time of the standalone
z-update (admm_profile, unfused mode, residual form) at N = 1000, (6, 3), batch 4096 for
    zdual_kernel       a plain ADMM_FLAG_UNFUSED handle on the box problem
    zdual_soc_kernel   ... on the thrust-bound problem
    consensus          G = 1, 64, 4096 on the box problem, and G = 64 on the thrust-bound problem (--zrows: also with given chunks)
The handles are timed in turn, ROUNDS times over (alternated: a drift of the box's clocks hits every kernel alike); the figure of a
kernel is the median of its rounds.  One JSON line.  --once runs every kernel a few times only (for a rocprofv3 --kernel-trace
pass, which times the kernels itself)."""
import argparse
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import admm_library_amd as pkg  # noqa: E402
from admm_library_amd import _abi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=1000)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--groups", type=int, nargs="*", default=[1, 64, 4096])
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--zrows", type=int, nargs="*", default=[], help="also time every consensus case with these Options.zrows (rows per chunk)")
ap.add_argument("--once", action="store_true")
a = ap.parse_args()

box = pkg.cw_rendezvous(N=a.N, batch=a.batch)
soc = pkg.cw_rendezvous(N=a.N, batch=a.batch, thrust_norm=True)
cases = [("zdual_kernel", box, None), ("zdual_soc_kernel", soc, None)]
cases = [c + (0,) for c in cases]
cases += [(f"consensus_G{G}", box, G, 0) for G in a.groups] + [("consensus_soc_G64", soc, 64, 0)]
cases += [(f"consensus_G{G}_zrows{zr}", box, G, zr) for G in a.groups for zr in a.zrows]
solvers, geometry = {}, {}
for name, p, G, zr in cases:
    if G is None:
        s = pkg.Solver(p, pkg.Options(rho=0.05, flags=_abi.FLAG_UNFUSED))
    else:
        s = pkg.Solver(dataclasses.replace(p, consensus=G), pkg.Options(rho=0.05, zrows=zr))
    s.run(3, 1)
    solvers[name], geometry[name] = s, s.geometry()
rounds = 1 if a.once else a.rounds
times = {name: [] for name in solvers}
for _ in range(rounds):
    for name, s in solvers.items():
        times[name].append(1e3 * s.profile(3 if a.once else a.iters, residuals=True, fused=False)["zdual_ms"])
for s in solvers.values():
    s.close()
med = {k: float(np.median(v)) for k, v in times.items()}
elements = a.N * 9 * a.batch
out = {"N": a.N, "batch": a.batch, "rounds": rounds, "zdual_us": {k: round(v, 2) for k, v in med.items()},
       "min_us": {k: round(min(v), 2) for k, v in times.items()}, "max_us": {k: round(max(v), 2) for k, v in times.items()},
       "TBps_at_40B": {k: round(40.0 * elements / (v * 1e-6) / 1e12, 3) for k, v in med.items()},
       "ratio_to_zdual_kernel": {k: round(v / med["zdual_kernel"], 3) for k, v in med.items()},
       "ratio_to_zdual_soc_kernel": {k: round(v / med["zdual_soc_kernel"], 3) for k, v in med.items()},
       "geometry": geometry}
print(json.dumps(out))
