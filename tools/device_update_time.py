#!/usr/bin/env python3
"""admm_update_problem from host arrays vs from GPU memory (a DeviceProblem: admm_update_problem_device), per-instance dynamics
and box at 4096 x 1000 stages, the two forms alternating on ONE handle in one process; then examples/scvx_batch_rendezvous.py
4096 200 with --device-data (both paths, solver-call time of each).  DESIGN.md §4.10.

    python tools/device_update_time.py [reps=3] [--no-example]"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import admm_library_amd as pkg  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
REPS = int(args[0]) if args else 3
N, BATCH = 1000, 4096

for make in (pkg.cw_formation_instances, pkg.cw_rendezvous_instances):
    p = make(N=N, batch=BATCH)
    dp = pkg.DeviceProblem.from_problem(p, "cuda:0")
    torch.cuda.synchronize()
    gb = (p.A.nbytes + p.B.nbytes + p.lo.nbytes + p.hi.nbytes + (0 if p.q is None else p.q.nbytes)) / 1e9
    with pkg.Solver(p, pkg.Options(rho=0.05)) as s:
        s.iterate(3)
        t = {"host": [], "device": []}
        c = {"host": [], "device": []}
        for _ in range(REPS):
            for form, prob in (("host", p), ("device", dp)):
                s.sync()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s.update_problem(prob)
                s.sync()
                t[form].append((time.perf_counter() - t0) * 1e3)
                c[form].append(s.last_update_ms)
        w_h, w_d = min(t["host"]), min(t["device"])
        print(f"(n, m) = ({p.n}, {p.m}), {BATCH} x {N}, per-instance dynamics + box ({gb:.1f} GB of A, B, box, q): "
              f"update_problem host arrays {w_h:.1f} ms (C call {min(c['host']):.1f} ms), "
              f"DeviceProblem {w_d:.1f} ms (C call {min(c['device']):.1f} ms); {w_h / w_d:.1f}x  "
              f"[all: host {' '.join('%.0f' % x for x in t['host'])}, device {' '.join('%.0f' % x for x in t['device'])}]", flush=True)
    del p, dp
    torch.cuda.empty_cache()

if "--no-example" not in sys.argv:
    cmd = [sys.executable, os.path.join(ROOT, "examples", "scvx_batch_rendezvous.py"), "4096", "200", "--device-data"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    print("examples/scvx_batch_rendezvous.py 4096 200 --device-data:\n" + r.stdout + r.stderr[-2000:], flush=True)
    sys.exit(r.returncode)
