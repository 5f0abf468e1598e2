"""Time the step between two MPC solves on one handle, three ways, interleaved in one process:

  device   Solver.mpc_advance with dx as a CUDA tensor (admm_mpc_advance_device: finite scan of dx, two kernels)
  torch    the same step from calls that predate it: get_device, a torch shift, update_instances, set_state with CUDA tensors
  numpy    the host route: get, NumPy shift, update_instances, set_state

and the device route alone (no input array: the two kernels, no finite scan) under each chunk count of --chunks
(ADMM_MPC_CHUNKS), with the achieved bytes/s against the algorithmic 16 B per stacked element per array.

  python tools/mpc_time.py [--batch 4096] [--N 1000] [--chunks 0,16,32,64,128] [--out FILE] [--only-device]

Every timing is a host clock around work that ends in a synchronisation of the handle's stream; warm-up runs for --warm seconds
per route, the figure is the median of --repeats."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import admm_library_amd as pkg  # noqa: E402
from admm_library_amd.mpc import plant_step, shift_horizon  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--N", type=int, default=1000)
    ap.add_argument("--chunks", default="0,8,16,32,64,128")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warm", type=float, default=0.5)
    ap.add_argument("--max-iter", type=int, default=600)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-device", action="store_true", help="the device route alone (for a profiler run)")
    a = ap.parse_args()
    import torch
    if pkg.device_count() < 1:
        raise SystemExit("mpc_time.py: no HIP device")
    dev = "cuda:0"
    p = pkg.cw_rendezvous(N=a.N, batch=a.batch)
    n, m, nb = p.n, p.m, p.nb
    rng = np.random.default_rng(0)
    dx = 1e-3 * rng.standard_normal((p.batch, n))
    tdx = torch.from_numpy(dx).to(dev)
    tA, tB = torch.from_numpy(p.A).to(dev), torch.from_numpy(p.B).to(dev)
    res = {"shape": dict(N=a.N, n=n, m=m, batch=a.batch), "repeats": a.repeats}
    with pkg.Solver(p, pkg.Options(rho=0.05, max_iter=a.max_iter)) as s:
        pitch = s.geometry()["pitch"]
        info = s.solve()
        res["solve"] = dict(iters=info.iters_run, converged=info.n_converged, ms=info.solve_ms)
        x0 = [torch.from_numpy(p.x0).to(dev)]

        def device():
            _, x = s.mpc_advance(dx=tdx)
            s.sync()
            x0[0] = x

        def kernels_only():
            s.mpc_advance()
            s.sync()

        def torch_route():
            w, z, y = s.get_device()
            xn = x0[0] @ tA.T + z[:, :m] @ tB.T + tdx
            sh = [torch.cat([t[:, nb:], t[:, -nb:]], dim=1) for t in (w, z, y)]
            s.update_instances(x0=xn)
            s.set_state(*sh)
            s.sync()
            x0[0] = xn

        def numpy_route():
            w, z, y = s.get()
            xn = plant_step(x0[0].cpu().numpy(), z[:, :m], p.A, p.B, dx)
            s.update_instances(xn)
            s.set_state(shift_horizon(w, nb), shift_horizon(z, nb), shift_horizon(y, nb))
            s.sync()
            x0[0] = torch.from_numpy(xn).to(dev)

        def once(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3

        def warm(fn):
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < a.warm:
                fn()

        routes = {"device": device} if a.only_device else {"device": device, "torch": torch_route}
        for fn in routes.values():
            warm(fn)
        times = {k: [] for k in routes}
        for _ in range(a.repeats):                     # interleaved: one of each per round
            for k, fn in routes.items():
                times[k].append(once(fn))
        for k, v in times.items():
            res[k + "_ms"] = dict(median=statistics.median(v), min=min(v), max=max(v))
        if not a.only_device:
            numpy_route()
            v = [once(numpy_route) for _ in range(3)]
            res["numpy_ms"] = dict(median=statistics.median(v), min=min(v), max=max(v))
            res["device_over_torch"] = res["torch_ms"]["median"] / res["device_ms"]["median"]
        # the two kernels alone under each chunk count; bytes: 16 B (one load, one store) per element of w, z, y
        algo_bytes = 16.0 * a.N * nb * pitch * 3
        table = []
        for c in [int(v) for v in a.chunks.split(",")]:
            if c:
                os.environ["ADMM_MPC_CHUNKS"] = str(c)
            else:
                os.environ.pop("ADMM_MPC_CHUNKS", None)
            warm(kernels_only)
            v = [once(kernels_only) for _ in range(a.repeats)]
            med = statistics.median(v)
            table.append(dict(chunks=c or "default", median_ms=med, min_ms=min(v), algorithmic_TBps=algo_bytes / (med * 1e-3) / 1e12))
        os.environ.pop("ADMM_MPC_CHUNKS", None)
        res["chunks"] = table
        res["algorithmic_bytes"] = algo_bytes
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
