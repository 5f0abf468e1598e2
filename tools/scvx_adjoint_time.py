#!/usr/bin/env python3
"""admm_scvx_adjoint_device alone against a torch route that does the same recursion as N batched mat-vecs, on
one GPU: HIP events on torch's current stream, a warm-up, the median of --reps calls.  Shapes: 4096 x 200 and 64 x 1000 (or
--shape B N).  The inputs are synthetic (A = I + 0.05 randn, the rest randn, controls clipped to the box): the kernel does not
branch on values.  Algorithmic bytes: (63 + 12) 8 per trajectory-stage, i.e. ub, A, B, q read once and nu, primer, grad written
once.  --only-device: the library's call alone (for a `rocprofv3 --kernel-trace --stats` pass of its own)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from admm_library_amd import _abi                    # noqa: E402
from admm_library_amd import scvx as sc              # noqa: E402
from admm_library_amd.solver import _check, _stream, load_library      # noqa: E402

DEV = torch.device("cuda:0")
P = sc.DeviceOuterStep.ptr


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def torch_route(ub, A, Bm, q, lo, hi):
    """The same recursion as N batched mat-vecs (one einsum per stage), then primer, grad, dJdx0, stat and n_bound batched."""
    Bn, N = ub.shape[:2]
    nu = torch.empty((Bn, N, 6), dtype=torch.float64, device=ub.device)
    qx = q[..., 3:]
    nu[:, -1] = -qx[:, -1]
    for k in range(N - 2, -1, -1):
        nu[:, k] = torch.einsum("bji,bj->bi", A[:, k + 1], nu[:, k + 1]) - qx[:, k]
    primer = torch.einsum("bkij,bki->bkj", Bm, nu)
    grad = q[..., :3] - primer
    dJdx0 = -torch.einsum("bji,bj->bi", A[:, 0], nu[:, 0])
    at_lo, at_hi = ub == lo, ub == hi
    v = torch.where(at_lo, (-grad).clamp_min(0.0), torch.where(at_hi, grad.clamp_min(0.0), grad.abs()))
    return nu, primer, grad, dJdx0, v.amax(dim=(1, 2)), (at_lo | at_hi).sum(dim=(1, 2), dtype=torch.int32)


def run(lib, Bn, N, warmup, reps, only_device):
    g = torch.Generator(device=DEV).manual_seed(11)

    def randn(*shape):
        return torch.randn(shape, dtype=torch.float64, device=DEV, generator=g)
    A = torch.eye(6, dtype=torch.float64, device=DEV) + 0.05 * randn(Bn, N, 6, 6)
    Bm, q = 0.1 * randn(Bn, N, 6, 3), randn(Bn, N, 9)
    ub = (3.0 * randn(Bn, N, 3)).clamp(-3.0, 3.0)
    params = _abi.CScvxParams(fd_eps=1e-6, tol=1e-6, rho_reject=0.1, rho_expand=0.7)
    params.u_lo[:], params.u_hi[:] = [-3.0] * 3, [3.0] * 3
    lo, hi = torch.full((3,), -3.0, dtype=torch.float64, device=DEV), torch.full((3,), 3.0, dtype=torch.float64, device=DEV)
    t = dict(nu=torch.empty((Bn, N, 6), dtype=torch.float64, device=DEV), primer=torch.empty_like(ub), grad=torch.empty_like(ub),
             dJdx0=torch.empty((Bn, 6), dtype=torch.float64, device=DEV), stat=torch.empty(Bn, dtype=torch.float64, device=DEV),
             n_bound=torch.empty(Bn, dtype=torch.int32, device=DEV))
    out = _abi.CScvxAdjointOut(**{k: P(v) for k, v in t.items()})

    def call():
        _check(lib, lib.admm_scvx_adjoint_device(0, N, Bn, C.byref(params), P(ub), P(A), P(Bm), P(q), C.byref(out), _stream(DEV)))
    med, lo_ms, hi_ms = timed(call, warmup, reps)
    nbytes = Bn * N * (63 + 12) * 8
    rec = dict(batch=Bn, N=N, call_ms=med, call_ms_min=lo_ms, call_ms_max=hi_ms, algorithmic_MB=nbytes / 1e6,
               achieved_GBps=nbytes / med / 1e6, reps=reps)
    if not only_device:
        ref = torch_route(ub, A, Bm, q, lo, hi)
        torch.cuda.synchronize()
        scale = ref[0].abs().amax()
        rec["max_rel_diff_vs_torch"] = max(float((a - b).abs().max() / scale) for a, b in zip(ref[:4], (t["nu"], t["primer"], t["grad"], t["dJdx0"])))
        rec["n_bound_equal"] = bool(torch.equal(ref[5], t["n_bound"]))
        tm, tlo, thi = timed(lambda: torch_route(ub, A, Bm, q, lo, hi), 1, max(3, reps // 4))
        rec.update(torch_ms=tm, torch_ms_min=tlo, torch_ms_max=thi, speedup=tm / med)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=2, action="append", metavar=("B", "N"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only-device", action="store_true")
    args = ap.parse_args()
    lib = load_library()
    for Bn, N in args.shape or [(4096, 200), (64, 1000)]:
        print(json.dumps(run(lib, Bn, N, args.warmup, args.reps, args.only_device)))


if __name__ == "__main__":
    main()
