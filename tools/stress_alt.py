"""Stress of the iteration paths on a GPU box (STRESS_FLAGS=1: random option flags too; default: the
alternating path only): seeded random problems over the
compiled (n, m) set, with / without q, box or thrust-magnitude bound, many rho -- more iterations and far
more draws than the unit tests -- against the C oracle.  Prints the error distribution.

    python tools/stress_alt.py [seed] [trials] [--long]

--long: the long-run regime of DESIGN.md §4.8 instead -- cw_rendezvous at N = 1000, 80 ... 400 iterations, rho 0.05 ... 32 (handles
whose forward form fails its host gate run the plain kernels and are counted as such).  There the error of the alternating path
is reported apart for the stages below 16, where the forward form's early-stage gains let it drift past 1e-10, and for the stages
from 64 on, where 1e-10 holds at any count: a FAIL is a trial above 1e-10 on the latter, or anywhere on a plain handle."""
import os, sys, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np
import admm_library_amd as pkg
import oracle_c as oc

dims = [(1, 1), (2, 1), (2, 2), (3, 1), (3, 2), (4, 1), (4, 3), (5, 2), (6, 1), (6, 3), (6, 4), (7, 3), (8, 2), (8, 4),
        (9, 3), (10, 2), (10, 4), (12, 3), (12, 4), (12, 6)]
LONG = "--long" in sys.argv
argv = [a for a in sys.argv[1:] if a != "--long"]
rng = np.random.default_rng(int(argv[0]) if len(argv) > 0 else 7)
trials = int(argv[1]) if len(argv) > 1 else (40 if LONG else 300)
worst, alt_on, errs, early = (0.0, None), 0, [], []
for trial in range(trials):
    n, m = dims[rng.integers(len(dims))]
    N = int(rng.integers(1, 160))
    batch = int(rng.choice([511, 1025, 2049, 4096, 4160]) if os.environ.get("STRESS_BIG") else rng.choice([1, 3, 64, 65, 130, 300]))
    segs = int(rng.choice([0, 0, 1, 2, 3, 5, 8, 13]))
    alpha = float(rng.choice([1.0, 1.0, 1.5]))
    with_q = bool(rng.integers(2))
    soc = bool(rng.integers(4) == 0)
    rho = float(rng.choice([0.02, 0.1, 0.5, 2.0, 8.0]))
    iters = int(rng.choice([3, 8, 17, 40]))
    flags = int(rng.choice([0, 0, 0, 8, 2, 16, 4, 6, 24])) if os.environ.get("STRESS_FLAGS") else 0
    if LONG:
        batch, segs, with_q = int(rng.choice([1, 3, 64, 70])), int(rng.choice([0, 0, 1, 16, 64])), False
        rho = float(rng.choice([0.05, 0.2, 0.8, 1.5, 2.0, 8.0, 16.0, 32.0]))
        iters = int(rng.choice([80, 120, 200, 400]))
        p = pkg.cw_rendezvous(N=1000, batch=batch, seed0=500 + trial, thrust_norm=soc)
    elif rng.integers(3) == 0:
        p = pkg.cw_rendezvous(N=max(N, 8) * 4, batch=batch, seed0=500 + trial, thrust_norm=soc)
    else:
        p = pkg.random_ltv(N=N, n=n, m=m, batch=batch, seed=3000 + trial, with_q=with_q, state_bounds=bool(rng.integers(2)),
                           thrust_norm=soc)
    ref = oc.solve(p, rho=rho, alpha=alpha, max_iter=iters, check_interval=1, eps_abs=0, eps_rel=0, stop=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore" if LONG else "default", RuntimeWarning)      # (--long: the gate's fallback is counted through path())
        s = pkg.Solver(p, pkg.Options(rho=rho, alpha=alpha, segments=segs, flags=flags))
    with s:
        on = s.path()["alternating"]
        s.set_state(z=np.zeros((p.batch, p.L)), y=np.zeros((p.batch, p.L)))
        s.run(iters, residual_every=int(rng.choice([0, 1, 4])))
        w, z, y = s.get()
    e = max(np.abs(a - b).max() / max(1.0, np.abs(b).max()) for a, b in ((w, ref["w"]), (z, ref["z"]), (y, ref["y"])))
    alt_on += on
    if LONG and on:      # the drift of the first stages is the form's (§4.8): judged on the stages past the early-gain zone
        split = lambda k0, k1: max((np.abs(a - b).reshape(p.batch, p.N, p.nb)[:, k0:k1].max() / max(1.0, np.abs(b).max()))
                                   for a, b in ((w, ref["w"]), (z, ref["z"]), (y, ref["y"])))
        early.append((split(0, 16), rho, iters))
        e = split(64, p.N)
    errs.append(e)
    if e > worst[0]:
        worst = (e, dict(trial=trial, name=p.name, n=p.n, m=p.m, N=p.N, batch=batch, segs=segs, alpha=alpha, rho=rho, q=p.q is not None,
                         soc=soc, iters=iters, alt=on, flags=flags))
    if e > 1e-10:
        print("FAIL", e, worst[1], flush=True)
errs = np.array(errs)
print(f"{trials} trials, alternating path on in {alt_on}; relative error max {errs.max():.2e}, 99th pct {np.percentile(errs, 99):.2e}, "
      f"median {np.median(errs):.2e}; > 1e-11: {(errs > 1e-11).sum()}, > 1e-10: {(errs > 1e-10).sum()}")
print("worst:", worst)
if early:
    print("alternating handles, stages < 16 (the drift of DESIGN.md §4.8): max %.2e at rho = %g after %d iterations; > 1e-10: %d of %d"
          % (max(early) + (sum(x[0] > 1e-10 for x in early), len(early))))
