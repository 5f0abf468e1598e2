"""Cases and helpers of the long-run drift tests of the alternating path: tests/test_alt_drift_host.py pins the
inputs on the CPU, tests/test_gpu_alt_drift.py runs the kernels.

The forward-elimination form of the x-update loses accuracy in the controls of the first stages of the horizon (backward gains
Kb_k of 2.5e4 at k = 0 on the N = 1000 rendezvous), and on that problem ADMM contracts what it loses slowly: the error of the
alternating iteration against the Riccati loop GROWS with the iteration count at rho >= 0.2.  Errors are therefore split into the
stages below EARLY (where the drift sits) and the stages from LATE on (where none is), and the first are held to the NumPy emulation
of the same iteration from the library's own host records (_segmented.alternating_loop), not to an absolute figure."""
import dataclasses
import functools
import json
import os

import numpy as np

import admm_library_amd as pkg
import oracle_c as oc
from admm_library_amd.solver import host_factor
from _segmented import alternating_loop

CHECKPOINTS = (8, 16, 40, 80, 120, 200, 400)      # the GPU tier's
HOST_CHECKPOINTS = (8, 16, 40, 80, 120)           # the part of them the CPU tier re-derives
EARLY, LATE = 16, 64                              # stages < EARLY: the early-gain zone; stages >= LATE: past it
TOL = 1e-10                                       # the project's tolerance on fp64 iterates
FRESH = 16                                        # iterations from a fresh handle through which TOL holds on every stage
EMU_QPS = 2                                       # QPs the emulation runs (its cost is the Python loop over the stages)
EMU_FLOOR = 1e-12                                 # e_dev <= M max(e_emu, EMU_FLOOR)
ORACLE_QPS = 8                                    # QPs of a handle's batch the oracle follows
BATCH_MFMA, BATCH_ONE_LANE = 3, 70
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "alt_drift_emulation.json")


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    make: object               # batch -> Problem
    rho: float
    segments: int
    alpha: float = 1.0
    control: bool = False      # a benign problem: no drift expected
    wide: bool = False         # (12, 6): one family only, whichever is the default


CASES = [
    Case("rdv_rho0.05_s16", lambda b: pkg.cw_rendezvous(N=1000, batch=b), 0.05, 16),
    Case("rdv_rho0.8_s16", lambda b: pkg.cw_rendezvous(N=1000, batch=b), 0.8, 16),
    Case("rdv_rho0.8_s1", lambda b: pkg.cw_rendezvous(N=1000, batch=b), 0.8, 1),
    Case("rdv_rho0.8_s64", lambda b: pkg.cw_rendezvous(N=1000, batch=b), 0.8, 64),
    Case("rdv_rho2_s16", lambda b: pkg.cw_rendezvous(N=1000, batch=b), 2.0, 16),
    Case("rdv_rho16_s16", lambda b: pkg.cw_rendezvous(N=1000, batch=b), 16.0, 16),
    Case("rdv_soc_rho0.8_s16", lambda b: pkg.cw_rendezvous(N=1000, batch=b, thrust_norm=True), 0.8, 16),
    Case("rdv_rho0.8_s16_alpha1.6", lambda b: pkg.cw_rendezvous(N=1000, batch=b), 0.8, 16, alpha=1.6),
    Case("formation_rho0.8_s16", lambda b: pkg.cw_formation(N=1000, batch=b), 0.8, 16, wide=True),
    Case("rdv200_rho0.8_s4", lambda b: pkg.cw_rendezvous(N=200, batch=b), 0.8, 4, control=True),
    Case("ltv40_6_1_rho0.02_s4", lambda b: pkg.random_ltv(N=40, n=6, m=1, batch=b, seed=14, with_q=False), 0.02, 4, control=True),
]
BY_ID = {c.id: c for c in CASES}

# the two full solves of the GPU tier: 70 QPs of the headline problem with the adaptive rule (rho ends at 0.4; 870 / 520 iterations)
SOLVE_KW = dict(rho=0.05, eps_abs=1e-6, eps_rel=1e-6, max_iter=4000, check_interval=10, adapt_interval=20)
SOLVE_ALPHAS = (1.0, 1.6)


def solve_problem():
    return pkg.cw_rendezvous(N=1000, batch=BATCH_ONE_LANE)


def pick(p, idx):
    """The QPs `idx` of p as a batch of their own (QPs are independent; Problem.slice for a list of indices)."""
    parts = [p.slice(int(i), int(i) + 1) for i in idx]
    return dataclasses.replace(parts[0], x0=np.concatenate([s.x0 for s in parts]),
                               q=None if p.q is None else np.concatenate([s.q for s in parts]))


def spread(batch, count=ORACLE_QPS):
    """`count` QP indices spread over the batch, first and last included (all of a smaller batch)."""
    return sorted(set(np.linspace(0, batch - 1, min(count, batch)).round().astype(int).tolist()))


def split_errors(got, ref, p):
    """Worst error over w, z, y relative to max(1, |ref|_inf): on the stages < EARLY, on the stages >= LATE
    (0 where the horizon has no such stage), and on all stages."""
    early = late = total = 0.0
    for a, b in zip(got, ref):
        d = np.abs(np.asarray(a) - np.asarray(b)).reshape(-1, p.N, p.nb) / max(1.0, np.abs(b).max())
        early = max(early, float(d[:, :EARLY].max()))
        if p.N > LATE:
            late = max(late, float(d[:, LATE:].max()))
        total = max(total, float(d.max()))
    return early, late, total


def oracle_checkpoints(p, rho, alpha, checkpoints=CHECKPOINTS):
    """{K: (w, z, y)} of the C oracle's Riccati loop from (z, y) = 0, continued from checkpoint to checkpoint."""
    out, z, y, done = {}, None, None, 0
    for K in checkpoints:
        r = oc.solve(p, rho=rho, alpha=alpha, max_iter=K - done, check_interval=K - done, z0=z, y0=y, stop=False)
        z, y, done = r["z"], r["y"], K
        out[K] = (r["w"], z, y)
    return out


def emulate(case, checkpoints=HOST_CHECKPOINTS, qps=EMU_QPS):
    """The alternating and the plain emulation of `case` on its first `qps` QPs against the oracle.  Returns a dict:
    alt_ok, segments, K, and per K the split errors of the first (early / late / total) and the error of the second (plain_total),
    the forms that ran, and the emulation's and the oracle's last (w, z, y) for the active-set comparison."""
    p = case.make(qps)
    rec = host_factor(p, case.rho, case.segments)
    out = dict(alt_ok=bool(rec["alt_ok"]), K=list(checkpoints), p=p, segments=len(rec["seg_start"]) - 1)
    if not rec["alt_ok"]:
        return out
    ref = oracle_checkpoints(p, case.rho, case.alpha, checkpoints)
    alt, forms = alternating_loop(rec, p, case.rho, checkpoints[-1], alpha=case.alpha, checkpoints=checkpoints)
    pln, _ = alternating_loop(rec, p, case.rho, checkpoints[-1], alpha=case.alpha, checkpoints=checkpoints, plain=True)
    e = [split_errors(alt[K], ref[K], p) for K in checkpoints]
    ep = [split_errors(pln[K], ref[K], p) for K in checkpoints]
    out.update(early=[x[0] for x in e], late=[x[1] for x in e], total=[x[2] for x in e], plain_total=[x[2] for x in ep],
               forms=forms, last=alt[checkpoints[-1]], last_ref=ref[checkpoints[-1]])
    return out


def active_sets(p, z):
    """Which rows of z sit on a bound: the lower and the upper face of the box, and per stage the thrust ball."""
    import admm_ref as ar
    lo, hi = ar.expand_bounds(p.lo, p.hi, p.N, p.nb)
    sets = [z == lo, z == hi]
    if p.unorm is not None:
        un = ar.expand_unorm(p.unorm, p.N)
        nrm = np.sqrt(np.sum(z.reshape(-1, p.N, p.nb)[:, :, :p.m] ** 2, axis=2))
        sets.append(nrm >= un[None, :] * (1.0 - 1e-12))
    return sets


@functools.lru_cache(maxsize=None)
def fixture():
    """tests/golden/alt_drift_emulation.json (written by tests/golden/make_alt_drift.py): per case the emulation's errors at
    CHECKPOINTS, 400 iterations of it being too slow for a GPU test file."""
    with open(FIXTURE) as f:
        return json.load(f)


def emu_running_max(case_id):
    """{K: running maximum over the checkpoints <= K of the emulation's error (all stages)} from the fixture."""
    d = fixture()["cases"][case_id]
    assert tuple(d["K"]) == CHECKPOINTS
    return dict(zip(d["K"], np.maximum.accumulate(d["total"]).tolist()))
