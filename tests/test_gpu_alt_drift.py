"""Long runs of the default (alternating) path at rho >= 0.8 on N = 1000 horizons against the C oracle (cases and
helpers: tests/_alt_drift.py, their conditions: tests/test_alt_drift_host.py).

The forward-elimination form of every other iteration is less accurate in the controls of the first stages (backward gains of
2.5e4 at stage 0 of the rendezvous), and at rho >= 0.2 ADMM contracts that error slowly: in the NumPy emulation of the iteration
from the library's host records the stages below 16 leave 1e-10 after ~80 iterations at rho = 0.8 and reach 3e-10 at 400, while
every stage from 64 on stays at 1e-12 and the plain path at 2e-13.  What is asserted, per case, on three kinds of handle (batch 3,
default flags: MFMA family, matrix-vector scan; batch 70, ADMM_FLAG_NO_MFMA: one-lane kernels, two waves, clamped lanes; batch 70,
plain path; the thrust-bound case and the (6, 1) control have no MFMA form, their batch-3 handle runs the one-lane kernels with
the matrix-vector scan; the (12, 6) formation runs on its default family and its plain path at batch 3), at 8, 16, 40, 80, 120, 200,
400 iterations reached by successive calls with read-outs in between, and at 400 in one call:

  A  plain path: within 1e-10 on every stage at every checkpoint;
  B  alternating paths, stages >= 64: within 1e-10 at every checkpoint;
  C  alternating paths, stages < 16, through the first 16 iterations: within 1e-10;
  D  alternating paths, all stages, all K: e_dev(K) <= M max(e_emu(K), 1e-12), both the running maximum over the checkpoints up
     to K of the error against the oracle, e_emu the emulation's (2 QPs, tests/golden/alt_drift_emulation.json; the CPU tier
     re-derives it up to K = 120).  M: the next power of two at or above 4x the worst ratio measured on the MI355X (the
     convention of the read-out tests) -- the kernels lose what the form loses, no more;
  E  full solves of 70 QPs of the headline problem with the adaptive rule (rho 0.05 -> 0.4 by iteration 60; 870 iterations, 520
     with alpha = 1.6): counts, rho and status as the oracle's, the plain handle's solution within 1e-10, the default handle's
     within D, its KKT certificate (tests/_indep.py) no worse than twice the plain handle's.

The reference is the oracle's Riccati loop on 8 QPs spread over the batch, continued from checkpoint to checkpoint."""
import functools

import numpy as np
import pytest

import admm_library_amd as pkg
from admm_library_amd import _abi
import oracle_c as oc
import _alt_drift as ad
import _indep

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error:.*forward-elimination form failed:RuntimeWarning")]

# Bound D.  MEASURED on the MI355X (worst e_dev(K) / max(e_emu(K), 1e-12) over the checkpoints and both ways to get there; the table
# per case and checkpoint is in DESIGN.md §5): MFMA family 0.67 ... 1.29 on the rendezvous cases at rho <= 2 and alpha = 1.6,
# 1.96 on the formation, 3.62 at rho = 16 (2.1e-9 at K = 400 against the emulation's 5.7e-10 and the one-lane kernels' 9.1e-10: the
# worst of all, on a handle whose forward form passes its host gate by the least); one-lane family 0.87 ... 1.74, and 2.33 on
# the N = 200 control (3.7e-12 against 1.6e-12).  4 x 3.62 = 14.5 -> the next power of two.
M = 16
NO_ALT, NO_MFMA = _abi.FLAG_NO_ALTERNATE, _abi.FLAG_NO_MFMA
MFMA_DIMS = {(12, 6), (6, 3), (10, 4)}
KINDS = {
    # kind: (batch, flags, alternating)
    "mfma_b3": (ad.BATCH_MFMA, 0, True),
    "one_lane_b70": (ad.BATCH_ONE_LANE, NO_MFMA, True),
    "plain_b70": (ad.BATCH_ONE_LANE, NO_MFMA | NO_ALT, False),
    # (12, 6): the family it defaults to, and its plain path
    "default_b3": (ad.BATCH_MFMA, 0, True),
    "plain_b3": (ad.BATCH_MFMA, NO_ALT, False),
}
PARAMS = [(c, k) for c in ad.CASES for k in (("default_b3", "plain_b3") if c.wide else ("mfma_b3", "one_lane_b70", "plain_b70"))]


def _family(p, flags):
    """The family a handle of p with these flags runs: the fp64 MFMA form by default for a small batch of a compiled shape
    without q or thrust bound (csrc/admm_setup.hip); the one-lane kernels otherwise."""
    small = p.batch <= 64 or (p.n >= 9 and p.batch <= 128)
    mfma = not (flags & (NO_MFMA | NO_ALT)) and (p.n, p.m) in MFMA_DIMS and p.q is None and p.unorm is None and small
    return "mfma_fp64" if mfma else "one_lane_fp64"


@functools.lru_cache(maxsize=None)
def _reference(case_id, batch):
    """The oracle's checkpoints on the spread QPs of the case's problem at this batch: computed once, shared by the kinds."""
    case = ad.BY_ID[case_id]
    p = case.make(batch)
    idx = ad.spread(batch)
    sub = ad.pick(p, idx)
    ref = ad.oracle_checkpoints(sub, case.rho, case.alpha)
    for v in ref.values():
        for a in v:
            a.setflags(write=False)
    return p, idx, sub, ref


def _handle(p, case, flags, alternating):
    s = pkg.Solver(p, pkg.Options(rho=case.rho, alpha=case.alpha, segments=case.segments, flags=flags))
    path = s.path()
    assert path["alternating"] == alternating and path["kernel_family"] == _family(p, flags) and path["segments"] == case.segments
    return s


@pytest.mark.parametrize("case,kind", PARAMS, ids=[f"{c.id}-{k}" for c, k in PARAMS])
def test_drift_of_long_runs(gpu, case, kind):
    batch, flags, alternating = KINDS[kind]
    p, idx, sub, ref = _reference(case.id, batch)
    Ks = ad.CHECKPOINTS
    step, done = {}, 0
    with _handle(p, case, flags, alternating) as s:          # successive calls, a read-out at every checkpoint
        for K in Ks:
            s.iterate(K - done)
            done = K
            step[K] = ad.split_errors([a[idx] for a in s.get()], ref[K], sub)
    with _handle(p, case, flags, alternating) as s:          # one uninterrupted call
        s.iterate(Ks[-1])
        whole = ad.split_errors([a[idx] for a in s.get()], ref[Ks[-1]], sub)
    emu = ad.emu_running_max(case.id)
    run = dict(zip(Ks, np.maximum.accumulate([step[K][2] for K in Ks]).tolist()))
    ratio = max(max(run[K] / max(emu[K], ad.EMU_FLOOR) for K in Ks), whole[2] / max(emu[Ks[-1]], ad.EMU_FLOOR))
    fmt = lambda v: " ".join(f"{x:.1e}" for x in v)
    print(f"\n{case.id} {kind}: K = {list(Ks)}\n  stages < {ad.EARLY}:  {fmt(step[K][0] for K in Ks)} | one call: {whole[0]:.1e}"
          f"\n  stages >= {ad.LATE}: {fmt(step[K][1] for K in Ks)} | one call: {whole[1]:.1e}"
          f"\n  all stages:   {fmt(step[K][2] for K in Ks)} | one call: {whole[2]:.1e}"
          f"\n  emulation:    {fmt(emu[K] for K in Ks)} (running maximum)\n  worst e_dev / max(e_emu, {ad.EMU_FLOOR:g}) = {ratio:.2f}")
    if not alternating:
        assert max(max(step[K][2] for K in Ks), whole[2]) <= ad.TOL                       # A
        return
    assert max(max(step[K][1] for K in Ks), whole[1]) <= ad.TOL                           # B
    assert max(step[K][0] for K in Ks if K <= ad.FRESH) <= ad.TOL                         # C
    assert ratio <= M                                                                     # D


@functools.lru_cache(maxsize=None)
def _solve_reference(alpha):
    p = ad.solve_problem()
    return p, oc.solve(p, alpha=alpha, **ad.SOLVE_KW)


# The yardstick of a solve's bound D: the emulation's largest figure through 400 iterations at rho = 0.8, the case of the table
# next above the rho = 0.4 both solves spend all but their first 60 iterations at.  (The solves run longer at that rho than the
# emulation's 400 iterations; its growth has flattened by then -- 2.3e-10 at 200, 2.8e-10 at 400 -- and the stopping rule ends
# a solve where the iterates have all but stopped moving.  MEASURED: 0.33 and 0.32 of the yardstick, 9.3e-11 and 9.1e-11.)
SOLVE_YARDSTICK = {1.0: "rdv_rho0.8_s16", 1.6: "rdv_rho0.8_s16_alpha1.6"}


@pytest.mark.parametrize("alpha", ad.SOLVE_ALPHAS)
def test_solves_through_the_drifting_regime(gpu, alpha):
    p, ref = _solve_reference(alpha)
    idx = ad.spread(p.batch)
    sub = ad.pick(p, idx)
    got = {}
    for name, flags in (("default", 0), ("plain", NO_ALT)):
        with pkg.Solver(p, pkg.Options(alpha=alpha, flags=flags, **ad.SOLVE_KW)) as s:
            assert (s.path()["alternating"], s.path()["kernel_family"]) == (name == "default", "one_lane_fp64")
            info = s.solve()
            w, z, y = s.get()
        assert int(info.iters_run) == int(ref["iters_run"]) and float(info.rho) == float(ref["rho"])
        assert int(info.rho_updates) == int(ref["rho_updates"])
        np.testing.assert_array_equal(info.status, ref["status"])
        assert np.abs(info.iters.astype(int) - ref["iters"].astype(int)).max() <= ad.SOLVE_KW["check_interval"]
        err = ad.split_errors([a[idx] for a in (w, z, y)], [ref[k][idx] for k in ("w", "z", "y")], sub)
        cert = _indep.kkt_certificate_batch(sub, z[idx], y[idx], float(info.rho))[:4]
        got[name] = (err, [float(c.max()) for c in cert])
        print(f"\nalpha = {alpha} {name}: {info.iters_run} iterations, rho = {info.rho}; error on stages < {ad.EARLY}: {err[0]:.1e}, "
              f">= {ad.LATE}: {err[1]:.1e}, all: {err[2]:.1e}; certificate (dynamics, box, stationarity, complementarity): "
              + " ".join(f"{c:.2e}" for c in got[name][1]))
    assert got["plain"][0][2] <= ad.TOL
    assert got["default"][0][1] <= ad.TOL
    yard = max(ad.emu_running_max(SOLVE_YARDSTICK[alpha]).values())
    print(f"  default / max(e_emu, floor) = {got['default'][0][2] / max(yard, ad.EMU_FLOOR):.2f}")
    assert got["default"][0][2] <= M * max(yard, ad.EMU_FLOOR)
    for a, b in zip(got["default"][1], got["plain"][1]):
        assert a <= 2.0 * b, (got["default"][1], got["plain"][1])

