"""CPU tier of the long-run drift tests of the alternating path (cases: tests/_alt_drift.py).  Pins what
tests/test_gpu_alt_drift.py rests on, with the C oracle and the NumPy emulation of the whole alternating iteration only:

  * every case passes the library's host gate (alt_ok), so its handle really alternates;
  * the emulation with the Riccati form on every iteration -- the plain path's arithmetic, segment algebra and dense scan
    included -- stays within 2e-12 of the oracle through 120 iterations: what the alternating emulation loses, the
    forward-elimination form loses, not the segments;
  * the alternating emulation is within 1e-10 through the first 16 iterations on every case and within 1e-11 on the stages
    from 64 on at every checkpoint, and at least three cases leave 1e-10 on the stages below 16 by iteration 120 -- the
    statement the GPU tier is about;
  * the active sets of the emulation and the oracle agree at iteration 120 (the drift is no change of active set);
  * the committed 400-iteration figures (tests/golden/alt_drift_emulation.json) are what this emulation gives up to 120;
  * no stopping or adaptive-rule decision of the two full solves of the GPU tier is within a relative 1e-6 of its threshold.

MEASURED (2 QPs per case; worst over w, z, y relative to max(1, |ref|_inf); K = 8, 16, 40, 80, 120; -s prints every figure):
plain emulation <= 2.4e-13; alternating emulation <= 3.1e-11 through K = 16 and <= 1.0e-12 from stage 64 on; below stage 16 at
K = 120: 1.8e-10 at rho = 0.8 (1, 16 or 64 segments alike: 1.8e-10, 1.8e-10, 1.7e-10), 1.3e-10 at rho = 2, 1.8e-10 at rho = 16,
2.2e-10 with alpha = 1.6 -- six cases outside 1e-10 --, 1.5e-11 at rho = 0.05, 4.8e-11 with the thrust bound, 5.1e-11 on the
formation, 1.3e-12 and 8.3e-14 on the controls.  The solves: 870 iterations (alpha = 1) and 520 (1.6), rho 0.05 -> 0.4 in 3 updates."""
import functools

import numpy as np
import pytest

import admm_library_amd as pkg
import _alt_drift as ad
from _handle_model import HandleModel
from _segmented import form_schedule

PLAIN_TOL = 2e-12        # plain emulation vs oracle, every checkpoint
LATE_TOL = 1e-11         # alternating emulation vs oracle on the stages >= ad.LATE, every checkpoint
MIN_DRIFTING = 3         # cases that must exceed ad.TOL on the stages < ad.EARLY by the last checkpoint


@functools.lru_cache(maxsize=None)
def _emulated(case_id):
    return ad.emulate(ad.BY_ID[case_id])


def test_form_schedule_is_next_form():
    """form_schedule against next_form / after_form of csrc/admm_launch.hip, worked by hand: the first iteration of a fresh handle
    is plain (v is not valid yet); a backward (forward-elimination) iteration starts only with an even number of iterations of
    the call remaining; a call never ends on one; the state a call leaves carries into the next (admm_get leaves it alone)."""
    assert form_schedule(1) == (["plain"], "none")
    assert form_schedule(2) == (["plain", "plain"], "none")
    assert form_schedule(3) == (["plain", "fwd_start", "plain"], "none")
    assert form_schedule(4) == (["plain", "fwd_start", "bwd", "fwd"], "fwd")
    assert form_schedule(5) == (["plain", "fwd_start", "fwd_start", "bwd", "fwd"], "fwd")
    assert form_schedule(2, True, "fwd") == (["bwd", "fwd"], "fwd")
    assert form_schedule(3, True, "fwd") == (["fwd_start", "bwd", "fwd"], "fwd")
    assert form_schedule(1, True, "fwd") == (["plain"], "none")
    assert form_schedule(2, True, "none") == (["fwd_start", "plain"], "none")
    # the GPU tier's two ways to iteration 400 run the SAME forms (every call length between checkpoints is even): the
    # forward-elimination form on the odd iterations from 3 on
    whole, _ = form_schedule(ad.CHECKPOINTS[-1])
    parts, v, st = [], False, "none"
    for c in np.diff((0,) + ad.CHECKPOINTS):
        f, st = form_schedule(int(c), v, st)
        parts += f
        v = True
    want = [it >= 3 and it % 2 == 1 for it in range(1, ad.CHECKPOINTS[-1] + 1)]
    assert [f == "bwd" for f in whole] == want and [f == "bwd" for f in parts] == want


@pytest.mark.parametrize("case", ad.CASES, ids=lambda c: c.id)
def test_conditions_on_the_inputs(lib, case):
    e = _emulated(case.id)
    assert e["alt_ok"] and e["segments"] == case.segments
    K = e["K"]
    assert tuple(K) == ad.HOST_CHECKPOINTS
    print(f"\n{case.id}: K = {K}\n  alternating, stages < {ad.EARLY}: " + " ".join(f"{v:.1e}" for v in e["early"]) +
          f"\n  alternating, stages >= {ad.LATE}: " + " ".join(f"{v:.1e}" for v in e["late"]) +
          "\n  alternating, all stages: " + " ".join(f"{v:.1e}" for v in e["total"]) +
          "\n  plain, all stages:       " + " ".join(f"{v:.1e}" for v in e["plain_total"]))
    assert [f == "bwd" for f in e["forms"]] == [it >= 3 and it % 2 == 1 for it in range(1, K[-1] + 1)]
    assert max(e["plain_total"]) <= PLAIN_TOL
    assert all(t <= ad.TOL for k, t in zip(K, e["total"]) if k <= ad.FRESH)
    assert max(e["late"]) <= LATE_TOL
    for a, b in zip(ad.active_sets(e["p"], e["last"][1]), ad.active_sets(e["p"], e["last_ref"][1])):
        assert np.array_equal(a, b)
    # the committed figures of the same emulation (the yardstick of the GPU tier's bound D): its running maximum, within
    # the factor 2 that another BLAS's summation order in the scan product may move a rounding-level figure by
    fix = ad.emu_running_max(case.id)
    here = np.maximum.accumulate(e["total"])
    for k, v in zip(K, here):
        a, b = max(v, ad.EMU_FLOOR), max(fix[k], ad.EMU_FLOOR)
        assert a <= 2 * b and b <= 2 * a, (k, v, fix[k])


def test_the_drift_is_there(lib):
    """By iteration 120 at least three cases are outside 1e-10 on the stages below 16 in the emulation, none of them a control,
    and the controls stay well inside: the GPU tier's bound D is about something."""
    last = {c.id: _emulated(c.id)["early"][-1] for c in ad.CASES}
    drifting = [i for i, v in last.items() if v > ad.TOL]
    print("\nstages <", ad.EARLY, "at K = 120:", {i: f"{v:.1e}" for i, v in last.items()})
    assert len(drifting) >= MIN_DRIFTING
    assert not any(ad.BY_ID[i].control for i in drifting)
    assert all(max(_emulated(c.id)["total"]) <= 0.5 * ad.TOL for c in ad.CASES if c.control)


@pytest.mark.parametrize("alpha", ad.SOLVE_ALPHAS)
def test_no_decision_of_the_solves_is_near_its_threshold(built, alpha):
    """The two full solves of the GPU tier (oracle run of all 70 QPs, through the host model of a handle): every comparison of
    the stopping rule and of the adaptive rule stays a relative 1e-6 from its threshold, as in tests/test_handle_model_host.py,
    so that the drift of the default path cannot flip one; and the run ends where DESIGN.md §4.8 says it does."""
    m = HandleModel(ad.solve_problem(), pkg.Options(alpha=alpha, **ad.SOLVE_KW))
    info = m.solve()
    print(f"\nalpha = {alpha}: {info['iters_run']} iterations, rho = {info['rho']}, {info['rho_updates']} updates, "
          f"{int(info['status'].sum())} of {len(info['status'])} converged")
    assert info["status"].all()
    assert (info["iters_run"], info["rho"], info["rho_updates"]) == {1.0: (870, 0.4, 3), 1.6: (520, 0.4, 3)}[alpha]
    assert m.margins
    for what, lhs, thr in m.margins:
        assert abs(lhs - thr) > 1e-6 * max(abs(lhs), abs(thr)), (what, lhs, thr)
