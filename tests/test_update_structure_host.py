"""The inputs of the structure-changing update tests (tests/_update_structure.py), pinned on the oracle alone: no GPU.

These are CONDITIONS on the committed cases, not tolerances: a case built on a problem whose state rows are never active would
pass whatever the kernels did with the dual of those rows.  Each test prints the values it checks (pytest -s)."""
import dataclasses

import numpy as np
import pytest

from admm_library_amd.solver import host_factor

import _update_structure as us
from _handle_model import HandleModel

CASES = us.cases()
IDS = [us.cid(c) for c in CASES]
DROPS = ("open", "open_partial", "set_state_open")       # transitions after which a handle could wrongly take the state-row dual for zero
SCAN_GROWTH_MAX = 100.0                                  # admm_setup's conditioning bound (tests/test_shapes.py)


def _first_change(case):
    """(index of the first update / set_state op, the model's (z, y, rho, problem) before it)."""
    ref = us.reference(case)
    i = min(ref.states)
    return i, ref.states[i]


def _opened_rows(p_before, p_after):
    """(L,) mask of the state rows that are bounded in p_before and (-inf, inf) in p_after."""
    N, nb = p_before.N, p_before.nb
    was = np.isfinite(np.broadcast_to(p_before.lo, (N, nb))) | np.isfinite(np.broadcast_to(p_before.hi, (N, nb)))
    now = np.isneginf(np.broadcast_to(p_after.lo, (N, nb))) & np.isposinf(np.broadcast_to(p_after.hi, (N, nb)))
    mask = was & now
    mask[:, :p_before.m] = False
    return mask.reshape(-1)


def _one_iteration(case, p, z, y, rho):
    m = HandleModel(p, us.options(case), fused=not us.KINDS[case.kind].get("unfused", False))
    m.rho = rho
    m.set_state(z=z, y=y)
    m.run(1, 0)
    return m.w


def test_every_cell_runs_or_is_skipped_by_its_table_entry():
    ran = {(c.transition, c.kind) for c in CASES}
    skipped = {(t, k) for t, k, _ in us.skipped()}
    assert not ran & skipped
    assert ran | skipped == {(t, k) for t in us.TRANSITIONS for k in us.KINDS}
    assert all(why for _, _, why in us.skipped())
    assert len(set(CASES)) == len(CASES)
    for c in CASES:
        n, m, N, batch = us.SHAPES[c.shape]
        assert N <= 45 and batch <= 69
        probs = us.problems(c)
        assert len({(p.N, p.n, p.m, p.batch, p.q is None, p.unorm is None) for p in probs}) == 1
    print(f"{len(CASES)} cases, {len(skipped)} (transition, kind) cells skipped by the table")


@pytest.mark.parametrize("case", [c for c in CASES if c.transition in DROPS], ids=lambda c: us.cid(c))
def test_state_rows_carry_a_dual_and_dropping_it_shows(built, case):
    """Before open / open_partial / set_state_open at least half of the QPs hold a non-zero dual on a state row that is open
    afterwards, and a reference that zeroes those duals before it goes on differs from the true chain by more than 1e-3 in w after
    one iteration: the GPU comparison (1e-10) cannot miss a handle that drops them."""
    probs = us.problems(case)
    i, (z, y, rho, p_before) = _first_change(case)
    if case.transition == "set_state_open":
        y = us.set_state_y(p_before)
        p_after, rows = p_before, _opened_rows(us.base(case.kind, case.shape), p_before)
    else:
        p_after = dataclasses.replace(probs[1], fuel=p_before.fuel, soft=p_before.soft, consensus=p_before.consensus)
        rows = _opened_rows(p_before, p_after)
    assert rows.any()
    carrying = int(np.any(y[:, rows] != 0.0, axis=1).sum())
    ymax = float(np.abs(y[:, rows]).max())
    y_mut = y.copy()
    y_mut[:, rows] = 0.0
    dw = float(np.abs(_one_iteration(case, p_after, z, y, rho) - _one_iteration(case, p_after, z, y_mut, rho)).max())
    print(f"{us.cid(case)}: {carrying} of {p_before.batch} QPs carry a state-row dual, max |y_x| = {ymax:.3g}; dropping it moves w by {dw:.3g}")
    assert 2 * carrying >= p_before.batch
    assert dw > 1e-3


@pytest.mark.parametrize("case", [c for c in CASES if c.transition == "close"], ids=lambda c: us.cid(c))
def test_the_open_solution_violates_the_box_that_closes(built, case):
    """Before close, the iterate of the open problem lies outside p2's state box on at least half of the QPs: the duals come back."""
    probs = us.problems(case)
    i, (z, y, rho, p_before) = _first_change(case)
    N, nb, m = p_before.N, p_before.nb, p_before.m
    lo, hi = (np.broadcast_to(a, (N, nb)).reshape(-1) for a in (probs[1].lo, probs[1].hi))
    state = np.tile(np.arange(nb) >= m, N)
    out = ((z < lo) | (z > hi)) & state
    n_out = int(np.any(out, axis=1).sum())
    assert not np.any(y[:, state] != 0.0)                  # (an open row holds no dual)
    print(f"{us.cid(case)}: {n_out} of {p_before.batch} QPs outside the closing box, worst by {float(np.maximum(lo - z, z - hi)[out].max()):.3g}")
    assert 2 * n_out >= p_before.batch


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_gate_and_the_growth_bound_are_as_stated(built, case):
    """host_factor(...)["alt_ok"] of every problem of every case has the stated value (at RHO, and the last problem at RHO_AFTER,
    where admm_set_rho refactors it), and max |W| (and |WB| where that form exists) stays inside the conditioning bound."""
    probs = us.problems(case)
    want, want_after = us.alt_ok_expected(case)
    got = []
    for p, rho in [(p, us.RHO) for p in probs] + [(probs[-1], us.RHO_AFTER)]:
        hf = host_factor(dataclasses.replace(p, fuel=None, soft=None, consensus=None), rho, us.SEGMENTS)
        growth = max(np.abs(hf["scanW"]).max(), np.abs(hf["scanWB"]).max() if hf["alt_ok"] else 0.0)
        assert growth <= SCAN_GROWTH_MAX, (us.cid(case), rho, growth)
        got.append(bool(hf["alt_ok"]))
    assert got == want + [want_after], (us.cid(case), got, want, want_after)


@pytest.mark.parametrize("case", [c for c in CASES if c.transition == "thrust_move"], ids=lambda c: us.cid(c))
def test_thrust_move_has_stages_of_either_kind_on_their_bounds(built, case):
    """Each problem has ball stages and box stages, they swap, and after the pre-phase and at the end of the post-phase some stage sits
    on its ball and some on its box: both branches of the z-update do work on both sides of the update."""
    p1, p2 = us.problems(case)
    b1, b2 = np.isfinite(p1.unorm), np.isfinite(p2.unorm)
    assert b1.any() and (~b1).any() and np.array_equal(b2, ~b1)
    for p, ball in ((p1, b1), (p2, b2)):
        assert np.all(np.isfinite(p.lo[~ball, :p.m])) and np.all(np.isinf(p.lo[ball, :p.m]))
    ref = us.reference(case)
    i, (z_pre, _, _, _) = _first_change(case)
    z_end = [l for l in ref.log if l and "z" in l][-1]["z"]
    for what, p, z in (("pre-phase", p1, z_pre), ("end", p2, z_end)):
        u = z.reshape(p.batch, p.N, p.nb)[:, :, :p.m]
        ball = np.isfinite(p.unorm)
        on_ball = int((np.linalg.norm(u[:, ball], axis=2) >= p.unorm[ball] * (1.0 - 1e-12)).any(axis=0).sum())
        on_box = int(((u[:, ~ball] == p.lo[~ball, :p.m]) | (u[:, ~ball] == p.hi[~ball, :p.m])).any(axis=(0, 2)).sum())
        print(f"{us.cid(case)} {what}: {on_ball} of {int(ball.sum())} ball stages on the ball, {on_box} of {int((~ball).sum())} box stages on the box")
        assert on_ball >= 1 and on_box >= 1


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_no_decision_of_a_case_is_near_its_threshold(built, case):
    """The rule of tests/test_handle_model_host.py: every comparison of the stopping rule and of the adaptive rule along the
    reference stays a relative 1e-6 away from its threshold, so rounding on the GPU cannot flip one."""
    ref = us.reference(case)
    cfg = us.KINDS[case.kind]
    if cfg.get("solve", True) and "world" not in cfg:
        assert ref.margins
    near = min((abs(a - b) / max(abs(a), abs(b)) for _, a, b in ref.margins), default=np.inf)
    for what, lhs, thr in ref.margins:
        assert abs(lhs - thr) > 1e-6 * max(abs(lhs), abs(thr)), (what, lhs, thr)
    assert all(np.all(np.isfinite(a)) for l in ref.log if l for k, a in l.items() if k in ("w", "z", "y"))
    print(f"{us.cid(case)}: {len(ref.margins)} comparisons, the nearest a relative {near:.2e} from its threshold")


@pytest.mark.parametrize("kind", us.PROBE_KINDS)
def test_the_probe_chain_flags_what_the_box_implies(built, kind):
    """The reference of the probe test: flagged under the corridor, not flagged without it, flagged again; every decision of the
    probe (sep against -eps, the open-row magnitude against eps |mu|_inf) a relative 1e-6 from its threshold, and no zero / nonzero
    decision within rounding of flipping where a flag depends on it."""
    ref = us.probe_reference(kind)
    for out, want in zip(ref.outs, us.PROBE_FLAGS):
        assert out["infeasible"].tolist() == want, (out["infeasible"], out["sep"])
    for what, lhs, thr in ref.margins:
        assert abs(lhs - thr) > 1e-6 * max(abs(lhs), abs(thr)), (what, lhs, thr)
    print(kind, "sep:", [np.round(o["sep"], 3).tolist() for o in ref.outs], "unclear:", ref.unclear)
    # the feasible QP 0 converges: its drift is a rounding error, and `defect` -- a quotient by it -- is left out of the GPU comparison
    # there (defect_clear).  No flag and no sep depends on such a decision: mu = 0 is clear everywhere, and a flagged QP is clear.
    assert all(what == "drift>0" and b == 0 for _, what, b, _, _ in ref.unclear), ref.unclear
    assert all(o["defect_clear"][np.asarray(want, bool)].all() for o, want in zip(ref.outs, us.PROBE_FLAGS))
