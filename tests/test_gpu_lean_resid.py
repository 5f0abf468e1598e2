"""GPU tests of the lean residual forms of the alternating kernels ("lean residual iterations";
csrc/admm_kernels_alt.hpp, LEAN): consecutive residual-evaluating iterations of admm_run on a handle whose state rows are
unbounded everywhere neither read nor write v of those rows; the state rows' share of the dual residual is rolled out from
the control rows' difference instead.  Every output but s is BIT-identical to the full forms (ADMM_NO_LEAN_RESID=1); s agrees
within ten times the disagreement measured on the host (tests/test_lean_resid_host.py: 8.1e-15 relative to the largest s of
the run, for 62-stage segments; the segments here are shorter)."""
import numpy as np
import pytest

import admm_library_amd as pkg
from admm_library_amd import _abi

pytestmark = pytest.mark.gpu

S_TOL = 10 * 8.1e-15            # relative to max(s) over the read-outs compared (tests/test_lean_resid_host.py)
ONE_LANE = _abi.FLAG_NO_MFMA    # the lean forms are one-lane fp64 kernels (small batches of these shapes default to MFMA)
CALLS = (1, 2, 3, 7, 10)        # both parities; a call of 1 is a plain iteration, of 3 begins with a start form

CASES = {
    # two column blocks with clamped lanes, unequal segments
    "cw_rendezvous_6_3": (lambda: pkg.cw_rendezvous(N=130, batch=300), 0.05, 4),
    "cw_formation_12_6": (lambda: pkg.cw_formation(N=70, batch=70), 0.05, 3),
    "random_ltv_6_3": (lambda: pkg.random_ltv(N=45, n=6, m=3, batch=67, seed=77, with_q=False, state_bounds=False), 0.3, 4),
}


def _readout(s):
    return s.get() + tuple(s.residuals())


def _run(p, rho, segs, lean, monkeypatch, script):
    if lean:
        monkeypatch.delenv("ADMM_NO_LEAN_RESID", raising=False)
    else:
        monkeypatch.setenv("ADMM_NO_LEAN_RESID", "1")
    with pkg.Solver(p, pkg.Options(rho=rho, segments=segs, flags=ONE_LANE)) as s:
        path = s.path()
        assert path["alternating"] and path["xfree"] and path["kernel_family"] == "one_lane_fp64"
        outs = script(s)
        return outs, s.lean_iterations()


def _compare(lean_outs, full_outs):
    names = ("w", "z", "y", "r", "s", "norm_w", "norm_z", "norm_y")
    smax = max(f[4].max() for f in full_outs[1:])           # (the first read-out follows a plain iteration: identical anyway)
    worst = 0.0
    for i, (a, b) in enumerate(zip(lean_outs, full_outs)):
        for name, x, y in zip(names, a, b):
            if name == "s":
                worst = max(worst, np.abs(x - y).max())
            else:
                np.testing.assert_array_equal(x, y, err_msg=f"{name} at read-out {i}")
    print(f"lean vs full s: worst |diff| {worst:.3e} = {worst / smax:.3e} of max(s) {smax:.3e} (bound {S_TOL:.1e})")
    assert worst <= S_TOL * smax


@pytest.fixture(scope="module")
def problems():
    return {k: v[0]() for k, v in CASES.items()}


@pytest.mark.parametrize("case", list(CASES))
def test_lean_forms_change_nothing_but_the_last_bits_of_s(gpu, case, problems, monkeypatch):
    """Calls of 1, 2, 3, 7 and 10 iterations with residuals every iteration, a full read-out after each."""
    p, (_, rho, segs) = problems[case], CASES[case]

    def script(s):
        outs = []
        for k in CALLS:
            s.run(k, residual_every=1)
            outs.append(_readout(s))
        return outs

    lean, n_lean = _run(p, rho, segs, True, monkeypatch, script)
    full, n_full = _run(p, rho, segs, False, monkeypatch, script)
    # (next_form) call of 1: plain; of 2: start form + plain; of 3: start form, then 2 lean; of 7: start form + 6; of 10: all ten
    assert n_full == 0 and n_lean == 2 + 6 + 10
    _compare(lean, full)


def test_state_changes_drop_the_side_data(gpu, problems, monkeypatch):
    """admm_set_rho, admm_set_state and admm_update_instances between calls: the iteration after each reads the full state."""
    p = problems["cw_rendezvous_6_3"]
    p2 = pkg.cw_rendezvous(N=130, batch=300, seed0=4242)
    counts = []

    def script(s):
        outs = []
        s.run(4, residual_every=1)
        outs.append(_readout(s))
        counts.append(s.lean_iterations())
        s.set_rho(0.2)
        s.run(4, residual_every=1)
        outs.append(_readout(s))
        counts.append(s.lean_iterations())
        w, z, y = outs[-1][:3]
        s.set_state(z=z * 0.5, y=y)
        s.run(6, residual_every=1)
        outs.append(_readout(s))
        counts.append(s.lean_iterations())
        s.update_instances(x0=p2.x0)
        s.run(4, residual_every=1)
        outs.append(_readout(s))
        counts.append(s.lean_iterations())
        s.run(2, residual_every=1)                 # nothing in between: resumes lean from the first iteration
        outs.append(_readout(s))
        counts.append(s.lean_iterations())
        s.step_x()
        s.run(2, residual_every=1)
        outs.append(_readout(s))
        counts.append(s.lean_iterations())
        return outs

    lean, _ = _run(p, 0.05, 4, True, monkeypatch, script)
    lean_counts = counts[:]
    del counts[:]
    full, _ = _run(p, 0.05, 4, False, monkeypatch, script)
    # a call that starts from (z, y) runs a plain iteration and a start form first (4 -> 2 lean, 6 -> 4); after
    # update_instances (v kept, elimination dropped) a call of 4 runs two start forms; a call of 2 after step_x none
    assert lean_counts == [2, 4, 8, 10, 12, 12] and counts == [0] * 6
    _compare(lean, full)


def test_lean_forms_run_and_only_where_they_apply(gpu, problems, monkeypatch):
    """Coverage guard: the counter moves in the benchmark's call pattern, and stays at 0 after iterations without residuals,
    with graph replay, with over-relaxation and on a handle with bounded state rows; the profile entry point runs the forms."""
    monkeypatch.delenv("ADMM_NO_LEAN_RESID", raising=False)
    p = problems["cw_rendezvous_6_3"]
    with pkg.Solver(p, pkg.Options(rho=0.05, segments=4, flags=ONE_LANE)) as s:
        s.run(20, residual_every=1)                # warm-up call, then the timed call: resumes lean across the boundary
        assert s.lean_iterations() == 18         # plain + start form first
        s.run(10, residual_every=1)
        assert s.lean_iterations() == 28
        s.run(12, residual_every=4)                # a predecessor without residuals: never lean
        s.iterate(3)
        assert s.lean_iterations() == 28
        pr = s.profile(2, residuals=True, alternating=True, lean=True)
        assert pr["xfze_ms"] > 0 and pr["xbze_ms"] > 0
        s.profile(2, residuals=True, alternating=True)      # the full forms: leaves no side data
        s.run(2, residual_every=1)
        assert s.lean_iterations() == 28 + 1
    for kw in (dict(flags=ONE_LANE | _abi.FLAG_GRAPH), dict(flags=ONE_LANE, alpha=1.6)):
        with pkg.Solver(p, pkg.Options(rho=0.05, segments=4, **kw)) as s:
            s.run(6, residual_every=1)
            assert s.lean_iterations() == 0
    pb = pkg.random_ltv(N=45, n=6, m=3, batch=67, seed=77, with_q=False)       # bounded state rows
    with pkg.Solver(pb, pkg.Options(rho=0.3, segments=4, flags=ONE_LANE)) as s:
        s.run(6, residual_every=1)
        assert s.lean_iterations() == 0
        with pytest.raises(pkg.AdmmError):
            s.profile(2, residuals=True, alternating=True, lean=True)
