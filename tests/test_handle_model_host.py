"""The host model of a handle (tests/_handle_model.py) and the committed call sequences (tests/_op_sequences.py), pinned without a
GPU: the model against the oracles it is built from, the sequences' coverage of ops and of neighbouring op classes, and the
distance of every stopping-rule / adaptive-rule decision along them from its threshold."""
import functools

import numpy as np
import pytest

import admm_library_amd as pkg
import oracle_c as oc
import _fuel_ref as fr
import _op_sequences as ops
from _handle_model import HandleModel

SOLVE = dict(eps_abs=1e-3, eps_rel=1e-3, max_iter=60, check_interval=5)
ADAPT = dict(adapt_interval=5, adapt_mu=2.0, adapt_tau=2.0, adapt_max=16)


def _problems():
    fuel = ops.problem("fuel_thrust_bound")
    return {"shared": pkg.random_ltv(N=12, n=4, m=2, batch=7, seed=3),
            "thrust": pkg.random_ltv(N=11, n=6, m=3, batch=5, seed=4, thrust_norm=True),
            "fuel": fuel,
            "per_instance": pkg.random_instances(N=10, n=4, m=2, batch=6, seed=5)}


def _oracle(p, **kw):
    if p.fuel is not None:
        r = fr.solve(p, **kw)
        return dict(w=r.w, z=r.z, y=r.y, r=r.r, s=r.s, rho=r.rho, rho_updates=r.rho_updates, iters=r.iters, status=r.status,
                    iters_run=r.iters_run)
    return oc.solve(p, **kw)


def _same(a, b, tol=1e-13):
    return np.abs(np.asarray(a) - np.asarray(b)).max() <= tol * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("alpha", [1.0, 1.6])
@pytest.mark.parametrize("name", ["shared", "thrust", "fuel", "per_instance"])
def test_iterate_and_run_compose_to_one_oracle_run(built, name, alpha):
    p = _problems()[name]
    m = HandleModel(p, pkg.Options(rho=0.3, alpha=alpha))
    calls = [("iterate", 1), ("run", 4, 3), ("run", 1, 2), ("iterate", 6), ("run", 9, 1), ("run", 7, 0), ("run", 5, 5)]
    total = 0
    for c in calls:
        getattr(m, c[0])(*c[1:])
        total += c[1]
    ref = _oracle(p, rho=0.3, alpha=alpha, max_iter=total, check_interval=total, stop=False)
    assert m.iterations == total
    for k, a in zip(("w", "z", "y"), m.get()):
        assert _same(a, ref[k]), k
    assert _same(m.residuals()[0], ref["r"]) and _same(m.residuals()[1], ref["s"])     # (the last call ended on a residual iteration)


@pytest.mark.parametrize("name", ["shared", "fuel"])
def test_set_rho_reproduces_an_adaptive_solve(built, name):
    """iterate + set_rho at the iterations where the oracle's adaptive rule changed rho = that solve's (z, y, rho)."""
    p = _problems()[name]
    kw = dict(rho=0.3, max_iter=40, check_interval=5, stop=False, **ADAPT)
    ref = _oracle(p, **kw)
    assert ref["rho_updates"] >= 2
    # rho in force during iteration T + 1 = rho at the end of a run of T + 1 iterations (the rule does not fire at max_iter)
    rho_after = {T: _oracle(p, **dict(kw, max_iter=T + 1))["rho"] for T in range(5, 40, 5)}
    m = HandleModel(p, pkg.Options(rho=0.3))
    for T in range(5, 45, 5):
        m.iterate(5)
        if T in rho_after:
            m.set_rho(rho_after[T])
    assert m.rho == ref["rho"]
    for k, a in zip(("w", "z", "y"), m.get()):
        assert _same(a, ref[k]), k


@pytest.mark.parametrize("alpha", [1.0, 1.6])
@pytest.mark.parametrize("name", ["shared", "thrust", "fuel"])
def test_step_x_then_step_z_is_one_iteration(built, name, alpha):
    p = _problems()[name]
    a, b = HandleModel(p, pkg.Options(rho=0.3, alpha=alpha)), HandleModel(p, pkg.Options(rho=0.3, alpha=alpha))
    a.iterate(3)
    b.iterate(3)
    a.run(1, 1)
    b.step_x()
    b.step_z(True)
    for x, y in zip(a.get() + a.residuals(), b.get() + b.residuals()):
        assert _same(y, x)


def test_step_x_with_per_instance_dynamics(built):
    p = pkg.random_instances(N=10, n=4, m=2, batch=6, seed=5)
    a, b = HandleModel(p, pkg.Options(rho=0.3)), HandleModel(p, pkg.Options(rho=0.3))
    a.iterate(4)
    b.iterate(3)
    b.step_x()
    b.iterate(1)
    assert _same(b.w, a.w) and _same(b.z, a.z)


@pytest.mark.parametrize("name", ["shared", "thrust", "fuel", "per_instance"])
def test_solve_is_the_oracles_solve(built, name):
    """The model's solve loop (pieces over oracle iterations) against ONE oracle solve with the stopping and adaptive rules,
    from a warm (z, y); with per-instance dynamics every QP keeps its own rho."""
    p = _problems()[name]
    opt = pkg.Options(rho=0.3, **SOLVE, **ADAPT)
    m = HandleModel(p, opt)
    m.iterate(3)
    z0, y0 = m.z.copy(), m.y.copy()
    info = m.solve()
    ref = _oracle(p, rho=0.3, z0=z0, y0=y0, stop=True, **SOLVE, **ADAPT)
    assert info["iters_run"] == ref["iters_run"]
    assert np.array_equal(info["iters"], ref["iters"]) and np.array_equal(info["status"], ref["status"])
    assert np.array_equal(m.rho_per_qp(), np.broadcast_to(ref["rho"], (p.batch,)))
    assert info["rho_updates"] == np.sum(ref["rho_updates"]) and info["rho_updates"] >= 1
    assert 0 < info["status"].sum()
    for k, a in zip(("w", "z", "y"), m.get()):
        assert _same(a, ref[k]), k


def test_a_refused_call_leaves_the_model_alone(built):
    from _handle_model import INVALID, Refused
    p = _problems()["fuel"]
    m = HandleModel(p, pkg.Options(rho=0.3))
    m.run(3, 1)
    before = [a.copy() for a in m.get() + m.residuals()]
    bad = m.z.copy()
    bad[0, 0] = np.nan
    for call in (lambda: m.set_state(z=bad), lambda: m.set_fuel(-np.ones(p.N)),
                 lambda: m.update_problem(ops.problem("fuel_thrust_bound", 2, dN=1))):
        with pytest.raises(Refused) as e:
            call()
        assert e.value.code == INVALID
    assert m.p is p and all(np.array_equal(a, b) for a, b in zip(before, m.get() + m.residuals()))


# ---- the committed sequences ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _model_run(kind, seed):
    return ops.run_model(kind, seed)


@pytest.mark.parametrize("kind", list(ops.KINDS))
def test_sequences_cover_every_op_and_every_pair_of_classes(kind):
    classes = ops.classes_of(kind)
    legal = ops.legal_ops(kind)
    seen_ops, seen_pairs = set(), set()
    for seed in ops.seeds(kind):
        seq = ops.sequence(kind, seed)
        assert seq == ops.sequence(kind, seed)                   # determined by (kind, seed)
        assert 30 <= len(seq) <= 50
        cls = [ops.op_class(n, a) for n, a in seq]
        for (n, a), c in zip(seq, cls):
            assert n in legal[c], (n, a, c)
            seen_ops.add((c, n))
        seen_pairs |= set(zip(cls, cls[1:]))
    assert seen_ops == {(c, n) for c in classes for n in legal[c]}, {(c, n) for c in classes for n in legal[c]} - seen_ops
    assert seen_pairs == {(a, b) for a in classes for b in classes}
    lengths = {a[0] for seed in ops.seeds(kind) for n, a in ops.sequence(kind, seed) if n in ("iterate", "run")}
    assert any(k % 2 for k in lengths) and any(k % 2 == 0 for k in lengths)
    runs = [a for seed in ops.seeds(kind) for n, a in ops.sequence(kind, seed) if n == "run"]
    assert {e for k, e in runs if e in (0, 1, 2)} == {0, 1, 2} and any(e == k > 2 for k, e in runs)      # every in {0, 1, 2, k}


@pytest.mark.parametrize("kind,seed", ops.CASES)
def test_no_decision_of_a_sequence_is_near_its_threshold(built, kind, seed):
    """Every comparison of the stopping rule (r against e_pri, s against e_dua) and of the adaptive rule (R against mu^2 S, S
    against mu^2 R) along the model's run stays a relative 1e-6 away from its threshold: rounding-level differences on the GPU
    cannot flip a decision.  A condition on the committed inputs (other seeds are picked until it holds), not a tolerance."""
    model, log = _model_run(kind, seed)
    assert model.iterations <= ops.MAX_ITERATIONS
    if ops.KINDS[kind].get("solve", True):
        assert model.margins
    for what, lhs, thr in model.margins:
        assert abs(lhs - thr) > 1e-6 * max(abs(lhs), abs(thr)), (what, lhs, thr)
    # what the model refuses: the refused class, and a residual read-out before any residual iteration
    for i, name, args, out, code in log:
        refused = name.startswith("refuse_") or (name == "residuals" and out is None)
        assert (code is not None) == refused, (i, name, args, code)
    assert all(np.all(np.isfinite(a)) for a in model.get())


def test_the_sequences_exercise_the_rules(built):
    """Some solve of the adaptive kinds changes rho, some QPs converge and some do not, and per-QP rho values move apart."""
    changed = converged = open_ = apart = 0
    for kind in ("with_q_two_blocks", "thrust_bound", "pinst_lane_per_qp"):
        for seed in ops.seeds(kind):
            model, log = _model_run(kind, seed)
            for _, name, _, out, _ in log:
                if out and "info" in out:
                    changed += out["info"]["rho_updates"]
                    converged += int(out["info"]["status"].sum())
                    open_ += int((out["info"]["status"] == 0).sum())
            apart += len(set(model.rho_per_qp())) > 1
    assert changed > 0 and converged > 0 and open_ > 0 and apart > 0, (changed, converged, open_, apart)
