"""The host model of a handle (tests/_handle_model.py) and the committed call sequences (tests/_op_sequences.py), pinned without a
GPU: the model against the oracles it is built from, the sequences' coverage of ops and of neighbouring op classes, and the
distance of every stopping-rule / adaptive-rule decision along them from its threshold."""
import dataclasses
import functools
import hashlib

import numpy as np
import pytest

import admm_library_amd as pkg
import oracle_c as oc
import _consensus_ref as cs
import _fuel_ref as fr
import _infeas_ref as ir
import _op_sequences as ops
import _soft_ref as sr
from _handle_model import INVALID, UNSUPPORTED, HandleModel, Refused
from admm_library_amd import mpc

SOLVE = dict(eps_abs=1e-3, eps_rel=1e-3, max_iter=60, check_interval=5)
ADAPT = dict(adapt_interval=5, adapt_mu=2.0, adapt_tau=2.0, adapt_max=16)


def _problems():
    fuel = ops.problem("fuel_thrust_bound")
    return {"shared": pkg.random_ltv(N=12, n=4, m=2, batch=7, seed=3),
            "thrust": pkg.random_ltv(N=11, n=6, m=3, batch=5, seed=4, thrust_norm=True),
            "fuel": fuel,
            "per_instance": pkg.random_instances(N=10, n=4, m=2, batch=6, seed=5)}


def _oracle(p, **kw):
    if p.fuel is not None or p.soft is not None or p.consensus is not None:
        r = (sr if p.soft is not None else cs if p.consensus is not None else fr).solve(p, **kw)
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


# ---- soft weights, scenario groups, the receding-horizon step, the probe ----

def _ext_problems():
    from test_soft_host import random_soft
    base = pkg.random_ltv(N=12, n=4, m=2, batch=6, seed=3)
    return {"soft": dataclasses.replace(base, soft=random_soft(base)),
            "consensus": dataclasses.replace(base, consensus=3),
            "soft_fuel": ops.problem("soft_fuel_thrust")}


EXT = ["soft", "consensus", "soft_fuel"]


@pytest.mark.parametrize("alpha", [1.0, 1.6])
@pytest.mark.parametrize("name", EXT)
def test_ext_iterate_and_run_compose_to_one_reference_run(built, name, alpha):
    p = _ext_problems()[name]
    m = HandleModel(p, pkg.Options(rho=0.3, alpha=alpha))
    assert not m.fused
    calls = [("iterate", 1), ("run", 4, 3), ("run", 1, 2), ("iterate", 6), ("run", 9, 1), ("run", 7, 0), ("run", 5, 5)]
    total = 0
    for c in calls:
        getattr(m, c[0])(*c[1:])
        total += c[1]
        assert m.pair_form
    ref = _oracle(p, rho=0.3, alpha=alpha, max_iter=total, check_interval=total, stop=False)
    assert m.iterations == total
    for k, a in zip(("w", "z", "y"), m.get()):
        assert _same(a, ref[k]), k
    assert _same(m.residuals()[0], ref["r"]) and _same(m.residuals()[1], ref["s"])


@pytest.mark.parametrize("alpha", [1.0, 1.6])
@pytest.mark.parametrize("name", EXT)
def test_ext_step_x_then_step_z_is_one_iteration(built, name, alpha):
    p = _ext_problems()[name]
    a, b = HandleModel(p, pkg.Options(rho=0.3, alpha=alpha)), HandleModel(p, pkg.Options(rho=0.3, alpha=alpha))
    a.iterate(3)
    b.iterate(3)
    a.run(1, 1)
    b.step_x()
    b.step_z(True)
    for x, y in zip(a.get() + a.residuals(), b.get() + b.residuals()):
        assert _same(y, x)


@pytest.mark.parametrize("name", EXT)
def test_ext_solve_is_the_references_solve(built, name):
    p = _ext_problems()[name]
    opt = pkg.Options(rho=0.3, **SOLVE, **ADAPT)
    m = HandleModel(p, opt)
    m.iterate(3)
    z0, y0 = m.z.copy(), m.y.copy()
    info = m.solve()
    ref = _oracle(p, rho=0.3, z0=z0, y0=y0, stop=True, **SOLVE, **ADAPT)
    assert info["iters_run"] == ref["iters_run"]
    assert np.array_equal(info["iters"], ref["iters"]) and np.array_equal(info["status"], ref["status"])
    assert m.rho == ref["rho"] and info["rho_updates"] == ref["rho_updates"] and info["rho_updates"] >= 1
    for k, a in zip(("w", "z", "y"), m.get()):
        assert _same(a, ref[k]), k


@pytest.mark.parametrize("name", EXT)
def test_ext_set_rho_reproduces_an_adaptive_solve(built, name):
    p = _ext_problems()[name]
    kw = dict(rho=0.3, max_iter=40, check_interval=5, stop=False, **ADAPT)
    ref = _oracle(p, **kw)
    assert ref["rho_updates"] >= 1
    rho_after = {T: _oracle(p, **dict(kw, max_iter=T + 1))["rho"] for T in range(5, 40, 5)}
    m = HandleModel(p, pkg.Options(rho=0.3))
    for T in range(5, 45, 5):
        m.iterate(5)
        if T in rho_after:
            m.set_rho(rho_after[T])
    assert m.rho == ref["rho"]
    for k, a in zip(("w", "z", "y"), m.get()):
        assert _same(a, ref[k]), k


@pytest.mark.parametrize("tail", ["copy", "zero"])
@pytest.mark.parametrize("name", ["shared", "thrust", "fuel", "soft", "soft_fuel"])
def test_mpc_advance_is_get_shift_update_set_state(built, name, tail):
    """The defining property of admm_mpc_advance (admm_library_amd/mpc.py), bit for bit: with du, dx and a plant; with x_meas and
    q_tail (on a problem with q)."""
    p = dict(_problems(), **_ext_problems())[name]
    rng = np.random.default_rng(5)
    a, b = HandleModel(p, pkg.Options(rho=0.3)), HandleModel(p, pkg.Options(rho=0.3))
    for step in range(2):
        a.run(4, 2)
        b.run(4, 2)
        du, dx = 0.05 * rng.standard_normal((p.batch, p.m)), 0.02 * rng.standard_normal((p.batch, p.n))
        A0, B0 = mpc.model_plant(p)
        plant = (A0 * 1.01, B0 * 0.99)
        x_meas = rng.standard_normal((p.batch, p.n))
        q_tail = None if p.q is None else rng.standard_normal((p.batch, p.nb))
        kw = dict(du=du, dx=dx, plant=plant) if step == 0 else dict(x_meas=x_meas, q_tail=q_tail)
        out = a.mpc_advance(tail=tail, **kw)
        w, z, y = b.get()
        u = z[:, :p.m] + du if step == 0 else z[:, :p.m]
        xn = mpc.plant_step(b.p.x0, u, *plant, dx) if step == 0 else x_meas
        q = None if p.q is None else mpc.shift_horizon(b.p.q, p.nb, tail, None if step == 0 else q_tail)
        b.update_instances(xn, q)
        b.set_state(*(mpc.shift_horizon(v, p.nb, tail) for v in (w, z, y)))
        assert np.array_equal(out["u"], u) and np.array_equal(out["x_next"], xn)
        assert np.array_equal(a.p.x0, b.p.x0) and (p.q is None or np.array_equal(a.p.q, b.p.q))
        assert all(np.array_equal(x, y) for x, y in zip(a.get(), b.get())) and a.pair_form
    a.run(3, 3)
    b.run(3, 3)
    assert all(np.array_equal(x, y) for x, y in zip(a.get() + a.residuals(), b.get() + b.residuals()))


@pytest.mark.parametrize("name", ["shared", "thrust", "fuel", "soft", "soft_fuel"])
def test_infeasibility_is_the_probe_of_recorded_iterates(built, name):
    """One reference run with its iterates recorded at 6 and 6 + span; the model's probe is the reference's of the two y, on the
    problem with the rows of a finite soft weight opened, and the state afterwards that of run(span)."""
    import test_gpu_soft
    p = dict(_problems(), **_ext_problems())[name]
    span, eps = 5, 1e-6
    if p.fuel is not None or p.soft is not None:
        r = (sr if p.soft is not None else fr).solve(p, rho=0.3, max_iter=6 + span, check_interval=100, stop=False, record={6, 6 + span})
        (_, _, _, ya), (_, _, zb, yb) = r.history
    else:                                       # (the C oracle records nothing: the same run, left at 6 and at 6 + span)
        ya = _oracle(p, rho=0.3, max_iter=6, check_interval=100, stop=False)["y"]
        r = _oracle(p, rho=0.3, max_iter=6 + span, check_interval=100, stop=False)
        zb, yb = r["z"], r["y"]
    m = HandleModel(p, pkg.Options(rho=0.3))
    m.iterate(6)
    got = m.infeasibility(span, eps, True)
    opened = test_gpu_soft._opened(p) if p.soft is not None else p
    want = ir.probe(opened, ya, yb, span, eps)
    for k, v in want.items():
        assert np.array_equal(got[k], v), k
    assert np.array_equal(m.y, yb) and np.array_equal(m.z, zb) and m.iterations == 6 + span and m.pair_form == (not m.fused)
    if p.soft is not None:
        o = m.opened()
        assert np.array_equal(o.lo, opened.lo) and np.array_equal(o.hi, opened.hi) and o.soft is None
        assert np.isinf(o.lo).sum() > np.isinf(p.lo).sum()


def test_a_refused_new_op_leaves_the_model_alone(built):
    probs = _ext_problems()
    for name, p in probs.items():
        m = HandleModel(p, pkg.Options(rho=0.3))
        m.run(3, 1)
        before = [a.copy() for a in m.get() + m.residuals()]
        nan_du = np.zeros((p.batch, p.m))
        nan_du[0, 0] = np.nan
        calls = [(lambda: m.profile(1, False, 1), UNSUPPORTED), (lambda: m.infeasibility(0), INVALID)]
        if p.consensus is not None:
            calls += [(lambda: m.mpc_advance(), UNSUPPORTED), (lambda: m.infeasibility(3), UNSUPPORTED),
                      (lambda: m.set_soft(np.ones_like(p.lo)), INVALID), (lambda: m.soft_report(), INVALID)]
        else:
            neg = np.array(p.soft, np.float64)
            neg[np.isfinite(neg)] = -1.0
            calls += [(lambda: m.mpc_advance(x_meas=p.x0, dx=np.zeros_like(p.x0)), INVALID), (lambda: m.mpc_advance(du=nan_du), INVALID),
                      (lambda: m.mpc_advance(x_meas=p.x0, plant=mpc.model_plant(p)), INVALID), (lambda: m.set_soft(neg), INVALID),
                      (lambda: m.set_soft(np.where(np.isfinite(p.soft), np.nan, p.soft)), INVALID), (lambda: m.consensus(), INVALID)]
            if p.q is None:
                calls.append((lambda: m.mpc_advance(q_tail=np.zeros((p.batch, p.nb))), INVALID))
        if name == "soft_fuel":
            f = np.array(p.fuel, np.float64)
            f[ops.SOFT_FUEL_STAGE] = 0.1
            finite_on_ball = np.array(p.soft, np.float64)
            finite_on_ball[np.flatnonzero(np.isfinite(p.unorm))[0], 0] = 1.0
            calls += [(lambda: m.set_fuel(f), INVALID), (lambda: m.set_soft(finite_on_ball), INVALID)]
        for call, code in calls:
            with pytest.raises(Refused) as e:
                call()
            assert e.value.code == code
        assert m.p is p and all(np.array_equal(a, b) for a, b in zip(before, m.get() + m.residuals())) and not m.margins
    pi = HandleModel(_problems()["per_instance"], pkg.Options(rho=0.3))
    for call in (lambda: pi.mpc_advance(), lambda: pi.infeasibility(3)):
        with pytest.raises(Refused) as e:
            call()
        assert e.value.code == UNSUPPORTED


def test_update_problem_keeps_soft_weights_and_groups(built):
    for kind in ("soft_fuel_thrust", "consensus_G65_fuel"):
        m = ops.new_model(kind)
        p = m.p
        m.update_problem(ops.materialise(kind, "update_problem", (3,), m, None)["problem"])
        assert m.p.soft is p.soft and m.p.consensus == p.consensus and m.p.fuel is p.fuel and m.p.A is not p.A


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
        assert len(seq) == len(classes) ** 2 + 1 and len(seq) in (37, 50, 65)
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
    cannot flip a decision; so do the probe's decisions (sep against -eps, the open-row magnitude against eps |mu|_inf) on the kinds that
    draw it.  A condition on the committed inputs (other seeds are picked until it holds), not a tolerance."""
    model, log = _model_run(kind, seed)
    assert model.iterations <= ops.MAX_ITERATIONS
    if ops.KINDS[kind].get("solve", True):
        assert model.margins
    for what, lhs, thr in model.margins:
        assert abs(lhs - thr) > 1e-6 * max(abs(lhs), abs(thr)), (what, lhs, thr)
    # the probe's zero / nonzero decisions (mu = 0, lambda = 0): none within rounding of flipping -- but on the soft-box kinds, whose
    # persistently violated rows hold y = s / rho: a bounded share of the probed QPs there, and defect is not compared on them
    share = ops.KINDS[kind].get("stationary_rows")
    if share:
        assert len({(k, b) for k, _, b, _, _ in model.unclear}) <= share * model.probes * model.p.batch, len(model.unclear)
    else:
        assert not model.unclear, model.unclear[:5]
    # what the model refuses: the refused class, and a residual read-out before any residual iteration
    for i, name, args, out, code in log:
        refused = name.startswith("refuse_") or (name == "residuals" and out is None)
        assert (code is not None) == refused, (i, name, args, code)
    assert all(np.all(np.isfinite(a)) for a in model.get())


def test_the_old_kinds_keep_their_sequences():
    """The kinds that predate ext=True draw what they drew: sha256 of repr(sequence(kind, seed)), taken before the flag existed."""
    old = [(kind, seed) for kind in ops.OLD_KINDS for seed in ops.seeds(kind)]
    assert sorted(ops.DIGESTS) == sorted(old) and len(old) == 57
    for kind, seed in old:
        assert not ops.KINDS[kind].get("ext")
        assert hashlib.sha256(repr(ops.sequence(kind, seed)).encode()).hexdigest() == ops.DIGESTS[kind, seed], (kind, seed)


def test_the_new_kinds_are_what_they_are_for(built):
    """Set-up facts of the kinds with ext=True that need no GPU."""
    assert len(ops.NEW_KINDS) == 16 and all(ops.KINDS[k].get("ext") and len(ops.seeds(k)) == 3 for k in ops.NEW_KINDS)
    p = ops.problem("consensus_wide")
    assert p.m == 6 and p.consensus > 256 and p.batch == 2 * p.consensus     # a group wider than the tile of m = 6: the two-pass route
    p = ops.problem("soft_box_relaxed")
    assert p.L % 8 and (p.L % 8) % 4 and p.batch % 2 and p.q is not None     # a short last chunk, no multiple of 4; a pad column
    for kind in ops.NEW_KINDS:
        cfg, classes = ops.KINDS[kind], ops.classes_of(kind)
        assert ("probe" in classes) == (not cfg.get("consensus"))
        names = {n for ns in ops.legal_ops(kind).values() for n in ns}
        assert ("set_soft" in names) == bool(cfg.get("soft")) and ("consensus" in names) == bool(cfg.get("consensus"))
        assert ("mpc_advance" in names) == (not cfg.get("consensus")) and ("refuse_mpc" in names) == bool(cfg.get("consensus"))


def test_the_new_sequences_exercise_what_they_are_for(built):
    """Over the committed seeds of the kinds with ext=True: probes with a finite sep and with +inf; flags of both values in each
    probe_* kind and in soft_probe_corridor (a flag of 1 there: the corridor rows were made hard by admm_set_soft); soft reports with and without violated rows, every finite-weight row of every report clear of its decisions; a rho
    change inside a solve of a soft kind and of a consensus kind; every new refused op refused with the code of include/admm_hip.h."""
    codes = {"refuse_mpc_xmeas_and_dx": INVALID, "refuse_mpc_nan_du": INVALID, "refuse_mpc_qtail_without_q": INVALID,
             "refuse_set_soft_neg": INVALID, "refuse_set_fuel_on_soft_rows": INVALID, "refuse_profile_fused": UNSUPPORTED,
             "refuse_mpc": UNSUPPORTED, "refuse_probe": UNSUPPORTED}
    seen, finite, infinite, viol, clean = set(), 0, 0, 0, 0
    flags = {k: set() for k in ("probe_di_position_box", "probe_di_pinned", "soft_probe_corridor")}
    rho_in_solve = {"soft": 0, "consensus": 0}
    for kind in ops.NEW_KINDS:
        cfg = ops.KINDS[kind]
        for seed in ops.seeds(kind):
            model, log = _model_run(kind, seed)
            assert all(bad == 0 for rows, bad in model.soft_rows), (kind, seed, model.soft_rows)
            for i, name, args, out, code in log:
                if name in codes:
                    assert code == codes[name], (kind, seed, i, name, code)
                    seen.add(name)
                if out and "probe" in out:
                    finite += int(np.isfinite(out["probe"]["sep"]).sum())
                    infinite += int(np.isinf(out["probe"]["sep"]).sum())
                    if kind in flags:
                        flags[kind] |= set(out["probe"]["infeasible"].tolist())
                if out and "soft_report" in out:
                    viol += int(out["soft_report"]["n_violated"].sum() > 0)
                    clean += int(out["soft_report"]["n_violated"].sum() == 0)
                if out and "info" in out:
                    for k in rho_in_solve:
                        rho_in_solve[k] += out["info"]["rho_updates"] if cfg.get(k) else 0
                if out and "mpc" in out:
                    seen.add("mpc")
    assert seen == set(codes) | {"mpc"}, set(codes) - seen
    assert finite > 0 and infinite > 0 and viol > 0 and clean > 0, (finite, infinite, viol, clean)
    assert all(v == {0, 1} for v in flags.values()), flags
    assert all(v > 0 for v in rho_in_solve.values()), rho_in_solve


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
