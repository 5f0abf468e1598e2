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
import _cone_ref as cn
import _consensus_ref as cs
import _fuel_ref as fr
import _halfspace_ref as hr
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
    if p.fuel is not None or p.z_kind is not None:
        r = {"soft": sr, "consensus": cs, "halfspace": hr, "cone": cn, None: fr}[p.z_kind].solve(p, **kw)
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


def _plane_problems():
    from test_cone_host import random_cones
    from test_halfspace_host import random_planes
    base = pkg.random_ltv(N=12, n=4, m=2, batch=6, seed=3)
    return {"halfspace": random_planes(base, 2, True), "cone": random_cones(base, 2, False),
            "halfspace_fuel": ops.problem("halfspace_perqp_fuel"), "cone_fuel": ops.problem("cone_perqp_fuel")}


def _all_ext():
    return dict(_ext_problems(), **_plane_problems())


PLANES = ["halfspace", "cone", "halfspace_fuel", "cone_fuel"]
EXT = ["soft", "consensus", "soft_fuel"] + PLANES


@pytest.mark.parametrize("alpha", [1.0, 1.6])
@pytest.mark.parametrize("name", EXT)
def test_ext_iterate_and_run_compose_to_one_reference_run(built, name, alpha):
    p = _all_ext()[name]
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
    p = _all_ext()[name]
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
    p = _all_ext()[name]
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
    p = _all_ext()[name]
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


@pytest.mark.parametrize("name", PLANES)
def test_a_refused_plane_op_leaves_the_model_alone(built, name):
    """Every refusal of admm_set_halfspace* / admm_set_cone* (a NaN, an a'a / c'c that is no normal number, a slope that is none, a
    closed box under the new payload, another form, a handle of another kind), of admm_update_problem (a closed box under a payload
    in force), and the calls such a handle does not have."""
    p = _plane_problems()[name]
    cone = p.z_kind == "cone"
    m = HandleModel(p, pkg.Options(rho=0.3))
    assert not m.fused
    m.run(3, 1)
    before = [a.copy() for a in m.get() + m.residuals()]
    edge = m._edge.copy()
    pay = [np.array(a, np.float64) for a in ops.plane_payload(p)]
    nh, N = ops.plane_nh(p), p.N

    def changed(i, where, value):
        arrs = [a.copy() for a in pay]
        arrs[i].reshape((-1, N) + arrs[i].shape[pay[0].ndim - 1:])[where] = value
        return arrs
    live = int(np.flatnonzero(np.any(pay[0].reshape(-1, N, nh) != 0, axis=(0, 2)))[0])
    bad = [changed(0, (0, live, 0), np.nan), changed(1, (0, live), np.inf), changed(0, (0, live), 1e-170 * np.eye(1, nh)[0]),
           changed(0, (0, 2, 0), 1.0), [a[..., :-1] for a in pay] if pay[0].ndim == 2 else [a[:-1] for a in pay]]
    if cone:
        bad += [changed(2, (0, live), g) for g in (0.0, -0.5, 1e-310, 1e200, np.nan)]
    setter = m.set_cone if cone else m.set_halfspace
    calls = [((lambda arrs=arrs: setter(*arrs)), INVALID) for arrs in bad]
    closed = dataclasses.replace(p, lo=np.array(p.lo), **ops._DROP)
    closed.lo[live, p.m + nh - 1] = -5.0
    other = (m.set_halfspace, (pay[0], pay[1])) if cone else (m.set_cone, (pay[0], pay[0], pay[1]))
    calls += [(lambda: m.update_problem(closed), INVALID), (lambda: other[0](*other[1]), INVALID),
              (lambda: (m.halfspace if cone else m.cone)(), INVALID), (lambda: (m.halfspace_report if cone else m.cone_report)(), INVALID),
              (lambda: m.set_soft(np.ones_like(p.lo)), INVALID), (lambda: m.consensus(), INVALID),
              (lambda: m.mpc_advance(), UNSUPPORTED), (lambda: m.infeasibility(3), UNSUPPORTED), (lambda: m.infeasibility(0), INVALID),
              (lambda: m.profile(1, False, 1), UNSUPPORTED)]
    for i, (call, code) in enumerate(calls):
        with pytest.raises(Refused) as e:
            call()
        assert e.value.code == code, i
    assert m.p is p and all(np.array_equal(a, b) for a, b in zip(before, m.get() + m.residuals())) and not m.margins
    assert np.array_equal(edge, m._edge) and not m.plane_stages
    # a stage without a plane / cone: its slope and its box are not looked at; a payload on a dormant stage is accepted
    ok = changed(0, (slice(None), live), 0.0)
    if cone:
        ok[2].reshape(-1, N)[:, live] = -1.0
    setter(*ok)
    assert all(np.array_equal(a, b) for a, b in zip((m.cone if cone else m.halfspace)(), ok)) and m.p is not p
    m.update_problem(closed)                    # ... and the box of that stage may close now


def test_update_problem_keeps_planes_and_cones(built):
    for kind in ("halfspace_perqp_fuel", "cone_shared_relaxed"):
        m = ops.new_model(kind)
        p = m.p
        new = ops.materialise(kind, "update_problem", (3,), m, None)["problem"]
        assert new.z_kind is None and new.fuel is None
        m.update_problem(new)
        assert all(a is b for a, b in zip(ops.plane_payload(m.p), ops.plane_payload(p))) and m.p.fuel is p.fuel and m.p.A is not p.A
        assert m.p.z_kind == p.z_kind
        # the open-box rule is re-checked with the stages of the payload in force, not with those of set-up
        full = ops.new_payload(kind, 1.0, 5)
        gained = np.any(full[0].reshape(-1, p.N, ops.plane_nh(p)) != 0, axis=(0, 2)) & ops.dormant_stages(p.N)
        assert gained.any()
        closed = dataclasses.replace(new, lo=np.array(new.lo))
        closed.lo[np.flatnonzero(gained)[0], p.m] = -5.0
        m.update_problem(closed)                # dormant at set-up: its box may close
        m.update_problem(new)
        (m.set_cone if p.z_kind == "cone" else m.set_halfspace)(*full)
        with pytest.raises(Refused) as e:
            m.update_problem(closed)
        assert e.value.code == INVALID


def test_the_unclear_stage_rule(built):
    """A z-update input put on a plane, and on a cone's surface, marks the stage; one put clear of them does not; set_state with a y
    clears the marks; a multiplier of rounding size is unclear at the report."""
    for name in ("halfspace", "cone"):
        p = _plane_problems()[name]
        m = HandleModel(p, pkg.Options(rho=0.3))
        m.iterate(2)
        nh = ops.plane_nh(p)
        rep = (m.halfspace_report if name == "halfspace" else m.cone_report)
        base = rep()["unclear"].sum()
        k = int(np.flatnonzero(np.any(np.asarray(ops.plane_payload(p)[0]).reshape(-1, p.N, nh) != 0, axis=(0, 2)))[0])
        rows = slice(k * p.nb + p.m, k * p.nb + p.m + nh)
        if name == "halfspace":
            a, b = hr.planes(p)
            on = a[0, k] * b[0, k] / (a[0, k] @ a[0, k])                    # a point of the plane
        else:
            c, apex, g = cn.cones(p)
            e = c[0, k] / np.linalg.norm(c[0, k])
            on = apex[0, k] + 1.0 * e + g[0, k] * np.array([-e[1], e[0]])   # s = 1, r = g: on the surface (nh = 2)
        w = m.w.copy()
        w[0, rows] = on * (1.0 + 1e-9)
        m.set_state(w=w, y=np.zeros_like(m.y))
        m.alpha = 1.0
        m.step_z()                              # v = w
        assert m._edge[0, k] and m._edge.sum() <= 1 + base
        r = rep()
        assert r["unclear"][0] >= 1 and m.plane_stages[-1][1] >= 1
        m.set_state(y=m.y)
        assert not m._edge.any()
        w[0, rows] = on * 1.01
        m.set_state(w=w, y=np.zeros_like(m.y))
        m.step_z()
        assert not m._edge[0, k]
        y = np.zeros_like(m.y)
        y[0, rows] = 1e-9 * (a[0, k] if name == "halfspace" else np.ones(nh))  # 0 < lam <= 1e-6: a decision rounding could flip
        m.set_state(y=y)
        assert rep()["unclear"][0] == 1


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


def test_the_ext_kinds_keep_their_sequences():
    """The kinds with ext=True that predate the half-space and cone kinds draw what they drew: sha256 of repr(sequence(kind, seed)),
    taken before legal_ops() and sequence() learnt the new ops."""
    ext = [(kind, seed) for kind in ops.NEW_KINDS for seed in ops.seeds(kind)]
    assert sorted(ops.EXT_DIGESTS) == sorted(ext) and len(ext) == 48
    for kind, seed in ext:
        assert ops.KINDS[kind].get("ext") and not ops.KINDS[kind].get("plane")
        assert hashlib.sha256(repr(ops.sequence(kind, seed)).encode()).hexdigest() == ops.EXT_DIGESTS[kind, seed], (kind, seed)
    assert list(ops.KINDS) == list(ops.OLD_KINDS + ops.NEW_KINDS + ops.PLANE_KINDS)


def test_the_plane_kinds_are_what_they_are_for(built):
    """Set-up facts of the half-space and cone kinds that need no GPU: the shapes behind the z kernel's geometry, the closed, open
    and dormant stages, and the classes and ops of such a handle."""
    assert len(ops.PLANE_KINDS) == 6 and all(len(ops.seeds(k)) == 3 for k in ops.PLANE_KINDS)
    for kind in ops.PLANE_KINDS:
        cfg, p = ops.KINDS[kind], ops.problem(kind)
        assert cfg["ext"] and cfg["unfused"] and cfg["family"] == "one_lane_fp64" and p.z_kind == cfg["plane"]
        assert "probe" not in ops.classes_of(kind) and len(ops.classes_of(kind)) == 7
        nh, N, m = ops.plane_nh(p), p.N, p.m
        live = np.any(np.asarray(ops.plane_payload(p)[0]).reshape(-1, N, nh) != 0, axis=(0, 2))
        closed, dormant = ops.closed_stages(N), ops.dormant_stages(N)
        assert np.array_equal(live, ~closed & ~dormant) and 0.25 <= dormant.sum() / (~closed).sum() <= 0.4
        for variant in range(1, 6):             # the box of every variant: open on the open stages, closed on the others
            q = ops.problem(kind, variant)
            assert np.all(q.lo[~closed, m:m + nh] == -np.inf) and np.all(q.hi[~closed, m:m + nh] == np.inf)
            assert np.all(np.isfinite(q.lo[closed, m:m + nh]).any(axis=1) | np.isfinite(q.hi[closed, m:m + nh]).any(axis=1))
        names = {n for ns in ops.legal_ops(kind).values() for n in ns}
        x = cfg["plane"]
        assert {f"set_{x}", f"get_{x}", f"{x}_report", f"{x}_report_device", "refuse_mpc", "refuse_probe", "refuse_profile_fused",
                "refuse_update_closed_box", f"refuse_set_{x}_closed_box", f"refuse_set_{x}_nan"} <= names
        assert ("refuse_set_cone_gamma" in names) == (x == "cone") and "mpc_advance" not in names and "infeasibility" not in names
        assert (f"set_{x}_device" in names) == (f"refuse_set_{x}_nan_device" in names) == bool(cfg.get("device_io"))
        other = "cone" if x == "halfspace" else "halfspace"
        assert not any(other in n for n in names)
    for kind in ops.OLD_KINDS + ops.NEW_KINDS:  # the new ops are absent from the sequences of every other kind
        assert not any("halfspace" in n or "cone" in n or n == "refuse_update_closed_box" for ns in ops.legal_ops(kind).values() for n in ns)
    for x in ("halfspace", "cone"):
        p = ops.problem(f"{x}_shared_relaxed")  # a pad column; chunks of 4 blocks, the last of one
        opt = ops.options(f"{x}_shared_relaxed")
        assert p.batch % 2 and opt.zrows == 4 * p.nb and p.N % 4 == 1 and p.q is not None and opt.alpha == 1.6 and opt.adapt_interval > 0
        assert np.ndim(ops.plane_payload(p)[0]) == 2
        p = ops.problem(f"{x}_perqp_fuel")      # two blocks per chunk beside the ball and the fuel shrink, the last of one
        opt = ops.options(f"{x}_perqp_fuel")
        assert opt.zrows == 2 * p.nb and p.N % 2 == 1 and p.fuel is not None and np.isfinite(p.unorm).any() and np.ndim(ops.plane_payload(p)[0]) == 3
        p = ops.problem(f"{x}_perqp_graph")     # a second workgroup along the batch (512 columns each, two QPs per lane)
        assert p.batch > 512 and ops.options(f"{x}_perqp_graph").flags & ops.F.FLAG_GRAPH and np.ndim(ops.plane_payload(p)[0]) == 3


def test_the_plane_sequences_exercise_what_they_are_for(built):
    """Over the committed seeds of the half-space and cone kinds: every new refused op refused with the code of include/admm_hip.h; in
    every kind a stage gains and a stage loses its plane / cone; all three branches of the cone's projection at the z-updates of
    every cone kind, active and satisfied planes at those of every half-space kind; reports with n_active > 0 and with
    max_violation > 0, with and without lam; a rho change inside a solve of a half-space kind and of a cone kind; and no unclear
    stage in any report (a condition on the committed seeds, as the margins are: other seeds are picked until it holds)."""
    codes = {"refuse_mpc": UNSUPPORTED, "refuse_probe": UNSUPPORTED, "refuse_profile_fused": UNSUPPORTED, "refuse_update_closed_box": INVALID,
             "refuse_set_cone_gamma": INVALID, "refuse_set_cone_gamma_device": INVALID}
    for x in ("halfspace", "cone"):
        for r in ("closed_box", "nan"):
            codes.update({f"refuse_set_{x}_{r}": INVALID, f"refuse_set_{x}_{r}_device": INVALID})
    seen = set()
    rho_in_solve = {"halfspace": 0, "cone": 0}
    for kind in ops.PLANE_KINDS:
        cfg = ops.KINDS[kind]
        x = cfg["plane"]
        gained = lost = active = viol = with_lam = without = gets = 0
        kinds = []
        for seed in ops.seeds(kind):
            model, log = _model_run(kind, seed)
            share = cfg.get("unclear_stages", 0.0)
            assert share <= 0.02 and model.plane_stages
            assert all(bad <= share * stages for stages, bad in model.plane_stages), (kind, seed, model.plane_stages)
            kinds += model.z_stage_kinds
            m2 = ops.new_model(kind)            # the stages with a plane / cone before and after every accepted admm_set_*
            for i, name, args, out, code in log:
                if name in codes:
                    assert code == codes[name], (kind, seed, i, name, code)
                    seen.add(name)
                if name in ops.SET_PLANE:
                    assert code is None
                    N, nh = m2.p.N, ops.plane_nh(m2.p)
                    old = np.any(np.asarray(ops.plane_payload(m2.p)[0]).reshape(-1, N, nh) != 0, axis=(0, 2))
                    new = ops.new_payload(kind, *args)
                    getattr(m2, "set_" + x)(*new)
                    now = np.any(new[0].reshape(-1, N, nh) != 0, axis=(0, 2))
                    gained += int((now & ~old).sum())
                    lost += int((old & ~now).sum())
                    assert not now[ops.closed_stages(N)].any()
                if out and "payload" in out:
                    gets += 1
                if out and "plane_report" in out:
                    r = out["plane_report"]
                    active += int(r["n_active"].sum() > 0)
                    viol += int(r["max_violation"].max() > 0)
                    with_lam += r["with_lam"]
                    without += not r["with_lam"]
                if out and "info" in out:
                    rho_in_solve[x] += out["info"]["rho_updates"]
        assert gained > 0 and lost > 0 and active > 0 and viol > 0 and with_lam > 0 and without > 0 and gets > 0, \
            (kind, gained, lost, active, viol, with_lam, without, gets)
        total = np.sum(kinds, axis=0)
        assert len(total) == (4 if x == "cone" else 3) and (total > 0).all(), (kind, total)     # every branch, and stages without
    assert seen == set(codes), set(codes) - seen
    assert all(v > 0 for v in rho_in_solve.values()), rho_in_solve


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
