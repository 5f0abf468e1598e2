"""admm_update_problem calls that change the KIND of a live handle's problem -- state rows opened or closed, LTI <-> LTV data, a
shared <-> per-stage box, a thrust bound that moves between stages, a problem that fails the forward-elimination gate -- and
admm_set_state with duals on open state rows, on a handle that holds a warm state in one of its hidden forms
(tests/_update_structure.py: the cases, the script of calls, the reference; tests/test_update_structure_host.py: the conditions on
the inputs).

Per case: the script runs on a Solver; every read-out is compared with the host model (the oracle chain): iterates and residual
norms within 1e-10 x max(1, |ref|_inf) (1e-5 in the mixed mode, tests/test_gpu_mfma.py), the certificate on the scales
of tests/test_gpu_cert.py, iteration counts, rho_updates, rho and status of a full adaptive solve exactly.  After every update the
path is asserted (xfree follows the new box; alternating follows the gate until it first fails and stays off afterwards; the
RuntimeWarning comes exactly at the failing call), and a FRESH twin handle of the new problem, given the updated handle's (w, z, y),
is driven through the same calls: equal bit for bit (s within S_TOL of tests/test_gpu_lean_resid.py where a lean iteration ran) --
but after a gate failure, where the updated handle stays on the plain kernels and the fresh one does not.
"""
import dataclasses
import types
import warnings

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: one HIP runtime in the process)

import admm_library_amd as pkg
from admm_library_amd import mpc
from admm_library_amd.solver import AdmmError

import _infeas_cases as ic
import _timeshard as ts
import _update_structure as us
import test_gpu_sequences as tgs
from _handle_model import INVALID, HandleModel
from test_gpu_lean_resid import S_TOL

pytestmark = pytest.mark.gpu

CASES = us.cases()
SINGLE = [c for c in CASES if "world" not in us.KINDS[c.kind]]
SHARDED = [c for c in CASES if "world" in us.KINDS[c.kind]]
U = 2.0 ** -53
_COVER = {"lean": 0, "xfree2": 0, "graph": 0, "mfma": 0}       # forms launched AFTER an update, over the cases run so far


def _quiet(call, *args, **kw):
    """call(...) -> (result, the RuntimeWarnings it raised)."""
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = call(*args, **kw)
    return out, [w for w in caught if issubclass(w.category, RuntimeWarning)]


def _read(s, name):
    if name == "get":
        return dict(zip(("w", "z", "y"), s.get()))
    if name == "residuals":
        return dict(resid=s.residuals())
    if name == "certificate":
        return dict(cert=s.certificate(costates=True))
    raise KeyError(name)


class _Twin:
    """A fresh handle of the updated handle's problem, started from its (w, z, y) and driven through the same calls."""

    def __init__(self, s, opt):
        self.s, _ = _quiet(pkg.Solver, s.problem, opt)
        self.s.set_state(*s.get())
        self.lean0 = (s.lean_iterations(), self.s.lean_iterations())
        self.has_resid = False

    def close(self):
        self.s.close()

    def compare(self, s, name, what):
        if name == "residuals" and not self.has_resid:
            return                                         # (a fresh handle has none before its first residual iteration)
        got, want = _read(s, name), _read(self.s, name)
        lean = s.lean_iterations() > self.lean0[0] or self.s.lean_iterations() > self.lean0[1]
        if name == "get":
            for k in ("w", "z", "y"):
                assert np.array_equal(got[k], want[k]), f"{what}: {k} of the updated handle differs from the fresh twin's by {np.abs(got[k] - want[k]).max():.3e}"
        elif name == "residuals":
            for k, a, b in zip(("r", "s", "nw", "nz", "ny"), got["resid"], want["resid"]):
                if k == "s" and lean:
                    assert np.abs(a - b).max() <= S_TOL * max(np.abs(b).max(), 1e-300), (what, k, np.abs(a - b).max())
                else:
                    assert np.array_equal(a, b), f"{what}: residual norm {k} differs from the fresh twin's by {np.abs(a - b).max():.3e}"


def _run_case(case):
    ref, probs, opt, cfg, script = us.reference(case), us.problems(case), us.options(case), us.KINDS[case.kind], us.script(case)
    tol = cfg.get("tol", 1e-10)
    ok, ok_after = us.alt_ok_expected(case)
    s, warned = _quiet(pkg.Solver, probs[0], opt)
    twin = None
    try:
        path = s.path()
        print(us.cid(case), path)
        requested = path["alt_requested"]
        alive = requested and ok[0]                        # the handle still alternates
        failed = requested and not ok[0]                   # the gate has failed once: the latch
        assert path["alternating"] == alive and bool(warned) == failed, (path, warned)
        assert path["segments"] == us.SEGMENTS and path["xfree"] == us.state_rows_open(probs[0])
        if alive and "family" in cfg:
            assert path["kernel_family"] == cfg["family"], path
        cur, lean_seen, last_z, updated = probs[0], 0, np.zeros((probs[0].batch, probs[0].L)), False
        for i, op in enumerate(script):
            name = op[0]
            what = f"{us.cid(case)} op {i} {op}"
            if name == "run":
                s.run(op[1], op[2])
                if twin:
                    twin.s.run(op[1], op[2])
                    twin.has_resid = twin.has_resid or (op[2] > 0 and op[1] // op[2] >= 1)
                if updated and alive:
                    p_ = s.path()
                    _COVER["xfree2"] += int(p_["xfree"] and op[2] == 0 and op[1] >= 3 and opt.alpha == 1.0 and not opt.flags & pkg._abi.FLAG_GRAPH)
                    _COVER["graph"] += int(bool(opt.flags & pkg._abi.FLAG_GRAPH) and op[1] >= 3)
                    _COVER["mfma"] += int(p_["kernel_family"] == "mfma_fp64")
            elif name in ("update", "set_rho"):
                good = ok[op[1]] if name == "update" else ok_after
                fails = alive and not good
                if name == "update":
                    _, warned = _quiet(s.update_problem, probs[op[1]])
                    cur, updated = probs[op[1]], True
                else:
                    _, warned = _quiet(s.set_rho, op[1])
                    if twin:
                        _quiet(twin.s.set_rho, op[1])
                # the RuntimeWarning exactly at the failing call, admm_last_warning empty at the others
                assert bool(warned) == fails and bool(s.last_warning) == fails, (what, [str(w.message) for w in warned], s.last_warning)
                if fails:
                    assert "forward-elimination" in s.last_warning
                alive, failed = alive and good, failed or fails
                path = s.path()
                assert path["alternating"] == alive, (what, path)
                assert path["xfree"] == us.state_rows_open(cur), (what, path)
                if alive and "family" in cfg:
                    assert path["kernel_family"] == cfg["family"], (what, path)
            elif name == "set_state_y":
                s.set_state(y=us.set_state_y(cur))
                updated = True
            elif name == "twin":
                if twin:
                    twin.close()
                twin = None if failed else _Twin(s, opt)
            elif name == "solve_begin":
                s.solve_begin()
            elif name == "solve":
                info, _ = _quiet(s.solve)                  # (a rho of the adaptive rule may fail the gate: a legal fall-back, warned)
                tgs._compare(dict(info=info), ref.log[i], None, tol)
                if twin and not s.last_warning:
                    info2, _ = _quiet(twin.s.solve)
                    assert (info.iters_run, info.rho, info.rho_updates) == (info2.iters_run, info2.rho, info2.rho_updates), what
                    assert np.array_equal(info.iters, info2.iters) and np.array_equal(info.status, info2.status), what
                    assert np.array_equal(info.r, info2.r), what
                elif twin:
                    twin.close()
                    twin = None
            elif name == "lean":
                n = s.lean_iterations()
                assert n > lean_seen, f"{what}: no lean iteration since the last guard ({n})"
                _COVER["lean"] += (n - lean_seen) if updated else 0
                lean_seen = n
            else:
                got = _read(s, name)
                if name == "get":
                    last_z = ref.log[i]["z"]
                try:
                    tgs._compare(got, ref.log[i], types.SimpleNamespace(p=cur, z=last_z), tol)
                except AssertionError as e:
                    raise AssertionError(f"{what} differs from the oracle chain: {e}\nscript: {script[:i + 1]}") from e
                if twin:
                    twin.compare(s, name, what)
    finally:
        s.close()
        if twin:
            twin.close()


@pytest.mark.parametrize("case", SINGLE, ids=[us.cid(c) for c in SINGLE])
def test_a_structure_changing_update_follows_the_chain_and_equals_a_fresh_twin(gpu, case):
    _run_case(case)
    print("forms launched after an update so far:", _COVER)


def test_the_lean_xfree_graph_and_mfma_forms_ran_after_updates(gpu):
    """Coverage guard, like test_the_lean_kind_runs_lean_iterations: over the cases, iterations AFTER an update ran in the lean
    residual forms (counted by the library), and calls were made whose launch rules take the XFREE = 2 forms (state rows open, three
    or more iterations without residuals, direct launches, alpha = 1), replay captured graphs, and run the fp64 MFMA kernels."""
    if not all(_COVER.values()):                           # (this test run on its own)
        for c in SINGLE:
            if (c.transition, c.kind) in (("open", "one_lane"), ("open", "graph"), ("open", "mfma_fp64")):
                _run_case(c)
    print(_COVER)
    assert all(v > 0 for v in _COVER.values()), _COVER


# ---- time shards ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", SHARDED, ids=[us.cid(c) for c in SHARDED])
def test_two_time_shards_follow_the_chain_through_the_update(gpu, case):
    """Two ranks as two threads (the exchange of tests/_timeshard.py): every rank makes the same calls, the update is local to each;
    the windows put together are the chain's iterates, the residual norms -- whole-horizon quantities -- are equal on both ranks."""
    ref, probs, script = us.reference(case), us.problems(case), us.script(case)
    cfg = us.KINDS[case.kind]
    opts = dataclasses.asdict(us.options(case))

    def work(s, rank):
        outs = []
        for op in script:
            if op[0] == "run":
                s.run(op[1], op[2])
            elif op[0] == "update":
                s.update_problem(probs[op[1]])
                assert s.path()["xfree"] == us.state_rows_open(probs[op[1]])
            elif op[0] == "set_rho":
                s.set_rho(op[1])
            elif op[0] == "get":
                outs.append(ts.read_into(s, np.nan))
            elif op[0] == "residuals":
                outs.append(s.residuals())
        return outs

    run = ts.run_ranks(probs[0], opts, cfg["world"], work)
    reads = [i for i, op in enumerate(script) if op[0] in ("get", "residuals")]
    assert all(len(o) == len(reads) for o in run.outs)
    nb = probs[0].nb
    for j, i in enumerate(reads):
        if script[i][0] == "get":
            full = ts.assemble([o[j] for o in run.outs], run.wins, nb)
            tgs._compare(dict(zip(("w", "z", "y"), full)), ref.log[i], None, 1e-10)
        else:                                              # r and s: the norms every rank holds for the whole horizon
            for o in run.outs:
                for k, g, r in zip(("r", "s"), o[j], ref.log[i]["resid"]):
                    tgs._close("residuals." + k, g, r, 1e-10)
                assert np.array_equal(o[j][0], run.outs[0][j][0]) and np.array_equal(o[j][1], run.outs[0][j][1])


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def _refusals():
    thrust, box, with_q = us.base("thrust", "n6m3"), us.base("one_lane", "n6m3"), us.base("with_q", "n6m3")
    lo, hi = box.lo.copy(), box.hi.copy()
    lo[5, :box.m], hi[5, :box.m] = -np.inf, np.inf
    un = np.full(box.N, np.inf)
    un[5] = 0.4
    return {
        "no_finite_unorm_left": ("thrust", thrust, dataclasses.replace(thrust, unorm=np.full(thrust.N, np.inf))),
        "unorm_on_a_box_handle": ("one_lane", box, dataclasses.replace(box, lo=lo, hi=hi, unorm=un)),
        "q_dropped": ("with_q", with_q, dataclasses.replace(with_q, q=None)),
        "another_N": ("one_lane", box, pkg.random_ltv(N=box.N + 1, n=box.n, m=box.m, batch=box.batch, seed=7, with_q=False)),
    }


@pytest.mark.parametrize("which", ["no_finite_unorm_left", "unorm_on_a_box_handle", "q_dropped", "another_N"])
def test_a_refused_update_leaves_the_handle_as_a_twin_that_never_made_the_call(gpu, which):
    kind, p, bad = _refusals()[which]
    bad.validate()                                         # a valid problem in itself: the HANDLE refuses it
    opt = us.options(us.Case("open", kind, "n6m3"))
    with pkg.Solver(p, opt) as s, pkg.Solver(p, opt) as twin:
        for h in (s, twin):
            h.run(7, 1)                                    # v-form, after a forward form, residuals held
        with pytest.raises(AdmmError) as e:
            s.update_problem(bad)
        assert e.value.code == INVALID, e.value
        assert "admm_update_problem" in str(e.value)
        assert s.problem is p and s.path() == twin.path()
        for h in (s, twin):
            h.run(4, 2)
        for a, b in zip(s.get() + s.residuals(), twin.get() + twin.residuals()):
            assert np.array_equal(a, b)


# ---- the read-outs that keep device copies of the problem -------------------------------------------------------------------

@pytest.mark.parametrize("kind", us.PROBE_KINDS)
def test_the_infeasibility_flags_follow_the_box(gpu, kind):
    """di_position_box of tests/_infeas_cases.py and its opened box, and back: QPs 1, 2, 3 are flagged under the corridor, none
    without it (tests/test_infeas_host.py establishes both with linprog); the probe's device copy of the box follows the update."""
    probs, opt = us.probe_problems(), us.probe_options(kind)
    ref = us.probe_reference(kind)
    with pkg.Solver(probs[0], opt) as s:
        for j, (p, (k, span), want, model_out) in enumerate(zip(probs, us.PROBE_RUNS, us.PROBE_FLAGS, ref.outs)):
            if j:
                s.update_problem(p)
                assert s.path()["xfree"] == us.state_rows_open(p)
            s.run(k, 0)
            got = s.infeasibility(span, ic.EPS, costates=True)
            assert got.infeasible.tolist() == want, (j, got.infeasible, got.sep)
            tgs._compare(dict(probe=got), dict(probe=model_out), None, 1e-10)


@pytest.mark.parametrize("direction", ["lti_ltv", "ltv_lti"])
def test_the_default_plant_of_mpc_advance_is_that_of_the_updated_problem(gpu, direction):
    """admm_mpc_advance with Ap = Bp = NULL reads A_0, B_0 from the handle's host copy: after an LTI <-> LTV update, p2's."""
    p = us.base("with_q", "n6m3")
    other = dataclasses.replace(p, A=np.ascontiguousarray(p.A[3]), B=np.ascontiguousarray(p.B[3]))     # LTI data that are NOT stage 0 of p
    p1, p2 = (other, p) if direction == "lti_ltv" else (p, other)
    A0, B0 = mpc.model_plant(p2)
    assert not np.array_equal(A0, mpc.model_plant(p1)[0])
    opt = us.options(us.Case(direction, "with_q", "n6m3"))
    model = HandleModel(p1, opt)
    s, _ = _quiet(pkg.Solver, p1, opt)                     # (whether the LTI data pass the gate is not this test's subject)
    with s:
        s.run(7, 1)
        model.run(7, 1)
        _quiet(s.update_problem, p2)
        model.update_problem(p2)
        s.run(3, 0)
        model.run(3, 0)
        z = s.get()[1]
        u, xn = s.mpc_advance()
        out = model.mpc_advance()
        assert np.array_equal(u, z[:, :p.m])
        want = mpc.plant_step(p2.x0, u, A0, B0, None)
        bound = 2 * (p.n + p.m + 1) * U * (np.abs(p2.x0) @ np.abs(A0).T + np.abs(u) @ np.abs(B0).T)      # test_gpu_mpc.py::test_outputs
        print("x_next: max err / bound", float((np.abs(xn - want) / bound).max()))
        assert (np.abs(xn - want) <= bound).all()
        tgs._compare(dict(mpc=dict(u=u, x_next=xn)), dict(mpc=out), None, 1e-10)
        s.run(4, 1)
        model.run(4, 1)
        tgs._compare(dict(zip(("w", "z", "y"), s.get()), resid=s.residuals()),
                     dict(zip(("w", "z", "y"), model.get()), resid=model.residuals()), None, 1e-10)
