"""Problem updates that change the STRUCTURE of a live handle's problem (tests/test_update_structure_host.py on the CPU,
tests/test_gpu_update_structure.py on the GPU): the cases, the script of calls each case runs, and the reference.  No GPU here.

A case is (transition, kind, shape).  The transition gives a list of problems p1, p2 (, p3): the handle is set up with p1 and moved
on by admm_update_problem; every problem after the first is built from its predecessor with dataclasses.replace, so only the named
structure changes (gate_fail_pass draws other dynamics: that is what it is about).  The kind gives the handle's options and what its
problems carry (q, a thrust bound, fuel weights, soft weights, scenario groups).

script(case) is the list of calls both sides make -- the Solver and the host model (tests/_handle_model.py, which is the oracle chain
of the parity tests: oracle_c.solve(..., z0=, y0=, max_iter=k, stop=False) leg after leg, tests/_fuel_ref, _soft_ref, _consensus_ref
on the handles they belong to, tests/_cert_ref for the certificate).  reference(case) runs it on the model, once per process.
"""
import collections
import dataclasses
import functools

import numpy as np

import admm_library_amd as pkg
from admm_library_amd import _abi as F

import _shapes
from _handle_model import HandleModel

RHO = 0.3
SEGMENTS = 4                      # given explicitly: a fresh twin handle runs the same count
BOX_SCALE = 0.25                  # of the state box of random_ltv: state rows are active on most QPs (the host test pins how many)
RHO_AFTER = 0.8                   # admm_set_rho at the end of the post-phase: a refactor from the handle's NEW host copy
SOLVE = dict(eps_abs=1e-3, eps_rel=1e-3, max_iter=40, check_interval=5)
ADAPT = dict(adapt_interval=5, adapt_mu=2.0, adapt_tau=2.0, adapt_max=16)
GATE_SEEDS = (41, 42)             # (6, 3), N = 33, 4 segments at rho = 0.3: 41 passes the forward-elimination gate, 42 fails it

# shape id -> (n, m, N, batch); the dynamics are those of random_ltv at the seed of _shapes.ALT_TABLE
SHAPES = {"n6m3": (6, 3, 33, 69), "n4m2": (4, 2, 30, 20), "n12m6": (12, 6, 24, 9), "n6m3b16": (6, 3, 33, 16),
          "n6m3N40": (6, 3, 40, 20)}

# Handle kinds.  opt: Options fields on top of rho / segments / SOLVE / ADAPT; shapes: where the kind runs; carries: what its
# problems hold; tol: iterates and residual norms (1e-10 x max(1, |ref|_inf); 1e-5 in the mixed mode, the file
# header of tests/test_gpu_mfma.py); lean: the lean residual forms apply once the state rows are open; solve: a full admm_solve
# is compared (the mixed mode refines in fp64 after an fp32 phase: its iteration counts are its own); unfused: the handle runs
# the unfused path; world: time shards, one thread per rank
KINDS = {
    "one_lane": dict(opt=dict(flags=F.FLAG_NO_MFMA), shapes=("n6m3", "n4m2", "n12m6"), family="one_lane_fp64", lean=True),
    "one_lane_relaxed": dict(opt=dict(flags=F.FLAG_NO_MFMA, alpha=1.6), shapes=("n6m3",), family="one_lane_fp64"),
    "with_q": dict(opt=dict(flags=F.FLAG_NO_MFMA), shapes=("n6m3", "n4m2"), carries=("q",), family="one_lane_fp64"),
    "graph": dict(opt=dict(flags=F.FLAG_NO_MFMA | F.FLAG_GRAPH), shapes=("n6m3",), family="one_lane_fp64"),
    "mfma_fp64": dict(opt=dict(precision_mode=F.PRECISION_FP64_MFMA), shapes=("n12m6", "n6m3b16"), family="mfma_fp64"),
    "mixed": dict(opt=dict(precision_mode=F.PRECISION_MIXED), shapes=("n6m3b16",), family="mfma_mixed", tol=1e-5, solve=False),
    "no_alternate": dict(opt=dict(flags=F.FLAG_NO_ALTERNATE), shapes=("n6m3",)),
    "unfused": dict(opt=dict(flags=F.FLAG_UNFUSED), shapes=("n6m3",), unfused=True),
    "thrust": dict(opt=dict(), shapes=("n6m3",), carries=("q", "thrust")),
    "fuel": dict(opt=dict(), shapes=("n6m3",), carries=("thrust", "fuel")),
    "soft": dict(opt=dict(), shapes=("n6m3",), carries=("soft",), unfused=True),
    "consensus": dict(opt=dict(alpha=1.6), shapes=("n6m3",), carries=("q", "consensus"), unfused=True),
    "timeshard": dict(opt=dict(flags=F.FLAG_NO_MFMA), shapes=("n6m3N40",), carries=("q",), world=2),
}

TRANSITIONS = ("open", "close", "open_partial", "lti_ltv", "ltv_lti", "box_shared_stage", "thrust_move", "gate_fail_pass",
               "set_state_open")

# (transition, kind) -> why the cell does not run; every other cell runs at every shape of its kind (gate_fail_pass: the (6, 3)
# shapes at N = 33 only, where the pair of GATE_SEEDS is known).  Written out: nothing is skipped by catching an error.
_TS_ONLY = "a time-sharded handle runs open, close and lti_ltv only"
_NO_THRUST = "the handle has no thrust bound"
SKIP = {}
for _t in ("open_partial", "ltv_lti", "box_shared_stage", "thrust_move", "gate_fail_pass", "set_state_open"):
    SKIP[_t, "timeshard"] = _TS_ONLY
for _k in KINDS:
    if "thrust" not in KINDS[_k].get("carries", ()):
        SKIP["thrust_move", _k] = _NO_THRUST
SKIP.update({
    # a fuel weight stays in force per stage and needs open control rows there: the box cannot move onto those stages
    ("thrust_move", "fuel"): "admm_update_problem keeps the fuel weights: a stage with a positive weight cannot take a control box",
    ("gate_fail_pass", "soft"): "soft and consensus handles run the unfused path only: they never alternate, there is no latch",
    ("gate_fail_pass", "consensus"): "soft and consensus handles run the unfused path only: they never alternate, there is no latch",
    ("gate_fail_pass", "no_alternate"): "ADMM_FLAG_NO_ALTERNATE: the handle never alternates, there is no latch",
    ("gate_fail_pass", "unfused"): "ADMM_FLAG_UNFUSED: the handle never alternates, there is no latch",
    ("gate_fail_pass", "mixed"): "the mixed mode runs its MFMA form whether or not the gate passes (tests/test_gpu_mfma.py)",
})
del _t, _k

Case = collections.namedtuple("Case", "transition kind shape")


def cases():
    out = []
    for t in TRANSITIONS:
        for k, cfg in KINDS.items():
            if (t, k) in SKIP:
                continue
            for sh in cfg["shapes"]:
                if t == "gate_fail_pass" and SHAPES[sh][:3] != (6, 3, 33):
                    continue
                out.append(Case(t, k, sh))
    return out


def skipped():
    return [(t, k, SKIP[t, k]) for t in TRANSITIONS for k in KINDS if (t, k) in SKIP]


def cid(c):
    return f"{c.transition}-{c.kind}-{c.shape}"


# ---- problems ---------------------------------------------------------------------------------------------------------------

def base(kind, shape, seed=None):
    """The boxed LTV problem of (kind, shape): random_ltv at the ALT_TABLE seed, its state box scaled by BOX_SCALE."""
    n, m, N, batch = SHAPES[shape]
    carries = KINDS[kind].get("carries", ())
    p = pkg.random_ltv(N=N, n=n, m=m, batch=batch, seed=_shapes.ALT_TABLE[n, m][0] if seed is None else seed,
                       with_q="q" in carries, thrust_norm="thrust" in carries)
    lo, hi = p.lo.copy(), p.hi.copy()
    lo[:, m:] *= BOX_SCALE
    hi[:, m:] *= BOX_SCALE
    p = dataclasses.replace(p, lo=lo, hi=hi)
    if "fuel" in carries:          # a weight only where the controls have no box (tests/_op_sequences.py)
        w = np.random.default_rng(p.N + 99).uniform(0.02, 0.3, p.N)
        p = dataclasses.replace(p, fuel=np.where(np.isfinite(p.unorm), w, 0.0))
    if "soft" in carries:          # finite weights on state rows only: `open` changes which rows the penalty sees
        sw = np.random.default_rng(5).choice([np.inf, 0.05, 0.3, 1.0], size=(p.N, p.nb), p=[0.25, 0.25, 0.3, 0.2])
        sw[:, :m] = np.inf
        p = dataclasses.replace(p, soft=sw)
    if "consensus" in carries:
        p = dataclasses.replace(p, consensus=3)
    return p


def opened(p, keep_stage=None):
    """p with every state row (-inf, inf) -- at every stage but keep_stage."""
    lo, hi = np.array(p.lo, np.float64), np.array(p.hi, np.float64)
    lo[..., p.m:], hi[..., p.m:] = -np.inf, np.inf
    if keep_stage is not None:
        lo[keep_stage], hi[keep_stage] = p.lo[keep_stage], p.hi[keep_stage]
    return dataclasses.replace(p, lo=lo, hi=hi)


def lti(p):
    """p with the dynamics of stage 0 at every stage, given as LTI data."""
    return dataclasses.replace(p, A=np.ascontiguousarray(p.A[0]), B=np.ascontiguousarray(p.B[0]))


def shared_box(p):
    """p with one box for every stage -- (nb,) arrays --, a scalar thrust bound and scalar fuel weight where p has them (the
    control rows are then open at every stage).  The state box is that of the first stage on which every state row is bounded."""
    m = p.m
    k = next(k for k in range(p.N) if np.all(np.isfinite(p.lo[k, m:])) and np.all(np.isfinite(p.hi[k, m:])))
    lo, hi = p.lo[k].copy(), p.hi[k].copy()
    rep = {}
    if p.unorm is not None:
        lo[:m], hi[:m] = -np.inf, np.inf
        rep["unorm"] = np.float64(np.min(p.unorm))
    if p.fuel is not None:
        rep["fuel"] = np.float64(0.1)
    if p.soft is not None:
        rep["soft"] = np.array(p.soft[k])
    return dataclasses.replace(p, lo=lo, hi=hi, **rep)


def stage_box(p_shared, p):
    """The per-stage counterpart of shared_box(p): p's (N, nb) box and (N,) thrust bound.  With a fuel term the weight of shared_box
    is positive on every stage and stays in force: every stage then keeps open control rows and gets a finite radius."""
    rep = dict(lo=p.lo.copy(), hi=p.hi.copy())
    if p.unorm is not None:
        rep["unorm"] = p.unorm.copy()
    if p.fuel is not None:
        rep["lo"][:, :p.m], rep["hi"][:, :p.m] = -np.inf, np.inf
        rep["unorm"] = np.where(np.isfinite(p.unorm), p.unorm, 0.33)
        rep["fuel"] = np.full(p.N, 0.1)
    if p.soft is not None:
        rep["soft"] = np.array(np.broadcast_to(p_shared.soft, (p.N, p.nb)))
    return dataclasses.replace(p_shared, **rep)


def thrust_moved(p):
    """The stages with a finite unorm and those with a box on the control rows swap."""
    m = p.m
    ball = np.isfinite(p.unorm)
    rng = np.random.default_rng(17)
    lo, hi = p.lo.copy(), p.hi.copy()
    lo[ball, :m], hi[ball, :m] = -rng.uniform(0.1, 0.6, (int(ball.sum()), m)), rng.uniform(0.1, 0.6, (int(ball.sum()), m))
    lo[~ball, :m], hi[~ball, :m] = -np.inf, np.inf
    return dataclasses.replace(p, lo=lo, hi=hi, unorm=np.where(ball, np.inf, rng.uniform(0.15, 0.7, p.N)))


def problems(case):
    """[p1, p2 (, p3)]: set-up, then one admm_update_problem each."""
    t = case.transition
    p = base(case.kind, case.shape)
    if t == "open":
        return [p, opened(p)]
    if t == "close":
        return [opened(p), p]
    if t == "open_partial":
        return [p, opened(p, keep_stage=p.N // 2)]
    if t == "lti_ltv":
        return [lti(p), p]
    if t == "ltv_lti":
        return [p, lti(p)]
    if t == "box_shared_stage":
        sh = shared_box(p)
        st = stage_box(sh, p)
        return [sh, st, sh]
    if t == "thrust_move":
        return [p, thrust_moved(p)]
    if t == "gate_fail_pass":
        a, b = (base(case.kind, case.shape, seed=s) for s in GATE_SEEDS)
        return [a, b, a]
    if t == "set_state_open":
        return [opened(p)]
    raise KeyError(t)


def options(case):
    cfg = KINDS[case.kind]
    return pkg.Options(**dict(dict(SOLVE, **ADAPT), rho=RHO, segments=SEGMENTS, **cfg["opt"]))


def state_rows_open(p):
    return bool(np.all(np.isneginf(np.asarray(p.lo)[..., p.m:])) and np.all(np.isposinf(np.asarray(p.hi)[..., p.m:])))


def set_state_y(p):
    """What set_state_open hands to admm_set_state: a random y, non-zero on every row -- the open state rows among them."""
    return 0.3 * np.random.default_rng(23).standard_normal((p.batch, p.L)) + 0.05


# ---- the script of a case ---------------------------------------------------------------------------------------------------
# ops: ("run", k, every) ("update", j) ("set_state_y",) ("set_rho", rho) ("solve_begin",) ("solve",) ("lean",) -- a coverage guard:
# lean_iterations() has grown since the last one -- and the read-outs ("get",) ("residuals",) ("certificate",); ("twin",) marks where the fresh twin
# is built from the handle's state

POST = (((1, 1), (2, 0), (3, 2), (7, 1)),         # a residual iteration first; ends on seven residual iterations (lean where capable)
        ((7, 0), (1, 2), (2, 1), (3, 1)),         # seven iterations without residuals first (XFREE = 2 where the rows are open)
        ((3, 0), (7, 2), (1, 1), (2, 2)))


LEAN_DIMS = ((6, 3), (12, 6))     # the pairs the lean residual forms are compiled for (alt_lean_dims, csrc/admm_dispatch.hpp)


def lean_capable(case, p):
    """The lean residual forms apply to the handle of `case` while its problem is p (and the gate has not failed)."""
    return bool(KINDS[case.kind].get("lean")) and SHAPES[case.shape][:2] in LEAN_DIMS and state_rows_open(p)


def alt_ok_expected(case):
    """The stated outcome of the forward-elimination gate (host_factor(...)["alt_ok"] at RHO with SEGMENTS) for every problem of
    the case, and for the last one at RHO_AFTER; tests/test_update_structure_host.py holds the library's host code to it.  The
    dynamics of ALT_TABLE pass as LTV data; stage 0 of the (12, 6) draw repeated over the horizon does not, and neither does
    GATE_SEEDS[1]."""
    t = case.transition
    n = len(problems(case))
    ok = [True] * n
    if t == "gate_fail_pass":
        ok = [True, False, True]
    if SHAPES[case.shape][:2] == (12, 6) and t in ("lti_ltv", "ltv_lti"):
        ok = [False, True] if t == "lti_ltv" else [True, False]
    return ok, ok[-1]


def script(case):
    t, cfg = case.transition, KINDS[case.kind]
    probs = problems(case)
    idx = cases().index(case)
    ts = "world" in cfg            # a time shard: iteration calls are collective, solve and certificate are left to its own tests
    # a certificate first, at the zero state: its device copy of the dynamics and weights exists when the update comes (cert_valid)
    ops = [] if ts else [("certificate",)]
    # pre-phase: the hidden state the transition is about
    if t == "close" or (t == "set_state_open" and idx % 2):
        ops += [("run", 10, 1), ("run", 7, 0)]            # lean residual iterations, then XFREE = 2 ones: v of the state rows unwritten
        if lean_capable(case, probs[0]):
            ops.append(("lean",))
    elif idx % 2:
        ops += [("run", 7, 1)]                             # odd: the call ends on a forward form
    else:
        ops += [("run", 4, 2), ("run", 6, 0)]              # even: ends on a backward form; graphs captured and replayed
    if not ts:
        ops += [("solve_begin",)]                          # background candidates of the adaptive rule (they read the host copy)
    for j in range(1, max(2, len(probs))):
        last = j == max(2, len(probs)) - 1
        if t == "set_state_open":
            ops.append(("set_state_y",))
        else:
            ops.append(("update", j))
        ops.append(("twin",))
        for k, every in POST[(idx + j) % 3]:
            ops += [("run", k, every), ("get",), ("residuals",)]
        if lean_capable(case, probs[min(j, len(probs) - 1)]):
            ops += [("run", 4, 1), ("get",), ("residuals",), ("lean",)]      # four residual iterations in one call: lean ones among them
        if last:
            ops += [("set_rho", RHO_AFTER), ("run", 5, 2), ("get",), ("residuals",)]
            if cfg.get("solve", True) and not ts:
                ops += [("solve",), ("get",)]
            if not ts:
                ops += [("certificate",)]
    return ops


def apply_model(model, op, case, probs):
    """One op on the host model -> what a read-out reads (the dicts of tests/_op_sequences.apply_model), else None."""
    name = op[0]
    if name == "run":
        return model.run(op[1], op[2])
    if name == "update":
        return model.update_problem(dataclasses.replace(probs[op[1]], fuel=None, soft=None))
    if name == "set_state_y":
        return model.set_state(y=set_state_y(model.p))
    if name == "set_rho":
        return model.set_rho(op[1])
    if name == "solve":
        return dict(info=dict(model.solve()))
    if name == "get":
        return {k: a.copy() for k, a in zip(("w", "z", "y"), model.get())}
    if name == "residuals":
        return dict(resid=tuple(a.copy() for a in model.residuals()))
    if name == "certificate":
        return dict(cert=model.certificate())
    if name in ("solve_begin", "twin", "lean"):
        return None
    raise KeyError(name)


Reference = collections.namedtuple("Reference", "log margins states")


@functools.lru_cache(maxsize=None)
def reference(case):
    """The script on the host model, once: log[i] = the read-out of op i (None for the others), margins = every stopping-rule /
    adaptive-rule comparison taken, states[i] = (z, y, rho) BEFORE op i where op i is an update or a set_state (what the host test's
    conditions are about)."""
    probs = problems(case)
    cfg = KINDS[case.kind]
    model = HandleModel(probs[0], options(case), fused=not cfg.get("unfused", False))
    log, states = [], {}
    for i, op in enumerate(script(case)):
        if op[0] in ("update", "set_state_y"):
            states[i] = (model.z.copy(), model.y.copy(), model.rho, model.p)
        log.append(apply_model(model, op, case, probs))
    return Reference(log, list(model.margins), states)


# ---- the infeasibility probe across open / close -----------------------------------------------------------------------------
# di_position_box of tests/_infeas_cases.py (a corridor on the position row), its opened box, and the corridor again.  Per problem:
# (iterations before the probe, span) and the flags tests/test_infeas_host.py establishes with linprog: QPs 1, 2, 3 cannot stay in
# the corridor, every QP is feasible without it.
PROBE_KINDS = ("one_lane", "one_lane_relaxed", "graph")
PROBE_RUNS = ((100, 10), (20, 10), (100, 10))
PROBE_FLAGS = ([0, 1, 1, 1], [0, 0, 0, 0], [0, 1, 1, 1])


def probe_problems():
    import _infeas_cases as ic
    p = ic.di_position_box()
    return [p, opened(p), p]


def probe_options(kind):
    import _infeas_cases as ic
    return pkg.Options(**dict(dict(SOLVE, **ADAPT), rho=ic.RHO, segments=3, **KINDS[kind]["opt"]))


ProbeReference = collections.namedtuple("ProbeReference", "outs margins unclear")


@functools.lru_cache(maxsize=None)
def probe_reference(kind):
    """The host model through set-up, probe, open, probe, close, probe -> (the three probe read-outs, the margins of their decisions,
    the zero / nonzero decisions rounding could flip)."""
    import _infeas_cases as ic
    probs = probe_problems()
    model = HandleModel(probs[0], probe_options(kind))
    outs = []
    for j, (p, (k, span)) in enumerate(zip(probs, PROBE_RUNS)):
        if j:
            model.update_problem(p)
        model.run(k, 0)
        outs.append(model.infeasibility(span, ic.EPS, True))
    return ProbeReference(outs, list(model.margins), list(model.unclear))
