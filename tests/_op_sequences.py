"""Seeded call sequences on solver handles (tests/test_gpu_sequences.py, tests/test_handle_model_host.py).

sequence(kind, seed) -> [(op, args), ...], fully determined by (kind, seed) through numpy.random.default_rng; the arguments are
small scalars (lengths, flags, seeds of arrays), so a failing test can print the list.  materialise() turns one op into the
concrete arrays both sides get, apply_model() runs it on the host model (tests/_handle_model.py).

The ops fall into seven classes -- odd iteration call, even iteration call, residual-evaluating call, state change, refused
call, read-out, solve.  The class of every op of a sequence follows a random Eulerian circuit of the complete directed graph
(loops included) over the classes of the kind: EVERY ordered pair of classes occurs as neighbours in every sequence (50 ops with
seven classes, 37 on the kind without a solve), and read-outs come where the circuit puts them, not after every op -- a read-out
brings the hidden state of a handle into its normal form.  Within a class the op and its arguments are drawn at random.
"""
import dataclasses

import numpy as np

import admm_library_amd as pkg
from admm_library_amd import _abi

CLASSES = ("odd", "even", "resid", "change", "refused", "readout", "solve")
MAX_ITERATIONS = 200           # per sequence: the range over which test_config2_slice_many_iterations holds 1e-10
SOLVE = dict(eps_abs=1e-2, eps_rel=1e-2, max_iter=12, check_interval=4)
ADAPT = dict(adapt_interval=4, adapt_mu=2.0, adapt_tau=2.0, adapt_max=16)
F = _abi


def _ltv(**kw):
    return lambda seed, dN=0: pkg.random_ltv(**dict(kw, N=kw["N"] + dN, seed=seed))


def _inst(**kw):
    return lambda seed, dN=0: pkg.random_instances(**dict(kw, N=kw["N"] + dN, seed=seed))


def _formation(seed, dN=0):
    return pkg.cw_formation(N=64 + dN, batch=17, seed0=20231004 + 1000 * (seed - 1))


def _fuel(seed, dN=0):
    p = pkg.random_ltv(N=37 + dN, n=6, m=3, batch=9, seed=seed, thrust_norm=True)
    w = np.random.default_rng(seed + 99).uniform(0.02, 0.3, p.N)
    return dataclasses.replace(p, fuel=np.where(np.isfinite(p.unorm), w, 0.0))      # a weight only where the controls have no box


_FIRST = dict(N=33, n=6, m=3, batch=69, with_q=False)
_THRUST = dict(N=37, n=6, m=3, batch=9, thrust_norm=True)

# make(seed, dN): the problem of variant `seed` (1 = set-up, others = admm_update_problem), dN: another horizon (a refused update)
# family: path()["kernel_family"] at set-up; alt: profile modes 2 / 3 are drawn; tol: iterates and residuals
KINDS = {
    "one_lane_alt": dict(make=_ltv(**_FIRST), opt=dict(rho=0.3, segments=4, flags=F.FLAG_NO_MFMA), family="one_lane_fp64",
                         alt=True, device_io=True),
    "one_lane_alt_relaxed": dict(make=_ltv(**_FIRST), opt=dict(rho=0.3, alpha=1.6, segments=4, flags=F.FLAG_NO_MFMA),
                                 family="one_lane_fp64", alt=True),
    "with_q_two_blocks": dict(make=_ltv(N=30, n=4, m=2, batch=300), opt=dict(rho=0.3, segments=4, **ADAPT)),
    "lean_xfree": dict(make=_ltv(N=45, n=6, m=3, batch=67, with_q=False, state_bounds=False),
                       opt=dict(rho=0.3, segments=4, flags=F.FLAG_NO_MFMA), family="one_lane_fp64", alt=True, lean=True),
    "plain_fused": dict(make=_ltv(**_FIRST), opt=dict(rho=0.3, segments=4, flags=F.FLAG_NO_ALTERNATE)),
    "plain_fused_chain": dict(make=_ltv(**_FIRST), opt=dict(rho=0.3, segments=4, flags=F.FLAG_NO_ALTERNATE | F.FLAG_SCAN_CHAIN)),
    "unfused": dict(make=_ltv(**_FIRST), opt=dict(rho=0.3, segments=4, flags=F.FLAG_UNFUSED), unfused=True),
    "graph_replay": dict(make=_ltv(**_FIRST), opt=dict(rho=0.3, segments=4, flags=F.FLAG_NO_MFMA | F.FLAG_GRAPH),
                         family="one_lane_fp64", alt=True),
    "thrust_bound": dict(make=_ltv(**_THRUST), opt=dict(rho=0.3, segments=5, **ADAPT)),
    "fuel_thrust_bound": dict(make=_fuel, opt=dict(rho=0.3, segments=5), fuel=True),
    "mfma_fp64_formation": dict(make=_formation, opt=dict(rho=0.05, precision_mode=F.PRECISION_FP64_MFMA), family="mfma_fp64",
                                alt=True),
    "mfma_fp64_ltv": dict(make=_ltv(N=30, n=10, m=4, batch=5, with_q=False), seed0=3,
                          opt=dict(rho=0.3, segments=3, precision_mode=F.PRECISION_FP64_MFMA), family="mfma_fp64", alt=True),
    "mfma_default_formation": dict(make=_formation, opt=dict(rho=0.05), family="mfma_fp64", alt=True, seeds=(1, 2, 7)),
    "mixed": dict(make=_formation, opt=dict(rho=0.05, precision_mode=F.PRECISION_MIXED), family="mfma_mixed", tol=1e-5,
                  solve=False),
    "wide_one_lane": dict(make=_ltv(N=24, n=12, m=6, batch=3), seed0=6, opt=dict(rho=0.3, segments=4)),
    "pinst_lane_per_qp": dict(make=_inst(N=30, n=6, m=3, batch=70), opt=dict(rho=0.3, segments=5, **ADAPT), pinst=True,
                              device_io=True),
    "pinst_rows_over_lanes": dict(make=_inst(N=24, n=6, m=3, batch=9), opt=dict(rho=0.3), pinst=True,
                                  env={"ADMM_PI_ROWS": "1"}),
    "pinst_wide_one_segment": dict(make=_inst(N=20, n=12, m=6, batch=5), opt=dict(rho=0.3, segments=1), pinst=True),
    "pinst_wide_four_segments": dict(make=_inst(N=20, n=12, m=6, batch=5), opt=dict(rho=0.3, segments=4), pinst=True),
}
SEEDS = (1, 2, 3)


def seeds(kind):
    """The committed seeds of a kind: together they hold every op legal on it (tests/test_handle_model_host.py)."""
    return KINDS[kind].get("seeds", SEEDS)


CASES = [(kind, seed) for kind in KINDS for seed in seeds(kind)]


def problem(kind, variant=1, dN=0):
    cfg = KINDS[kind]
    return cfg["make"](cfg.get("seed0", 10) + variant - 1, dN)


def options(kind):
    return pkg.Options(**dict(SOLVE, **KINDS[kind]["opt"]))


def classes_of(kind):
    return tuple(c for c in CLASSES if c != "solve" or KINDS[kind].get("solve", True))


def legal_ops(kind):
    """{class: [op names]} of the kind -- what include/admm_hip.h allows on such a handle."""
    cfg = KINDS[kind]
    pinst, dev = cfg.get("pinst", False), cfg.get("device_io", False)
    ops = {
        "odd": ["iterate", "run"] + ([] if pinst else ["step_z"]) + ["profile"],
        "even": ["iterate", "run", "profile"],
        "resid": ["run", "profile"] + ([] if pinst else ["step_z"]),
        "change": ["step_x", "set_rho", "set_state", "update_instances", "update_problem"] + (["set_fuel"] if cfg.get("fuel") else [])
                  + (["set_state_device"] if dev else []),
        "refused": ["refuse_set_state_nan", "refuse_update_N", "refuse_update_lohi"] + (["refuse_set_fuel_neg"] if cfg.get("fuel") else []),
        "readout": ["get", "residuals", "rho_per_qp"] + ([] if pinst else ["certificate"]) + (["get_device"] if dev else []),
        "solve": ["solve", "solve_pieces"],
    }
    return {c: ops[c] for c in classes_of(kind)}


def _circuit(rng, classes):
    """Random Eulerian circuit (Hierholzer) of the complete digraph with loops on `classes`: len(classes)^2 + 1 nodes."""
    out = {c: [classes[i] for i in rng.permutation(len(classes))] for c in classes}
    stack, walk = [classes[int(rng.integers(len(classes)))]], []
    while stack:
        v = stack[-1]
        if out[v]:
            stack.append(out[v].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


def sequence(kind, seed):
    cfg = KINDS[kind]
    rng = np.random.default_rng([seed, sum(map(ord, kind))])
    walk = _circuit(rng, classes_of(kind))
    ops_of = legal_ops(kind)
    profile_modes = [0] if cfg.get("unfused") else [1, 2, 3] if cfg.get("alt") else [1]
    cost = {"odd": 1, "even": 2, "resid": 1, "solve": SOLVE["max_iter"]}        # the least an op of the class applies
    used, seq = 0, []
    for i, cls in enumerate(walk):
        reserve = sum(cost.get(c, 0) for c in walk[i + 1:])
        room = MAX_ITERATIONS - used - reserve
        name = ops_of[cls][int(rng.integers(len(ops_of[cls])))]
        k = int(rng.integers(1, 10))                                            # lengths 1 .. 9: both parities
        if cls == "odd":
            k = k if k % 2 else k - 1 if k > 1 else 1
        elif cls == "even":
            k = k + 1 if k % 2 else k
            k = min(k, 8)
        if cls in ("odd", "even", "resid") and k > room:
            k = 2 if cls == "even" else 1
        args = ()
        if name == "iterate":
            args = (k,)
        elif name == "run":
            if cls == "resid":
                every = (1, 2, k)[int(rng.integers(3))]
                every = min(every, k)
            else:
                every = 0 if k > 1 or rng.integers(2) else 2                    # run(1, 2): a residual interval that never comes
            args = (k, every)
        elif name == "step_z":
            k, args = 1, (cls == "resid",)
        elif name == "profile":
            if cls == "resid":
                mode = profile_modes[int(rng.integers(len(profile_modes)))]
                iters = 1 + int(rng.integers(2))
                k = {0: iters, 1: iters, 2: 2 * iters + 2, 3: 2}[mode]
                if k > room:
                    mode, iters, k = profile_modes[0], 1, 1
                args = (iters, True, mode)
            else:
                k = min(k, 4) if cls == "even" else min(k, 3)
                args = (k, False, profile_modes[0])
        elif name in ("solve", "solve_pieces"):
            k = SOLVE["max_iter"]
            args = () if name == "solve" else (int(rng.integers(3)),)           # steps before solve_end; 0: until done
        elif name == "set_rho":
            args = (float(np.round(4.0 ** rng.uniform(-1.0, 1.0), 3)),)         # within a factor of 4 of the start value
        elif name in ("set_state", "set_state_device"):
            mask = int(rng.integers(1, 8))
            args = (mask,) + tuple(float(x) for x in np.round(rng.uniform(0.5, 1.5, 3), 3))
        elif name == "update_instances":
            which = int(rng.integers(1, 4)) if problem_has_q(kind) else 1       # 1: x0, 2: q, 3: both
            args = (which, int(rng.integers(1 << 30)))
        elif name == "update_problem":
            args = (2 + int(rng.integers(4)),)
        elif name == "set_fuel":
            args = (float(np.round(rng.uniform(0.3, 2.0), 3)),)
        elif name == "certificate":
            args = (bool(rng.integers(2)),)
        elif name in ("get", "get_device"):
            args = (int(rng.integers(1, 8)),)
        elif name == "refuse_set_state_nan":
            args = (int(rng.integers(3)),)
        if cls in cost:
            used += k
        seq.append((name, args))
    return seq


def problem_has_q(kind):
    return problem(kind).q is not None


def op_class(name, args):
    if name in ("solve", "solve_pieces"):
        return "solve"
    if name.startswith("refuse_"):
        return "refused"
    if name in ("get", "get_device", "residuals", "rho_per_qp", "certificate"):
        return "readout"
    if name == "step_z":
        return "resid" if args[0] else "odd"
    if name == "profile":
        return "resid" if args[1] else ("odd" if args[0] % 2 else "even")
    if name == "run":
        k, every = args
        return "resid" if every and k // every >= 1 else ("odd" if k % 2 else "even")
    if name == "iterate":
        return "odd" if args[0] % 2 else "even"
    return "change"


# ---- from an op to what both sides are given ------------------------------------------------------------------------------

def initial_snapshot(kind, seed):
    """What set_state scales before the first read-out: small random arrays."""
    p = problem(kind)
    rng = np.random.default_rng([seed, 7])
    return tuple(0.1 * rng.standard_normal((p.batch, p.L)) for _ in range(3))


def materialise(kind, name, args, model, snap):
    """Concrete arguments of one op: arrays are built from the MODEL's problem and from `snap`, the model's (w, z, y) at the
    last state read-out, so the handle and the model are given the same numbers."""
    p = model.p
    if name in ("set_state", "set_state_device"):
        mask, scales = args[0], args[1:]
        return {k: (snap[i] * scales[i] if mask >> i & 1 else None) for i, k in enumerate(("w", "z", "y"))}
    if name == "refuse_set_state_nan":
        arrs = {k: None for k in ("w", "z", "y")}
        a = snap[args[0]].copy()
        a[p.batch - 1, p.L // 2] = np.nan
        arrs[("w", "z", "y")[args[0]]] = a
        return arrs
    if name == "update_instances":
        which, s = args
        rng = np.random.default_rng(s)
        x0 = p.x0 * (1.0 + 0.2 * rng.standard_normal(p.x0.shape)) if which & 1 else None
        q = p.q * (1.0 + 0.2 * rng.standard_normal(p.q.shape)) + 0.02 * rng.standard_normal(p.q.shape) if which & 2 else None
        return dict(x0=x0, q=q)
    if name == "update_problem":
        return dict(problem=dataclasses.replace(problem(kind, args[0]), fuel=None))     # (the handle's weights stay in force)
    if name == "refuse_update_N":
        return dict(problem=dataclasses.replace(problem(kind, 2, dN=1), fuel=None))
    if name == "refuse_update_lohi":
        new = dataclasses.replace(problem(kind, 2), fuel=None)
        lo = np.array(new.lo, np.float64)
        finite = np.flatnonzero(np.isfinite(np.asarray(new.hi).reshape(-1)))
        k = int(finite[len(finite) // 2])                                       # one bounded row in the middle of the box
        lo.reshape(-1)[k] = np.asarray(new.hi).reshape(-1)[k] + 1.0
        return dict(problem=dataclasses.replace(new, lo=lo))
    if name == "set_fuel":
        return dict(fuel=np.asarray(problem(kind).fuel) * args[0])
    if name == "refuse_set_fuel_neg":
        f = np.array(p.fuel, np.float64)
        f[p.N // 3] = -0.1
        return dict(fuel=f)
    if name == "set_rho":
        return dict(rho=KINDS[kind]["opt"]["rho"] * args[0])
    return {}


def apply_model(model, name, args, concrete):
    """Run one op on the host model; returns what a read-out op reads (a dict), else None.  Raises _handle_model.Refused."""
    if name == "iterate":
        return model.iterate(args[0])
    if name == "run":
        return model.run(*args)
    if name == "step_x":
        return model.step_x()
    if name == "step_z":
        return model.step_z(args[0])
    if name == "profile":
        return model.profile(*args)
    if name == "solve":
        return dict(info=model.solve())
    if name == "solve_pieces":
        return dict(info=model.solve(max_steps=args[0] or None))
    if name == "set_rho":
        return model.set_rho(concrete["rho"])
    if name in ("set_state", "set_state_device", "refuse_set_state_nan"):
        return model.set_state(**concrete)
    if name == "update_instances":
        return model.update_instances(**concrete)
    if name in ("update_problem", "refuse_update_N", "refuse_update_lohi"):
        return model.update_problem(concrete["problem"])
    if name in ("set_fuel", "refuse_set_fuel_neg"):
        return model.set_fuel(concrete["fuel"])
    if name == "certificate":
        return dict(cert=model.certificate())
    if name in ("get", "get_device"):
        w, z, y = model.get()
        return {k: a.copy() for i, (k, a) in enumerate(zip(("w", "z", "y"), (w, z, y))) if args[0] >> i & 1}
    if name == "residuals":
        return dict(resid=tuple(a.copy() for a in model.residuals()))
    if name == "rho_per_qp":
        return dict(rho_per_qp=model.rho_per_qp())
    raise KeyError(name)


def new_model(kind, alternating=None):
    from _handle_model import HandleModel
    cfg = KINDS[kind]
    return HandleModel(problem(kind), options(kind), alternating=cfg.get("alt", False) if alternating is None else alternating,
                       fused=not cfg.get("unfused", False))


def run_model(kind, seed):
    """The whole sequence on the host model -> (model, [(index, op, args, read-out or None, refused code or None)])."""
    from _handle_model import Refused
    model = new_model(kind)
    snap = initial_snapshot(kind, seed)
    log = []
    for i, (name, args) in enumerate(sequence(kind, seed)):
        concrete = materialise(kind, name, args, model, snap)
        try:
            out = apply_model(model, name, args, concrete)
            log.append((i, name, args, out, None))
        except Refused as e:
            log.append((i, name, args, None, e.code))
        if name in ("get", "get_device"):
            snap = tuple(a.copy() for a in model.get())
    return model, log
