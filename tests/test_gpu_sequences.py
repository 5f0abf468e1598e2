"""Random call sequences on solver handles against the host model (tests/_handle_model.py, tests/_op_sequences.py).

One test per (kind, seed): the sequence runs on a Solver and on the model; at every read-out op of the sequence, and once at
the end, whatever was read is compared.  Nothing is compared after the other ops: a read-out brings the handle's hidden state
(v against (z, y), stale w, elimination direction, side data of the lean forms, a deferred finalise) into its normal form, and
the point of the sequences is what the library does when nothing has.

Tolerance: 1e-10 x max(1, |ref|_inf) on iterates and residual norms, that of every fp64 path of the suite (1e-5 on the mixed
kind, the file header of test_gpu_mfma.py); the certificate as in test_gpu_cert.py; iteration counts, status, rho exactly.  The
host tests keep every stopping-rule and adaptive-rule comparison of these sequences a relative 1e-6 away from its threshold, so
rounding on the GPU cannot flip one.  A set_rho / update_problem refused with ADMM_ERR_NUMERIC (conditioning bound) and a
fall-back to the plain kernels with a warning are legal outcomes; the iterates must match either way.

The kinds with ext=True add the receding-horizon step (its outputs u and x_next are compared like a read-out, and the model goes on
from its own x+), the infeasibility probe (the scales and the flag rule of tests/test_gpu_infeas.py, _infeas_ref.check; flags equal and
sep finite on the same QPs: the host tests keep every sep away from -eps and every open row away from eps |mu|_inf; defect is left out
on the QPs where the model finds mu or lambda to be a rounding error of a stationary y -- none in the committed sequences but for the
rows of the soft kinds that stay violated, y = s / rho there: stationary_rows in tests/_op_sequences.py), the consensus read-out and the soft report.  The bounds of the soft report follow from the iterate tolerance tau = 1e-10 max(1, |z|_inf) of the
model's z: max_violation is a difference of z and a bound (tau), the penalty a sum of weight times violation (tau x the sum of the
finite weights), and n_violated is exact -- the host tests keep every finite-weight row of every committed report clearly outside its
box, clearly inside, or exactly on a bound with |y| away from s / rho.

The half-space and cone kinds (ops.PLANE_KINDS): admm_get_halfspace / admm_get_cone must return the last accepted payload bit for
bit, and the bounds of the reports follow from the iterate tolerances tau_w, tau_y = 1e-10 max(1, |.|_inf) of the model's w and y,
which bound every entry, so a stage's nh rows differ by at most sqrt(nh) tau in the 2-norm.  max_violation is the distance of w_xi
from the half-space (a . w_xi - b)+ / |a|, or from the cone (r - g s)+ / sqrt(1 + g^2): a distance to a convex set is 1-Lipschitz in
w_xi, and so is the maximum over the stages: sqrt(nh) tau_w.  A plane's lam_k = rho (a_k . y_xi) / |a_k|^2 changes by at most
rho |a_k| sqrt(nh) tau_y / |a_k|^2 = rho sqrt(nh) tau_y / |a_k|; a cone's lam_k = rho |y_xi|_2 by at most rho sqrt(nh) tau_y; both are
exactly 0 where the stage has no plane / cone.  n_active counts exact decisions (lam > 0; y_xi != 0) and is compared exactly: the
host tests keep every stage of every committed report clear of the unclear-stage rule of tests/_handle_model.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: one HIP runtime in the process, also when this file runs alone)

import admm_library_amd as pkg
from admm_library_amd import _abi
from admm_library_amd.solver import AdmmError

import _infeas_ref as ir
import _op_sequences as ops
from _handle_model import NUMERIC, Refused

pytestmark = pytest.mark.gpu
_LEAN = {}          # seed -> lean_iterations() of the lean kind's sequence
_WORST = {}         # compared quantity -> worst error / bound over the tests run so far (printed by every test)


def _tensor(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _rc(lib, rc):
    if rc:
        raise AdmmError(rc, lib.admm_last_error().decode())


def _mpc_args(c, device=False):
    per_qp = ("du", "dx", "x_meas", "q_tail")
    return {k: (_tensor(v) if device and k in per_qp else v) for k, v in c.items()}


def _probe_device(s, span, eps, costates):
    """admm_probe_infeasibility_device on a handle set up from host arrays -> an Infeasibility of NumPy arrays."""
    import torch
    from admm_library_amd.solver import Infeasibility, _stream, _tptr
    p, dev = s.problem, "cuda:0"
    outs = [torch.empty(s.batch, dtype=torch.float64, device=dev) for _ in range(3)]
    flag = torch.empty(s.batch, dtype=torch.int32, device=dev)
    nu = torch.empty((s.batch, p.N, p.n), dtype=torch.float64, device=dev) if costates else None
    _rc(s._lib, s._lib.admm_probe_infeasibility_device(s._h, int(span), float(eps), *[_tptr(o) for o in outs],
                                                       C.cast(C.c_void_p(flag.data_ptr()), _abi.c_int32_p), _tptr(nu), _stream(dev)))
    torch.cuda.synchronize()
    return Infeasibility(*[o.cpu().numpy() for o in outs], flag.cpu().numpy(), None if nu is None else nu.cpu().numpy())


def _apply_gpu(s, name, args, c):
    """One op on the Solver; returns what a read-out op reads.  Raises AdmmError (ValueError from the wrapper's own checks)."""
    lib = s._lib
    if name == "mpc_advance" or name.startswith("refuse_mpc"):
        u, x = s.mpc_advance(**_mpc_args(c))
        return dict(mpc=dict(u=u, x_next=x))
    if name == "mpc_advance_device":
        import torch
        u, x = s.mpc_advance(**_mpc_args(c, device=True))
        assert u.is_cuda and x.is_cuda                        # (the device form ran)
        torch.cuda.synchronize()
        return dict(mpc=dict(u=u.cpu().numpy(), x_next=x.cpu().numpy()))
    if name == "infeasibility":
        return dict(probe=s.infeasibility(args[0], ops.PROBE_EPS, args[1]))
    if name == "infeasibility_device":
        return dict(probe=_probe_device(s, args[0], ops.PROBE_EPS, args[1]))
    if name == "refuse_probe":
        return dict(probe=s.infeasibility(3, ops.PROBE_EPS, False))
    if name == "refuse_profile_fused":
        return s.profile(1, residuals=False, fused=True) and None
    if name == "set_soft":
        return s.set_soft(c["soft"])
    if name == "refuse_set_soft_neg":         # Problem.validate would stop it in the wrapper: hand the weights to the library itself
        return _rc(lib, lib.admm_set_soft(s._h, _abi.dptr(np.ascontiguousarray(c["soft"], np.float64))))
    if name == "refuse_set_fuel_on_soft_rows":          # (likewise)
        return _rc(lib, lib.admm_set_fuel(s._h, _abi.dptr(np.ascontiguousarray(c["fuel"], np.float64))))
    plane = getattr(s.problem, "z_kind", None)
    plane = plane if plane in ("halfspace", "cone") else None
    if (name == "refuse_update_N" and (getattr(s.problem, "soft", None) is not None or plane)) or name == "refuse_update_closed_box":
        cp, keep = _abi.marshal_problem(c["problem"], s._row_major)        # (likewise: the wrapper re-attaches the weights, planes, cones)
        return _rc(lib, lib.admm_update_problem(s._h, C.byref(cp)))
    if name in ops.SET_PLANE:
        return getattr(s, "set_" + plane)(*[_tensor(a) if name.endswith("_device") else a for a in c["payload"]])
    if name.startswith(("refuse_set_halfspace", "refuse_set_cone")):
        if name.endswith("_device"):          # the wrapper checks shapes and devices only: the findings are the device's
            return getattr(s, "set_" + plane)(*[_tensor(a) for a in c["payload"]])
        return _rc(lib, getattr(lib, "admm_set_" + plane)(s._h, *[_abi.dptr(np.ascontiguousarray(a, np.float64)) for a in c["payload"]]))
    if name in ("get_halfspace", "get_cone"):
        return dict(payload=getattr(s, plane)())
    if name in ops.PLANE_REPORTS:
        r = getattr(s, plane + "_report")(multipliers=args[0], device=name.endswith("_device"))
        if name.endswith("_device"):
            import torch
            torch.cuda.synchronize()
            r = [None if a is None else a.cpu().numpy() for a in (r.max_violation, r.n_active, r.lam)]
        else:
            r = [r.max_violation, r.n_active, r.lam]
        return dict(plane_report=dict(max_violation=r[0], n_active=r[1], lam=r[2]))
    if name == "soft_report":
        r = s.soft_report()
        return dict(soft_report=dict(penalty=r.penalty, max_violation=r.max_violation, n_violated=r.n_violated))
    if name == "soft_report_device":
        import torch
        r = s.soft_report(device=True)
        torch.cuda.synchronize()
        return dict(soft_report=dict(penalty=r.penalty.cpu().numpy(), max_violation=r.max_violation.cpu().numpy(),
                                     n_violated=r.n_violated.cpu().numpy()))
    if name == "consensus":
        return dict(consensus=s.consensus())
    if name == "consensus_device":
        import torch
        from admm_library_amd.solver import _stream, _tptr
        p = s.problem
        out = torch.empty((s.batch // int(p.consensus), p.N, p.m), dtype=torch.float64, device="cuda:0")
        _rc(lib, lib.admm_get_consensus_device(s._h, _tptr(out), _stream("cuda:0")))
        torch.cuda.synchronize()
        return dict(consensus=out.cpu().numpy())
    if name == "iterate":
        return s.iterate(args[0])
    if name == "run":
        return s.run(*args)
    if name == "step_x":
        return s.step_x()
    if name == "step_z":
        return s.step_z(args[0])
    if name == "profile":
        iters, res, mode = args
        return s.profile(iters, residuals=res, fused=mode == 1, alternating=mode in (2, 3), back_to_back=mode == 3) and None
    if name == "solve":
        return dict(info=s.solve())
    if name == "solve_pieces":
        s.solve_begin()
        steps = 0
        while True:
            it, nconv, R, S = s.solve_step(sums=True)
            steps += 1
            if nconv >= s.batch or it >= s.options.max_iter or (args[0] and steps >= args[0]):
                break
            s.solve_adapt(R, S)
        return dict(info=s.solve_end())
    if name == "set_rho":
        return s.set_rho(c["rho"])
    if name in ("set_state", "refuse_set_state_nan"):
        return s.set_state(**c)
    if name == "set_state_device":
        return s.set_state(**{k: _tensor(a) for k, a in c.items()})
    if name == "update_instances":
        return s.update_instances(**c)
    if name in ("update_problem", "refuse_update_N"):
        return s.update_problem(c["problem"])
    if name == "refuse_update_lohi":          # Problem.validate would stop it in the wrapper: hand the box to the library itself
        good = c["problem"]
        import dataclasses
        cp, keep = _abi.marshal_problem(dataclasses.replace(good, lo=np.minimum(good.lo, good.hi)), s._row_major)
        keep["lo"][...] = good.lo
        rc = lib.admm_update_problem(s._h, C.byref(cp))
        if rc:
            raise AdmmError(rc, lib.admm_last_error().decode())
        return None
    if name == "set_fuel":
        return s.set_fuel(c["fuel"])
    if name == "refuse_set_fuel_neg":         # (likewise)
        rc = lib.admm_set_fuel(s._h, _abi.dptr(np.ascontiguousarray(c["fuel"], np.float64)))
        if rc:
            raise AdmmError(rc, lib.admm_last_error().decode())
        return None
    if name == "certificate":
        return dict(cert=s.certificate(costates=args[0]))
    if name == "get":
        got = s.get(*[bool(args[0] >> i & 1) for i in range(3)])
        return {k: a for k, a in zip(("w", "z", "y"), got) if a is not None}
    if name == "get_device":
        import torch
        got = s.get_device(*[bool(args[0] >> i & 1) for i in range(3)])
        torch.cuda.synchronize()
        return {k: a.cpu().numpy() for k, a in zip(("w", "z", "y"), got) if a is not None}
    if name == "residuals":
        return dict(resid=s.residuals())
    if name == "rho_per_qp":
        return dict(rho_per_qp=s.rho_per_qp())
    raise KeyError(name)


def _close(what, got, ref, tol):
    err = np.abs(np.asarray(got) - np.asarray(ref)).max()
    bound = tol * max(1.0, np.abs(ref).max())
    print(f"    {what}: |gpu - model| = {err:.3e} (bound {bound:.1e})")
    _worst(what.split(".")[0] if what.startswith("residuals") else what, err / bound, tol)
    assert err <= bound, (what, err, bound)


def _worst(what, ratio, tol):
    key = what if tol == 1e-10 else f"{what} (tolerance {tol:g})"
    _WORST[key] = max(_WORST.get(key, 0.0), float(ratio))


def _compare(got, ref, model, tol, unclear_ok=False):
    for k in ("w", "z", "y"):
        if k in ref:
            _close(k, got[k], ref[k], tol)
    if "resid" in ref:
        for k, g, r in zip(("r", "s", "nw", "nz", "ny"), got["resid"], ref["resid"]):
            _close("residuals." + k, g, r, tol)
    if "rho_per_qp" in ref:
        assert np.array_equal(got["rho_per_qp"], ref["rho_per_qp"]), (got["rho_per_qp"], ref["rho_per_qp"])
    if "info" in ref:
        g, r = got["info"], ref["info"]
        assert (g.iters_run, g.n_converged, g.rho, g.rho_updates) == (r["iters_run"], r["n_converged"], r["rho"], r["rho_updates"]), (g, r)
        assert np.array_equal(g.iters, r["iters"]) and np.array_equal(g.status, r["status"]), (g.iters, r["iters"], g.status, r["status"])
        _close("info.r", g.r, r["r"], tol)
        _close("info.s", g.s, r["s"], tol)
    if "cert" in ref:               # the scales of test_gpu_cert.py
        g, r = got["cert"], ref["cert"]
        b = model.p.batch
        s_nu = np.maximum(1.0, np.abs(r["nu"]).reshape(b, -1).max(axis=1))
        s_obj = np.maximum(1.0, r["obj_abs"])
        s_z = np.maximum(1.0, np.abs(model.z).reshape(b, -1).max(axis=1))
        ratios = {"stat": (np.abs(g.stat - r["stat"]) / (tol * s_nu)).max(), "obj": (np.abs(g.obj - r["obj"]) / (tol * s_obj)).max(),
                  "feas_dyn": (np.abs(g.feas_dyn - r["feas_dyn"]) / (tol * s_z)).max()}
        if g.nu is not None:
            ratios["nu"] = (np.abs(g.nu - r["nu"]).reshape(b, -1).max(axis=1) / (tol * s_nu)).max()
        print("    certificate, error / tolerance:", {k: float(f"{v:.3g}") for k, v in ratios.items()})
        for k, v in ratios.items():
            _worst("certificate." + k, v, tol)
        assert all(v <= 1.0 for v in ratios.values()), ratios
    if "mpc" in ref:
        _close("u", got["mpc"]["u"], ref["mpc"]["u"], tol)
        _close("x_next", got["mpc"]["x_next"], ref["mpc"]["x_next"], tol)
    if "consensus" in ref:
        assert got["consensus"].shape == ref["consensus"].shape
        _close("consensus", got["consensus"], ref["consensus"], tol)
    if "probe" in ref:
        g, r = got["probe"], ref["probe"]
        assert (g.nu is not None) == r["costates"]
        for k, v in ir.check(r, g, r["eps"], tol, flags_exact=True, defect_on=r["defect_clear"]).items():
            _worst("probe." + k, v, tol)
    if "soft_report" in ref:
        g, r = got["soft_report"], ref["soft_report"]
        tau = tol * max(1.0, np.abs(model.z).max())
        e_pen = np.abs(g["penalty"] - r["penalty"]).max()
        ratios = {"max_violation": np.abs(g["max_violation"] - r["max_violation"]).max() / tau,
                  "penalty": e_pen / (tau * r["weight_sum"]) if r["weight_sum"] > 0 else (0.0 if e_pen == 0 else np.inf)}
        print("    soft report, error / bound:", {k: float(f"{v:.3g}") for k, v in ratios.items()}, "violated rows:", int(r["n_violated"].sum()))
        for k, v in ratios.items():
            _worst("soft_report." + k, v, tol)
        assert all(v <= 1.0 for v in ratios.values()), ratios
        assert g["n_violated"].dtype == np.int32 and np.array_equal(g["n_violated"], r["n_violated"]), (g["n_violated"], r["n_violated"])
    if "payload" in ref:
        assert len(got["payload"]) == len(ref["payload"])
        for g, r in zip(got["payload"], ref["payload"]):
            assert g.shape == r.shape and np.array_equal(g, r), np.abs(g - r).max()
    if "plane_report" in ref:       # the bounds of the file header
        g, r = got["plane_report"], ref["plane_report"]
        kind, nh = model.p.z_kind, ops.plane_nh(model.p)
        tau_w, tau_y = (tol * max(1.0, np.abs(a).max()) for a in (model.w, model.y))
        ratios = {"max_violation": np.abs(g["max_violation"] - r["max_violation"]).max() / (np.sqrt(nh) * tau_w)}
        assert (g["lam"] is not None) == r["with_lam"]
        if r["with_lam"]:
            act = r["norm"] != 0.0
            bound = model.rho * np.sqrt(nh) * tau_y / (np.where(act, r["norm"], 1.0) if kind == "halfspace" else 1.0)
            assert g["lam"].shape == r["lam"].shape and not g["lam"][~act].any()
            ratios["lam"] = (np.abs(g["lam"] - r["lam"]) / bound)[act].max() if act.any() else 0.0
        print(f"    {kind} report, error / bound:", {k: float(f"{v:.3g}") for k, v in ratios.items()}, "active stages:",
              int(r["n_active"].sum()), "unclear:", int(r["unclear"].sum()))
        for k, v in ratios.items():
            _worst(f"{kind}_report.{k}", v, tol)
        assert all(v <= 1.0 for v in ratios.values()), ratios
        assert g["n_active"].dtype == np.int32
        if unclear_ok:              # (a kind that declares unclear_stages: within the QP's unclear stages)
            assert np.all(np.abs(g["n_active"].astype(np.int64) - r["n_active"]) <= r["unclear"]), (g["n_active"], r["n_active"], r["unclear"])
        else:
            assert np.array_equal(g["n_active"], r["n_active"]), (g["n_active"], r["n_active"])


def _run(kind, seed, monkeypatch, compare=True):
    cfg = ops.KINDS[kind]
    for var in ("ADMM_PI_LANE_PER_QP", "ADMM_PI_ROWS", "ADMM_PI_ROWS_FACTOR", "ADMM_NO_LEAN_RESID", "ADMM_NO_SKIPV_STORE"):
        monkeypatch.delenv(var, raising=False)
    for k, v in cfg.get("env", {}).items():
        monkeypatch.setenv(k, v)
    tol = cfg.get("tol", 1e-10)
    seq = ops.sequence(kind, seed)
    snap = ops.initial_snapshot(kind, seed)
    final = [("get", (7,)), ("residuals", ()), ("rho_per_qp", ())]
    last_ok = -1
    with pkg.Solver(ops.problem(kind), ops.options(kind)) as s:
        path = s.path()
        print(kind, seed, path)
        if "family" in cfg:
            assert path["kernel_family"] == cfg["family"], path
        assert path["per_instance"] == bool(cfg.get("pinst", False))
        model = ops.new_model(kind, alternating=path["alternating"])
        for i, (name, args) in enumerate(seq + final):
            if name == "profile":
                model.alternating = s.path()["alternating"]          # (a refactor may have left the alternating kernels)
            c = ops.materialise(kind, name, args, model, snap)
            got = exc = None
            try:
                got = _apply_gpu(s, name, args, c)
            except (AdmmError, ValueError) as e:
                exc = e
            if isinstance(exc, AdmmError) and exc.code == NUMERIC and name in ("set_rho", "update_problem"):
                print(f"  op {i} {name}{args}: refused by the conditioning bound, the model stays as it was")
                continue
            try:
                ref = ops.apply_model(model, name, args, c)
            except Refused as r:
                ok = (isinstance(exc, AdmmError) and exc.code == r.code) or \
                     (isinstance(exc, ValueError) and name == "refuse_update_N" and cfg.get("fuel"))
                assert ok, f"op {i} {name}{args}: the model refuses it with code {r.code}, the library answered {exc!r}\n{seq[:i + 1]}"
                continue
            assert exc is None, f"op {i} {name}{args}: the library refused what the model accepts: {exc!r}\n{seq[:i + 1]}"
            if name in ("get", "get_device"):
                snap = tuple(a.copy() for a in model.get())
            if ref is None or not compare:
                continue
            print(f"  op {i} {name}{args}")
            try:
                _compare(got, ref, model, tol, bool(cfg.get("unclear_stages")))
            except AssertionError as e:
                raise AssertionError(f"{kind} seed {seed}: read-out {i} {name}{args} differs from the model: {e}\n"
                                     f"first op after the last passing read-out: {last_ok + 1}\nops so far: {(seq + final)[:i + 1]}") from e
            last_ok = i
        return s.lean_iterations(), model


@pytest.mark.parametrize("kind,seed", ops.CASES)
def test_sequence_matches_the_host_model(gpu, kind, seed, monkeypatch):
    lean, model = _run(kind, seed, monkeypatch)
    print(f"{kind} seed {seed}: {model.iterations} iterations, lean {lean}")
    print("worst error / bound so far:", {k: float(f"{v:.3g}") for k, v in sorted(_WORST.items())})
    if ops.KINDS[kind].get("lean"):
        _LEAN[seed] = lean


def test_the_lean_kind_runs_lean_iterations(gpu, monkeypatch):
    """Coverage guard: over its seeds the lean kind's sequences launch iterations in the lean residual form."""
    kind = next(k for k, c in ops.KINDS.items() if c.get("lean"))
    for seed in ops.seeds(kind):
        if seed not in _LEAN:                 # (this test run on its own)
            _LEAN[seed] = _run(kind, seed, monkeypatch, compare=False)[0]
    print("lean iterations per seed:", _LEAN)
    assert sum(_LEAN.values()) > 0
