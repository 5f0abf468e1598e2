"""The model interface of the device SCvx outer step (ADMM_HIP_HAS_SCVX_MODELS), host side: the ABI surface and the
ctypes mirror of admm_scvx_dynamics, the refusals (no GPU needed: every check precedes the first HIP call), the register report of
csrc/admm_scvx_models.hip, the CR3BP model against facts that do not come from this code, model=None against today's behaviour, the
host loop on the Earth-Moon L2 scenario, and the inputs of tests/test_gpu_scvx_models.py themselves (tests/_scvx_models_case.py).
No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import admm_library_amd as pkg
from admm_library_amd import _abi
from admm_library_amd import scvx as sc

import _scvx_case as case
import _scvx_device_case as dc
import _scvx_models_case as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("admm_scvx_rollout_model_device", "admm_scvx_init_model_device", "admm_scvx_prepare_model_device",
         "admm_scvx_advance_model_device")
SYMBOLS = CALLS + ("admm_scvx_model_name",)
INVALID = 1


# ---- 1. ABI surface
def test_abi_surface(lib):
    hdr = open(os.path.join(ROOT, "include", "admm_hip.h")).read()
    assert "#define ADMM_HIP_HAS_SCVX_MODELS 1" in hdr
    assert "#define ADMM_HIP_ABI_VERSION 9" in hdr and lib.admm_abi_version() == 9
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.library_path()], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        assert name in pkg.solver._SIGNATURES and hasattr(lib, name) and f" T {name}\n" in nm, name
    assert lib.admm_scvx_model_name(0) == b"relative_circular" and lib.admm_scvx_model_name(1) == b"crtbp"
    assert lib.admm_scvx_model_name(2) is None and lib.admm_scvx_model_name(-1) is None
    assert (_abi.SCVX_RELATIVE_CIRCULAR, _abi.SCVX_CRTBP) == (0, 1)
    assert sc.relative_circular().name == "relative_circular" and sc.crtbp(0.3).name == "crtbp"
    assert (sc.relative_circular().kind, sc.crtbp(0.3).kind) == (0, 1)


def test_ctypes_dynamics_has_the_c_size(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "admm_hip.h"\n'
                   "int main(void) { printf(\"%zu %zu %zu %zu %d %d\\n\", sizeof(admm_scvx_dynamics), offsetof(admm_scvx_dynamics, reserved),\n"
                   "  offsetof(admm_scvx_dynamics, par), offsetof(admm_scvx_dynamics, kind), ADMM_SCVX_RELATIVE_CIRCULAR, ADMM_SCVX_CRTBP);\n"
                   "  return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D = _abi.CScvxDynamics
    assert got == [C.sizeof(D), D.reserved.offset, D.par.offset, D.kind.offset, _abi.SCVX_RELATIVE_CIRCULAR, _abi.SCVX_CRTBP]


# ---- 2. refusals
def _dynamics(**kw):
    par = kw.pop("par", None)
    d = _abi.CScvxDynamics(**dict(dict(N=4, batch=3, substeps=4, kind=1, dt=0.1), **kw))
    par = (sc.MU_EARTH_MOON, 1.1) if par is None else par
    d.par[:len(par)] = list(par)
    return d


REFUSALS = [("dynamics.N", dict(N=0)), ("dynamics.N", dict(N=-1)), ("dynamics.batch", dict(batch=0)), ("dynamics.batch", dict(batch=-2)),
            ("dynamics.substeps", dict(substeps=0)), ("dynamics.substeps", dict(substeps=-1))] + \
           [("dynamics.dt", dict(dt=v)) for v in (0.0, -0.1, np.inf, np.nan)] + \
           [("dynamics.kind", dict(kind=v)) for v in (2, -1, 1 << 20)] + \
           [("dynamics.reserved", dict(reserved=v)) for v in (1, -1)] + \
           [("dynamics.par[2]", dict(par=(0.3, 0.4, 1e-300))), ("dynamics.par[3]", dict(par=(0.3, 0.4, 0.0, np.nan))),
            ("dynamics.par[1]", dict(kind=0, par=(7000.0, 1.0))), ("dynamics.par[3]", dict(kind=0, par=(7000.0, 0.0, 0.0, -1.0)))] + \
           [("dynamics.par[0] (rc)", dict(kind=0, par=(v,))) for v in (0.0, -7000.0, np.inf, np.nan)] + \
           [("dynamics.par[0] (mu)", dict(par=(v, 0.4))) for v in (0.0, 1.0, -0.1, 1.5, np.inf, np.nan)] + \
           [("dynamics.par[1] (x_ref)", dict(par=(0.3, v))) for v in (np.inf, -np.inf, np.nan)]


def test_every_refusal_names_the_field_and_precedes_any_hip_call(lib):
    """Each refusal of the model calls gives ADMM_ERR_INVALID (never ADMM_ERR_NO_DEVICE or ADMM_ERR_HIP: this machine may have no
    device) with the field's name; a valid dynamics then reaches the pointer checks (NULL arguments, by name)."""
    params = _abi.CScvxParams(fd_eps=1e-6, tol=1e-6, rho_reject=0.1, rho_expand=0.7)
    state = _abi.CScvxState(history_capacity=4)
    n = C.c_int32(-1)
    null = _abi.c_double_p()
    calls = {CALLS[0]: lambda d: lib.admm_scvx_rollout_model_device(0, d, null, null, null, None),
             CALLS[1]: lambda d: lib.admm_scvx_init_model_device(0, d, C.byref(params), null, C.byref(state), 1.0, 1.0, None),
             CALLS[2]: lambda d: lib.admm_scvx_prepare_model_device(0, d, C.byref(params), null, C.byref(state), null, null, null, null, null, None),
             CALLS[3]: lambda d: lib.admm_scvx_advance_model_device(0, d, C.byref(params), null, null, C.byref(state), C.byref(n), None)}
    for name, fn in calls.items():
        for word, kw in REFUSALS:
            assert fn(C.byref(_dynamics(**kw))) == INVALID, (name, word, kw)
            msg = lib.admm_last_error().decode()
            assert msg.startswith(name + ": " + word), (name, word, kw, msg)
        assert fn(None) == INVALID and lib.admm_last_error().decode() == name + ": dynamics is NULL"
        for kind, par in ((0, (7000.0,)), (1, (0.3, 0.4)), (1, (sc.MU_EARTH_MOON, -1.0))):
            assert fn(C.byref(_dynamics(kind=kind, par=par))) == INVALID
            msg = lib.admm_last_error().decode()
            assert msg.startswith(name + ": ") and msg.endswith(" is NULL"), msg
    assert n.value == -1
    # params are checked as in the old calls
    bad = _abi.CScvxParams(fd_eps=0.0, tol=1e-6, rho_reject=0.1, rho_expand=0.7)
    assert lib.admm_scvx_prepare_model_device(0, C.byref(_dynamics()), C.byref(bad), null, C.byref(state), null, null, null, null, null, None) == INVALID
    assert "params.fd_eps" in lib.admm_last_error().decode()


def test_python_refusals():
    with pytest.raises(ValueError, match="mu"):
        sc.crtbp(1.0)
    with pytest.raises(ValueError, match="which"):
        sc.crtbp_collinear_point(0.3, 4)
    m = sc.crtbp(0.3, 0.4)
    with pytest.raises(dataclasses_error()):
        m.kind = 0


def dataclasses_error():
    import dataclasses
    return dataclasses.FrozenInstanceError


# ---- 3. the new unit
def test_the_models_unit_holds_the_crtbp_kernels_and_does_not_spill(tmp_path):
    """csrc/admm_scvx_models.hip compiled on its own with the library's flags and the compiler's resource report: the CR3BP
    instantiations of rollout (both forms), linearise and advance are there -- and no other scvx kernel: the shipped model's and
    the commit kernel live in admm_scvx.hip alone --; no scratch, no VGPR spill, LDS <= 64 KiB."""
    import __graft_entry__ as ge
    assert "admm_scvx_models.hip" in ge.SOURCES
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-Rpass-analysis=kernel-resource-usage"] + ge.HIPCC_FLAGS +
                       ["-c", os.path.join(ge.CSRC, "admm_scvx_models.hip"), "-o", str(tmp_path / "admm_scvx_models.o")],
                       cwd=ge.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = ge.parse_resource_usage(r.stderr)
    mine = [x for x in rows if "scvx_" in x["name"]]
    for x in mine:
        print(f'{x["name"]}: {x["vgpr"]} VGPRs, {x["agpr"]} AGPRs, {x["sgpr"]} SGPRs, LDS {x["lds"]} B, scratch {x["scratch"]} B, '
              f'occupancy {x["occupancy"]}')
    assert sorted(x["name"] for x in mine) == ["scvx_advance_kernel<admm::ScvxCrtbp>", "scvx_linearise_kernel<admm::ScvxCrtbp>",
                                               "scvx_rollout_kernel<admm::ScvxCrtbp, false>", "scvx_rollout_kernel<admm::ScvxCrtbp, true>"]
    assert all(x["scratch"] == 0 and x["vgpr_spill"] == 0 for x in rows), [x["name"] for x in rows if x["scratch"] or x["vgpr_spill"]]
    assert all(x["lds"] <= 65536 for x in rows)


# ---- 4. the model against facts that do not come from this code
@pytest.mark.parametrize("mu", [sc.MU_EARTH_MOON, 0.3])
@pytest.mark.parametrize("which", [1, 2, 3])
def test_collinear_points_are_equilibria(mu, which):
    X = sc.crtbp_collinear_point(mu, which)
    lo, hi = {1: (-mu, 1 - mu), 2: (1 - mu, 2.0), 3: (-2.0, -mu)}[which]
    assert lo < X < hi
    m = sc.crtbp(mu, X)
    rest = float(np.abs(m.rhs(np.zeros(6), np.zeros(3))).max())
    print(f"mu = {mu}, L{which}: X = {X!r}, |rhs at rest| = {rest:.2e}")
    assert rest < 1e-14
    assert m.kind == 1 and m.par == (mu, X)


def _jacobi(x, p):
    X = p.x_ref + x[..., 0]
    y, z = x[..., 1], x[..., 2]
    r1 = np.sqrt((X + p.mu) ** 2 + y ** 2 + z ** 2)
    r2 = np.sqrt((X - 1 + p.mu) ** 2 + y ** 2 + z ** 2)
    return X ** 2 + y ** 2 + 2 * (1 - p.mu) / r1 + 2 * p.mu / r2 - (x[..., 3:] ** 2).sum(axis=-1)


JACOBI_DT = 0.2          # stages of the drift check: h = 0.05 | 0.025, the drift 1e-9 | 1e-10 against a rounding floor of 1e-15


def test_the_jacobi_constant_drifts_as_rk4s_order_says():
    """Uncontrolled from the em_l2 scenario's x0 (long double, so that rounding does not enter; fp64 printed next to it): the Jacobi
    constant's drift over the horizon at substeps = 4 over that at substeps = 8 lies in [8, 32] -- a halved step divides the
    global error of a fourth-order method by 16."""
    p = mc.EM_L2._replace(dt=JACOBI_DT)
    x0 = np.concatenate([[mc.EM_X0], mc.em_l2_x0(3)])
    u = np.zeros((4, 10, 3))
    drift, drift64 = {}, {}
    for s in (4, 8):
        q = p._replace(substeps=s)
        x = mc.ld_rollout(x0, u, q)
        drift[s] = np.abs(_jacobi(x[:, -1], q) - _jacobi(np.asarray(x0, mc.LD), q))
        x64 = sc.rollout(x0, u, q.dt, mc.step_of(q))
        drift64[s] = np.abs(_jacobi(x64[:, -1], q) - _jacobi(x0, q))
    ratio, ratio64 = drift[4] / drift[8], drift64[4] / drift64[8]
    print("Jacobi drift, substeps 4:", drift[4].astype(float), "8:", drift[8].astype(float), "ratio", ratio.astype(float), "fp64 ratio", ratio64)
    assert (drift[8] > 1e-13).all()                               # truncation, not rounding
    assert ((ratio >= 8) & (ratio <= 32)).all() and ((ratio64 >= 8) & (ratio64 <= 32)).all()


def _analytic_jacobian(s, mu, x_ref):
    x, y, z = s[:3]
    X = x_ref + x
    d1, d2 = X + mu, X - 1 + mu
    r1, r2 = np.sqrt(d1 ** 2 + y ** 2 + z ** 2), np.sqrt(d2 ** 2 + y ** 2 + z ** 2)
    k = (1 - mu) / r1 ** 3 + mu / r2 ** 3
    S = (1 - mu) / r1 ** 5 + mu / r2 ** 5
    Sd = (1 - mu) * d1 / r1 ** 5 + mu * d2 / r2 ** 5
    Sdd = (1 - mu) * d1 ** 2 / r1 ** 5 + mu * d2 ** 2 / r2 ** 5
    G = np.array([[1 - k + 3 * Sdd, 3 * y * Sd, 3 * z * Sd],
                  [3 * y * Sd, 1 - k + 3 * y * y * S, 3 * y * z * S],
                  [3 * z * Sd, 3 * y * z * S, -k + 3 * z * z * S]])
    J = np.zeros((6, 9))
    J[:3, 3:6] = np.eye(3)
    J[3:, :3] = G
    J[3, 4], J[4, 3] = 2.0, -2.0
    J[3:, 6:] = np.eye(3)
    return J


@pytest.mark.parametrize("mu,x_ref,s", [(sc.MU_EARTH_MOON, mc.X_L2, [0.03, -0.03, 0.015, 0.1, -0.2, 0.05]),
                                        (0.3, 0.4, [0.05, 0.1, -0.07, -0.3, 0.2, 0.1]), (0.3, 0.0, [-0.9, 0.4, 0.3, 0.0, 0.5, -0.5])])
def test_analytic_jacobian_agrees_with_central_differences(mu, x_ref, s):
    """The gradient of the effective potential, written down independently of crtbp_rhs, against central differences of rhs
    (linearise's scheme: eps = 1e-6, (f(+) - f(-)) / 2 eps): 1e-7."""
    m = sc.crtbp(mu, x_ref)
    s, u, eps = np.array(s), np.array([0.1, -0.2, 0.3]), 1e-6
    fd = np.empty((6, 9))
    for j in range(9):
        d = np.zeros(9); d[j] = eps
        fd[:, j] = (m.rhs(s + d[:6], u + d[6:]) - m.rhs(s - d[:6], u - d[6:])) / (2 * eps)
    err = np.abs(fd - _analytic_jacobian(s, mu, x_ref)).max()
    print(f"mu = {mu}, x_ref = {x_ref}: max |fd - analytic| = {err:.2e}")
    assert err <= 1e-7


def test_rhs_torch_is_the_numpy_rhs():
    import torch
    rng = np.random.default_rng(3)
    s, u = rng.standard_normal((5, 7, 6)) * 0.1, rng.standard_normal((5, 7, 3))
    for m in (sc.crtbp(0.3, 0.4), sc.relative_circular(7000.0)):
        got = m.rhs_torch(torch.as_tensor(s), torch.as_tensor(u)).numpy()
        ref = m.rhs(s, u)
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
        np.testing.assert_array_equal(m.step(s, u, 0.1, substeps=2), sc._rk4(m.rhs, s, u, 0.1, 2))


# ---- 5. model=None changes nothing
def test_model_none_and_the_shipped_model_give_the_same_bits():
    args = (case.X0, 20, case.DT, case.Q, case.R, case.QN, -case.U_MAX, case.U_MAX)
    kw = dict(tr_u=1.0, tr_x=100.0, max_outer=4, tol=1e-7)
    a = sc.scvx(*args, qp_solver=case.oracle_qp_solver(**case.QP), **kw)
    b = sc.scvx(*args, qp_solver=case.oracle_qp_solver(**case.QP), model=None, **kw)
    c = sc.scvx(*args, qp_solver=case.oracle_qp_solver(**case.QP), model=sc.relative_circular(), **kw)
    for r in (b, c):
        np.testing.assert_array_equal(r.u, a.u)
        np.testing.assert_array_equal(r.x, a.x)
        assert r.cost == a.cost and r.history == a.history and r.outer_iterations == a.outer_iterations == 4
    step = lambda s, u, dt: sc.rk4_step(s, u, dt)      # noqa: E731
    for f, x0 in ((sc.scvx, case.X0), (sc.scvx_batch, case.X0[None])):
        with pytest.raises(ValueError, match="model and step"):
            f(x0, *args[1:], model=sc.relative_circular(), step=step)
    # and the refusal of a foreign step for the device outer step stands
    with pytest.raises(ValueError, match="outer_on_device"):
        sc.scvx_batch(case.X0[None], *args[1:], outer_on_device=True, linearise_on="cuda:0", step=step)


# ---- 6. the host loop converges
def _kinds(history):
    return {(h["accepted"], bool(h["ratio"] >= 0.7)) for h in history}


def test_the_host_loop_acquires_l2():
    """scvx() and a three-trajectory scvx_batch() with crtbp(Earth-Moon, L2) and the CPU oracle as QP solver, from the em_l2 scenario
    (N = 40, dt = 0.05, an insertion error of 0.03 per axis, box +-0.5, the loop's default radii): converge within max_outer, through
    a rejected and an accepted-and-expanded step; the uncontrolled trajectory leaves by more than 0.5."""
    m = mc.model_of(mc.EM_L2)
    free = sc.rollout(mc.EM_X0, np.zeros((mc.EM_N, 3)), mc.EM_DT, m.step)
    assert np.linalg.norm(free[-1, :3]) > 0.5
    r = sc.scvx(*mc.em_l2_args(mc.EM_X0), qp_solver=case.oracle_qp_solver(**case.QP), model=m, **mc.EM_SCVX)
    print("scvx:", r.outer_iterations, r.accepted, r.converged, f"cost {r.cost:.3e}", [("A" if h["accepted"] else "R") + f'{h["ratio"]:.2f}' for h in r.history])
    assert r.converged and r.outer_iterations <= mc.EM_SCVX["max_outer"]
    assert _kinds(r.history) >= {(True, True), (False, False)}
    assert np.abs(r.x[-1]).max() < 1e-3 and (np.abs(r.u) <= mc.EM_U_MAX).all()
    np.testing.assert_array_equal(r.x, sc.rollout(mc.EM_X0, r.u, mc.EM_DT, m.step))
    x0 = mc.em_l2_x0(3)
    res = sc.scvx_batch(*mc.em_l2_args(x0), qp_solver=case.oracle_qp_solver(**case.QP), model=m, **mc.EM_SCVX)
    for b, r in enumerate(res):
        print(f"scvx_batch[{b}]:", r.outer_iterations, r.accepted, r.converged, [("A" if h["accepted"] else "R") + f'{h["ratio"]:.2f}' for h in r.history])
        assert r.converged and r.outer_iterations <= mc.EM_SCVX["max_outer"] and np.abs(r.x[-1]).max() < 1e-3
        assert _kinds(r.history) >= {(True, True), (False, False)}


# ---- 7. preconditions of the GPU tests
def test_long_double_is_extended_precision():
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    x0, u, x, *_ = mc.scattered(63, 7, "general3")
    ld = mc.ld_rollout(x0, u, mc.PARAMS["general3"])
    assert ld.dtype == np.longdouble and 0 < np.abs(ld - x).max() < 1e-14


def test_parameter_sets_are_what_the_tests_say():
    assert mc.SHAPES == [(1, 1), (63, 7), (65, 64), (130, 65)] and sorted(mc.PARAMS) == ["em_l2", "general1", "general3"]
    e, g1, g3 = (mc.PARAMS[k] for k in ("em_l2", "general1", "general3"))
    assert (e.mu, e.x_ref, e.substeps, e.dt, e.fd_eps) == (sc.MU_EARTH_MOON, sc.crtbp_collinear_point(sc.MU_EARTH_MOON, 2), 4, 0.05, 1e-6)
    for s, g in ((1, g1), (3, g3)):
        assert (g.mu, g.x_ref, g.substeps, g.fd_eps) == (0.3, 0.4, s, 1e-5) and g.dt == g1.dt
        for a, b in zip(g[1:6], dc.GENERAL[s][1:6]):
            np.testing.assert_array_equal(a, b)                     # the dense SPD weights and the asymmetric box of _general


@pytest.mark.parametrize("name", sorted(mc.PARAMS))
@pytest.mark.parametrize("B,N", mc.SHAPES)
def test_scatter_preconditions_and_recorded_constants(B, N, name):
    """Every scattered state stays MIN_DISTANCE from both primaries; FP64_VS_LD[name, B, N] bounds max |NumPy fp64 - long double|
    per quantity on scattered(B, N, name) today and is no more than twice it; a kernel with mu and 1 - mu, or d1 and d2, swapped
    would be told from the right one (the long-double rollout moves by >= 1e-3); each A block differs from its transpose."""
    p = mc.PARAMS[name]
    x0, u, x, tru, trx, active = mc.scattered(B, N, name)
    d = mc.primary_distance(np.concatenate([x0[:, None], x], axis=1), p)
    assert d >= mc.MIN_DISTANCE, d
    assert (u >= p.u_lo).all() and (u <= p.u_hi).all()
    r = mc.reference(B, N, name)
    got = mc.fp64_vs_ld(B, N, name)
    print(f"fp64 vs long double, {name}, B={B} N={N}:", {k: f"{v:.3e}" for k, v in got.items()}, f"; nearest primary {d:.3f}")
    for k, v in got.items():
        c = mc.FP64_VS_LD[name, B, N][k]
        assert v <= c <= 2.0 * v, (k, v, c)
    for wrong in ("x_mu_swapped", "x_d_swapped"):
        assert np.abs(r[wrong] - r["ld"]["x"]).max() >= 1e-3, wrong
    A = r["np"]["A"]
    assert (np.abs(A - np.swapaxes(A, -1, -2)).max(axis=(2, 3)) >= 1e-2).all()
    assert B == 1 or ((r["lo"][~active] == 0).all() and (~active).any())


@pytest.mark.parametrize("params", mc.DECISION_PARAMS)
@pytest.mark.parametrize("B,N", mc.DECISION_SHAPES)
def test_decision_inputs_reach_every_branch_with_margin(B, N, params):
    """What tests/test_gpu_scvx_models.py asserts first, at ten times the knife-edge margin: every branch is taken B // 6 times (the
    lone trajectory of B = 1 is accepted), no finite ratio within 1e-2 of a threshold; the candidates stay clear of the primaries."""
    state, ref = mc.decision_inputs(B, N, params)
    taken = [dc.branch_of(b, state, ref) for b in range(B)]
    if B == 1:
        assert taken == ["accepted"]
    else:
        assert all(taken.count(t) >= B // 6 for t in mc.BRANCHES), {t: taken.count(t) for t in mc.BRANCHES}
        assert [t == "inactive" for t in taken] == (ref["kind"] == 5).tolist()
    assert dc.ratio_margin(ref["records"].values()) > 1e-2
    p = mc.PARAMS[params]
    assert mc.primary_distance(ref["x_new"], p) >= mc.MIN_DISTANCE and mc.primary_distance(state["xb"], p) >= mc.MIN_DISTANCE
    assert (state["ub"] >= p.u_lo).all() and (state["ub"] <= p.u_hi).all()


def test_nonfinite_inputs_are_what_the_gpu_test_needs():
    """The host reference of the non-finite candidates: a NaN cost on the two trajectories that start on a primary, a non-finite
    one on the overflowing trajectory, every one of them rejected with halved radii and still active; the ordinary trajectories
    have finite costs and no ratio within 1e-2 of a threshold."""
    p, state, ref = mc.nonfinite_inputs()
    for b in range(6):
        rec = ref["records"][b]
        if b in mc.NONFINITE_ROWS:
            assert np.isnan(ref["J_new"][b]) if mc.NONFINITE_ROWS[b] == "nan" else not np.isfinite(ref["J_new"][b]), (b, ref["J_new"][b])
            assert not rec["accepted"] and not ref["take"][b] and ref["active"][b] and not ref["converged"][b]
            assert ref["tr_u"][b] == 0.5 * state["tr_u"][b] and ref["tr_x"][b] == 0.5 * state["tr_x"][b] and ref["J"][b] == state["J"][b]
            assert rec["predicted"] > 1e-3 * state["J"][b] and np.isfinite(state["J"][b])
        else:
            assert np.isfinite(ref["J_new"][b]) and np.isfinite(rec["ratio"])
    assert dc.ratio_margin([ref["records"][b] for b in range(6) if b not in mc.NONFINITE_ROWS]) > 1e-2


@pytest.mark.parametrize("params", mc.DECISION_PARAMS)
def test_recorded_candidate_constant_is_current(params):
    v, c = mc.candidate_fp64_vs_ld(params), mc.CANDIDATE_FP64_VS_LD[params]
    print(f"candidates, {params}: fp64 vs long double {v:.3e}")
    assert v <= c <= 2.0 * v


def test_the_recorded_lockstep_selection_is_what_its_criterion_gives():
    assert mc.LOCKSTEP_KEEP == mc.lockstep_select()


def test_lockstep_preconditions_hold_with_ten_times_the_margin():
    """The host model of the lockstep test with the CPU oracle as QP solver: _scvx_device_case.lockstep_preconditions holds at ten
    times the margin the GPU test asks for; LOCKSTEP_FP64_VS_LD is what NumPy differs from long double over this run."""
    host = mc.lockstep_host()
    solve = case.oracle_qp_solver(**mc.LOCKSTEP_QP)
    p = host.p
    worst = dict(x=0.0, A=0.0, B=0.0, q=0.0)
    for it in range(mc.LOCKSTEP["max_outer"]):
        assert host.active.any()
        qp = host.qp()
        xprev = np.concatenate([host.x0[:, None, :], host.xb[:, :-1, :]], axis=1)
        A, Bm = mc.ld_linearise(xprev, host.ub, p)
        q = dc.linear_term(host.xb, host.ub, p.Q, p.R, p.QN, mc.LD)
        out = host.advance(solve(qp)[0], it)
        x = mc.ld_rollout(host.x0, out["u_new"], p)
        for k, a, b in (("A", qp.A, A), ("B", qp.B, Bm), ("q", qp.q.reshape(q.shape), q), ("x", out["x_new"], x)):
            worst[k] = max(worst[k], float(np.abs(a - b).max()))
    seen = dc.lockstep_preconditions(host, margin=10.0)
    print("lockstep with the oracle:", {k: v for k, v in seen.items() if k != "mixed"}, len(seen["mixed"]), "mixed; fp64 vs long double",
          {k: f"{v:.3e}" for k, v in worst.items()}, f"; |x| up to {np.abs(host.xb).max():.2f}")
    for k in worst:
        assert worst[k] <= mc.LOCKSTEP_FP64_VS_LD[k] <= 2.0 * worst[k], (k, worst[k])
