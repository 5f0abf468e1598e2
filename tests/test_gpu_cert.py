"""On-device certificate: admm_get_certificate / admm_get_certificate_device against the NumPy reference
tests/_cert_ref.py (one segment, sequential) on the (z, y) the handle returns.

Tolerance: the project's 1e-10, relative to max(1, max |nu|) of the QP for nu and stat, to max(1, sum |terms|)
for obj and to max(1, max |z|) for feas_dyn: the two sides differ in summation order (and in the segment link) only.

The sweep over every compiled pair at the edges of the LDS refill loop (test 1b) compares with the same definitions in
np.longdouble and adds a rounding-level bound on the same scales (M_CERT)."""
import ctypes as C

import numpy as np
import pytest
import torch

import admm_library_amd as pkg
import _cert_ref as cr
import _fuel_ref as fr
import _indep
import _readout_cases as rc
from _readout_cases import lti as _lti, stage_fuel as _stage_fuel
from _shapes import CHUNK_EDGE_CASES, SHARED, sid
from admm_library_amd import _abi

pytestmark = pytest.mark.gpu

CODE = {v: k for k, v in _abi.STATUS_NAMES.items()}
DEV = "cuda:0"
TOL = 1e-10


# (id, problem factory, options)
CASES = [
    ("ltv_4x2_b3_seg1", lambda: pkg.random_ltv(13, 4, 2, 3, seed=41), dict(rho=0.3, segments=1)),
    ("ltv_4x2_b70_seg4", lambda: pkg.random_ltv(13, 4, 2, 70, seed=42), dict(rho=0.3, segments=4)),
    ("ltv_4x2_b300_segN_noalt", lambda: pkg.random_ltv(13, 4, 2, 300, seed=43), dict(rho=0.3, segments=13, flags=_abi.FLAG_NO_ALTERNATE)),
    ("lti_4x2_b70_seg4_noq", lambda: _lti(pkg.random_ltv(13, 4, 2, 70, seed=44, with_q=False)), dict(rho=0.3, segments=4)),
    ("ltv_6x3_b70_seg4", lambda: pkg.random_ltv(50, 6, 3, 70, seed=45), dict(rho=0.3, segments=4)),
    ("ltv_6x3_b300_seg1_unfused", lambda: pkg.random_ltv(50, 6, 3, 300, seed=46), dict(rho=0.3, segments=1, flags=_abi.FLAG_UNFUSED)),
    # a segment longer than the LDS chunk (75 stages against 64) on the default path: k = 1, 7, 8 cover both parkings of the state
    ("ltv_6x3_N150_b70_seg2", lambda: pkg.random_ltv(150, 6, 3, 70, seed=55), dict(rho=0.3, segments=2)),
    ("ltv_6x3_b3_segN_noq", lambda: pkg.random_ltv(50, 6, 3, 3, seed=47, with_q=False), dict(rho=0.3, segments=50)),
    ("cw_6x3_b70_seg4", lambda: pkg.cw_rendezvous(N=50, batch=70), dict(rho=0.05, segments=4)),
    ("cw_6x3_b300_auto", lambda: pkg.cw_rendezvous(N=50, batch=300), dict(rho=0.05)),
    ("ltv_6x3_thrust_b70_seg4", lambda: pkg.random_ltv(50, 6, 3, 70, seed=48, thrust_norm=True), dict(rho=0.3, segments=4)),
    ("lti_6x3_thrust_b3_seg4_noalt", lambda: _lti(pkg.random_ltv(50, 6, 3, 3, seed=49, thrust_norm=True)),
     dict(rho=0.3, segments=4, flags=_abi.FLAG_NO_ALTERNATE)),
    ("cw_fuel_b70_seg4", lambda: pkg.cw_rendezvous_fuel(N=50, batch=70), dict(rho=0.05, segments=4)),
    ("ltv_6x3_stage_fuel_b300_seg4", lambda: _stage_fuel(pkg.random_ltv(50, 6, 3, 300, seed=50, thrust_norm=True)), dict(rho=0.3, segments=4)),
    ("cw_6x3_b16_mfma", lambda: pkg.cw_rendezvous(N=50, batch=16), dict(rho=0.05, segments=4, precision_mode=_abi.PRECISION_FP64_MFMA)),
    ("ltv_12x6_b3_seg1", lambda: pkg.random_ltv(17, 12, 6, 3, seed=51), dict(rho=0.3, segments=1)),
    ("ltv_12x6_b70_seg4", lambda: pkg.random_ltv(17, 12, 6, 70, seed=52), dict(rho=0.3, segments=4)),
    ("ltv_12x6_b300_segN_noq", lambda: pkg.random_ltv(17, 12, 6, 300, seed=53, with_q=False), dict(rho=0.3, segments=17)),
    ("lti_12x6_b70_seg4_unfused", lambda: _lti(pkg.random_ltv(17, 12, 6, 70, seed=54)), dict(rho=0.3, segments=4, flags=_abi.FLAG_UNFUSED)),
]
IDS = [c[0] for c in CASES]
BY_ID = {c[0]: c for c in CASES}


def _scales(p, z, ref):
    b = p.batch
    return (np.maximum(1.0, np.abs(ref["nu"]).reshape(b, -1).max(axis=1)), np.maximum(1.0, ref["obj_abs"]),
            np.maximum(1.0, np.abs(z).reshape(b, -1).max(axis=1)))


def _compare(p, z, y, rho, c, fuel="problem"):
    """All four outputs of certificate `c` against the reference at (z, y); returns the worst error / tolerance ratio."""
    ref = cr.certificate(p, z, y, rho, fuel=fuel)
    s_nu, s_obj, s_z = _scales(p, z, ref)
    ratios = {"nu": (np.abs(c.nu - ref["nu"]).reshape(p.batch, -1).max(axis=1) / (TOL * s_nu)).max(),
              "stat": (np.abs(c.stat - ref["stat"]) / (TOL * s_nu)).max(),
              "obj": (np.abs(c.obj - ref["obj"]) / (TOL * s_obj)).max(),
              "feas_dyn": (np.abs(c.feas_dyn - ref["feas_dyn"]) / (TOL * s_z)).max()}
    print("error / tolerance:", {k: float(f"{v:.3g}") for k, v in ratios.items()})
    for name, r in ratios.items():
        assert r <= 1.0, (name, r)
    return ref


@pytest.mark.parametrize("k", [1, 7, 8])
@pytest.mark.parametrize("case", IDS)
def test_matches_reference_after_k_iterations(gpu, case, k):
    """1. Not converged, odd and even iteration counts (alternation parks the state differently), every path and problem
    class.  Measured worst error / tolerance ratio over all cases on the MI355X: see DESIGN.md §2.9."""
    _, make, kw = BY_ID[case]
    p = make()
    with pkg.Solver(p, pkg.Options(**kw)) as s:
        if "segN" in case:
            assert s.geometry()["segments"] == p.N
        s.run(k)
        c = s.certificate(costates=True)
        _, z, y = s.get()
    assert c.nu.shape == (p.batch, p.N, p.n)
    _compare(p, z, y, kw["rho"], c)


# Rounding-level bound of the sweep below, per output: the device's worst error against the np.longdouble reference is at most M
# times that of the fp64 NumPy reference (floored at 2^-52), both on the scales of _compare.  MEASURED_RATIO is the worst
# e_dev / max(e_np, 2^-52) over the 87 cells on the MI355X; M is the next power of two at or above 4 x that (the 4 x for a
# compiler that orders or contracts the chains differently: the arithmetic is deterministic, so there is no run-to-run spread).
# Worst cells: nu (10, 4) refill, stat (5, 1) refill, obj (5, 1) fit, feas_dyn (12, 6) fit; the device's own worst errors are
# 1.0e-15, 7.8e-16, 9.6e-16 and 4.8e-16 x scale.
MEASURED_RATIO = {"nu": 1.87, "stat": 2.18, "obj": 4.33, "feas_dyn": 2.07}
M_CERT = {"nu": 8.0, "stat": 16.0, "obj": 32.0, "feas_dyn": 16.0}
LD = np.longdouble


@pytest.mark.parametrize("edge", CHUNK_EDGE_CASES)
@pytest.mark.parametrize("pair", SHARED, ids=sid)
def test_certificate_at_every_pair_and_chunk_edge(gpu, pair, edge):
    """1b. Every compiled (n, m) at the edges of the LDS refill loop (tests/_shapes.py: chunk_edge; CH = cert_chunk(n, m)):
      refill  one segment of 2 CH + 1 stages -- chunks CH, CH, 1: two refills, stage 0 (x0) alone in the last; q, thrust bounds,
              per-stage fuel weights
      fit     segments [0, CH) and [CH, 2 CH + 1) (seg_start[s] = floor(s N / S); asserted on the CPU in
              tests/test_readout_refs_host.py): segment 0, with stage 0, has exactly CH stages and must end without a refill,
              segment 1, with the terminal stage, has CH + 1; batch 261 = pitch 320, a second block with one active wave and three
              idle ones that must reach the barriers; LTI data and a shared box, expanded by the host; certificate() without
              costates must return the same bits
      stage   three one-stage segments: k = N - 1 (QN) and k = 0 (x0) each on its own
    on the plain one-lane path with the segment count given, so neither the host probe nor the batch chooses the kernels.
    All four outputs against the np.longdouble reference at the handle's (z, y): within 1e-10 x scale, and within M_CERT x the
    error of the fp64 NumPy reference.  Measured on the MI355X, worst ratio e_dev / max(e_np, 2^-52) over the 87 cells: nu 1.87,
    stat 2.18, obj 4.33, feas_dyn 2.07; hence M = 8, 16, 32, 16 (M_CERT above)."""
    p, S = rc.problem(pair, edge, probe=False)
    opt = pkg.Options(rho=rc.RHO, segments=S, flags=_abi.FLAG_NO_ALTERNATE | _abi.FLAG_NO_MFMA)
    with pkg.Solver(p, opt) as s:
        assert s.geometry()["segments"] == S and s.path()["kernel_family"] == "one_lane_fp64" and not s.path()["alternating"]
        s.run(rc.CERT_ITERS)
        c = s.certificate(costates=True)
        lean = s.certificate() if edge == "fit" else None
        _, z, y = s.get()
    assert c.nu.shape == (p.batch, p.N, p.n)
    if lean is not None:
        assert lean.nu is None
        for name in ("obj", "feas_dyn", "stat"):
            assert np.array_equal(getattr(lean, name), getattr(c, name)), name
    ld = cr.certificate(p, z, y, rc.RHO, dtype=LD)
    e_dev = rc.cert_errors(p, z, c, ld)
    e_np = rc.cert_errors(p, z, cr.certificate(p, z, y, rc.RHO), ld)
    print("RATIOS cert", sid(pair), edge, {k: (float(f"{e_dev[k]:.3g}"), float(f"{e_np[k]:.3g}"),
                                                 float(f"{e_dev[k] / max(e_np[k], rc.EPS64):.3g}")) for k in e_dev})
    for name in e_dev:
        rc.two_sided(name, e_dev[name], e_np[name], TOL, M_CERT[name])


@pytest.mark.parametrize("case", ["ltv_4x2_b70_seg4", "ltv_6x3_b70_seg4", "ltv_12x6_b70_seg4"])
def test_costates_close_the_kkt_system_independently(gpu, case):
    """2. With G from _indep.dynamics_matrix and the GPU's nu: max |g + G'nu| = stat_gpu, and the state rows vanish."""
    _, make, kw = BY_ID[case]
    p = make()
    with pkg.Solver(p, pkg.Options(**kw)) as s:
        s.run(7)
        c = s.certificate(costates=True)
        _, z, y = s.get()
    g = cr.gradient(p, z, y, kw["rho"]).reshape(p.batch, p.L)
    G = _indep.dynamics_matrix(p)
    res = (g + (G.T @ c.nu.reshape(p.batch, -1).T).T).reshape(p.batch, p.N, p.nb)
    scale = np.maximum(1.0, np.abs(c.nu).reshape(p.batch, -1).max(axis=1))
    assert np.all(np.abs(res[:, :, p.m:]).reshape(p.batch, -1).max(axis=1) <= TOL * scale)
    assert np.all(np.abs(np.abs(res).reshape(p.batch, -1).max(axis=1) - c.stat) <= TOL * scale)


@pytest.fixture(scope="module")
def fuel_solution():
    p = pkg.cw_rendezvous_fuel(N=150, batch=8)
    rho = 1.0
    ref = fr.solve(p, rho=rho, eps_abs=1e-8, eps_rel=1e-8, max_iter=6000, check_interval=10)
    assert ref.status.all()
    return p, rho, ref


def test_at_a_solution_of_the_fuel_problem(gpu, fuel_solution):
    """3. cw_rendezvous_fuel solved to 1e-8: stat against the reference and against a 1e-4 solve, Lawden's condition at the coast
    stages, the objective against the reference solution's."""
    p, rho, ref = fuel_solution
    opt = dict(rho=rho, max_iter=6000, check_interval=10)
    with pkg.Solver(p, pkg.Options(eps_abs=1e-8, eps_rel=1e-8, **opt)) as s:
        info = s.solve()
        assert info.n_converged == p.batch
        c = s.certificate(costates=True)
        _, z, y = s.get()
    with pkg.Solver(p, pkg.Options(eps_abs=1e-4, eps_rel=1e-4, **opt)) as s:
        s.solve()
        loose = s.certificate()
    stat_ref = cr.certificate(p, z, y, rho)["stat"]
    print("stat gpu", c.stat.max(), "ref", stat_ref.max(), "at 1e-4", loose.stat.min())
    assert np.all(c.stat <= 10.0 * stat_ref)
    assert np.all(c.stat < loose.stat) and np.all(stat_ref < loose.stat)
    A, B = _indep.stage_dynamics(p)
    primer = np.einsum("kij,bki->bkj", B, c.nu)                            # B_k' nu_{k+1}
    zu = z.reshape(p.batch, p.N, p.nb)[:, :, :p.m]
    coast = np.all(zu == 0.0, axis=2)
    assert coast.any()
    f = float(p.fuel)
    bound = f + np.sqrt(p.m) * c.stat[:, None]
    assert np.all(np.linalg.norm(primer, axis=2)[coast] <= np.broadcast_to(bound, coast.shape)[coast])
    obj_ref = cr.certificate(p, ref.z, ref.y, ref.rho)["obj"]
    assert np.all(np.abs(c.obj - obj_ref) <= 1e-5 * np.abs(obj_ref))


def test_state_handling_is_that_of_get(gpu):
    """4. run; certificate; run leaves the handle bit-identical to run; get; run -- on the alternating, the plain and the unfused
    path -- and a second certificate() returns the same bits."""
    p = pkg.cw_rendezvous(N=50, batch=70)
    for flags in (0, _abi.FLAG_NO_ALTERNATE, _abi.FLAG_UNFUSED):
        outs = []
        for use_cert in (True, False):
            with pkg.Solver(p, pkg.Options(rho=0.05, segments=4, flags=flags)) as s:
                s.run(9, 1)
                if use_cert:
                    c1 = s.certificate(costates=True)
                    c2 = s.certificate(costates=True)
                    for name in ("obj", "feas_dyn", "stat", "nu"):
                        assert np.array_equal(getattr(c1, name), getattr(c2, name)), name
                else:
                    s.get()
                s.run(9, 1)
                outs.append(s.get() + s.residuals())
        for a, b in zip(*outs):
            assert np.array_equal(a, b)


def test_freshness_after_set_rho_update_problem_set_fuel(gpu):
    """5. rho, the problem data and the fuel weights are those in force at the call."""
    p = pkg.random_ltv(13, 4, 2, 70, seed=61)
    p2 = pkg.random_ltv(13, 4, 2, 70, seed=62)
    with pkg.Solver(p, pkg.Options(rho=0.3, segments=4)) as s:
        s.run(5)
        s.certificate()                      # (operands of p are on the device now)
        s.set_rho(0.7)
        c = s.certificate(costates=True)
        _, z, y = s.get()
        _compare(p, z, y, 0.7, c)
        s.update_problem(p2)
        s.run(3)
        c = s.certificate(costates=True)
        _, z, y = s.get()
        _compare(p2, z, y, 0.7, c)
    pf = pkg.cw_rendezvous_fuel(N=50, batch=3)
    with pkg.Solver(pf, pkg.Options(rho=0.05, segments=4)) as s:
        s.run(8)
        c = s.certificate(costates=True)
        _, z, y = s.get()
        _compare(pf, z, y, 0.05, c)
        s.set_fuel(0.5)
        c2 = s.certificate(costates=True)
        _, z, y = s.get()
        ref = _compare(pf, z, y, 0.05, c2, fuel=0.5)
        # the same z under the new weights: obj moves by exactly (f_new - f_old) sum_k ||z_u,k||  (zero for a QP that has not
        # started to thrust after 8 iterations; positive for the others)
        thrust = np.linalg.norm(z.reshape(pf.batch, pf.N, pf.nb)[:, :, :pf.m], axis=2).sum(axis=1)
        assert thrust.max() > 0.0
        assert np.all(np.abs((c2.obj - c.obj) - (0.5 - float(pf.fuel)) * thrust) <= TOL * np.maximum(1.0, ref["obj_abs"]))
        assert np.all(c2.obj[thrust > 0] > c.obj[thrust > 0])


def _dp(t):
    return None if t is None else C.cast(C.c_void_p(t.data_ptr()), _abi.c_double_p)


def test_device_form(gpu):
    """6. Torch outputs (one a view at an 8-byte offset) equal the host form bit for bit; NULL combinations; host pointers and
    too-short allocations are refused with the argument named."""
    lib = pkg.load_library()
    p = pkg.random_ltv(13, 4, 2, 70, seed=71)
    dp = pkg.DeviceProblem.from_problem(p, DEV)
    stream = lambda: pkg.solver._stream(DEV)
    with pkg.Solver(p, pkg.Options(rho=0.3, segments=4)) as sh, pkg.Solver(dp, pkg.Options(rho=0.3, segments=4)) as sd:
        sh.run(7)
        sd.run(7)
        ch = sh.certificate(costates=True)
        cd = sd.certificate(costates=True)
        assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in (cd.obj, cd.feas_dyn, cd.stat, cd.nu))
        for name in ("obj", "feas_dyn", "stat", "nu"):
            assert np.array_equal(getattr(cd, name).cpu().numpy(), getattr(ch, name)), name
        assert sd.certificate().nu is None
        # a view at a storage offset of one element (8-byte, not 16-byte aligned); every NULL combination
        nn = p.batch * p.N * p.n
        for mask in range(16):
            bufs = [torch.full(((nn if j == 3 else p.batch) + 1,), -1.0, dtype=torch.float64, device=DEV) for j in range(4)]
            views = [b[1:] if mask >> j & 1 else None for j, b in enumerate(bufs)]
            rc = lib.admm_get_certificate_device(sd._h, *[_dp(v) for v in views], stream())
            assert rc == 0, lib.admm_last_error().decode()
            torch.cuda.synchronize()
            for j, name in enumerate(("obj", "feas_dyn", "stat", "nu")):
                got = bufs[j].cpu().numpy()
                assert got[0] == -1.0
                if views[j] is None:
                    assert (got == -1.0).all()
                else:
                    assert np.array_equal(got[1:], getattr(ch, name).reshape(-1)), (mask, name)
        # host and pinned pointers
        hostv = np.zeros(nn)
        pinned = torch.zeros(nn, dtype=torch.float64).pin_memory()
        for host in (_abi.dptr(hostv), _dp(pinned)):
            for j, name in enumerate(("obj", "feas_dyn", "stat", "nu")):
                args = [None] * 4
                args[j] = host
                assert lib.admm_get_certificate_device(sd._h, *args, stream()) == CODE["ADMM_ERR_INVALID"]
                assert f"admm_get_certificate_device: {name} is not device memory" in lib.admm_last_error().decode()
        assert (hostv == 0).all() and (pinned == 0).all()
        # too short: the last entries of an allocation that is a block of its own in torch's allocator (24 MiB, a multiple of the
        # 2 MiB granularity), so the runtime reports its true end
        big = torch.zeros(3 * 2 ** 20, dtype=torch.float64, device=DEV)
        for j, (name, need) in enumerate((("obj", p.batch), ("feas_dyn", p.batch), ("stat", p.batch), ("nu", nn))):
            args = [None] * 4
            args[j] = _dp(big[big.numel() - (need - 1):])
            assert lib.admm_get_certificate_device(sd._h, *args, stream()) == CODE["ADMM_ERR_INVALID"]
            msg = lib.admm_last_error().decode()
            assert f"admm_get_certificate_device: {name} ends before its {need} doubles" in msg, msg
        torch.cuda.synchronize()
        assert (big == 0).all()
        # the handle is unharmed
        sh.run(3)
        sd.run(3)
        for a, b in zip(sh.get(), sd.get()):
            assert np.array_equal(a, b)


def test_refusals_leave_the_handle_alone(gpu):
    """7. Per-instance dynamics and time-sharded handles: ADMM_ERR_UNSUPPORTED, and a following run matches a handle that never
    made the call."""
    lib = pkg.load_library()
    out = np.zeros(8)
    cases = [(pkg.random_instances(N=6, n=4, m=2, batch=3), dict(rho=0.3), None, "per-instance"),
             (pkg.cw_rendezvous(N=40, batch=4), dict(rho=0.05, segments=2), (0, 1, None), "time-sharded")]
    for p, kw, ts, word in cases:
        with pkg.Solver(p, pkg.Options(**kw), timeshard=ts) as s, pkg.Solver(p, pkg.Options(**kw), timeshard=ts) as twin:
            s.run(5)
            twin.run(5)
            with pytest.raises(pkg.AdmmError) as e:
                s.certificate(costates=True)
            assert e.value.code == CODE["ADMM_ERR_UNSUPPORTED"] and word in str(e.value)
            assert lib.admm_get_certificate_device(s._h, _abi.dptr(out), None, None, None, None) == CODE["ADMM_ERR_UNSUPPORTED"]
            assert word in lib.admm_last_error().decode()
            s.run(4)
            twin.run(4)
            for a, b in zip(s.get(), twin.get()):
                assert np.array_equal(a, b)
