"""On-device infeasibility probe: admm_probe_infeasibility / admm_probe_infeasibility_device against the NumPy
reference tests/_infeas_ref.py (one segment, sequential) on the handle's own two y arrays.

Tolerance: the project's 1e-10, relative to max(1, max |nu|) of the QP for nu, to max(1, sum |terms| / |mu|_inf) for
sep, to max(1, drift) for drift and to max(1, defect, max |nu| / |mu|_inf) for defect (an absolute error of 1e-10 max |nu| in
|mu - lambda|_inf, divided by |mu|_inf): the two sides differ in summation order (and in the segment link) only.

The sweep over every compiled pair at the edges of the LDS refill loop (test 1b) compares with the same table in np.longdouble
and adds a rounding-level bound on the same scales (M_PROBE)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import admm_library_amd as pkg
import _infeas_cases as ic
import _infeas_ref as ir
import _readout_cases as rc
from _shapes import CHUNK_EDGE_CASES, SHARED, sid
from admm_library_amd import _abi

pytestmark = pytest.mark.gpu

CODE = {v: k for k, v in _abi.STATUS_NAMES.items()}
DEV = "cuda:0"
TOL = 1e-10
NAMES = ("sep", "drift", "defect", "infeasible", "nu")


def _compare(p, y0, y1, span, eps, r):
    """All five outputs of probe `r` against the reference on (y0, y1); +inf must match as +inf."""
    ref = ir.probe(p, y0, y1, span, eps)
    ir.check(ref, r, eps, TOL)               # (the scales and the flag rule: shared with tests/test_gpu_sequences.py)
    return ref


# (n, m, N, segments)
SHAPES = [(2, 1, 13, 2), (6, 3, 24, 1), (6, 3, 24, 2), (6, 3, 24, 3), (6, 3, 24, 4), (6, 3, 150, 2), (12, 6, 40, 1), (12, 6, 40, 2)]


@pytest.mark.parametrize("batch", [3, 70, 300])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_m%d_N%d_seg%d" % s)
def test_matches_reference(gpu, shape, batch):
    """1. 20 iterations, then two probes of span 5 on a time-varying problem with one-sided boxes, q and thrust bounds on most
    stages: with the default eps (a QP with an open row gives +inf, others are flagged or not) and with eps = 1e3 (the open rule
    never applies: sep is finite wherever mu != 0).  The state box of random_ltv is shrunk to 0.3 of itself: as drawn it is
    never active within 25 iterations, y is 0 on every state row and the comparison would be one of zeros.  The y arrays are a
    twin's, read with get() around its run(5)."""
    n, m, N, seg = shape
    p = pkg.random_ltv(N, n, m, batch, seed=100 + N + seg, thrust_norm=True)
    p.lo[:, m:] *= 0.3
    p.hi[:, m:] *= 0.3
    opt = pkg.Options(rho=0.3, segments=seg)
    with pkg.Solver(p, opt) as s, pkg.Solver(p, opt) as twin:
        assert s.geometry()["segments"] == seg
        s.run(20)
        twin.run(20)
        ys = [twin.get()[2]]
        probes = []
        for eps in (1e-6, 1e3):
            probes.append(s.infeasibility(span=5, eps=eps, costates=True))
            twin.run(5)
            ys.append(twin.get()[2])
        for a, b in zip(s.get(), twin.get()):
            assert np.array_equal(a, b)
    assert probes[0].nu.shape == (batch, N, n)
    _compare(p, ys[0], ys[1], 5, 1e-6, probes[0])
    ref = _compare(p, ys[1], ys[2], 5, 1e3, probes[1])
    moving = ref["mu_max"] > 0.0                                     # (not a comparison of zeros)
    assert np.array_equal(np.isfinite(ref["sep"]), moving) and moving.sum() >= (20 if batch >= 70 else 1)


# Rounding-level bound of the sweep below, per output: the device's worst error against the np.longdouble reference is at most M
# times that of the fp64 NumPy reference (floored at 2^-52), both on the scales of _compare.  MEASURED_RATIO is the worst
# e_dev / max(e_np, 2^-52) over the 87 cells x 2 probes on the MI355X; M is the next power of two at or above 4 x that (the 4 x
# for a compiler that orders or contracts the chains differently: the arithmetic is deterministic, so there is no run-to-run spread).
# Worst cells: nu (1, 1) refill, sep (3, 1) fit, drift (12, 4) fit, defect (2, 1) fit; the device's own worst errors are 2.5e-16,
# 4.7e-16, 8.9e-17 and 2.6e-16 x scale (drift is one subtraction and one division per row: the same bits on both sides).
MEASURED_RATIO = {"nu": 1.00, "sep": 1.62, "drift": 0.40, "defect": 1.07}
M_PROBE = {"nu": 4.0, "sep": 8.0, "drift": 2.0, "defect": 8.0}
LD = np.longdouble


@pytest.mark.parametrize("edge", CHUNK_EDGE_CASES)
@pytest.mark.parametrize("pair", SHARED, ids=sid)
def test_probe_at_every_pair_and_chunk_edge(gpu, pair, edge):
    """1b. Every compiled (n, m) at the edges of the LDS refill loop (tests/_shapes.py: chunk_edge; CH = cert_chunk(n, m)):
      refill  one segment of 2 CH + 1 stages -- chunks CH, CH, 1 of A_k | B_k and of the box: two refills, stage 0 (x0) alone in
              the last; thrust bounds on most stages
      fit     segments [0, CH) and [CH, 2 CH + 1) (seg_start[s] = floor(s N / S); asserted on the CPU in
              tests/test_readout_refs_host.py): segment 0, with stage 0 and the x0 term, has exactly CH stages and must end
              without a refill, segment 1 has CH + 1; batch 261 = pitch 320, a second block with one active wave and three idle
              ones that must reach the barriers; LTI data and one shared box, expanded by the host
      stage   three one-stage segments: k = N - 1 and k = 0 each on its own
    on the plain one-lane path with the segment count given.  The twin-handle pattern of test_matches_reference: run(20), then
    probes of span 5 with eps = 1e-6 and eps = 1e3; the state box shrunk to 0.3 of itself.  All five outputs against the
    np.longdouble reference on the twin's y: +inf as +inf, flags equal (none sits within the tolerance of -eps: a condition
    tests/test_readout_refs_host.py keeps on the oracle's iterates, and the rule of _compare still applies), the four real outputs
    within 1e-10 x scale and within M_PROBE x the error of the fp64 NumPy reference.  Measured on the MI355X, worst ratio
    e_dev / max(e_np, 2^-52) over the 87 cells and both probes: nu 1.00, sep 1.62, drift 0.40, defect 1.07; hence M = 4, 8, 2, 8
    (M_PROBE above)."""
    p, S = rc.problem(pair, edge, probe=True)
    opt = pkg.Options(rho=rc.RHO, segments=S, flags=_abi.FLAG_NO_ALTERNATE | _abi.FLAG_NO_MFMA)
    with pkg.Solver(p, opt) as s, pkg.Solver(p, opt) as twin:
        assert s.geometry()["segments"] == S and s.path()["kernel_family"] == "one_lane_fp64" and not s.path()["alternating"]
        s.run(rc.PROBE_ITERS)
        twin.run(rc.PROBE_ITERS)
        ys = [twin.get()[2]]
        probes = []
        for eps in rc.PROBE_EPS:
            probes.append(s.infeasibility(span=rc.PROBE_SPAN, eps=eps, costates=True))
            twin.run(rc.PROBE_SPAN)
            ys.append(twin.get()[2])
        for a, b in zip(s.get(), twin.get()):
            assert np.array_equal(a, b)
    assert probes[0].nu.shape == (p.batch, p.N, p.n)
    for i, (eps, r) in enumerate(zip(rc.PROBE_EPS, probes)):
        ld = ir.probe(p, ys[i], ys[i + 1], rc.PROBE_SPAN, eps, dtype=LD)
        f64 = ir.probe(p, ys[i], ys[i + 1], rc.PROBE_SPAN, eps)
        assert np.array_equal(np.isinf(r.sep), np.isinf(ld["sep"])) and np.all(r.sep[np.isinf(r.sep)] > 0)
        assert np.array_equal(np.isinf(r.defect), np.isinf(ld["defect"]))
        fs = np.isfinite(ld["sep"])
        near = fs & (np.abs(np.where(fs, ld["sep"], 0.0) + LD(eps)) <= TOL * np.maximum(1.0, ld["sep_abs"]))
        assert r.infeasible.dtype == np.int32 and np.array_equal(r.infeasible[~near], ld["infeasible"][~near])
        e_dev = rc.probe_errors(p, r, ld)
        e_np = rc.probe_errors(p, f64, ld)
        print("RATIOS probe", sid(pair), edge, eps, {k: (float(f"{e_dev[k]:.3g}"), float(f"{e_np[k]:.3g}"),
                                                          float(f"{e_dev[k] / max(e_np[k], rc.EPS64):.3g}")) for k in e_dev},
              "mu_max > 0:", int((ld["mu_max"] > 0).sum()), "finite sep:", int(fs.sum()), "flags:", int(ld["infeasible"].sum()))
        for name in e_dev:
            rc.two_sided(name, e_dev[name], e_np[name], TOL, M_PROBE[name])
        assert (ld["mu_max"] > 0).any()                              # (not a comparison of zeros)


@pytest.fixture(scope="module")
def classified():
    """The four classification problems on the GPU at the host test's iterations, costates included; computed once."""
    out = {}
    for case, (make, its, _, _, _) in ic.CASES.items():
        p = make()
        with pkg.Solver(p, pkg.Options(rho=ic.RHO)) as s:
            s.run(its[0])
            out[case] = (p, s.infeasibility(span=its[1] - its[0], eps=ic.EPS, costates=True))
    return out


@pytest.mark.parametrize("case", list(ic.CASES))
def test_classification(gpu, classified, case):
    """2. The flags are the expected sets; sep agrees with the reference on the oracle's iterates to 1e-6 relative."""
    p, r = classified[case]
    _, _, _, host = ic.oracle_probe(case)
    print(case, "sep gpu", r.sep, "host", host["sep"], "drift", r.drift, "defect", r.defect)
    assert r.infeasible.tolist() == ic.CASES[case][2]
    assert np.array_equal(np.isinf(r.sep), np.isinf(host["sep"]))
    fin = np.isfinite(host["sep"])
    assert np.all(np.abs(r.sep - host["sep"])[fin] <= 1e-6 * np.abs(host["sep"])[fin])


@pytest.mark.parametrize("case", list(ic.CASES))
def test_device_costates_prove_infeasibility_independently(gpu, classified, case):
    """3. For every flagged QP the device's nu satisfies the Farkas inequality in the dense restatement (G, h of
    oracle/admm_ref.dense_qp, sigma_C row by row), which also reproduces the device's sep."""
    p, r = classified[case]
    assert r.infeasible.any()
    for b in np.flatnonzero(r.infeasible):
        dense = ir.dense_farkas(p, b, r.nu[b], ic.EPS)
        print(case, b, "dense", dense, "gpu", r.sep[b])
        assert dense < -ic.EPS
        assert abs(dense - r.sep[b]) <= 1e-9 * max(1.0, abs(dense))


def _info(s):
    iters, status = np.empty(s.batch, np.int32), np.empty(s.batch, np.int32)
    assert s._lib.admm_get_info(s._h, _abi.iptr(iters), _abi.iptr(status), None, None) == 0
    return iters, status


STATE_CASES = {
    "alternating": (lambda: pkg.cw_rendezvous(N=50, batch=70), dict(rho=0.05, segments=4)),
    "no_alternate": (lambda: pkg.cw_rendezvous(N=50, batch=70), dict(rho=0.05, segments=4, flags=_abi.FLAG_NO_ALTERNATE)),
    "unfused": (lambda: pkg.cw_rendezvous(N=50, batch=70), dict(rho=0.05, segments=4, flags=_abi.FLAG_UNFUSED)),
    "fuel": (lambda: pkg.cw_rendezvous_fuel(N=50, batch=70), dict(rho=0.05, segments=4)),
    "fp64_mfma_b16": (lambda: pkg.cw_rendezvous(N=50, batch=16), dict(rho=0.05, segments=4, precision_mode=_abi.PRECISION_FP64_MFMA)),
}


@pytest.mark.parametrize("case", list(STATE_CASES))
def test_state_is_that_of_get_run_get(gpu, case):
    """4. infeasibility(span=7); run(4); get() equals, bit for bit, a twin's get(); run(7); get(); run(4); get().  iters and status
    are untouched."""
    make, kw = STATE_CASES[case]
    p = make()
    with pkg.Solver(p, pkg.Options(**kw)) as s, pkg.Solver(p, pkg.Options(**kw)) as twin:
        if case == "alternating":
            assert s.path()["alternating"]
        s.run(6, 3)
        twin.run(6, 3)
        before = _info(s)
        r = s.infeasibility(span=7)
        assert r.nu is None
        for a, b in zip(before, _info(s)):
            assert np.array_equal(a, b)
        twin.get()
        twin.run(7)
        mid = twin.get()
        for a, b in zip(s.get(), mid):
            assert np.array_equal(a, b)
        s.run(4)
        twin.run(4)
        for a, b in zip(s.get(), twin.get()):
            assert np.array_equal(a, b)
        for a, b in zip(_info(s), _info(twin)):
            assert np.array_equal(a, b)


def _dp(t):
    return None if t is None else C.cast(C.c_void_p(t.data_ptr()), _abi.c_double_p)


def _ip(t):
    return None if t is None else C.cast(C.c_void_p(t.data_ptr()), _abi.c_int32_p)


def test_device_form(gpu):
    """5. Torch outputs (views at a storage offset of one element) equal the host form bit for bit; every NULL combination; host
    pointers and too-short allocations are refused with the argument named."""
    lib = pkg.load_library()
    p = pkg.random_ltv(13, 4, 2, 70, seed=71, thrust_norm=True)
    p.lo[:, p.m:] *= 0.3                                 # (an active state box, as in test_matches_reference)
    p.hi[:, p.m:] *= 0.3
    dp = pkg.DeviceProblem.from_problem(p, DEV)
    stream = lambda: pkg.solver._stream(DEV)
    opt = pkg.Options(rho=0.3, segments=4)
    with pkg.Solver(p, opt) as sh, pkg.Solver(dp, opt) as sd:
        sh.run(7)
        sd.run(7)
        ch = sh.infeasibility(span=5, eps=1e3, costates=True)
        cd = sd.infeasibility(span=5, eps=1e3, costates=True)
        assert all(isinstance(getattr(cd, k), torch.Tensor) and getattr(cd, k).is_cuda for k in NAMES)
        assert cd.infeasible.dtype == torch.int32 and np.isfinite(ch.sep).sum() >= 20
        for name in NAMES:
            assert np.array_equal(getattr(cd, name).cpu().numpy(), getattr(ch, name)), name
        assert sd.infeasibility(span=1).nu is None
        sh.infeasibility(span=1)
        nn = p.batch * p.N * p.n
        for mask in range(32):
            ch = sh.infeasibility(span=1, eps=1e3, costates=True)
            bufs = [torch.full(((nn if j == 4 else p.batch) + 1,), -1, dtype=torch.int32 if j == 3 else torch.float64, device=DEV)
                    for j in range(5)]
            views = [b[1:] if mask >> j & 1 else None for j, b in enumerate(bufs)]
            rc = lib.admm_probe_infeasibility_device(sd._h, 1, 1e3, _dp(views[0]), _dp(views[1]), _dp(views[2]), _ip(views[3]),
                                                     _dp(views[4]), stream())
            assert rc == 0, lib.admm_last_error().decode()
            torch.cuda.synchronize()
            for j, name in enumerate(NAMES):
                got = bufs[j].cpu().numpy()
                assert got[0] == -1
                if views[j] is None:
                    assert (got == -1).all()
                else:
                    assert np.array_equal(got[1:], getattr(ch, name).reshape(-1)), (mask, name)
        # host and pinned pointers
        hostv = np.zeros(nn)
        pinned = torch.zeros(nn, dtype=torch.float64).pin_memory()
        for host in (hostv.ctypes.data, pinned.data_ptr()):
            for j, name in enumerate(NAMES):
                args = [None] * 5
                args[j] = C.cast(C.c_void_p(host), _abi.c_int32_p if j == 3 else _abi.c_double_p)
                assert lib.admm_probe_infeasibility_device(sd._h, 1, 1e-6, *args, stream()) == CODE["ADMM_ERR_INVALID"]
                assert f"admm_probe_infeasibility_device: {name} is not device memory" in lib.admm_last_error().decode()
        assert (hostv == 0).all() and (pinned == 0).all()
        # too short: the last entries of an allocation that is a block of its own in torch's allocator (24 MiB, a multiple of the
        # 2 MiB granularity), so the runtime reports its true end
        big = torch.zeros(3 * 2 ** 20, dtype=torch.float64, device=DEV)
        bigi = big.view(torch.int32)
        for j, (name, need) in enumerate(zip(NAMES, (p.batch, p.batch, p.batch, p.batch, nn))):
            args = [None] * 5
            args[j] = _ip(bigi[bigi.numel() - (need - 1):]) if j == 3 else _dp(big[big.numel() - (need - 1):])
            assert lib.admm_probe_infeasibility_device(sd._h, 1, 1e-6, *args, stream()) == CODE["ADMM_ERR_INVALID"]
            msg = lib.admm_last_error().decode()
            unit = "int32 entries" if j == 3 else "doubles"
            assert f"admm_probe_infeasibility_device: {name} ends before its {need} {unit}" in msg, msg
        torch.cuda.synchronize()
        assert (big == 0).all()
        # the refused calls ran nothing: both handles are where the 34 accepted probes of span 1 (and the first of span 5) left them
        sh.run(3)
        sd.run(3)
        for a, b in zip(sh.get(), sd.get()):
            assert np.array_equal(a, b)


def test_refusals_leave_the_handle_alone(gpu):
    """6. Per-instance dynamics, time-sharded handles and MIXED: ADMM_ERR_UNSUPPORTED naming the reason; span = 0, eps = nan and
    eps = -1: ADMM_ERR_INVALID.  A following run matches a handle that never made the call."""
    lib = pkg.load_library()
    out = np.zeros(8)
    U, I = CODE["ADMM_ERR_UNSUPPORTED"], CODE["ADMM_ERR_INVALID"]
    ok = (10, 1e-6)
    cases = [(pkg.random_instances(N=6, n=4, m=2, batch=3), dict(rho=0.3), None, ok, U, "per-instance"),
             (pkg.cw_rendezvous(N=40, batch=4), dict(rho=0.05, segments=2), (0, 1, None), ok, U, "time-sharded"),
             (pkg.cw_formation(N=40, batch=4), dict(rho=0.05, precision_mode=_abi.PRECISION_MIXED), None, ok, U, "MIXED"),
             (pkg.cw_rendezvous(N=40, batch=4), dict(rho=0.05, segments=2), None, (0, 1e-6), I, "span"),
             (pkg.cw_rendezvous(N=40, batch=4), dict(rho=0.05, segments=2), None, (10, float("nan")), I, "eps"),
             (pkg.cw_rendezvous(N=40, batch=4), dict(rho=0.05, segments=2), None, (10, -1.0), I, "eps")]
    for p, kw, ts, (span, eps), code, word in cases:
        with pkg.Solver(p, pkg.Options(**kw), timeshard=ts) as s, pkg.Solver(p, pkg.Options(**kw), timeshard=ts) as twin:
            s.run(5)
            twin.run(5)
            with pytest.raises(pkg.AdmmError) as e:
                s.infeasibility(span=span, eps=eps, costates=True)
            assert e.value.code == code and word in str(e.value), str(e.value)
            assert lib.admm_probe_infeasibility_device(s._h, span, eps, _abi.dptr(out), None, None, None, None, None) == code
            assert word in lib.admm_last_error().decode()
            assert (out == 0).all()
            s.run(4)
            twin.run(4)
            for a, b in zip(s.get(), twin.get()):
                assert np.array_equal(a, b)


def test_update_problem_brings_the_new_box(gpu):
    """7. A QP flagged under |u| <= 1 is no longer flagged once admm_update_problem has widened the control box to |u| <= 100; the
    probe after the update matches the reference evaluated with the NEW box."""
    p = ic.di_pinned()
    wide = dataclasses.replace(p, lo=p.lo.copy(), hi=p.hi.copy())
    wide.lo[:, :p.m] = -100.0
    wide.hi[:, :p.m] = 100.0
    with pkg.Solver(p, pkg.Options(rho=ic.RHO)) as s:
        s.run(200)
        assert s.infeasibility(span=10, eps=ic.EPS).infeasible.tolist() == [0, 1, 1, 1, 1, 1]
        s.update_problem(wide)
        s.run(200)
        y0 = s.get()[2]
        r = s.infeasibility(span=10, eps=ic.EPS, costates=True)
        y1 = s.get()[2]
    print("sep after the update:", r.sep, "drift", r.drift)
    assert not r.infeasible.any()
    _compare(wide, y0, y1, 10, ic.EPS, r)
