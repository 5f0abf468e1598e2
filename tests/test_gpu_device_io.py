"""The device-memory entry points (ABI v9): admm_setup_device, admm_update_problem_device, admm_update_instances_device,
admm_set_state_device, admm_get_device -- and the Python surface over them (DeviceProblem, Solver with CUDA tensors,
Solver.get_device, scvx_batch(..., qp_data_on_device=True)).

The device forms read the caller's arrays with the same layout kernels the host forms feed from their staging buffer, so every
result is compared EXACTLY with the host form's: iterates, per-QP rho, path, per-QP info, and for refused data the status and
message.  A refused call must leave the handle bit for bit as it was (compared with a twin handle that saw no call)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import admm_library_amd as pkg
from admm_library_amd import _abi
from admm_library_amd import scvx as sc

pytestmark = pytest.mark.gpu

CODE = {v: k for k, v in _abi.STATUS_NAMES.items()}
DEV = "cuda:0"


def _stream():
    """torch's current stream as the hip_stream argument (synchronised and NULL if it is the null stream: solver._stream)."""
    return pkg.solver._stream(DEV)


# (id, problem factory (seed) -> Problem, options)
CASES = [
    ("pinst_6x3_one_lane_b70_auto", lambda s: pkg.random_instances(N=40, n=6, m=3, batch=70, seed=s), dict(rho=0.3)),
    ("pinst_6x3_one_lane_b70_seg2", lambda s: pkg.random_instances(N=40, n=6, m=3, batch=70, seed=s), dict(rho=0.3, segments=2)),
    ("pinst_6x3_rows_b16_auto", lambda s: pkg.random_instances(N=40, n=6, m=3, batch=16, seed=s), dict(rho=0.3)),
    ("pinst_6x3_rows_b16_seg1", lambda s: pkg.random_instances(N=40, n=6, m=3, batch=16, seed=s), dict(rho=0.3, segments=1)),
    ("pinst_12x6_tiled_box", lambda s: pkg.random_instances(N=24, n=12, m=6, batch=20, seed=s), dict(rho=0.3)),
    ("pinst_6x3_thrust_norm", lambda s: pkg.random_instances(N=40, n=6, m=3, batch=70, seed=s, thrust_norm=True), dict(rho=0.3)),
    ("shared_lti_fp64", lambda s: pkg.cw_rendezvous(N=100, batch=8, seed0=s), dict(rho=0.05)),
    ("shared_lti_mixed", lambda s: pkg.cw_rendezvous(N=100, batch=8, seed0=s), dict(rho=0.05, precision_mode=_abi.PRECISION_MIXED)),
    ("shared_ltv_fp64", lambda s: pkg.random_ltv(N=60, n=6, m=3, batch=8, seed=s), dict(rho=0.3)),
    ("shared_ltv_mixed", lambda s: pkg.random_ltv(N=60, n=6, m=3, batch=8, seed=s, with_q=False),
     dict(rho=0.3, precision_mode=_abi.PRECISION_MIXED)),
]
IDS = [c[0] for c in CASES]


def _opts(kw):
    return pkg.Options(max_iter=300, check_interval=10, eps_abs=1e-7, eps_rel=1e-7, **kw)


def _snapshot(s):
    """Everything a caller can read of a handle after a solve and 7 more iterations."""
    info = s.solve()
    s.iterate(7)
    return {"state": s.get(), "rho": s.rho_per_qp(), "path": s.path(),
            "info": (info.iters_run, info.n_converged, info.max_r, info.max_s, info.rho, info.rho_updates, info.mixed_iters,
                     info.iters, info.status, info.r, info.s)}


def _assert_same(a, b):
    for x, y in zip(a["state"], b["state"]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a["rho"], b["rho"])
    assert a["path"] == b["path"]
    for x, y in zip(a["info"], b["info"]):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("colmajor", [False, True], ids=["row_major", "colmajor"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_update_equals_host_update(gpu, case, colmajor, monkeypatch):
    _, make, kw = case
    if colmajor:
        monkeypatch.setenv("ADMM_PY_COLMAJOR", "1")
    else:
        monkeypatch.delenv("ADMM_PY_COLMAJOR", raising=False)
    p0, p1 = make(3), make(4)
    with pkg.Solver(p0, _opts(kw)) as sh, pkg.Solver(p0, _opts(kw)) as sd:
        sh.update_problem(p1)
        sd.update_problem(pkg.DeviceProblem.from_problem(p1, DEV))
        _assert_same(_snapshot(sh), _snapshot(sd))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_setup_from_device_problem_equals_setup_from_problem(gpu, case):
    _, make, kw = case
    p = make(5)
    with pkg.Solver(p, _opts(kw)) as sh, pkg.Solver(pkg.DeviceProblem.from_problem(p, DEV), _opts(kw)) as sd:
        assert sd._row_major == sh._row_major
        sh.run(6, residual_every=2)
        sd.run(6, residual_every=2)
        for x, y in zip(sh.get(), sd.get()):
            np.testing.assert_array_equal(x, y)
        _assert_same(_snapshot(sh), _snapshot(sd))


@pytest.mark.parametrize("case", [CASES[0], CASES[4], CASES[8]], ids=[IDS[0], IDS[4], IDS[8]])
def test_instances_state_and_read_out_through_tensors(gpu, case):
    _, make, kw = case
    p = make(6)
    rng = np.random.default_rng(9)
    x0 = p.x0 * 0.5 + 0.01
    q = None if p.q is None else rng.standard_normal(p.q.shape) * 0.01
    z, y = rng.standard_normal((p.batch, p.L)) * 0.1, rng.standard_normal((p.batch, p.L)) * 0.01
    t = lambda a: torch.as_tensor(a, device=DEV)           # noqa: E731
    with pkg.Solver(p, _opts(kw)) as sh, pkg.Solver(p, _opts(kw)) as sd:
        sh.update_instances(x0, q)
        sd.update_instances(t(x0), None if q is None else t(q))
        sh.set_state(z=z, y=y)
        sd.set_state(z=t(z), y=t(y))
        sh.iterate(9)
        sd.iterate(9)
        ref = sh.get()
        got = sd.get_device()
        for a, b in zip(ref, got):
            assert b.device == torch.device(DEV) and b.shape == (p.batch, p.L)
            np.testing.assert_array_equal(a, b.cpu().numpy())
        for a, b in zip(ref, sd.get()):
            np.testing.assert_array_equal(a, b)
        # read-out consumed on a non-default stream without a host synchronisation, right after asynchronous iterations
        sh.iterate(5)
        sd.iterate(5, sync=False)
        side = torch.cuda.Stream(DEV)
        with torch.cuda.stream(side):
            w2, z2, y2 = sd.get_device()
            checksum = (w2 * 2.0 + z2 - y2).sum(dim=1)       # queued on `side` behind the library's writes
        side.synchronize()
        w1, z1, y1 = (t(a) for a in sh.get())
        expect = (w1 * 2.0 + z1 - y1).sum(dim=1)
        np.testing.assert_array_equal(checksum.cpu().numpy(), expect.cpu().numpy())
        # a view at a storage offset of one element (8-byte, not 16-byte, aligned) as input and as output
        buf = torch.zeros(p.batch * p.L + 1, dtype=torch.float64, device=DEV)
        view = buf[1:].view(p.batch, p.L)
        assert view.storage_offset() == 1
        view.copy_(t(z))
        sh.set_state(z=z)
        sd.set_state(z=view)
        sh.iterate(3)
        sd.iterate(3)
        out = torch.full((p.batch * p.L + 1,), -1.0, dtype=torch.float64, device=DEV)
        ov = out[1:].view(p.batch, p.L)
        rc = pkg.load_library().admm_get_device(sd._h, None, C.cast(C.c_void_p(ov.data_ptr()), _abi.c_double_p), None, _stream())
        assert rc == 0
        np.testing.assert_array_equal(ov.cpu().numpy(), sh.get()[1])
        assert out[0].item() == -1.0                          # nothing written before the view


# ---- validation parity: the same bad data through both forms -----------------------------------------------------------------

def _bad_cases(p):
    """(kind, mutate(arrays: dict of A, B, lo, hi, q, unorm as writable NumPy arrays or torch tensors, flattened views), message)"""
    nbnd = p.lo.size
    i1, i2 = nbnd - 7 * p.nb + p.m + 1, nbnd - 3 * p.nb + p.m       # two late state rows, i1 < i2
    nan_at = p.A.size - 5

    def nan_in_A(a):
        a["A"][nan_at] = float("nan")

    def lo_gt_hi(a):
        for i in (i2, i1):
            a["lo"][i] = 2.0
            a["hi"][i] = 1.0

    def bounded_control_row(a):
        k = max(i for i in range(p.N) if np.isfinite(p.unorm[i]))   # the last stage with a finite unorm; QP batch - 3, control row 1
        a["lo"][((p.batch - 3) * p.N + k) * p.nb + 1] = -5.0

    def inf_in_q(a):
        a["q"][p.q.size - 11] = float("inf")
    return [("nan_in_A", nan_in_A, "non-finite entry in A, B, Q, R or QN"),
            ("lo_gt_hi", lo_gt_hi, f"lo > hi at bound index {i1}"),
            ("bounded_control_row", bounded_control_row, "control rows must be unbounded (-inf, inf) where unorm is finite"),
            ("inf_in_q", inf_in_q, "non-finite entry in q")]


def _flat(keep):
    out = {}
    for k in ("A", "B", "lo", "hi", "q"):
        v = keep[k]
        out[k] = v.reshape(-1)
    return out


@pytest.mark.parametrize("kind", ["nan_in_A", "lo_gt_hi", "bounded_control_row", "inf_in_q"])
def test_validation_parity_and_refused_handle_unchanged(gpu, kind):
    lib = pkg.load_library()
    p0 = pkg.random_instances(N=30, n=6, m=3, batch=70, seed=21, thrust_norm=True)
    assert p0.unorm is not None and np.isfinite(p0.unorm).any() and p0.per_instance_bounds
    p1 = pkg.random_instances(N=30, n=6, m=3, batch=70, seed=22, thrust_norm=True)
    _, mutate, msg = next(c for c in _bad_cases(p1) if c[0] == kind)
    kw = dict(rho=0.3)
    with pkg.Solver(p0, _opts(kw)) as sh, pkg.Solver(p0, _opts(kw)) as sd, pkg.Solver(p0, _opts(kw)) as twin:
        for s in (sh, sd, twin):
            s.iterate(4)
        cp, keep = _abi.marshal_problem(p1, sh._row_major)
        mutate(_flat(keep))
        rc_h = lib.admm_update_problem(sh._h, C.byref(cp))
        msg_h = lib.admm_last_error().decode()
        dp = pkg.DeviceProblem.from_problem(p1, DEV)
        cpd, keepd = _abi.marshal_device_problem(dp, sd._row_major)
        mutate(_flat(keepd))
        rc_d = lib.admm_update_problem_device(sd._h, C.byref(cpd), _stream())
        msg_d = lib.admm_last_error().decode()
        assert rc_h == rc_d == CODE["ADMM_ERR_INVALID"]
        assert msg_h == msg_d == msg
        for s in (sd, twin):
            s.iterate(6)
        _assert_same(_snapshot(sd), _snapshot(twin))


def test_device_checks_of_instances_and_state(gpu):
    lib = pkg.load_library()
    p = pkg.random_instances(N=30, n=6, m=3, batch=70, seed=23)
    with pkg.Solver(p, _opts(dict(rho=0.3))) as sd, pkg.Solver(p, _opts(dict(rho=0.3))) as twin:
        x0 = torch.as_tensor(p.x0 * 2.0, device=DEV)
        q = torch.as_tensor(p.q, device=DEV)
        q.view(-1)[123] = float("nan")
        with pytest.raises(ValueError, match="non-finite entry in x0"):
            sd.update_instances(torch.full_like(x0, float("inf")), q)
        with pytest.raises(pkg.AdmmError, match="non-finite entry in q"):
            sd.update_instances(x0, q)          # x0 is fine, q is not: x0 must not have been written either
        z = torch.zeros((p.batch, p.L), dtype=torch.float64, device=DEV)
        y = z.clone()
        y[5, 7] = float("-inf")
        with pytest.raises(pkg.AdmmError, match="non-finite entry in w, z or y"):
            sd.set_state(z=z, y=y)
        assert lib.admm_get_device(None, None, None, None, None) == CODE["ADMM_ERR_INVALID"]
        sd.iterate(5)
        twin.iterate(5)
        for a, b in zip(sd.get(), twin.get()):
            np.testing.assert_array_equal(a, b)


def test_host_checks_of_instances_and_state(gpu):
    """The host twin of test_device_checks_of_instances_and_state, through the C ABI (the Python wrapper would refuse a non-finite entry
    itself; a MATLAB or C host does not): everything is checked before anything of the handle is touched, so a refused call
    leaves it bit for bit as it was -- x0 in particular, which is fine in the two calls that are refused for their q."""
    lib = pkg.load_library()
    INVALID = CODE["ADMM_ERR_INVALID"]
    p = pkg.random_instances(N=30, n=6, m=3, batch=70, seed=23)
    noq = pkg.random_instances(N=30, n=6, m=3, batch=70, seed=23, with_q=False)
    assert p.q is not None and noq.q is None
    x0 = np.ascontiguousarray(p.x0 * 2.0)
    q_nan = np.ascontiguousarray(p.q).copy()
    q_nan.reshape(-1)[123] = float("nan")
    q_ok = np.ascontiguousarray(p.q)
    z = np.zeros((p.batch, p.L))
    y = z.copy()
    y[5, 7] = float("-inf")
    o = _opts(dict(rho=0.3))
    with pkg.Solver(p, o) as s, pkg.Solver(p, o) as twin, pkg.Solver(noq, o) as s_noq, pkg.Solver(noq, o) as twin_noq:
        for h in (s, twin, s_noq, twin_noq):
            h.iterate(4)
        assert lib.admm_update_instances(s._h, _abi.dptr(x0), _abi.dptr(q_nan)) == INVALID       # x0 is fine, q is not
        assert lib.admm_last_error().decode() == "non-finite entry in q"
        assert lib.admm_update_instances(s_noq._h, _abi.dptr(x0), _abi.dptr(q_ok)) == INVALID    # x0 is fine, q cannot be taken
        assert "handle was set up without q" in lib.admm_last_error().decode()
        for h in (s, s_noq):
            assert lib.admm_set_state(h._h, None, _abi.dptr(z), _abi.dptr(y)) == INVALID
            assert lib.admm_last_error().decode() == "non-finite entry in w, z or y"
        for h in (s, twin, s_noq, twin_noq):
            h.iterate(5)
        for h, t in ((s, twin), (s_noq, twin_noq)):
            for a, b in zip(h.get(), t.get()):
                np.testing.assert_array_equal(a, b)


def _ip(t):
    return C.cast(C.c_void_p(t.data_ptr()), _abi.c_int32_p)


@pytest.mark.parametrize("mode", ["stream", "null_stream"])
def test_host_and_device_forms_of_every_pair_are_bit_equal(gpu, mode):
    """One short call sequence on two handles, one through host arrays and one through device tensors -- every paired entry point:
    admm_update_instances, admm_set_state, admm_get, admm_get_certificate, admm_probe_infeasibility, admm_mpc_advance, and on a
    handle with 10 groups of 7 admm_get_consensus -- with hip_stream torch's current (side) stream, or NULL.  Every output and
    the state after 3 more iterations are equal bit for bit.  batch 70 in a pitch of 128: pad columns the transposes must not leak."""
    lib = pkg.load_library()
    p = pkg.random_ltv(N=30, n=6, m=3, batch=70, seed=61)
    rng = np.random.default_rng(62)
    B, L, N, n, m = p.batch, p.L, p.N, p.n, p.m
    x0 = p.x0 * 0.5 + 0.01
    q = rng.standard_normal((B, L)) * 0.01
    w, z, y = (rng.standard_normal((B, L)) * s for s in (0.1, 0.1, 0.01))
    du, dx, qt = rng.standard_normal((B, m)) * 0.01, rng.standard_normal((B, n)) * 0.01, rng.standard_normal((B, p.nb)) * 0.01
    t = lambda a: torch.as_tensor(a, device=DEV)           # noqa: E731
    empty = lambda *shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=DEV)      # noqa: E731
    host = lambda *ts: [a.cpu().numpy() for a in ts]        # noqa: E731  (on the current stream, behind the library's writes)

    def same(got, ref, what):
        for k, (a, b) in enumerate(zip(got, ref)):
            np.testing.assert_array_equal(a, np.asarray(b).reshape(a.shape), err_msg=f"{what}[{k}]")

    side = torch.cuda.Stream(DEV)
    opt = pkg.Options(rho=0.3, segments=3)
    torch.cuda.synchronize()
    with torch.cuda.stream(side if mode == "stream" else torch.cuda.current_stream(DEV)):
        assert bool(_stream().value) == (mode == "stream")
        with pkg.Solver(p, opt) as sh, pkg.Solver(p, opt) as sd:
            for s in (sh, sd):
                s.iterate(4)
            sh.update_instances(x0, q)
            sd.update_instances(t(x0), t(q))
            sh.set_state(w, z, y)
            sd.set_state(t(w), t(z), t(y))
            sh.iterate(3)
            sd.iterate(3, sync=False)
            same(host(*sd.get_device()), sh.get(), "get")
            ch = sh.certificate(costates=True)
            outs = [empty(B), empty(B), empty(B), empty(B, N, n)]
            assert lib.admm_get_certificate_device(sd._h, *[_dp(o) for o in outs], _stream()) == 0, lib.admm_last_error().decode()
            same(host(*outs), (ch.obj, ch.feas_dyn, ch.stat, ch.nu), "certificate")
            ih = sh.infeasibility(span=2, eps=1e-6, costates=True)
            outs, flag, nu = [empty(B), empty(B), empty(B)], empty(B, dtype=torch.int32), empty(B, N, n)
            assert lib.admm_probe_infeasibility_device(sd._h, 2, 1e-6, *[_dp(o) for o in outs], _ip(flag), _dp(nu), _stream()) == 0
            same(host(*outs, flag, nu), (ih.sep, ih.drift, ih.defect, ih.infeasible, ih.nu), "infeasibility")
            same(host(*sd.mpc_advance(du=t(du), dx=t(dx), q_tail=t(qt), tail="zero")), sh.mpc_advance(du=du, dx=dx, q_tail=qt, tail="zero"), "mpc")
            sh.iterate(3)
            sd.iterate(3, sync=False)
            same(host(*sd.get_device()), sh.get(), "state after the sequence")
            same(sd.get(), sh.get(), "state, host read-out of the device handle")
        pc = dataclasses.replace(p, consensus=7)
        with pkg.Solver(pc, opt) as sh, pkg.Solver(pc, opt) as sd:
            sh.update_instances(x0, q)
            sd.update_instances(t(x0), t(q))
            sh.set_state(z=z, y=y)
            sd.set_state(z=t(z), y=t(y))
            sh.iterate(3)
            sd.iterate(3, sync=False)
            ubar = empty(10, N, m)
            assert lib.admm_get_consensus_device(sd._h, _dp(ubar), _stream()) == 0, lib.admm_last_error().decode()
            same(host(ubar), [sh.consensus()], "consensus")
            same(host(*sd.get_device()), sh.get(), "state of the consensus handle")
    torch.cuda.synchronize()


def test_numeric_refusal_through_the_device_path_leaves_the_handle_unchanged(gpu):
    from test_gpu_guards import _sensitive_instances
    p = _sensitive_instances()
    # conditioning bound (automatic segments): a faster-growing plant with hardly any control authority
    worse = dataclasses.replace(p, A=p.A + 0.3 * np.eye(2), B=p.B * 1e-3, x0=p.x0 + 1.0, lo=p.lo * 0.5, hi=p.hi * 0.5)
    # S_k not positive definite
    not_pd = dataclasses.replace(p, R=-0.5 * np.eye(1) - 10.0 * np.eye(1))
    with pkg.Solver(p, pkg.Options(rho=0.1)) as sd, pkg.Solver(p, pkg.Options(rho=0.1)) as twin:
        assert sd.geometry()["segments"] == 8 and sd.path()["auto_segments"]
        sd.iterate(4)
        twin.iterate(4)
        for bad in (worse, not_pd):
            with pytest.raises(pkg.AdmmError) as e:
                sd.update_problem(pkg.DeviceProblem.from_problem(bad, DEV))
            assert e.value.code == CODE["ADMM_ERR_NUMERIC"] and "refused" in str(e.value)
        sd.iterate(6)
        twin.iterate(6)
        _assert_same(_snapshot(sd), _snapshot(twin))
        ok = dataclasses.replace(p, x0=p.x0 * 0.5)              # an acceptable update still goes through (trial buffers reused)
        sd.update_problem(pkg.DeviceProblem.from_problem(ok, DEV))
        twin.update_problem(ok)
        sd.iterate(3)
        twin.iterate(3)
        for a, b in zip(sd.get(), twin.get()):
            np.testing.assert_array_equal(a, b)


# ---- pointer checks ----------------------------------------------------------------------------------------------------------

def _dp(t):
    return C.cast(C.c_void_p(t.data_ptr()), _abi.c_double_p)


def test_host_and_pinned_pointers_are_refused_with_the_argument_named(gpu):
    lib = pkg.load_library()
    p = pkg.random_instances(N=20, n=6, m=3, batch=16, seed=31)
    dp = pkg.DeviceProblem.from_problem(p, DEV)
    co = _opts(dict(rho=0.3, flags=_abi.FLAG_ROW_MAJOR)).to_c()
    hostv = np.zeros((p.batch, p.L))
    pinned = torch.zeros((p.batch, p.L), dtype=torch.float64).pin_memory()
    for host in (_abi.dptr(hostv), _dp(pinned)):
        for field in ("A", "lo", "x0", "q"):
            cp, keep = _abi.marshal_device_problem(dp, True)
            setattr(cp, field, host)
            h = C.c_void_p()
            assert lib.admm_setup_device(C.byref(h), C.byref(cp), C.byref(co), _stream()) == CODE["ADMM_ERR_INVALID"]
            assert not h.value
            msg = lib.admm_last_error().decode()
            assert f"admm_setup_device: {field} is not device memory" in msg, msg
        with pkg.Solver(dp, _opts(dict(rho=0.3))) as s:
            cp, keep = _abi.marshal_device_problem(dp, True)
            cp.B = host
            assert lib.admm_update_problem_device(s._h, C.byref(cp), _stream()) == CODE["ADMM_ERR_INVALID"]
            assert "admm_update_problem_device: B is not device memory" in lib.admm_last_error().decode()
            assert lib.admm_update_instances_device(s._h, None, host, _stream()) == CODE["ADMM_ERR_INVALID"]
            assert "admm_update_instances_device: q is not device memory" in lib.admm_last_error().decode()
            assert lib.admm_set_state_device(s._h, None, None, host, _stream()) == CODE["ADMM_ERR_INVALID"]
            assert "admm_set_state_device: y is not device memory" in lib.admm_last_error().decode()
            assert lib.admm_get_device(s._h, host, None, None, _stream()) == CODE["ADMM_ERR_INVALID"]
            assert "admm_get_device: w is not device memory" in lib.admm_last_error().decode()
    assert (hostv == 0).all() and (pinned == 0).all()
    # an array shorter than its size
    short = torch.zeros(p.batch * p.L - 1, dtype=torch.float64, device=DEV)
    with pkg.Solver(dp, _opts(dict(rho=0.3))) as s:
        rc = lib.admm_get_device(s._h, None, _dp(short), None, _stream())
        if rc != 0:           # (where the runtime reports the allocation's extent; torch's caching allocator may round it up)
            assert rc == CODE["ADMM_ERR_INVALID"] and "z" in lib.admm_last_error().decode()


def test_time_sharded_handles_refuse_the_device_forms(gpu):
    lib = pkg.load_library()
    p = pkg.cw_rendezvous(N=40, batch=4)
    dp = pkg.DeviceProblem.from_problem(p, DEV)
    zero = torch.zeros((p.batch, p.L), dtype=torch.float64, device=DEV)
    with pkg.Solver(p, pkg.Options(rho=0.05, segments=2), timeshard=(0, 1, None)) as s:
        cp, keep = _abi.marshal_device_problem(dp)
        for rc in (lib.admm_update_problem_device(s._h, C.byref(cp), _stream()),
                   lib.admm_update_instances_device(s._h, _dp(dp.x0), None, _stream()),
                   lib.admm_set_state_device(s._h, None, _dp(zero), None, _stream()),
                   lib.admm_get_device(s._h, None, _dp(zero), None, _stream())):
            assert rc == CODE["ADMM_ERR_UNSUPPORTED"]


# ---- batched SCvx ---------------------------------------------------------------------------------------------------------------

def test_scvx_batch_with_qp_data_on_device_equals_the_default_path(gpu):
    B, N = 64, 200
    dt = 2 * np.pi / N
    Q = np.diag([1, 1, 1, .1, .1, .1]) * dt * 1e-3
    R = np.eye(3) * dt * 0.05
    QN = np.diag([50., 50, 50, 20, 20, 20])
    rng = np.random.default_rng(11)
    x0 = np.array([10.0, 150.0, 30.0, 0.0, -15.0, 0.0]) * (1.0 + 0.05 * rng.standard_normal((B, 6)))
    kw = dict(tr_u=1.0, tr_x=100.0, max_outer=6, tol=1e-7, linearise_on=DEV)
    ref = sc.scvx_batch(x0, N, dt, Q, R, QN, -3.0, 3.0, **kw)
    got = sc.scvx_batch(x0, N, dt, Q, R, QN, -3.0, 3.0, qp_data_on_device=True, **kw)
    for a, b in zip(ref, got):
        assert a.outer_iterations == b.outer_iterations and a.accepted == b.accepted and a.converged == b.converged
        assert [h["accepted"] for h in a.history] == [h["accepted"] for h in b.history]
        assert [h["cost"] for h in a.history] == [h["cost"] for h in b.history]
        np.testing.assert_array_equal(a.u, b.u)
        np.testing.assert_array_equal(a.x, b.x)
        assert a.cost == b.cost
