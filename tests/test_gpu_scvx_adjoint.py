"""admm_scvx_adjoint_device and DeviceOuterStep.certify() (ADMM_HIP_HAS_SCVX_ADJOINT) on the GPU against
scvx.adjoint: the kernel alone on what the device prepare wrote, certify() against the host linearisation, the optional outputs
behind guard bands, the refusals, a caller's stream, the three model families, and scvx_batch(outer_on_device=True, certify=True).
Inputs, references and the recorded constants: tests/_scvx_adjoint_case.py (checked on the CPU by tests/test_scvx_adjoint_host.py)."""
import ctypes as C
import dataclasses
import math
import time

import numpy as np
import pytest
import torch          # before libadmm_hip.so is loaded (the `gpu` fixture): both then share one HIP runtime

from admm_library_amd import _abi
from admm_library_amd import scvx as sc
from admm_library_amd.solver import _stream

import _scvx_adjoint_case as ac
import _scvx_case as case
import _scvx_device_case as dc
import _scvx_models_case as mc
import _scvx_stage_case as st

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = 1
BOX = (-case.U_MAX, case.U_MAX)
FIELDS = ("nu", "primer", "grad", "dJdx0", "stat", "n_bound")
P = sc.DeviceOuterStep.ptr


def _t(a, dtype=None):
    return torch.as_tensor(np.array(a, dtype), device=DEV)


def _loop(x0, N, u, x, p=dc.ORIGINAL, **kw):
    """The loop object under a parameter set, its reference set to (u, x)."""
    kw = dict(dict(device=DEV, tol=dc.TOL, substeps=p.substeps, eps=p.fd_eps), **kw)
    loop = sc.DeviceOuterStep(x0, N, p.dt, *(np.array(a) for a in (p.Q, p.R, p.QN, p.u_lo, p.u_hi)), **kw)
    loop.t["ub"].copy_(_t(u))
    loop.t["xb"].copy_(_t(x))
    return loop


def _sizes(B, N):
    return dict(nu=B * N * 6, primer=B * N * 3, grad=B * N * 3, dJdx0=B * 6, stat=B, n_bound=B)


def _shapes(B, N):
    return dict(nu=(B, N, 6), primer=(B, N, 3), grad=(B, N, 3), dJdx0=(B, 6), stat=(B,), n_bound=(B,))


def _outputs(B, N, names=FIELDS, guard=0, fill=-7.0):
    """Output tensors by name, each inside a buffer of its own with `guard` entries of `fill` on both sides: (views, buffers)."""
    views, bufs = {}, {}
    for k in names:
        n = _sizes(B, N)[k]
        bufs[k] = torch.full((n + 2 * guard,), fill, dtype=torch.int32 if k == "n_bound" else torch.float64, device=DEV)
        views[k] = bufs[k][guard:guard + n]
    return views, bufs


def _call(lib, loop, outs, **replace):
    """admm_scvx_adjoint_device on the loop's tensors (some replaced), queued on torch's current stream."""
    a = dict(N=loop.N, batch=loop.batch, params=C.byref(loop.params), ub=P(loop.t["ub"]), A=P(loop.A), B=P(loop.B), q=P(loop.q))
    a.update(replace)
    out = a["out"] if "out" in a else C.byref(_abi.CScvxAdjointOut(**{k: P(v) for k, v in outs.items()}))
    return lib.admm_scvx_adjoint_device(0, a["N"], a["batch"], a["params"], a["ub"], a["A"], a["B"], a["q"], out, _stream(loop.device))


def _host(c):
    return {k: getattr(c, k) for k in FIELDS}


def _errors(got, ref):
    """Per output, max |got - ref| / max |nu| per trajectory (n_bound: whether equal)."""
    scale = ac.nu_scale(ref["nu"])
    err = ac.scaled_errors(got, {k: ref[k] for k in ("nu", "primer", "grad", "dJdx0")}, scale)
    err["stat"] = float((np.abs(got["stat"] - ref["stat"]) / scale).max())
    return err


@pytest.mark.parametrize("B,N", dc.SHAPES)
def test_the_kernel_alone_matches_the_host_recursion(gpu, lib, B, N):
    """The device prepare's A, B downloaded and fed to scvx.adjoint(A=, B=); the kernel on the same arrays.  Every output agrees to
    dc.GPU_MARGIN x ac.FP64_VS_LD[B, N] (what the fp64 host recursion differs from a long-double restatement of it on these inputs:
    3.6e-17 .. 1.2e-14 of max |nu| per trajectory), stat to grad's bound; n_bound exactly.  About a third of the controls sit on each
    bound."""
    x0, u, x = ac.scattered_clipped(B, N)
    loop = _loop(x0, N, u, x)
    loop.prepare()
    outs, _ = _outputs(B, N)
    assert _call(lib, loop, outs) == 0, lib.admm_last_error().decode()
    got = {k: v.cpu().numpy().reshape(_shapes(B, N)[k]) for k, v in outs.items()}
    ref = _host(sc.adjoint(x0, u, x, dc.DT, case.Q, case.R, case.QN, *BOX, A=loop.A.cpu().numpy(), B=loop.B.cpu().numpy()))
    err = _errors(got, ref)
    tol = dict(ac.FP64_VS_LD[B, N], stat=ac.FP64_VS_LD[B, N]["grad"])
    print(f"adjoint kernel B={B} N={N}:", {k: f"{v:.3e} (bound {dc.GPU_MARGIN * tol[k]:.1e})" for k, v in err.items()})
    np.testing.assert_array_equal(got["n_bound"], ref["n_bound"])
    for k, v in err.items():
        assert v <= dc.GPU_MARGIN * tol[k], (k, v)


@pytest.mark.parametrize("B,N", dc.SHAPES)
def test_certify_matches_the_host_adjoint_with_the_host_linearisation(gpu, B, N):
    """DeviceOuterStep.certify() against scvx.adjoint with scvx.linearise: the device's A, B differ from the host's by up to 5e-7
    per entry (tests/test_gpu_scvx_device.py), which ac.linearisation_bound carries through the long-double recursion to first
    order -- at (65, 64): 1.0e-3 of max |nu| on nu and dJdx0, 4.5e-5 on primer, grad and stat; the rounding of the recursion
    (dc.GPU_MARGIN x ac.FP64_VS_LD) is added.  The measured difference is printed next to the bound.  n_bound is exact."""
    x0, u, x = ac.scattered_clipped(B, N)
    loop = _loop(x0, N, u, x)
    c = loop.certify()
    got = {k: getattr(c, k).cpu().numpy() for k in FIELDS}
    assert {k: v.shape for k, v in got.items()} == _shapes(B, N) and got["n_bound"].dtype == np.int32
    A, Bm = ac.host_jacobians(B, N)
    ref = _host(sc.adjoint(x0, u, x, dc.DT, case.Q, case.R, case.QN, *BOX))
    bound = ac.linearisation_bound(A, Bm, ref["nu"])
    rounding = dict(ac.FP64_VS_LD[B, N], stat=ac.FP64_VS_LD[B, N]["grad"])
    err = _errors(got, ref)
    print(f"certify B={B} N={N}:", {k: f"{v:.3e} (bound {bound[k] + dc.GPU_MARGIN * rounding[k]:.1e})" for k, v in err.items()})
    np.testing.assert_array_equal(got["n_bound"], ref["n_bound"])
    for k, v in err.items():
        assert v <= bound[k] + dc.GPU_MARGIN * rounding[k], (k, v)
    lean = loop.certify(costates=False)
    assert lean.nu is None and lean.primer is None
    for k in FIELDS[2:]:
        assert torch.equal(getattr(lean, k), getattr(c, k)), k


def test_optional_outputs_guard_bands_and_refusals(gpu, lib):
    """(65, 64): each output alone gives the bits it has when all are asked for, and 64 guard entries on both sides of every
    output keep theirs.  Every field NULL, a host pointer (pageable or pinned) or an allocation that ends early, for every input and
    every output: ADMM_ERR_INVALID with the argument's name, and nothing is written."""
    B, N = 65, 64
    x0, u, x = ac.scattered_clipped(B, N)
    loop = _loop(x0, N, u, x)
    loop.prepare()
    G = 64
    full, fbufs = _outputs(B, N, guard=G)
    assert _call(lib, loop, full) == 0, lib.admm_last_error().decode()
    torch.cuda.synchronize()
    for k, b in fbufs.items():
        assert (b[:G] == -7).all() and (b[-G:] == -7).all(), k
        assert not (full[k] == -7).all(), k
    for k in FIELDS:
        one, bufs = _outputs(B, N, names=(k,), guard=G)
        assert _call(lib, loop, one) == 0, lib.admm_last_error().decode()
        torch.cuda.synchronize()
        assert (bufs[k][:G] == -7).all() and (bufs[k][-G:] == -7).all(), k
        assert torch.equal(one[k].view(torch.int32), full[k].view(torch.int32)), k         # the bits, NaN or not

    before = {k: v.clone() for k, v in fbufs.items()}

    def refused(word, **kw):
        assert _call(lib, loop, full, **kw) == INVALID, word
        msg = lib.admm_last_error().decode()
        assert msg.startswith("admm_scvx_adjoint_device: ") and word in msg, (word, msg)

    refused("every field of out is NULL", out=C.byref(_abi.CScvxAdjointOut()))
    refused("out is NULL", out=C.POINTER(_abi.CScvxAdjointOut)())
    refused("N must be >= 1", N=0)
    refused("batch must be >= 1", batch=0)
    hostv = np.zeros(B * N * 36)
    hosti = np.zeros(B, np.int32)
    pinned = torch.zeros(B * N * 36, dtype=torch.float64).pin_memory()
    big = torch.zeros(3 * 2 ** 20, dtype=torch.float64, device=DEV)      # a block of its own in torch's allocator: its true end is known
    bigi = big.view(torch.int32)

    def wrong(count, is_int):
        if is_int:
            yield "is not device memory", _abi.iptr(hosti)
            yield f"ends before its {count} int32 entries", P(bigi[bigi.numel() - (count - 1):])
        else:
            yield "is not device memory", _abi.dptr(hostv)
            yield "is not device memory", P(pinned)
            yield f"ends before its {count} doubles", P(big[big.numel() - (count - 1):])
    for arg, count in dict(ub=B * N * 3, A=B * N * 36, B=B * N * 18, q=B * N * 9).items():
        refused(f"{arg} is NULL", **{arg: _abi.c_double_p()})
        for word, p in wrong(count, False):
            refused(f"{arg} {word}", **{arg: p})
    for k, count in _sizes(B, N).items():
        for word, p in wrong(count, k == "n_bound"):
            refused(f"out.{k} {word}", out=C.byref(_abi.CScvxAdjointOut(**dict({f: P(v) for f, v in full.items()}, **{k: p}))))
    torch.cuda.synchronize()
    for k, v in fbufs.items():
        assert torch.equal(v.view(torch.int32), before[k].view(torch.int32)), k
    assert (big == 0).all() and (hostv == 0).all() and (hosti == 0).all() and (pinned == 0).all()


def test_the_call_is_ordered_on_a_callers_stream(gpu, lib):
    """The call behind a busy non-default stream: `side` is given a chain of fp64 matmuls (their number from one timed matmul, for
    >= 200 ms of work) that ends by writing ub, A, B, q into the tensors the call reads; the call is queued while the chain is still
    running (side.query() is False just before -- the test fails as vacuous otherwise), and only then is the stream waited for.  The
    outputs have the bits of the same call on the default stream."""
    B, N = 65, 64
    x0, u, x = ac.scattered_clipped(B, N)
    loop = _loop(x0, N, u, x)
    loop.prepare()
    want, _ = _outputs(B, N)
    assert _call(lib, loop, want) == 0, lib.admm_last_error().decode()
    torch.cuda.synchronize()
    src = dict(ub=loop.t["ub"], A=loop.A, B=loop.B, q=loop.q)
    dirty = {k: torch.full_like(v, 7.0) for k, v in src.items()}           # what a call that did not wait would read
    got, _ = _outputs(B, N)
    side = torch.cuda.Stream(device=DEV)
    assert side.cuda_stream != 0
    a = torch.eye(2048, dtype=torch.float64, device=DEV).roll(1, 0)
    bufs = [a.clone(), torch.empty_like(a)]
    torch.mm(a, bufs[0], out=bufs[1])                              # warm-up (library initialisation), then one timed product
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    torch.mm(a, bufs[1], out=bufs[0])
    torch.cuda.synchronize()
    count = max(16, math.ceil(0.2 / max(time.perf_counter() - t0, 1e-6)))
    try:
        with torch.cuda.stream(side):
            for i in range(count):
                torch.mm(a, bufs[i % 2], out=bufs[(i + 1) % 2])
            for k, v in dirty.items():
                v.copy_(src[k])
            busy = not side.query()
            rc = _call(lib, loop, got, **{k: P(v) for k, v in dirty.items()})
        side.synchronize()
    finally:
        del a, bufs
        torch.cuda.empty_cache()                                   # the 32 MB blocks go back: later tests expect fresh blocks for large tensors
    assert rc == 0, lib.admm_last_error().decode()
    assert busy, f"vacuous: the stream had already finished its {count} matmuls when the call was queued"
    for k in FIELDS:
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k


def _family(name):
    """(parameter set, model, x0, u, x) at (5, 12) for one model family: the box's clipped random controls, the host rollout."""
    B, N = 5, 12
    rng = np.random.default_rng(11)
    if name == "relative_circular":
        p, model = dc.ORIGINAL, sc.relative_circular()
        x0 = ac.scattered_clipped(B, N)[0]
    elif name == "crtbp":
        p, model = mc.EM_L2, mc.model_of(mc.EM_L2)
        x0 = mc.scattered(B, N, "em_l2")[0]
    else:
        p, model = st.ELLIPTIC, st.model_of(st.ELLIPTIC)
        x0 = ac.scattered_clipped(B, N)[0]
    u = np.clip(rng.uniform(3.0 * p.u_lo, 3.0 * p.u_hi, (B, N, 3)), p.u_lo, p.u_hi)
    x = sc.rollout(x0, u, p.dt, model=model)
    assert np.isfinite(x).all()
    return p, model, x0, u, x


@pytest.mark.parametrize("name", ["relative_circular", "crtbp", "elliptic"])
def test_certify_under_the_three_model_families(gpu, name):
    """certify() through admm_scvx_prepare_{device, model_device, stage_device} at (5, 12) against scvx.adjoint(model=...): the
    bound of the test above (the linearisation's 5e-7 carried through the recursion, plus the rounding recorded at (130, 65))."""
    p, model, x0, u, x = _family(name)
    loop = _loop(x0, 12, u, x, p, model=None if name == "relative_circular" else model)
    c = loop.certify()
    got = {k: getattr(c, k).cpu().numpy() for k in FIELDS}
    ref = _host(sc.adjoint(x0, u, x, p.dt, p.Q, p.R, p.QN, p.u_lo, p.u_hi, model=model))
    A, Bm = sc.linearise(np.concatenate([x0[:, None, :], x[:, :-1, :]], axis=1), u, p.dt, model=model)
    bound = ac.linearisation_bound(A, Bm, ref["nu"])
    rounding = dict(ac.FP64_VS_LD[130, 65], stat=ac.FP64_VS_LD[130, 65]["grad"])
    err = _errors(got, ref)
    print(f"certify {name}:", {k: f"{v:.3e} (bound {bound[k] + dc.GPU_MARGIN * rounding[k]:.1e})" for k, v in err.items()},
          "on a bound:", got["n_bound"].tolist())
    np.testing.assert_array_equal(got["n_bound"], ref["n_bound"])
    assert got["n_bound"].min() >= 12
    for k, v in err.items():
        assert v <= bound[k] + dc.GPU_MARGIN * rounding[k], (k, v)


def test_scvx_batch_on_the_device_with_the_certificate(gpu):
    """scvx_batch(outer_on_device=True, certify=True) at B = 5, N = 20 (stages of a twentieth of an orbit, so that the box does
    not hold every control): every other field of every result equals the certify=False
    run bit for bit, and the certificate has the bits of a separate certify() about the returned trajectories."""
    rng = np.random.default_rng(11)
    B, N = 5, 20
    x0s = case.X0[None] * (1.0 + 0.05 * rng.standard_normal((B, 6)))
    dt = 2 * np.pi / N
    args = (x0s, N, dt, case.Q, case.R, case.QN, *BOX)
    kw = dict(qp_options=case.QP, linearise_on=DEV, outer_on_device=True, **dict(case.SCVX, max_outer=6))
    plain = sc.scvx_batch(*args, **kw)
    res = sc.scvx_batch(*args, certify=True, **kw)
    for i, (r, o) in enumerate(zip(res, plain)):
        assert o.certificate is None and isinstance(r.certificate, sc.ScvxCertificate)
        for f in dataclasses.fields(sc.ScvxResult):
            if f.name in ("u", "x"):
                np.testing.assert_array_equal(getattr(r, f.name), getattr(o, f.name), err_msg=f"{f.name} of trajectory {i}")
            elif f.name != "certificate":
                assert getattr(r, f.name) == getattr(o, f.name), (f.name, i)
    loop = _loop(x0s, N, np.stack([r.u for r in res]), np.stack([r.x for r in res]), dc.ORIGINAL._replace(dt=dt), tol=case.SCVX["tol"])
    c = loop.certify()
    for k in FIELDS:
        got = np.stack([np.asarray(getattr(r.certificate, k)) for r in res])
        np.testing.assert_array_equal(got, getattr(c, k).cpu().numpy(), err_msg=k)
    print("scvx_batch on the device: stat", [f"{r.certificate.stat:.2e}" for r in res], "n_bound", [r.certificate.n_bound for r in res],
          "converged", [r.converged for r in res])
