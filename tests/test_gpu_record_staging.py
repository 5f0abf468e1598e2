"""Record staging of the one-lane fused kernels (DESIGN.md §4.5 "record staging"; xfze_kernel / xbze_kernel): the stage records of
a segment reach LDS chunk by chunk through an asynchronous copy into two buffers, the next chunk in flight while the stages of the
current one run.  What can go wrong is a stage reading a record that has not landed, or the other buffer's -- at chunk edges --, so
these tests sweep SEGMENT LENGTHS around the chunk sizes of both kernels (batch 64: one workgroup per segment) and compare the
iterates after 6 and 7 iterations (both directions; with residuals every iteration the lean forms run from the third on) with
the C oracle at the tolerance of tests/test_gpu_alternating.py.  The copy moves whole KiB pieces, so the device arrays carry a
KiB of slack: the host-side test of that (admm_record_alloc_check, applied by admm_setup and every refactor) is checked without
a GPU at the end of the file."""
import ctypes as C

import numpy as np
import pytest

import admm_library_amd as pkg
from admm_library_amd import _abi
from admm_library_amd.solver import AdmmError, _check
import oracle_c as oc

TOL = 1e-10                        # tests/test_gpu_alternating.py
ONE_LANE = _abi.FLAG_NO_MFMA       # small q-free batches of an MFMA-compiled shape default to the MFMA family
B = 64


def chunk(rec_doubles: int) -> int:
    """stage_chunk2 (csrc/admm_kernels.hpp) at prefetch depth 1: stages per LDS buffer, two buffers with their 16-double tails in
    64 KiB, at most 128."""
    return max(1, min(128, (4096 - 16) // rec_doubles))


def chunks(n: int, m: int):
    rfe, rbe = C.c_int32(), C.c_int32()
    lib = pkg.load_library()
    _check(lib, lib.admm_record_sizes_alt(n, m, C.byref(rfe), C.byref(rbe)))
    return chunk(rfe.value), chunk(rbe.value)


def edge_lengths(n: int, m: int):
    out = set()
    for ch in chunks(n, m):
        out |= {1, 2, ch - 1, ch, ch + 1, 2 * ch - 1, 2 * ch, 2 * ch + 1, 3 * ch + 2}
    return sorted(v for v in out if v >= 1)


def _close(a, b):
    return np.abs(a - b).max() <= TOL * max(1.0, np.abs(b).max())


def _check_6_and_7(p, rho, segments=1, alpha=1.0, every=1, lean=False, prepare=None):
    """6 and then 1 more iteration on one handle against the oracle's 6 and 7 from the same start (zero state)."""
    with pkg.Solver(p, pkg.Options(rho=rho, alpha=alpha, segments=segments, flags=ONE_LANE)) as s:
        if prepare is not None:
            p, rho = prepare(s)
        path = s.path()
        assert path["alternating"] and path["kernel_family"] == "one_lane_fp64"
        assert s.geometry()["segments"] == segments
        n0 = s.lean_iterations()
        done = 0
        for k in (6, 1):
            s.run(k, residual_every=every)
            done += k
            ref = oc.solve(p, rho=rho, alpha=alpha, max_iter=done, check_interval=1, eps_abs=0, eps_rel=0, stop=False)
            w, z, y = s.get()
            assert _close(w, ref["w"]) and _close(z, ref["z"]) and _close(y, ref["y"]), (p.N, done)
            if every:
                r, sd = s.residuals()[:2]
                assert np.abs(r - ref["r"]).max() <= 1e-10 and np.abs(sd - ref["s"]).max() <= 1e-10, (p.N, done)
        if lean:
            assert s.lean_iterations() > n0


@pytest.mark.gpu
@pytest.mark.parametrize("N", edge_lengths(6, 3))
def test_segment_lengths_around_the_chunk_edges(gpu, N):
    """(6, 3), one segment of N stages: N = 1, 2 and CH - 1 ... 3 CH + 2 for the chunk sizes of both kernels."""
    assert chunks(6, 3) == (16, 19)
    _check_6_and_7(pkg.cw_rendezvous(N=N, batch=B), 0.05, lean=N >= 2)


@pytest.mark.gpu
def test_unequal_segments(gpu):
    _check_6_and_7(pkg.cw_rendezvous(N=50, batch=B), 0.05, segments=3, lean=True)


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["1", "8"])
def test_scan_rows_of_one_slab_and_of_eight(gpu, monkeypatch, split):
    """The head's scan rows: one load per row when the scan wrote one slab (every batch that fills the chip; forced here at a
    small one), the sum of the slabs otherwise -- the same iterates either way."""
    monkeypatch.setenv("ADMM_SCAN_SPLIT", split)
    _check_6_and_7(pkg.cw_rendezvous(N=50, batch=B), 0.05, segments=3, lean=True)
    _check_6_and_7(pkg.random_ltv(N=39, n=6, m=3, batch=B, seed=31, thrust_norm=True), 0.3, segments=4, alpha=1.6)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [33, 39, 50])
def test_forms_without_residuals(gpu, N):
    """No residuals: the forms that neither read (XFREE = 1) nor write (XFREE = 2) the unbounded state rows."""
    _check_6_and_7(pkg.cw_rendezvous(N=N, batch=B), 0.05, every=0)


@pytest.mark.gpu
def test_linear_term_thrust_bound_and_relaxation(gpu):
    _check_6_and_7(pkg.random_ltv(N=39, n=6, m=3, batch=B, seed=31, thrust_norm=True), 0.3, alpha=1.6)


@pytest.mark.gpu
def test_wide_block(gpu):
    """(12, 6): a few stages per buffer, the 512-register forms."""
    chf, chb = chunks(12, 6)
    assert (chf, chb) == (4, 5)
    _check_6_and_7(pkg.cw_formation(N=3 * chb + 2, batch=B), 0.05, lean=True)
    _check_6_and_7(pkg.cw_formation(N=2 * chf, batch=B), 0.05, lean=True)


@pytest.mark.gpu
def test_tiny_blocks(gpu):
    """(2, 1): the whole record is a few registers, over a hundred stages per buffer; (1, 1): the 128-stage cap."""
    chf, chb = chunks(2, 1)
    assert chf < 128 and chb < 128
    _check_6_and_7(pkg.double_integrator(N=2 * max(chf, chb) + 1, batch=B), 1.0)
    assert chunks(1, 1) == (128, 128)
    _check_6_and_7(pkg.random_ltv(N=257, n=1, m=1, batch=B, seed=7, with_q=False, state_bounds=False), 0.3)


@pytest.mark.gpu
def test_after_set_rho(gpu):
    """admm_set_rho uploads new records into the arrays of admm_setup (their slack included)."""
    p = pkg.cw_rendezvous(N=39, batch=B)
    zero = np.zeros((B, p.L))

    def prepare(s):
        s.run(3, residual_every=1)
        s.set_rho(0.2)
        s.set_state(z=zero, y=zero)
        return p, 0.2
    _check_6_and_7(p, 0.05, lean=True, prepare=prepare)


@pytest.mark.gpu
def test_after_update_problem(gpu):
    p = pkg.cw_rendezvous(N=39, batch=B)
    p2 = pkg.cw_rendezvous(N=39, batch=B, seed0=4242, u_max=0.1)
    zero = np.zeros((B, p.L))

    def prepare(s):
        s.run(4, residual_every=1)
        s.update_problem(p2)
        s.set_state(z=zero, y=zero)
        return p2, 0.05
    _check_6_and_7(p, 0.05, lean=True, prepare=prepare)


def test_chunk_sizes_follow_the_record_layout(lib):
    """Two buffers, each with the 16-double tail and rounded up to a KiB, in 64 KiB -- for every compiled block."""
    for n in range(1, 13):
        for m in range(1, 7):
            rfe, rbe = C.c_int32(), C.c_int32()
            _check(lib, lib.admm_record_sizes_alt(n, m, C.byref(rfe), C.byref(rbe)))
            for rec in (rfe.value, rbe.value):
                ch = chunk(rec)
                buf = -(-((ch * rec + 16) * 8) // 1024) * 1024
                assert ch >= 2 and 2 * buf <= 65536, (n, m, rec, ch)
                pieces = -(-(ch * rec * 8) // 1024)
                assert pieces * 1024 <= buf              # the last KiB piece of a full chunk ends inside its own buffer


def test_record_allocations_carry_the_slack_of_the_copy(lib):
    """admm_record_alloc_check: the allocation must cover stages x bytes rounded up to the next KiB -- what the last piece of the
    last chunk reads.  admm_setup's allocation (records + 1 KiB) passes for every length; one without the slack does not."""
    need = C.c_int64()
    for n, m, N in ((6, 3, 1000), (6, 3, 1), (6, 3, 33), (12, 6, 14), (2, 1, 227), (1, 1, 257)):
        rfe, rbe = C.c_int32(), C.c_int32()
        _check(lib, lib.admm_record_sizes_alt(n, m, C.byref(rfe), C.byref(rbe)))
        for rec in (rfe.value, rbe.value):
            exact = N * rec * 8
            _check(lib, lib.admm_record_alloc_check(exact + 1024, N, rec * 8, C.byref(need)))
            assert need.value == -(-exact // 1024) * 1024 and exact <= need.value <= exact + 1008
            if exact % 1024:
                with pytest.raises(AdmmError, match="LDS-DMA"):
                    _check(lib, lib.admm_record_alloc_check(exact, N, rec * 8, None))
            with pytest.raises(AdmmError):
                _check(lib, lib.admm_record_alloc_check(need.value - 8, N, rec * 8, None))
    _check(lib, lib.admm_record_alloc_check(0, 0, 1984, None))
    with pytest.raises(AdmmError):
        _check(lib, lib.admm_record_alloc_check(-1, 1, 1984, None))
