"""The compiled shape lists (tests/_shapes.py) and the shape sweep's problem table, on the CPU: a pair added to or dropped from
the build changes a pinned list here until the sweeps are looked at, and a change of the forward-elimination probe that would
send a sweep cell to the plain kernels fails here before the GPU suite runs."""
import os
import re

import numpy as np
import pytest

import admm_library_amd as pkg
from admm_library_amd.solver import host_factor, host_scan_packed
from _shapes import (ALT_TABLE, CERT_CHUNK_CAP, CERT_LDS_DOUBLES, CHUNK_EDGE_CASES, CSRC, MFMA, PER_INSTANCE, PLAIN_ONLY, SCAN_EMPTY_SLICE, SCAN_GEOMETRIES, SCAN_REFACTOR_RHO,
                     SCAN_REFACTOR_SEED, SCAN_SLICEABLE, SHARED, SWEEP_N, SWEEP_SEGMENTS, WIDE, cert_chunk, chunk_edge, gid, scan_shape)
from _timeshard import ADAPT as TS_ADAPT, ADAPT_DOUBLINGS as TS_ADAPT_DOUBLINGS
from _timeshard import CASES as TS_CASES, RHO_FACTOR as TS_RHO_FACTOR, UPDATE_CASES as TS_UPDATE_CASES
from _timeshard import host_scan_timeshard as ts_host_scan, host_segments as ts_host_segments, second_problem as ts_second_problem


def test_compiled_shape_lists_are_pinned():
    assert SHARED == [(1, 1), (2, 1), (2, 2), (3, 1), (3, 2), (3, 3), (4, 1), (4, 2), (4, 3), (4, 4), (5, 1), (5, 2), (5, 3),
                      (6, 1), (6, 2), (6, 3), (6, 4), (6, 6), (7, 2), (7, 3), (8, 2), (8, 3), (8, 4), (9, 3), (10, 2), (10, 4),
                      (12, 3), (12, 4), (12, 6)]
    assert PER_INSTANCE == [(1, 1), (2, 1), (2, 2), (3, 2), (4, 1), (4, 2), (6, 1), (6, 2), (6, 3), (6, 4), (8, 4), (9, 3),
                            (12, 3), (12, 6)]
    assert WIDE == [(8, 4), (9, 3), (12, 3), (12, 6)]
    assert MFMA == [(6, 3), (10, 4), (12, 6)]
    assert (len(SHARED), len(PER_INSTANCE), len(WIDE), len(MFMA)) == (29, 14, 4, 3)
    assert set(WIDE) <= set(PER_INSTANCE) and set(MFMA) <= set(SHARED)


def test_sweep_table_covers_every_shared_pair(lib):
    assert sorted(ALT_TABLE) == SHARED
    assert set(PLAIN_ONLY) <= set(SHARED)
    for (n, m) in PLAIN_ONLY:          # (the GPU sweep asserts the warning and the plain path for these)
        seed, rho = ALT_TABLE[(n, m)]
        assert not host_factor(pkg.random_ltv(N=SWEEP_N, n=n, m=m, batch=7, seed=seed), rho, SWEEP_SEGMENTS)["alt_ok"]


@pytest.mark.parametrize("shape", [s for s in SHARED if s not in PLAIN_ONLY], ids=lambda s: f"n{s[0]}m{s[1]}")
def test_sweep_problems_pass_the_forward_elimination_probe(lib, shape):
    """Every pair the GPU sweep expects on the alternating path passes the probe, deterministically, whatever the form's
    problem data (q, state rows unbounded, thrust bound) and batch."""
    n, m = shape
    seed, rho = ALT_TABLE[shape]
    for with_q, xfree, soc, batch in ((False, False, False, 7), (True, True, True, 67)):
        p = pkg.random_ltv(N=SWEEP_N, n=n, m=m, batch=batch, seed=seed, with_q=with_q, state_bounds=not xfree, thrust_norm=soc)
        assert host_factor(p, rho, SWEEP_SEGMENTS)["alt_ok"], (shape, with_q, xfree, soc, batch)
        assert host_factor(p, rho, SWEEP_SEGMENTS)["alt_ok"]


SCAN_GROWTH_MAX = 100.0     # admm_setup's conditioning bound on max|W|, max|WB| (automatic segment counts; include/admm_hip.h)


def test_scan_geometry_table_covers_what_it_promises():
    """Widths, segment counts, S = N, S > N, unequal segments, N <= 200, only compiled pairs, one m per n."""
    G = SCAN_GEOMETRIES
    assert len(set(g[:4] for g in G)) == len(G)
    assert all((n, m) in SHARED and N <= 200 for n, m, N, _, _, _ in G)
    widths = {}
    for n, m, *_ in G:
        widths.setdefault(n, set()).add(m)
    assert set(widths) == {1, 2, 5, 6, 7, 12} and all(len(v) == 1 for v in widths.values())
    assert {S for _, _, _, S, _, _ in G} == {1, 2, 3, 11, 21, 43, 64}
    assert sum(S == N for _, _, N, S, _, _ in G) == 1 and sum(S > N for _, _, N, S, _, _ in G) == 1
    assert all(N % S != 0 for _, _, N, S, _, _ in G if 1 < S < N)
    assert {g[:2] for g in SCAN_SLICEABLE} & set(MFMA) and {g[:2] for g in SCAN_EMPTY_SLICE} & set(MFMA)
    assert len(SCAN_SLICEABLE) >= 3 and len(SCAN_EMPTY_SLICE) >= 2 and not set(SCAN_SLICEABLE) & set(SCAN_EMPTY_SLICE)
    assert max(scan_shape(n, N, S)[2] for n, _, N, S, _, _ in G) == 1568 and max(scan_shape(n, N, S)[3] for n, _, N, S, _, _ in G) == 24


@pytest.mark.parametrize("geom", SCAN_GEOMETRIES, ids=gid)
def test_scan_geometries_pass_the_probe_and_the_growth_bound(lib, geom):
    """Every entry of the geometry table runs the alternating kernels (alt_check <= alt_gate) whatever the form's problem data,
    keeps both scan matrices inside the conditioning bound, and is listed as sliceable / empty-slice exactly when the packed
    k-step ranges of W say so."""
    n, m, N, S, seed, rho = geom
    for with_q, xfree, soc, batch in ((False, False, False, 5), (True, True, True, 67)):
        p = pkg.random_ltv(N=N, n=n, m=m, batch=batch, seed=seed, with_q=with_q, state_bounds=not xfree, thrust_norm=soc)
        hf = host_factor(p, rho, S)
        assert hf["alt_ok"], (geom, with_q, xfree, soc, batch)
        assert len(hf["seg_start"]) == min(S, N) + 1
        growth = np.abs(hf["scanW"]).max(), np.abs(hf["scanWB"]).max()
        assert max(growth) <= SCAN_GROWTH_MAX, (geom, growth)
    _, rng, M, K = host_scan_packed(p, rho, S)
    assert (min(S, N), M, K, len(rng)) == scan_shape(n, N, S)
    widest = int((rng[:, 1] - rng[:, 0]).max()) // 8          # batches of SCAN_U = 8 k-steps
    assert (geom in SCAN_SLICEABLE) == (widest >= 8), (geom, widest)
    assert (geom in SCAN_EMPTY_SLICE) == (S <= 4 and widest < 4), (geom, widest)


@pytest.mark.parametrize("case", TS_CASES)
def test_timeshard_cases_pass_the_growth_bound(lib, case):
    """Every case of tests/test_gpu_timeshard_ranks.py -- with the rho values and the second problem its state changes move a
    handle to -- keeps both scan matrices, in the rank-by-rank layout the handles run, inside the conditioning bound: the 1e-10
    the GPU tests ask for rests on inputs the reference handles as well.  The path the table records (the forward-elimination
    probe passes or not) and the window shape it records (ranks of unequal length, an interior rank) are checked here too."""
    c = TS_CASES[case]
    p, S, rho = c.make(), ts_host_segments(c), c.opts["rho"]
    assert S % c.world == 0
    adaptive = [(p, TS_ADAPT[case]["rho"] * 2.0 ** k) for k in range(TS_ADAPT_DOUBLINGS + 1)] if case in TS_ADAPT else []
    for prob, r in [(p, rho), (p, TS_RHO_FACTOR * rho)] + ([(ts_second_problem(p), rho)] if case in TS_UPDATE_CASES else []) + adaptive:
        W, WB, ok = ts_host_scan(prob, r, S, c.world)
        growth = np.abs(W).max(), np.abs(WB).max() if ok else 0.0
        assert max(growth) <= SCAN_GROWTH_MAX, (case, r, growth)
        assert ok == (c.alternating or bool(c.opts.get("flags", 0))), (case, r)       # (B: the probe passes, the flag declines)
    seg = host_factor(p, rho, S)["seg_start"]
    sl = S // c.world
    lens = [int(seg[(r + 1) * sl] - seg[r * sl]) for r in range(c.world)]
    assert sum(lens) == p.N and (len(set(lens)) > 1) == c.uneven, (case, lens)


def test_scan_refactor_problems_pass_the_probe_and_the_growth_bound(lib):
    """The rho and the second seed the refactor test moves a split handle to (tests/test_gpu_scan_geometry.py)."""
    n, m, N, S, seed, _ = SCAN_SLICEABLE[0]
    for sd in (seed, SCAN_REFACTOR_SEED):
        hf = host_factor(pkg.random_ltv(N=N, n=n, m=m, batch=67, seed=sd), SCAN_REFACTOR_RHO, S)
        assert hf["alt_ok"] and max(np.abs(hf["scanW"]).max(), np.abs(hf["scanWB"]).max()) <= SCAN_GROWTH_MAX, sd


def test_cert_chunk_restates_the_header():
    """cert_rec and cert_chunk of csrc/admm_cert_kernels.hpp, read from the source: stages of n (n + m) doubles, 4096 doubles of
    LDS, at most 64 stages, at least 1.  A change of either constant (or of the formula's shape) fails here until
    tests/_shapes.py follows, and with it the chunk-edge sweeps of the read-out kernels."""
    src = open(os.path.join(CSRC, "admm_cert_kernels.hpp")).read()
    assert re.search(r"constexpr int cert_rec\(int nx, int nu\) \{ return nx \* \(nx \+ nu\); \}", src)
    body = re.search(r"constexpr int cert_chunk\(int nx, int nu\) \{(.*?)\n\}", src, re.S).group(1)
    lds = re.search(r"int ch = (\d+) / cert_rec\(nx, nu\);", body)
    cap = re.search(r"return ch > (\d+) \? (\d+) : \(ch < 1 \? 1 : ch\);", body)
    assert lds and cap and cap.group(1) == cap.group(2)
    assert (int(lds.group(1)), int(cap.group(1))) == (CERT_LDS_DOUBLES, CERT_CHUNK_CAP) == (4096, 64)
    # the infeasibility kernels take the same chunk
    assert "CH = cert_chunk(NX, NU)" in open(os.path.join(CSRC, "admm_infeas_kernels.hpp")).read()
    assert [cert_chunk(n, m) for n, m in ((1, 1), (6, 3), (6, 4), (8, 4), (12, 6))] == [64, 64, 64, 42, 18]
    assert {cert_chunk(n, m) for n, m in SHARED} >= {64, 18} and min(cert_chunk(n, m) for n, m in SHARED) == 18


def test_chunk_edge_table_puts_every_pair_on_the_edges():
    """refill: chunks CH, CH, 1; fit: floor(s N / S) splits 2 CH + 1 stages into CH and CH + 1, pitch 320; stage: one stage each."""
    assert CHUNK_EDGE_CASES == ("refill", "fit", "stage")
    for n, m in SHARED:
        ch = cert_chunk(n, m)
        assert chunk_edge(n, m, "refill") == (2 * ch + 1, 1, 70) and chunk_edge(n, m, "stage") == (3, 3, 3)
        N, S, batch = chunk_edge(n, m, "fit")
        assert [s * N // S for s in range(S + 1)] == [0, ch, 2 * ch + 1] and (batch + 63) // 64 * 64 == 320
        assert N <= 129
