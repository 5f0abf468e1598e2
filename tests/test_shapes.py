"""The compiled shape lists (tests/_shapes.py) and the shape sweep's problem table, on the CPU: a pair added to or dropped from
the build changes a pinned list here until the sweeps are looked at, and a change of the forward-elimination probe that would
send a sweep cell to the plain kernels fails here before the GPU suite runs."""
import numpy as np
import pytest

import admm_library_amd as pkg
from admm_library_amd.solver import host_factor, host_scan_packed
from _shapes import (ALT_TABLE, MFMA, PER_INSTANCE, PLAIN_ONLY, SCAN_EMPTY_SLICE, SCAN_GEOMETRIES, SCAN_REFACTOR_RHO,
                     SCAN_REFACTOR_SEED, SCAN_SLICEABLE, SHARED, SWEEP_N, SWEEP_SEGMENTS, WIDE, gid, scan_shape)


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


def test_scan_refactor_problems_pass_the_probe_and_the_growth_bound(lib):
    """The rho and the second seed the refactor test moves a split handle to (tests/test_gpu_scan_geometry.py)."""
    n, m, N, S, seed, _ = SCAN_SLICEABLE[0]
    for sd in (seed, SCAN_REFACTOR_SEED):
        hf = host_factor(pkg.random_ltv(N=N, n=n, m=m, batch=67, seed=sd), SCAN_REFACTOR_RHO, S)
        assert hf["alt_ok"] and max(np.abs(hf["scanW"]).max(), np.abs(hf["scanWB"]).max()) <= SCAN_GROWTH_MAX, sd
