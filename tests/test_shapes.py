"""The compiled shape lists (tests/_shapes.py) and the shape sweep's problem table, on the CPU: a pair added to or dropped from
the build changes a pinned list here until the sweeps are looked at, and a change of the forward-elimination probe that would
send a sweep cell to the plain kernels fails here before the GPU suite runs."""
import pytest

import admm_library_amd as pkg
from admm_library_amd.solver import host_factor
from _shapes import ALT_TABLE, MFMA, PER_INSTANCE, PLAIN_ONLY, SHARED, SWEEP_N, SWEEP_SEGMENTS, WIDE


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
