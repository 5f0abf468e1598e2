"""The row walk of the standalone z-update and read-out kernels (csrc/admm_zdual.hpp): the tail of a chunk and a short last chunk,
for every kernel that is built on z_walk_rows / z_walk_blocks at once.

(n, m) = (4, 2), N = 5: L = 30 rows; batch 70: a pitch of 128 with pad columns and idle lanes; alpha 1 and 1.6 (both RELAX forms);
residuals every iteration (the RESID forms).  zrows = 7 on the box and soft-box handles: every chunk is one group of four rows in
flight and a tail of three, the last chunk has two rows.  zrows = 12 on the thrust and soft + thrust handles: two blocks per chunk
and one in the last.  Each handle is compared with the same handle at zrows = L, one chunk: the iterates bit for bit, the
residuals -- chunk sums added in another order -- within the tolerance of tests/test_gpu_soft.py."""
import dataclasses

import numpy as np
import pytest

import admm_library_amd as pkg
import test_soft_host as host
from admm_library_amd import _abi
from test_gpu_soft import TOL, _close

pytestmark = pytest.mark.gpu
N, SHAPE, BATCH, ITERS = 5, (4, 2), 70, 6
ZROWS = {"box": 7, "soft": 7, "thrust": 12, "soft_thrust": 12}


def _problem(kind):
    p = pkg.random_ltv(N=N, n=SHAPE[0], m=SHAPE[1], batch=BATCH, seed=314, thrust_norm="thrust" in kind)
    return dataclasses.replace(p, soft=host.random_soft(p)) if "soft" in kind else p


def _decoupled(p):
    """p with the dynamics and cost of tests/_prox_cases.py (B = 0, R = 0, A a cyclic permutation, Q = QN = I, no linear term; rho
    a power of two): the x-update is exact in every kernel family, so a fused and an unfused handle hold the same iterates."""
    n, m = p.n, p.m
    return dataclasses.replace(p, A=np.roll(np.eye(n), 1, axis=1), B=np.zeros((n, m)), Q=np.eye(n), R=np.zeros((m, m)), QN=np.eye(n), q=None)


def _run(p, zrows, chunks, **kw):
    with pkg.Solver(p, pkg.Options(zrows=zrows, **kw)) as s:
        geo = s.geometry()
        assert (geo["pitch"], geo["zrows"], geo["zchunks"]) == (128, zrows, chunks), geo
        s.run(ITERS, residual_every=1)
        return s.get(), tuple(s.residuals())


@pytest.mark.parametrize("alpha", [1.0, 1.6])
@pytest.mark.parametrize("kind", list(ZROWS))
def test_chunks_with_a_tail_give_the_bits_of_one_chunk(gpu, kind, alpha):
    p = _problem(kind)
    assert p.L == 30
    kw = dict(rho=0.3, alpha=alpha, flags=0 if "soft" in kind else _abi.FLAG_UNFUSED)
    zr = ZROWS[kind]
    state, res = _run(p, zr, -(-p.L // zr), **kw)
    state1, res1 = _run(p, p.L, 1, **kw)
    for name, a, b in zip("wzy", state, state1):
        assert np.isfinite(a).all() and np.array_equal(a, b), (name, np.abs(a - b).max())
    assert np.abs(state[1]).max() > 0.05 and np.abs(state[2]).max() > 1e-3          # bounds are active: y is not zero
    for name, a, b in zip(("r", "s", "nw", "nz", "ny"), res, res1):
        assert _close(a, b, TOL), (name, np.abs(a - b).max())


@pytest.mark.parametrize("alpha", [1.0, 1.6])
@pytest.mark.parametrize("kind", ["box", "thrust"])
def test_read_out_of_a_fused_handle_gives_the_unfused_state(gpu, kind, alpha):
    """get() of a fused handle rebuilds (z, y) from v with v_to_zy_kernel / v_to_zy_soc_kernel, over the same chunks as the unfused
    handle's z-update.  From a random state (the decoupled problem would stay at zero on its control rows), after every iteration."""
    p = _decoupled(_problem(kind))
    zr = ZROWS[kind]
    rng = np.random.default_rng(27)
    z0, y0 = 0.5 * rng.standard_normal((BATCH, p.L)), 0.2 * rng.standard_normal((BATCH, p.L))
    kw = dict(rho=0.25, alpha=alpha, zrows=zr)
    with pkg.Solver(p, pkg.Options(flags=_abi.FLAG_NO_MFMA, **kw)) as fused, pkg.Solver(p, pkg.Options(flags=_abi.FLAG_UNFUSED, **kw)) as unfused:
        assert fused.geometry() == unfused.geometry() and fused.geometry()["zchunks"] == -(-p.L // zr)
        clipped = 0
        for h in (fused, unfused):
            h.set_state(z=z0, y=y0)
        for it in range(ITERS):
            for h in (fused, unfused):
                h.run(1, residual_every=1)
            (_, z, y), (_, zu, yu) = fused.get(), unfused.get()
            assert np.isfinite(z).all() and np.array_equal(z, zu) and np.array_equal(y, yu), (it, np.abs(z - zu).max(), np.abs(y - yu).max())
            clipped += int((np.abs(y) > 1e-3).sum())
        assert clipped > BATCH
