"""Host packing of the segment scan (pack_scan in csrc/admm_factor.cpp), on the CPU: what xscan_mfma_kernel
reads -- the scan matrix in MFMA fragment order and the k-step range of every row group -- against the dense matrices of
admm_host_scan_matrix / admm_host_factor_alt, at every geometry of tests/_shapes.py SCAN_GEOMETRIES and for both scan
matrices (W, and WB of the forward-elimination form).  The kernel's split-K slice rule is restated here and must tile every
group's range exactly -- empty slices included --, and the product emulated slice by slice from the packed operand, summed
in split order as the consumers do, must be W @ in.  A range one batch short, a tile packed out of place or a slice counted
twice fails here before a GPU is involved."""
import ctypes as C

import numpy as np
import pytest

import admm_library_amd as pkg
from admm_library_amd import _abi
from admm_library_amd.solver import host_factor, host_scan_packed
from _shapes import SCAN_EMPTY_SLICE, SCAN_GEOMETRIES, SCAN_SLICEABLE, gid, scan_shape

SCAN_U, SCAN_MT = 8, 4        # k-steps per batch, 16-row tiles per row group (csrc/admm_factor.hpp)
SPLITS = (1, 2, 4, 8)
TOL = 1e-13


@pytest.fixture(scope="module")
def packs(lib):
    """(dense W, packed Wp, ranges, M, K) of both scan matrices per geometry, computed once."""
    out = {}
    for geom in SCAN_GEOMETRIES:
        n, m, N, S, seed, rho = geom
        p = pkg.random_ltv(N=N, n=n, m=m, batch=3, seed=seed)
        hf = host_factor(p, rho, S)
        assert hf["alt_ok"], geom
        out[geom] = {"W": (hf["scanW"],) + host_scan_packed(p, rho, S), "WB": (hf["scanWB"],) + host_scan_packed(p, rho, S, True)}
    return out


def _slices(kb, ke, nsplit):
    """xscan_mfma_kernel's slice rule: the k-steps [b, e) of slice z = blockIdx.z (b >= e: the slice stores zeros)."""
    if nsplit == 1:
        return [(kb, ke)]
    per = (((ke - kb) // SCAN_U + nsplit - 1) // nsplit) * SCAN_U
    return [(kb + z * per, min(kb + z * per + per, ke)) for z in range(nsplit)]


def _unpack(Wp, M, K):
    """Walk Wp in the kernel's order: k-step-major, M / 16 tiles of 64 doubles per k-step, A[i = lane & 15][k = lane >> 4]."""
    mtiles, ksteps = M // 16, K // 4
    assert Wp.size == ksteps * mtiles * 64
    W = np.full((M, K), np.nan)
    lane = np.arange(64)
    t = Wp.reshape(ksteps, mtiles, 64)
    for ks in range(ksteps):
        for mt in range(mtiles):
            W[16 * mt + (lane & 15), 4 * ks + (lane >> 4)] = t[ks, mt]
    return W


def _emulate(Wp, rng, M, K, vin, nsplit):
    """out = sum over the slices, in split order, of each slice's partial product: per row group, the MFMA steps of the slice's
    k-steps on the fragments of Wp (tile t of group g at k-step ks: Wp[(ks * mtiles + g * SCAN_MT + t) * 64 + lane])."""
    mtiles = M // 16
    t = Wp.reshape(K // 4, mtiles, 4, 16)                   # [k-step][tile][k = lane >> 4][i = lane & 15]
    slabs = np.zeros((nsplit, M) + vin.shape[1:])
    for g, (kb, ke) in enumerate(rng):
        for z, (b, e) in enumerate(_slices(int(kb), int(ke), nsplit)):
            for ks in range(b, e):
                a = t[ks, g * SCAN_MT:(g + 1) * SCAN_MT]                                 # (tile, k, i)
                slabs[z, g * 64:(g + 1) * 64] += np.einsum("tki,kc->tic", a, vin[4 * ks:4 * ks + 4]).reshape(64, -1)
    out = slabs[0].copy()
    for z in range(1, nsplit):
        out += slabs[z]
    return out


@pytest.mark.parametrize("which", ["W", "WB"])
@pytest.mark.parametrize("geom", SCAN_GEOMETRIES, ids=gid)
def test_packed_operand_and_ranges_are_the_dense_matrix(packs, geom, which):
    n, m, N, S, seed, rho = geom
    W, Wp, rng, M, K = packs[geom][which]
    Se, Me, Ke, groups = scan_shape(n, N, S)
    assert (M, K, len(rng)) == (Me, Ke, groups) and W.shape == (M, K)
    np.testing.assert_array_equal(_unpack(Wp, M, K), W)
    # padding: rows past S n in either half and columns past (2 S + 1) n are exactly zero
    Mt, Sn = M // 2, Se * n
    assert not W[Sn:Mt].any() and not W[Mt + Sn:].any() and not W[:, 2 * Sn + n:].any()
    for g, (kb, ke) in enumerate(rng):
        assert kb % SCAN_U == 0 and ke % SCAN_U == 0 and 0 <= kb <= ke <= K // 4, (g, kb, ke)
        rows = W[g * 64:(g + 1) * 64]
        assert not rows[:, :4 * kb].any() and not rows[:, 4 * ke:].any(), (g, kb, ke)
        if ke > kb:      # no wider than the batch alignment asks: the first and the last batch hold a non-zero
            assert rows[:, 4 * kb:4 * (kb + SCAN_U)].any() and rows[:, 4 * (ke - SCAN_U):4 * ke].any(), (g, kb, ke)
        else:
            assert (kb, ke) == (0, 0) and not rows.any()


@pytest.mark.parametrize("which", ["W", "WB"])
@pytest.mark.parametrize("geom", SCAN_GEOMETRIES, ids=gid)
def test_slices_tile_every_range_and_their_sum_is_the_product(packs, geom, which):
    W, Wp, rng, M, K = packs[geom][which]
    vin = np.random.default_rng(geom[4]).standard_normal((K, 3))
    ref = W @ vin
    empty = {ns: 0 for ns in SPLITS}
    for nsplit in SPLITS:
        for kb, ke in rng:
            sl = _slices(int(kb), int(ke), nsplit)
            assert len(sl) == nsplit
            steps = [ks for b, e in sl for ks in range(b, e)]
            assert steps == list(range(kb, ke)), (nsplit, kb, ke, sl)           # no k-step twice, none missed, in order
            assert all(b % SCAN_U == 0 and (e <= b or e % SCAN_U == 0) for b, e in sl)
            empty[nsplit] += sum(e <= b for b, e in sl)
        out = _emulate(Wp, rng, M, K, vin, nsplit)
        err = np.abs(out - ref).max()
        assert err <= TOL * max(1.0, np.abs(ref).max()), (nsplit, err)
    assert empty[1] == sum(ke == kb for kb, ke in rng)
    widest = int((rng[:, 1] - rng[:, 0]).max()) // SCAN_U
    if which == "W" and geom in SCAN_EMPTY_SLICE:          # fewer batches than slices: every group leaves slices of 4 and 8 empty
        assert widest < 4 and empty[4] >= len(rng) and empty[8] >= 5 * len(rng)
    if which == "W" and geom in SCAN_SLICEABLE:
        # the widest group has >= 8 batches: ceil(b / ceil(b / 8)) >= 5 of the 8 slices have work (b = 9: 2 batches each in 5
        # slices, 3 empty), and at least 3 of 4 and both of 2
        kb, ke = rng[np.argmax(rng[:, 1] - rng[:, 0])]
        assert widest >= 8
        for nsplit, least in ((2, 2), (4, 3), (8, 5)):
            assert sum(e > b for b, e in _slices(int(kb), int(ke), nsplit)) >= least, (nsplit, kb, ke)


def test_scan_packed_entry_point_contract(lib):
    """Size query with NULL arrays, the backward flag, NULL outputs and a NULL problem."""
    p = pkg.random_ltv(N=10, n=6, m=3, batch=2, seed=2099)
    cp, keep = _abi.marshal_problem(p)
    sizes = np.full(4, -1, np.int32)
    assert lib.admm_host_scan_packed(C.byref(cp), 0.3, 3, 0, None, None, _abi.iptr(sizes)) == 0
    assert sizes.tolist() == [128, 64, 2, 1]
    assert lib.admm_host_scan_packed(C.byref(cp), 0.3, 3, 1, None, None, _abi.iptr(sizes)) == 0 and sizes[3] == 1
    rng = np.full(4, -1, np.int32)
    assert lib.admm_host_scan_packed(C.byref(cp), 0.3, 3, 0, None, _abi.iptr(rng), None) == 0
    assert rng.tolist() == host_scan_packed(p, 0.3, 3)[1].ravel().tolist()
    invalid = {v: k for k, v in _abi.STATUS_NAMES.items()}["ADMM_ERR_INVALID"]
    assert lib.admm_host_scan_packed(None, 0.3, 3, 0, None, None, _abi.iptr(sizes)) == invalid
    assert lib.admm_get_scan_geometry(None, None, None, None, None) == invalid
    del keep
