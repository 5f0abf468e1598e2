"""Host check of the lean residual forms of the alternating kernels ("lean residual iterations";
csrc/admm_kernels_alt.hpp, LEAN): where every state row is unbounded, the dual-residual sum over the state rows,

    sum_k |x+_{k+1} - x_old,{k+1}|^2,

is rolled out from the difference of the control rows,  dx_{k+1} = A_k dx_k + B_k (u+_k - u_old,k)  in the forward kernel and
dx_k = AI_k dx_{k+1} + AIB_k (u+_k - u_old,k)  in the backward kernel, segment by segment, instead of being read back from the
stored state rows.  Here both ways are computed in NumPy on consecutive iterates of the alternating iteration (forward-rollout
form, backward-rollout form, ... exactly as xfze_kernel / xbze_kernel alternate), emulated from the host records, for the
configs[2] generator (N = 1000, n = 6, m = 3, 16 segments).

MEASURED (this file, 4 QPs, iterations 2..40 and 302..304, both directions): worst |s_lean - s_direct| = 1.04e-15 absolute
= 8.1e-15 relative to the largest s of the run (max s = 0.1296, at iteration 2).  Relative to s ITSELF the disagreement
reaches 1.5e-5 at iteration 304, where s has fallen to 5e-11: the error is absolute in nature (rounding of O(1) states over a
62-stage segment), as is that of the direct sum, whose terms are differences of rounded O(1) states too.
Ten times the measured figure -- 8.1e-14 relative to max(s) -- is the bound tests/test_gpu_lean_resid.py holds s to."""
import numpy as np
import pytest

import admm_library_amd as pkg
import oracle_c as oc
from admm_library_amd.solver import host_factor
from _segmented import unpack_alt, x_update_alt, x_update_segmented

RHO, SEGS = 0.05, 16
# the bound the issue sets for going ahead at all: disagreement relative to the largest s
GO_AHEAD = 1e-12
# measured worst disagreement relative to max(s) (docstring) -- asserted with the safety factor the GPU test uses
MEASURED_REL_TO_MAX = 8.1e-15


def _iterate(p, rec, a, z, y, forward):
    """One ADMM iteration in the given rollout direction.  Returns the new state, s computed directly, and what the lean form
    of the NEXT iteration needs: w_u and the state each segment's rollout ended with."""
    n, m, nb, N = p.n, p.m, p.nb, p.N
    seg = rec["seg_start"]
    S = len(seg) - 1
    g = -RHO * (z - y)
    if forward:
        w, parts = x_update_segmented(rec, n, m, g, p.x0, scan="gemm", return_parts=True)
        start = parts["xin"]                                   # x at the first stage of each segment (scan output)
    else:
        w = x_update_alt(rec, n, m, g, p.x0)
        start = None
    wb = w.reshape(p.batch, N, nb)
    if forward:                                                # the rolled-out x_{k1}: what block k1 - 1 stores
        bnd = np.stack([wb[:, seg[s + 1] - 1, m:] for s in range(S)])
    else:                                                      # the rolled-out x_{k0} (stored nowhere in w)
        start = np.stack([wb[:, seg[s + 1] - 1, m:] for s in range(S)])       # x_end(s): scan output = first block written
        bnd = np.stack([wb[:, seg[s], m:] @ a["AI"][seg[s]].T + wb[:, seg[s], :m] @ a["AIB"][seg[s]].T for s in range(S)])
    lo = np.tile(np.asarray(p.lo, np.float64), N)
    hi = np.tile(np.asarray(p.hi, np.float64), N)
    v = w + y
    zn = np.minimum(np.maximum(v, lo), hi)
    yn = v - zn
    return dict(w=w, z=zn, y=yn, start=start, bnd=bnd, forward=forward)


def _s_direct(p, new, z_old):
    return RHO * np.sqrt(np.sum((new["z"] - z_old) ** 2, axis=1))


def _s_lean(p, rec, a, new, old, z_old):
    n, m, nb, N = p.n, p.m, p.nb, p.N
    seg = rec["seg_start"]
    S = len(seg) - 1
    wn, wo = new["w"].reshape(p.batch, N, nb), old["w"].reshape(p.batch, N, nb)
    zn, zo = new["z"].reshape(p.batch, N, nb), z_old.reshape(p.batch, N, nb)
    acc = np.sum((zn[:, :, :m] - zo[:, :, :m]) ** 2, axis=(1, 2))          # control rows: as before
    assert new["forward"] != old["forward"]
    for s in range(S):
        dx = new["start"][s] - old["bnd"][s]
        if new["forward"]:
            for k in range(seg[s], seg[s + 1]):
                du = wn[:, k, :m] - wo[:, k, :m]
                dx = dx @ a["A"][k].T + du @ a["B"][k].T
                acc = acc + np.sum(dx * dx, axis=1)
        else:
            for k in range(seg[s + 1] - 1, seg[s] - 1, -1):
                acc = acc + np.sum(dx * dx, axis=1)
                du = wn[:, k, :m] - wo[:, k, :m]
                dx = dx @ a["AI"][k].T + du @ a["AIB"][k].T
    return RHO * np.sqrt(acc)


@pytest.fixture(scope="module")
def measured(lib):
    p = pkg.cw_rendezvous(N=1000, batch=4)
    rec = host_factor(p, RHO, SEGS)
    assert rec["alt_ok"]
    a = unpack_alt(rec, p.n, p.m)
    rows = []                       # (iteration, s_direct, s_lean)

    def chain(z, y, first_it, count):
        old = None
        for j in range(count):
            new = _iterate(p, rec, a, z, y, forward=(j % 2 == 0))
            if old is not None:
                rows.append((first_it + j, _s_direct(p, new, z), _s_lean(p, rec, a, new, old, z)))
            old, z, y = new, new["z"], new["y"]

    zero = np.zeros((p.batch, p.L))
    chain(zero, zero, 1, 40)
    late = oc.solve(p, rho=RHO, max_iter=300, stop=False)
    chain(late["z"], late["y"], 301, 4)
    return rows


def test_delta_rollout_reproduces_the_state_rows_dual_residual(measured):
    its = [r[0] for r in measured]
    assert its[:3] == [2, 3, 4] and 40 in its and its[-1] == 304            # both directions, early and late
    smax = max(r[1].max() for r in measured)
    worst_abs = max(np.abs(r[1] - r[2]).max() for r in measured)
    worst_rel_self = max((np.abs(r[1] - r[2]) / r[1]).max() for r in measured)
    print(f"lean vs direct s: worst abs {worst_abs:.3e}, rel to max(s) {worst_abs / smax:.3e}, rel to s {worst_rel_self:.3e}, "
          f"max(s) {smax:.3e}, s at the last iteration {measured[-1][1].max():.3e}")
    assert worst_abs / smax <= GO_AHEAD
    # the figures quoted in the docstring and in DESIGN.md §4.8, within the GPU test's safety factor
    assert worst_abs / smax <= 10 * MEASURED_REL_TO_MAX
