// admm_soft_kernels.hpp -- the z-update of a handle with soft box constraints and the read-out of its penalty.
// Row i of the stacked vector carries a weight s_i >= 0 (+inf: the hard box) and the cost gains  s_i dist(w_i, [lo_i, hi_i]);
// with kap_i = s_i / rho the z-update of the row is soft_clip of admm_prox.hpp:
//     c = clip(v, lo, hi),  e = v - c,  z = |e| <= kap ? c : (e > 0 ? v - kap : v + kap),  y = v - z
// That prox (SoftBoxProx) is all this file adds to the z-update: the walk over the rows, the relaxation, v+ = w^ + y, the five
// residual sums and their order are those of zdual_kernel / zdual_soc_kernel (admm_zdual.hpp), the same functions.  With every
// kap = +inf the select always takes c: the bits of those kernels, residual partials included, given the same rows per chunk.
//
// zdual_soft_kernel<RESID, RELAX, SOC>
//   SOC = false: z_walk_rows, as zdual_kernel.  In place: 40 B per stacked element with RESID or RELAX, 32 B without; the kap
//       array is L doubles for the whole batch.
//   SOC = true: z_walk_blocks, as zdual_soc_kernel.  The control rows of a stage with a finite thrust bound or a fuel weight
//       take soc_factor (their weights are +inf: checked at set-up); every other row takes soft_clip.
//
// soft_report_kernel: one lane = one QP walks its column of z (a wave reads 64 adjacent columns: coalesced), four rows in flight.
// Over the rows with a finite weight, in row order:  penalty = fma(s_i, d_i, penalty),  d_i = max(lo_i - z_i, 0, z_i - hi_i);
// the largest d_i; the number of rows with d_i > 0.  One chain per QP, no chunks, no atomics: bitwise repeatable.
#pragma once

#include "admm_kernels.hpp"
#include "admm_soft.hpp"

namespace admm {

// The soft box as a prox of the z walks: lo, hi and kap of a row are wave-uniform (scalar loads)
struct SoftBoxProx {
  cdouble_p lo, hi, kap;
  __device__ __forceinline__ ZY2 operator()(double2 v, int r) const {
    const double l = lo[r], h = hi[r], k = kap[r];
    const double2 z = make_double2(soft_clip(v.x, l, h, k), soft_clip(v.y, l, h, k));
    return ZY2{z, make_double2(v.x - z.x, v.y - z.y)};
  }
};

template <bool RESID, bool RELAX, bool SOC>
__global__ __launch_bounds__(Z_THREADS) void zdual_soft_kernel(
    const double* __restrict__ w, double* __restrict__ z, double* __restrict__ y,
    const double* __restrict__ lo_, const double* __restrict__ hi_, const double* __restrict__ skap_,
    const double* __restrict__ ub_, const double* __restrict__ kap_,
    double* __restrict__ part, double alpha, int L, int zrows, int pitch, int nb, int m) {
  const StateSource<RESID, RELAX> src{w, z, y, alpha};
  const SoftBoxProx prox{as_const(lo_), as_const(hi_), as_const(skap_)};
  if constexpr (SOC) z_walk_blocks(src, prox, z, y, ub_, kap_, part, L, zrows, pitch, nb, m);
  else z_walk_rows(src, prox, z, y, part, L, zrows, pitch);
}

constexpr int SOFT_REPORT_THREADS = 64;

// d = dist(z, [lo, hi]) of a row with a finite weight s, added to the three results of a QP
__device__ __forceinline__ void soft_report_row(double zv, double lo, double hi, double s, double& pen, double& mx, int& cnt) {
  if (!(s < INFINITY)) return;                      // (wave-uniform) a hard row: not part of the penalty
  const double d = fmax(fmax(lo - zv, 0.0), zv - hi);
  pen = fma(s, d, pen);
  mx = fmax(mx, d);
  cnt += d > 0.0 ? 1 : 0;
}

static __global__ __launch_bounds__(SOFT_REPORT_THREADS) void soft_report_kernel(
    const double* __restrict__ z, const double* __restrict__ lo_, const double* __restrict__ hi_, const double* __restrict__ soft_,
    double* __restrict__ penalty, double* __restrict__ max_violation, int* __restrict__ n_violated, int L, int pitch, int batch) {
  const int b = blockIdx.x * SOFT_REPORT_THREADS + threadIdx.x;
  if (b >= batch) return;
  cdouble_p lo = as_const(lo_);
  cdouble_p hi = as_const(hi_);
  cdouble_p sv = as_const(soft_);
  const size_t P = (size_t)pitch;
  double pen = 0.0, mx = 0.0;
  int cnt = 0;
  constexpr int U = 4;
  int r = 0;
  for (; r + U <= L; r += U) {
    double zv[U];
#pragma unroll
    for (int i = 0; i < U; ++i) zv[i] = z[(size_t)(r + i) * P + b];
#pragma unroll
    for (int i = 0; i < U; ++i) soft_report_row(zv[i], lo[r + i], hi[r + i], sv[r + i], pen, mx, cnt);
  }
  for (; r < L; ++r) soft_report_row(z[(size_t)r * P + b], lo[r], hi[r], sv[r], pen, mx, cnt);
  penalty[b] = pen;
  max_violation[b] = mx;
  n_violated[b] = cnt;
}

}  // namespace admm
