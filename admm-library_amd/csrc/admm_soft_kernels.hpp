// admm_soft_kernels.hpp -- the z-update of a handle with soft box constraints and the read-out of its penalty.
// Row i of the stacked vector carries a weight s_i >= 0 (+inf: the hard box) and the cost gains  s_i dist(w_i, [lo_i, hi_i]);
// with kap_i = s_i / rho the z-update of the row is soft_clip of admm_prox.hpp:
//     c = clip(v, lo, hi),  e = v - c,  z = |e| <= kap ? c : (e > 0 ? v - kap : v + kap),  y = v - z
// and everything else -- the relaxation, v+ = w^ + y, the five residual sums and their order -- is that of zdual_kernel /
// zdual_soc_kernel (admm_kernels.hpp), whose helpers are used as they are.  With every kap = +inf the select always takes c: the
// bits of those kernels, residual partials included, given the same rows per chunk.
//
// zdual_soft_kernel<RESID, RELAX, SOC>
//   SOC = false: zdual_kernel's geometry.  One lane = two adjacent QPs (16-byte accesses), four rows in flight, blockIdx.y = row
//       chunk; lo, hi and kap of a row are wave-uniform and read through the constant address space (scalar loads).  In place:
//       40 B per stacked element with RESID or RELAX, 32 B without; the kap array is L doubles for the whole batch.
//   SOC = true: zdual_soc_kernel's, a chunk being a whole number of blocks.  The control rows of a stage with a finite thrust
//       bound or a fuel weight take soc_factor (their weights are +inf: checked at set-up); every other row takes soft_clip.
// Pad columns (batch .. pitch - 1) are computed like any other, as in those kernels: their state is zero and stays finite.
//
// soft_report_kernel: one lane = one QP walks its column of z (a wave reads 64 adjacent columns: coalesced), four rows in flight.
// Over the rows with a finite weight, in row order:  penalty = fma(s_i, d_i, penalty),  d_i = max(lo_i - z_i, 0, z_i - hi_i);
// the largest d_i; the number of rows with d_i > 0.  One chain per QP, no chunks, no atomics: bitwise repeatable.
#pragma once

#include "admm_kernels.hpp"
#include "admm_soft.hpp"

namespace admm {

// One row of two adjacent QPs by the soft box
__device__ __forceinline__ ZY2 zy2_soft(double2 v, double lo, double hi, double kap) {
  const double2 z = make_double2(soft_clip(v.x, lo, hi, kap), soft_clip(v.y, lo, hi, kap));
  return ZY2{z, make_double2(v.x - z.x, v.y - z.y)};
}

// zdual_row with the soft box in place of the clip
template <bool RESID, bool RELAX>
__device__ __forceinline__ void zdual_soft_row(double2 wv, double2 zv, double2 yv, bool scaled, double2 c, double lo, double hi,
                                               double kap, double alpha, double* z, double* y, ResidSums (&acc)[2]) {
  const double2 v = v_plus2<RELAX>(alpha, wv, zv, yv);
  const ZY2 p = scaled ? zy2_scaled(v, c) : zy2_soft(v, lo, hi, kap);
  zy2_store(p, z, y);
  if (RESID) {
    acc[0].add(wv.x, p.z.x, zv.x, p.y.x);
    acc[1].add(wv.y, p.z.y, zv.y, p.y.y);
  }
}

template <bool RESID, bool RELAX, bool SOC>
__global__ __launch_bounds__(Z_THREADS) void zdual_soft_kernel(
    const double* __restrict__ w, double* __restrict__ z, double* __restrict__ y,
    const double* __restrict__ lo_, const double* __restrict__ hi_, const double* __restrict__ skap_,
    const double* __restrict__ ub_, const double* __restrict__ kap_,
    double* __restrict__ part, double alpha, int L, int zrows, int pitch, int nb, int m) {
  const int col = (blockIdx.x * Z_THREADS + threadIdx.x) * 2;
  if (col >= pitch) return;
  const int chunk = blockIdx.y;
  const int r_begin = chunk * zrows;
  const int r_end = (r_begin + zrows < L) ? r_begin + zrows : L;
  const size_t P = (size_t)pitch;
  cdouble_p lo = as_const(lo_);
  cdouble_p hi = as_const(hi_);
  cdouble_p sk = as_const(skap_);
  ResidSums acc[2];
  if constexpr (!SOC) {
    constexpr int U = 4;
    int r = r_begin;
    for (; r + U <= r_end; r += U) {
      double2 wv[U], yv[U], zv[U];
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const size_t o = (size_t)(r + i) * P + col;
        wv[i] = *reinterpret_cast<const double2*>(w + o);
        yv[i] = *reinterpret_cast<const double2*>(y + o);
        zv[i] = make_double2(0.0, 0.0);
        if (RESID || RELAX) zv[i] = *reinterpret_cast<const double2*>(z + o);
      }
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const size_t o = (size_t)(r + i) * P + col;
        zdual_soft_row<RESID, RELAX>(wv[i], zv[i], yv[i], false, wv[i], lo[r + i], hi[r + i], sk[r + i], alpha, z + o, y + o, acc);
      }
    }
    for (; r < r_end; ++r) {
      const size_t o = (size_t)r * P + col;
      const double2 wv = *reinterpret_cast<const double2*>(w + o);
      const double2 yv = *reinterpret_cast<const double2*>(y + o);
      double2 zv = {0, 0};
      if (RESID || RELAX) zv = *reinterpret_cast<const double2*>(z + o);
      zdual_soft_row<RESID, RELAX>(wv, zv, yv, false, wv, lo[r], hi[r], sk[r], alpha, z + o, y + o, acc);
    }
  } else {
    cdouble_p ubv = as_const(ub_);
    cdouble_p kapv = as_const(kap_);
    for (int rb = r_begin; rb < r_end; rb += nb) {
      const double ub = ubv[rb / nb], kap = kapv[rb / nb];
      const bool soc = ub < INFINITY || kap > 0.0;      // a finite thrust bound or a fuel weight (else the control rows use their soft box)
      double2 cs = {1.0, 1.0};
      if (soc) {
        double2 ss = {0.0, 0.0};
        for (int j = 0; j < m; ++j) {
          const size_t o = (size_t)(rb + j) * P + col;
          const double2 wv = *reinterpret_cast<const double2*>(w + o);
          const double2 yv = *reinterpret_cast<const double2*>(y + o);
          double2 zv = {0, 0};
          if (RELAX) zv = *reinterpret_cast<const double2*>(z + o);
          const double2 vn = v_plus2<RELAX>(alpha, wv, zv, yv);
          ss.x = fma(vn.x, vn.x, ss.x);
          ss.y = fma(vn.y, vn.y, ss.y);
        }
        cs = soc_scale2(ss, ub, kap);
      }
      for (int r = 0; r < nb; ++r) {
        const int row = rb + r;
        const size_t o = (size_t)row * P + col;
        const double2 wv = *reinterpret_cast<const double2*>(w + o);
        const double2 yv = *reinterpret_cast<const double2*>(y + o);
        double2 zv = {0, 0};
        if (RESID || RELAX) zv = *reinterpret_cast<const double2*>(z + o);
        zdual_soft_row<RESID, RELAX>(wv, zv, yv, soc && r < m, cs, lo[row], hi[row], sk[row], alpha, z + o, y + o, acc);
      }
    }
  }
  if (RESID) store_sums2(part + (size_t)chunk * 5 * P + col, P, acc);
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
