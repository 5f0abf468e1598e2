// admm_halfspace_kernels.hpp -- the z-update of a handle with one half-space per stage and its read-out.
// Stage k constrains xi_k, the first nh state rows of block k = (u_k, x_{k+1}):  a_k' xi_k <= b_k.  With v = w^ + y on those rows
// the z-update is the Euclidean projection, halfspace_acc / halfspace_step / halfspace_row of admm_prox.hpp:
//     nn = a'a,  d = a'v - b  (fma chains in row order),  t = d > 0 ? d / nn : 0,  z_i = fma(-t, a_i, v_i),  y_i = v_i - z_i
// nn == 0 (a_k = 0) is a stage without a half-space: its rows take their box.  That is all this file adds to the z-update: the
// walk over the blocks, the relaxation, v+ = w^ + y, the five residual sums and their order, and the ball / fuel projection of
// the control rows are z_walk_blocks' (admm_zdual.hpp), the same functions.  With every a = 0 each row goes through BoxProx:
// the bits of zdual_kernel / zdual_soc_kernel, residual partials included, given the same rows per chunk.
//
// zdual_halfspace_kernel<RESID, RELAX, SOC, PERQP>
//   A block with a plane is visited twice, as a thrust stage is for its norm: its nh state rows for d (the re-read hits
//   L1 / L2), then all rows to apply.  SOC: the control rows of the same block take soc_factor; without it ub / kap are not read.
//   PERQP = false: a[k][i], b[k] are shared by the batch: wave-uniform scalar loads through the constant address space, and
//       "the stage has a plane" is wave-uniform -- a block without one is not read twice.
//   PERQP = true: a[k][i][pitch], b[k][pitch] batch-minor, read as the state is, in 16-byte pairs of adjacent QPs; "has a
//       plane" is per lane (a select per row: plane or box).  Pad columns carry a = 0.  8 (nh + 1) more bytes per stage and QP.
//
// halfspace_report_kernel: one lane = one QP walks its stages (a wave reads 64 adjacent columns: coalesced).  Per QP
//     max_violation = max_k (a_k' w_xi - b_k)+ / sqrt(nn_k)    on w, the dynamics-feasible iterate of the last x-update
//     n_active      = number of stages with lam_k > 0
//     lam[k][b]     = rho (a_k' y_xi) / nn_k                   the multiplier of the stage's inequality (0 where nn_k = 0)
// One chain per QP and stage, no chunks, no atomics: bitwise repeatable.
//
// halfspace_scan_kernel: the device-side findings of admm_set_halfspace_device on per-QP planes -- per stage, whether any QP
// has a plane there and whether some a'a is not a normal number.  Plain stores of the same value from every finder.
#pragma once

#include "admm_kernels.hpp"
#include "admm_halfspace.hpp"

namespace admm {

// The half-space as a plane of z_walk_blocks.  a, b: [N][nh], [N] (PERQP = false) or [N][nh][pitch], [N][pitch] (true).
template <bool SOC, bool PERQP>
struct HalfspacePlane {
  static constexpr bool enabled = true, soc = SOC;
  const double* a;
  const double* b;
  int nh, m;
  struct Step {
    double2 t;                     // the step of either QP (0 where d <= 0 or the QP's stage has no plane)
    bool ax, ay;                   // the stage has a plane: PERQP = false: ax == ay, wave-uniform
    size_t ao;                     // element offset of a_k[0] (PERQP: of this lane's pair)
  };

  template <class Source>
  __device__ __forceinline__ Step step(const Source& src, int k, int rb, const ZChunk& c) const {
    constexpr int U = ADMM_Z_UNROLL;
    Step s{{0.0, 0.0}, false, false, 0};
    if constexpr (PERQP) {
      s.ao = (size_t)k * nh * c.P + c.col;
      double2 nn = {0.0, 0.0};
      for (int i = 0; i < nh; ++i) {
        const double2 ai = load2(a + s.ao + (size_t)i * c.P);
        nn.x = fma(ai.x, ai.x, nn.x);
        nn.y = fma(ai.y, ai.y, nn.y);
      }
      s.ax = nn.x != 0.0;
      s.ay = nn.y != 0.0;
      if (s.ax || s.ay) {
        const double2 bk = load2(b + (size_t)k * c.P + c.col);
        double2 d = {-bk.x, -bk.y};
        for (int i0 = 0; i0 < nh; i0 += U) {      // up to U rows in flight; the chain stays in row order
          typename Source::Row row[U];
          double2 ai[U];
#pragma unroll
          for (int j = 0; j < U; ++j)
            if (i0 + j < nh) {
              ai[j] = load2(a + s.ao + (size_t)(i0 + j) * c.P);
              row[j] = src.load((size_t)(rb + m + i0 + j) * c.P + c.col);
            }
#pragma unroll
          for (int j = 0; j < U; ++j)
            if (i0 + j < nh) {
              const double2 vi = src.v(row[j]);
              d.x = fma(ai[j].x, vi.x, d.x);
              d.y = fma(ai[j].y, vi.y, d.y);
            }
        }
        if (s.ax) s.t.x = halfspace_step(d.x, nn.x);
        if (s.ay) s.t.y = halfspace_step(d.y, nn.y);
      }
    } else {
      cdouble_p av = as_const(a);
      s.ao = (size_t)k * nh;
      double nn = 0.0;
      for (int i = 0; i < nh; ++i) nn = fma(av[s.ao + i], av[s.ao + i], nn);
      s.ax = s.ay = nn != 0.0;
      if (s.ax) {
        const double bk = as_const(b)[k];
        double2 d = {-bk, -bk};
        for (int i0 = 0; i0 < nh; i0 += U) {      // up to U rows in flight; the chain stays in row order
          typename Source::Row row[U];
#pragma unroll
          for (int j = 0; j < U; ++j)
            if (i0 + j < nh) row[j] = src.load((size_t)(rb + m + i0 + j) * c.P + c.col);
#pragma unroll
          for (int j = 0; j < U; ++j)
            if (i0 + j < nh) {
              const double ai = av[s.ao + i0 + j];
              const double2 vi = src.v(row[j]);
              d.x = fma(ai, vi.x, d.x);
              d.y = fma(ai, vi.y, d.y);
            }
        }
        s.t = make_double2(halfspace_step(d.x, nn), halfspace_step(d.y, nn));
      }
    }
    return s;
  }

  // wave-uniform: row r of the block is one of the nh rows, and (PERQP = false) the stage has a plane
  __device__ __forceinline__ bool covers(const Step& s, int r) const {
    const bool in = r >= m && r < m + nh;
    return PERQP ? in : in && s.ax;
  }

  __device__ __forceinline__ ZY2 row(const Step& s, double2 v, int r, const ZY2& box, size_t P) const {
    double2 z;
    if constexpr (PERQP) {
      const double2 ai = load2(a + s.ao + (size_t)(r - m) * P);
      z = make_double2(s.ax ? halfspace_row(s.t.x, ai.x, v.x) : box.z.x, s.ay ? halfspace_row(s.t.y, ai.y, v.y) : box.z.y);
    } else {
      const double ai = as_const(a)[s.ao + (r - m)];
      z = make_double2(halfspace_row(s.t.x, ai, v.x), halfspace_row(s.t.y, ai, v.y));
    }
    return ZY2{z, make_double2(v.x - z.x, v.y - z.y)};
  }
};

template <bool RESID, bool RELAX, bool SOC, bool PERQP>
__global__ __launch_bounds__(Z_THREADS) void zdual_halfspace_kernel(
    const double* __restrict__ w, double* __restrict__ z, double* __restrict__ y,
    const double* __restrict__ lo_, const double* __restrict__ hi_, const double* __restrict__ ub_, const double* __restrict__ kap_,
    const double* __restrict__ a_, const double* __restrict__ b_,
    double* __restrict__ part, double alpha, int L, int zrows, int pitch, int nb, int m, int nh) {
  z_walk_blocks(StateSource<RESID, RELAX>{w, z, y, alpha}, BoxProx{as_const(lo_), as_const(hi_)}, z, y, ub_, kap_, part, L, zrows,
                pitch, nb, m, HalfspacePlane<SOC, PERQP>{a_, b_, nh, m});
}

constexpr int HS_REPORT_THREADS = 64;

// sa: stride between a_k[i] and a_k[i + 1] (pitch per QP, 1 shared); per QP the arrays are offset by the QP's column
static __global__ __launch_bounds__(HS_REPORT_THREADS) void halfspace_report_kernel(
    const double* __restrict__ w, const double* __restrict__ y, const double* __restrict__ a_, const double* __restrict__ b_,
    double* __restrict__ max_violation, int* __restrict__ n_active, double* __restrict__ lam, double rho, int N, int nb, int m, int nh,
    int pitch, int batch, int perqp) {
  const int q = blockIdx.x * HS_REPORT_THREADS + threadIdx.x;
  if (q >= batch) return;
  const size_t P = (size_t)pitch, sa = perqp ? P : 1, col = perqp ? (size_t)q : 0;
  double mx = 0.0;
  int cnt = 0;
  for (int k = 0; k < N; ++k) {
    const double* ak = a_ + (size_t)k * nh * sa + col;
    const double bk = b_[(size_t)k * sa + col];
    const size_t o = ((size_t)k * nb + m) * P + q;
    double nn = 0.0, dw = -bk, dy = 0.0;
    for (int i = 0; i < nh; ++i) {
      const double ai = ak[(size_t)i * sa];
      nn = fma(ai, ai, nn);
      dw = fma(ai, w[o + (size_t)i * P], dw);
      dy = fma(ai, y[o + (size_t)i * P], dy);
    }
    double lk = 0.0;
    if (nn != 0.0) {
      mx = fmax(mx, fmax(dw, 0.0) / sqrt(nn));
      lk = rho * dy / nn;
      cnt += lk > 0.0 ? 1 : 0;
    }
    if (lam) lam[(size_t)k * P + q] = lk;
  }
  max_violation[q] = mx;
  n_active[q] = cnt;
}

constexpr int HS_SCAN_THREADS = 256;

// a: the caller's (batch, N, nh) array.  any[k] = 1: some QP has a plane at stage k; bad[k] = 1: some a'a there is not a normal
// number (halfspace_norm_ok: the projection divides by it).  Every finder stores the same 1: no atomics, no order.
static __global__ __launch_bounds__(HS_SCAN_THREADS) void halfspace_scan_kernel(const double* __restrict__ a, int batch, int N, int nh,
                                                                                int* __restrict__ any, int* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * HS_SCAN_THREADS + threadIdx.x;
  if (i >= (size_t)batch * N) return;
  const int k = (int)(i % N);
  const double* ak = a + i * nh;
  double nn = 0.0;
  bool nz = false;
  for (int j = 0; j < nh; ++j) {
    nn = fma(ak[j], ak[j], nn);
    nz = nz || ak[j] != 0.0;
  }
  if (nz) any[k] = 1;
  if (nz && !halfspace_norm_ok(nn)) bad[k] = 1;
}

}  // namespace admm
