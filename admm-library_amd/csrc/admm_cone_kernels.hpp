// admm_cone_kernels.hpp -- the z-update of a handle with one approach cone per stage and its read-out.
// Stage k constrains xi_k, the first nh state rows of block k = (u_k, x_{k+1}), to the second-order cone of axis c_k, apex p_k and
// slope g_k:  r <= g s  with  e = c / |c|,  s = e'(xi - p),  r = |(xi - p) - s e|.  With v = w^ + y on those rows the z-update is
// the Euclidean projection, cone_norm / cone_acc / cone_step / cone_row of admm_prox.hpp: three fma chains over the rows, then per
// row a select between v (inside), p_i (the polar cone: the apex) and fma(kap, c_i, fma(bet, v_i - p_i, p_i)) (the surface).
// nn == 0 (c_k = 0) is a stage without a cone: its rows take their box.  That is all this file adds to the z-update: the walk over
// the blocks, the relaxation, v+ = w^ + y, the five residual sums and their order, and the ball / fuel projection of the control
// rows are z_walk_blocks' (admm_zdual.hpp), the same functions, and the cone is a plane policy of that walk as HalfspacePlane
// is.  With every c = 0 each row goes through BoxProx: the bits of zdual_kernel / zdual_soc_kernel, residual partials included,
// given the same rows per chunk.
//
// zdual_cone_kernel<RESID, RELAX, SOC, PERQP>
//   A block with a cone is visited twice, as a thrust stage is for its norm: its nh state rows for the chains d and q (the
//   re-read hits L1 / L2), then all rows to apply.  SOC: the control rows of the same block take soc_factor; without it ub / kap
//   are not read.
//   PERQP = false: c[k][i], p[k][i], g[k] are shared by the batch: wave-uniform scalar loads through the constant address space,
//       and "the stage has a cone" is wave-uniform -- a block without one is not read twice.
//   PERQP = true: c[k][i][pitch], p[k][i][pitch], g[k][pitch] batch-minor, read as the state is, in 16-byte pairs of adjacent
//       QPs; "has a cone" is per lane (a select per row: cone or box).  Pad columns carry c = 0.  8 (2 nh + 1) more bytes per stage
//       and QP.
//
// cone_report_kernel: one lane = one QP walks its stages (a wave reads 64 adjacent columns: coalesced).  Per QP
//     max_violation = max_k (r_k - g_k s_k)+ / sqrt(1 + g_k^2)   on w, the dynamics-feasible iterate of the last x-update: the
//                                                                 distance of w_xi from the cone where it is outside
//     n_active      = number of stages with a cone whose y_xi has a nonzero entry
//     lam[k][b]     = rho |y_xi|_2                                the size of the stage's multiplier (0 where nn_k = 0)
// One chain per QP and stage, no chunks, no atomics: bitwise repeatable.
//
// cone_scan_kernel: the device-side findings of admm_set_cone_device on per-QP cones -- per stage, whether any QP has a cone
// there, whether some c'c is not a normal number and whether some slope of a stage with a cone is unusable.  Plain stores of the
// same value from every finder.
#pragma once

#include "admm_kernels.hpp"
#include "admm_halfspace.hpp"
#include "admm_cone.hpp"

namespace admm {

// The cone as a plane of z_walk_blocks.  c, p, g: [N][nh], [N][nh], [N] (PERQP = false) or [N][nh][pitch] twice, [N][pitch] (true).
template <bool SOC, bool PERQP>
struct ConePlane {
  static constexpr bool enabled = true, soc = SOC;
  const double* c;
  const double* p;
  const double* g;
  int nh, m;
  struct Step {
    ConeStep x, y;                 // kap, bet and the branch of either QP (unused where the QP's stage has no cone)
    bool ax, ay;                   // the stage has a cone: PERQP = false: ax == ay, wave-uniform
    size_t co;                     // element offset of c_k[0] and p_k[0] (PERQP: of this lane's pair)
  };

  template <class Source>
  __device__ __forceinline__ Step step(const Source& src, int k, int rb, const ZChunk& ch) const {
    constexpr int U = ADMM_Z_UNROLL;
    Step s{{0.0, 0.0, CONE_INSIDE}, {0.0, 0.0, CONE_INSIDE}, false, false, 0};
    if constexpr (PERQP) {
      s.co = (size_t)k * nh * ch.P + ch.col;
      double2 nn = {0.0, 0.0};
      for (int i = 0; i < nh; ++i) {
        const double2 ci = load2(c + s.co + (size_t)i * ch.P);
        nn.x = cone_norm(ci.x, nn.x);
        nn.y = cone_norm(ci.y, nn.y);
      }
      s.ax = nn.x != 0.0;
      s.ay = nn.y != 0.0;
      if (s.ax || s.ay) {
        const double2 gk = load2(g + (size_t)k * ch.P + ch.col);
        double2 d = {0.0, 0.0}, q = {0.0, 0.0};
        for (int i0 = 0; i0 < nh; i0 += U) {      // up to U rows in flight; the chains stay in row order
          typename Source::Row row[U];
          double2 ci[U], pi[U];
#pragma unroll
          for (int j = 0; j < U; ++j)
            if (i0 + j < nh) {
              ci[j] = load2(c + s.co + (size_t)(i0 + j) * ch.P);
              pi[j] = load2(p + s.co + (size_t)(i0 + j) * ch.P);
              row[j] = src.load((size_t)(rb + m + i0 + j) * ch.P + ch.col);
            }
#pragma unroll
          for (int j = 0; j < U; ++j)
            if (i0 + j < nh) {
              const double2 vi = src.v(row[j]);
              cone_acc(ci[j].x, pi[j].x, vi.x, d.x, q.x);
              cone_acc(ci[j].y, pi[j].y, vi.y, d.y, q.y);
            }
        }
        // (a lane whose stage has no cone: nn = 1 keeps its unused quotients finite)
        s.x = cone_step(s.ax ? nn.x : 1.0, d.x, q.x, gk.x);
        s.y = cone_step(s.ay ? nn.y : 1.0, d.y, q.y, gk.y);
      }
    } else {
      cdouble_p cv = as_const(c);
      cdouble_p pv = as_const(p);
      s.co = (size_t)k * nh;
      double nn = 0.0;
      for (int i = 0; i < nh; ++i) nn = cone_norm(cv[s.co + i], nn);
      s.ax = s.ay = nn != 0.0;
      if (s.ax) {
        const double gk = as_const(g)[k];
        double2 d = {0.0, 0.0}, q = {0.0, 0.0};
        for (int i0 = 0; i0 < nh; i0 += U) {      // up to U rows in flight; the chains stay in row order
          typename Source::Row row[U];
#pragma unroll
          for (int j = 0; j < U; ++j)
            if (i0 + j < nh) row[j] = src.load((size_t)(rb + m + i0 + j) * ch.P + ch.col);
#pragma unroll
          for (int j = 0; j < U; ++j)
            if (i0 + j < nh) {
              const double ci = cv[s.co + i0 + j], pi = pv[s.co + i0 + j];
              const double2 vi = src.v(row[j]);
              cone_acc(ci, pi, vi.x, d.x, q.x);
              cone_acc(ci, pi, vi.y, d.y, q.y);
            }
        }
        s.x = cone_step(nn, d.x, q.x, gk);
        s.y = cone_step(nn, d.y, q.y, gk);
      }
    }
    return s;
  }

  // wave-uniform: row r of the block is one of the nh rows, and (PERQP = false) the stage has a cone
  __device__ __forceinline__ bool covers(const Step& s, int r) const {
    const bool in = r >= m && r < m + nh;
    return PERQP ? in : in && s.ax;
  }

  __device__ __forceinline__ ZY2 row(const Step& s, double2 v, int r, const ZY2& box, size_t P) const {
    double2 z;
    if constexpr (PERQP) {
      const double2 ci = load2(c + s.co + (size_t)(r - m) * P);
      const double2 pi = load2(p + s.co + (size_t)(r - m) * P);
      z = make_double2(s.ax ? cone_row(s.x, ci.x, pi.x, v.x) : box.z.x, s.ay ? cone_row(s.y, ci.y, pi.y, v.y) : box.z.y);
    } else {
      const double ci = as_const(c)[s.co + (r - m)], pi = as_const(p)[s.co + (r - m)];
      z = make_double2(cone_row(s.x, ci, pi, v.x), cone_row(s.y, ci, pi, v.y));
    }
    return ZY2{z, make_double2(v.x - z.x, v.y - z.y)};
  }
};

template <bool RESID, bool RELAX, bool SOC, bool PERQP>
__global__ __launch_bounds__(Z_THREADS) void zdual_cone_kernel(
    const double* __restrict__ w, double* __restrict__ z, double* __restrict__ y,
    const double* __restrict__ lo_, const double* __restrict__ hi_, const double* __restrict__ ub_, const double* __restrict__ kap_,
    const double* __restrict__ c_, const double* __restrict__ p_, const double* __restrict__ g_,
    double* __restrict__ part, double alpha, int L, int zrows, int pitch, int nb, int m, int nh) {
  z_walk_blocks(StateSource<RESID, RELAX>{w, z, y, alpha}, BoxProx{as_const(lo_), as_const(hi_)}, z, y, ub_, kap_, part, L, zrows,
                pitch, nb, m, ConePlane<SOC, PERQP>{c_, p_, g_, nh, m});
}

constexpr int CONE_REPORT_THREADS = 64;

// sa: stride between c_k[i] and c_k[i + 1] (pitch per QP, 1 shared); per QP the arrays are offset by the QP's column
static __global__ __launch_bounds__(CONE_REPORT_THREADS) void cone_report_kernel(
    const double* __restrict__ w, const double* __restrict__ y, const double* __restrict__ c_, const double* __restrict__ p_,
    const double* __restrict__ g_, double* __restrict__ max_violation, int* __restrict__ n_active, double* __restrict__ lam, double rho,
    int N, int nb, int m, int nh, int pitch, int batch, int perqp) {
  const int qp = blockIdx.x * CONE_REPORT_THREADS + threadIdx.x;
  if (qp >= batch) return;
  const size_t P = (size_t)pitch, sa = perqp ? P : 1, col = perqp ? (size_t)qp : 0;
  double mx = 0.0;
  int cnt = 0;
  for (int k = 0; k < N; ++k) {
    const double* ck = c_ + (size_t)k * nh * sa + col;
    const double* pk = p_ + (size_t)k * nh * sa + col;
    const size_t o = ((size_t)k * nb + m) * P + qp;
    double nn = 0.0, d = 0.0, q = 0.0, yy = 0.0;
    bool moved = false;
    for (int i = 0; i < nh; ++i) {
      const double ci = ck[(size_t)i * sa], yi = y[o + (size_t)i * P];
      nn = cone_norm(ci, nn);
      cone_acc(ci, pk[(size_t)i * sa], w[o + (size_t)i * P], d, q);
      yy = fma(yi, yi, yy);
      moved = moved || yi != 0.0;
    }
    double lk = 0.0;
    if (nn != 0.0) {
      const double gk = g_[(size_t)k * sa + col];
      const double s = d / sqrt(nn);
      const double r = sqrt(fmax(fma(-s, s, q), 0.0));
      mx = fmax(mx, fmax(fma(-gk, s, r), 0.0) / sqrt(fma(gk, gk, 1.0)));
      lk = rho * sqrt(yy);
      cnt += moved ? 1 : 0;
    }
    if (lam) lam[(size_t)k * P + qp] = lk;
  }
  max_violation[qp] = mx;
  n_active[qp] = cnt;
}

constexpr int CONE_SCAN_THREADS = 256;

// c, g: the caller's (batch, N, nh) and (batch, N) arrays.  any[k] = 1: some QP has a cone at stage k; badn[k] = 1: some c'c there
// is not a normal number (halfspace_norm_ok: the projection divides by its root); badg[k] = 1: the slope of some QP's cone there is
// unusable (cone_slope_ok).  Every finder stores the same 1: no atomics, no order.
static __global__ __launch_bounds__(CONE_SCAN_THREADS) void cone_scan_kernel(const double* __restrict__ c, const double* __restrict__ g,
                                                                            int batch, int N, int nh, int* __restrict__ any,
                                                                            int* __restrict__ badn, int* __restrict__ badg) {
  const size_t i = (size_t)blockIdx.x * CONE_SCAN_THREADS + threadIdx.x;
  if (i >= (size_t)batch * N) return;
  const int k = (int)(i % N);
  const double* ck = c + i * nh;
  double nn = 0.0;
  bool nz = false;
  for (int j = 0; j < nh; ++j) {
    nn = cone_norm(ck[j], nn);
    nz = nz || ck[j] != 0.0;
  }
  if (!nz) return;
  any[k] = 1;
  if (!halfspace_norm_ok(nn)) badn[k] = 1;
  if (!cone_slope_ok(g[i])) badg[k] = 1;
}

}  // namespace admm
