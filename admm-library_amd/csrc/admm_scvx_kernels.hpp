// admm_scvx_kernels.hpp -- the outer step of the batched successive-convexification loop on the device: the
// device counterparts of scvx.rollout, scvx.linearise, scvx.correction_qp_batch and the decision block of scvx.scvx_batch, for the
// model M the kernels are instantiated for (n = 6, m = 3; the shipped one, scvx.relative_motion_rhs, in admm_scvx.hip; DESIGN.md
// §2.8.2: the CR3BP in admm_scvx_models.hip; §2.8.3: the models that read per-node data in admm_scvx_stage.hip).  fp64, explicit
// fma(), no inline assembly.
//
// Every caller-visible array is QP-major C order (the shapes of Problem / DeviceProblem): u (B, N, 3), x (B, N, 6) = x_1 .. x_N,
// A (B, N, 6, 6) and B (B, N, 6, 3) as row-major blocks, lo | hi | q | z (B, N, 9) in block order (u_k, x_{k+1}).
//
//   scvx_rollout_kernel    one lane per trajectory, sequential in k; a wave's 64 rows of u are N * 24 bytes apart, so a chunk of
//                          stages goes through LDS: loaded as contiguous per-trajectory runs, read back lane-wise; x the same way
//                          in reverse.  INIT form: also the cost and the start values of the loop's state (admm_scvx_init_device)
//   scvx_linearise_kernel  one lane per (trajectory, stage), 64 consecutive (b, k) pairs of the flattened index b N + k per wave,
//                          so a wave's 64 x 36 (64 x 18) entries of A (B) are ONE contiguous run whatever N is; the 2 (n + m)
//                          central differences are written into LDS and leave as whole contiguous rows; q, lo, hi likewise
//   scvx_advance_kernel    one lane per trajectory, sequential in k: the candidate (u_new, x_new), J_lin, J_new, du_max and the
//                          accept / reject / stop decision; inactive trajectories are loaded and left untouched
//   scvx_commit_kernel     elementwise: candidate -> reference where `take` is set (no model: it lives in admm_scvx.hip)
//
// Every kernel runs one wave per workgroup (SCVX_THREADS = 64).  No early return before a barrier: lanes past the end load the last
// trajectory / stage and store nothing.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/admm_hip.h"

namespace admm {

constexpr int SCVX_THREADS = 64;        // one wave: the LDS chunk belongs to it
constexpr int SCVX_NX = 6, SCVX_NU = 3, SCVX_NB = 9;
constexpr int SCVX_ROLL_CH = 8;         // stages per LDS chunk, rollout (64 x (24 + 1 + 48 + 1) doubles = 37 KB)
constexpr int SCVX_ADV_CH = 4;          // ... advance (64 x (36 + 12 + 24 + 3 + 12 + 24 + 2) doubles = 57 KB)
constexpr int SCVX_HIST = 9;            // doubles per history record

// What every model carries: the horizon and the step sizes the host derives once (dt / substeps, h / 2, h / 6)
struct ScvxGrid {
  int N, batch, substeps;
  double h, hh, h6;
};

// A model type M is the grid plus the parameters the host derives once from the caller's struct, and
//   static void rhs(const double (&s)[6], const double (&u)[3], const M& md, double (&d)[6])      d = f(s, u)
// (a model that reads per-node data: ScvxTakesNodes below) -- nothing else: RK4, the LDS chunking, the central differences, the cost chains and the decision below are one copy of code.

// scvx.relative_motion_rhs (admm_scvx_model; ADMM_SCVX_RELATIVE_CIRCULAR): the formulas in the same order (rd^3 = r2 sqrt(r2) for
// pow(r2, 1.5)); rc3 = rc^3
struct ScvxRelativeCircular : ScvxGrid {
  double rc, rc3;
  __device__ __forceinline__ static void rhs(const double (&s)[6], const double (&u)[3], const ScvxRelativeCircular& md, double (&d)[6]) {
    const double xr = md.rc + s[0];
    const double r2 = fma(s[2], s[2], fma(s[1], s[1], xr * xr));
    const double k = md.rc3 / (r2 * sqrt(r2));
    d[0] = s[3];
    d[1] = s[4];
    d[2] = s[5];
    d[3] = fma(-k, xr, fma(2.0, s[4], s[0]) + md.rc) + u[0];
    d[4] = fma(-k, s[1], fma(-2.0, s[3], s[1])) + u[1];
    d[5] = fma(-k, s[2], u[2]);
  }
};

// scvx.crtbp_rhs (ADMM_SCVX_CRTBP): the circular restricted three-body problem in the rotating frame, primaries at X = -mu and
// X = 1 - mu, position measured from (x_ref, 0, 0); om = 1 - mu.  The formulas in the same order (r sqrt(r) for the 3/2 power); no
// special handling near a primary: inf / NaN propagate into the cost, and the candidate then fails ratio >= rho_reject
struct ScvxCrtbp : ScvxGrid {
  double mu, om, x_ref;
  __device__ __forceinline__ static void rhs(const double (&s)[6], const double (&u)[3], const ScvxCrtbp& md, double (&d)[6]) {
    const double X = md.x_ref + s[0];
    const double d1 = X + md.mu, d2 = (X - 1.0) + md.mu;
    const double yz = fma(s[2], s[2], s[1] * s[1]);
    const double r1 = fma(d1, d1, yz), r2 = fma(d2, d2, yz);
    const double k1 = md.om / (r1 * sqrt(r1)), k2 = md.mu / (r2 * sqrt(r2));
    const double k12 = k1 + k2;
    d[0] = s[3];
    d[1] = s[4];
    d[2] = s[5];
    d[3] = fma(-k2, d2, fma(-k1, d1, fma(2.0, s[4], X))) + u[0];
    d[4] = fma(-k12, s[1], fma(-2.0, s[3], s[1])) + u[1];
    d[5] = fma(-k12, s[2], u[2]);
  }
};

// A model may read per-node data: it declares `static constexpr int NODE_PAR = ADMM_SCVX_NODE_PAR`, carries
// `const double* nodes` (row-major rows of NODE_PAR doubles, one per RK4 node of the horizon, shared by the batch) and its rhs takes
// the node's row: rhs(s, u, md, e, d).  A compile-time property: for the models without it the code below is the code it was.
template <class M, class = void>
struct ScvxTakesNodes { static constexpr bool value = false; };
template <class M>
struct ScvxTakesNodes<M, decltype((void)M::NODE_PAR)> { static constexpr bool value = true; };

// scvx.relative_tabulated_rhs (ADMM_SCVX_STAGE_RELATIVE_TABULATED): exact relative motion in the rotating frame of a chief that moves
// in a plane, x radial, y along-track, z cross-track; the node's row e = (rc, w, wd, g): chief radius, angular rate, angular
// acceleration, the chief's radial gravity mu / rc^2.  The formulas in the same order (r2 sqrt(r2) for the 3/2 power)
struct ScvxRelativeTabulated : ScvxGrid {
  static constexpr int NODE_PAR = ADMM_SCVX_NODE_PAR;
  double mu;
  const double* nodes;
  __device__ __forceinline__ static void rhs(const double (&s)[6], const double (&u)[3], const ScvxRelativeTabulated& md,
                                             const double (&e)[4], double (&d)[6]) {
    const double xr = e[0] + s[0];
    const double r2 = fma(s[2], s[2], fma(s[1], s[1], xr * xr));
    const double k = md.mu / (r2 * sqrt(r2));
    const double w2 = e[1] * e[1], tw = 2.0 * e[1];
    d[0] = s[3];
    d[1] = s[4];
    d[2] = s[5];
    d[3] = fma(-k, xr, fma(w2, s[0], fma(e[2], s[1], tw * s[4])) + e[3]) + u[0];
    d[4] = fma(-k, s[1], fma(w2, s[1], fma(-e[2], s[0], -tw * s[3]))) + u[1];
    d[5] = fma(-k, s[2], u[2]);
  }
};

template <class M>
__device__ __forceinline__ void scvx_rhs(const double (&s)[6], const double (&u)[3], const M& md, const double (&e)[4], double (&d)[6]) {
  if constexpr (ScvxTakesNodes<M>::value) M::rhs(s, u, md, e, d);
  else M::rhs(s, u, md, d);
}

// the first node row of stage k: global node 2 substeps k (a model without node data: no pointer)
template <class M>
__device__ __forceinline__ const double* scvx_stage_nodes(const M& md, int k) {
  if constexpr (ScvxTakesNodes<M>::value) return md.nodes + (size_t)k * (2 * md.substeps) * M::NODE_PAR;
  else return nullptr;
}

// rk4_step of the model: s <- F(s, u), classical RK4 over `substeps` sub-intervals under a held control.  nd: the stage's first
// node row (scvx_stage_nodes); sub-interval i reads rows 2 i (k1), 2 i + 1 (k2, k3) and 2 i + 2 (k4, the next one's first)
template <class M>
__device__ __forceinline__ void scvx_step(double (&s)[6], const double (&u)[3], const M& md, const double* __restrict__ nd) {
  constexpr bool NODES = ScvxTakesNodes<M>::value;
  double e0[4] = {}, e1[4] = {}, e2[4] = {};
  if constexpr (NODES) {
#pragma unroll
    for (int i = 0; i < 4; ++i) e0[i] = nd[i];
  }
#pragma unroll 1
  for (int sub = 0; sub < md.substeps; ++sub) {
    if constexpr (NODES) {
#pragma unroll
      for (int i = 0; i < 4; ++i) { e1[i] = nd[(2 * sub + 1) * 4 + i]; e2[i] = nd[(2 * sub + 2) * 4 + i]; }
    }
    double k[6], acc[6], t[6];
    scvx_rhs(s, u, md, e0, k);
#pragma unroll
    for (int i = 0; i < 6; ++i) { acc[i] = k[i]; t[i] = fma(md.hh, k[i], s[i]); }
    scvx_rhs(t, u, md, e1, k);
#pragma unroll
    for (int i = 0; i < 6; ++i) { acc[i] = fma(2.0, k[i], acc[i]); t[i] = fma(md.hh, k[i], s[i]); }
    scvx_rhs(t, u, md, e1, k);
#pragma unroll
    for (int i = 0; i < 6; ++i) { acc[i] = fma(2.0, k[i], acc[i]); t[i] = fma(md.h, k[i], s[i]); }
    scvx_rhs(t, u, md, e2, k);
#pragma unroll
    for (int i = 0; i < 6; ++i) s[i] = fma(md.h6, acc[i] + k[i], s[i]);
    if constexpr (NODES) {
#pragma unroll
      for (int i = 0; i < 4; ++i) e0[i] = e2[i];
    }
  }
}

// v' M v added to acc (M row-major, D x D): one fma chain per row, one per accumulator
template <int D>
__device__ __forceinline__ double scvx_quad(const double* M, const double (&v)[D], double acc) {
#pragma unroll
  for (int i = 0; i < D; ++i) {
    double r = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) r = fma(M[i * D + j], v[j], r);
    acc = fma(v[i], r, acc);
  }
  return acc;
}

// scvx.trajectory_cost, stage by stage: cu += u' R u, then x' Q x (cx) or, at the last stage, x' QN x (cn)
__device__ __forceinline__ void scvx_cost_stage(const admm_scvx_params& pr, const double (&u)[3], const double (&x)[6], bool last,
                                                double& cu, double& cx, double& cn) {
  cu = scvx_quad<3>(pr.R, u, cu);
  if (last) cn = scvx_quad<6>(pr.QN, x, cn);
  else cx = scvx_quad<6>(pr.Q, x, cx);
}
__device__ __forceinline__ double scvx_cost_total(double cu, double cx, double cn) { return 0.5 * cu + 0.5 * cx + 0.5 * cn; }

// A wave's chunk of a (batch, N, W) array: stages [k0, k0 + kc) of trajectories b0 .. b0 + 63 (past the batch: the last one), as 64
// contiguous runs of kc W doubles; LDS row t (stride W CH + 1, odd: lane-wise reads of one column hit distinct banks) holds run t.
template <int W, int CH>
__device__ __forceinline__ void scvx_chunk_load(double* lds, const double* __restrict__ g, int b0, int batch, int N, int k0, int kc,
                                                int lane) {
  constexpr int STRIDE = W * CH + 1;
  const int run = kc * W;
  for (int i = lane; i < SCVX_THREADS * run; i += SCVX_THREADS) {
    const int t = i / run, j = i - t * run;
    const int b = min(b0 + t, batch - 1);
    lds[t * STRIDE + j] = g[((size_t)b * N + k0) * W + j];
  }
}

// ... and back: rows of trajectories inside the batch whose flag (if given) is set
template <int W, int CH>
__device__ __forceinline__ void scvx_chunk_store(const double* lds, double* __restrict__ g, int b0, int batch, int N, int k0, int kc,
                                                 int lane, const int* row_on = nullptr) {
  constexpr int STRIDE = W * CH + 1;
  const int run = kc * W;
  for (int i = lane; i < SCVX_THREADS * run; i += SCVX_THREADS) {
    const int t = i / run, j = i - t * run;
    if (b0 + t < batch && (!row_on || row_on[t])) g[((size_t)(b0 + t) * N + k0) * W + j] = lds[t * STRIDE + j];
  }
}

// x is a NaN, by its bits: exponent all ones, mantissa not zero (isnan() is folded away under -fno-honor-nans)
__device__ __forceinline__ bool scvx_is_nan(double x) {
  return ((unsigned long long)__double_as_longlong(x) & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
}

// What admm_scvx_init_device sets besides ub = 0 and xb = rollout(x0, 0)
struct ScvxInit {
  double *J, *tr_u, *tr_x;
  int32_t *active, *converged, *accepted, *outer, *take;
  double tr_u0, tr_x0;
};

template <class M, bool INIT>
__global__ __launch_bounds__(SCVX_THREADS) void scvx_rollout_kernel(M md, admm_scvx_params pr, const double* __restrict__ x0,
                                                                    const double* __restrict__ u, double* __restrict__ x, ScvxInit in) {
  constexpr int CH = SCVX_ROLL_CH, SU = SCVX_NU * CH + 1, SX = SCVX_NX * CH + 1;
  __shared__ double lu[SCVX_THREADS * SU];
  __shared__ double lx[SCVX_THREADS * SX];
  const int lane = threadIdx.x, b0 = blockIdx.x * SCVX_THREADS;
  const bool valid = b0 + lane < md.batch;
  const int b = valid ? b0 + lane : md.batch - 1;
  double s[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) s[i] = x0[(size_t)b * 6 + i];
  double cu = 0.0, cx = 0.0, cn = 0.0;
  for (int k0 = 0; k0 < md.N; k0 += CH) {
    const int kc = min(CH, md.N - k0);
    scvx_chunk_load<SCVX_NU, CH>(lu, u, b0, md.batch, md.N, k0, kc, lane);
    __syncthreads();
    for (int kk = 0; kk < kc; ++kk) {
      double uk[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) uk[i] = lu[lane * SU + kk * 3 + i];
      scvx_step(s, uk, md, scvx_stage_nodes(md, k0 + kk));
#pragma unroll
      for (int i = 0; i < 6; ++i) lx[lane * SX + kk * 6 + i] = s[i];
      if (INIT) scvx_cost_stage(pr, uk, s, k0 + kk == md.N - 1, cu, cx, cn);
    }
    __syncthreads();
    scvx_chunk_store<SCVX_NX, CH>(lx, x, b0, md.batch, md.N, k0, kc, lane);
  }
  if (INIT && valid) {
    in.J[b] = scvx_cost_total(cu, cx, cn);
    in.tr_u[b] = in.tr_u0;
    in.tr_x[b] = in.tr_x0;
    in.active[b] = 1;
    in.converged[b] = 0;
    in.accepted[b] = 0;
    in.outer[b] = 0;
    in.take[b] = 0;
  }
}

// One lane per (trajectory, stage): flat index i = b N + k.  A_k, B_k of scvx.linearise at (xprev_k, u_k) -- xprev_0 = x0, else
// xb_{k-1} --, and the stage's q, lo, hi of scvx.correction_qp_batch; an inactive trajectory gets trust radii 0.
template <class M>
__global__ __launch_bounds__(SCVX_THREADS) void scvx_linearise_kernel(M md, admm_scvx_params pr, const double* __restrict__ x0,
                                                                      const double* __restrict__ ub, const double* __restrict__ xb,
                                                                      const double* __restrict__ tr_u, const double* __restrict__ tr_x,
                                                                      const int32_t* __restrict__ active, double* __restrict__ A,
                                                                      double* __restrict__ Bm, double* __restrict__ lo,
                                                                      double* __restrict__ hi, double* __restrict__ q) {
  constexpr int SA = 37, SB = 19, SQ = 9;        // odd LDS row strides of the 36 | 18 | 9 entries a lane leaves
  __shared__ double lds[SCVX_THREADS * SA];
  const int lane = threadIdx.x;
  const size_t total = (size_t)md.batch * md.N, i0 = (size_t)blockIdx.x * SCVX_THREADS;
  const int nvalid = (int)(total - i0 < (size_t)SCVX_THREADS ? total - i0 : (size_t)SCVX_THREADS);
  const size_t i = i0 + (lane < nvalid ? lane : nvalid - 1);
  const int b = (int)(i / md.N), k = (int)(i - (size_t)b * md.N);
  double xp[6], u[3];
  const double* xsrc = k == 0 ? x0 + (size_t)b * 6 : xb + (i - 1) * 6;
#pragma unroll
  for (int r = 0; r < 6; ++r) xp[r] = xsrc[r];
#pragma unroll
  for (int r = 0; r < 3; ++r) u[r] = ub[i * 3 + r];
  const double eps = pr.fd_eps, inv = 2.0 * eps;
  const double* nd = scvx_stage_nodes(md, k);          // this lane's stage: its own rows

  // direction j: state j (j < 6: column j of A), control j - 6 (column j - 6 of B).  The perturbation is added as in the host code,
  // x + d with d = eps e_j (x + 0.0 = x on the other rows), selected per row so that no register array is indexed by j
#pragma unroll 1
  for (int j = 0; j < 9; ++j) {
    if (j == 6) {                                // A complete: out as one contiguous run
      __syncthreads();
      for (int e = lane; e < nvalid * 36; e += SCVX_THREADS) A[i0 * 36 + e] = lds[(e / 36) * SA + e % 36];
      __syncthreads();
    }
    double fp[6], fm[6], up[3];
#pragma unroll
    for (int r = 0; r < 6; ++r) fp[r] = xp[r] + (r == j ? eps : 0.0);
#pragma unroll
    for (int r = 0; r < 3; ++r) up[r] = u[r] + (r + 6 == j ? eps : 0.0);
    scvx_step(fp, up, md, nd);
#pragma unroll
    for (int r = 0; r < 6; ++r) fm[r] = xp[r] - (r == j ? eps : 0.0);
#pragma unroll
    for (int r = 0; r < 3; ++r) up[r] = u[r] - (r + 6 == j ? eps : 0.0);
    scvx_step(fm, up, md, nd);
    if (j < 6) {
#pragma unroll
      for (int r = 0; r < 6; ++r) lds[lane * SA + r * 6 + j] = (fp[r] - fm[r]) / inv;
    } else {
#pragma unroll
      for (int r = 0; r < 6; ++r) lds[lane * SB + r * 3 + (j - 6)] = (fp[r] - fm[r]) / inv;
    }
  }
  __syncthreads();
  for (int e = lane; e < nvalid * 18; e += SCVX_THREADS) Bm[i0 * 18 + e] = lds[(e / 18) * SB + e % 18];
  __syncthreads();

  // q = (R ub_k, Q xb_k) -- QN at the last stage --; lo, hi: the control box inside the trust radius, the state trust radius
  double xs[6];
#pragma unroll
  for (int r = 0; r < 6; ++r) xs[r] = xb[i * 6 + r];
  const bool on = active[b] != 0;
  const double tu = on ? tr_u[b] : 0.0, tx = on ? tr_x[b] : 0.0;
  double* lq = lds;
  double* llo = lds + SCVX_THREADS * SQ;
  double* lhi = lds + 2 * SCVX_THREADS * SQ;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double a = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) a = fma(pr.R[r * 3 + c], u[c], a);
    lq[lane * SQ + r] = a;
    llo[lane * SQ + r] = fmax(pr.u_lo[r] - u[r], -tu);
    lhi[lane * SQ + r] = fmin(pr.u_hi[r] - u[r], tu);
  }
  const bool last = k == md.N - 1;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    double a = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) a = fma(last ? pr.QN[r * 6 + c] : pr.Q[r * 6 + c], xs[c], a);
    lq[lane * SQ + 3 + r] = a;
    llo[lane * SQ + 3 + r] = -tx;
    lhi[lane * SQ + 3 + r] = tx;
  }
  __syncthreads();
  for (int e = lane; e < nvalid * 9; e += SCVX_THREADS) {
    q[i0 * 9 + e] = lq[e];
    lo[i0 * 9 + e] = llo[e];
    hi[i0 * 9 + e] = lhi[e];
  }
}

// The decision block of scvx.scvx_batch for every ACTIVE trajectory, after the candidate has been built from z in one pass over the
// stages; adds the number of trajectories still active afterwards to *n_active (one atomic per wave).
template <class M>
__global__ __launch_bounds__(SCVX_THREADS) void scvx_advance_kernel(M md, admm_scvx_params pr, const double* __restrict__ x0,
                                                                    const double* __restrict__ z, admm_scvx_state st,
                                                                    int* __restrict__ n_active) {
  constexpr int CH = SCVX_ADV_CH, SZ = SCVX_NB * CH + 1, SU = SCVX_NU * CH + 1, SX = SCVX_NX * CH + 1;
  __shared__ double lz[SCVX_THREADS * SZ];
  __shared__ double lu[SCVX_THREADS * SU];
  __shared__ double lx[SCVX_THREADS * SX];
  __shared__ double ou[SCVX_THREADS * SU];
  __shared__ double ox[SCVX_THREADS * SX];
  __shared__ int row_on[SCVX_THREADS];
  const int lane = threadIdx.x, b0 = blockIdx.x * SCVX_THREADS;
  const bool valid = b0 + lane < md.batch;
  const int b = valid ? b0 + lane : md.batch - 1;
  const bool on = valid && st.active[b] != 0;
  row_on[lane] = on;
  double s[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) s[i] = x0[(size_t)b * 6 + i];
  double lu_c = 0.0, lx_c = 0.0, ln_c = 0.0;     // J_lin = cost(xb + dx, ub + du)
  double nu_c = 0.0, nx_c = 0.0, nn_c = 0.0;     // J_new = cost(x_new, u_new)
  double du_max = 0.0;
  for (int k0 = 0; k0 < md.N; k0 += CH) {
    const int kc = min(CH, md.N - k0);
    scvx_chunk_load<SCVX_NB, CH>(lz, z, b0, md.batch, md.N, k0, kc, lane);
    scvx_chunk_load<SCVX_NU, CH>(lu, st.ub, b0, md.batch, md.N, k0, kc, lane);
    scvx_chunk_load<SCVX_NX, CH>(lx, st.xb, b0, md.batch, md.N, k0, kc, lane);
    __syncthreads();
    for (int kk = 0; kk < kc; ++kk) {
      const bool last = k0 + kk == md.N - 1;
      double ul[3], xl[6], un[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double du = lz[lane * SZ + kk * 9 + i], ubk = lu[lane * SU + kk * 3 + i];
        du_max = fmax(du_max, fabs(du));
        ul[i] = ubk + du;
        un[i] = fmin(fmax(ul[i], pr.u_lo[i]), pr.u_hi[i]);
        ou[lane * SU + kk * 3 + i] = un[i];
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) xl[i] = lx[lane * SX + kk * 6 + i] + lz[lane * SZ + kk * 9 + 3 + i];
      scvx_cost_stage(pr, ul, xl, last, lu_c, lx_c, ln_c);
      scvx_step(s, un, md, scvx_stage_nodes(md, k0 + kk));
#pragma unroll
      for (int i = 0; i < 6; ++i) ox[lane * SX + kk * 6 + i] = s[i];
      scvx_cost_stage(pr, un, s, last, nu_c, nx_c, nn_c);
    }
    __syncthreads();
    scvx_chunk_store<SCVX_NU, CH>(ou, st.u_cand, b0, md.batch, md.N, k0, kc, lane, row_on);
    scvx_chunk_store<SCVX_NX, CH>(ox, st.x_cand, b0, md.batch, md.N, k0, kc, lane, row_on);
  }
  bool still = false;
  if (on) {
    const double J = st.J[b], tu = st.tr_u[b], tx = st.tr_x[b];
    const double J_lin = scvx_cost_total(lu_c, lx_c, ln_c), J_new = scvx_cost_total(nu_c, nx_c, nn_c);
    const double predicted = J - J_lin, actual = J - J_new;
    // a NaN compares false in scvx.outer_update: no stop, no accept.  Device code is built with -fno-honor-nans, under which a
    // compare and its complement are interchangeable, so the NaN cases are taken out by a test of the bits before any compare
    const bool pred_nan = scvx_is_nan(predicted);
    const double ratio = !pred_nan && predicted > 0.0 ? actual / predicted : -INFINITY;
    const bool ratio_nan = scvx_is_nan(ratio);
    const int it = st.outer[b];
    bool acc = false, stop = false;
    if (!pred_nan && predicted <= pr.tol * fmax(1.0, fabs(J))) {          // the model sees nothing left to gain
      stop = true;
    } else {
      acc = !ratio_nan && ratio >= pr.rho_reject;
      if (acc) {
        st.J[b] = J_new;
        st.accepted[b] += 1;
        if (ratio >= pr.rho_expand) { st.tr_u[b] = 2.0 * tu; st.tr_x[b] = 2.0 * tx; }
      } else {
        st.tr_u[b] = 0.5 * tu;
        st.tr_x[b] = 0.5 * tx;
      }
      stop = acc && du_max <= pr.tol;
    }
    double* rec = st.history + ((size_t)it * md.batch + b) * SCVX_HIST;
    rec[0] = J; rec[1] = J_new; rec[2] = predicted; rec[3] = actual; rec[4] = ratio;
    rec[5] = tu; rec[6] = tx; rec[7] = du_max; rec[8] = acc ? 1.0 : 0.0;
    st.outer[b] = it + 1;
    if (stop) { st.converged[b] = 1; st.active[b] = 0; }
    st.take[b] = acc ? 1 : 0;
    still = !stop;
  } else if (valid) {
    st.take[b] = 0;
  }
  const unsigned long long m = __ballot(still);
  if (lane == 0 && m) atomicAdd(n_active, __popcll(m));
}

}  // namespace admm
