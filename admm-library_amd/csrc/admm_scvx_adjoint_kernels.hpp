// admm_scvx_adjoint_kernels.hpp -- costates, primer vector, reduced gradient and the first-order optimality measure of the NONLINEAR
// problem the device SCvx loop works on (ADMM_HIP_HAS_SCVX_ADJOINT): one backward sweep over what
// admm_scvx_prepare_device wrote about the current reference.  Model-independent: it reads ub, A, B, q and the control box, nothing
// else.  fp64, explicit fma(), no inline assembly.
//
// Per trajectory, k = N-1 .. 0 (arrays as in admm_scvx_kernels.hpp; q_k = (qu_k, qx_k) = q[b, k, 0:3 | 3:9]):
//   nu_N     = -qx_{N-1}
//   nu_{k+1} = A_{k+1}' nu_{k+2} - qx_k          acc = -qx_k[i]; acc = fma(A_{k+1}[j][i], nu_{k+2}[j], acc), j = 0 .. 5
//   primer_k = B_k' nu_{k+1}                     acc = 0;        acc = fma(B_k[i][j], nu_{k+1}[i], acc),     i = 0 .. 5
//   grad_k   = qu_k - primer_k
//   dJdx0    = -(A_0' nu_1)                      acc = 0;        acc = fma(A_0[j][i], nu_1[j], acc),         j = 0 .. 5; negated
//   stat     = max over (k, j) of the violation of grad_k[j] at ub_k[j] in the box (scvx_adjoint_violation); NaN if a grad is
//   n_bound  = the number of (k, j) with ub_k[j] == u_lo[j] or ub_k[j] == u_hi[j]
//
//   scvx_adjoint_kernel  one lane per trajectory, one wave per workgroup, sequential in k.  A lane's stage record (36 + 18 + 9 + 3
//                        doubles) lies N 36 8 bytes from its neighbour's, so every stage goes through LDS: the wave fetches the 64
//                        records as contiguous runs into REGISTERS (66 loads per lane), puts them into LDS rows of odd stride and
//                        each lane reads its own row back.  The fetch of stage k - 1 is issued before stage k is consumed; the
//                        registers are put into LDS after it.  The three per-stage outputs leave the same way in reverse.
//                        A runs one stage behind B, q, u (the record of stage k holds A_{k+1}): the recursion needs them together.
//                        One stage per chunk: a second one would not fit beside the first (2 x 34 KB + outputs > 64 KB), and the
//                        registers that hold the stage in flight are what a deeper chunk would need LDS for.
// No early return before a barrier: lanes past the end fetch the last trajectory and store nothing.
#pragma once

#include "admm_scvx_kernels.hpp"

namespace admm {

constexpr int SCVX_ADJ_IN = 67;         // doubles per LDS row of a stage record: A 0..35 | B 36..53 | q 54..62 | u 63..65, + 1 (odd)
constexpr int SCVX_ADJ_OUT = 13;        // ... of a stage's outputs: nu 0..5 | primer 6..8 | grad 9..11, + 1 (odd)
constexpr int SCVX_ADJ_A = 0, SCVX_ADJ_B = 36, SCVX_ADJ_Q = 54, SCVX_ADJ_U = 63;
constexpr int SCVX_ADJ_NU = 0, SCVX_ADJ_PRIMER = 6, SCVX_ADJ_GRAD = 9;

struct ScvxBox { double lo[3], hi[3]; };
constexpr int SCVX_ADJ_MAX_N = 900000;  // 64 N 36 entries of a wave's A rows are indexed by an int

// Stage k of a (batch, N, W) array for the wave's 64 trajectories (past the batch: the last one), 64 runs of W doubles, into W
// registers per lane.  The runs are taken in G groups of TPG trajectories that S = W / gcd(W, 64) instructions cover exactly
// (64 S = TPG W), so that a lane's place (t, j) in instruction s of group g is (g TPG + (lane + 64 s) / W, (lane + 64 s) % W): S
// divisions per lane, not W, and offsets that fit an int (the host refuses N > SCVX_ADJ_MAX_N).  tmax = batch - 1 - b0
template <int W>
struct ScvxAdjRuns {
  static constexpr int gcd(int a, int b) { return b == 0 ? a : gcd(b, a % b); }
  static constexpr int S = W / gcd(W, SCVX_THREADS), TPG = SCVX_THREADS * S / W, G = SCVX_THREADS / TPG;
  static_assert(S * G == W && TPG * G == SCVX_THREADS, "the groups tile the wave's runs");
};

template <int W>
__device__ __forceinline__ void scvx_adjoint_fetch(double (&r)[W], const double* __restrict__ g, int b0, int tmax, int N, int k, int lane) {
  using R = ScvxAdjRuns<W>;
  const double* base = g + ((size_t)b0 * N + k) * W;
  const int NW = N * W;
#pragma unroll
  for (int gr = 0; gr < R::G; ++gr) {
#pragma unroll
    for (int s = 0; s < R::S; ++s) {
      const int i = lane + SCVX_THREADS * s, tl = i / W, j = i - tl * W;
      r[gr * R::S + s] = base[min(gr * R::TPG + tl, tmax) * NW + j];
    }
  }
}

// ... from the registers into the LDS rows: run t at lds[t STRIDE + OFF ..]
template <int W, int STRIDE, int OFF>
__device__ __forceinline__ void scvx_adjoint_put(double* lds, const double (&r)[W], int lane) {
  using R = ScvxAdjRuns<W>;
#pragma unroll
  for (int gr = 0; gr < R::G; ++gr) {
#pragma unroll
    for (int s = 0; s < R::S; ++s) {
      const int i = lane + SCVX_THREADS * s, tl = i / W, j = i - tl * W;
      lds[(gr * R::TPG + tl) * STRIDE + OFF + j] = r[gr * R::S + s];
    }
  }
}

// Stage k of a (batch, N, W) output from the LDS rows, as contiguous runs; rows of trajectories inside the batch only
template <int W, int STRIDE, int OFF>
__device__ __forceinline__ void scvx_adjoint_store(const double* lds, double* __restrict__ g, int b0, int tmax, int N, int k, int lane) {
  using R = ScvxAdjRuns<W>;
  double* base = g + ((size_t)b0 * N + k) * W;
  const int NW = N * W;
#pragma unroll
  for (int gr = 0; gr < R::G; ++gr) {
#pragma unroll
    for (int s = 0; s < R::S; ++s) {
      const int i = lane + SCVX_THREADS * s, tl = i / W, j = i - tl * W, t = gr * R::TPG + tl;
      if (t <= tmax) base[t * NW + j] = lds[t * STRIDE + OFF + j];
    }
  }
}

// The violation of first-order optimality of a component with gradient g at u in [lo, hi], exact comparisons: a fixed component
// has none; on a bound only the sign that pushes inwards counts; in the interior |g|.  g is not a NaN here (the caller's test)
__device__ __forceinline__ double scvx_adjoint_violation(double g, double u, double lo, double hi) {
  if (lo == hi) return 0.0;
  if (u == lo) return fmax(-g, 0.0);
  if (u == hi) return fmax(g, 0.0);
  return fabs(g);
}

__global__ __launch_bounds__(SCVX_THREADS) void scvx_adjoint_kernel(int N, int batch, ScvxBox box, const double* __restrict__ ub,
                                                                    const double* __restrict__ A, const double* __restrict__ Bm,
                                                                    const double* __restrict__ q, admm_scvx_adjoint_out out) {
  constexpr int SI = SCVX_ADJ_IN, SO = SCVX_ADJ_OUT;
  __shared__ double lin[SCVX_THREADS * SI];
  __shared__ double lout[SCVX_THREADS * SO];
  const int lane = threadIdx.x, b0 = blockIdx.x * SCVX_THREADS;
  const int tmax = min(batch - 1 - b0, SCVX_THREADS - 1);
  const bool valid = lane <= tmax;
  const double* row = lin + lane * SI;
  double* orow = lout + lane * SO;

  // the record in flight.  A runs one stage behind: next to B_k, q_k, u_k the row holds A_{k+1} (none at k = N - 1)
  double fa[36], fb[18], fq[9], fu[3];
  scvx_adjoint_fetch<18>(fb, Bm, b0, tmax, N, N - 1, lane);
  scvx_adjoint_fetch<9>(fq, q, b0, tmax, N, N - 1, lane);
  scvx_adjoint_fetch<3>(fu, ub, b0, tmax, N, N - 1, lane);
  scvx_adjoint_put<18, SI, SCVX_ADJ_B>(lin, fb, lane);
  scvx_adjoint_put<9, SI, SCVX_ADJ_Q>(lin, fq, lane);
  scvx_adjoint_put<3, SI, SCVX_ADJ_U>(lin, fu, lane);
  __syncthreads();

  double nu[6];                                   // nu_{k+2}
#pragma unroll
  for (int i = 0; i < 6; ++i) nu[i] = 0.0;
  double stat = 0.0;
  bool has_nan = false;
  int n_bound = 0;

  for (int k = N - 1; k >= 0; --k) {
    // the next record's loads leave before this one is consumed: A_k (the last one for dJdx0) and B, q, u of stage k - 1
    scvx_adjoint_fetch<36>(fa, A, b0, tmax, N, k, lane);
    if (k > 0) {
      scvx_adjoint_fetch<18>(fb, Bm, b0, tmax, N, k - 1, lane);
      scvx_adjoint_fetch<9>(fq, q, b0, tmax, N, k - 1, lane);
      scvx_adjoint_fetch<3>(fu, ub, b0, tmax, N, k - 1, lane);
    }
    double nn[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double acc = -row[SCVX_ADJ_Q + 3 + i];
      if (k < N - 1) {
#pragma unroll
        for (int j = 0; j < 6; ++j) acc = fma(row[SCVX_ADJ_A + j * 6 + i], nu[j], acc);
      }
      nn[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) nu[i] = nn[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double p = 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) p = fma(row[SCVX_ADJ_B + i * 3 + j], nu[i], p);
      const double g = row[SCVX_ADJ_Q + j] - p, u = row[SCVX_ADJ_U + j];
      if (scvx_is_nan(g)) has_nan = true;
      else stat = fmax(stat, scvx_adjoint_violation(g, u, box.lo[j], box.hi[j]));
      n_bound += (u == box.lo[j] || u == box.hi[j]) ? 1 : 0;
      if (out.primer) orow[SCVX_ADJ_PRIMER + j] = p;
      if (out.grad) orow[SCVX_ADJ_GRAD + j] = g;
    }
    if (out.nu) {
#pragma unroll
      for (int i = 0; i < 6; ++i) orow[SCVX_ADJ_NU + i] = nu[i];
    }
    __syncthreads();                              // every row of this stage read, every output row written
    if (out.nu) scvx_adjoint_store<6, SO, SCVX_ADJ_NU>(lout, out.nu, b0, tmax, N, k, lane);
    if (out.primer) scvx_adjoint_store<3, SO, SCVX_ADJ_PRIMER>(lout, out.primer, b0, tmax, N, k, lane);
    if (out.grad) scvx_adjoint_store<3, SO, SCVX_ADJ_GRAD>(lout, out.grad, b0, tmax, N, k, lane);
    scvx_adjoint_put<36, SI, SCVX_ADJ_A>(lin, fa, lane);
    if (k > 0) {
      scvx_adjoint_put<18, SI, SCVX_ADJ_B>(lin, fb, lane);
      scvx_adjoint_put<9, SI, SCVX_ADJ_Q>(lin, fq, lane);
      scvx_adjoint_put<3, SI, SCVX_ADJ_U>(lin, fu, lane);
    }
    __syncthreads();                              // the next record is in place, the output rows are free
  }
  if (valid) {
    const int b = b0 + lane;
    if (out.dJdx0) {                              // the row's A is A_0, nu is nu_1
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) acc = fma(row[SCVX_ADJ_A + j * 6 + i], nu[j], acc);
        out.dJdx0[(size_t)b * 6 + i] = -acc;
      }
    }
    // a NaN by its bits: the unit is built with -fno-honor-nans, under which fmax need not keep one
    if (out.stat) out.stat[b] = has_nan ? __longlong_as_double(0x7ff8000000000000ll) : stat;
    if (out.n_bound) out.n_bound[b] = n_bound;
  }
}

}  // namespace admm
