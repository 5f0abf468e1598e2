// admm_infeas_kernels.hpp -- infeasibility kernels: a Farkas certificate of every QP from the drift of the scaled
// dual, lambda = (y - y0) / span, on the device.  fp64, one lane per QP (batch-minor coalesced rows, wave-uniform stage operands
// staged through LDS and read as broadcasts: DESIGN.md §4.5), parallel in time over the handle's segments like the certificate
// kernels (admm_cert_kernels.hpp), whose link kernel, A_k | B_k records and Phi_s they share:
//
//   pass A   (column block, segment): the ray-costate recursion over the segment's stages with zero inflow; reads the state rows
//            of y, y0 only and leaves the carry it hands to the previous segment, c_s (n doubles per QP)
//   link     cert_link_kernel
//   pass B   the same recursion from the true inflow: writes nu (if asked for), forms mu^u = B' nu and the segment's partial
//            support function, max |mu|, open, max |mu - lambda| and max |lambda|; segment 0 adds x0' (A_0' nu_1)
//   finalise per QP, the S partials in segment order (deterministic); the open rule, the normalisation and the flag
//
// With block k = (u_k, x_{k+1}) and carry c = A_{k+1}' nu_{k+2} (0 at the horizon's end):
//   nu_{k+1} = c - lambda^x_{k+1};   mu^x_{k+1} = lambda^x_{k+1};   mu^u_k = B_k' nu_{k+1};   c <- A_k' nu_{k+1}
#pragma once

#include "admm_cert_kernels.hpp"
#include "admm_infeas.hpp"

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace admm {

constexpr int infeas_bnd(int nx, int nu) { return 2 * (nx + nu) + 1; }            // doubles per stage: lo | hi | thrust bound

// (CERT_FENCE of admm_cert_kernels.hpp: bounds how far the LDS operand reads of a (12, 6) mat-vec are hoisted)
#define INFEAS_FENCE(ROW, STEP) do { if constexpr (NX + NU >= 10) { if (((ROW) % (STEP)) == (STEP) - 1) __builtin_amdgcn_sched_barrier(0); } } while (0)

// A box row's term of the support function: hi mu (mu > 0), lo mu (mu < 0).  An infinite bound is selected away BEFORE the
// multiplication (no inf * 0): the row then contributes nothing and |mu| enters `open`.
__device__ __forceinline__ void infeas_box_row(double mu, double lo, double hi, double& sig, double& open) {
  const double b = mu > 0.0 ? hi : lo;
  const bool fin = fabs(b) != INFINITY;
  sig = fma(fin ? b : 0.0, mu, sig);
  open = fmax(open, fin ? 0.0 : fabs(mu));
}

template <int NX, int NU, bool PASSB>
__global__ __launch_bounds__(CERT_THREADS) __attribute__((amdgpu_waves_per_eu(1, 2))) void infeas_pass_kernel(
    const double* __restrict__ y, const double* __restrict__ y0, const double* __restrict__ x0, const double* __restrict__ AB,
    const double* __restrict__ bnd, const int* __restrict__ seg_start, const double* __restrict__ cin, double* __restrict__ cseg,
    double* __restrict__ part, double* __restrict__ nu_out, double span, int pitch) {
  constexpr int NB = NX + NU, RAB = cert_rec(NX, NU), RBD = infeas_bnd(NX, NU), CH = cert_chunk(NX, NU);
  __shared__ double rec[CH * RAB];
  __shared__ double box[PASSB ? CH * RBD : 1];

  // no early return (every wave reaches the barriers): lanes past the pitch load the last column and store nothing
  const int col_raw = blockIdx.x * CERT_THREADS + threadIdx.x;
  const bool active = col_raw < pitch;
  const size_t P = (size_t)pitch, col = active ? col_raw : pitch - 1;
  const int s = blockIdx.y;
  const int k0 = seg_start[s], k1 = seg_start[s + 1];

  double c[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) c[i] = PASSB ? cin[((size_t)s * NX + i) * P + col] : 0.0;
  double sig = 0.0, mumax = 0.0, open = 0.0, dmax = 0.0, lmax = 0.0;

  for (int kc = k1 - 1; kc >= k0; kc -= CH) {          // LDS refill: stages kc, kc - 1, ..., klo
    const int klo = (kc - CH + 1 > k0) ? kc - CH + 1 : k0;
    __syncthreads();
    for (int i = threadIdx.x; i < (kc - klo + 1) * RAB; i += CERT_THREADS) rec[i] = AB[(size_t)klo * RAB + i];
    if (PASSB)
      for (int i = threadIdx.x; i < (kc - klo + 1) * RBD; i += CERT_THREADS) box[i] = bnd[(size_t)klo * RBD + i];
    __syncthreads();
    for (int k = kc; k >= klo; --k) {
      const double* Ak = rec + (k - klo) * RAB;        // column-major: A(i, j) = Ak[i + j NX]
      const double* Bk = Ak + NX * NX;                 //               B(i, l) = Bk[i + l NX]
      const size_t row0 = (size_t)k * NB;
      double lx[NX], nu[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        const size_t o = (row0 + NU + i) * P + col;
        lx[i] = (y[o] - y0[o]) / span;
        nu[i] = c[i] - lx[i];
      }
      if (PASSB) {
        const double* lo = box + (k - klo) * RBD;      // rows of block k: controls, then states
        const double* hi = lo + NB;
        const double ub = lo[2 * NB];
        if (nu_out && active) {
#pragma unroll
          for (int i = 0; i < NX; ++i) nu_out[((size_t)k * NX + i) * P + col] = nu[i];
        }
        // state rows: mu = lambda by construction
#pragma unroll
        for (int i = 0; i < NX; ++i) {
          const double a = fabs(lx[i]);
          mumax = fmax(mumax, a);
          lmax = fmax(lmax, a);
          infeas_box_row(lx[i], lo[NU + i], hi[NU + i], sig, open);
        }
        // control rows: mu = B' nu replaces lambda; the ball's support function where the stage has a thrust bound
        const bool ball = fabs(ub) != INFINITY;        // (wave-uniform)
        double nrm2 = 0.0;
#pragma unroll
        for (int j = 0; j < NU; ++j) {
          const size_t o = (row0 + j) * P + col;
          const double lu = (y[o] - y0[o]) / span;
          double mu = 0.0;
#pragma unroll
          for (int i = 0; i < NX; ++i) mu = fma(Bk[i + j * NX], nu[i], mu);
          mumax = fmax(mumax, fabs(mu));
          lmax = fmax(lmax, fabs(lu));
          dmax = fmax(dmax, fabs(mu - lu));
          if (ball) nrm2 = fma(mu, mu, nrm2);
          else infeas_box_row(mu, lo[j], hi[j], sig, open);
          INFEAS_FENCE(j, 3);
        }
        if (ball) sig = fma(ub, sqrt(nrm2), sig);
      }
      // carry to the previous block: c = A_k' nu
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        double a = 0.0;
#pragma unroll
        for (int j = 0; j < NX; ++j) a = fma(Ak[j + i * NX], nu[j], a);
        c[i] = a;
        INFEAS_FENCE(i, 3);
      }
    }
  }
  if (!active) return;                                  // (after the last barrier)
  if (PASSB) {
    if (s == 0) {                                       // h' nu = x0' (A_0' nu_1)
#pragma unroll
      for (int i = 0; i < NX; ++i) sig = fma(x0[(size_t)i * P + col], c[i], sig);
    }
    const size_t o = (size_t)s * 5 * P + col;
    part[o] = sig;
    part[o + P] = mumax;
    part[o + 2 * P] = open;
    part[o + 3 * P] = dmax;
    part[o + 4 * P] = lmax;
  } else {
#pragma unroll
    for (int i = 0; i < NX; ++i) cseg[((size_t)s * NX + i) * P + col] = c[i];
  }
}

// the S partials of a QP in segment order: sigma summed, the four norms maximised; then the open rule, the normalisation, the flag
static __global__ __launch_bounds__(64) void infeas_finalize_kernel(const double* __restrict__ part, double* __restrict__ out,
                                                                    double eps, int S, int pitch) {
  const int col = blockIdx.x * 64 + threadIdx.x;
  if (col >= pitch) return;
  const size_t P = (size_t)pitch;
  double sig = 0.0, mumax = 0.0, open = 0.0, dmax = 0.0, lmax = 0.0;
  for (int s = 0; s < S; ++s) {
    const size_t o = (size_t)s * 5 * P + col;
    sig += part[o];
    mumax = fmax(mumax, part[o + P]);
    open = fmax(open, part[o + 2 * P]);
    dmax = fmax(dmax, part[o + 3 * P]);
    lmax = fmax(lmax, part[o + 4 * P]);
  }
  const bool ray = mumax > 0.0 && open <= eps * mumax;
  const double sep = ray ? sig / mumax : INFINITY;
  out[col] = sep;
  out[P + col] = lmax;
  out[2 * P + col] = mumax > 0.0 ? dmax / mumax : (dmax > 0.0 ? INFINITY : 0.0);
  out[3 * P + col] = sep < -eps ? 1.0 : 0.0;
  out[4 * P + col] = mumax;
}

// Instantiated per (n, m) by the translation units of the one-lane family (admm_dims_impl.hpp), next to the certificate kernels,
// so the build's register report and spill gate cover them.
template <int NX, int NU>
inline void launch_infeas_dim(const InfeasLaunch& l) {
  const dim3 grid((l.pitch + CERT_THREADS - 1) / CERT_THREADS, l.S), block(CERT_THREADS);
  const dim3 cols(l.pitch / 64), wave(64);
  auto pass = [&](auto PB) {
    hipLaunchKernelGGL((infeas_pass_kernel<NX, NU, PB()>), grid, block, 0, l.stream, l.y, l.y0, l.x0, l.AB, l.bnd, l.seg_start,
                       l.cin, l.cseg, l.part, l.nu, l.span, l.pitch);
  };
  pass(std::false_type{});
  hipLaunchKernelGGL((cert_link_kernel<NX>), cols, wave, 0, l.stream, l.cseg, l.Phi, l.cin, l.S, l.pitch);
  pass(std::true_type{});
  hipLaunchKernelGGL(infeas_finalize_kernel, cols, wave, 0, l.stream, l.part, l.out, l.eps, l.S, l.pitch);
}

#undef INFEAS_FENCE

}  // namespace admm
