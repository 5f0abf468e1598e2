// admm_cert_kernels.hpp -- certificate kernels: costates, objective, dynamics defect and stationarity defect of every
// QP at the handle's (z, y) pair, on the device.  fp64, one lane per QP (batch-minor coalesced state rows, wave-uniform stage
// operands staged through LDS and read as broadcasts: DESIGN.md §4.5), parallel in time over the handle's segments:
//
//   pass A   (column block, segment): the costate recursion over the segment's stages with zero inflow; reads the state rows of
//            z, y, q only and leaves the carry it hands to the previous segment, c_s (n doubles per QP)
//   link     per QP, sequential in S:  c_in(S-1) = 0,  c_in(s-1) = c_s + Phi_s c_in(s)      (Phi_s: host, fp64)
//   pass B   the same recursion from the true inflow: writes nu (if asked for) and the segment's partial objective,
//            max |dynamics defect| and max |stationarity defect|
//   finalise per QP, the S partials in segment order (deterministic)
//
// With block k = (u_k, x_{k+1}), g = P z + q + rho y and carry c = A_{k+1}' nu_{k+2} (0 at the horizon's end):
//   nu_{k+1} = c - g^x_{k+1};   defect_u = g^u_k - B_k' nu_{k+1};   e = x_{k+1} - A_k x_k - B_k u_k;   c <- A_k' nu_{k+1}
#pragma once

#include "admm_cert.hpp"
#include "admm_select.hpp"

#include <cstddef>
#include <cstdint>

namespace admm {

constexpr int CERT_THREADS = 256;

constexpr int cert_rec(int nx, int nu) { return nx * (nx + nu); }                 // doubles per stage: A_k | B_k
constexpr int cert_chunk(int nx, int nu) {                                        // stages staged in LDS at once (<= 32 KiB)
  int ch = 4096 / cert_rec(nx, nu);
  return ch > 64 ? 64 : (ch < 1 ? 1 : ch);
}

// Large blocks: a scheduling barrier every few rows of a mat-vec bounds how far the LDS operand reads are hoisted ahead of their
// FMAs (without it the (12, 6) forms hold several operators in registers at once and spill).
#define CERT_FENCE(ROW, STEP) do { if constexpr (NX + NU >= 10) { if (((ROW) % (STEP)) == (STEP) - 1) __builtin_amdgcn_sched_barrier(0); } } while (0)

template <int NX, int NU, bool HASQ, bool PASSB>
__global__ __launch_bounds__(CERT_THREADS) __attribute__((amdgpu_waves_per_eu(1, 2))) void cert_pass_kernel(
    const double* __restrict__ z, const double* __restrict__ y, const double* __restrict__ q, const double* __restrict__ x0,
    const double* __restrict__ AB, const double* __restrict__ QR, const double* __restrict__ fuel,
    const int* __restrict__ seg_start, const double* __restrict__ cin, double* __restrict__ cseg, double* __restrict__ part,
    double* __restrict__ nu_out, double rho, int N, int pitch) {
  constexpr int NB = NX + NU, RAB = cert_rec(NX, NU), CH = cert_chunk(NX, NU);
  __shared__ double rec[CH * RAB];
  __shared__ double wQ[NX * NX], wQN[NX * NX], wR[NU * NU];

  // no early return (every wave reaches the barriers): lanes past the pitch load the last column and store nothing
  const int col_raw = blockIdx.x * CERT_THREADS + threadIdx.x;
  const bool active = col_raw < pitch;
  const size_t P = (size_t)pitch, col = active ? col_raw : pitch - 1;
  const int s = blockIdx.y;
  const int k0 = seg_start[s], k1 = seg_start[s + 1];

  for (int i = threadIdx.x; i < NX * NX; i += CERT_THREADS) { wQ[i] = QR[i]; wQN[i] = QR[NX * NX + i]; }
  for (int i = threadIdx.x; i < NU * NU; i += CERT_THREADS) wR[i] = QR[2 * NX * NX + i];

  double c[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) c[i] = PASSB ? cin[((size_t)s * NX + i) * P + col] : 0.0;
  double obj = 0.0, feas = 0.0, stat = 0.0;

  for (int kc = k1 - 1; kc >= k0; kc -= CH) {          // LDS refill: stages kc, kc - 1, ..., klo
    const int klo = (kc - CH + 1 > k0) ? kc - CH + 1 : k0;
    __syncthreads();
    for (int i = threadIdx.x; i < (kc - klo + 1) * RAB; i += CERT_THREADS) rec[i] = AB[(size_t)klo * RAB + i];
    __syncthreads();
    for (int k = kc; k >= klo; --k) {
      const double* Ak = rec + (k - klo) * RAB;        // column-major: A(i, j) = Ak[i + j NX]
      const double* Bk = Ak + NX * NX;                 //               B(i, l) = Bk[i + l NX]
      const double* Qk = (k == N - 1) ? wQN : wQ;
      const size_t row0 = (size_t)k * NB;
      double zx[NX], gx[NX], nu[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        const size_t o = (row0 + NU + i) * P + col;
        zx[i] = z[o];
        gx[i] = rho * y[o];
        if (HASQ) gx[i] += q[o];
      }
      double zu[NU], gu[NU], xp[NX];
      if (PASSB) {
#pragma unroll
        for (int j = 0; j < NU; ++j) {
          const size_t o = (row0 + j) * P + col;
          zu[j] = z[o];
          gu[j] = rho * y[o];
          if (HASQ) { const double qq = q[o]; gu[j] += qq; obj = fma(qq, zu[j], obj); }
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) {
          xp[i] = k > 0 ? z[(row0 - NB + NU + i) * P + col] : x0[(size_t)i * P + col];
          if (HASQ) obj = fma(q[(row0 + NU + i) * P + col], zx[i], obj);
        }
      }
      // state rows: g^x = Q z_x + q_x + rho y_x, nu = c - g^x
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        double a = 0.0;
#pragma unroll
        for (int j = 0; j < NX; ++j) a = fma(Qk[i * NX + j], zx[j], a);
        if (PASSB) obj = fma(0.5 * zx[i], a, obj);
        gx[i] += a;
        nu[i] = c[i] - gx[i];
        CERT_FENCE(i, 3);
      }
      if (PASSB) {
        if (nu_out && active) {
#pragma unroll
          for (int i = 0; i < NX; ++i) nu_out[((size_t)k * NX + i) * P + col] = nu[i];
        }
        // control rows: g^u = R z_u + q_u + rho y_u, stationarity defect g^u - B' nu; fuel term
        double nrm2 = 0.0;
#pragma unroll
        for (int j = 0; j < NU; ++j) {
          double a = 0.0;
#pragma unroll
          for (int l = 0; l < NU; ++l) a = fma(wR[j * NU + l], zu[l], a);
          obj = fma(0.5 * zu[j], a, obj);
          double d = gu[j] + a;
#pragma unroll
          for (int i = 0; i < NX; ++i) d = fma(-Bk[i + j * NX], nu[i], d);
          stat = fmax(stat, fabs(d));
          nrm2 = fma(zu[j], zu[j], nrm2);
          CERT_FENCE(j, 3);
        }
        obj = fma(fuel[k], sqrt(nrm2), obj);
        // dynamics defect of stage k
#pragma unroll
        for (int i = 0; i < NX; ++i) {
          double e = zx[i];
#pragma unroll
          for (int j = 0; j < NX; ++j) e = fma(-Ak[i + j * NX], xp[j], e);
#pragma unroll
          for (int l = 0; l < NU; ++l) e = fma(-Bk[i + l * NX], zu[l], e);
          feas = fmax(feas, fabs(e));
          CERT_FENCE(i, 3);
        }
      }
      // carry to the previous block: c = A_k' nu
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        double a = 0.0;
#pragma unroll
        for (int j = 0; j < NX; ++j) a = fma(Ak[j + i * NX], nu[j], a);
        c[i] = a;
        CERT_FENCE(i, 3);
      }
    }
  }
  if (!active) return;                                  // (after the last barrier)
  if (PASSB) {
    const size_t o = (size_t)s * 3 * P + col;
    part[o] = obj;
    part[o + P] = feas;
    part[o + 2 * P] = stat;
  } else {
#pragma unroll
    for (int i = 0; i < NX; ++i) cseg[((size_t)s * NX + i) * P + col] = c[i];
  }
}

// c_in(S-1) = 0;  c_in(s-1) = c_s + Phi_s c_in(s).  One lane per QP; Phi is wave-uniform.
template <int NX>
__global__ __launch_bounds__(64) void cert_link_kernel(const double* __restrict__ cseg, const double* __restrict__ Phi,
                                                       double* __restrict__ cin, int S, int pitch) {
  const int col = blockIdx.x * 64 + threadIdx.x;
  if (col >= pitch) return;
  const size_t P = (size_t)pitch;
  double c[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) { c[i] = 0.0; cin[((size_t)(S - 1) * NX + i) * P + col] = 0.0; }
  for (int s = S - 1; s >= 1; --s) {
    const double* F = Phi + (size_t)s * NX * NX;
    double t[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      double a = cseg[((size_t)s * NX + i) * P + col];
#pragma unroll
      for (int j = 0; j < NX; ++j) a = fma(F[i * NX + j], c[j], a);
      t[i] = a;
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) { c[i] = t[i]; cin[((size_t)(s - 1) * NX + i) * P + col] = t[i]; }
  }
}

// the S partials of a QP in segment order: obj summed, the two defects maximised
static __global__ __launch_bounds__(64) void cert_finalize_kernel(const double* __restrict__ part, double* __restrict__ out, int S,
                                                                  int pitch) {
  const int col = blockIdx.x * 64 + threadIdx.x;
  if (col >= pitch) return;
  const size_t P = (size_t)pitch;
  double obj = 0.0, feas = 0.0, stat = 0.0;
  for (int s = 0; s < S; ++s) {
    const size_t o = (size_t)s * 3 * P + col;
    obj += part[o];
    feas = fmax(feas, part[o + P]);
    stat = fmax(stat, part[o + 2 * P]);
  }
  out[col] = obj;
  out[P + col] = feas;
  out[2 * P + col] = stat;
}

// Instantiated per (n, m) by the translation units of the one-lane family (admm_dims_impl.hpp), so the build's register report
// and spill gate cover these kernels with the rest of a shape's.
template <int NX, int NU>
inline void launch_cert_dim(const CertLaunch& l) {
  const dim3 grid((l.pitch + CERT_THREADS - 1) / CERT_THREADS, l.S), block(CERT_THREADS);
  const dim3 cols(l.pitch / 64), wave(64);
  auto pass = [&](auto HQ, auto PB) {
    hipLaunchKernelGGL((cert_pass_kernel<NX, NU, HQ(), PB()>), grid, block, 0, l.stream, l.z, l.y, l.q, l.x0, l.AB, l.QR, l.fuel,
                       l.seg_start, l.cin, l.cseg, l.part, l.nu, l.rho, l.N, l.pitch);
  };
  with_flags(pass, l.has_q, false);       // (HASQ, second pass)
  hipLaunchKernelGGL((cert_link_kernel<NX>), cols, wave, 0, l.stream, l.cseg, l.Phi, l.cin, l.S, l.pitch);
  with_flags(pass, l.has_q, true);
  hipLaunchKernelGGL(cert_finalize_kernel, cols, wave, 0, l.stream, l.part, l.out, l.S, l.pitch);
}

#undef CERT_FENCE

}  // namespace admm

