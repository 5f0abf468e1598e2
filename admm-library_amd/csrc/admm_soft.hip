// admm_soft.hip -- solver runtime: the z-update kernel of handles with soft box constraints, the read-out of the penalty, and their
// launch geometry (admm_soft.hpp).  The kernels take n and m at run time: eight forms for every shape, compiled here once.
#include "admm_soft.hpp"
#include "admm_soft_kernels.hpp"
#include "admm_select.hpp"

namespace admm {

void launch_soft(const SoftLaunch& l) {
  const dim3 grid((l.pitch / 2 + Z_THREADS - 1) / Z_THREADS, l.zchunks), block(Z_THREADS);
  const bool relax = l.alpha != 1.0;
  with_flags([&](auto RS, auto RX, auto SOC) {
    hipLaunchKernelGGL((zdual_soft_kernel<RS(), RX(), SOC()>), grid, block, 0, l.stream, l.w, l.z, l.y, l.lo, l.hi, l.skap, l.ub, l.kap,
                       l.part, l.alpha, l.L, l.zrows, l.pitch, l.nb, l.m);
  }, l.resid, relax, l.soc);
}

void launch_soft_report(hipStream_t stream, const double* z, const double* lo, const double* hi, const double* soft, double* penalty,
                        double* max_violation, int* n_violated, int L, int pitch, int batch) {
  const dim3 grid((batch + SOFT_REPORT_THREADS - 1) / SOFT_REPORT_THREADS), block(SOFT_REPORT_THREADS);
  hipLaunchKernelGGL(soft_report_kernel, grid, block, 0, stream, z, lo, hi, soft, penalty, max_violation, n_violated, L, pitch, batch);
}

}  // namespace admm
