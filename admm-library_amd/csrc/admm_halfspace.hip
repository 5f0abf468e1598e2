// admm_halfspace.hip -- solver runtime: the z-update kernel of handles with one half-space per stage, its read-out, the device-side
// scan of per-QP planes, and their launch geometry (admm_halfspace.hpp).  The kernels take n, m and nh at run
// time: sixteen forms for every shape, compiled here once.
#include "admm_halfspace.hpp"
#include "admm_halfspace_kernels.hpp"
#include "admm_select.hpp"

namespace admm {

void launch_halfspace(const HalfspaceLaunch& l) {
  const dim3 grid((l.pitch / 2 + Z_THREADS - 1) / Z_THREADS, l.zchunks), block(Z_THREADS);
  const bool relax = l.alpha != 1.0;
  with_flags([&](auto RS, auto RX, auto SOC, auto PQ) {
    hipLaunchKernelGGL((zdual_halfspace_kernel<RS(), RX(), SOC(), PQ()>), grid, block, 0, l.stream, l.w, l.z, l.y, l.lo, l.hi, l.ub, l.kap,
                       l.a, l.b, l.part, l.alpha, l.L, l.zrows, l.pitch, l.nb, l.m, l.nh);
  }, l.resid, relax, l.soc, l.perqp);
}

void launch_halfspace_report(hipStream_t stream, const double* w, const double* y, const double* a, const double* b,
                             double* max_violation, int* n_active, double* lam, double rho, int N, int nb, int m, int nh, int pitch,
                             int batch, bool perqp) {
  const dim3 grid((batch + HS_REPORT_THREADS - 1) / HS_REPORT_THREADS), block(HS_REPORT_THREADS);
  hipLaunchKernelGGL(halfspace_report_kernel, grid, block, 0, stream, w, y, a, b, max_violation, n_active, lam, rho, N, nb, m, nh,
                     pitch, batch, perqp ? 1 : 0);
}

void launch_halfspace_scan(hipStream_t stream, const double* a, int batch, int N, int nh, int* any, int* bad) {
  const size_t items = (size_t)batch * N;
  const dim3 grid((unsigned)((items + HS_SCAN_THREADS - 1) / HS_SCAN_THREADS)), block(HS_SCAN_THREADS);
  hipLaunchKernelGGL(halfspace_scan_kernel, grid, block, 0, stream, a, batch, N, nh, any, bad);
}

}  // namespace admm
