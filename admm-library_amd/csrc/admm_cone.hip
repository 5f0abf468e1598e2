// admm_cone.hip -- solver runtime: the z-update kernel of handles with one approach cone per stage, its read-out, the device-side
// scan of per-QP cones, and their launch geometry (admm_cone.hpp).  The kernels take n, m and nh at run time:
// sixteen forms for every shape, compiled here once.
#include "admm_cone.hpp"
#include "admm_cone_kernels.hpp"
#include "admm_select.hpp"

namespace admm {

void launch_cone(const ConeLaunch& l) {
  const dim3 grid((l.pitch / 2 + Z_THREADS - 1) / Z_THREADS, l.zchunks), block(Z_THREADS);
  const bool relax = l.alpha != 1.0;
  with_flags([&](auto RS, auto RX, auto SOC, auto PQ) {
    hipLaunchKernelGGL((zdual_cone_kernel<RS(), RX(), SOC(), PQ()>), grid, block, 0, l.stream, l.w, l.z, l.y, l.lo, l.hi, l.ub, l.kap,
                       l.c, l.p, l.g, l.part, l.alpha, l.L, l.zrows, l.pitch, l.nb, l.m, l.nh);
  }, l.resid, relax, l.soc, l.perqp);
}

void launch_cone_report(hipStream_t stream, const double* w, const double* y, const double* c, const double* p, const double* g,
                        double* max_violation, int* n_active, double* lam, double rho, int N, int nb, int m, int nh, int pitch,
                        int batch, bool perqp) {
  const dim3 grid((batch + CONE_REPORT_THREADS - 1) / CONE_REPORT_THREADS), block(CONE_REPORT_THREADS);
  hipLaunchKernelGGL(cone_report_kernel, grid, block, 0, stream, w, y, c, p, g, max_violation, n_active, lam, rho, N, nb, m, nh, pitch,
                     batch, perqp ? 1 : 0);
}

void launch_cone_scan(hipStream_t stream, const double* c, const double* g, int batch, int N, int nh, int* flags) {
  const size_t items = (size_t)batch * N;
  const dim3 grid((unsigned)((items + CONE_SCAN_THREADS - 1) / CONE_SCAN_THREADS)), block(CONE_SCAN_THREADS);
  hipLaunchKernelGGL(cone_scan_kernel, grid, block, 0, stream, c, g, batch, N, nh, flags, flags + N, flags + 2 * (size_t)N);
}

}  // namespace admm
