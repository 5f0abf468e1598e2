// admm_halfspace.hpp -- boundary between the solver runtime and the kernels of handles with one half-space per stage
// (admm_halfspace_kernels.hpp).  The kernels take n, m, nh at run time; they are instantiated in
// admm_halfspace.hip, a unit of its own as admm_soft.hip is; the build keeps that unit's resource report and refuses scratch memory
// in it (__graft_entry__.py, NO_SCRATCH_UNITS), and tests/test_halfspace_host.py checks its sixteen forms and the two read-outs.
#pragma once

#include <hip/hip_runtime.h>

namespace admm {

// a'a of a stage with a plane must be a normal number: the projection divides by it (an underflowed or overflowed sum of squares of
// finite entries is refused at set-up: scale the row).  Host and device.
__host__ __device__ inline bool halfspace_norm_ok(double nn) { return nn >= 2.2250738585072014e-308 && nn < INFINITY; }

struct HalfspaceLaunch {
  hipStream_t stream;
  const double* w;
  double *z, *y;
  const double *lo, *hi;            // [L] box per stacked row
  const double *ub, *kap;           // [N] thrust bound and fuel weight / rho per stage (read by the SOC forms only)
  const double *a, *b;              // shared: [N][nh], [N]; per QP: [N][nh][pitch], [N][pitch]
  double* part;
  double alpha;
  int L, zrows, zchunks, pitch, nb, m, nh;
  bool resid, soc, perqp;
};

void launch_halfspace(const HalfspaceLaunch& l);
// per QP: the largest violation of a plane by w, the stages with a positive multiplier, and (lam != NULL) the multipliers [N][pitch]
void launch_halfspace_report(hipStream_t stream, const double* w, const double* y, const double* a, const double* b,
                             double* max_violation, int* n_active, double* lam, double rho, int N, int nb, int m, int nh, int pitch,
                             int batch, bool perqp);
// a: a caller's (batch, N, nh) device array; any, bad: [N] ints, zeroed by the caller
void launch_halfspace_scan(hipStream_t stream, const double* a, int batch, int N, int nh, int* any, int* bad);

}  // namespace admm
