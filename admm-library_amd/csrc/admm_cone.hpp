// admm_cone.hpp -- boundary between the solver runtime and the kernels of handles with one approach cone per stage
// (admm_cone_kernels.hpp).  The kernels take n, m, nh at run time; they are instantiated in admm_cone.hip, a unit
// of its own as admm_halfspace.hip is; the build keeps that unit's resource report and refuses scratch memory in it
// (__graft_entry__.py, NO_SCRATCH_UNITS), and tests/test_cone_host.py checks its sixteen forms and the two read-outs.
#pragma once

#include <hip/hip_runtime.h>

namespace admm {

// the slope of a stage with a cone must be a positive normal number with 1 + g^2 finite: the surface branch divides by the latter
// and by r, which the slope scales.  Host and device.
__host__ __device__ inline bool cone_slope_ok(double g) { return g >= 2.2250738585072014e-308 && fma(g, g, 1.0) < INFINITY; }

struct ConeLaunch {
  hipStream_t stream;
  const double* w;
  double *z, *y;
  const double *lo, *hi;            // [L] box per stacked row
  const double *ub, *kap;           // [N] thrust bound and fuel weight / rho per stage (read by the SOC forms only)
  const double *c, *p, *g;          // axis, apex, slope.  shared: [N][nh], [N][nh], [N]; per QP: [N][nh][pitch], [N][nh][pitch], [N][pitch]
  double* part;
  double alpha;
  int L, zrows, zchunks, pitch, nb, m, nh;
  bool resid, soc, perqp;
};

void launch_cone(const ConeLaunch& l);
// per QP: the largest violation of a cone by w, the stages whose y_xi is not zero, and (lam != NULL) rho |y_xi| as [N][pitch]
void launch_cone_report(hipStream_t stream, const double* w, const double* y, const double* c, const double* p, const double* g,
                        double* max_violation, int* n_active, double* lam, double rho, int N, int nb, int m, int nh, int pitch,
                        int batch, bool perqp);
// c, g: a caller's (batch, N, nh) and (batch, N) device arrays; flags: [3][N] ints, zeroed by the caller -- some QP has a cone at
// the stage | some c'c there is not a normal number | some slope of a stage with a cone is unusable
void launch_cone_scan(hipStream_t stream, const double* c, const double* g, int batch, int N, int nh, int* flags);

}  // namespace admm
