// admm_soft.hpp -- boundary between the solver runtime and the kernels of handles with soft box constraints
// (admm_soft_kernels.hpp).  The kernels take n, m at run time; they are instantiated in admm_soft.hip, a unit of
// its own as admm_consensus.hip is; the build keeps that unit's resource report and refuses scratch memory in it
// (__graft_entry__.py, NO_SCRATCH_UNITS), and tests/test_soft_host.py checks its eight forms and the report kernel.
#pragma once

#include <hip/hip_runtime.h>

namespace admm {

struct SoftLaunch {
  hipStream_t stream;
  const double* w;
  double *z, *y;
  const double *lo, *hi, *skap;     // [L] box and weight / rho per stacked row
  const double *ub, *kap;           // [N] thrust bound and fuel weight / rho per stage (read by the block-structured form only)
  double* part;
  double alpha;
  int L, zrows, zchunks, pitch, nb, m;
  bool resid, soc;
};

void launch_soft(const SoftLaunch& l);
// per QP over the rows with a finite weight: sum s_i dist_i, max dist_i, the number of rows with dist_i > 0
void launch_soft_report(hipStream_t stream, const double* z, const double* lo, const double* hi, const double* soft, double* penalty,
                        double* max_violation, int* n_violated, int L, int pitch, int batch);

}  // namespace admm
