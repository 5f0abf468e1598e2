// admm_consensus.hpp -- boundary between the solver runtime and the z-update kernel of scenario-consensus handles
// (admm_consensus_kernels.hpp).  The kernel takes n, m and G at run time; it is instantiated in
// admm_consensus.hip, a unit of its own as admm_mpc.hip is; the build keeps that unit's resource report and refuses scratch
// memory in it (__graft_entry__.py, NO_SCRATCH_UNITS), and tests/test_consensus_host.py checks its four forms.
#pragma once

#include <hip/hip_runtime.h>

namespace admm {

constexpr int CONS_MAX_M = 6;      // control rows the kernel's LDS arrays are sized for: the widest compiled shape, (12, 6)

struct ConsLaunch {
  hipStream_t stream;
  const double* w;
  double *z, *y;
  const double *lo, *hi, *ub, *kap;
  double* part;
  double alpha;
  int L, zrows, zchunks, pitch, nb, m, G, batch;
  bool resid;
};

// workgroups along the batch: whole groups each (floor(tile / G) of them, or one group wider than the tile)
int consensus_col_groups(int batch, int G, int m);
bool consensus_wide(int G, int m);      // a group wider than a workgroup's tile: the two-pass route
void launch_consensus(const ConsLaunch& l);
// read-out (admm_launch.hip): out (ngroups, N, m) = the control rows of z at each group's first column
void launch_consensus_gather(hipStream_t stream, const double* z, double* out, int ngroups, int G, int N, int nb, int m, int pitch);

}  // namespace admm
