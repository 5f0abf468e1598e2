// admm_consensus.hip -- solver runtime: the z-update kernel of scenario-consensus handles and its launch geometry (admm_consensus.hpp,
// DESIGN.md §2.12).  The kernel takes n, m and G at run time: four forms for every shape, compiled here once.
#include "admm_consensus.hpp"
#include "admm_consensus_kernels.hpp"
#include "admm_select.hpp"

namespace admm {

bool consensus_wide(int G, int m) { return G > consensus_tile(m); }

int consensus_col_groups(int batch, int G, int m) {
  const int T = consensus_tile(m);
  const int ngroups = batch / G;
  if (G > T) return ngroups;
  const int gpw = T / G;
  return (ngroups + gpw - 1) / gpw;
}

void launch_consensus(const ConsLaunch& l) {
  const dim3 grid(consensus_col_groups(l.batch, l.G, l.m), l.zchunks), block(Z_THREADS);
  const bool relax = l.alpha != 1.0;
  // LDS: zbar and the upper tree levels, then m rows of sums -- and, G <= T, of v, and of w and the old z with residuals
  // (m <= CONS_MAX_M: admm_setup_consensus refuses more)
  const size_t lds = consensus_lds_bytes(l.m, l.G, l.resid);
  with_flags([&](auto RS, auto RX) {
    hipLaunchKernelGGL((zdual_consensus_kernel<RS(), RX()>), grid, block, lds, l.stream, l.w, l.z, l.y, l.lo, l.hi, l.ub, l.kap,
                       l.part, l.alpha, l.L, l.zrows, l.pitch, l.nb, l.m, l.G, l.batch);
  }, l.resid, relax);
}

}  // namespace admm
