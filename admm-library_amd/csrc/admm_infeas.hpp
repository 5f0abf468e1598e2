// admm_infeas.hpp -- boundary between the solver runtime and the infeasibility kernels (admm_infeas_kernels.hpp):
// a Farkas certificate of every QP from the drift of the scaled dual over a span of iterations.
#pragma once

#include <hip/hip_runtime.h>

namespace admm {

struct InfeasLaunch {
  hipStream_t stream;
  int n, m, N, S, pitch;
  double span, eps;               // lambda = (y - y0) / span; threshold of the open rule and of the flag
  const double *y, *y0, *x0;      // scaled dual now and at the snapshot, batch-minor ([L][pitch]); x0 ([n][pitch])
  const double* AB;               // [N][n n + n m]: A_k then B_k, both column-major (the certificate's copy, CertLaunch::AB)
  const double* Phi;              // [S][n n] row-major (the certificate's copy, CertLaunch::Phi)
  const double* bnd;              // [N][2 nb + 1]: lo, hi of block k = (u_k, x_{k+1}), then the thrust bound (inf = off)
  const int* seg_start;           // [S + 1], device
  double* cseg;                   // [S][n][pitch] pass A: carry a segment hands to its predecessor with zero inflow
  double* cin;                    // [S][n][pitch] link: true inflow of every segment
  double* part;                   // [S][5][pitch] pass B: sigma (segment 0: + x0'c), max |mu|, open, max |mu - lambda|, max |lambda|
  double* out;                    // [5][pitch] sep, drift, defect, infeasible (0 / 1), max |mu|
  double* nu;                     // [N n][pitch] ray costates nu_1 .. nu_N, batch-minor, or NULL
};

// true if (n, m) is compiled (and, unless query_only, pass A, link, pass B and finalise were enqueued on l.stream).  The kernels
// (admm_infeas_kernels.hpp) are instantiated beside the certificate's, group by group (admm_dims_g*.hip).
bool launch_infeas(const InfeasLaunch& l, bool query_only);
bool launch_infeas_group0(const InfeasLaunch& l, bool query_only);
bool launch_infeas_group1(const InfeasLaunch& l, bool query_only);
bool launch_infeas_group2(const InfeasLaunch& l, bool query_only);
bool launch_infeas_group3(const InfeasLaunch& l, bool query_only);

// the flag row of InfeasLaunch::out as int32 (read-out)
void launch_infeas_flags(hipStream_t stream, const double* flag_row, int* dst, int count);

}  // namespace admm
