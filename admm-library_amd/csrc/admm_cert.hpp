// admm_cert.hpp -- boundary between the solver runtime and the certificate kernels (admm_cert_kernels.hpp):
// costates of the dynamics, objective, dynamics defect and stationarity defect of every QP at the handle's (z, y) pair.
#pragma once

#include <hip/hip_runtime.h>

namespace admm {

struct CertLaunch {
  hipStream_t stream;
  int n, m, N, S, pitch;
  bool has_q;
  double rho;
  const double *z, *y, *q, *x0;   // batch-minor state ([L][pitch]), linear term (NULL without), x0 ([n][pitch])
  const double* AB;               // [N][n n + n m]: A_k then B_k, both column-major (the caller's arrays, LTI expanded)
  const double* QR;               // Q | QN | R, symmetrised (n n, n n, m m)
  const double* Phi;              // [S][n n] row-major: Phi_s = A_k0' A_k0+1' ... A_k1-1' of segment s = [k0, k1)
  const double* fuel;             // [N] weights of the fuel term (zeros without)
  const int* seg_start;           // [S + 1], device
  double* cseg;                   // [S][n][pitch] pass A: carry a segment hands to its predecessor with zero inflow
  double* cin;                    // [S][n][pitch] link: true inflow of every segment
  double* part;                   // [S][3][pitch] pass B: partial obj, max |defect|, max |stationarity|
  double* out;                    // [3][pitch] obj, feas_dyn, stat
  double* nu;                     // [N n][pitch] costates nu_1 .. nu_N, batch-minor, or NULL
};

// true if (n, m) is compiled (and, unless query_only, pass A, link, pass B and finalise were enqueued on l.stream).  The kernels
// (admm_cert_kernels.hpp) are instantiated beside the one-lane family's, group by group (admm_dims_g*.hip).
bool launch_cert(const CertLaunch& l, bool query_only);
bool launch_cert_group0(const CertLaunch& l, bool query_only);
bool launch_cert_group1(const CertLaunch& l, bool query_only);
bool launch_cert_group2(const CertLaunch& l, bool query_only);
bool launch_cert_group3(const CertLaunch& l, bool query_only);

}  // namespace admm
