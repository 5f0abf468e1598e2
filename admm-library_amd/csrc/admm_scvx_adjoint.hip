// admm_scvx_adjoint.hip -- host side of admm_scvx_adjoint_device (ADMM_HIP_HAS_SCVX_ADJOINT; the kernel:
// admm_scvx_adjoint_kernels.hpp).  No handle, no model: one launch on the caller's stream, no host synchronisation; every check --
// arguments first, without a HIP call; then the pointers -- comes before the launch (shared code: admm_scvx_host.hpp).
#include "admm_scvx_host.hpp"
#include "admm_scvx_adjoint_kernels.hpp"

using namespace admm::scvx_host;

extern "C" int admm_scvx_adjoint_device(int32_t device, int32_t N, int32_t batch, const admm_scvx_params* params, const double* ub,
                                        const double* A, const double* B, const double* q, const admm_scvx_adjoint_out* out,
                                        void* hip_stream) {
  const char* fn = "admm_scvx_adjoint_device";
  int rc;
  if (N < 1) return bad(fn, "N must be >= 1");
  if (batch < 1) return bad(fn, "batch must be >= 1");
  if (N > admm::SCVX_ADJ_MAX_N) return bad(fn, "N must be <= " + std::to_string(admm::SCVX_ADJ_MAX_N));
  if (!params) return bad(fn, "params is NULL");
  const size_t Bn = batch, Nn = N;
  const Arg in[4] = {{ub, Bn * Nn * 3, "ub", false}, {A, Bn * Nn * 36, "A", false}, {B, Bn * Nn * 18, "B", false}, {q, Bn * Nn * 9, "q", false}};
  if ((rc = check_null(fn, in, 4))) return rc;
  if (!out) return bad(fn, "out is NULL");
  const Arg all[6] = {{out->nu, Bn * Nn * 6, "out.nu", false}, {out->primer, Bn * Nn * 3, "out.primer", false},
                      {out->grad, Bn * Nn * 3, "out.grad", false}, {out->dJdx0, Bn * 6, "out.dJdx0", false},
                      {out->stat, Bn, "out.stat", false}, {out->n_bound, Bn, "out.n_bound", true}};
  Arg given[6];
  int ng = 0;
  for (int i = 0; i < 6; ++i)
    if (all[i].ptr) given[ng++] = all[i];
  if (ng == 0) return bad(fn, "every field of out is NULL");
  if ((rc = enter_device(fn, device)) || (rc = check_device(fn, device, in, 4)) || (rc = check_device(fn, device, given, ng))) return rc;
  admm::ScvxBox box;
  for (int i = 0; i < 3; ++i) { box.lo[i] = params->u_lo[i]; box.hi[i] = params->u_hi[i]; }
  hipLaunchKernelGGL(admm::scvx_adjoint_kernel, dim3(waves_of(batch)), dim3(admm::SCVX_THREADS), 0, static_cast<hipStream_t>(hip_stream),
                     N, batch, box, ub, A, B, q, *out);
  HIP_TRY(hipGetLastError());
  return ADMM_OK;
}
