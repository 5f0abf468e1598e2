// admm_scvx.hip -- host side of the device outer step of the batched successive-convexification loop (ADMM_HIP_HAS_SCVX;
// DESIGN.md §2.8.1; kernels: admm_scvx_kernels.hpp) for the shipped model, the one instance of the model interface (§2.8.2) that is
// instantiated here.  The entry points take no handle: every launch goes onto the caller's stream, and every check -- arguments
// first, without a HIP call; then the pointers -- comes before the first launch (shared code: admm_scvx_host.hpp).
#include "admm_scvx_host.hpp"

namespace admm {

// candidate -> reference for the trajectories the decision accepted (u: B N 3 elements, then x: B N 6).  It has no
// model, so it is defined here, once for the library, and launched through scvx_host::scvx_commit
__global__ __launch_bounds__(256) void scvx_commit_kernel(int N, size_t nu_total, size_t total, const int32_t* __restrict__ take,
                                                          const double* __restrict__ u_cand, const double* __restrict__ x_cand,
                                                          double* __restrict__ ub, double* __restrict__ xb) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    if (e < nu_total) {
      if (take[e / ((size_t)N * 3)]) ub[e] = u_cand[e];
    } else {
      const size_t f = e - nu_total;
      if (take[f / ((size_t)N * 6)]) xb[f] = x_cand[f];
    }
  }
}

namespace scvx_host {

int scvx_commit(hipStream_t s, int N, int batch, const admm_scvx_state* state) {
  const size_t nu_total = (size_t)batch * N * 3, total = (size_t)batch * N * 9;
  const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 8192);
  hipLaunchKernelGGL(admm::scvx_commit_kernel, dim3(blocks), dim3(256), 0, s, N, nu_total, total, state->take, state->u_cand,
                     state->x_cand, state->ub, state->xb);
  HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

template int scvx_rollout<ScvxRelativeCircular>(const char*, int, const ScvxRelativeCircular&, const double*, const double*, double*, void*);
template int scvx_init<ScvxRelativeCircular>(const char*, int, const ScvxRelativeCircular&, const admm_scvx_params*, const double*,
                                             admm_scvx_state*, double, double, void*);
template int scvx_prepare<ScvxRelativeCircular>(const char*, int, const ScvxRelativeCircular&, const admm_scvx_params*, const double*,
                                                const admm_scvx_state*, double*, double*, double*, double*, double*, void*);
template int scvx_advance<ScvxRelativeCircular>(const char*, int, const ScvxRelativeCircular&, const admm_scvx_params*, const double*,
                                                const double*, admm_scvx_state*, int32_t*, void*);

}  // namespace scvx_host
}  // namespace admm

using namespace admm::scvx_host;

namespace {

int check_model(const char* fn, const admm_scvx_model* m) {
  if (!m) return bad(fn, "model is NULL");
  if (int rc = check_grid(fn, "model.", m->N, m->batch, m->substeps, m->dt)) return rc;
  if (!std::isfinite(m->rc) || m->rc <= 0.0) return bad(fn, "model.rc must be finite and positive");
  return ADMM_OK;
}

admm::ScvxRelativeCircular device_model(const admm_scvx_model* m) { return relative_circular(m->N, m->batch, m->substeps, m->dt, m->rc); }

}  // namespace

extern "C" {

int admm_scvx_rollout_device(int32_t device, const admm_scvx_model* model, const double* x0, const double* u, double* x,
                             void* hip_stream) {
  const char* fn = "admm_scvx_rollout_device";
  if (int rc = check_model(fn, model)) return rc;
  return scvx_rollout(fn, device, device_model(model), x0, u, x, hip_stream);
}

int admm_scvx_init_device(int32_t device, const admm_scvx_model* model, const admm_scvx_params* params, const double* x0,
                          admm_scvx_state* state, double tr_u, double tr_x, void* hip_stream) {
  const char* fn = "admm_scvx_init_device";
  if (int rc = check_model(fn, model)) return rc;
  return scvx_init(fn, device, device_model(model), params, x0, state, tr_u, tr_x, hip_stream);
}

int admm_scvx_prepare_device(int32_t device, const admm_scvx_model* model, const admm_scvx_params* params, const double* x0,
                             const admm_scvx_state* state, double* A, double* B, double* lo, double* hi, double* q, void* hip_stream) {
  const char* fn = "admm_scvx_prepare_device";
  if (int rc = check_model(fn, model)) return rc;
  return scvx_prepare(fn, device, device_model(model), params, x0, state, A, B, lo, hi, q, hip_stream);
}

int admm_scvx_advance_device(int32_t device, const admm_scvx_model* model, const admm_scvx_params* params, const double* x0,
                             const double* z, admm_scvx_state* state, int32_t* n_active, void* hip_stream) {
  const char* fn = "admm_scvx_advance_device";
  if (int rc = check_model(fn, model)) return rc;
  return scvx_advance(fn, device, device_model(model), params, x0, z, state, n_active, hip_stream);
}

}  // extern "C"
