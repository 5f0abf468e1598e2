// admm_scvx_models.hip -- the model interface of the device SCvx outer step (ADMM_HIP_HAS_SCVX_MODELS): the
// admm_scvx_*_model_device entry points, which take an admm_scvx_dynamics (a kind and its parameters), and the kernels of the
// circular restricted three-body problem (ScvxCrtbp, admm_scvx_kernels.hpp), instantiated here.  Kind 0 goes to the shipped
// model's code in admm_scvx.hip.  Checks, Arg tables, the counter and the launch code: admm_scvx_host.hpp.
#include "admm_scvx_host.hpp"

using namespace admm::scvx_host;

namespace {

constexpr int NPAR = 4;

int check_dynamics(const char* fn, const admm_scvx_dynamics* d) {
  if (!d) return bad(fn, "dynamics is NULL");
  if (int rc = check_grid(fn, "dynamics.", d->N, d->batch, d->substeps, d->dt)) return rc;
  int used = 0;
  if (d->kind == ADMM_SCVX_RELATIVE_CIRCULAR) used = 1;
  else if (d->kind == ADMM_SCVX_CRTBP) used = 2;
  else return bad(fn, "dynamics.kind " + std::to_string(d->kind) + " is not a known model");
  if (d->reserved != 0) return bad(fn, "dynamics.reserved must be 0");
  for (int i = used; i < NPAR; ++i)
    if (!(d->par[i] == 0.0)) return bad(fn, "dynamics.par[" + std::to_string(i) + "] is not used by this kind and must be 0");
  if (d->kind == ADMM_SCVX_RELATIVE_CIRCULAR) {
    if (!std::isfinite(d->par[0]) || d->par[0] <= 0.0) return bad(fn, "dynamics.par[0] (rc) must be finite and positive");
  } else {
    if (!std::isfinite(d->par[0]) || d->par[0] <= 0.0 || d->par[0] >= 1.0) return bad(fn, "dynamics.par[0] (mu) must be finite and in (0, 1)");
    if (!std::isfinite(d->par[1])) return bad(fn, "dynamics.par[1] (x_ref) must be finite");
  }
  return ADMM_OK;
}

admm::ScvxRelativeCircular relative_of(const admm_scvx_dynamics* d) { return relative_circular(d->N, d->batch, d->substeps, d->dt, d->par[0]); }

admm::ScvxCrtbp crtbp_of(const admm_scvx_dynamics* d) {
  admm::ScvxCrtbp m{};
  fill_grid(m, d->N, d->batch, d->substeps, d->dt);
  m.mu = d->par[0];
  m.om = 1.0 - d->par[0];
  m.x_ref = d->par[1];
  return m;
}

}  // namespace

extern "C" {

const char* admm_scvx_model_name(int32_t kind) {
  switch (kind) {
    case ADMM_SCVX_RELATIVE_CIRCULAR: return "relative_circular";
    case ADMM_SCVX_CRTBP: return "crtbp";
    default: return nullptr;
  }
}

int admm_scvx_rollout_model_device(int32_t device, const admm_scvx_dynamics* dynamics, const double* x0, const double* u, double* x,
                                   void* hip_stream) {
  const char* fn = "admm_scvx_rollout_model_device";
  if (int rc = check_dynamics(fn, dynamics)) return rc;
  if (dynamics->kind == ADMM_SCVX_CRTBP) return scvx_rollout(fn, device, crtbp_of(dynamics), x0, u, x, hip_stream);
  return scvx_rollout(fn, device, relative_of(dynamics), x0, u, x, hip_stream);
}

int admm_scvx_init_model_device(int32_t device, const admm_scvx_dynamics* dynamics, const admm_scvx_params* params, const double* x0,
                                admm_scvx_state* state, double tr_u, double tr_x, void* hip_stream) {
  const char* fn = "admm_scvx_init_model_device";
  if (int rc = check_dynamics(fn, dynamics)) return rc;
  if (dynamics->kind == ADMM_SCVX_CRTBP) return scvx_init(fn, device, crtbp_of(dynamics), params, x0, state, tr_u, tr_x, hip_stream);
  return scvx_init(fn, device, relative_of(dynamics), params, x0, state, tr_u, tr_x, hip_stream);
}

int admm_scvx_prepare_model_device(int32_t device, const admm_scvx_dynamics* dynamics, const admm_scvx_params* params, const double* x0,
                                   const admm_scvx_state* state, double* A, double* B, double* lo, double* hi, double* q,
                                   void* hip_stream) {
  const char* fn = "admm_scvx_prepare_model_device";
  if (int rc = check_dynamics(fn, dynamics)) return rc;
  if (dynamics->kind == ADMM_SCVX_CRTBP) return scvx_prepare(fn, device, crtbp_of(dynamics), params, x0, state, A, B, lo, hi, q, hip_stream);
  return scvx_prepare(fn, device, relative_of(dynamics), params, x0, state, A, B, lo, hi, q, hip_stream);
}

int admm_scvx_advance_model_device(int32_t device, const admm_scvx_dynamics* dynamics, const admm_scvx_params* params, const double* x0,
                                   const double* z, admm_scvx_state* state, int32_t* n_active, void* hip_stream) {
  const char* fn = "admm_scvx_advance_model_device";
  if (int rc = check_dynamics(fn, dynamics)) return rc;
  if (dynamics->kind == ADMM_SCVX_CRTBP) return scvx_advance(fn, device, crtbp_of(dynamics), params, x0, z, state, n_active, hip_stream);
  return scvx_advance(fn, device, relative_of(dynamics), params, x0, z, state, n_active, hip_stream);
}

}  // extern "C"
