// admm_scvx_stage.hip -- time-dependent models of the device SCvx outer step (ADMM_HIP_HAS_SCVX_STAGE_MODELS):
// the admm_scvx_*_stage_device entry points, which take an admm_scvx_stage_dynamics -- a kind, its parameters and a table of
// ADMM_SCVX_NODE_PAR doubles per RK4 node of the horizon in GPU memory, shared by the batch --, and the kernels of
// ScvxRelativeTabulated (admm_scvx_kernels.hpp), instantiated here and nowhere else.  The library computes no epoch: all time
// dependence is in the table.  Checks, Arg tables, the counter and the launch code: admm_scvx_host.hpp.
#include "admm_scvx_host.hpp"

using namespace admm::scvx_host;

namespace {

constexpr int NPAR = 4;

int check_stage_dynamics(const char* fn, const admm_scvx_stage_dynamics* d) {
  if (!d) return bad(fn, "dynamics is NULL");
  if (int rc = check_grid(fn, "dynamics.", d->N, d->batch, d->substeps, d->dt)) return rc;
  if (d->kind != ADMM_SCVX_STAGE_RELATIVE_TABULATED) return bad(fn, "dynamics.kind " + std::to_string(d->kind) + " is not a known model");
  if (d->reserved != 0) return bad(fn, "dynamics.reserved must be 0");
  if (!std::isfinite(d->par[0]) || d->par[0] <= 0.0) return bad(fn, "dynamics.par[0] (mu) must be finite and positive");
  for (int i = 1; i < NPAR; ++i)
    if (!(d->par[i] == 0.0)) return bad(fn, "dynamics.par[" + std::to_string(i) + "] is not used by this kind and must be 0");
  if (!d->nodes) return bad(fn, "dynamics.nodes is NULL");
  const int64_t want = (int64_t)2 * d->substeps * d->N + 1;
  if (d->n_nodes != want)
    return bad(fn, "dynamics.n_nodes is " + std::to_string(d->n_nodes) + ", expected 2 substeps N + 1 = " + std::to_string(want));
  return ADMM_OK;
}

admm::ScvxRelativeTabulated tabulated_of(const admm_scvx_stage_dynamics* d) {
  admm::ScvxRelativeTabulated m{};
  fill_grid(m, d->N, d->batch, d->substeps, d->dt);
  m.mu = d->par[0];
  m.nodes = d->nodes;
  return m;
}

}  // namespace

extern "C" {

const char* admm_scvx_stage_model_name(int32_t kind) {
  return kind == ADMM_SCVX_STAGE_RELATIVE_TABULATED ? "relative_tabulated" : nullptr;
}

int admm_scvx_rollout_stage_device(int32_t device, const admm_scvx_stage_dynamics* dynamics, const double* x0, const double* u, double* x,
                                   void* hip_stream) {
  const char* fn = "admm_scvx_rollout_stage_device";
  if (int rc = check_stage_dynamics(fn, dynamics)) return rc;
  return scvx_rollout(fn, device, tabulated_of(dynamics), x0, u, x, hip_stream);
}

int admm_scvx_init_stage_device(int32_t device, const admm_scvx_stage_dynamics* dynamics, const admm_scvx_params* params, const double* x0,
                                admm_scvx_state* state, double tr_u, double tr_x, void* hip_stream) {
  const char* fn = "admm_scvx_init_stage_device";
  if (int rc = check_stage_dynamics(fn, dynamics)) return rc;
  return scvx_init(fn, device, tabulated_of(dynamics), params, x0, state, tr_u, tr_x, hip_stream);
}

int admm_scvx_prepare_stage_device(int32_t device, const admm_scvx_stage_dynamics* dynamics, const admm_scvx_params* params, const double* x0,
                                   const admm_scvx_state* state, double* A, double* B, double* lo, double* hi, double* q,
                                   void* hip_stream) {
  const char* fn = "admm_scvx_prepare_stage_device";
  if (int rc = check_stage_dynamics(fn, dynamics)) return rc;
  return scvx_prepare(fn, device, tabulated_of(dynamics), params, x0, state, A, B, lo, hi, q, hip_stream);
}

int admm_scvx_advance_stage_device(int32_t device, const admm_scvx_stage_dynamics* dynamics, const admm_scvx_params* params, const double* x0,
                                   const double* z, admm_scvx_state* state, int32_t* n_active, void* hip_stream) {
  const char* fn = "admm_scvx_advance_stage_device";
  if (int rc = check_stage_dynamics(fn, dynamics)) return rc;
  return scvx_advance(fn, device, tabulated_of(dynamics), params, x0, z, state, n_active, hip_stream);
}

}  // extern "C"
