// admm_scvx.hip -- host side of the device outer step of the batched successive-convexification loop (ADMM_HIP_HAS_SCVX;
// DESIGN.md §2.8.1; kernels: admm_scvx_kernels.hpp).  The entry points take no handle: every launch goes onto the caller's stream,
// and every check -- arguments first, without a HIP call; then the pointers -- comes before the first launch.
#include "admm_runtime.hpp"
#include "admm_scvx_kernels.hpp"

#include <mutex>

using namespace admm::rt;

namespace {

constexpr int MAX_DEVICES = 64;
// the counter advance adds to and its pinned landing place, per device, allocated on first use and kept; one advance per device at
// a time (the mutex is held until the count has reached the host)
struct Counter { int* dev = nullptr; int* host = nullptr; std::mutex mu; };
Counter g_counter[MAX_DEVICES];

int bad(const char* fn, const std::string& what) { return fail(ADMM_ERR_INVALID, std::string(fn) + ": " + what); }

int check_model(const char* fn, const admm_scvx_model* m) {
  if (!m) return bad(fn, "model is NULL");
  if (m->N < 1) return bad(fn, "model.N must be >= 1");
  if (m->batch < 1) return bad(fn, "model.batch must be >= 1");
  if (m->substeps < 1) return bad(fn, "model.substeps must be >= 1");
  if (!std::isfinite(m->dt) || m->dt <= 0.0) return bad(fn, "model.dt must be finite and positive");
  if (!std::isfinite(m->rc) || m->rc <= 0.0) return bad(fn, "model.rc must be finite and positive");
  return ADMM_OK;
}

int check_params(const char* fn, const admm_scvx_params* p) {
  if (!p) return bad(fn, "params is NULL");
  if (!std::isfinite(p->fd_eps) || p->fd_eps <= 0.0) return bad(fn, "params.fd_eps must be finite and positive");
  if (!finite_all(p->Q, 36) || !finite_all(p->R, 9) || !finite_all(p->QN, 36)) return bad(fn, "params: non-finite entry in Q, R or QN");
  for (int i = 0; i < 3; ++i)
    if (std::isnan(p->u_lo[i]) || std::isnan(p->u_hi[i]) || p->u_lo[i] > p->u_hi[i]) return bad(fn, "params: u_lo <= u_hi violated");
  if (!std::isfinite(p->tol) || !std::isfinite(p->rho_reject) || !std::isfinite(p->rho_expand))
    return bad(fn, "params: tol, rho_reject and rho_expand must be finite");
  return ADMM_OK;
}

struct Arg { const void* ptr; size_t count; const char* name; bool is_int; };

int check_null(const char* fn, const Arg* a, int count) {
  for (int i = 0; i < count; ++i)
    if (!a[i].ptr) return bad(fn, std::string(a[i].name) + " is NULL");
  return ADMM_OK;
}

int check_device(const char* fn, int device, const Arg* a, int count) {
  for (int i = 0; i < count; ++i) {
    const int rc = a[i].is_int ? check_device_ptr(device, a[i].ptr, a[i].count * sizeof(int32_t), fn, a[i].name, sizeof(int32_t), "int32 entries")
                               : check_device_ptr(device, a[i].ptr, a[i].count * sizeof(double), fn, a[i].name);
    if (rc) return rc;
  }
  return ADMM_OK;
}

// the arrays of an admm_scvx_state, by the names of its fields
int state_args(const admm_scvx_model* m, const admm_scvx_state* s, Arg* a) {
  const size_t B = m->batch, N = m->N;
  const Arg all[13] = {{s->ub, B * N * 3, "state.ub", false}, {s->xb, B * N * 6, "state.xb", false},
                       {s->u_cand, B * N * 3, "state.u_cand", false}, {s->x_cand, B * N * 6, "state.x_cand", false},
                       {s->J, B, "state.J", false}, {s->tr_u, B, "state.tr_u", false}, {s->tr_x, B, "state.tr_x", false},
                       {s->active, B, "state.active", true}, {s->converged, B, "state.converged", true},
                       {s->accepted, B, "state.accepted", true}, {s->outer, B, "state.outer", true}, {s->take, B, "state.take", true},
                       {s->history, (size_t)std::max(s->history_capacity, 0) * B * admm::SCVX_HIST, "state.history", false}};
  for (int i = 0; i < 13; ++i) a[i] = all[i];
  return 13;
}

admm::ScvxModel device_model(const admm_scvx_model* m) {
  admm::ScvxModel d{};
  d.N = m->N; d.batch = m->batch; d.substeps = m->substeps;
  d.h = m->dt / m->substeps;
  d.hh = 0.5 * d.h;
  d.h6 = d.h / 6.0;
  d.rc = m->rc;
  d.rc3 = std::pow(m->rc, 3.0);
  return d;
}

int enter_device(const char* fn, int device) {
  if (device < 0 || device >= MAX_DEVICES) return bad(fn, "device must be a device ordinal");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 1) {
    (void)hipGetLastError();
    return fail(ADMM_ERR_NO_DEVICE, std::string(fn) + ": no HIP device");
  }
  if (device >= count) return bad(fn, "device must be a device ordinal (" + std::to_string(count) + " visible)");
  HIP_TRY(hipSetDevice(device));
  return ADMM_OK;
}

unsigned waves_of(int batch) { return (unsigned)((batch + admm::SCVX_THREADS - 1) / admm::SCVX_THREADS); }

}  // namespace

extern "C" {

int admm_scvx_rollout_device(int32_t device, const admm_scvx_model* model, const double* x0, const double* u, double* x,
                             void* hip_stream) {
  const char* fn = "admm_scvx_rollout_device";
  int rc;
  if ((rc = check_model(fn, model))) return rc;
  const size_t B = model->batch, N = model->N;
  const Arg args[] = {{x0, B * 6, "x0", false}, {u, B * N * 3, "u", false}, {x, B * N * 6, "x", false}};
  if ((rc = check_null(fn, args, 3)) || (rc = enter_device(fn, device)) || (rc = check_device(fn, device, args, 3))) return rc;
  hipLaunchKernelGGL(admm::scvx_rollout_kernel<false>, dim3(waves_of(model->batch)), dim3(admm::SCVX_THREADS), 0,
                     static_cast<hipStream_t>(hip_stream), device_model(model), admm_scvx_params{}, x0, u, x, admm::ScvxInit{});
  HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

int admm_scvx_init_device(int32_t device, const admm_scvx_model* model, const admm_scvx_params* params, const double* x0,
                          admm_scvx_state* state, double tr_u, double tr_x, void* hip_stream) {
  const char* fn = "admm_scvx_init_device";
  int rc;
  if ((rc = check_model(fn, model)) || (rc = check_params(fn, params))) return rc;
  if (!state) return bad(fn, "state is NULL");
  if (!std::isfinite(tr_u) || tr_u < 0.0) return bad(fn, "tr_u must be finite and >= 0");
  if (!std::isfinite(tr_x) || tr_x < 0.0) return bad(fn, "tr_x must be finite and >= 0");
  if (state->history_capacity < 1) return bad(fn, "state.history_capacity must be >= 1");
  Arg args[14];
  const int ns = state_args(model, state, args);
  args[ns] = Arg{x0, (size_t)model->batch * 6, "x0", false};
  if ((rc = check_null(fn, args, ns + 1)) || (rc = enter_device(fn, device)) || (rc = check_device(fn, device, args, ns + 1))) return rc;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  HIP_TRY(hipMemsetAsync(state->ub, 0, sizeof(double) * (size_t)model->batch * model->N * 3, s));
  const admm::ScvxInit in{state->J, state->tr_u, state->tr_x, state->active, state->converged, state->accepted, state->outer,
                          state->take, tr_u, tr_x};
  hipLaunchKernelGGL(admm::scvx_rollout_kernel<true>, dim3(waves_of(model->batch)), dim3(admm::SCVX_THREADS), 0, s,
                     device_model(model), *params, x0, state->ub, state->xb, in);
  HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

int admm_scvx_prepare_device(int32_t device, const admm_scvx_model* model, const admm_scvx_params* params, const double* x0,
                             const admm_scvx_state* state, double* A, double* B, double* lo, double* hi, double* q, void* hip_stream) {
  const char* fn = "admm_scvx_prepare_device";
  int rc;
  if ((rc = check_model(fn, model)) || (rc = check_params(fn, params))) return rc;
  if (!state) return bad(fn, "state is NULL");
  const size_t Bn = model->batch, N = model->N;
  const Arg args[] = {{x0, Bn * 6, "x0", false}, {state->ub, Bn * N * 3, "state.ub", false}, {state->xb, Bn * N * 6, "state.xb", false},
                      {state->tr_u, Bn, "state.tr_u", false}, {state->tr_x, Bn, "state.tr_x", false}, {state->active, Bn, "state.active", true},
                      {A, Bn * N * 36, "A", false}, {B, Bn * N * 18, "B", false}, {lo, Bn * N * 9, "lo", false},
                      {hi, Bn * N * 9, "hi", false}, {q, Bn * N * 9, "q", false}};
  constexpr int na = sizeof args / sizeof args[0];
  if ((rc = check_null(fn, args, na)) || (rc = enter_device(fn, device)) || (rc = check_device(fn, device, args, na))) return rc;
  const size_t blocks = (Bn * N + admm::SCVX_THREADS - 1) / admm::SCVX_THREADS;
  if (blocks > 0x7fffffffu) return bad(fn, "batch * N is too large");
  hipLaunchKernelGGL(admm::scvx_linearise_kernel, dim3((unsigned)blocks), dim3(admm::SCVX_THREADS), 0, static_cast<hipStream_t>(hip_stream),
                     device_model(model), *params, x0, state->ub, state->xb, state->tr_u, state->tr_x, state->active, A, B, lo, hi, q);
  HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

int admm_scvx_advance_device(int32_t device, const admm_scvx_model* model, const admm_scvx_params* params, const double* x0,
                             const double* z, admm_scvx_state* state, int32_t* n_active, void* hip_stream) {
  const char* fn = "admm_scvx_advance_device";
  int rc;
  if ((rc = check_model(fn, model)) || (rc = check_params(fn, params))) return rc;
  if (!state) return bad(fn, "state is NULL");
  if (!n_active) return bad(fn, "n_active is NULL");
  if (state->history_capacity < 1) return bad(fn, "state.history_capacity must be >= 1");
  const size_t Bn = model->batch, N = model->N;
  Arg args[15];
  const int ns = state_args(model, state, args);
  args[ns] = Arg{x0, Bn * 6, "x0", false};
  args[ns + 1] = Arg{z, Bn * N * 9, "z", false};
  if ((rc = check_null(fn, args, ns + 2)) || (rc = enter_device(fn, device)) || (rc = check_device(fn, device, args, ns + 2))) return rc;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  // every active trajectory writes record outer[b]: it must exist (two small copies; nothing has been launched yet)
  std::vector<int32_t> flags(2 * Bn);
  HIP_TRY(hipMemcpyAsync(flags.data(), state->outer, sizeof(int32_t) * Bn, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(flags.data() + Bn, state->active, sizeof(int32_t) * Bn, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (size_t b = 0; b < Bn; ++b)
    if (flags[Bn + b] && (flags[b] < 0 || flags[b] >= state->history_capacity))
      return bad(fn, "state.history_capacity (" + std::to_string(state->history_capacity) + ") exhausted: trajectory " + std::to_string(b) +
                         " would write record " + std::to_string(flags[b]));
  Counter& c = g_counter[device];
  std::lock_guard<std::mutex> lock(c.mu);
  if (!c.dev && (rc = dalloc(&c.dev, 1))) return rc;
  if (!c.host) HIP_TRY(hipHostMalloc((void**)&c.host, sizeof(int), hipHostMallocDefault));
  HIP_TRY(hipMemsetAsync(c.dev, 0, sizeof(int), s));
  hipLaunchKernelGGL(admm::scvx_advance_kernel, dim3(waves_of(model->batch)), dim3(admm::SCVX_THREADS), 0, s, device_model(model), *params,
                     x0, z, *state, c.dev);
  HIP_TRY(hipGetLastError());
  const size_t nu_total = Bn * N * 3, total = Bn * N * 9;
  const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 8192);
  hipLaunchKernelGGL(admm::scvx_commit_kernel, dim3(blocks), dim3(256), 0, s, model->N, nu_total, total, state->take, state->u_cand,
                     state->x_cand, state->ub, state->xb);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(c.host, c.dev, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *n_active = *c.host;
  return ADMM_OK;
}

}  // extern "C"
