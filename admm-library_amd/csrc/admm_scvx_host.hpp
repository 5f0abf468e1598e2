// admm_scvx_host.hpp -- host side shared by the units that instantiate the SCvx kernels for a model (admm_scvx.hip: the shipped
// model and the admm_scvx_*_device entry points; admm_scvx_models.hip: the CR3BP and the admm_scvx_*_model_device entry points;
// admm_scvx_stage.hip: the models that read per-node data and the admm_scvx_*_stage_device entry points).  Argument checks, the Arg tables, enter_device, the per-device counter and the launch code, once.
// Every check -- arguments first, without a HIP call; then the pointers -- comes before the first launch.  An entry point checks
// its own model struct, builds the device-side model M (admm_scvx_kernels.hpp) and calls scvx_<call><M>.
#pragma once

#include "admm_runtime.hpp"
#include "admm_scvx_kernels.hpp"

#include <mutex>

namespace admm {
namespace scvx_host {

using namespace admm::rt;

constexpr int MAX_DEVICES = 64;
// the counter advance adds to and its pinned landing place, per device, allocated on first use and kept; one advance per device at
// a time (the mutex is held until the count has reached the host).  One instance for the library (C++17 inline variable)
struct Counter { int* dev = nullptr; int* host = nullptr; std::mutex mu; };
inline Counter g_counter[MAX_DEVICES];

inline int bad(const char* fn, const std::string& what) { return fail(ADMM_ERR_INVALID, std::string(fn) + ": " + what); }

// N, batch, substeps, dt of a model struct; `prefix` names the struct ("model." | "dynamics.")
inline int check_grid(const char* fn, const char* prefix, int N, int batch, int substeps, double dt) {
  const std::string p(prefix);
  if (N < 1) return bad(fn, p + "N must be >= 1");
  if (batch < 1) return bad(fn, p + "batch must be >= 1");
  if (substeps < 1) return bad(fn, p + "substeps must be >= 1");
  if (!std::isfinite(dt) || dt <= 0.0) return bad(fn, p + "dt must be finite and positive");
  return ADMM_OK;
}

inline void fill_grid(ScvxGrid& g, int N, int batch, int substeps, double dt) {
  g.N = N; g.batch = batch; g.substeps = substeps;
  g.h = dt / substeps;
  g.hh = 0.5 * g.h;
  g.h6 = g.h / 6.0;
}

inline ScvxRelativeCircular relative_circular(int N, int batch, int substeps, double dt, double rc) {
  ScvxRelativeCircular d{};
  fill_grid(d, N, batch, substeps, dt);
  d.rc = rc;
  d.rc3 = std::pow(rc, 3.0);
  return d;
}

inline int check_params(const char* fn, const admm_scvx_params* p) {
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

inline int check_null(const char* fn, const Arg* a, int count) {
  for (int i = 0; i < count; ++i)
    if (!a[i].ptr) return bad(fn, std::string(a[i].name) + " is NULL");
  return ADMM_OK;
}

inline int check_device(const char* fn, int device, const Arg* a, int count) {
  for (int i = 0; i < count; ++i) {
    const int rc = a[i].is_int ? check_device_ptr(device, a[i].ptr, a[i].count * sizeof(int32_t), fn, a[i].name, sizeof(int32_t), "int32 entries")
                               : check_device_ptr(device, a[i].ptr, a[i].count * sizeof(double), fn, a[i].name);
    if (rc) return rc;
  }
  return ADMM_OK;
}

// the arrays of an admm_scvx_state, by the names of its fields
inline int state_args(const ScvxGrid& g, const admm_scvx_state* s, Arg* a) {
  const size_t B = g.batch, N = g.N;
  const Arg all[13] = {{s->ub, B * N * 3, "state.ub", false}, {s->xb, B * N * 6, "state.xb", false},
                       {s->u_cand, B * N * 3, "state.u_cand", false}, {s->x_cand, B * N * 6, "state.x_cand", false},
                       {s->J, B, "state.J", false}, {s->tr_u, B, "state.tr_u", false}, {s->tr_x, B, "state.tr_x", false},
                       {s->active, B, "state.active", true}, {s->converged, B, "state.converged", true},
                       {s->accepted, B, "state.accepted", true}, {s->outer, B, "state.outer", true}, {s->take, B, "state.take", true},
                       {s->history, (size_t)std::max(s->history_capacity, 0) * B * admm::SCVX_HIST, "state.history", false}};
  for (int i = 0; i < 13; ++i) a[i] = all[i];
  return 13;
}

inline int enter_device(const char* fn, int device) {
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

// a model that reads per-node data (admm::ScvxTakesNodes): its table joins the call's arrays, checked like them.
// The entry point has checked that the pointer is not NULL and that the table has 2 substeps N + 1 rows.  Returns the new count
template <class M>
int node_args(const M& md, Arg* a, int count) {
  if constexpr (admm::ScvxTakesNodes<M>::value)
    a[count++] = Arg{md.nodes, ((size_t)2 * md.substeps * md.N + 1) * M::NODE_PAR, "nodes", false};
  return count;
}

inline unsigned waves_of(int batch) { return (unsigned)((batch + admm::SCVX_THREADS - 1) / admm::SCVX_THREADS); }

// scvx_commit_kernel on stream s (it has no model; defined in admm_scvx.hip)
int scvx_commit(hipStream_t s, int N, int batch, const admm_scvx_state* state);

// ---- the four calls for a device-side model md whose own struct the entry point has checked.  Function templates: each is
// instantiated in the unit that owns the model (explicitly, below for the shipped one), and the kernels with it
template <class M>
int scvx_rollout(const char* fn, int device, const M& md, const double* x0, const double* u, double* x, void* hip_stream) {
  int rc;
  const size_t B = md.batch, N = md.N;
  Arg args[4] = {{x0, B * 6, "x0", false}, {u, B * N * 3, "u", false}, {x, B * N * 6, "x", false}};
  const int na = node_args(md, args, 3);
  if ((rc = check_null(fn, args, na)) || (rc = enter_device(fn, device)) || (rc = check_device(fn, device, args, na))) return rc;
  hipLaunchKernelGGL((admm::scvx_rollout_kernel<M, false>), dim3(waves_of(md.batch)), dim3(admm::SCVX_THREADS), 0,
                     static_cast<hipStream_t>(hip_stream), md, admm_scvx_params{}, x0, u, x, admm::ScvxInit{});
  HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

template <class M>
int scvx_init(const char* fn, int device, const M& md, const admm_scvx_params* params, const double* x0, admm_scvx_state* state,
              double tr_u, double tr_x, void* hip_stream) {
  int rc;
  if ((rc = check_params(fn, params))) return rc;
  if (!state) return bad(fn, "state is NULL");
  if (!std::isfinite(tr_u) || tr_u < 0.0) return bad(fn, "tr_u must be finite and >= 0");
  if (!std::isfinite(tr_x) || tr_x < 0.0) return bad(fn, "tr_x must be finite and >= 0");
  if (state->history_capacity < 1) return bad(fn, "state.history_capacity must be >= 1");
  Arg args[15];
  const int ns = state_args(md, state, args);
  args[ns] = Arg{x0, (size_t)md.batch * 6, "x0", false};
  const int na = node_args(md, args, ns + 1);
  if ((rc = check_null(fn, args, na)) || (rc = enter_device(fn, device)) || (rc = check_device(fn, device, args, na))) return rc;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  HIP_TRY(hipMemsetAsync(state->ub, 0, sizeof(double) * (size_t)md.batch * md.N * 3, s));
  const admm::ScvxInit in{state->J, state->tr_u, state->tr_x, state->active, state->converged, state->accepted, state->outer,
                          state->take, tr_u, tr_x};
  hipLaunchKernelGGL((admm::scvx_rollout_kernel<M, true>), dim3(waves_of(md.batch)), dim3(admm::SCVX_THREADS), 0, s, md, *params, x0,
                     state->ub, state->xb, in);
  HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

template <class M>
int scvx_prepare(const char* fn, int device, const M& md, const admm_scvx_params* params, const double* x0, const admm_scvx_state* state,
                 double* A, double* B, double* lo, double* hi, double* q, void* hip_stream) {
  int rc;
  if ((rc = check_params(fn, params))) return rc;
  if (!state) return bad(fn, "state is NULL");
  const size_t Bn = md.batch, N = md.N;
  Arg args[12] = {{x0, Bn * 6, "x0", false}, {state->ub, Bn * N * 3, "state.ub", false}, {state->xb, Bn * N * 6, "state.xb", false},
                      {state->tr_u, Bn, "state.tr_u", false}, {state->tr_x, Bn, "state.tr_x", false}, {state->active, Bn, "state.active", true},
                      {A, Bn * N * 36, "A", false}, {B, Bn * N * 18, "B", false}, {lo, Bn * N * 9, "lo", false},
                      {hi, Bn * N * 9, "hi", false}, {q, Bn * N * 9, "q", false}};
  const int na = node_args(md, args, 11);
  if ((rc = check_null(fn, args, na)) || (rc = enter_device(fn, device)) || (rc = check_device(fn, device, args, na))) return rc;
  const size_t blocks = (Bn * N + admm::SCVX_THREADS - 1) / admm::SCVX_THREADS;
  if (blocks > 0x7fffffffu) return bad(fn, "batch * N is too large");
  hipLaunchKernelGGL((admm::scvx_linearise_kernel<M>), dim3((unsigned)blocks), dim3(admm::SCVX_THREADS), 0, static_cast<hipStream_t>(hip_stream),
                     md, *params, x0, state->ub, state->xb, state->tr_u, state->tr_x, state->active, A, B, lo, hi, q);
  HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

template <class M>
int scvx_advance(const char* fn, int device, const M& md, const admm_scvx_params* params, const double* x0, const double* z,
                 admm_scvx_state* state, int32_t* n_active, void* hip_stream) {
  int rc;
  if ((rc = check_params(fn, params))) return rc;
  if (!state) return bad(fn, "state is NULL");
  if (!n_active) return bad(fn, "n_active is NULL");
  if (state->history_capacity < 1) return bad(fn, "state.history_capacity must be >= 1");
  const size_t Bn = md.batch, N = md.N;
  Arg args[16];
  const int ns = state_args(md, state, args);
  args[ns] = Arg{x0, Bn * 6, "x0", false};
  args[ns + 1] = Arg{z, Bn * N * 9, "z", false};
  const int na = node_args(md, args, ns + 2);
  if ((rc = check_null(fn, args, na)) || (rc = enter_device(fn, device)) || (rc = check_device(fn, device, args, na))) return rc;
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
  hipLaunchKernelGGL((admm::scvx_advance_kernel<M>), dim3(waves_of(md.batch)), dim3(admm::SCVX_THREADS), 0, s, md, *params, x0, z, *state,
                     c.dev);
  HIP_TRY(hipGetLastError());
  if ((rc = scvx_commit(s, md.N, md.batch, state))) return rc;
  HIP_TRY(hipMemcpyAsync(c.host, c.dev, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *n_active = *c.host;
  return ADMM_OK;
}

// the shipped model's four are instantiated in admm_scvx.hip alone (its kernels with them); admm_scvx_models.hip calls them for
// kind ADMM_SCVX_RELATIVE_CIRCULAR
extern template int scvx_rollout<ScvxRelativeCircular>(const char*, int, const ScvxRelativeCircular&, const double*, const double*, double*, void*);
extern template int scvx_init<ScvxRelativeCircular>(const char*, int, const ScvxRelativeCircular&, const admm_scvx_params*, const double*,
                                                    admm_scvx_state*, double, double, void*);
extern template int scvx_prepare<ScvxRelativeCircular>(const char*, int, const ScvxRelativeCircular&, const admm_scvx_params*, const double*,
                                                       const admm_scvx_state*, double*, double*, double*, double*, double*, void*);
extern template int scvx_advance<ScvxRelativeCircular>(const char*, int, const ScvxRelativeCircular&, const admm_scvx_params*, const double*,
                                                       const double*, admm_scvx_state*, int32_t*, void*);

}  // namespace scvx_host
}  // namespace admm
