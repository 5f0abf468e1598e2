// A stub of the part of the C ABI (include/admm_hip.h) that matlab/admm_mex.cpp calls: no HIP, no arithmetic.  It records what
// it was given, READS every element the header entitles the library to read (so that a sanitizer sees an array that is too
// short), WRITES every element the library may write, with recognisable patterns, and can be told to fail or to leave a warning.
// The warning text follows the library's rule: cleared at the start of setup, update_problem and solve, untouched by the rest.
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "admm_hip.h"

struct admm_handle { int id, N, n, m, batch, frees; };

namespace {

std::vector<admm_handle*> g_handles;          // every handle ever made since stub_reset (kept after admm_free: frees are counted)
std::map<std::string, int> g_calls;
std::map<std::string, double> g_num;          // scalars seen: problem / options fields, sums of the arrays read
std::map<std::string, uint64_t> g_ptr;        // pointers seen
std::map<std::string, std::pair<int, std::string>> g_fail;
std::map<std::string, std::string> g_warn;
std::string g_error, g_warning;
int g_history = 0;

double read_sum(const double* p, size_t count) {
  double s = 0;
  for (size_t i = 0; i < count; ++i) s += p[i];
  return s;
}

void see(const char* name, const double* p, size_t count) {
  g_ptr[name] = reinterpret_cast<uintptr_t>(p);
  g_num[std::string("count_") + name] = p ? static_cast<double>(count) : 0.0;
  g_num[std::string("sum_") + name] = p ? read_sum(p, count) : 0.0;
}

// the sizes of admm_problem's arrays, as the comments of admm_hip.h give them
void see_problem(const admm_problem* p) {
  const size_t N = p->N, n = p->n, m = p->m, batch = p->batch, nb = n + m;
  const size_t stages = p->time_varying == 0 ? 1 : p->time_varying == 1 ? N : N * batch;
  const size_t boxes = p->stage_bounds == 0 ? 1 : p->stage_bounds == 1 ? N : N * batch;
  g_num["N"] = p->N; g_num["n"] = p->n; g_num["m"] = p->m; g_num["batch"] = p->batch;
  g_num["time_varying"] = p->time_varying; g_num["stage_bounds"] = p->stage_bounds;
  see("A", p->A, n * n * stages); see("B", p->B, n * m * stages);
  see("Q", p->Q, n * n); see("R", p->R, m * m); see("QN", p->QN, n * n);
  see("x0", p->x0, n * batch); see("lo", p->lo, nb * boxes); see("hi", p->hi, nb * boxes);
  see("q", p->q, N * nb * batch);
  see("unorm", p->unorm, p->stage_bounds ? N : 1);
}

int enter(const char* sym, bool clears_warning) {
  ++g_calls[sym];
  if (clears_warning) g_warning.clear();
  auto f = g_fail.find(sym);
  if (f != g_fail.end()) { g_error = f->second.second; return f->second.first; }
  auto w = g_warn.find(sym);
  if (clears_warning && w != g_warn.end()) g_warning = w->second;
  return ADMM_OK;
}

void fill(double* p, size_t count, double base) {
  for (size_t i = 0; p && i < count; ++i) p[i] = base + static_cast<double>(i);
}
void fill(int32_t* p, size_t count, int32_t base) {
  for (size_t i = 0; p && i < count; ++i) p[i] = base + static_cast<int32_t>(i);
}

}  // namespace

extern "C" {

// ---- control surface of the tests -------------------------------------------------------------------------------------
void stub_reset(void) {
  for (admm_handle* h : g_handles) delete h;
  g_handles.clear(); g_calls.clear(); g_num.clear(); g_ptr.clear(); g_fail.clear(); g_warn.clear();
  g_error.clear(); g_warning.clear(); g_history = 0;
}
void stub_fail(const char* sym, int code, const char* text) { g_fail[sym] = {code, text}; }
void stub_warn(const char* sym, const char* text) { g_warn[sym] = text; }
void stub_clear_faults(void) { g_fail.clear(); g_warn.clear(); }
void stub_set_history(int k) { g_history = k; }
int stub_calls(const char* sym) { auto it = g_calls.find(sym); return it == g_calls.end() ? 0 : it->second; }
int stub_total_calls(void) { int k = 0; for (auto& c : g_calls) k += c.second; return k; }
int stub_has(const char* key) { return g_num.count(key) != 0; }
double stub_num(const char* key) { auto it = g_num.find(key); return it == g_num.end() ? -12345.0 : it->second; }
uint64_t stub_ptr(const char* key) { auto it = g_ptr.find(key); return it == g_ptr.end() ? ~0ull : it->second; }
int stub_handles(void) { return static_cast<int>(g_handles.size()); }
int stub_frees(int i) { return g_handles[i]->frees; }
uint64_t stub_handle(int i) { return reinterpret_cast<uintptr_t>(g_handles[i]); }

// ---- the ABI ------------------------------------------------------------------------------------------------------------
// deliberately NOT the library's defaults: a gateway that hard-codes a default instead of asking for it is caught
void admm_default_options(admm_options* o) {
  ++g_calls["admm_default_options"];
  *o = admm_options{0.375, 1.25, 3e-5, 7e-4, 123, 7, 3, 2, 11, 5, 21, 9, 4.5, 1.75, 2, 0};
}

int admm_setup_fuel(admm_handle** out, const admm_problem* p, const admm_options* o, const double* fuel) {
  g_num.clear(); g_ptr.clear();
  see_problem(p);
  see("fuel", fuel, p->stage_bounds ? p->N : 1);
  g_num["rho"] = o->rho; g_num["alpha"] = o->alpha; g_num["eps_abs"] = o->eps_abs; g_num["eps_rel"] = o->eps_rel;
  g_num["max_iter"] = o->max_iter; g_num["check_interval"] = o->check_interval; g_num["segments"] = o->segments;
  g_num["device"] = o->device; g_num["zrows"] = o->zrows; g_num["flags"] = o->flags; g_num["adapt_interval"] = o->adapt_interval;
  g_num["adapt_max"] = o->adapt_max; g_num["adapt_mu"] = o->adapt_mu; g_num["adapt_tau"] = o->adapt_tau;
  g_num["precision_mode"] = o->precision_mode; g_num["reserved"] = o->reserved;
  if (int rc = enter("admm_setup_fuel", true)) return rc;
  admm_handle* h = new admm_handle{static_cast<int>(g_handles.size()), p->N, p->n, p->m, p->batch, 0};
  g_handles.push_back(h);
  *out = h;
  return ADMM_OK;
}

int admm_update_problem(admm_handle* h, const admm_problem* p) {
  g_num.clear(); g_ptr.clear();
  g_ptr["handle"] = reinterpret_cast<uintptr_t>(h);
  see_problem(p);
  return enter("admm_update_problem", true);
}

int admm_solve(admm_handle* h, const double* z0, const double* y0, admm_info* info) {
  const size_t LB = static_cast<size_t>(h->N) * (h->n + h->m) * h->batch;
  g_ptr["handle"] = reinterpret_cast<uintptr_t>(h);
  see("z0", z0, LB); see("y0", y0, LB);
  if (int rc = enter("admm_solve", true)) return rc;
  *info = admm_info{41, 42, 43.5, 44.5, 45.5, 46.5, 47, 48};
  return ADMM_OK;
}

int admm_get_rho(admm_handle* h, double* rho) {
  if (int rc = enter("admm_get_rho", false)) return rc;
  fill(rho, h->batch, 500.0);
  return ADMM_OK;
}

int admm_get_info(admm_handle* h, int32_t* iters, int32_t* status, double* r, double* s) {
  if (int rc = enter("admm_get_info", false)) return rc;
  fill(iters, h->batch, 600); fill(status, h->batch, 700); fill(r, h->batch, 800.0); fill(s, h->batch, 900.0);
  return ADMM_OK;
}

int admm_get(admm_handle* h, double* w, double* z, double* y) {
  const size_t LB = static_cast<size_t>(h->N) * (h->n + h->m) * h->batch;
  g_ptr["get_w"] = reinterpret_cast<uintptr_t>(w); g_ptr["get_z"] = reinterpret_cast<uintptr_t>(z);
  g_ptr["get_y"] = reinterpret_cast<uintptr_t>(y);
  if (int rc = enter("admm_get", false)) return rc;
  fill(w, LB, 1e6); fill(z, LB, 2e6); fill(y, LB, 3e6);
  return ADMM_OK;
}

int admm_get_history(admm_handle*, int32_t capacity, int32_t* count, int32_t* iteration, int32_t* n_converged, double* max_r,
                     double* max_s, double* rho) {
  if (int rc = enter("admm_get_history", false)) return rc;
  g_num["history_capacity"] = capacity;
  if (count) *count = g_history;
  const size_t k = capacity < g_history ? (capacity < 0 ? 0 : capacity) : g_history;
  fill(iteration, k, 10); fill(n_converged, k, 20); fill(max_r, k, 30.0); fill(max_s, k, 40.0); fill(rho, k, 50.0);
  return ADMM_OK;
}

int admm_get_path(admm_handle*, admm_path_info* pi) {
  if (int rc = enter("admm_get_path", false)) return rc;
  *pi = admm_path_info{1, 2, 3, 4, 5, 6, 7, 8, 9.5, 10.5, 11.5};
  return ADMM_OK;
}

int admm_iterate(admm_handle* h, int32_t iters) {
  g_ptr["handle"] = reinterpret_cast<uintptr_t>(h);
  g_num["iterate_iters"] = iters;
  return enter("admm_iterate", false);
}

int admm_sync(admm_handle*) { return enter("admm_sync", false); }

void admm_free(admm_handle* h) {
  ++g_calls["admm_free"];
  if (h) ++h->frees;
}

const char* admm_last_error(void) { return g_error.c_str(); }
const char* admm_last_warning(void) { return g_warning.c_str(); }

}  // extern "C"
