// admm_mex.cpp -- MEX gateway: marshals mxArray <-> the C ABI of libadmm_hip.so
// (include/admm_hip.h).  It contains no arithmetic.
//
// STATUS: written against the documented MEX C API (mex.h / matrix.h).  It is EXECUTED against a stand-in that restates that
// documentation (tests/mex_shim: trailing singleton dimensions dropped, mxGetN, mxGetField, mxGetPr, errors that do not
// return) -- on the CPU with a stub of the C ABI, stand-alone under ASan / UBSan included (tests/test_mex_host.py), and on the
// GPU with libadmm_hip.so, bit for bit against the ctypes host (tests/test_gpu_mex.py).  It has STILL NEVER been linked
// against libmx / libmex or run under MATLAB: no MATLAB, Octave, mex or mex.h exists in the build image or on the GPU box
// (SURVEY.md §8b).  The reference defines no MEX interface to mirror (README.md:1-2 only), so the command set below is this
// repository's own.
//
// Build (on a machine with MATLAB + ROCm):
//   mex -I../include admm_mex.cpp -L../admm-library_amd -ladmm_hip
//
// Usage from MATLAB (see admm_setup.m / admm_solve.m / admm_update.m / admm_free.m):
//   h    = admm_mex('setup', problem, options)   % uint64 scalar handle
//   info = admm_mex('solve', h, z0, y0)          % z0, y0 optional / []
//   [w, z, y] = admm_mex('get', h)
//   admm_mex('iterate', h, iters)
//   admm_mex('update', h, problem)               % new shared data on a live handle (admm_update_problem)
//   hist = admm_mex('history', h)                % the records of ADMM_FLAG_HISTORY (options.flags = 64)
//   p    = admm_mex('path', h)                   % kernels in use, margin of the default path (admm_get_path)
//   admm_mex('free', h)
//
// MATLAB arrays are column-major doubles, exactly the ABI's layout: A (n x n or
// n x n x N), B (n x m [x N]), x0 (n x batch), q (L x batch), lo/hi ((m+n) x 1 or
// (m+n) x N) are passed by pointer, no copies -- after every array's class and full size have been checked: the ABI takes
// raw pointers, so what is let through here is read past its end.
#include <cstdint>
#include <cstring>
#include <vector>

#include "mex.h"

#include "admm_hip.h"

namespace {

void fail(const char* id, const char* msg) { mexErrMsgIdAndTxt(id, "%s", msg); }

void check(int rc) {
  if (rc != ADMM_OK) mexErrMsgIdAndTxt("admm:library", "libadmm_hip error %d: %s", rc, admm_last_error());
}

// A call that succeeded but changed the kernels the handle runs says so (ABI v6): pass it on as a MATLAB warning.  Only after
// the calls that can set the text -- admm_setup*, admm_update_problem, admm_solve: the library clears it at the start of those
// and of no other call, so asking after any other call would repeat an old warning (Solver._warn of the Python host: same rule).
void forward_warning() {
  const char* w = admm_last_warning();
  if (w && w[0]) mexWarnMsgIdAndTxt("admm:path", "%s", w);
}

const mxArray* field(const mxArray* s, const char* name, bool required) {
  const mxArray* f = mxGetField(s, 0, name);
  if (!f && required) mexErrMsgIdAndTxt("admm:input", "problem field '%s' is missing", name);
  return f;
}

const double* dbl(const mxArray* a, const char* name) {
  if (!a || mxIsEmpty(a)) return nullptr;
  if (!mxIsDouble(a) || mxIsComplex(a) || mxIsSparse(a))
    mexErrMsgIdAndTxt("admm:input", "'%s' must be a full real double array", name);
  return mxGetPr(a);
}

// a required array: as dbl, and not empty
const double* req(const mxArray* a, const char* name) {
  const double* p = dbl(a, name);
  if (!p) mexErrMsgIdAndTxt("admm:input", "'%s' must not be empty", name);
  return p;
}

// one real number (any numeric class, or a logical); mxGetScalar promises nothing for an empty array, a struct or a cell
double number(const mxArray* a, const char* name) {
  if (!a || !(mxIsNumeric(a) || mxIsLogical(a)) || mxIsComplex(a) || mxIsSparse(a) || mxGetNumberOfElements(a) != 1)
    mexErrMsgIdAndTxt("admm:input", "'%s' must be a real scalar", name);
  return mxGetScalar(a);
}

int32_t integer(const mxArray* a, const char* name) {
  const double v = number(a, name);
  if (!(v >= -2147483648.0 && v <= 2147483647.0) || v != static_cast<double>(static_cast<int32_t>(v)))
    mexErrMsgIdAndTxt("admm:input", "'%s' must be an integer", name);
  return static_cast<int32_t>(v);
}

double scalar_or(const mxArray* s, const char* name, double dflt) {
  const mxArray* f = s ? mxGetField(s, 0, name) : nullptr;
  return (f && !mxIsEmpty(f)) ? number(f, name) : dflt;
}

int32_t integer_or(const mxArray* s, const char* name, int32_t dflt) {
  const mxArray* f = s ? mxGetField(s, 0, name) : nullptr;
  return (f && !mxIsEmpty(f)) ? integer(f, name) : dflt;
}

bool flag(const mxArray* s, const char* name) {
  const mxArray* f = mxGetField(s, 0, name);
  return f && !mxIsEmpty(f) && number(f, name) != 0.0;
}

// The C ABI takes raw pointers: this is the only place where the size of a MATLAB array can be checked.  True iff `a` is
// d0 x d1 x d2 x d3 as MATLAB stores it: trailing singleton dimensions are dropped on creation (n x n x N x 1 IS 3-D,
// n x n x 1 IS 2-D), so the dimensions an array does not have count as 1.
bool is_size(const mxArray* a, size_t d0, size_t d1, size_t d2 = 1, size_t d3 = 1) {
  const size_t want[4] = {d0, d1, d2, d3};
  const mwSize nd = mxGetNumberOfDimensions(a);
  const mwSize* d = mxGetDimensions(a);
  for (mwSize i = 0; i < nd || i < 4; ++i)
    if ((i < nd ? d[i] : 1) != (i < 4 ? want[i] : 1)) return false;
  return true;
}

admm_handle* handle_of(const mxArray* a) {
  if (!a || !mxIsUint64(a) || mxIsComplex(a) || mxGetNumberOfElements(a) != 1) fail("admm:input", "handle must be a uint64 scalar");
  admm_handle* h = reinterpret_cast<admm_handle*>(static_cast<uintptr_t>(*static_cast<const uint64_t*>(mxGetData(a))));
  if (!h) fail("admm:input", "handle is null (already freed?)");
  return h;
}

// sizes remembered per handle so that 'get' can size its outputs.  Unbounded (a vector, freed slots are
// reused); every handle still alive when MATLAB clears the MEX file or exits is released by at_exit().
struct Dims { admm_handle* h; int L, batch; };
std::vector<Dims> g_dims;
bool g_at_exit_registered = false;

void at_exit() {
  for (Dims& d : g_dims)
    if (d.h) { admm_free(d.h); d.h = nullptr; }
  g_dims.clear();
}

void remember(admm_handle* h, int L, int batch) {
  if (!g_at_exit_registered) { mexAtExit(at_exit); g_at_exit_registered = true; }
  for (Dims& d : g_dims) if (!d.h) { d = {h, L, batch}; return; }
  g_dims.push_back({h, L, batch});
}
Dims* lookup(admm_handle* h) {
  for (Dims& d : g_dims) if (d.h == h) return &d;
  fail("admm:input", "unknown handle (freed, or not made by admm_setup)");
  return nullptr;
}

// MATLAB problem struct -> admm_problem (pointers into the struct's arrays; valid while P is).  Every array is checked for class
// and for its full size -- what Problem.validate of the Python host enforces -- before a pointer is handed on.
void parse_problem(const mxArray* P, admm_problem& p) {
  const mxArray *A = field(P, "A", true), *B = field(P, "B", true), *x0 = field(P, "x0", true);
  const mxArray *lo = field(P, "lo", true), *hi = field(P, "hi", true), *q = field(P, "q", false);
  const mxArray *Q = field(P, "Q", true), *R = field(P, "R", true), *QN = field(P, "QN", true);
  std::memset(&p, 0, sizeof p);
  p.N = integer(field(P, "N", true), "N");
  p.A = req(A, "A"); p.B = req(B, "B");
  p.Q = req(Q, "Q"); p.R = req(R, "R"); p.QN = req(QN, "QN");
  p.x0 = req(x0, "x0"); p.lo = req(lo, "lo"); p.hi = req(hi, "hi");
  p.q = dbl(q, "q");
  if (p.N < 1) fail("admm:input", "N must be at least 1");
  const mwSize* bd = mxGetDimensions(B);
  if (bd[0] > 0x7fffffff || bd[1] > 0x7fffffff || mxGetN(x0) > 0x7fffffff) fail("admm:input", "n, m and batch must fit in an int32");
  p.n = static_cast<int32_t>(bd[0]);
  p.m = static_cast<int32_t>(bd[1]);
  p.batch = static_cast<int32_t>(mxGetN(x0));
  const size_t N = p.N, n = p.n, m = p.m, batch = p.batch, nb = n + m;
  if (N * nb > 0x7fffffff) fail("admm:input", "N (n + m) must fit in an int32");
  // per_instance (logical field, optional): A is n x n x N x batch, B n x m x N x batch (time_varying = 2); with
  // per_instance_bounds lo / hi are (m+n) x N x batch (stage_bounds = 2).  Explicit flags, because MATLAB drops
  // trailing singleton dimensions (an n x n x N x 1 array IS 3-D).
  const bool per_inst = flag(P, "per_instance");
  const bool per_inst_b = flag(P, "per_instance_bounds");
  if (per_inst_b && !per_inst) fail("admm:input", "per_instance_bounds needs per_instance");
  if (!is_size(x0, n, batch)) fail("admm:input", "x0 must be n x batch");
  if (per_inst) {
    p.time_varying = 2;
    if (!is_size(A, n, n, N, batch) || !is_size(B, n, m, N, batch))
      fail("admm:input", "per-instance A / B must be n x n x N x batch / n x m x N x batch");
  } else if (mxGetNumberOfDimensions(A) == 2 && mxGetNumberOfDimensions(B) == 2) {      // (N = 1: n x n x 1 arrives 2-D)
    p.time_varying = 0;
    if (!is_size(A, n, n) || !is_size(B, n, m)) fail("admm:input", "A must be n x n and B n x m (n, m: the size of B)");
  } else {
    p.time_varying = 1;
    if (!is_size(A, n, n, N) || !is_size(B, n, m, N))
      fail("admm:input", "time-varying A / B must be n x n x N / n x m x N, both with N pages");
  }
  if (!is_size(Q, n, n) || !is_size(QN, n, n)) fail("admm:input", "Q and QN must be n x n");
  if (!is_size(R, m, m)) fail("admm:input", "R must be m x m");
  if (mxGetM(lo) != nb || mxGetM(hi) != nb) fail("admm:input", "lo/hi must have m+n rows (u block, then x block)");
  p.stage_bounds = per_inst_b ? 2 : (mxGetN(lo) > 1 ? 1 : 0);
  if (p.stage_bounds == 0 && !is_size(lo, nb, 1)) fail("admm:input", "lo must be (m+n) x 1 or (m+n) x N");
  if (p.stage_bounds == 1 && !is_size(lo, nb, N)) fail("admm:input", "per-stage bounds need N columns");
  if (p.stage_bounds == 2 && !is_size(lo, nb, N, batch)) fail("admm:input", "per-instance bounds must be (m+n) x N x batch");
  if (mxGetNumberOfDimensions(hi) != mxGetNumberOfDimensions(lo) ||
      std::memcmp(mxGetDimensions(hi), mxGetDimensions(lo), mxGetNumberOfDimensions(lo) * sizeof(mwSize)))
    fail("admm:input", "lo and hi must have the same size");
  const mxArray* un = field(P, "unorm", false);     // thrust-magnitude bound, optional: 1 or N entries
  p.unorm = dbl(un, "unorm");
  if (p.unorm && mxGetNumberOfElements(un) != (p.stage_bounds ? N : 1))
    fail("admm:input", "unorm must have 1 entry, or N entries together with per-stage bounds");
  if (p.q && !is_size(q, N * nb, batch)) fail("admm:input", "q must be L x batch");
}

// optional problem field `fuel` (minimum-fuel cost + sum_k fuel_k ||u_k||_2): 1 or N entries, as unorm
const double* parse_fuel(const mxArray* P, const admm_problem& p) {
  const mxArray* fu = field(P, "fuel", false);
  const double* fuel = dbl(fu, "fuel");
  if (fuel && mxGetNumberOfElements(fu) != static_cast<size_t>(p.stage_bounds ? p.N : 1))
    fail("admm:input", "fuel must have 1 entry, or N entries together with per-stage bounds");
  return fuel;
}

}  // namespace

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  if (nrhs < 1 || !mxIsChar(prhs[0])) fail("admm:input", "first argument must be a command string");
  char cmd[32];
  mxGetString(prhs[0], cmd, sizeof cmd);      // (a longer string is cut short, and is then no command)
  const char* commands[] = {"setup", "solve", "get", "history", "path", "iterate", "update", "free"};
  bool known = false;
  for (const char* c : commands) known = known || !std::strcmp(cmd, c);
  if (!known) mexErrMsgIdAndTxt("admm:input", "unknown command '%s'", cmd);

  if (!std::strcmp(cmd, "setup")) {
    if (nrhs < 2 || !mxIsStruct(prhs[1])) fail("admm:input", "setup needs a problem struct");
    const mxArray* P = prhs[1];
    const mxArray* O = (nrhs > 2 && !mxIsEmpty(prhs[2])) ? prhs[2] : nullptr;      // absent or []: the library's defaults
    if (O && !mxIsStruct(O)) fail("admm:input", "options must be a struct or []");
    admm_problem p;
    parse_problem(P, p);
    const double* fuel = parse_fuel(P, p);
    const int L = p.N * (p.n + p.m);
    admm_options o;
    admm_default_options(&o);
    o.rho = scalar_or(O, "rho", o.rho);
    o.alpha = scalar_or(O, "alpha", o.alpha);
    o.eps_abs = scalar_or(O, "eps_abs", o.eps_abs);
    o.eps_rel = scalar_or(O, "eps_rel", o.eps_rel);
    o.max_iter = integer_or(O, "max_iter", o.max_iter);
    o.check_interval = integer_or(O, "check_interval", o.check_interval);
    o.segments = integer_or(O, "segments", o.segments);      // (every absent field keeps what admm_default_options gave)
    o.device = integer_or(O, "device", o.device);
    o.flags = integer_or(O, "flags", o.flags);
    o.adapt_interval = integer_or(O, "adapt_interval", o.adapt_interval);
    o.adapt_max = integer_or(O, "adapt_max", o.adapt_max);
    o.adapt_mu = scalar_or(O, "adapt_mu", o.adapt_mu);
    o.adapt_tau = scalar_or(O, "adapt_tau", o.adapt_tau);
    o.precision_mode = integer_or(O, "precision_mode", o.precision_mode);   // ADMM_PRECISION_*
    admm_handle* h = nullptr;
    check(admm_setup_fuel(&h, &p, &o, fuel));      // (fuel = NULL: admm_setup)
    remember(h, L, p.batch);
    forward_warning();
    plhs[0] = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
    *static_cast<uint64_t*>(mxGetData(plhs[0])) = static_cast<uint64_t>(reinterpret_cast<uintptr_t>(h));
    return;
  }

  if (nrhs < 2) fail("admm:input", "this command needs a handle");
  admm_handle* h = handle_of(prhs[1]);
  Dims* d = lookup(h);

  if (!std::strcmp(cmd, "solve")) {
    const double* z0 = nrhs > 2 ? dbl(prhs[2], "z0") : nullptr;
    const double* y0 = nrhs > 3 ? dbl(prhs[3], "y0") : nullptr;
    if (z0 && !is_size(prhs[2], d->L, d->batch)) fail("admm:input", "z0 must be L x batch");
    if (y0 && !is_size(prhs[3], d->L, d->batch)) fail("admm:input", "y0 must be L x batch");
    admm_info info;
    check(admm_solve(h, z0, y0, &info));
    forward_warning();
    const char* names[] = {"iters_run", "n_converged", "max_r", "max_s", "solve_ms", "iters", "status", "r", "s",
                           "rho", "rho_updates", "mixed_iters", "rho_per_qp"};
    plhs[0] = mxCreateStructMatrix(1, 1, 13, names);
    {
      mxArray* rq = mxCreateDoubleMatrix(d->batch, 1, mxREAL);      // per-instance dynamics: each QP's own rho (ABI v5)
      check(admm_get_rho(h, mxGetPr(rq)));
      mxSetField(plhs[0], 0, "rho_per_qp", rq);
    }
    mxSetField(plhs[0], 0, "mixed_iters", mxCreateDoubleScalar(info.mixed_iters));
    mxSetField(plhs[0], 0, "rho", mxCreateDoubleScalar(info.rho));
    mxSetField(plhs[0], 0, "rho_updates", mxCreateDoubleScalar(info.rho_updates));
    mxSetField(plhs[0], 0, "iters_run", mxCreateDoubleScalar(info.iters_run));
    mxSetField(plhs[0], 0, "n_converged", mxCreateDoubleScalar(info.n_converged));
    mxSetField(plhs[0], 0, "max_r", mxCreateDoubleScalar(info.max_r));
    mxSetField(plhs[0], 0, "max_s", mxCreateDoubleScalar(info.max_s));
    mxSetField(plhs[0], 0, "solve_ms", mxCreateDoubleScalar(info.solve_ms));
    mxArray* it = mxCreateNumericMatrix(d->batch, 1, mxINT32_CLASS, mxREAL);
    mxArray* st = mxCreateNumericMatrix(d->batch, 1, mxINT32_CLASS, mxREAL);
    mxArray* r = mxCreateDoubleMatrix(d->batch, 1, mxREAL);
    mxArray* s = mxCreateDoubleMatrix(d->batch, 1, mxREAL);
    check(admm_get_info(h, static_cast<int32_t*>(mxGetData(it)), static_cast<int32_t*>(mxGetData(st)), mxGetPr(r), mxGetPr(s)));
    mxSetField(plhs[0], 0, "iters", it);
    mxSetField(plhs[0], 0, "status", st);
    mxSetField(plhs[0], 0, "r", r);
    mxSetField(plhs[0], 0, "s", s);
  } else if (!std::strcmp(cmd, "get")) {
    double* out[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < 3 && i < (nlhs > 0 ? nlhs : 1); ++i) {
      plhs[i] = mxCreateDoubleMatrix(d->L, d->batch, mxREAL);
      out[i] = mxGetPr(plhs[i]);
    }
    check(admm_get(h, out[0], out[1], out[2]));
  } else if (!std::strcmp(cmd, "history")) {      // admm_mex('history', h): the records of ADMM_FLAG_HISTORY (o.flags = 64)
    int32_t n = 0;
    check(admm_get_history(h, 0, &n, nullptr, nullptr, nullptr, nullptr, nullptr));
    const char* names[] = {"iteration", "n_converged", "max_r", "max_s", "rho"};
    plhs[0] = mxCreateStructMatrix(1, 1, 5, names);
    mxArray* it = mxCreateNumericMatrix(n, 1, mxINT32_CLASS, mxREAL);
    mxArray* nc = mxCreateNumericMatrix(n, 1, mxINT32_CLASS, mxREAL);
    mxArray* r = mxCreateDoubleMatrix(n, 1, mxREAL);
    mxArray* s = mxCreateDoubleMatrix(n, 1, mxREAL);
    mxArray* rho = mxCreateDoubleMatrix(n, 1, mxREAL);
    check(admm_get_history(h, n, &n, static_cast<int32_t*>(mxGetData(it)), static_cast<int32_t*>(mxGetData(nc)), mxGetPr(r),
                           mxGetPr(s), mxGetPr(rho)));
    mxSetField(plhs[0], 0, "iteration", it);
    mxSetField(plhs[0], 0, "n_converged", nc);
    mxSetField(plhs[0], 0, "max_r", r);
    mxSetField(plhs[0], 0, "max_s", s);
    mxSetField(plhs[0], 0, "rho", rho);
  } else if (!std::strcmp(cmd, "path")) {         // admm_mex('path', h): which kernels the handle runs + the default path's margin
    admm_path_info pi;
    check(admm_get_path(h, &pi));
    const char* names[] = {"alternating", "alt_requested", "mfma", "xfree", "segments", "auto_segments", "scan_form",
                           "per_instance", "alt_check", "alt_gate", "scan_growth"};
    plhs[0] = mxCreateStructMatrix(1, 1, 11, names);
    const double vals[] = {(double)pi.alternating, (double)pi.alt_requested, (double)pi.mfma, (double)pi.xfree, (double)pi.segments,
                           (double)pi.auto_segments, (double)pi.scan_form, (double)pi.per_instance, pi.alt_check, pi.alt_gate,
                           pi.scan_growth};
    for (int i = 0; i < 11; ++i) mxSetField(plhs[0], 0, names[i], mxCreateDoubleScalar(vals[i]));
  } else if (!std::strcmp(cmd, "iterate")) {
    if (nrhs < 3) fail("admm:input", "iterate needs an iteration count");
    check(admm_iterate(h, integer(prhs[2], "iters")));
    check(admm_sync(h));
  } else if (!std::strcmp(cmd, "update")) {       // admm_mex('update', h, problem): new shared data, same shape
    if (nrhs < 3 || !mxIsStruct(prhs[2])) fail("admm:input", "update needs a problem struct");
    admm_problem p;
    parse_problem(prhs[2], p);
    if (p.N * (p.n + p.m) != d->L || p.batch != d->batch) fail("admm:input", "update needs a problem of the handle's N, n, m and batch");
    check(admm_update_problem(h, &p));
    forward_warning();
  } else if (!std::strcmp(cmd, "free")) {
    d->h = nullptr;
    admm_free(h);
  }
}
