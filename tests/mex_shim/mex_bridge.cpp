// C bridge between a test (ctypes, or the replay program) and a MEX gateway linked with the stand-in: build inputs, call
// mexFunction the way MATLAB does, read outputs, warnings and the error back, count live arrays, fire the at-exit hook.
#include <cstdint>
#include <cstring>
#include <exception>

#include "mex_standin.hpp"

using namespace standin;

namespace {
Message g_error;            // of the last msb_call ("" / "" if it returned)
int g_orphans = 0;          // arrays the last successful call created and did not return
mxArray* g_plhs[16];

bool reachable(const mxArray* root, const mxArray* a) {
  if (!root) return false;
  if (root == a) return true;
  for (const mxArray* v : root->vals)
    if (reachable(v, a)) return true;
  return false;
}
}  // namespace

extern "C" {

// a numeric, logical or char array of MATLAB dimensions dims, its data copied from `data` (column-major, `bytes` long; NULL:
// zeros).  is_complex / is_sparse only mark the array, which is all the gateway may look at before it refuses one.
mxArray* msb_numeric(int cls, int is_complex, int is_sparse, int ndim, const uint64_t* dims, const void* data, uint64_t bytes) {
  std::vector<mwSize> d(dims, dims + ndim);
  mxArray* a = make(static_cast<mxClassID>(cls), d.size(), d.data(), is_complex != 0, is_sparse != 0);
  if (data && bytes == numel(a) * element_size(a->cls) && bytes) std::memcpy(a->data, data, bytes);
  else if (data && bytes) { mxDestroyArray(a); return nullptr; }
  return a;
}
mxArray* msb_string(const char* s) { return mxCreateString(s); }
mxArray* msb_struct(int nfields, const char** names) { return mxCreateStructMatrix(1, 1, nfields, names); }
void msb_set_field(mxArray* s, const char* name, mxArray* v) { mxSetField(s, 0, name, v); }
void msb_destroy(mxArray* a) { mxDestroyArray(a); }

// Call mexFunction as MATLAB does.  Returns 0 if it returned, 1 if it raised an error through mexErrMsgIdAndTxt, 2 if anything
// else was thrown.  MATLAB rules restated here:
//   - plhs has room for max(nlhs, 1) outputs: a MEX function may assign plhs[0] with nlhs = 0 (it becomes `ans`);
//   - on an error every array the call created is destroyed ("MATLAB automatically frees ... when the MEX function ends");
//   - after a normal return the arrays the call created and did not return are destroyed the same way (counted: msb_orphans).
// The outputs belong to the caller afterwards (msb_destroy).
int msb_call(int nlhs, int nrhs, mxArray** prhs) {
  begin_call();
  g_error = {};
  g_orphans = 0;
  for (mxArray*& p : g_plhs) p = nullptr;
  int rc = 0;
  try {
    mexFunction(nlhs, g_plhs, nrhs, const_cast<const mxArray**>(prhs));
  } catch (const MexError& e) {
    g_error = {e.id, e.text};
    rc = 1;
  } catch (const std::exception& e) {
    g_error = {"standin:exception", e.what()};
    rc = 2;
  }
  if (rc) {
    while (!created_in_call.empty()) destroy_shallow(created_in_call.back());
    for (mxArray*& p : g_plhs) p = nullptr;
    return rc;
  }
  const int nout = nlhs > 1 ? nlhs : 1;
  std::vector<mxArray*> lost;
  for (mxArray* a : created_in_call) {
    bool kept = false;
    for (int i = 0; i < nout && !kept; ++i) kept = reachable(g_plhs[i], a);
    if (!kept) lost.push_back(a);
  }
  g_orphans = static_cast<int>(lost.size());
  for (mxArray* a : lost) destroy_shallow(a);
  return 0;
}
mxArray* msb_output(int i) { return (i >= 0 && i < 16) ? g_plhs[i] : nullptr; }
int msb_orphans(void) { return g_orphans; }

int msb_class(const mxArray* a) { return a->cls; }
int msb_ndim(const mxArray* a) { return static_cast<int>(a->dims.size()); }
uint64_t msb_dim(const mxArray* a, int i) { return a->dims[i]; }
uint64_t msb_numel(const mxArray* a) { return numel(a); }
uint64_t msb_element_size(const mxArray* a) { return element_size(a->cls); }
const void* msb_data(const mxArray* a) { return a->data; }
int msb_nfields(const mxArray* a) { return mxGetNumberOfFields(a); }
const char* msb_field_name(const mxArray* a, int i) { return mxGetFieldNameByNumber(a, i); }
mxArray* msb_field(const mxArray* a, const char* name) { return mxGetField(a, 0, name); }

int msb_live(void) { return static_cast<int>(live.size()); }
int msb_warning_count(void) { return static_cast<int>(warnings.size()); }
const char* msb_warning_id(int i) { return warnings[i].id.c_str(); }
const char* msb_warning_text(int i) { return warnings[i].text.c_str(); }
const char* msb_error_id(void) { return g_error.id.c_str(); }
const char* msb_error_text(void) { return g_error.text.c_str(); }

int msb_at_exit_registrations(void) { return at_exit_registrations; }
// what clearing the MEX file does: the registered function runs (it stays registered: the gateway's statics live on here,
// where MATLAB would unload them with the file)
int msb_fire_at_exit(void) {
  if (!at_exit_fn) return 0;
  at_exit_fn();
  return 1;
}

}  // extern "C"
