// A functional stand-in for the part of the MEX / MX Matrix C API that matlab/admm_mex.cpp uses.  It is NOT MATLAB: every rule
// below restates, in one comment, the behaviour MathWorks documents for that function (the reference pages of the "C Matrix API"
// and "C MEX API"), and nothing more.  Where the documentation calls a use undefined or an error (mxGetScalar of an empty array,
// mxSetField of a field that does not exist), the stand-in raises "standin:undefined" so that a gateway relying on it is caught.
#include "mex_standin.hpp"

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace standin {

std::vector<mxArray*> live;
std::vector<mxArray*> created_in_call;
std::vector<Message> warnings;
void (*at_exit_fn)(void) = nullptr;
int at_exit_registrations = 0;

[[noreturn]] static void undefined(const char* what) { throw MexError{"standin:undefined", what}; }

// mxGetElementSize: bytes per element; a char is a 16-bit mxChar, a logical one byte
size_t element_size(mxClassID cls) {
  switch (cls) {
    case mxLOGICAL_CLASS: case mxINT8_CLASS: case mxUINT8_CLASS: return 1;
    case mxCHAR_CLASS: case mxINT16_CLASS: case mxUINT16_CLASS: return 2;
    case mxSINGLE_CLASS: case mxINT32_CLASS: case mxUINT32_CLASS: return 4;
    case mxDOUBLE_CLASS: case mxINT64_CLASS: case mxUINT64_CLASS: return 8;
    default: return 0;      // struct, cell: no numeric data
  }
}

size_t numel(const mxArray* a) {
  size_t k = 1;
  for (mwSize d : a->dims) k *= d;
  return k;
}

// mxCreateNumericArray and its kin: "any trailing singleton dimensions specified in the dims argument are automatically removed
// from the resulting array", and every array has at least two dimensions (ndim < 2 is taken as 2, the missing ones being 1).
// The data are zero-initialised.  Each array owns one allocation of its exact size, so a sanitizer sees where it ends; an
// empty array has no data (mxGetData returns NULL).
mxArray* make(mxClassID cls, mwSize ndim, const mwSize* dims, bool is_complex, bool is_sparse) {
  mxArray* a = new mxArray_tag{cls, std::vector<mwSize>(dims, dims + ndim), is_complex, is_sparse, nullptr, {}, {}};
  while (a->dims.size() < 2) a->dims.push_back(1);
  while (a->dims.size() > 2 && a->dims.back() == 1) a->dims.pop_back();
  const size_t bytes = numel(a) * element_size(cls);
  if (bytes) a->data = std::calloc(bytes, 1);
  live.push_back(a);
  created_in_call.push_back(a);
  return a;
}

void destroy_shallow(mxArray* a) {
  auto it = std::find(live.begin(), live.end(), a);
  if (it == live.end()) undefined("an array was destroyed twice, or never existed");
  live.erase(it);
  auto c = std::find(created_in_call.begin(), created_in_call.end(), a);
  if (c != created_in_call.end()) created_in_call.erase(c);
  std::free(a->data);
  delete a;
}

void begin_call() {
  created_in_call.clear();
  warnings.clear();
}

static std::string vformat(const char* fmt, va_list ap) {
  char buf[2048];
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  return buf;
}

}  // namespace standin

using namespace standin;

extern "C" {

// mexErrMsgIdAndTxt: "displays an error message and returns control to the MATLAB prompt": it never returns to the MEX function.
// MATLAB unwinds the call; the stand-in throws, and the bridge catches, records id and text and frees what the call created.
void mexErrMsgIdAndTxt(const char* id, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::string text = vformat(fmt, ap);
  va_end(ap);
  throw MexError{id ? id : "", text};
}

// mexWarnMsgIdAndTxt: "displays a warning message ... the MEX function continues executing"
void mexWarnMsgIdAndTxt(const char* id, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  warnings.push_back({id ? id : "", vformat(fmt, ap)});
  va_end(ap);
}

// mexAtExit: registers the function called when the MEX function is cleared or MATLAB exits; "each MEX function can register
// only one active exit function": a later call replaces the earlier one.  Returns 0.
int mexAtExit(void (*fn)(void)) {
  at_exit_fn = fn;
  ++at_exit_registrations;
  return 0;
}

// mxDestroyArray: frees the array and, for a struct, every field value; a NULL argument is allowed and does nothing
void mxDestroyArray(mxArray* a) {
  if (!a) return;
  for (mxArray* v : a->vals) mxDestroyArray(v);
  destroy_shallow(a);
}

mxClassID mxGetClassID(const mxArray* a) { return a->cls; }
bool mxIsDouble(const mxArray* a) { return a->cls == mxDOUBLE_CLASS; }
bool mxIsSingle(const mxArray* a) { return a->cls == mxSINGLE_CLASS; }
bool mxIsLogical(const mxArray* a) { return a->cls == mxLOGICAL_CLASS; }
bool mxIsChar(const mxArray* a) { return a->cls == mxCHAR_CLASS; }
bool mxIsStruct(const mxArray* a) { return a->cls == mxSTRUCT_CLASS; }
bool mxIsUint64(const mxArray* a) { return a->cls == mxUINT64_CLASS; }
// mxIsNumeric: true for the floating-point and integer classes; false for logical, char, struct, cell
bool mxIsNumeric(const mxArray* a) { return a->cls >= mxDOUBLE_CLASS && a->cls <= mxUINT64_CLASS; }
bool mxIsComplex(const mxArray* a) { return a->is_complex; }
bool mxIsSparse(const mxArray* a) { return a->is_sparse; }
// mxIsEmpty: true if any dimension is zero
bool mxIsEmpty(const mxArray* a) { return numel(a) == 0; }

// mxGetM: the first dimension
size_t mxGetM(const mxArray* a) { return a->dims[0]; }
// mxGetN: "if the array is N-dimensional, the product of dimensions 2 through N"
size_t mxGetN(const mxArray* a) {
  size_t k = 1;
  for (size_t i = 1; i < a->dims.size(); ++i) k *= a->dims[i];
  return k;
}
size_t mxGetNumberOfElements(const mxArray* a) { return numel(a); }
size_t mxGetElementSize(const mxArray* a) { return element_size(a->cls); }
// mxGetNumberOfDimensions: "always 2 or more"
mwSize mxGetNumberOfDimensions(const mxArray* a) { return a->dims.size(); }
const mwSize* mxGetDimensions(const mxArray* a) { return a->dims.data(); }

// mxGetData: the first element of the data; NULL if there are none
void* mxGetData(const mxArray* a) { return a->data; }
// mxGetPr: "the input argument must be of type double; otherwise returns NULL" (the non-interleaved API of the default build)
double* mxGetPr(const mxArray* a) { return a->cls == mxDOUBLE_CLASS ? static_cast<double*>(a->data) : nullptr; }

// mxGetScalar: the real part of the first element, converted to double, for numeric, logical and char arrays.  For an empty
// array, a struct or a cell the documentation promises nothing (an indeterminate value, or an error in current releases).
double mxGetScalar(const mxArray* a) {
  if (numel(a) == 0) undefined("mxGetScalar of an empty array");
  switch (a->cls) {
    case mxDOUBLE_CLASS: return *static_cast<const double*>(a->data);
    case mxSINGLE_CLASS: return *static_cast<const float*>(a->data);
    case mxLOGICAL_CLASS: case mxUINT8_CLASS: return *static_cast<const uint8_t*>(a->data);
    case mxINT8_CLASS: return *static_cast<const int8_t*>(a->data);
    case mxCHAR_CLASS: case mxUINT16_CLASS: return *static_cast<const uint16_t*>(a->data);
    case mxINT16_CLASS: return *static_cast<const int16_t*>(a->data);
    case mxINT32_CLASS: return *static_cast<const int32_t*>(a->data);
    case mxUINT32_CLASS: return *static_cast<const uint32_t*>(a->data);
    case mxINT64_CLASS: return static_cast<double>(*static_cast<const int64_t*>(a->data));
    case mxUINT64_CLASS: return static_cast<double>(*static_cast<const uint64_t*>(a->data));
    default: undefined("mxGetScalar of a struct or cell");
  }
}

// mxGetString: copies the characters into buf and terminates them; returns 0 on success and 1 on failure -- the array is not
// a char array, or it does not fit: then buflen - 1 characters are copied (and terminated)
int mxGetString(const mxArray* a, char* buf, mwSize buflen) {
  if (!buflen) return 1;
  if (a->cls != mxCHAR_CLASS) { buf[0] = 0; return 1; }
  const size_t k = numel(a), c = std::min<size_t>(k, buflen - 1);
  for (size_t i = 0; i < c; ++i) buf[i] = static_cast<char>(static_cast<const uint16_t*>(a->data)[i]);
  buf[c] = 0;
  return k > c;
}

int mxGetNumberOfFields(const mxArray* a) { return a->cls == mxSTRUCT_CLASS ? static_cast<int>(a->fields.size()) : 0; }
const char* mxGetFieldNameByNumber(const mxArray* a, int i) {
  return (a->cls == mxSTRUCT_CLASS && i >= 0 && i < static_cast<int>(a->fields.size())) ? a->fields[i].c_str() : nullptr;
}

// mxGetField: NULL if the array is not a struct, has no field of that name, the index is out of range, or the field of that
// element has no value
mxArray* mxGetField(const mxArray* a, mwIndex index, const char* name) {
  if (!a || a->cls != mxSTRUCT_CLASS || index >= numel(a)) return nullptr;
  for (size_t f = 0; f < a->fields.size(); ++f)
    if (a->fields[f] == name) return a->vals[index * a->fields.size() + f];
  return nullptr;
}

// mxSetField: stores the pointer (no copy: the struct owns the value from then on); it does not free a value already there.
// A field that does not exist, or a non-struct, is a misuse MATLAB does not define.
void mxSetField(mxArray* a, mwIndex index, const char* name, mxArray* v) {
  if (!a || a->cls != mxSTRUCT_CLASS || index >= numel(a)) undefined("mxSetField on a non-struct or out of range");
  for (size_t f = 0; f < a->fields.size(); ++f)
    if (a->fields[f] == name) { a->vals[index * a->fields.size() + f] = v; return; }
  undefined("mxSetField of a field the struct does not have");
}

mxArray* mxCreateNumericArray(mwSize ndim, const mwSize* dims, mxClassID cls, mxComplexity c) {
  return make(cls, ndim, dims, c == mxCOMPLEX, false);
}
mxArray* mxCreateNumericMatrix(mwSize m, mwSize n, mxClassID cls, mxComplexity c) {
  const mwSize d[2] = {m, n};
  return make(cls, 2, d, c == mxCOMPLEX, false);
}
mxArray* mxCreateDoubleMatrix(mwSize m, mwSize n, mxComplexity c) { return mxCreateNumericMatrix(m, n, mxDOUBLE_CLASS, c); }
mxArray* mxCreateDoubleScalar(double v) {
  mxArray* a = mxCreateDoubleMatrix(1, 1, mxREAL);
  *static_cast<double*>(a->data) = v;
  return a;
}
mxArray* mxCreateLogicalScalar(bool v) {
  const mwSize d[2] = {1, 1};
  mxArray* a = make(mxLOGICAL_CLASS, 2, d, false, false);
  *static_cast<uint8_t*>(a->data) = v;
  return a;
}
// mxCreateString: a 1 x strlen char array (0 x 0 for the empty string)
mxArray* mxCreateString(const char* s) {
  const size_t k = std::strlen(s);
  const mwSize d[2] = {k ? 1u : 0u, k};
  mxArray* a = make(mxCHAR_CLASS, 2, d, false, false);
  for (size_t i = 0; i < k; ++i) static_cast<uint16_t*>(a->data)[i] = static_cast<unsigned char>(s[i]);
  return a;
}
// mxCreateStructMatrix: an m x n struct with the given fields, every value unset (NULL)
mxArray* mxCreateStructMatrix(mwSize m, mwSize n, int nfields, const char** names) {
  const mwSize d[2] = {m, n};
  mxArray* a = make(mxSTRUCT_CLASS, 2, d, false, false);
  for (int i = 0; i < nfields; ++i) a->fields.push_back(names[i]);
  a->vals.assign(numel(a) * a->fields.size(), nullptr);
  return a;
}

}  // extern "C"
