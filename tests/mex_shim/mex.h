/* STAND-IN -- not MATLAB's mex.h.  Declares the handful of MEX C API symbols
 * matlab/admm_mex.cpp uses (and the few more the tests need to build inputs), with
 * the signatures MathWorks documents.  `g++ -fsyntax-only` type-checks the gateway
 * against it (tests/test_host.py); mex_standin.cpp implements it, restating the
 * documented behaviour rule by rule, so that the gateway can be linked and executed
 * in an image that has no MATLAB (tests/test_mex_host.py, tests/test_gpu_mex.py).
 * Nothing here is shipped. */
#ifndef MEX_SHIM_H
#define MEX_SHIM_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef struct mxArray_tag mxArray;
typedef size_t mwSize;
typedef size_t mwIndex;
typedef enum { mxREAL = 0, mxCOMPLEX = 1 } mxComplexity;
/* the values of matrix.h */
typedef enum {
  mxUNKNOWN_CLASS = 0, mxCELL_CLASS = 1, mxSTRUCT_CLASS = 2, mxLOGICAL_CLASS = 3, mxCHAR_CLASS = 4, mxVOID_CLASS = 5,
  mxDOUBLE_CLASS = 6, mxSINGLE_CLASS = 7, mxINT8_CLASS = 8, mxUINT8_CLASS = 9, mxINT16_CLASS = 10, mxUINT16_CLASS = 11,
  mxINT32_CLASS = 12, mxUINT32_CLASS = 13, mxINT64_CLASS = 14, mxUINT64_CLASS = 15, mxFUNCTION_CLASS = 16
} mxClassID;
/* the entry point of a MEX file has C linkage */
void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]);
void mexErrMsgIdAndTxt(const char* id, const char* fmt, ...);
void mexWarnMsgIdAndTxt(const char* id, const char* fmt, ...);
int mexAtExit(void (*fn)(void));
mxArray* mxGetField(const mxArray*, mwIndex, const char*);
bool mxIsEmpty(const mxArray*);
bool mxIsDouble(const mxArray*);
bool mxIsSingle(const mxArray*);
bool mxIsLogical(const mxArray*);
bool mxIsNumeric(const mxArray*);
bool mxIsComplex(const mxArray*);
bool mxIsSparse(const mxArray*);
bool mxIsChar(const mxArray*);
bool mxIsStruct(const mxArray*);
bool mxIsUint64(const mxArray*);
mxClassID mxGetClassID(const mxArray*);
double* mxGetPr(const mxArray*);
void* mxGetData(const mxArray*);
double mxGetScalar(const mxArray*);
size_t mxGetM(const mxArray*);
size_t mxGetN(const mxArray*);
size_t mxGetNumberOfElements(const mxArray*);
size_t mxGetElementSize(const mxArray*);
mwSize mxGetNumberOfDimensions(const mxArray*);
const mwSize* mxGetDimensions(const mxArray*);
int mxGetNumberOfFields(const mxArray*);
const char* mxGetFieldNameByNumber(const mxArray*, int);
int mxGetString(const mxArray*, char*, mwSize);
mxArray* mxCreateNumericArray(mwSize, const mwSize*, mxClassID, mxComplexity);
mxArray* mxCreateNumericMatrix(mwSize, mwSize, mxClassID, mxComplexity);
mxArray* mxCreateDoubleMatrix(mwSize, mwSize, mxComplexity);
mxArray* mxCreateDoubleScalar(double);
mxArray* mxCreateLogicalScalar(bool);
mxArray* mxCreateString(const char*);
mxArray* mxCreateStructMatrix(mwSize, mwSize, int, const char**);
void mxSetField(mxArray*, mwIndex, const char*, mxArray*);
void mxDestroyArray(mxArray*);
#ifdef __cplusplus
}
#endif
#endif
