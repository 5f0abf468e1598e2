// What the stand-in (mex_standin.cpp) shares with the bridge (mex_bridge.cpp): the array record, the registry of live arrays
// and the records of one mexFunction call.  Test code only.
#ifndef MEX_STANDIN_HPP
#define MEX_STANDIN_HPP
#include <string>
#include <vector>

#include "mex.h"

struct mxArray_tag {
  mxClassID cls;
  std::vector<mwSize> dims;        // at least 2 entries, no trailing singleton beyond the second
  bool is_complex, is_sparse;      // marks only: enough for mxIsComplex / mxIsSparse to answer as MATLAB would
  void* data;                      // numeric, logical, char: its own allocation of exactly numel * element size bytes; NULL when empty
  std::vector<std::string> fields; // struct: field names ...
  std::vector<mxArray*> vals;      // ... and numel * fields.size() values, element-major; owned; NULL = never set
};

namespace standin {

struct Message { std::string id, text; };
struct MexError { std::string id, text; };           // what mexErrMsgIdAndTxt throws

extern std::vector<mxArray*> live;                   // every array that exists, inputs included
extern std::vector<mxArray*> created_in_call;        // arrays created since begin_call()
extern std::vector<Message> warnings;                // mexWarnMsgIdAndTxt since begin_call()
extern void (*at_exit_fn)(void);
extern int at_exit_registrations;

mxArray* make(mxClassID cls, mwSize ndim, const mwSize* dims, bool is_complex, bool is_sparse);
size_t element_size(mxClassID cls);
size_t numel(const mxArray* a);
void destroy_shallow(mxArray* a);                    // this array only, not the values of a struct's fields
void begin_call();

}  // namespace standin
#endif
