// Stand-alone replay of gateway calls, for a sanitizer: links the gateway, the stand-in, the bridge and the ABI stub, reads a
// script (tests/_mex.py: Script) and makes the same calls the Python tests make through ctypes.  Exit status 0 iff every call
// ended as the script expects, no array outlived its step and the sanitizers the program was built with saw nothing.  Lines:
//   N id class complex sparse ndim d.. count v..   numeric array      S id text            char row
//   T id nfields name id ..                        1 x 1 struct       F symbol code text   the stub fails that call
//   C nlhs expect save nrhs id..                   call; expect = ok | error id; save = - | name (kept as @name)
//   R                                              fire the at-exit hook, drop the saved outputs, reset the stub
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "mex_standin.hpp"

extern "C" {
mxArray* msb_numeric(int, int, int, int, const uint64_t*, const void*, uint64_t);
int msb_call(int, int, mxArray**);
mxArray* msb_output(int);
int msb_live(void);
const char* msb_error_id(void);
const char* msb_error_text(void);
int msb_fire_at_exit(void);
void stub_reset(void);
void stub_fail(const char*, int, const char*);
}

namespace {

template <class T>
mxArray* typed(int cls, int cx, int sp, const std::vector<uint64_t>& dims, const std::vector<double>& v) {
  std::vector<T> data(v.begin(), v.end());
  return msb_numeric(cls, cx, sp, static_cast<int>(dims.size()), dims.data(), data.data(), data.size() * sizeof(T));
}

int die(int line, const std::string& why) {
  std::fprintf(stderr, "mex_replay: line %d: %s\n", line, why.c_str());
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return die(0, "usage: mex_replay SCRIPT");
  std::ifstream in(argv[1]);
  if (!in) return die(0, "cannot open the script");
  std::map<std::string, mxArray*> vals, saved;
  std::string text;
  int line = 0, calls = 0, failures = 0;
  while (std::getline(in, text)) {
    ++line;
    std::istringstream ss(text);
    std::string op, id;
    ss >> op;
    if (op == "N") {
      int cls, cx, sp, nd;
      size_t count;
      ss >> id >> cls >> cx >> sp >> nd;
      std::vector<uint64_t> dims(nd);
      for (uint64_t& d : dims) ss >> d;
      ss >> count;
      std::vector<double> v(count);
      for (double& x : v) {
        std::string tok;
        ss >> tok;
        x = std::strtod(tok.c_str(), nullptr);
      }
      mxArray* a = nullptr;
      switch (cls) {
        case mxDOUBLE_CLASS: a = typed<double>(cls, cx, sp, dims, v); break;
        case mxSINGLE_CLASS: a = typed<float>(cls, cx, sp, dims, v); break;
        case mxINT32_CLASS: a = typed<int32_t>(cls, cx, sp, dims, v); break;
        case mxUINT64_CLASS: a = typed<uint64_t>(cls, cx, sp, dims, v); break;
        case mxLOGICAL_CLASS: a = typed<uint8_t>(cls, cx, sp, dims, v); break;
        default: return die(line, "class not supported by the replay");
      }
      if (!a) return die(line, "data do not fill the dimensions");
      vals[id] = a;
    } else if (op == "S") {
      std::string s;
      ss >> id >> s;
      vals[id] = mxCreateString(s.c_str());
    } else if (op == "T") {
      int nf;
      ss >> id >> nf;
      std::vector<std::string> names(nf), ids(nf);
      for (int i = 0; i < nf; ++i) ss >> names[i] >> ids[i];
      std::vector<const char*> cn;
      for (auto& s : names) cn.push_back(s.c_str());
      mxArray* st = mxCreateStructMatrix(1, 1, nf, cn.data());
      for (int i = 0; i < nf; ++i) {
        mxSetField(st, 0, cn[i], vals.at(ids[i]));
        vals.erase(ids[i]);      // the struct owns it now
      }
      vals[id] = st;
    } else if (op == "F") {
      int code;
      std::string s;
      ss >> id >> code >> s;
      stub_fail(id.c_str(), code, s.c_str());
    } else if (op == "C") {
      int nlhs, nrhs;
      std::string expect, save;
      ss >> nlhs >> expect >> save >> nrhs;
      std::vector<mxArray*> prhs;
      for (int i = 0; i < nrhs; ++i) {
        ss >> id;
        prhs.push_back(id[0] == '@' ? saved.at(id.substr(1)) : vals.at(id));
      }
      const int rc = msb_call(nlhs, nrhs, prhs.data());
      ++calls;
      const std::string got = rc ? msb_error_id() : "ok";
      // (a call that ends otherwise than expected is reported and the replay goes on: what the library would then read is the point)
      if (got != expect) failures += die(line, "expected " + expect + ", got " + got + ": " + msb_error_text());
      for (int i = 0; i < 16; ++i) {
        mxArray* o = msb_output(i);
        if (!o) continue;
        if (i == 0 && save != "-") {
          if (saved.count(save)) mxDestroyArray(saved[save]);
          saved[save] = o;
        } else {
          mxDestroyArray(o);
        }
      }
      for (auto& kv : vals) mxDestroyArray(kv.second);
      vals.clear();
      if (msb_live() != static_cast<int>(saved.size())) return die(line, "an array outlived the call");
    } else if (op == "R") {
      msb_fire_at_exit();
      for (auto& kv : saved) mxDestroyArray(kv.second);
      saved.clear();
      stub_reset();
      if (msb_live() != 0) return die(line, "arrays are left after a reset");
    } else if (!op.empty()) {
      return die(line, "unknown line " + op);
    }
  }
  std::printf("mex_replay: %d calls replayed, %d ended otherwise than expected\n", calls, failures);
  return failures != 0;
}
