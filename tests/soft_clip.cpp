// soft_clip of csrc/admm_prox.hpp on the host, elementwise (tests/test_soft_host.py compiles this with the host compiler).
#include "admm_prox.hpp"

extern "C" void soft_clip_rows(int count, const double* v, const double* lo, const double* hi, const double* kap, double* z, double* y) {
  for (int i = 0; i < count; ++i) {
    z[i] = admm::soft_clip(v[i], lo[i], hi[i], kap[i]);
    y[i] = v[i] - z[i];
  }
}
