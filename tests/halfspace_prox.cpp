// halfspace_project of csrc/admm_prox.hpp on the host, stage by stage (tests/test_halfspace_host.py and tests/test_gpu_halfspace.py
// compile this with the host compiler).  active[s] = 0: a = 0, the stage's rows are left to their box (z = v, y = 0 here).
#include "admm_prox.hpp"

extern "C" void halfspace_stages(int count, int nh, const double* a, const double* b, const double* v, double* z, double* y, int* active) {
  for (int s = 0; s < count; ++s) {
    const double *as = a + (long)s * nh, *vs = v + (long)s * nh;
    double *zs = z + (long)s * nh, *ys = y + (long)s * nh;
    active[s] = admm::halfspace_project(as, b[s], nh, vs, zs, ys) ? 1 : 0;
    if (!active[s])
      for (int i = 0; i < nh; ++i) { zs[i] = vs[i]; ys[i] = 0.0; }
  }
}
