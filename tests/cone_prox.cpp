// cone_project of csrc/admm_prox.hpp on the host, stage by stage (tests/test_cone_host.py and tests/test_gpu_cone.py compile this with
// the host compiler).  branch[s] = -1: c = 0, the stage's rows are left to their box (z = v, y = 0 here); else 0 inside, 1 apex,
// 2 surface.
#include "admm_prox.hpp"

extern "C" void cone_stages(int count, int nh, const double* c, const double* p, const double* g, const double* v, double* z, double* y,
                            int* branch) {
  for (int s = 0; s < count; ++s) {
    const double *cs = c + (long)s * nh, *ps = p + (long)s * nh, *vs = v + (long)s * nh;
    double *zs = z + (long)s * nh, *ys = y + (long)s * nh;
    branch[s] = admm::cone_project(cs, ps, g[s], nh, vs, zs, ys);
    if (branch[s] < 0)
      for (int i = 0; i < nh; ++i) { zs[i] = vs[i]; ys[i] = 0.0; }
  }
}
