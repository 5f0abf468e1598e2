// Host wrapper of csrc/admm_prox.hpp for tests/test_prox_host.py (compiled by the test, not part of libadmm_hip.so): the z-update
// of whole blocks over the header's functions, composed the way the one-lane fused kernels compose them (the row text and the SOC
// pre-pass documented in the header), over arrays laid out [batch][N][n + m].  It pins the header's functions and that
// composition; it does not compile the kernels' own copies of that text, which only tests/test_gpu_prox_edges.py pins.
// vin = 0: the old state is the pair (s1, s0) = (z, y); vin = 1: s0 = v and the pair is rebuilt.
// fuel = 0 takes the per-instance kernels' factor (no fuel weight).
#include "admm_prox.hpp"

using namespace admm;

template <int NX, int NU, bool VIN, bool RELAX, bool FUEL>
static void block(const double* s0, const double* s1, const double* w, const double* lo, const double* hi, double ub, double kap,
                  double alpha, double* v, double* z, double* y, ResidSums& acc) {
  constexpr int NB = NX + NU;
  double c0[NB], vnu[NB];
  for (int r = 0; r < NB; ++r) c0[r] = s0[r];
  auto scale = [&](const double (&blk)[NB]) { return FUEL ? soc_scale<NU, NB>(blk, ub, kap) : ball_scale<NU, NB>(blk, ub); };
  const double cs_old = VIN ? scale(c0) : 1.0;
  for (int r = 0; r < NB; ++r) {       // the pre-pass: the control rows of v+ first
    if (r < NU) {
      double zo, yo;
      if (VIN) { zo = clip_hi(clip_lo(s0[r] * cs_old, lo[r]), hi[r]); yo = s0[r] - zo; }
      else { yo = s0[r]; zo = s1[r]; }
      vnu[r] = relaxed<RELAX>(alpha, w[r], zo) + yo;
    } else {
      vnu[r] = 0.0;
    }
  }
  const double cs_new = scale(vnu);
  for (int r = 0; r < NB; ++r) {
    const bool ball = r < NU;
    double zo, yo;
    if (VIN) { zo = clip(ball ? s0[r] * cs_old : s0[r], lo[r], hi[r]); yo = s0[r] - zo; }
    else { yo = s0[r]; zo = s1[r]; }
    const double vn = relaxed<RELAX>(alpha, w[r], zo) + yo;
    const double zn = clip(ball ? vn * cs_new : vn, lo[r], hi[r]);
    const double yn = vn - zn;
    v[r] = vn;
    z[r] = zn;
    y[r] = yn;
    acc.add(w[r], zn, zo, yn);
  }
}

typedef void (*block_fn)(const double*, const double*, const double*, const double*, const double*, double, double, double, double*,
                         double*, double*, ResidSums&);

template <int NX, int NU>
static block_fn pick(int vin, int relax, int fuel) {
  static const block_fn t[8] = {block<NX, NU, false, false, false>, block<NX, NU, false, false, true>, block<NX, NU, false, true, false>,
                                block<NX, NU, false, true, true>,   block<NX, NU, true, false, false>, block<NX, NU, true, false, true>,
                                block<NX, NU, true, true, false>,   block<NX, NU, true, true, true>};
  return t[(vin ? 4 : 0) + (relax ? 2 : 0) + (fuel ? 1 : 0)];
}

// sums: [batch][5], the five partial sums of ResidSums over all rows of a QP.  Returns 0, or -1 for a pair that is not compiled.
extern "C" int prox_zupdate(int n, int m, int vin, int relax, int fuel, int batch, int N, const double* s0, const double* s1,
                            const double* w, const double* lo, const double* hi, const double* ub, const double* kap, double alpha,
                            double* v, double* z, double* y, double* sums) {
  block_fn f = nullptr;
  if (n == 2 && m == 1) f = pick<2, 1>(vin, relax, fuel);
  if (n == 6 && m == 3) f = pick<6, 3>(vin, relax, fuel);
  if (!f) return -1;
  const int nb = n + m;
  for (int b = 0; b < batch; ++b) {
    ResidSums acc;
    for (int k = 0; k < N; ++k) {
      const long o = ((long)b * N + k) * nb;
      f(s0 + o, s1 + o, w + o, lo + o, hi + o, ub[k], kap[k], alpha, v + o, z + o, y + o, acc);
    }
    const double out[5] = {acc.r, acc.s, acc.w, acc.z, acc.y};
    for (int q = 0; q < 5; ++q) sums[b * 5 + q] = out[q];
  }
  return 0;
}
