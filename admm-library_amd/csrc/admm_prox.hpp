// The z-update of DESIGN.md §2.3 / §2.7, written once: every kernel family (admm_kernels.hpp, admm_kernels_alt.hpp,
// admm_mfma.hpp, admm_pinst.hpp, admm_pinst_rows.hpp) composes its rows from the functions below, so the iterates agree to
// the last bit across families and the v-form (§4.5) can rebuild (z, y) from v with the very operations that produced them.
// Arithmetic only: loads, stores, prefetch and scheduling stay with the kernels.  Callable on the host as well (plain
// inline functions without hipcc), which is how tests/test_prox_host.py pins this one definition without a GPU.
//
// One z-update of a row, from the old state (zo, yo), the x-update's w and the relaxation parameter alpha:
//     w^  = RELAX ? fma(alpha, w, (1 - alpha) zo) : w
//     v+  = w^ + yo
//     zn  = clip(c' v+, lo, hi),   yn = v+ - zn            (c' = 1 except on the control rows of a thrust stage)
// and the old state is either the loaded pair or, in the v-form, rebuilt as  zo = clip(c v, lo, hi), yo = v - zo.
//
// Thrust-magnitude stages (second-order cone, §2.7).  The control rows u of a stage with a thrust bound ub and a fuel
// weight f (kap = f / rho; cost term f ||u||_2) are shrunk by kap, then scaled onto the ball ||u||_2 <= ub:
//     t = min(ub, max(||u|| - kap, 0)),     c = ||u|| > t ? t / ||u|| : 1,      z_u = c u.
// kap = 0 is the plain ball projection (t = min(ub, ||u||); ||u|| > t iff ||u|| > ub), and ||u|| <= kap gives c = 0: a coast
// stage.  sqrt and the division are the correctly rounded fp64 forms and the sum of squares is an fma chain in row order --
// the operations of the CPU oracle.
// BRANCH-FREE in the fused kernels: a stage without a bound carries ub = +inf (and kap = 0), for which the factor is exactly
// 1 (norm > inf is false), and where a bound or a weight is set the box of the control rows is (-inf, inf) (validated at
// setup), so  z_u = clip(c v_u, lo, hi)  is the ball projection in the one case and the box projection in the other, bit
// for bit.  (The first version branched on the wave-uniform `ub < inf`: every row of the block then stayed live across the
// branch and the two sqrt / division sequences inside it, and the fused kernels went to scratch at most shapes.)
// A kernel that reaches the same bits by another sequence keeps it: the block walk of the standalone kernels (z_walk_blocks,
// admm_zdual.hpp: zdual_soc_kernel, v_to_zy_soc_kernel, zdual_soft_kernel<.., true>) branches on the wave-uniform
// `soc && r < m` and takes z_u = c v_u without the clip -- clip(x, -inf, inf) = x for every non-NaN x.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define ADMM_PROX_FN __host__ __device__ __forceinline__
#else
#define ADMM_PROX_FN inline
#endif

namespace admm {

// soc_factor is the general (fuel) form; ball_factor is the per-instance kernels' form, which carry no fuel weight: the two
// give the same bits at kap = 0 but are different instruction sequences, and the per-instance kernels do not pay for the max / subtract.
ADMM_PROX_FN double soc_factor(double nrm, double ub, double kap) {
  const double t = fmin(ub, fmax(nrm - kap, 0.0));
  return nrm > t ? t / nrm : 1.0;
}
ADMM_PROX_FN double ball_factor(double nrm, double ub) { return nrm > ub ? ub / nrm : 1.0; }

// ||u||_2 of the first NU rows of a block, accumulated in row order with fma
template <int NU, int NB>
ADMM_PROX_FN double rows_norm(const double (&blk)[NB]) {
  double ss = 0.0;
#pragma unroll
  for (int j = 0; j < NU; ++j) ss = fma(blk[j], blk[j], ss);
  return sqrt(ss);
}

// the factor of a block from its first NU rows
template <int NU, int NB>
ADMM_PROX_FN double soc_scale(const double (&blk)[NB], double ub, double kap) { return soc_factor(rows_norm<NU, NB>(blk), ub, kap); }
template <int NU, int NB>
ADMM_PROX_FN double ball_scale(const double (&blk)[NB], double ub) { return ball_factor(rows_norm<NU, NB>(blk), ub); }

// the clip and its two halves (a site whose bound is still in memory reads it between them: max, then min)
ADMM_PROX_FN double clip_lo(double v, double lo) { return fmax(v, lo); }
ADMM_PROX_FN double clip_hi(double v, double hi) { return fmin(v, hi); }
ADMM_PROX_FN double clip(double v, double lo, double hi) { return clip_hi(clip_lo(v, lo), hi); }

// Soft box: the prox of  kap dist(., [lo, hi])  at v, kap = s / rho >= 0 the row's weight over rho.  Inside the
// box, or outside by at most kap, the projection c itself; further out, v moved kap towards the box.  A SELECT on |e| <= kap,
// not v - clip(e, -kap, kap): with kap = +inf the result is c, the bits of clip(); with kap = 0 it is v wherever v != c.
ADMM_PROX_FN double soft_clip(double v, double lo, double hi, double kap) {
  const double c = clip(v, lo, hi);
  const double e = v - c;
  return fabs(e) <= kap ? c : (e > 0.0 ? v - kap : v + kap);
}

// Half-space of a stage: the Euclidean projection of the nh rows v onto  a'z <= b.
//     nn = a'a and d = a'v - b as fma chains in row order (d starts at -b),  t = d > 0 ? d / nn : 0,  z_i = fma(-t, a_i, v_i)
// nn == 0 (a = 0) is a stage without a half-space: its rows take their box, and nothing below is evaluated for it.  The chains
// are written where the rows are loaded (halfspace_acc per row); the step and the row are these two functions.  Independent
// of rho: the prox of an indicator.
ADMM_PROX_FN void halfspace_acc(double a, double v, double& nn, double& d) {
  nn = fma(a, a, nn);
  d = fma(a, v, d);
}
ADMM_PROX_FN double halfspace_step(double d, double nn) { return d > 0.0 ? d / nn : 0.0; }
ADMM_PROX_FN double halfspace_row(double t, double a, double v) { return fma(-t, a, v); }
// one stage on the host (tests) and wherever the rows sit in an array: z, y of the nh rows; false = the stage is inactive
ADMM_PROX_FN bool halfspace_project(const double* a, double b, int nh, const double* v, double* z, double* y) {
  double nn = 0.0, d = -b;
  for (int i = 0; i < nh; ++i) halfspace_acc(a[i], v[i], nn, d);
  if (nn == 0.0) return false;
  const double t = halfspace_step(d, nn);
  for (int i = 0; i < nh; ++i) {
    z[i] = halfspace_row(t, a[i], v[i]);
    y[i] = v[i] - z[i];
  }
  return true;
}

// Approach cone of a stage: the Euclidean projection of the nh rows v onto the second-order cone
//     { z :  r <= g s },   e = c / |c|,  s = e'(z - p),  r = |(z - p) - s e|      (axis c, apex p, slope g = tan of the half-angle)
// With dl_i = v_i - p_i and the three sums as fma chains in row order from 0 (cone_norm, cone_acc):
//     nn = c'c,  d = c'dl,  q = dl'dl,   rn = sqrt(nn),  s = d / rn,  r = sqrt(max(fma(-s, s, q), 0))
//     r <= g s         inside:   z_i = v_i      (the bits of v: y_i = +0)
//     else g r <= -s   polar:    z_i = p_i      (the apex)
//     else             surface:  t = fma(g, r, s) / fma(g, g, 1),  bet = g t / r,  kap = (t - bet s) / rn,
//                                z_i = fma(kap, c_i, fma(bet, dl_i, p_i))
// r > 0 in the third branch by the two tests before it.  nn == 0 (c = 0) is a stage without a cone: its rows take their box, and
// nothing below is evaluated for it.  Every product and difference outside an fma is rounded on its own: the functions switch
// contraction off, so that host and device give the same bits.  The row is a select between v, p and the surface expression (no
// divergent branch); the quotients of the surface branch are formed with r replaced by 1 where the branch is not taken, so no
// lane ever divides by zero.  Independent of rho: the prox of an indicator.
enum ConeBranch : int { CONE_INSIDE = 0, CONE_APEX = 1, CONE_SURFACE = 2 };
struct ConeStep {
  double kap, bet;
  int branch;
};
ADMM_PROX_FN double cone_norm(double c, double nn) { return fma(c, c, nn); }
ADMM_PROX_FN void cone_acc(double c, double p, double v, double& d, double& q) {
  const double dl = v - p;
  d = fma(c, dl, d);
  q = fma(dl, dl, q);
}
ADMM_PROX_FN ConeStep cone_step(double nn, double d, double q, double g) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double rn = sqrt(nn);
  const double s = d / rn;
  const double r = sqrt(fmax(fma(-s, s, q), 0.0));
  const double gr = g * r;
  const int branch = r <= g * s ? CONE_INSIDE : gr <= -s ? CONE_APEX : CONE_SURFACE;
  const double r1 = branch == CONE_SURFACE ? r : 1.0;
  const double t = fma(g, r, s) / fma(g, g, 1.0);
  const double gt = g * t;
  const double bet = gt / r1;
  const double bs = bet * s;
  const double kap = (t - bs) / rn;
  return ConeStep{kap, bet, branch};
}
ADMM_PROX_FN double cone_row(const ConeStep& st, double c, double p, double v) {
  const double dl = v - p;
  const double surf = fma(st.kap, c, fma(st.bet, dl, p));
  return st.branch == CONE_INSIDE ? v : st.branch == CONE_APEX ? p : surf;
}
// one stage on the host (tests) and wherever the rows sit in an array: z, y of the nh rows; returns the branch, -1 = no cone
ADMM_PROX_FN int cone_project(const double* c, const double* p, double g, int nh, const double* v, double* z, double* y) {
  double nn = 0.0, d = 0.0, q = 0.0;
  for (int i = 0; i < nh; ++i) {
    nn = cone_norm(c[i], nn);
    cone_acc(c[i], p[i], v[i], d, q);
  }
  if (nn == 0.0) return -1;
  const ConeStep st = cone_step(nn, d, q, g);
  for (int i = 0; i < nh; ++i) {
    z[i] = cone_row(st, c[i], p[i], v[i]);
    y[i] = v[i] - z[i];
  }
  return st.branch;
}

// the relaxed x-update output w^ from w and the old z
template <bool RELAX>
ADMM_PROX_FN double relaxed(double alpha, double w, double zo) {
  return RELAX ? fma(alpha, w, (1.0 - alpha) * zo) : w;
}

// What stays at the sites, and why.  A row of a kernel that has a thrust-bound (SOC) form is written over these functions as
//     zo = clip(ball ? v * c : v, lo, hi);  yo = v - zo;  vn = relaxed(alpha, w, zo) + yo;  zn = clip(ball ? vn * c' : vn, lo, hi);  yn = vn - zn;
// and the SOC pre-pass (z+ needs ||v+_u||, so the control rows of v+ are formed first, then the factor of v+) as the same
// operations on the control rows.  Functions returning the pair (z, y), and a pre-pass function taking the rows and bounds,
// were tried: the bits are the same, but the compiler orders the operations of every SOC form differently and 126 kernels
// came out with other register counts; with the text above every kernel has the registers it had.

// The five residual partial sums of a QP, in their one fixed order:  (w - z+)^2, (z+ - z)^2, w^2, z+^2, y+^2.
// xfz / xfze / xbze keep five scalars and add a row through an object built from them BY VALUE in the row's scope: the
// reference form below changed their registers, and one object for the whole kernel cost xfz_kernel 20-40 of them.
struct ResidSums {
  double r = 0.0, s = 0.0, w = 0.0, z = 0.0, y = 0.0;
  // the one definition, over five accumulators wherever a kernel keeps them (scalars, an array, this object)
  static ADMM_PROX_FN void add(double& r, double& s, double& w, double& z, double& y, double wv, double zn, double zo, double yn) {
    const double dr = wv - zn, ds = zn - zo;
    r = fma(dr, dr, r);
    s = fma(ds, ds, s);
    w = fma(wv, wv, w);
    z = fma(zn, zn, z);
    y = fma(yn, yn, y);
  }
  static ADMM_PROX_FN void add(double (&acc)[5], double wv, double zn, double zo, double yn) {
    add(acc[0], acc[1], acc[2], acc[3], acc[4], wv, zn, zo, yn);
  }
  ADMM_PROX_FN void add(double wv, double zn, double zo, double yn) { add(r, s, w, z, y, wv, zn, zo, yn); }
};

}  // namespace admm
