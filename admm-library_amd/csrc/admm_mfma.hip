// MFMA form of the fused iteration kernels (admm_mfma.hpp): instantiations and launcher.
// Adding a shape = adding X(n, m) to ADMM_MFMA_DIMS (n <= 12, m <= 8).
// Adding a form = a flag of the with_flags call in launch_dim and its line in `exists` (admm_select.hpp).
#include "admm_dispatch.hpp"
#include "admm_select.hpp"
#include "admm_mfma.hpp"

#define ADMM_MFMA_DIMS(X) X(12, 6) X(6, 3) X(10, 4)

namespace admm {

const char* dims_mfma() { return ADMM_MFMA_DIMS(ADMM_DIM_NAME); }

namespace {

template <int NX, int NU>
bool launch_dim(const XLaunch& l, XKernel k, bool resid, bool query_only) {
  const bool mixed = l.mfma_mode == 1;
  // mode 2 (fp64): the alternating pair; mode 1 (mixed): the pair, and the plain path's v-form kernels (xb / xfz roles)
  const bool pair = k == XKernel::XFZE || k == XKernel::XBZE, forward = k == XKernel::XFZE || k == XKernel::XFZ;
  if (!pair && !(mixed && (k == XKernel::XB || k == XKernel::XFZ))) return false;
  if (query_only) return true;
  // one 16-QP tile per wave for small batches (waves beyond the batch idle), two otherwise
  const bool nt1 = l.pitch <= 128;
  const dim3 grid = sweep_grid((l.pitch + mf_cols(nt1 ? 1 : 2) - 1) / mf_cols(nt1 ? 1 : 2), l.S), block(MF_THREADS);
  // A linear term q: HASQ forms of the fp64 alternating pair with one tile per wave (small batches), for the shape of the
  // successive-convexification QPs only -- every form doubles the compile time of this unit, and at n = 12 the extra
  // prefetch registers do not fit under the 256-register cap of two waves per SIMD.  (admm_setup picks the one-lane kernels
  // for every other problem with q.)
  if (l.has_q && !(NX == 6 && NU == 3 && nt1 && !mixed && pair)) return false;
  const bool plain_xb = k == XKernel::XB;      // the plain path's backward sweep: one form
  with_flags([&](auto nt1_, auto mx, auto rs, auto rx, auto pr, auto hq) {
    constexpr int NT = nt1_() ? 1 : 2;
    constexpr bool RS = rs(), RX = rx(), PAIR = pr(), HQ = hq();
    using TM = std::conditional_t<mx(), float, double>;      // mixed: fp32 substitution (forward) / elimination (backward)
    constexpr bool exists = HQ ? NX == 6 && NU == 3 && NT == 1 && !mx() && PAIR : PAIR || mx();
    if constexpr (exists) {
      with_int<0, 1, 2>(l.xfree == 2 ? 2 : l.xfree == 1 ? 1 : 0, [&](auto xf) {
        // XFREE forms for the non-residual, non-relaxed kernels that update v (not the plain path's backward sweep)
        constexpr int XF = !RS && !RX ? xf() : 0;
        if (forward) {        // PAIR = ELIM
          hipLaunchKernelGGL((xfzem_kernel<NX, NU, NT, TM, double, RS, RX, PAIR, XF, HQ>), grid, block, 0, l.stream, l.dbuf, l.tin,
                             l.xin, l.recMF, l.seg_start, l.v, l.mvec, l.tseg, l.eseg, l.part, l.alpha, l.rho, l.pitch, l.nsplit,
                             l.split_stride, l.batch, HQ ? l.q : nullptr);
        } else if constexpr (PAIR || (!RS && !RX && !HQ)) {      // PAIR = SUBST
          hipLaunchKernelGGL((xbzem_kernel<NX, NU, NT, double, TM, RS, RX, PAIR, PAIR ? XF : 0, HQ>), grid, block, 0, l.stream,
                             l.mvec, l.tin, l.xin, l.recMB, l.seg_start, l.v, l.dbuf, l.tseg, l.eseg, l.part, l.alpha, l.rho,
                             l.pitch, l.nsplit, l.split_stride, l.batch, HQ ? l.q : nullptr);
        }
      });
    }
  }, nt1, mixed, resid && !plain_xb, l.alpha != 1.0 && !plain_xb, pair, l.has_q);
  return true;
}

}  // namespace

bool launch_mfma(const XLaunch& l, XKernel k, bool resid, bool query_only) {
#define X(NX, NU) if (l.n == NX && l.m == NU) return launch_dim<NX, NU>(l, k, resid, query_only);
  ADMM_MFMA_DIMS(X)
#undef X
  return false;
}

}  // namespace admm
