// admm_dims_impl.hpp -- body shared by admm_dims_g*.hip.  The including file defines
//   ADMM_GROUP_FN    launch_groupK
//   ADMM_GROUP_LIST  dims_groupK
//   ADMM_GROUP_DIMS(X)   X(n, m) X(n, m) ...
//   ADMM_CERT_FN     launch_cert_groupK   (certificate kernels of the group's pairs, admm_cert_kernels.hpp)
//   ADMM_INFEAS_FN   launch_infeas_groupK (infeasibility kernels of the group's pairs, admm_infeas_kernels.hpp)
#include "admm_dispatch.hpp"
#include "admm_select.hpp"
#include "admm_kernels.hpp"
#include "admm_kernels_alt.hpp"
#include "admm_cert_kernels.hpp"
#include "admm_infeas_kernels.hpp"

namespace admm {

const char* ADMM_GROUP_LIST() { return ADMM_GROUP_DIMS(ADMM_DIM_NAME); }

namespace {

// One call site per kernel; which forms of it exist is written at that site (admm_select.hpp).  Adding a form = the kernel's
// template parameter, one more parameter of the lambda and its flag in the with_flags call (tests/golden/kernel_counts.json
// records the compiled set).
template <int NX, int NU>
void launch_dim(const XLaunch& l, XKernel k, bool a, bool b) {
  const dim3 grid = sweep_grid((l.pitch + XB_THREADS - 1) / XB_THREADS, l.S), block(XB_THREADS);
  const bool relax = l.alpha != 1.0;
  switch (k) {
    case XKernel::XB:
      with_flags([&](auto HQ, auto VF, auto soc) {
        constexpr bool SC = VF() && soc();       // the SOC form differs only where z is rebuilt from v (VFORM)
        hipLaunchKernelGGL((xb_kernel<NX, NU, HQ(), VF(), SC>), grid, block, 0, l.stream, VF() ? l.v : l.z, l.y, l.q, l.recB,
                           l.seg_start, l.dbuf, l.tseg, l.eseg, l.rho, l.pitch);
      }, l.has_q, a, l.has_soc);
      break;
    case XKernel::XF:
      hipLaunchKernelGGL((xf_kernel<NX, NU>), grid, block, 0, l.stream, l.dbuf, l.tin, l.xin, l.recF,
                         l.seg_start, l.w, l.pitch, l.nsplit, l.split_stride);
      break;
    case XKernel::XFZ:
      with_flags([&](auto RS, auto RX, auto VI, auto soc) {
        constexpr bool SC = (RS() || VI()) && soc();   // the SOC form matters where z is rebuilt from v (VIN) or z+ is formed (RESID)
        hipLaunchKernelGGL((xfz_kernel<NX, NU, RS(), RX(), VI(), SC>), grid, block, 0, l.stream, l.dbuf, l.tin, l.xin,
                           l.recF, l.seg_start, l.z, l.y, l.v, l.part, l.alpha, l.pitch, l.nsplit, l.split_stride);
      }, b, relax, a, l.has_soc);
      break;
    case XKernel::XSCAN_CHAIN:
      hipLaunchKernelGGL((xscan_kernel<NX>), dim3(l.pitch / 64), dim3(64), 0, l.stream, l.tseg, l.eseg, l.x0,
                         l.recS, l.tin, l.xin, l.S, l.pitch);
      break;
    case XKernel::XFZE:
    case XKernel::XBZE:
      if constexpr (alt_dims(NX, NU)) {
        with_flags([&](auto rs, auto rx, auto hq, auto sc) {
          constexpr bool RS = rs(), RX = rx(), HQ = hq(), SC = sc();
          // the scan's input / output slots are shared by both directions: (tseg, eseg) = (mseg, epsseg),
          // (tin, xin) = (m_in, x_end)
          auto form = [&](auto XF, auto LN) {
            if (k == XKernel::XFZE)
              hipLaunchKernelGGL((xfze_kernel<NX, NU, RS, RX, HQ, SC, XF(), LN()>), grid, block, 0, l.stream, l.dbuf, l.tin, l.xin,
                                 l.recFE, l.seg_start, l.q, l.v, l.mvec, l.tseg, l.eseg, l.part, l.alpha, l.rho,
                                 l.pitch, l.nsplit, l.split_stride, l.wu, l.xbnd);
            else
              hipLaunchKernelGGL((xbze_kernel<NX, NU, RS, RX, HQ, SC, XF(), LN()>), grid, block, 0, l.stream, l.mvec, l.tin, l.xin,
                                 l.recBE, l.seg_start, l.q, l.v, l.dbuf, l.tseg, l.eseg, l.part, l.alpha, l.rho,
                                 l.pitch, l.nsplit, l.split_stride, l.wu, l.xbnd);
          };
          auto full = [&](auto XF) { form(XF, int_c<0>{}); };
          // lean residual forms (l.lean = ALT_LEAN_SD | NR | NW, set by enqueue_one for the shapes of alt_lean_dims only)
          if constexpr (RS && !RX && !HQ && !SC && alt_lean_dims(NX, NU)) {
            if (with_int<4, 5, 6, 7>(l.lean, [&](auto LN) { form(int_c<1>{}, LN); })) return;
          }
          // XFREE forms (state rows unbounded everywhere: their v is not read -- 1 -- and, when the next iteration is of the
          // same kind, not written either -- 2) exist for the non-residual, non-relaxed kernels only ...
          if constexpr (!RS && !RX) with_int<0, 1, 2>(l.xfree == 2 ? 2 : l.xfree == 1 ? 1 : 0, full);
          // ... and 1 for the residual form with the state rows' shortcut: fp64-issue-bound blocks only
          else if constexpr (RS && !RX && NX + NU >= 12) with_int<0, 1>(l.xfree ? 1 : 0, full);
          else full(int_c<0>{});
        }, b, relax, l.has_q, l.has_soc);
      }
      break;
  }
}

}  // namespace

bool ADMM_GROUP_FN(const XLaunch& l, XKernel k, bool a, bool b, bool query_only) {
#define X(NX, NU)                               \
  if (l.n == NX && l.m == NU) {                 \
    if ((k == XKernel::XFZE || k == XKernel::XBZE) && !alt_dims(NX, NU)) return false; \
    if (!query_only) launch_dim<NX, NU>(l, k, a, b); \
    return true;                                \
  }
  ADMM_GROUP_DIMS(X)
#undef X
  return false;
}

bool ADMM_CERT_FN(const CertLaunch& l, bool query_only) {
#define X(NX, NU)                                \
  if (l.n == NX && l.m == NU) {                  \
    if (!query_only) launch_cert_dim<NX, NU>(l); \
    return true;                                 \
  }
  ADMM_GROUP_DIMS(X)
#undef X
  return false;
}

bool ADMM_INFEAS_FN(const InfeasLaunch& l, bool query_only) {
#define X(NX, NU)                                  \
  if (l.n == NX && l.m == NU) {                    \
    if (!query_only) launch_infeas_dim<NX, NU>(l); \
    return true;                                   \
  }
  ADMM_GROUP_DIMS(X)
#undef X
  return false;
}

}  // namespace admm
