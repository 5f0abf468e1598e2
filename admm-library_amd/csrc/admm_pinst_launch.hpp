// admm_pinst_launch.hpp -- the (n, m)-templated launcher of the per-instance kernels, shared by the translation units that
// instantiate them (admm_pinst.hip, admm_pinst_g1.hip: the shapes are split so that the build compiles them in parallel).
#pragma once

#include <atomic>

#include "admm_dispatch.hpp"
#include "admm_select.hpp"
#include "admm_pinst.hpp"
#include "admm_pinst_rows.hpp"
#include "admm_pinst_wide.hpp"

namespace admm {
namespace {

// Launch with dynamic LDS; beyond the 64 KB a kernel may use by default the limit is raised first (once per kernel and device).
template <auto Kernel, class... Args>
void launch_with_lds(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, Args... args) {
  if (lds_bytes > 64 * 1024) {
    static std::atomic<unsigned> raised{0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (!((raised.load(std::memory_order_relaxed) >> dev) & 1u)) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      raised.fetch_or(1u << dev, std::memory_order_relaxed);
    }
  }
  hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, stream, args...);
}

// Grid of the rows-over-lanes kernels: a wave serves QPW QPs; from 65 QPs on a workgroup takes the 16 / QPW waves whose
// accesses share the 128-byte lines of every array (their 8 * QPW-byte pieces would otherwise be fetched by different XCDs).
template <int NX>
struct RowsGrid {
  dim3 grid, block, grid1;     // grid1: without the segment dimension (factorisation)
  int waves_per_block;
  explicit RowsGrid(const PLaunch& l) {
    constexpr int QPW = PscanShape<NX>::QPW;
    const int wpb = l.pitch > 64 ? (16 / QPW > 1 ? 16 / QPW : 1) : 1;
    const int waves = l.pitch / QPW;
    block = dim3(PI_THREADS * wpb);
    waves_per_block = wpb;
    grid1 = dim3((waves + wpb - 1) / wpb);
    grid = dim3(grid1.x, l.S > 0 ? l.S : 1);
  }
};

// The rows-over-lanes sweeps, each written once for both launchers below.  WIDE: called for a wide shape's handle (or its twin):
// the bounds' tiled copies and the thrust bound are passed, and SOC selects the thrust-magnitude forms of the TILED kernels.
template <int NX, int NU, bool TILED, bool WIDE>
void launch_pxb_rows(const PLaunch& l, const RowsGrid<NX>& rg) {
  with_flags([&](auto HQ, auto VF, auto PB, auto SEG, auto soc) {
    constexpr bool SC = WIDE && TILED && VF() && soc();
    launch_with_lds<pxb_rows_kernel<NX, NU, HQ(), VF(), PB(), SEG(), TILED, SC>>(
        rg.grid, rg.block, TILED ? rg.waves_per_block * pxb_rows_lds_words<NX, NU, SEG()>() * sizeof(double) : 0, l.stream,
        VF() ? l.v : l.z, l.y, l.q, l.Ad, l.Bd, l.Kd, l.Sd, l.lo, l.hi, l.dbuf, l.rhov, l.N, l.pitch, SEG() ? l.Omd : nullptr,
        SEG() ? l.seg_start : nullptr, SEG() ? l.tseg : nullptr, SEG() ? l.eseg : nullptr, WIDE ? l.loT : nullptr,
        WIDE ? l.hiT : nullptr, WIDE ? l.ub : nullptr);
  }, l.has_q, l.vform, l.pbounds, l.S > 1, l.has_soc);
}

// zup = false: the read-out (w of the last x-update), one form per SEG
template <int NX, int NU, bool TILED, bool WIDE>
void launch_pxfz_rows(const PLaunch& l, const RowsGrid<NX>& rg, bool zup) {
  with_flags([&](auto ZUP, auto rs, auto rx, auto vi, auto pb, auto SEG, auto soc) {
    constexpr bool RS = ZUP() && rs(), RX = ZUP() && rx(), VI = ZUP() && vi(), PB = ZUP() && pb();
    constexpr bool SC = WIDE && TILED && (RS || VI) && soc();
    launch_with_lds<pxfz_rows_kernel<NX, NU, ZUP(), RS, RX, VI, PB, !ZUP(), SEG(), TILED, SC>>(
        rg.grid, rg.block, TILED ? rg.waves_per_block * pxfz_rows_lds_words<NX, NU, SEG()>() * sizeof(double) : 0, l.stream,
        l.dbuf, l.x0, l.Ad, l.Bd, l.Kd, l.lo, l.hi, l.z, l.y, l.v, l.w, l.part, l.alpha, l.N, l.pitch, SEG() ? l.Psd : nullptr,
        SEG() ? l.seg_start : nullptr, SEG() ? l.tin : nullptr, SEG() ? l.xin : nullptr, WIDE ? l.loT : nullptr,
        WIDE ? l.hiT : nullptr, WIDE ? l.ub : nullptr);
  }, zup, l.resid, l.alpha != 1.0, l.vform, l.pbounds, l.S > 1, l.has_soc);
}

// Wide shapes (admm_pinst_wide.hpp): every kernel in its rows-over-lanes form.  TILED: the operand arrays in the tiled layout
// (admm_pinst.hpp, Operand) -- the wide shapes' handles; false = the twin at (6, 3) on a batch-minor handle.
template <int NX, int NU, bool TILED = true>
void launch_dim_wide(const PLaunch& l, PKernel k) {
  const RowsGrid<NX> rg(l);
  switch (k) {
    case PKernel::SEGMENTS:
      hipLaunchKernelGGL((pseg_rows_kernel<NX, NU, TILED>), rg.grid, rg.block, 0, l.stream, l.Ad, l.Bd, l.Kd, l.Sd, l.seg_start, l.todo,
                         l.Omd, l.Psd, l.Segd, l.grow, l.pitch, l.batch, l.qflag);
      break;
    case PKernel::SCAN:
      hipLaunchKernelGGL((pscan_kernel<NX>), dim3(l.pitch / PscanShape<NX>::QPW), dim3(PI_THREADS), 0, l.stream, l.Segd, l.tseg,
                         l.eseg, l.x0, l.tin, l.xin, l.S, l.pitch);
      break;
    case PKernel::FACTOR:
      hipLaunchKernelGGL((pfactor_rows_kernel<NX, NU, TILED>), rg.grid1, rg.block, 0, l.stream, l.Ad, l.Bd, l.Q, l.R, l.QN, l.rhov,
                         l.todo, l.Kd, l.Sd, l.fail, l.N, l.pitch, l.batch, l.qflag);
      break;
    case PKernel::XB: launch_pxb_rows<NX, NU, TILED, true>(l, rg); break;
    case PKernel::XF: launch_pxfz_rows<NX, NU, TILED, true>(l, rg, false); break;
    case PKernel::XFZ: launch_pxfz_rows<NX, NU, TILED, true>(l, rg, true); break;
  }
}

// One-lane shapes: a QP per lane; l.rows: the sweeps in their rows-over-lanes form (batch-minor operands, no thrust bound).
template <int NX, int NU>
void launch_dim(const PLaunch& l, PKernel k) {
  const dim3 grid((l.pitch + PI_THREADS - 1) / PI_THREADS), block(PI_THREADS);
  const dim3 sgrid((l.pitch + PI_THREADS - 1) / PI_THREADS, l.S > 0 ? l.S : 1);     // one wave per (64 QPs, segment)
  const RowsGrid<NX> rg(l);                                                          // rows over lanes: QPW QPs per wave
  switch (k) {
    case PKernel::SEGMENTS:
      hipLaunchKernelGGL((pseg_kernel<NX, NU>), sgrid, block, 0, l.stream, l.Ad, l.Bd, l.Kd, l.Sd, l.seg_start, l.todo, l.Omd,
                         l.Psd, l.Segd, l.grow, l.pitch, l.batch, l.qflag);
      break;
    case PKernel::SCAN:
      hipLaunchKernelGGL((pscan_kernel<NX>), dim3(l.pitch / PscanShape<NX>::QPW), block, 0, l.stream, l.Segd, l.tseg, l.eseg, l.x0,
                         l.tin, l.xin, l.S, l.pitch);
      break;
    case PKernel::FACTOR:
      hipLaunchKernelGGL((pfactor_kernel<NX, NU>), grid, block, 0, l.stream, l.Ad, l.Bd, l.Q, l.R, l.QN, l.rhov, l.todo, l.Kd, l.Sd,
                         l.fail, l.N, l.pitch, l.batch, l.qflag);
      break;
    case PKernel::XB:
      if (l.rows) return launch_pxb_rows<NX, NU, false, false>(l, rg);
      with_flags([&](auto HQ, auto VF, auto PB, auto SEG, auto soc) {
        constexpr bool SC = VF() && soc();       // the (z, y) form carries the projected z: only the v-form projects
        hipLaunchKernelGGL((pxb_kernel<NX, NU, HQ(), VF(), PB(), SEG(), SC>), SEG() ? sgrid : grid, block, 0, l.stream,
                           VF() ? l.v : l.z, l.y, l.q, l.Ad, l.Bd, l.Kd, l.Sd, l.lo, l.hi, l.dbuf, l.rhov, l.N, l.pitch,
                           SEG() ? l.Omd : nullptr, SEG() ? l.seg_start : nullptr, SEG() ? l.tseg : nullptr,
                           SEG() ? l.eseg : nullptr, SC ? l.ub : nullptr);
      }, l.has_q, l.vform, l.pbounds, l.S > 1, l.has_soc);
      break;
    case PKernel::XF:       // read-out: w of the last x-update
    case PKernel::XFZ:
      if (l.rows) return launch_pxfz_rows<NX, NU, false, false>(l, rg, k == PKernel::XFZ);
      with_flags([&](auto ZUP, auto rs, auto rx, auto vi, auto pb, auto SEG, auto soc) {
        constexpr bool RS = ZUP() && rs(), RX = ZUP() && rx(), VI = ZUP() && vi(), PB = ZUP() && pb(), SC = ZUP() && soc();
        hipLaunchKernelGGL((pxfz_kernel<NX, NU, ZUP(), RS, RX, VI, PB, !ZUP(), SEG(), SC>), SEG() ? sgrid : grid, block, 0, l.stream,
                           l.dbuf, l.x0, l.Ad, l.Bd, l.Kd, l.lo, l.hi, l.z, l.y, l.v, l.w, l.part, l.alpha, l.N, l.pitch,
                           SEG() ? l.Psd : nullptr, SEG() ? l.seg_start : nullptr, SEG() ? l.tin : nullptr,
                           SEG() ? l.xin : nullptr, SC ? l.ub : nullptr);
      }, k == PKernel::XFZ, l.resid, l.alpha != 1.0, l.vform, l.pbounds, l.S > 1, l.has_soc);
      break;
  }
}

}  // namespace

}  // namespace admm

// bool launch_pinst_<group>(l, k, query_only) over the X(n, m) list DIMS with LAUNCH<n, m>(l, k) (launch_dim or launch_dim_wide),
// and the group's " (n,m) ..." string
#define ADMM_PINST_GROUP(NAME, DIMS, LAUNCH)                                \
  namespace admm {                                                          \
  bool launch_pinst_##NAME(const PLaunch& l, PKernel k, bool query_only) {  \
    auto launch = [&](auto NX, auto NU) { LAUNCH<NX(), NU()>(l, k); };      \
    DIMS(ADMM_PINST_TRY)                                                    \
    return false;                                                           \
  }                                                                         \
  const char* dims_pinst_##NAME() { return DIMS(ADMM_DIM_NAME); }           \
  }
#define ADMM_PINST_TRY(NX, NU)                                  \
  if (l.n == NX && l.m == NU) {                                 \
    if (!query_only) launch(int_c<NX>{}, int_c<NU>{});          \
    return true;                                                \
  }
