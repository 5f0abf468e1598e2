// admm_setup.hip -- set-up of a handle (admm_runtime.hpp): what an entry point asks for (SetupRequest), the steps setup_common runs in
// order, and every admm_setup* entry point of include/admm_hip.h.  The first failing check decides the message.
#include "admm_runtime.hpp"
#include "admm_consensus.hpp"

using namespace admm::rt;

namespace {

// What a set-up entry point asks for, filled in by field name.  ts_n > 0: a time shard (admm_setup_timeshard).  src = Mem::Device
// (admm_setup_device): p is a DeviceProblem's view -- small arrays on the host, the per-instance ones device memory, checked by the
// device-side findings `scan`.  One z-update kind per request: only the payload of `zkind` is read.
struct SetupRequest {
  SetupRequest(const admm_problem* p_, const admm_options* o_) : p(p_) {
    if (o_) o = *o_; else admm_default_options(&o);
  }
  const admm_problem* p;
  admm_options o;
  int ts_rank = 0, ts_n = 0;
  admm_exchange_fn ts_fn = nullptr;
  void* ts_ctx = nullptr;
  Mem src = Mem::Host;
  const DeviceScan* scan = nullptr;
  const double* fuel = nullptr;  // the weights of the minimum-fuel term, in unorm's shape; NULL = none (composes with every kind)
  ZKind zkind = ZKind::Box;
  int group = 0;                 // Consensus: QPs per scenario group
  const double* soft = nullptr;  // Soft: the weights of the soft box, in lo's shape
  // Halfspace: a[b][k][i], b[b][k] of one half-space per stage on the first hs_nh state rows (one "QP" unless hs_perqp);
  // hs_any: the stages with a plane for some QP, filled by check_setup_request
  const double *hs_a = nullptr, *hs_b = nullptr;
  int hs_nh = 0;
  bool hs_perqp = false;
  std::vector<char> hs_any;
  // Cone: c[b][k][i], apex[b][k][i], gamma[b][k] of one approach cone per stage on the first cone_nh state rows (one "QP" unless
  // cone_perqp); cone_any: the stages with a cone for some QP, filled by check_setup_request
  const double *cone_c = nullptr, *cone_p = nullptr, *cone_g = nullptr;
  int cone_nh = 0;
  bool cone_perqp = false;
  std::vector<char> cone_any;
};

// options and problem data, then what a fuel term, the z-update kind and time shards each exclude
int check_setup_request(SetupRequest& r) {
  const admm_problem* p = r.p;
  admm_options& o = r.o;
  int rc;
  if ((rc = validate_options(&o))) return rc;
  if ((rc = validate_problem(p, r.scan))) return rc;
  if (r.fuel) {
    if ((rc = validate_fuel(p, r.fuel, false))) return rc;
    // the shrink-and-scale projection is built into the one-lane fp64 kernels of batch-shared dynamics only
    if (p->time_varying == 2) return fail(ADMM_ERR_UNSUPPORTED, "a fuel term needs batch-shared dynamics (time_varying = 0 or 1)");
    if (o.precision_mode != ADMM_PRECISION_FP64)
      return fail(ADMM_ERR_UNSUPPORTED, "precision_mode " + std::to_string(o.precision_mode) + ": a fuel term is not supported by the MFMA forms (use ADMM_PRECISION_FP64)");
    if (r.ts_n) return fail(ADMM_ERR_UNSUPPORTED, "a fuel term is not supported on time-sharded handles");
  }
  if (r.zkind != ZKind::Box) {
    const ZKindInfo& k = zkind_info(r.zkind);
    const std::string fn = std::string(k.setup) + ": ";
    // (the group size is reported before the shared rules: the order of the messages is behaviour)
    if (r.zkind == ZKind::Consensus && (r.group < 1 || p->batch % r.group != 0))
      return fail(ADMM_ERR_INVALID, fn + "group_size " + std::to_string(r.group) + " must be >= 1 and divide batch = " + std::to_string(p->batch));
    // every extension exists as the standalone z kernel of the one-lane fp64 path of batch-shared dynamics only ...
    if (p->time_varying == 2) return fail(ADMM_ERR_UNSUPPORTED, fn + k.needs + " batch-shared dynamics (time_varying = 0 or 1)");
    if (o.precision_mode != ADMM_PRECISION_FP64)
      return fail(ADMM_ERR_UNSUPPORTED, fn + "precision_mode " + std::to_string(o.precision_mode) + ": " + k.is_not + " supported by the MFMA forms (use ADMM_PRECISION_FP64)");
    if (r.zkind == ZKind::Consensus) {
      if (p->m > admm::CONS_MAX_M)
        return fail(ADMM_ERR_UNSUPPORTED, fn + "m = " + std::to_string(p->m) + " exceeds " + std::to_string(admm::CONS_MAX_M) +
                                          " control rows (the LDS arrays of the group projection are sized for the compiled shapes)");
    } else if (r.zkind == ZKind::Soft) {
      std::vector<double> fk;
      if (r.fuel) { fk.resize(p->N); for (int k2 = 0; k2 < p->N; ++k2) fk[k2] = r.fuel[p->stage_bounds ? k2 : 0]; }
      if ((rc = validate_soft(p, r.soft, false, r.fuel ? fk.data() : nullptr))) return rc;
    } else if (r.zkind == ZKind::Cone) {
      if (r.cone_nh < 1 || r.cone_nh > p->n)
        return fail(ADMM_ERR_INVALID, fn + "nh = " + std::to_string(r.cone_nh) + " must lie in 1 .. n = " + std::to_string(p->n));
      if ((rc = cone_stages(k.setup, r.cone_c, r.cone_p, r.cone_g, r.cone_perqp ? p->batch : 1, p->N, r.cone_nh, r.cone_any)) ||
          (rc = halfspace_box_open(k.setup, p, r.cone_any, r.cone_nh, "a cone")))
        return rc;
    } else {
      if (r.hs_nh < 1 || r.hs_nh > p->n)
        return fail(ADMM_ERR_INVALID, fn + "nh = " + std::to_string(r.hs_nh) + " must lie in 1 .. n = " + std::to_string(p->n));
      if ((rc = halfspace_stages(k.setup, r.hs_a, r.hs_b, r.hs_perqp ? p->batch : 1, p->N, r.hs_nh, r.hs_any)) ||
          (rc = halfspace_box_open(k.setup, p, r.hs_any, r.hs_nh)))
        return rc;
    }
    // (no time-sharded form: admm_setup_timeshard takes no payload, so the combination cannot be asked for here)
    // ... and runs on the (z, y) pair, never the v-form: the v -> (z, y) read-out kernels know only the per-QP, per-row hard prox
    o.flags |= ADMM_FLAG_UNFUSED;
  }
  if (r.ts_n) {
    if (r.ts_n < 1 || r.ts_rank < 0 || r.ts_rank >= r.ts_n) return fail(ADMM_ERR_INVALID, "admm_setup_timeshard: need 0 <= rank < nranks");
    if (r.ts_n > 1 && !r.ts_fn) return fail(ADMM_ERR_INVALID, "admm_setup_timeshard: an exchange function is needed with more than one rank");
    if (p->time_varying == 2) return fail(ADMM_ERR_UNSUPPORTED, "time-sharded handles need batch-shared dynamics");
    if (o.flags & (ADMM_FLAG_UNFUSED | ADMM_FLAG_GRAPH | ADMM_FLAG_SCAN_CHAIN))
      return fail(ADMM_ERR_UNSUPPORTED, "time-sharded handles run the fused paths with direct launches (no ADMM_FLAG_UNFUSED / _GRAPH / _SCAN_CHAIN)");
    if (o.segments % r.ts_n != 0) return fail(ADMM_ERR_INVALID, "admm_setup_timeshard: options.segments (the total) must be a multiple of nranks");
    if (p->N < r.ts_n) return fail(ADMM_ERR_INVALID, "admm_setup_timeshard: fewer stages than ranks");
  }
  if (!dims_supported(p->n, p->m))
    return fail(ADMM_ERR_UNSUPPORTED, "(n, m) = (" + std::to_string(p->n) + ", " + std::to_string(p->m) +
                                          ") has no compiled kernel; supported: " + supported_list());
  return ADMM_OK;
}

// the device of options.device (< 0: the current one), made current
int pick_device(int asked, int* dev) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(ADMM_ERR_NO_DEVICE, "no HIP device visible: libadmm_hip has no CPU fallback");
  *dev = asked;
  if (*dev < 0) HIP_TRY(hipGetDevice(dev));
  if (*dev >= ndev) return fail(ADMM_ERR_INVALID, "device ordinal out of range");
  HIP_TRY(hipSetDevice(*dev));
  return ADMM_OK;
}

// the handle's copy of the request: sizes, options, the z-update kind with its payload, weights
void init_handle(admm_handle* h, const SetupRequest& r, int dev) {
  const admm_problem* p = r.p;
  h->device = dev;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) h->num_cus = prop.multiProcessorCount;
  h->opt = r.o;
  h->ts_n = r.ts_n; h->ts_rank = r.ts_rank; h->ts_fn = r.ts_fn; h->ts_ctx = r.ts_ctx;
  h->N = p->N; h->n = p->n; h->m = p->m; h->nb = p->n + p->m; h->batch = p->batch;
  h->L = p->N * h->nb;
  h->wk0 = 0; h->wk1 = p->N;           // stage window of the big arrays: the whole horizon unless this becomes a time shard (alloc_shared)
  h->pitch = ((p->batch + 63) / 64) * 64;
  h->has_q = p->q != nullptr;
  h->has_soc = problem_has_soc(p) || r.fuel != nullptr;    // a fuel handle runs the SOC forms with or without a thrust bound
  h->zkind = r.zkind;
  switch (r.zkind) {
    case ZKind::Box: break;
    case ZKind::Consensus: h->cons_G = r.group; break;
    case ZKind::Soft:
      h->soft.resize(h->L);
      for (int e = 0; e < h->L; ++e) h->soft[e] = r.soft[(p->stage_bounds ? (size_t)(e / h->nb) * h->nb : 0) + e % h->nb];
      break;
    case ZKind::Halfspace:
      h->hs_nh = r.hs_nh;
      h->hs_perqp = r.hs_perqp;
      h->hs_any = r.hs_any;
      break;
    case ZKind::Cone:
      h->cone_nh = r.cone_nh;
      h->cone_perqp = r.cone_perqp;
      h->cone_any = r.cone_any;
      break;
  }
  if (r.fuel) {
    h->has_fuel = true;
    h->fuel.resize(p->N);
    for (int k = 0; k < p->N; ++k) h->fuel[k] = r.fuel[p->stage_bounds ? k : 0];
  }
}

// x-update segments: ONE workgroup (256 columns x one segment) per CU -- the grid
// ceil(pitch / 256) x S should fill the 256 CUs once and not spill into a ragged second round
// (measured, DESIGN.md §4.6: pitch 4160 with S = 16 is 272 workgroups and runs 1.45x slower per
// QP than pitch 4096; S = 15 = 255 workgroups restores the rate).  The x kernels run as fast at
// one wave per SIMD as at two, and the scan's work grows with S^2, so fewer, longer segments win.
void choose_segments(admm_handle* h) {
  const int ts_n = h->ts_n;
  int S = h->opt.segments;
  if (S == 0) {
    const int col_blocks = (h->pitch + admm::XB_THREADS - 1) / admm::XB_THREADS;
    S = h->num_cus / col_blocks;
    // (a lone wave per segment is latency-bound at ~2.2 us per stage: with up to 64 QPs shorter segments
    //  pay -- N = 200, batch 1: 24.9 -> 19.9 us per iteration at S = 50 instead of 25; beyond 64 segments
    //  the host-side factorisation -- 80 ms at S = 125 -- costs more than a solve saves)
    const int per_seg = h->pitch <= 64 ? 4 : 8;
    const int max_by_len = h->N >= 2 * per_seg ? h->N / per_seg : 1;
    if (S > max_by_len) S = max_by_len;
    if (S > 64) S = 64;
    // a segment of the state must stay below the 2 GiB a buffer descriptor can span (with margin)
    const double total = (double)h->N * h->nb * h->pitch * 8.0;
    const int min_by_span = (int)(total / 1.9e9) + 1;
    if (S < min_by_span) S = min_by_span;
  }
  if (ts_n) {               // time shards: the rule above gives the segments of ONE rank's grid; the horizon gets nranks times as many
    if (h->opt.segments == 0) {
      const int max_total = h->N >= 16 ? h->N / 8 : h->N;
      S = std::max(1, std::min(S, max_total / ts_n)) * ts_n;
    }
    if (S > h->N) S = (h->N / ts_n) * ts_n;
  }
  if (S > h->N) S = h->N;
  if (S < 1) S = 1;
  h->S = S;
}

}  // namespace

namespace admm {
namespace rt {

// z-kernel chunking: ONE workgroup per CU (256 workgroups), rows per chunk a multiple of 4.
// Measured on configs[2]: 2000 workgroups 265 us, 504 -> 255 us, 256 -> 245 us,
// 200 -> 244 us, 360 -> 280 us (a ragged second round), 128 -> 301 us: few long-running
// workgroups, each streaming consecutive rows, and a grid that fills the CUs exactly once.
// zrows: options.zrows, 0 = this rule (setup_pinst: always, for its shared-bounds read-out kernel).
void choose_zchunks(admm_handle* h, int zrows) {
  const bool groups = h->zkind == ZKind::Consensus;
  int zr = zrows;
  if (zr == 0) {
    const int col_groups = groups ? admm::consensus_col_groups(h->batch, h->cons_G, h->m)      // whole groups per workgroup
                                  : (h->pitch / 2 + Z_THREADS - 1) / Z_THREADS;
    // (the consensus kernel synchronises per block and holds two workgroups per CU, whose barriers then overlap; a group wider
    //  than a workgroup's tile is walked by ONE workgroup, tile by tile, and wants twice as many, shorter chunks: DESIGN.md §2.12)
    const int wg_per_cu = !groups ? 1 : admm::consensus_wide(h->cons_G, h->m) ? 4 : 2;
    int chunks = (wg_per_cu * h->num_cus + col_groups - 1) / col_groups;
    if (chunks < 1) chunks = 1;
    zr = (h->L + chunks - 1) / chunks;
    zr = ((zr + 3) / 4) * 4;
    if (zr < 4) zr = 4;
  }
  if (h->has_soc || zkind_info(h->zkind).whole_blocks) zr = ((zr + h->nb - 1) / h->nb) * h->nb;   // block-structured kernels: whole blocks per chunk
  h->zrows = zr;
  h->zchunks = (h->L + zr - 1) / zr;
}

}  // namespace rt
}  // namespace admm

namespace {

// precision mode: the MFMA forms exist for a few (n, m), without q / thrust-magnitude bound
int choose_precision(admm_handle* h) {
  const admm_options& o = h->opt;
  admm::XLaunch lq{};
  lq.n = h->n; lq.m = h->m;
  lq.mfma_mode = o.precision_mode == ADMM_PRECISION_MIXED ? 1 : 2;
  const bool compiled = admm::mfma_dims(h->n, h->m) && admm::launch_mfma(lq, admm::XKernel::XFZE, false, true);
  std::string why;
  if (!compiled) why = "(n, m) has no MFMA instantiation; compiled: " + std::string(admm::dims_mfma());
  else if (h->has_q && !(h->n == 6 && h->m == 3 && h->pitch <= 128 && o.precision_mode != ADMM_PRECISION_MIXED))
    why = "a linear term q is supported by the fp64 MFMA forms of (6, 3) for batches of up to 128 QPs only";
  else if (h->has_soc) why = "a thrust-magnitude bound or fuel term is not supported by the MFMA forms";
  else if (o.flags & (ADMM_FLAG_UNFUSED | ADMM_FLAG_SCAN_CHAIN)) why = "ADMM_FLAG_UNFUSED / ADMM_FLAG_SCAN_CHAIN exclude the MFMA forms";
  if (o.precision_mode != ADMM_PRECISION_FP64) {
    if (!why.empty()) return fail(ADMM_ERR_UNSUPPORTED, "precision_mode " + std::to_string(o.precision_mode) + ": " + why);
    h->mfma_mode = lq.mfma_mode;
  } else if (why.empty() && !(o.flags & (ADMM_FLAG_NO_MFMA | ADMM_FLAG_NO_ALTERNATE)) &&
             (h->pitch <= 64 || (h->n >= 9 && h->pitch <= 128))) {
    // FP64: the fp64 MFMA form where it is the faster one (ADMM_FLAG_NO_MFMA).  Measured, round 3 (tools/family_time.py;
    // one-lane kernels with the operators distributed over the lanes, dpp_matvec_acc): the MFMA form wins for the
    // smallest batches only -- one wave per segment running ~15 MFMAs per stage instead of a few hundred dependent FMAs --
    // (6, 3): 22 vs 33 us per iteration for one QP, 27 vs 35 at 64 QPs, level at 128, 59 vs 41 at 256, 187 vs 151 at 4096;
    // (12, 6): 34 vs 72 us for one QP, 42 vs 76 at 64, 103 vs 95 at 256, 343 vs 315 at 4096.
    h->mfma_mode = 2;
  }
  // batches of a few QPs run the scan as a matrix-vector product (xscan_gemv_kernel) and need no MFMA-packed scan matrices
  h->scan_gemv = h->batch <= admm::SCAN_GEMV_MAXCOLS && !(o.flags & ADMM_FLAG_SCAN_CHAIN) &&
                 std::getenv("ADMM_NO_GEMV_SCAN") == nullptr;
  return ADMM_OK;
}

// The host factorisation at the chosen segment count, under the conditioning guard of the parallel-in-time form: the segment
// coupling is exact in exact arithmetic, but its transfer matrices are products of closed-loop matrices, and for a barely
// stabilised plant (tiny rho, no state cost, unstable A) their entries grow with the number of
// segments and amplify rounding (measured: max|W| 1e3 -> 1e-5 relative error in w, against
// 1e-14 for the workloads of DESIGN.md §3 where max|W| is O(1)).  With an automatic segment
// count, fall back to fewer, longer segments until the growth is benign.  Sets h->S (and a time shard's segment range).
int factor_with_guard(admm_handle* h, const admm_problem* p) {
  const admm_options& o = h->opt;
  const int ts_n = h->ts_n;
  std::string err;
  int rc = admm::factorise(*p, o.rho, h->S, h->fac, err, h->mfma_mode, !h->scan_gemv, ts_n, fuel_of(h));
  if (rc) return fail(rc, err);
  h->auto_segments = o.segments == 0;
  if (o.segments == 0 && ts_n && h->fac.S > ts_n && scan_growth(h->fac) > SCAN_GROWTH_MAX)      // (every rank must arrive at the same count: no silent back-off here)
    return fail(ADMM_ERR_NUMERIC, "admm_setup_timeshard: the segment transfer matrices grow beyond the conditioning bound with the "
                                  "automatic segment count; give options.segments (a multiple of nranks)");
  if (o.segments == 0 && !ts_n) {
    while (h->fac.S > 1 && scan_growth(h->fac) > SCAN_GROWTH_MAX) {
      const int S2 = std::max(1, h->fac.S / 2);
      rc = admm::factorise(*p, o.rho, S2, h->fac, err, h->mfma_mode, !h->scan_gemv, 0, fuel_of(h));
      if (rc) return fail(rc, err);
    }
  }
  h->S = h->fac.S;
  if (ts_n) {
    if (h->S % ts_n != 0) return fail(ADMM_ERR_INVALID, "admm_setup_timeshard: the segment count " + std::to_string(h->S) + " is not a multiple of nranks");
    h->ts_sl = h->S / ts_n;
    h->ts_s0 = h->ts_rank * h->ts_sl;
  }
  // the x kernels address one segment of an array through a 32-bit buffer descriptor
  int longest = 0;
  for (int s = 0; s < h->S; ++s) longest = std::max(longest, h->fac.seg_start[s + 1] - h->fac.seg_start[s]);
  if ((double)longest * h->nb * h->pitch * 8.0 >= 2147483648.0)
    return fail(ADMM_ERR_UNSUPPORTED, "one segment of the state exceeds 2 GiB: use more segments or a smaller batch per GPU");
  return ADMM_OK;
}

// what follows from the factor: the alternating-direction iteration (compiled for this (n, m), buildable for this problem, not
// disabled), whether launch_x routes to the MFMA form, the split-K factor of the scan
void choose_kernel_forms(admm_handle* h) {
  h->alt_requested = fused(h) && !(h->opt.flags & (ADMM_FLAG_SCAN_CHAIN | ADMM_FLAG_NO_ALTERNATE)) &&
                     dispatch_x(xlaunch_of(h), admm::XKernel::XFZE, false, false, /*query_only=*/true);
  h->alt = h->alt_allowed = h->fac.alt_ok && h->alt_requested;
  if (h->alt_requested && !h->fac.alt_ok) warn_alt_gate(h->fac, h->opt.rho, "admm_setup");
  h->mfma_on = h->mfma_mode != 0 && (h->opt.precision_mode == ADMM_PRECISION_MIXED || h->alt);
  // split-K of the scan when the grid would be small: aim at >= 256 workgroups, <= 8 slices
  const int wgs = (h->pitch / 64) * (h->fac.scanM / 16 / admm::SCAN_MT);
  int sp = 1;
  while (sp < 8 && wgs * sp < h->num_cus) sp *= 2;
  const int ksteps = h->fac.scanK / 4;
  while (sp > 1 && ksteps / sp < 2 * admm::SCAN_U) sp /= 2;     // at least two batches per slice
  if (const char* e = std::getenv("ADMM_SCAN_SPLIT")) {           // tuning override (1, 2, 4, 8)
    const int v = std::atoi(e);
    if (v == 1 || v == 2 || v == 4 || v == 8) sp = v;
  }
  if (h->scan_gemv) sp = 1;                        // the matrix-vector form writes whole sums
  h->scan_split = sp;
}

// the stream and every device array of a batch-shared handle; state and work arrays zeroed
int alloc_shared(admm_handle* h) {
  HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  const size_t P = h->pitch, L = h->L;
  const admm::Factor& f = h->fac;
  // the stage window of the big arrays: a time shard of several ranks holds its own stages only (admm_runtime.hpp)
  if (h->ts_n > 1 && std::getenv("ADMM_TS_FULL_ARRAYS") == nullptr) { h->wk0 = f.seg_start[h->ts_s0]; h->wk1 = f.seg_start[h->ts_s0 + h->ts_sl]; }
  const size_t Lw = win_rows(h), Nmw = (size_t)(h->wk1 - h->wk0) * h->m, bias = win_bias(h), bias_m = win_bias_m(h);
  // a per-stage array of the window: the field holds the allocation biased by the window's first row (h->owned keeps its address)
  auto win = [h](double** field, size_t count, size_t bias_, bool zeroed) {
    const int rc_ = dalloc(h, field, count, zeroed);
    if (!rc_) *field -= bias_;
    return rc_;
  };
  int rc;
  if ((rc = win(&h->w, Lw * P, bias, true)) || (rc = win(&h->z, Lw * P, bias, true)) || (rc = win(&h->y, Lw * P, bias, true)) ||
      (rc = win(&h->v, Lw * P, bias, true)) || (h->has_q && (rc = win(&h->q, Lw * P, bias, false))) ||
      (rc = win(&h->dbuf, Nmw * P, bias_m, true)))
    return rc;
  // scan operands: in = tseg | x0 | eseg | pad,  out = t_in | pad | x_in | pad  (admm_factor.hpp)
  if ((rc = dalloc(h, &h->scan_in, (size_t)f.scanK * P, true)) || (rc = dalloc(h, &h->scan_out, (size_t)h->scan_split * f.scanM * P, true)) ||
      (rc = dalloc(h, &h->scanWp, f.scanWp.size())) || (rc = dalloc(h, &h->scan_range, f.scanRange.size())))
    return rc;
  if (h->scan_gemv && ((rc = dalloc(h, &h->scanWd, f.scanW.size())) || (rc = dalloc(h, &h->scanWBd, f.scanW.size())) ||
                       (rc = dalloc(h, &h->scan_rows, (size_t)2 * f.scanM)) || (rc = dalloc(h, &h->scan_rowsB, (size_t)2 * f.scanM))))
    return rc;
  const size_t Sn = (size_t)h->S * h->n;
  h->tseg = h->scan_in;
  h->x0 = h->scan_in + Sn * P;
  h->eseg = h->scan_in + (Sn + h->n) * P;
  if (f.ts_ranks > 1) {     // time shards: rank-by-rank input rows (admm_factor.hpp); tseg / eseg = THIS rank's block
    const size_t blk = (size_t)2 * h->ts_sl * h->n;
    h->tseg = h->scan_in + (size_t)h->ts_rank * blk * P;
    h->eseg = h->tseg + (size_t)h->ts_sl * h->n * P;
    h->x0 = h->scan_in + 2 * Sn * P;
  }
  h->tin = h->scan_out;
  h->xin = h->scan_out + (size_t)f.scanMt * P;
  // MFMA fragment records (the LDS-DMA copy of a chunk moves whole KiB pieces, admm_mfma.hpp), status arrays of a MIXED solve's phase 1
  if (h->mfma_mode && ((rc = dalloc_records(h, &h->recMF, f.recMF.size())) || (rc = dalloc_records(h, &h->recMB, f.recMB.size())) ||
                       (!f.recMF64.empty() && ((rc = dalloc_records(h, &h->recMF64, f.recMF64.size())) ||
                                               (rc = dalloc_records(h, &h->recMB64, f.recMB64.size())))) ||
                       (rc = dalloc(h, &h->status1, P)) || (rc = dalloc(h, &h->iters1, P))))
    return rc;
  if (h->alt_allowed) {
    // (records: the fused kernels copy a chunk in whole KiB pieces, admm_kernels.hpp glds_chunk; mvec: db rows of the forward elimination)
    if ((rc = dalloc_records(h, &h->recFE, sizeof(double) * f.recFE.size(), &h->recFE_bytes)) ||
        (rc = dalloc_records(h, &h->recBE, sizeof(double) * f.recBE.size(), &h->recBE_bytes)) ||
        (rc = dalloc(h, &h->scanWpB, f.scanWpB.size())) || (rc = dalloc(h, &h->scan_rangeB, f.scanRangeB.size())) ||
        (rc = win(&h->mvec, Nmw * P, bias_m, true)))
      return rc;
    if (admm::alt_lean_dims(h->n, h->m) && !h->ts_n &&         // side data of the lean residual forms (admm_kernels_alt.hpp)
        ((rc = win(&h->wu, Nmw * P, bias_m, true)) || (rc = dalloc(h, &h->xbnd, (size_t)h->S * h->n * P, true))))
      return rc;
  }
  const size_t part_chunks = (size_t)(h->zchunks > h->S ? h->zchunks : h->S);
  const size_t hs_cols = h->hs_perqp ? P : 1;        // the planes: shared, or one set per QP (batch-minor)
  const size_t cone_cols = h->cone_perqp ? P : 1;    // the cones likewise
  h->stage_rows = Lw;
  if ((rc = dalloc(h, &h->part, part_chunks * 5 * P, true)) || (rc = dalloc(h, &h->resid, 5 * P, true)) ||
      (rc = dalloc(h, &h->lo, L)) || (rc = dalloc(h, &h->hi, L)) || (rc = dalloc(h, &h->ub, (size_t)h->N)) || (rc = dalloc(h, &h->kap, (size_t)h->N)) ||
      (h->zkind == ZKind::Soft && ((rc = dalloc(h, &h->soft_d, L)) || (rc = dalloc(h, &h->skap_d, L)))) ||
      (h->zkind == ZKind::Halfspace && ((rc = dalloc(h, &h->hs_a, (size_t)h->N * h->hs_nh * hs_cols, true)) ||
                                        (rc = dalloc(h, &h->hs_b, (size_t)h->N * hs_cols, true)))) ||
      (h->zkind == ZKind::Cone && ((rc = dalloc(h, &h->cone_c, (size_t)h->N * h->cone_nh * cone_cols, true)) ||
                                   (rc = dalloc(h, &h->cone_p, (size_t)h->N * h->cone_nh * cone_cols, true)) ||
                                   (rc = dalloc(h, &h->cone_g, (size_t)h->N * cone_cols, true)))) ||
      (rc = dalloc(h, &h->recB, f.recB.size())) || (rc = dalloc(h, &h->recF, f.recF.size())) || (rc = dalloc(h, &h->recS, f.recS.size())) ||
      (rc = dalloc(h, &h->seg_start, f.seg_start.size())) || (rc = dalloc(h, &h->status, P, true)) || (rc = dalloc(h, &h->iters, P, true)) ||
      (rc = dalloc(h, &h->nconv, 1)) || (rc = dalloc(h, &h->stage, Lw * (size_t)h->batch)))
    return rc;
  // the fills are asynchronous on the handle's NON-BLOCKING stream; the uploads of the factor are synchronous copies on the null
  // stream, which does not wait for it (see setup_pinst): no copy may land before the fill of its array
  HIP_TRY(hipStreamSynchronize(h->stream));
  return halloc(h, &h->h_nconv, 1);
}

int setup_common(admm_handle** out, SetupRequest& r) {
  if (!out || !r.p) return fail(ADMM_ERR_INVALID, "NULL argument");
  *out = nullptr;
  g_warn.clear();
  const admm_problem* p = r.p;
  int rc, dev;
  if ((rc = check_setup_request(r)) || (rc = pick_device(r.o.device, &dev))) return rc;
  HandleGuard guard(new admm_handle());          // released, with its memory, by every early return below
  admm_handle* h = guard.get();
  init_handle(h, r, dev);
  if ((h->opt.flags & ADMM_FLAG_ROW_MAJOR) && p->time_varying != 2)
    return fail(ADMM_ERR_UNSUPPORTED, "ADMM_FLAG_ROW_MAJOR: per-instance dynamics only (time_varying = 2)");
  if (p->time_varying == 2) {                    // per-instance dynamics: its own set-up (device factorisation)
    if ((rc = setup_pinst(h, p, r.src))) return rc;
    *out = guard.release();
    return ADMM_OK;
  }
  choose_segments(h);
  choose_zchunks(h, h->opt.zrows);
  if ((rc = choose_precision(h)) || (rc = factor_with_guard(h, p))) return rc;
  keep_shared(h, p);     // host copy of the shared problem data, for admm_set_rho / the adaptive rule
  choose_kernel_forms(h);
  if ((rc = alloc_shared(h))) return rc;
  if ((rc = upload_bounds(h, p)) || (rc = upload_factor(h, "admm_setup"))) return rc;
  HIP_TRY(hipMemcpy(h->seg_start, h->fac.seg_start.data(), sizeof(int32_t) * h->fac.seg_start.size(), hipMemcpyHostToDevice));
  if ((rc = upload_transposed(h, r.src, p->x0, h->x0, h->n))) return rc;
  if (h->has_q && (rc = upload_transposed(h, r.src, p->q, h->q, h->L))) return rc;
  if (h->zkind == ZKind::Halfspace && (rc = upload_halfspace(h, Mem::Host, r.hs_a, r.hs_b))) return rc;
  if (h->zkind == ZKind::Cone && (rc = upload_cone(h, Mem::Host, r.cone_c, r.cone_p, r.cone_g))) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  *out = guard.release();
  return ADMM_OK;
}

}  // namespace

extern "C" {

void admm_default_options(admm_options* o) {
  if (!o) return;
  o->rho = 0.1;
  o->alpha = 1.0;
  o->eps_abs = 1e-6;
  o->eps_rel = 1e-6;
  o->max_iter = 4000;
  o->check_interval = 10;
  o->segments = 0;
  o->device = -1;
  o->zrows = 0;
  o->flags = ADMM_FLAG_NONE;
  o->adapt_interval = 0;
  o->adapt_max = 16;
  o->adapt_mu = 10.0;
  o->adapt_tau = 2.0;
  o->precision_mode = ADMM_PRECISION_FP64;
  o->reserved = 0;
}

int admm_setup(admm_handle** out, const admm_problem* p, const admm_options* o) {
  SetupRequest r(p, o);
  return setup_common(out, r);
}

int admm_setup_fuel(admm_handle** out, const admm_problem* p, const admm_options* o, const double* fuel) {
  SetupRequest r(p, o);
  r.fuel = fuel;
  return setup_common(out, r);
}

// Scenario consensus: admm_setup_fuel with groups of group_size adjacent QPs sharing their control rows.
int admm_setup_consensus(admm_handle** out, const admm_problem* p, const admm_options* o, const double* fuel, int32_t group_size) {
  if (out) *out = nullptr;
  if (group_size < 1) return fail(ADMM_ERR_INVALID, "admm_setup_consensus: group_size " + std::to_string(group_size) + " must be >= 1 and divide batch");
  SetupRequest r(p, o);
  r.fuel = fuel;
  r.zkind = ZKind::Consensus;
  r.group = group_size;
  return setup_common(out, r);
}

// Soft box constraints: admm_setup_fuel with a weight per row of the box; the z-update is zdual_soft_kernel.
int admm_setup_soft(admm_handle** out, const admm_problem* p, const admm_options* o, const double* fuel, const double* soft) {
  if (out) *out = nullptr;
  if (!soft) return fail(ADMM_ERR_INVALID, "admm_setup_soft: soft must not be NULL (admm_setup / admm_setup_fuel set up a handle without weights)");
  SetupRequest r(p, o);
  r.fuel = fuel;
  r.zkind = ZKind::Soft;
  r.soft = soft;
  return setup_common(out, r);
}

// One half-space per stage: admm_setup_fuel with a' xi <= b on the first nh state rows of every block; the
// z-update is zdual_halfspace_kernel.
int admm_setup_halfspace(admm_handle** out, const admm_problem* p, const admm_options* o, const double* fuel, const double* a,
                         const double* b, int32_t nh, int32_t per_instance) {
  if (out) *out = nullptr;
  if (!a || !b) return fail(ADMM_ERR_INVALID, "admm_setup_halfspace: a and b must not be NULL (admm_setup / admm_setup_fuel set up a handle without half-spaces)");
  if (nh < 1) return fail(ADMM_ERR_INVALID, "admm_setup_halfspace: nh = " + std::to_string(nh) + " must lie in 1 .. n");
  SetupRequest r(p, o);
  r.fuel = fuel;
  r.zkind = ZKind::Halfspace;
  r.hs_a = a; r.hs_b = b; r.hs_nh = nh; r.hs_perqp = per_instance != 0;
  return setup_common(out, r);
}

// One approach cone per stage: admm_setup_fuel with the second-order cone of axis c, apex `apex` and slope gamma on
// the first nh state rows of every block; the z-update is zdual_cone_kernel.
int admm_setup_cone(admm_handle** out, const admm_problem* p, const admm_options* o, const double* fuel, const double* c,
                    const double* apex, const double* gamma, int32_t nh, int32_t per_instance) {
  if (out) *out = nullptr;
  if (!c || !apex || !gamma)
    return fail(ADMM_ERR_INVALID, "admm_setup_cone: c, apex and gamma must not be NULL (admm_setup / admm_setup_fuel set up a handle without approach cones)");
  if (nh < 1) return fail(ADMM_ERR_INVALID, "admm_setup_cone: nh = " + std::to_string(nh) + " must lie in 1 .. n");
  SetupRequest r(p, o);
  r.fuel = fuel;
  r.zkind = ZKind::Cone;
  r.cone_c = c; r.cone_p = apex; r.cone_g = gamma; r.cone_nh = nh; r.cone_perqp = per_instance != 0;
  return setup_common(out, r);
}

int admm_setup_device(admm_handle** out, const admm_problem* p, const admm_options* o, void* hip_stream) {
  if (!out || !p) return fail(ADMM_ERR_INVALID, "NULL argument");
  *out = nullptr;
  g_warn.clear();
  admm_options oo;
  if (o) oo = *o; else admm_default_options(&oo);
  int rc;
  if ((rc = validate_options(&oo)) || (rc = validate_dims(p))) return rc;
  int dev;
  if ((rc = pick_device(oo.device, &dev))) return rc;
  oo.device = dev;
  // the checks run on the caller's stream (ordered after its writes; the handle and its stream do not exist yet) and synchronise it,
  // so the handle's uploads below read finished data
  unsigned long long* scratch = nullptr;
  if ((rc = dalloc(&scratch, CHK_SLOTS))) return rc;
  DeviceProblem d;
  rc = prepare_device_problem(dev, static_cast<hipStream_t>(hip_stream), p, "admm_setup_device", scratch, d);
  (void)hipFree(scratch);
  if (rc) return rc;
  SetupRequest r(&d.hp, &oo);
  r.src = Mem::Device;
  r.scan = &d.scan;
  return setup_common(out, r);
}

int admm_setup_timeshard(admm_handle** out, const admm_problem* p, const admm_options* o, int32_t rank, int32_t nranks,
                         admm_exchange_fn exchange, void* ctx) {
  if (nranks < 1) return fail(ADMM_ERR_INVALID, "admm_setup_timeshard: nranks must be >= 1");
  SetupRequest r(p, o);
  r.ts_rank = rank; r.ts_n = nranks; r.ts_fn = exchange; r.ts_ctx = ctx;
  return setup_common(out, r);
}

}  // extern "C"
