// admm_api.hip -- C ABI of libadmm_hip.so (include/admm_hip.h): set-up, state, iteration, solve, read-out.  The runtime behind it is split over
// admm_launch.hip, admm_hostio.hip, admm_rho_update.hip, admm_pinst_rt.hip, admm_profile.hip (admm_runtime.hpp).  No CPU fallback: without a HIP device
// every compute entry point returns ADMM_ERR_NO_DEVICE.
#include "admm_runtime.hpp"
#include "admm_cert.hpp"
#include "admm_consensus.hpp"
#include "admm_infeas.hpp"
#include "admm_soft.hpp"
#include "admm_halfspace.hpp"


using namespace admm::rt;

// ---- set-up of a handle, step by step (setup_common below runs them in this order; the first failing check decides the message) ----
namespace admm {
namespace rt {

// What a set-up entry point asks for.  ts_n > 0: a time shard (admm_setup_timeshard).  src = Mem::Device (admm_setup_device): p is a
// DeviceProblem's view -- small arrays on the host, the per-instance ones device memory, checked by the device-side findings `scan`.
struct SetupRequest {
  const admm_problem* p;
  admm_options o;
  int ts_rank, ts_n;
  admm_exchange_fn ts_fn;
  void* ts_ctx;
  Mem src;
  const DeviceScan* scan;
  const double* fuel;            // admm_setup_fuel: the weights of the minimum-fuel term, in unorm's shape; NULL = none
  int group;                     // admm_setup_consensus: QPs per scenario group, 0 = a handle without groups
  const double* soft;            // admm_setup_soft: the weights of the soft box, in lo's shape; NULL = none
  // admm_setup_halfspace: a[b][k][i], b[b][k] of one half-space per stage on the first hs_nh state rows (one "QP" unless hs_perqp);
  // hs_nh = 0: none.  hs_any: the stages with a plane for some QP, filled by check_setup_request
  const double *hs_a = nullptr, *hs_b = nullptr;
  int hs_nh = 0;
  bool hs_perqp = false;
  std::vector<char> hs_any;
};

// options and problem data, then what a fuel term, scenario groups, soft weights and time shards each exclude (the standalone z
// kernels of groups and soft weights force ADMM_FLAG_UNFUSED into r.o)
static int check_setup_request(SetupRequest& r) {
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
  if (r.group) {
    // the group projection exists as the standalone z kernel of the one-lane fp64 path of batch-shared dynamics only
    if (r.group < 1 || p->batch % r.group != 0)
      return fail(ADMM_ERR_INVALID, "admm_setup_consensus: group_size " + std::to_string(r.group) + " must be >= 1 and divide batch = " + std::to_string(p->batch));
    if (p->time_varying == 2) return fail(ADMM_ERR_UNSUPPORTED, "admm_setup_consensus: scenario consensus needs batch-shared dynamics (time_varying = 0 or 1)");
    if (o.precision_mode != ADMM_PRECISION_FP64)
      return fail(ADMM_ERR_UNSUPPORTED, "admm_setup_consensus: precision_mode " + std::to_string(o.precision_mode) + ": scenario consensus is not supported by the MFMA forms (use ADMM_PRECISION_FP64)");
    if (p->m > admm::CONS_MAX_M)
      return fail(ADMM_ERR_UNSUPPORTED, "admm_setup_consensus: m = " + std::to_string(p->m) + " exceeds " + std::to_string(admm::CONS_MAX_M) +
                                        " control rows (the LDS arrays of the group projection are sized for the compiled shapes)");
    // (no time-sharded form: admm_setup_timeshard takes no group size, so the combination cannot be asked for here)
    o.flags |= ADMM_FLAG_UNFUSED;      // the (z, y) pair, never the v-form: the v -> (z, y) read-out kernels know only the per-QP prox
  }
  if (r.soft) {
    // the soft prox exists as the standalone z kernel of the one-lane fp64 path of batch-shared dynamics only
    if (p->time_varying == 2) return fail(ADMM_ERR_UNSUPPORTED, "admm_setup_soft: soft constraints need batch-shared dynamics (time_varying = 0 or 1)");
    if (o.precision_mode != ADMM_PRECISION_FP64)
      return fail(ADMM_ERR_UNSUPPORTED, "admm_setup_soft: precision_mode " + std::to_string(o.precision_mode) + ": soft constraints are not supported by the MFMA forms (use ADMM_PRECISION_FP64)");
    std::vector<double> fk;
    if (r.fuel) { fk.resize(p->N); for (int k = 0; k < p->N; ++k) fk[k] = r.fuel[p->stage_bounds ? k : 0]; }
    if ((rc = validate_soft(p, r.soft, false, r.fuel ? fk.data() : nullptr))) return rc;
    // (no time-sharded or consensus form: neither admm_setup_timeshard nor admm_setup_consensus takes weights)
    o.flags |= ADMM_FLAG_UNFUSED;      // the (z, y) pair, never the v-form: the v -> (z, y) read-out kernels know only the hard prox
  }
  if (r.hs_nh) {
    // the projection exists as the standalone z kernel of the one-lane fp64 path of batch-shared dynamics only
    if (p->time_varying == 2) return fail(ADMM_ERR_UNSUPPORTED, "admm_setup_halfspace: half-spaces need batch-shared dynamics (time_varying = 0 or 1)");
    if (o.precision_mode != ADMM_PRECISION_FP64)
      return fail(ADMM_ERR_UNSUPPORTED, "admm_setup_halfspace: precision_mode " + std::to_string(o.precision_mode) + ": half-spaces are not supported by the MFMA forms (use ADMM_PRECISION_FP64)");
    if (r.hs_nh < 1 || r.hs_nh > p->n)
      return fail(ADMM_ERR_INVALID, "admm_setup_halfspace: nh = " + std::to_string(r.hs_nh) + " must lie in 1 .. n = " + std::to_string(p->n));
    if ((rc = halfspace_stages("admm_setup_halfspace", r.hs_a, r.hs_b, r.hs_perqp ? p->batch : 1, p->N, r.hs_nh, r.hs_any)) ||
        (rc = halfspace_box_open("admm_setup_halfspace", p, r.hs_any, r.hs_nh)))
      return rc;
    // (no time-sharded, consensus or soft form: none of those set-up calls takes planes)
    o.flags |= ADMM_FLAG_UNFUSED;      // the (z, y) pair, never the v-form: the v -> (z, y) read-out kernels know only the per-row prox
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
static int pick_device(int asked, int* dev) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(ADMM_ERR_NO_DEVICE, "no HIP device visible: libadmm_hip has no CPU fallback");
  *dev = asked;
  if (*dev < 0) HIP_TRY(hipGetDevice(dev));
  if (*dev >= ndev) return fail(ADMM_ERR_INVALID, "device ordinal out of range");
  HIP_TRY(hipSetDevice(*dev));
  return ADMM_OK;
}

// the handle's copy of the request: sizes, options, weights
static void init_handle(admm_handle* h, const SetupRequest& r, int dev) {
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
  h->cons_G = r.group;
  h->hs_nh = r.hs_nh;
  h->hs_perqp = r.hs_perqp;
  h->hs_any = r.hs_any;
  if (r.soft) {
    h->has_soft = true;
    h->soft.resize(h->L);
    for (int e = 0; e < h->L; ++e) h->soft[e] = r.soft[(p->stage_bounds ? (size_t)(e / h->nb) * h->nb : 0) + e % h->nb];
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
static void choose_segments(admm_handle* h) {
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

// z-kernel chunking: ONE workgroup per CU (256 workgroups), rows per chunk a multiple of 4.
// Measured on configs[2]: 2000 workgroups 265 us, 504 -> 255 us, 256 -> 245 us,
// 200 -> 244 us, 360 -> 280 us (a ragged second round), 128 -> 301 us: few long-running
// workgroups, each streaming consecutive rows, and a grid that fills the CUs exactly once.
// zrows: options.zrows, 0 = this rule (setup_pinst: always, for its shared-bounds read-out kernel).
void choose_zchunks(admm_handle* h, int zrows) {
  int zr = zrows;
  if (zr == 0) {
    const int col_groups = h->cons_G ? admm::consensus_col_groups(h->batch, h->cons_G, h->m)      // whole groups per workgroup
                                     : (h->pitch / 2 + Z_THREADS - 1) / Z_THREADS;
    // (the consensus kernel synchronises per block and holds two workgroups per CU, whose barriers then overlap; a group wider
    //  than a workgroup's tile is walked by ONE workgroup, tile by tile, and wants twice as many, shorter chunks: DESIGN.md §2.12)
    const int wg_per_cu = !h->cons_G ? 1 : admm::consensus_wide(h->cons_G, h->m) ? 4 : 2;
    int chunks = (wg_per_cu * h->num_cus + col_groups - 1) / col_groups;
    if (chunks < 1) chunks = 1;
    zr = (h->L + chunks - 1) / chunks;
    zr = ((zr + 3) / 4) * 4;
    if (zr < 4) zr = 4;
  }
  if (h->has_soc || h->cons_G || h->hs_nh) zr = ((zr + h->nb - 1) / h->nb) * h->nb;   // block-structured kernels: whole blocks per chunk (also with soft weights)
  h->zrows = zr;
  h->zchunks = (h->L + zr - 1) / zr;
}

// precision mode: the MFMA forms exist for a few (n, m), without q / thrust-magnitude bound
static int choose_precision(admm_handle* h) {
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
static int factor_with_guard(admm_handle* h, const admm_problem* p) {
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
static void choose_kernel_forms(admm_handle* h) {
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
static int alloc_shared(admm_handle* h) {
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
  h->stage_rows = Lw;
  if ((rc = dalloc(h, &h->part, part_chunks * 5 * P, true)) || (rc = dalloc(h, &h->resid, 5 * P, true)) ||
      (rc = dalloc(h, &h->lo, L)) || (rc = dalloc(h, &h->hi, L)) || (rc = dalloc(h, &h->ub, (size_t)h->N)) || (rc = dalloc(h, &h->kap, (size_t)h->N)) ||
      (h->has_soft && ((rc = dalloc(h, &h->soft_d, L)) || (rc = dalloc(h, &h->skap_d, L)))) ||
      (h->hs_nh && ((rc = dalloc(h, &h->hs_a, (size_t)h->N * h->hs_nh * (h->hs_perqp ? P : 1), true)) ||
                    (rc = dalloc(h, &h->hs_b, (size_t)h->N * (h->hs_perqp ? P : 1), true)))) ||
      (rc = dalloc(h, &h->recB, f.recB.size())) || (rc = dalloc(h, &h->recF, f.recF.size())) || (rc = dalloc(h, &h->recS, f.recS.size())) ||
      (rc = dalloc(h, &h->seg_start, f.seg_start.size())) || (rc = dalloc(h, &h->status, P, true)) || (rc = dalloc(h, &h->iters, P, true)) ||
      (rc = dalloc(h, &h->nconv, 1)) || (rc = dalloc(h, &h->stage, Lw * (size_t)h->batch)))
    return rc;
  // the fills are asynchronous on the handle's NON-BLOCKING stream; the uploads of the factor are synchronous copies on the null
  // stream, which does not wait for it (see setup_pinst): no copy may land before the fill of its array
  HIP_TRY(hipStreamSynchronize(h->stream));
  return halloc(h, &h->h_nconv, 1);
}

}  // namespace rt
}  // namespace admm

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

const char* admm_last_error(void) { return g_err.c_str(); }
const char* admm_last_warning(void) { return g_warn.c_str(); }
int admm_abi_version(void) { return ADMM_HIP_ABI_VERSION; }

int admm_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

int admm_record_sizes(int32_t n, int32_t m, int32_t* rb, int32_t* rf, int32_t* rs) {
  if (n < 1 || m < 1) return fail(ADMM_ERR_INVALID, "n, m must be positive");
  if (rb) *rb = admm::rec_b_size(n, m);
  if (rf) *rf = admm::rec_f_size(n, m);
  if (rs) *rs = admm::rec_s_size(n);
  return ADMM_OK;
}

int admm_host_factor(const admm_problem* p, double rho, int32_t segments, double* K, double* Sinv,
                     double* recB, double* recF, double* recS, int32_t* seg_start) {
  if (!p) return fail(ADMM_ERR_INVALID, "NULL problem");
  admm::Factor f;
  std::string err;
  int rc = admm::factorise(*p, rho, segments, f, err);
  if (rc) return fail(rc, err);
  if (K) std::memcpy(K, f.K.data(), sizeof(double) * f.K.size());
  if (Sinv) std::memcpy(Sinv, f.Sinv.data(), sizeof(double) * f.Sinv.size());
  if (recB) std::memcpy(recB, f.recB.data(), sizeof(double) * f.recB.size());
  if (recF) std::memcpy(recF, f.recF.data(), sizeof(double) * f.recF.size());
  if (recS) std::memcpy(recS, f.recS.data(), sizeof(double) * f.recS.size());
  if (seg_start) std::memcpy(seg_start, f.seg_start.data(), sizeof(int32_t) * f.seg_start.size());
  return ADMM_OK;
}

int admm_host_scan_matrix(const admm_problem* p, double rho, int32_t segments, double* W, int32_t* M,
                          int32_t* Mt, int32_t* K) {
  if (!p) return fail(ADMM_ERR_INVALID, "NULL problem");
  admm::Factor f;
  std::string err;
  int rc = admm::factorise(*p, rho, segments, f, err);
  if (rc) return fail(rc, err);
  if (M) *M = f.scanM;
  if (Mt) *Mt = f.scanMt;
  if (K) *K = f.scanK;
  if (W) std::memcpy(W, f.scanW.data(), sizeof(double) * f.scanW.size());
  return ADMM_OK;
}

int admm_host_scan_packed(const admm_problem* p, double rho, int32_t segments, int32_t backward, double* Wp, int32_t* range,
                          int32_t* sizes) {
  if (!p) return fail(ADMM_ERR_INVALID, "NULL problem");
  admm::Factor f;
  std::string err;
  int rc = admm::factorise(*p, rho, segments, f, err);
  if (rc) return fail(rc, err);
  const bool ok = !backward || f.alt_ok;
  if (sizes) {
    sizes[0] = f.scanM;
    sizes[1] = f.scanK;
    sizes[2] = f.scanM / 16 / admm::SCAN_MT;
    sizes[3] = ok ? 1 : 0;
  }
  if (!ok) {                       // (without `sizes` nothing would tell the caller that Wp / range were left alone)
    if (!sizes) return fail(ADMM_ERR_NUMERIC, "admm_host_scan_packed: the forward-elimination form could not be built for this problem");
    return ADMM_OK;
  }
  const std::vector<double>& wp = backward ? f.scanWpB : f.scanWp;
  const std::vector<int32_t>& rg = backward ? f.scanRangeB : f.scanRange;
  if (Wp) std::memcpy(Wp, wp.data(), sizeof(double) * wp.size());
  if (range) std::memcpy(range, rg.data(), sizeof(int32_t) * rg.size());
  return ADMM_OK;
}

int admm_host_scan_matrices_timeshard(const admm_problem* p, double rho, int32_t segments, int32_t nranks, double* W, double* WB,
                                      int32_t* ok) {
  if (!p || nranks < 1 || segments < 1 || segments % nranks != 0) return fail(ADMM_ERR_INVALID, "need segments >= 1, a multiple of nranks >= 1");
  admm::Factor f;
  std::string err;
  int rc = admm::factorise(*p, rho, segments, f, err, 0, true, nranks);
  if (rc) return fail(rc, err);
  if (W) std::memcpy(W, f.scanW.data(), sizeof(double) * f.scanW.size());
  if (ok) *ok = f.alt_ok ? 1 : 0;
  if (WB && f.alt_ok) std::memcpy(WB, f.scanWB.data(), sizeof(double) * f.scanWB.size());
  return ADMM_OK;
}

int admm_record_sizes_alt(int32_t n, int32_t m, int32_t* rfe, int32_t* rbe) {
  if (n < 1 || m < 1) return fail(ADMM_ERR_INVALID, "n, m must be positive");
  if (rfe) *rfe = admm::rec_fe_size(n, m);
  if (rbe) *rbe = admm::rec_be_size(n, m);
  return ADMM_OK;
}

int admm_record_alloc_check(int64_t alloc_bytes, int32_t stages, int32_t stage_bytes, int64_t* needed) {
  if (alloc_bytes < 0 || stages < 0 || stage_bytes < 0) return fail(ADMM_ERR_INVALID, "sizes must not be negative");
  if (needed) *needed = (int64_t)rec_alloc_needed((size_t)stages, (size_t)stage_bytes);
  return check_record_alloc("admm_record_alloc_check", (size_t)alloc_bytes, (size_t)stages, (size_t)stage_bytes);
}

int admm_host_factor_alt(const admm_problem* p, double rho, int32_t segments, double* recFE, double* recBE,
                         double* WB, int32_t* ok) {
  if (!p) return fail(ADMM_ERR_INVALID, "NULL problem");
  admm::Factor f;
  std::string err;
  int rc = admm::factorise(*p, rho, segments, f, err);
  if (rc) return fail(rc, err);
  if (ok) *ok = f.alt_ok ? 1 : 0;
  if (!f.alt_ok) return ADMM_OK;
  if (recFE) std::memcpy(recFE, f.recFE.data(), sizeof(double) * f.recFE.size());
  if (recBE) std::memcpy(recBE, f.recBE.data(), sizeof(double) * f.recBE.size());
  if (WB) std::memcpy(WB, f.scanWB.data(), sizeof(double) * f.scanWB.size());
  return ADMM_OK;
}

int admm_mfma_record_bytes(int32_t n, int32_t m, int32_t mode, int32_t* fwd, int32_t* bwd) {
  if (!admm::mfma_dims(n, m)) return fail(ADMM_ERR_UNSUPPORTED, "the MFMA form needs 1 <= n <= 12 and 1 <= m <= 8");
  if (mode != 1 && mode != 2) return fail(ADMM_ERR_INVALID, "mode must be ADMM_PRECISION_MIXED or ADMM_PRECISION_FP64_MFMA");
  if (fwd) *fwd = admm::mfma_rec_bytes_fwd(n, m, mode);
  if (bwd) *bwd = admm::mfma_rec_bytes_bwd(n, m, mode);
  return ADMM_OK;
}

int admm_host_factor_mfma(const admm_problem* p, double rho, int32_t segments, int32_t mode, void* recMF,
                          void* recMB, int32_t* alt_ok) {
  if (!p) return fail(ADMM_ERR_INVALID, "NULL problem");
  if (mode != 1 && mode != 2) return fail(ADMM_ERR_INVALID, "mode must be ADMM_PRECISION_MIXED or ADMM_PRECISION_FP64_MFMA");
  admm::Factor f;
  std::string err;
  int rc = admm::factorise(*p, rho, segments, f, err, mode);
  if (rc) return fail(rc, err);
  if (recMF) std::memcpy(recMF, f.recMF.data(), f.recMF.size());
  if (recMB) std::memcpy(recMB, f.recMB.data(), f.recMB.size());
  if (alt_ok) *alt_ok = f.alt_ok ? 1 : 0;
  return ADMM_OK;
}

// the planes of a half-space handle into h->hs_a / h->hs_b (their addresses never change): the shared form as it is, the per-QP
// form through the transposing upload.  Returns with the copies complete.
static int upload_halfspace(admm_handle* h, Mem mem, const double* a, const double* b) {
  int rc;
  if (h->hs_perqp) {
    if ((rc = upload_transposed(h, mem, a, h->hs_a, h->N * h->hs_nh)) || (rc = upload_transposed(h, mem, b, h->hs_b, h->N))) return rc;
    return ADMM_OK;
  }
  const hipMemcpyKind kind = mem == Mem::Device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HIP_TRY(hipMemcpyAsync(h->hs_a, a, sizeof(double) * (size_t)h->N * h->hs_nh, kind, h->stream));
  HIP_TRY(hipMemcpyAsync(h->hs_b, b, sizeof(double) * (size_t)h->N, kind, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return ADMM_OK;
}

// the planes of admm_setup_halfspace
struct HalfspaceArgs { const double *a, *b; int nh; bool perqp; };

static int setup_common(admm_handle** out, const admm_problem* p, const admm_options* o_in, int ts_rank, int ts_n,
                        admm_exchange_fn ts_fn, void* ts_ctx, Mem src = Mem::Host, const DeviceScan* scan = nullptr,
                        const double* fuel = nullptr, int group = 0, const double* soft = nullptr, const HalfspaceArgs* hs = nullptr) {
  if (!out || !p) return fail(ADMM_ERR_INVALID, "NULL argument");
  *out = nullptr;
  g_warn.clear();
  SetupRequest r{p, {}, ts_rank, ts_n, ts_fn, ts_ctx, src, scan, fuel, group, soft};
  if (hs) { r.hs_a = hs->a; r.hs_b = hs->b; r.hs_nh = hs->nh; r.hs_perqp = hs->perqp; }
  if (o_in) r.o = *o_in; else admm_default_options(&r.o);
  int rc, dev;
  if ((rc = check_setup_request(r)) || (rc = pick_device(r.o.device, &dev))) return rc;
  HandleGuard guard(new admm_handle());          // released, with its memory, by every early return below
  admm_handle* h = guard.get();
  init_handle(h, r, dev);
  if ((h->opt.flags & ADMM_FLAG_ROW_MAJOR) && p->time_varying != 2)
    return fail(ADMM_ERR_UNSUPPORTED, "ADMM_FLAG_ROW_MAJOR: per-instance dynamics only (time_varying = 2)");
  if (p->time_varying == 2) {                    // per-instance dynamics: its own set-up (device factorisation)
    if ((rc = setup_pinst(h, p, src))) return rc;
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
  if ((rc = upload_transposed(h, src, p->x0, h->x0, h->n))) return rc;
  if (h->has_q && (rc = upload_transposed(h, src, p->q, h->q, h->L))) return rc;
  if (h->hs_nh && (rc = upload_halfspace(h, Mem::Host, r.hs_a, r.hs_b))) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  *out = guard.release();
  return ADMM_OK;
}

int admm_setup(admm_handle** out, const admm_problem* p, const admm_options* o) {
  return setup_common(out, p, o, 0, 0, nullptr, nullptr);
}

int admm_setup_fuel(admm_handle** out, const admm_problem* p, const admm_options* o, const double* fuel) {
  return setup_common(out, p, o, 0, 0, nullptr, nullptr, Mem::Host, nullptr, fuel);
}

// Scenario consensus: admm_setup_fuel with groups of group_size adjacent QPs sharing their control rows.
int admm_setup_consensus(admm_handle** out, const admm_problem* p, const admm_options* o, const double* fuel, int32_t group_size) {
  if (out) *out = nullptr;
  if (group_size < 1) return fail(ADMM_ERR_INVALID, "admm_setup_consensus: group_size " + std::to_string(group_size) + " must be >= 1 and divide batch");
  return setup_common(out, p, o, 0, 0, nullptr, nullptr, Mem::Host, nullptr, fuel, group_size);
}

// Soft box constraints: admm_setup_fuel with a weight per row of the box; the z-update is zdual_soft_kernel.
int admm_setup_soft(admm_handle** out, const admm_problem* p, const admm_options* o, const double* fuel, const double* soft) {
  if (out) *out = nullptr;
  if (!soft) return fail(ADMM_ERR_INVALID, "admm_setup_soft: soft must not be NULL (admm_setup / admm_setup_fuel set up a handle without weights)");
  return setup_common(out, p, o, 0, 0, nullptr, nullptr, Mem::Host, nullptr, fuel, 0, soft);
}

int admm_get_soft(admm_handle* h, double* soft) {
  if (!h || !soft) return fail(ADMM_ERR_INVALID, "NULL argument");
  for (int e = 0; e < h->L; ++e) soft[e] = h->has_soft ? h->soft[e] : INFINITY;
  return ADMM_OK;
}

// New weights on a soft handle: nothing of the handle is written before every check has passed.  The state is the (z, y) pair
// already (such a handle never enters the v-form); the factor does not depend on the weights, so only kappa is refreshed.
int admm_set_soft(admm_handle* h, const double* soft) {
  if (!h || !soft) return fail(ADMM_ERR_INVALID, "NULL argument");
  g_warn.clear();
  if (!h->has_soft) return fail(ADMM_ERR_INVALID, "admm_set_soft: soft weights cannot be added to a handle (set it up with admm_setup_soft)");
  HIP_TRY(hipSetDevice(h->device));
  const admm_problem p = shared_problem(h);
  int rc;
  if ((rc = validate_soft(&p, soft, false, fuel_of(h)))) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));   // kernels of the old weights are done before kappa changes
  for (int e = 0; e < h->L; ++e) h->soft[e] = soft[(h->stage_bounds ? (size_t)(e / h->nb) * h->nb : 0) + e % h->nb];
  h->infeas_valid = false;                    // the probe's bound table opens the rows with a finite weight
  return upload_kappa(h);
}

// penalty, largest violation and violated rows of every QP at the handle's z (soft_report_kernel)
static int soft_report_common(admm_handle* h, double* penalty, double* max_violation, int32_t* n_violated, Mem mem, void* hip_stream) {
  const char* fn = mem == Mem::Device ? "admm_get_soft_report_device" : "admm_get_soft_report";
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  if (!penalty && !max_violation && !n_violated) return fail(ADMM_ERR_INVALID, std::string(fn) + ": at least one output must be given");
  if (!h->has_soft) return fail(ADMM_ERR_INVALID, std::string(fn) + ": the handle has no soft weights (set it up with admm_setup_soft)");
  HIP_TRY(hipSetDevice(h->device));
  CallerIO io(h, fn, mem, hip_stream);
  int rc;
  const size_t bsz = sizeof(double) * (size_t)h->batch, csz = sizeof(int32_t) * (size_t)h->batch;
  if ((rc = io.check_ptr(penalty, bsz, "penalty")) || (rc = io.check_ptr(max_violation, bsz, "max_violation")) ||
      (rc = io.check_ptr(n_violated, csz, "n_violated", sizeof(int32_t), "int32 entries")))
    return rc;
  if (!h->soft_out && (rc = dalloc(h, &h->soft_out, (size_t)2 * h->pitch))) return rc;
  if (!h->soft_cnt && (rc = dalloc(h, &h->soft_cnt, (size_t)h->pitch))) return rc;
  if ((rc = ensure_zy(h))) return rc;                   // the state as the (z, y) pair, as admm_get reads it
  if ((rc = io.begin())) return rc;
  admm::launch_soft_report(h->stream, h->z, h->lo, h->hi, h->soft_d, h->soft_out, h->soft_out + h->pitch, h->soft_cnt, h->L, h->pitch,
                           h->batch);
  HIP_TRY(hipGetLastError());
  if (penalty && (rc = io.copy_out(penalty, h->soft_out, bsz))) return rc;
  if (max_violation && (rc = io.copy_out(max_violation, h->soft_out + h->pitch, bsz))) return rc;
  if (n_violated && (rc = io.copy_out(n_violated, h->soft_cnt, csz))) return rc;
  return io.finish();
}

int admm_get_soft_report(admm_handle* h, double* penalty, double* max_violation, int32_t* n_violated) {
  return soft_report_common(h, penalty, max_violation, n_violated, Mem::Host, nullptr);
}
int admm_get_soft_report_device(admm_handle* h, double* penalty, double* max_violation, int32_t* n_violated, void* hip_stream) {
  return soft_report_common(h, penalty, max_violation, n_violated, Mem::Device, hip_stream);
}

// One half-space per stage: admm_setup_fuel with a' xi <= b on the first nh state rows of every block; the
// z-update is zdual_halfspace_kernel.
int admm_setup_halfspace(admm_handle** out, const admm_problem* p, const admm_options* o, const double* fuel, const double* a,
                         const double* b, int32_t nh, int32_t per_instance) {
  if (out) *out = nullptr;
  if (!a || !b) return fail(ADMM_ERR_INVALID, "admm_setup_halfspace: a and b must not be NULL (admm_setup / admm_setup_fuel set up a handle without half-spaces)");
  if (nh < 1) return fail(ADMM_ERR_INVALID, "admm_setup_halfspace: nh = " + std::to_string(nh) + " must lie in 1 .. n");
  const HalfspaceArgs hs{a, b, nh, per_instance != 0};
  return setup_common(out, p, o, 0, 0, nullptr, nullptr, Mem::Host, nullptr, fuel, 0, nullptr, &hs);
}

// New planes on a half-space handle, same form and nh: nothing of the handle is written before every check has passed.  The
// state is the (z, y) pair already (such a handle never enters the v-form) and the factor does not depend on the planes.
static int set_halfspace_common(admm_handle* h, const double* a, const double* b, Mem mem, void* hip_stream) {
  const char* fn = mem == Mem::Device ? "admm_set_halfspace_device" : "admm_set_halfspace";
  if (!h || !a || !b) return fail(ADMM_ERR_INVALID, "NULL argument");
  g_warn.clear();
  if (!h->hs_nh) return fail(ADMM_ERR_INVALID, std::string(fn) + ": half-spaces cannot be added to a handle (set it up with admm_setup_halfspace)");
  HIP_TRY(hipSetDevice(h->device));
  CallerIO io(h, fn, mem, hip_stream);
  const int cnt = h->hs_perqp ? h->batch : 1, N = h->N, nh = h->hs_nh;
  const size_t na = (size_t)cnt * N * nh, nbv = (size_t)cnt * N;
  int rc;
  if ((rc = io.check_ptr(a, na * sizeof(double), "a")) || (rc = io.check_ptr(b, nbv * sizeof(double), "b"))) return rc;
  std::vector<char> any;
  if (!io.dev()) {
    if ((rc = halfspace_stages(fn, a, b, cnt, N, nh, any))) return rc;
  } else {
    int bad;
    if ((rc = io.begin()) || (rc = io.check_finite({{a, na, "a"}, {b, nbv, "b"}}, &bad))) return rc;
    if (bad >= 0) return fail(ADMM_ERR_INVALID, std::string(fn) + ": non-finite entry in a or b");
    if (h->hs_perqp) {              // the device-side findings: which stages have a plane for some QP, and whether an a'a is unusable
      if (!h->hs_flags && (rc = dalloc(h, &h->hs_flags, (size_t)2 * N))) return rc;
      std::vector<int> fl((size_t)2 * N);
      HIP_TRY(hipMemsetAsync(h->hs_flags, 0, sizeof(int) * fl.size(), h->stream));
      admm::launch_halfspace_scan(h->stream, a, h->batch, N, nh, h->hs_flags, h->hs_flags + N);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(fl.data(), h->hs_flags, sizeof(int) * fl.size(), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(hipStreamSynchronize(h->stream));
      any.assign(N, 0);
      for (int k = 0; k < N; ++k) {
        if (fl[N + k]) return fail(ADMM_ERR_INVALID, std::string(fn) + ": a'a of stage " + std::to_string(k) + " is not a normal number (scale the row)");
        any[k] = fl[k] != 0;
      }
    } else {                        // the shared form is N (nh + 1) doubles: checked on the host, as a DeviceProblem's small arrays are
      std::vector<double> ah(na), bh(nbv);
      HIP_TRY(hipMemcpyAsync(ah.data(), a, sizeof(double) * na, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(hipMemcpyAsync(bh.data(), b, sizeof(double) * nbv, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(hipStreamSynchronize(h->stream));
      if ((rc = halfspace_stages(fn, ah.data(), bh.data(), 1, N, nh, any))) return rc;
    }
  }
  const admm_problem p = shared_problem(h);
  if ((rc = halfspace_box_open(fn, &p, any, nh))) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));   // kernels of the old planes are done before they change
  if ((rc = upload_halfspace(h, mem, a, b))) return rc;
  h->hs_any = any;
  return io.finish();
}

int admm_set_halfspace(admm_handle* h, const double* a, const double* b) { return set_halfspace_common(h, a, b, Mem::Host, nullptr); }
int admm_set_halfspace_device(admm_handle* h, const double* a, const double* b, void* hip_stream) {
  return set_halfspace_common(h, a, b, Mem::Device, hip_stream);
}

// the planes in force, in the caller's order (a[b][k][i], b[b][k]; one "QP" in the shared form)
int admm_get_halfspace(admm_handle* h, double* a, double* b) {
  if (!h || !a || !b) return fail(ADMM_ERR_INVALID, "NULL argument");
  if (!h->hs_nh) return fail(ADMM_ERR_INVALID, "admm_get_halfspace: the handle has no half-spaces (set it up with admm_setup_halfspace)");
  HIP_TRY(hipSetDevice(h->device));
  int rc;
  if (h->hs_perqp) {
    if ((rc = download_transposed(h, Mem::Host, h->hs_a, a, h->N * h->hs_nh))) return rc;
    return download_transposed(h, Mem::Host, h->hs_b, b, h->N);
  }
  HIP_TRY(hipMemcpyAsync(a, h->hs_a, sizeof(double) * (size_t)h->N * h->hs_nh, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(b, h->hs_b, sizeof(double) * (size_t)h->N, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return ADMM_OK;
}

// largest violation of a plane by w, the stages with a positive multiplier, and the multipliers (halfspace_report_kernel)
static int halfspace_report_common(admm_handle* h, double* max_violation, int32_t* n_active, double* lam, Mem mem, void* hip_stream) {
  const char* fn = mem == Mem::Device ? "admm_get_halfspace_report_device" : "admm_get_halfspace_report";
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  if (!max_violation && !n_active && !lam) return fail(ADMM_ERR_INVALID, std::string(fn) + ": at least one output must be given");
  if (!h->hs_nh) return fail(ADMM_ERR_INVALID, std::string(fn) + ": the handle has no half-spaces (set it up with admm_setup_halfspace)");
  HIP_TRY(hipSetDevice(h->device));
  CallerIO io(h, fn, mem, hip_stream);
  int rc;
  const size_t bsz = sizeof(double) * (size_t)h->batch, csz = sizeof(int32_t) * (size_t)h->batch;
  if ((rc = io.check_ptr(max_violation, bsz, "max_violation")) ||
      (rc = io.check_ptr(n_active, csz, "n_active", sizeof(int32_t), "int32 entries")) || (rc = io.check_ptr(lam, bsz * h->N, "lam")))
    return rc;
  if (!h->hs_out && (rc = dalloc(h, &h->hs_out, (size_t)h->pitch))) return rc;
  if (!h->hs_cnt && (rc = dalloc(h, &h->hs_cnt, (size_t)h->pitch))) return rc;
  if (lam && !h->hs_lam && (rc = dalloc(h, &h->hs_lam, (size_t)h->N * h->pitch, true))) return rc;
  if ((rc = ensure_w(h)) || (rc = ensure_zy(h))) return rc;      // w of the last x-update; the state as the (z, y) pair
  if ((rc = io.begin())) return rc;
  admm::launch_halfspace_report(h->stream, h->w, h->y, h->hs_a, h->hs_b, h->hs_out, h->hs_cnt, lam ? h->hs_lam : nullptr, h->fac.rho,
                                h->N, h->nb, h->m, h->hs_nh, h->pitch, h->batch, h->hs_perqp);
  HIP_TRY(hipGetLastError());
  if (max_violation && (rc = io.copy_out(max_violation, h->hs_out, bsz))) return rc;
  if (n_active && (rc = io.copy_out(n_active, h->hs_cnt, csz))) return rc;
  if (lam && (rc = download_transposed(h, mem, h->hs_lam, lam, h->N))) return rc;
  return io.finish();
}

int admm_get_halfspace_report(admm_handle* h, double* max_violation, int32_t* n_active, double* lam) {
  return halfspace_report_common(h, max_violation, n_active, lam, Mem::Host, nullptr);
}
int admm_get_halfspace_report_device(admm_handle* h, double* max_violation, int32_t* n_active, double* lam, void* hip_stream) {
  return halfspace_report_common(h, max_violation, n_active, lam, Mem::Device, hip_stream);
}

// the control rows of each group's z, (ngroups, N, m): column g * G of the rows j < m of every block (consensus_gather_kernel)
static int consensus_common(admm_handle* h, double* ubar, Mem mem, void* hip_stream) {
  const char* fn = mem == Mem::Device ? "admm_get_consensus_device" : "admm_get_consensus";
  if (!h || !ubar) return fail(ADMM_ERR_INVALID, "NULL argument");
  if (!h->cons_G) return fail(ADMM_ERR_INVALID, std::string(fn) + ": the handle has no scenario groups (set it up with admm_setup_consensus)");
  HIP_TRY(hipSetDevice(h->device));
  CallerIO io(h, fn, mem, hip_stream);
  int rc;
  const int ngroups = h->batch / h->cons_G;
  const size_t bytes = sizeof(double) * (size_t)ngroups * h->N * h->m;
  if ((rc = io.check_ptr(ubar, bytes, "ubar"))) return rc;
  if ((rc = ensure_zy(h))) return rc;                   // the state as the (z, y) pair, as admm_get reads it
  if ((rc = io.begin())) return rc;
  admm::launch_consensus_gather(h->stream, h->z, io.dev() ? ubar : h->stage, ngroups, h->cons_G, h->N, h->nb, h->m, h->pitch);
  HIP_TRY(hipGetLastError());
  if (!io.dev()) return download_d2h(h, ubar, h->stage, bytes);      // (returns with the copy complete)
  return io.finish();
}

int admm_get_consensus(admm_handle* h, double* ubar) { return consensus_common(h, ubar, Mem::Host, nullptr); }
int admm_get_consensus_device(admm_handle* h, double* ubar, void* hip_stream) { return consensus_common(h, ubar, Mem::Device, hip_stream); }

int admm_get_fuel(admm_handle* h, double* fuel) {
  if (!h || !fuel) return fail(ADMM_ERR_INVALID, "NULL argument");
  for (int k = 0; k < h->N; ++k) fuel[k] = h->has_fuel ? h->fuel[k] : 0.0;
  return ADMM_OK;
}

// New weights on a fuel handle: nothing of the handle is written before every check has passed.  The state is switched to the
// (z, y) pair (as admm_set_rho does): v alone would be read back through the NEW prox.
int admm_set_fuel(admm_handle* h, const double* fuel) {
  if (!h || !fuel) return fail(ADMM_ERR_INVALID, "NULL argument");
  g_warn.clear();
  if (!h->has_fuel) return fail(ADMM_ERR_INVALID, "admm_set_fuel: a fuel term cannot be added to a handle (set it up with admm_setup_fuel)");
  HIP_TRY(hipSetDevice(h->device));
  const admm_problem p = shared_problem(h);
  int rc;
  if ((rc = validate_fuel(&p, fuel, false))) return rc;
  if (h->has_soft) {                          // a stage that gains a fuel weight must not hold a finite soft weight on its control rows
    std::vector<double> fk(h->N);
    for (int k = 0; k < h->N; ++k) fk[k] = fuel[h->stage_bounds ? k : 0];
    if ((rc = validate_soft(&p, h->soft.data(), true, fk.data()))) return rc;
  }
  if ((rc = ensure_w(h))) return rc;          // w of the last x-update belongs to the old records
  if ((rc = ensure_zy(h))) return rc;
  h->zy_valid = true;
  h->v_valid = false;
  drop_side_data(h);
  HIP_TRY(hipStreamSynchronize(h->stream));   // kernels of the old weights are done before the records change
  h->spec.clear();                            // candidate factors of the adaptive rule carry the old weights (joins their threads)
  h->spec_stale.clear();
  for (int k = 0; k < h->N; ++k) h->fuel[k] = fuel[h->stage_bounds ? k : 0];
  admm::fill_fuel(h->fac, h->fuel.data());
  return upload_factor(h);
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
  return setup_common(out, &d.hp, &oo, 0, 0, nullptr, nullptr, Mem::Device, &d.scan);
}

int admm_setup_timeshard(admm_handle** out, const admm_problem* p, const admm_options* o, int32_t rank, int32_t nranks,
                         admm_exchange_fn exchange, void* ctx) {
  if (nranks < 1) return fail(ADMM_ERR_INVALID, "admm_setup_timeshard: nranks must be >= 1");
  return setup_common(out, p, o, rank, nranks, exchange, ctx);
}

int admm_get_window(admm_handle* h, int32_t* stage_lo, int32_t* stage_hi, int32_t* seg_lo, int32_t* segs_local, int32_t* segs_total) {
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  const bool ts = h->ts_n > 0 && !h->pinst;
  const int s0 = ts ? h->ts_s0 : 0, sl = ts ? h->ts_sl : h->S;
  if (stage_lo) *stage_lo = h->pinst ? 0 : h->fac.seg_start[s0];
  if (stage_hi) *stage_hi = h->pinst ? h->N : h->fac.seg_start[s0 + sl];
  if (seg_lo) *seg_lo = s0;
  if (segs_local) *segs_local = sl;
  if (segs_total) *segs_total = h->S;
  return ADMM_OK;
}

// Both forms: everything is checked before anything of the handle is touched; a refused call leaves it as it was.
static int update_instances_common(admm_handle* h, const double* x0, const double* q, Mem mem, void* hip_stream) {
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  if (mem == Mem::Device && h->ts_n) return fail(ADMM_ERR_UNSUPPORTED, "admm_update_instances_device: not available on a time-sharded handle");
  HIP_TRY(hipSetDevice(h->device));
  CallerIO io(h, mem == Mem::Device ? "admm_update_instances_device" : "admm_update_instances", mem, hip_stream);
  const size_t nx = (size_t)h->n * h->batch, nq = (size_t)h->L * h->batch;
  int rc, bad;
  if ((rc = io.check_ptr(x0, nx * sizeof(double), "x0")) || (rc = io.check_ptr(q, nq * sizeof(double), "q"))) return rc;
  if (!x0 && !q) return ADMM_OK;
  if ((rc = io.begin()) || (rc = io.check_finite({{x0, nx, "x0"}, {q, nq, "q"}}, &bad))) return rc;
  if (bad == 0) return fail(ADMM_ERR_INVALID, "non-finite entry in x0");
  if (q && !h->has_q) return fail(ADMM_ERR_INVALID, "handle was set up without q; cannot add one later");
  if (bad == 1) return fail(ADMM_ERR_INVALID, "non-finite entry in q");
  if ((rc = ensure_w(h))) return rc;                 // w of the last x-update belongs to the old instance data
  drop_side_data(h);
  h->alt_state = admm_handle::ALT_NONE;
  if (x0 && (rc = upload_transposed(h, mem, x0, h->x0, h->n))) return rc;
  if (q && (rc = upload_transposed(h, mem, q, h->q, h->L))) return rc;
  return ADMM_OK;
}

int admm_update_instances(admm_handle* h, const double* x0, const double* q) {
  return update_instances_common(h, x0, q, Mem::Host, nullptr);
}
int admm_update_instances_device(admm_handle* h, const double* x0, const double* q, void* hip_stream) {
  return update_instances_common(h, x0, q, Mem::Device, hip_stream);
}

// Both forms: all three are checked before any is written.
static int set_state_common(admm_handle* h, const double* w, const double* z, const double* y, Mem mem, void* hip_stream) {
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  if (mem == Mem::Device && h->ts_n) return fail(ADMM_ERR_UNSUPPORTED, "admm_set_state_device: not available on a time-sharded handle");
  HIP_TRY(hipSetDevice(h->device));
  CallerIO io(h, mem == Mem::Device ? "admm_set_state_device" : "admm_set_state", mem, hip_stream);
  const size_t cnt = (size_t)h->L * h->batch;
  int rc, bad;
  if ((rc = io.check_ptr(w, cnt * sizeof(double), "w")) || (rc = io.check_ptr(z, cnt * sizeof(double), "z")) ||
      (rc = io.check_ptr(y, cnt * sizeof(double), "y")))
    return rc;
  if (!w && !z && !y) return ADMM_OK;
  // the device code is compiled with -fno-honor-nans on the premise that nothing non-finite gets in
  if ((rc = io.begin()) || (rc = io.check_finite({{w, cnt, "w"}, {z, cnt, "z"}, {y, cnt, "y"}}, &bad))) return rc;
  if (bad >= 0) return fail(ADMM_ERR_INVALID, "non-finite entry in w, z or y");
  if (w) {
    if ((rc = upload_transposed(h, mem, w, h->w, h->L))) return rc;
    h->w_stale = false;
  }
  if (z || y) {
    if ((rc = ensure_zy(h))) return rc;        // keep the one that is not overwritten
    if (z && (rc = upload_transposed(h, mem, z, h->z, h->L))) return rc;
    if (y && (rc = upload_transposed(h, mem, y, h->y, h->L))) return rc;
    h->zy_valid = true;
    h->v_valid = false;                         // an arbitrary (z, y) pair need not be of the form (clip(v), v - clip(v))
    drop_side_data(h);
    h->alt_state = admm_handle::ALT_NONE;
  }
  return ADMM_OK;
}

int admm_set_state(admm_handle* h, const double* w, const double* z, const double* y) {
  return set_state_common(h, w, z, y, Mem::Host, nullptr);
}
int admm_set_state_device(admm_handle* h, const double* w, const double* z, const double* y, void* hip_stream) {
  return set_state_common(h, w, z, y, Mem::Device, hip_stream);
}

int admm_step_x(admm_handle* h) {
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  HIP_TRY(hipSetDevice(h->device));
  int rc = step_x(h);
  if (rc) return rc;
  h->w_stale = false;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  return ADMM_OK;
}

int admm_step_z(admm_handle* h, int32_t residuals) {
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  if (h->pbounds) return fail(ADMM_ERR_UNSUPPORTED, "admm_step_z: the standalone z kernel has no per-instance bounds form");
  if (h->ts_n) return fail(ADMM_ERR_UNSUPPORTED, "admm_step_z is not available on a time-sharded handle (the standalone z kernel's partial sums are not per segment)");
  HIP_TRY(hipSetDevice(h->device));
  int rc = ensure_w(h);
  if (!rc) rc = ensure_zy(h);
  if (!rc) rc = launch_z(h, residuals != 0);
  if (rc) return rc;
  h->v_valid = false;
  drop_side_data(h);
  h->alt_state = admm_handle::ALT_NONE;
  if (residuals) {
    launch_finalize(h, 0, h->zchunks);
    h->resid_valid = true;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  return ADMM_OK;
}


int admm_run(admm_handle* h, int32_t iters, int32_t residual_every) {
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  if (iters < 0 || residual_every < 0) return fail(ADMM_ERR_INVALID, "iters / residual_every must be >= 0");
  HIP_TRY(hipSetDevice(h->device));
  const bool use_graph = (h->opt.flags & ADMM_FLAG_GRAPH) != 0;
  if (use_graph && !h->graph_exec[0]) {
    int rc = capture_iterations(h);
    if (rc) return rc;
  }
  for (int it = 1; it <= iters; ++it) {
    const bool resid = residual_every > 0 && (it % residual_every == 0);
    const bool next_resid = it < iters && residual_every > 0 && ((it + 1) % residual_every == 0);
    const bool next_plain = it < iters && !next_resid;
    int rc = enqueue_one(h, resid, use_graph, iters - it + 1, 0, next_plain, next_resid);
    if (rc) return rc;
  }
  int rcf = flush_finalize(h);
  if (rcf) return rcf;
  HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

int admm_iterate(admm_handle* h, int32_t iters) { return admm_run(h, iters, 0); }

int admm_get_lean_iterations(admm_handle* h, int64_t* count) {
  if (!h || !count) return fail(ADMM_ERR_INVALID, "NULL argument");
  *count = (int64_t)h->lean_count;
  return ADMM_OK;
}

int admm_sync(admm_handle* h) {
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return ADMM_OK;
}

int admm_solve_begin(admm_handle* h, const double* z0, const double* y0) {
  g_warn.clear();
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  HIP_TRY(hipSetDevice(h->device));
  h->solve_t0 = std::chrono::steady_clock::now();
  int rc;
  if ((rc = admm_set_state(h, nullptr, z0, y0))) return rc;
  const size_t P = h->pitch;
  HIP_TRY(hipMemsetAsync(h->status, 0, sizeof(int) * P, h->stream));
  {
    std::vector<int> init(P, h->opt.max_iter);
    HIP_TRY(hipMemcpyAsync(h->iters, init.data(), sizeof(int) * P, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  const bool use_graph = (h->opt.flags & ADMM_FLAG_GRAPH) != 0;
  if (use_graph && !h->graph_exec[0] && (rc = capture_iterations(h))) return rc;
  h->rho_updates = 0;
  h->history.clear();
  if (h->pinst) HIP_TRY(hipMemsetAsync(h->nupd_d, 0, sizeof(int) * P, h->stream));
  h->spec_hits = h->spec_misses = 0;
  h->solve_active = true;
  spec_start(h);                               // adaptive rule: factorise rho tau and rho / tau while the GPU iterates
  h->solve_it = 0;
  h->solve_nconv = 0;
  h->mixed_iters = 0;
  h->mixed_phase1 = h->opt.precision_mode == ADMM_PRECISION_MIXED;
  if (h->mixed_phase1) {
    if ((rc = flush_finalize(h))) return rc;
    set_mixed_form(h, true);
    HIP_TRY(hipMemsetAsync(h->status1, 0, sizeof(int) * P, h->stream));
  }
  return ADMM_OK;
}

int admm_solve_step(admm_handle* h, int32_t* iters_done, int32_t* n_converged, double* R_out, double* S_out) {
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  if (h->solve_it >= h->opt.max_iter) return fail(ADMM_ERR_INVALID, "admm_solve_step: max_iter already reached");
  HIP_TRY(hipSetDevice(h->device));
  const bool use_graph = (h->opt.flags & ADMM_FLAG_GRAPH) != 0;
  if (use_graph && !h->graph_exec[0]) { int rc0 = capture_iterations(h); if (rc0) return rc0; }
  const int ci = h->opt.check_interval;
  const size_t P = h->pitch;
  int rc;
  for (;;) {
    const int it = ++h->solve_it;
    const bool check = (it % ci == 0) || it == h->opt.max_iter;
    if (!check) {
      const int next_check = std::min(((it / ci) + 1) * ci, h->opt.max_iter);
      if ((rc = enqueue_one(h, false, use_graph, next_check - it + 1, 0, /*next_plain=*/it + 1 < next_check))) return rc;
      continue;
    }
    // checked iteration: launched directly so that the finalise kernel gets the iteration number
    HIP_TRY(hipMemsetAsync(h->nconv, 0, sizeof(int), h->stream));
    if ((rc = enqueue_one(h, true, use_graph, 1, it))) return rc;
    HIP_TRY(hipMemcpyAsync(h->h_nconv, h->nconv, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->solve_nconv = *h->h_nconv;
    h->resid_valid = true;
    if (h->opt.flags & ADMM_FLAG_HISTORY) {
      std::vector<double> rs(2 * P);
      HIP_TRY(hipMemcpy(rs.data(), h->resid, sizeof(double) * 2 * P, hipMemcpyDeviceToHost));
      admm_handle::HistoryEntry e{it, h->solve_nconv, 0.0, 0.0, h->opt.rho};
      for (int b = 0; b < h->batch; ++b) { e.max_r = std::max(e.max_r, rs[b]); e.max_s = std::max(e.max_s, rs[P + b]); }
      if (h->pinst) {
        std::vector<double> rq(P);
        HIP_TRY(hipMemcpy(rq.data(), h->rho_d, sizeof(double) * P, hipMemcpyDeviceToHost));
        e.rho = *std::max_element(rq.begin(), rq.begin() + h->batch);
      }
      if (h->mixed_phase1) e.nconv = 0;            // (the fp32 phase counts against raised tolerances: nothing has converged)
      h->history.push_back(e);
    }
    if (h->mixed_phase1) {
      // fp32 phase: the count is of the RAISED tolerances.  Once every QP meets them (or the budget is spent) the
      // solve continues with the fp64 kernels, which check the rule as given; nothing has converged so far.
      h->mixed_iters = h->solve_it;
      if (h->solve_nconv >= h->batch) {
        h->mixed_phase1 = false;
        set_mixed_form(h, false);
      }
      h->solve_nconv = 0;
    }
    break;
  }
  if (iters_done) *iters_done = h->solve_it;
  if (n_converged) *n_converged = h->solve_nconv;
  if (R_out || S_out) {
    // sums of r^2 and s^2 over the QPs that have not converged, in batch order (adaptive-rho rule)
    std::vector<double> rs(2 * P);
    std::vector<int> st(P);
    HIP_TRY(hipMemcpy(rs.data(), h->resid, sizeof(double) * 2 * P, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(st.data(), h->status, sizeof(int) * P, hipMemcpyDeviceToHost));
    double R = 0.0, S = 0.0;
    for (int b = 0; b < h->batch; ++b)
      if (!st[b]) { R += rs[b] * rs[b]; S += rs[P + b] * rs[P + b]; }
    if (R_out) *R_out = R;
    if (S_out) *S_out = S;
  }
  return ADMM_OK;
}

int admm_solve_adapt(admm_handle* h, double R, double S, int32_t* changed) {
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  HIP_TRY(hipSetDevice(h->device));
  if (changed) *changed = 0;
  const int it = h->solve_it;
  if (!(h->opt.adapt_interval > 0 && it % h->opt.adapt_interval == 0 && (h->pinst || h->rho_updates < h->opt.adapt_max) &&
        it < h->opt.max_iter))
    return ADMM_OK;                      // (per-instance: adapt_max is counted per QP, on the device)
  const double mu2 = h->opt.adapt_mu * h->opt.adapt_mu;
  if (h->pinst) {
    // Per-instance dynamics: the rule runs QP by QP on the device (csrc/admm_pinst.hpp, padapt_kernel); R and S -- the
    // batch sums of the shared-factor rule -- are not used, so a sharded solve needs no exchange for it.
    int rc;
    HIP_TRY(hipMemsetAsync(h->nchanged_d, 0, sizeof(int), h->stream));
    if ((rc = pinst_alloc_trial(h, false))) return rc;
    admm::launch_padapt(h->stream, h->resid, h->status, h->rho_d, h->nupd_d, h->todo_d, h->cscale_d, h->nchanged_d, mu2,
                        h->opt.adapt_tau, h->opt.adapt_max, h->pitch, h->batch, h->rho2_d);
    HIP_TRY(hipGetLastError());
    int nchanged = 0;
    HIP_TRY(hipMemcpyAsync(&nchanged, h->nchanged_d, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (!nchanged) return ADMM_OK;
    if (h->S > 1 && h->auto_segments) {
      // the candidates are factorised on trial (scratch K / S, transfer matrices not stored); a QP whose new rho
      // breaks the conditioning bound of its segments -- or has no factor -- keeps its rho and stops adapting, before its dual
      // is rescaled or its factor touched: what the batch-level rule does for shared dynamics.
      int not_pd = 0, grown = 0;
      if ((rc = pinst_try(h, h->Ad, h->Bd, h->Qd, h->Rd, h->QNd, h->rho_d, h->todo_d, &not_pd, &grown))) return rc;
      if (not_pd || grown) {
        int nveto = 0;
        HIP_TRY(hipMemsetAsync(h->nveto_d, 0, sizeof(int), h->stream));
        admm::launch_padapt_veto(h->stream, h->qflag_d, h->rho2_d, h->rho_d, h->nupd_d, h->todo_d, h->cscale_d, h->nchanged_d,
                                 h->nveto_d, h->opt.adapt_max, h->pitch);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&nveto, h->nveto_d, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(&nchanged, h->nchanged_d, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        g_warn = "adaptive rho: the change of " + std::to_string(nveto) + " QP(s) was refused (segment transfer matrices beyond the "
                 "conditioning bound, or no factor, with the new rho); those QPs keep their rho and stop adapting for this solve";
        if (!nchanged) return ADMM_OK;
      }
    }
    if ((rc = ensure_w(h))) return rc;            // w of the last x-update is rebuilt with the OLD factors (rho is not used)
    if ((rc = ensure_zy(h))) return rc;
    admm::launch_padapt_scale(h->stream, h->y, h->cscale_d, h->todo_d, h->L, h->pitch);
    HIP_TRY(hipGetLastError());
    h->zy_valid = true;
    h->v_valid = false;
    if ((rc = pinst_factor(h, /*only_marked=*/true))) return rc;
    h->rho_updates += nchanged;
    if (changed) *changed = 1;
    return ADMM_OK;
  }
  double rho_new = h->opt.rho;
  if (R > mu2 * S) rho_new = h->opt.rho * h->opt.adapt_tau;
  else if (S > mu2 * R) rho_new = h->opt.rho / h->opt.adapt_tau;
  if (rho_new != h->opt.rho) {
    int rc = set_rho_internal(h, rho_new);
    if (rc == ADMM_ERR_NUMERIC) {          // refused (conditioning guard / factorisation): keep rho, stop adapting
      g_warn = "adaptive rho: the change to rho = " + std::to_string(rho_new) + " was refused (" + g_err + "); rho stays at " +
               std::to_string(h->opt.rho) + " and the rule stops adapting for this solve";
      h->rho_updates = h->opt.adapt_max;
      spec_start(h);
      return ADMM_OK;
    }
    if (rc) return rc;
    ++h->rho_updates;
    spec_start(h);                         // the candidates of the new rho
    if (changed) *changed = 1;
  }
  return ADMM_OK;
}

int admm_solve_end(admm_handle* h, admm_info* info) {
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipGetLastError());
  if (std::getenv("ADMM_SPEC_DEBUG"))
    std::fprintf(stderr, "[admm] rho changes served by a background / kept factor: %d, factorised on demand: %d\n", h->spec_hits, h->spec_misses);
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->iters_run = h->solve_it;
  h->solve_active = false;                      // candidates of the adaptive rule are not kept between solves (their threads
  for (auto& sp2 : h->spec) h->spec_stale.push_back(std::move(sp2));      // are joined lazily, or by admm_free / admm_update_problem)
  h->spec.clear();
  spec_reap(h, false);
  if (h->opt.precision_mode == ADMM_PRECISION_MIXED) {
    if (h->mixed_phase1) h->mixed_iters = h->solve_it;
    h->mixed_phase1 = false;
    set_mixed_form(h, true);                 // admm_run / admm_iterate after a solve run the fp32 form again
  }
  const size_t P = h->pitch;
  if (info) {
    info->iters_run = h->solve_it;
    info->n_converged = h->solve_nconv;
    std::vector<double> rs(2 * P);
    HIP_TRY(hipMemcpy(rs.data(), h->resid, sizeof(double) * 2 * P, hipMemcpyDeviceToHost));
    double mr = 0, ms = 0;
    for (int b = 0; b < h->batch; ++b) {
      if (rs[b] > mr) mr = rs[b];
      if (rs[P + b] > ms) ms = rs[P + b];
    }
    info->max_r = mr;
    info->max_s = ms;
    info->solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h->solve_t0).count();
    info->rho = h->opt.rho;
    if (h->pinst) {                       // per-QP rho: the largest in force (admm_get_rho returns all of them)
      std::vector<double> r(h->pitch);
      HIP_TRY(hipMemcpy(r.data(), h->rho_d, sizeof(double) * r.size(), hipMemcpyDeviceToHost));
      info->rho = *std::max_element(r.begin(), r.begin() + h->batch);
    }
    info->rho_updates = h->rho_updates;
    info->mixed_iters = h->opt.precision_mode == ADMM_PRECISION_MIXED ? h->mixed_iters : 0;
  }
  return ADMM_OK;
}

int admm_solve(admm_handle* h, const double* z0, const double* y0, admm_info* info) {
  int rc = admm_solve_begin(h, z0, y0);
  if (rc) return rc;
  const bool adaptive = h->opt.adapt_interval > 0;
  for (;;) {
    int32_t it = 0, nconv = 0;
    double R = 0.0, S = 0.0;
    if ((rc = admm_solve_step(h, &it, &nconv, adaptive ? &R : nullptr, adaptive ? &S : nullptr))) return rc;
    if (nconv >= h->batch || it >= h->opt.max_iter) break;
    if (adaptive && (rc = admm_solve_adapt(h, R, S, nullptr))) return rc;
  }
  return admm_solve_end(h, info);
}

int admm_get_residuals(admm_handle* h, double* r, double* s, double* nw, double* nz, double* ny) {
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  if (!h->resid_valid) return fail(ADMM_ERR_INVALID, "no residual-evaluating z step has run yet");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  double* dst[5] = {r, s, nw, nz, ny};
  for (int v = 0; v < 5; ++v)
    if (dst[v]) HIP_TRY(hipMemcpy(dst[v], h->resid + (size_t)v * h->pitch, sizeof(double) * h->batch, hipMemcpyDeviceToHost));
  return ADMM_OK;
}

// Device form: the read-out kernels write the caller's arrays on the handle's stream, after what the caller had queued on hip_stream;
// hip_stream then waits for them (no host synchronisation), or, with hip_stream = NULL, this call does.
static int get_common(admm_handle* h, double* w, double* z, double* y, Mem mem, void* hip_stream) {
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  if (mem == Mem::Device && h->ts_n) return fail(ADMM_ERR_UNSUPPORTED, "admm_get_device: not available on a time-sharded handle");
  HIP_TRY(hipSetDevice(h->device));
  CallerIO io(h, mem == Mem::Device ? "admm_get_device" : "admm_get", mem, hip_stream);
  const size_t bytes = sizeof(double) * (size_t)h->L * h->batch;
  int rc;
  if ((rc = io.check_ptr(w, bytes, "w")) || (rc = io.check_ptr(z, bytes, "z")) || (rc = io.check_ptr(y, bytes, "y"))) return rc;
  if (w && (rc = ensure_w(h))) return rc;
  if ((z || y) && (rc = ensure_zy(h))) return rc;
  if ((rc = io.begin())) return rc;
  if (w && (rc = download_transposed(h, mem, h->w, w, h->L))) return rc;
  if (z && (rc = download_transposed(h, mem, h->z, z, h->L))) return rc;
  if (y && (rc = download_transposed(h, mem, h->y, y, h->L))) return rc;
  return io.dev() ? io.finish() : ADMM_OK;      // (a host download returns with the copy complete)
}

int admm_get(admm_handle* h, double* w, double* z, double* y) { return get_common(h, w, z, y, Mem::Host, nullptr); }
int admm_get_device(admm_handle* h, double* w, double* z, double* y, void* hip_stream) { return get_common(h, w, z, y, Mem::Device, hip_stream); }

// ---- certificate (kernels in admm_cert_kernels.hpp) ----

// Device copies of the raw problem (A_k | B_k per stage, Q | QN | R symmetrised, the segment products Phi_s) and the work
// buffers, on the first call and after admm_update_problem; the fuel weights whenever they differ from the copy on the device.
static int cert_prepare(admm_handle* h, bool want_nu) {
  int rc;
  const int n = h->n, m = h->m, N = h->N, S = h->S;
  const size_t P = h->pitch, rab = (size_t)n * (n + m);
  // field by field: a failed allocation leaves a handle whose next call allocates what is missing (and uploads the operands again)
  auto lazy = [h](double** field, size_t count) {
    if (*field) return (int)ADMM_OK;
    h->cert_valid = false;
    h->cert_fuel_h.clear();
    return dalloc(h, field, count);
  };
  if ((rc = lazy(&h->certAB, (size_t)N * rab)) || (rc = lazy(&h->certQR, (size_t)2 * n * n + (size_t)m * m)) ||
      (rc = lazy(&h->certPhi, (size_t)S * n * n)) || (rc = lazy(&h->cert_fuel, (size_t)N)) ||
      (rc = lazy(&h->cert_cseg, (size_t)S * n * P)) || (rc = lazy(&h->cert_cin, (size_t)S * n * P)) ||
      (rc = lazy(&h->cert_part, (size_t)S * 3 * P)) || (rc = lazy(&h->cert_out, 3 * P)))
    return rc;
  if (want_nu && !h->cert_nu && (rc = dalloc(h, &h->cert_nu, (size_t)N * n * P))) return rc;
  bool uploaded = false;
  std::vector<double> ab, qr, phi;          // (alive until the synchronisation below)
  if (!h->cert_valid) {
    ab.resize((size_t)N * rab);
    for (int k = 0; k < N; ++k) {
      const double* A = h->pA.data() + (h->time_varying ? (size_t)k * n * n : 0);
      const double* B = h->pB.data() + (h->time_varying ? (size_t)k * n * m : 0);
      std::copy(A, A + (size_t)n * n, ab.begin() + (size_t)k * rab);
      std::copy(B, B + (size_t)n * m, ab.begin() + (size_t)k * rab + (size_t)n * n);
    }
    qr.resize((size_t)2 * n * n + (size_t)m * m);
    auto sym = [](const std::vector<double>& a, int d, double* out) {      // as admm_setup symmetrises the weights
      for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) out[(size_t)i * d + j] = 0.5 * (a[(size_t)i * d + j] + a[(size_t)j * d + i]);
    };
    sym(h->pQ, n, qr.data());
    sym(h->pQN, n, qr.data() + (size_t)n * n);
    sym(h->pR, m, qr.data() + (size_t)2 * n * n);
    // Phi_s = A_k0' A_k0+1' ... A_k1-1' (row-major), built from the segment's last stage down
    phi.assign((size_t)S * n * n, 0.0);
    std::vector<double> t((size_t)n * n);
    for (int s = 0; s < S; ++s) {
      double* F = phi.data() + (size_t)s * n * n;
      for (int i = 0; i < n; ++i) F[(size_t)i * n + i] = 1.0;
      for (int k = h->fac.seg_start[s + 1] - 1; k >= h->fac.seg_start[s]; --k) {
        const double* A = ab.data() + (size_t)k * rab;                      // column-major: A'(i, l) = A[l + i n]
        for (int i = 0; i < n; ++i)
          for (int j = 0; j < n; ++j) {
            double a = 0.0;
            for (int l = 0; l < n; ++l) a += A[(size_t)l + (size_t)i * n] * F[(size_t)l * n + j];
            t[(size_t)i * n + j] = a;
          }
        std::copy(t.begin(), t.end(), F);
      }
    }
    HIP_TRY(hipMemcpyAsync(h->certAB, ab.data(), sizeof(double) * ab.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->certQR, qr.data(), sizeof(double) * qr.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->certPhi, phi.data(), sizeof(double) * phi.size(), hipMemcpyHostToDevice, h->stream));
    uploaded = true;
  }
  std::vector<double> fu(N, 0.0);
  if (h->has_fuel) fu = h->fuel;
  if (fu != h->cert_fuel_h) {
    HIP_TRY(hipMemcpyAsync(h->cert_fuel, fu.data(), sizeof(double) * N, hipMemcpyHostToDevice, h->stream));
    uploaded = true;
  }
  if (uploaded) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->cert_valid = true;
    h->cert_fuel_h = fu;
  }
  return ADMM_OK;
}

static int certificate_common(admm_handle* h, double* obj, double* feas_dyn, double* stat, double* nu, Mem mem, void* hip_stream) {
  const char* fn = mem == Mem::Device ? "admm_get_certificate_device" : "admm_get_certificate";
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  if (h->pinst) return fail(ADMM_ERR_UNSUPPORTED, std::string(fn) + ": not available with per-instance dynamics (time_varying = 2)");
  if (h->ts_n) return fail(ADMM_ERR_UNSUPPORTED, std::string(fn) + ": not available on a time-sharded handle");
  HIP_TRY(hipSetDevice(h->device));
  CallerIO io(h, fn, mem, hip_stream);
  int rc;
  const size_t bsz = sizeof(double) * (size_t)h->batch, nusz = bsz * (size_t)h->N * h->n;
  if ((rc = io.check_ptr(obj, bsz, "obj")) || (rc = io.check_ptr(feas_dyn, bsz, "feas_dyn")) || (rc = io.check_ptr(stat, bsz, "stat")) ||
      (rc = io.check_ptr(nu, nusz, "nu")))
    return rc;
  admm::CertLaunch l{};
  l.n = h->n; l.m = h->m;
  if (!admm::launch_cert(l, /*query_only=*/true))
    return fail(ADMM_ERR_UNSUPPORTED, std::string(fn) + ": no certificate kernel for this (n, m)");
  if ((rc = ensure_zy(h))) return rc;                   // the state as the (z, y) pair, as admm_get reads it
  if ((rc = cert_prepare(h, nu != nullptr))) return rc;
  if ((rc = io.begin())) return rc;
  l.stream = h->stream;
  l.N = h->N; l.S = h->S; l.pitch = h->pitch;
  l.has_q = h->has_q;
  l.rho = h->opt.rho;
  l.z = h->z; l.y = h->y; l.q = h->q; l.x0 = h->x0;
  l.AB = h->certAB; l.QR = h->certQR; l.Phi = h->certPhi; l.fuel = h->cert_fuel;
  l.seg_start = h->seg_start;
  l.cseg = h->cert_cseg; l.cin = h->cert_cin; l.part = h->cert_part; l.out = h->cert_out;
  l.nu = nu ? h->cert_nu : nullptr;
  admm::launch_cert(l, false);
  HIP_TRY(hipGetLastError());
  double* dst[3] = {obj, feas_dyn, stat};
  for (int v = 0; v < 3; ++v)
    if (dst[v] && (rc = io.copy_out(dst[v], h->cert_out + (size_t)v * h->pitch, bsz))) return rc;
  if (nu && (rc = download_transposed(h, mem, h->cert_nu, nu, h->N * h->n))) return rc;
  return io.finish();
}

int admm_get_certificate(admm_handle* h, double* obj, double* feas_dyn, double* stat, double* nu) {
  return certificate_common(h, obj, feas_dyn, stat, nu, Mem::Host, nullptr);
}

// The device-memory form: the rules of admm_get_device (pointer checks, ordering against hip_stream, no host synchronisation
// once the operands are on the device).
int admm_get_certificate_device(admm_handle* h, double* obj, double* feas_dyn, double* stat, double* nu, void* hip_stream) {
  return certificate_common(h, obj, feas_dyn, stat, nu, Mem::Device, hip_stream);
}

// ---- infeasibility probe (kernels in admm_infeas_kernels.hpp) ----

// The snapshot and work buffers on the first call; the box and thrust bound of every stage ([N][2 nb + 1]: lo | hi | unorm, from the
// handle's host copy of the problem) on the first call and after admm_update_problem.  A_k | B_k and Phi_s are the certificate's.
static int infeas_prepare(admm_handle* h, bool want_nu, bool want_flag) {
  int rc;
  const int nb = h->nb, N = h->N, S = h->S, rbd = 2 * nb + 1;
  const size_t P = h->pitch;
  if ((rc = cert_prepare(h, want_nu))) return rc;
  auto lazy = [h](double** field, size_t count) {      // (field by field, as cert_prepare)
    if (*field) return (int)ADMM_OK;
    h->infeas_valid = false;
    return dalloc(h, field, count);
  };
  if ((rc = lazy(&h->infeas_y0, (size_t)h->L * P)) || (rc = lazy(&h->infeas_bnd, (size_t)N * rbd)) ||
      (rc = lazy(&h->infeas_part, (size_t)S * 5 * P)) || (rc = lazy(&h->infeas_out, 5 * P)))
    return rc;
  if (want_flag && !h->infeas_flag && (rc = dalloc(h, &h->infeas_flag, P))) return rc;
  if (!h->infeas_valid) {
    std::vector<double> bd((size_t)N * rbd);
    for (int k = 0; k < N; ++k) {
      const size_t o = h->stage_bounds ? (size_t)k * nb : 0;
      std::copy(h->plo.begin() + o, h->plo.begin() + o + nb, bd.begin() + (size_t)k * rbd);
      std::copy(h->phi.begin() + o, h->phi.begin() + o + nb, bd.begin() + (size_t)k * rbd + nb);
      bd[(size_t)k * rbd + 2 * nb] = h->pun.empty() ? INFINITY : h->pun[h->stage_bounds ? k : 0];
      if (h->has_soft)                      // a row with a finite weight can be violated at a price: open for feasibility
        for (int j = 0; j < nb; ++j)
          if (h->soft[(size_t)k * nb + j] < INFINITY) { bd[(size_t)k * rbd + j] = -INFINITY; bd[(size_t)k * rbd + nb + j] = INFINITY; }
    }
    HIP_TRY(hipMemcpyAsync(h->infeas_bnd, bd.data(), sizeof(double) * bd.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->infeas_valid = true;
  }
  return ADMM_OK;
}

static int infeasibility_common(admm_handle* h, int32_t span, double eps, double* sep, double* drift, double* defect,
                                int32_t* infeasible, double* nu, Mem mem, void* hip_stream) {
  const char* fn = mem == Mem::Device ? "admm_probe_infeasibility_device" : "admm_probe_infeasibility";
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  if (span < 1) return fail(ADMM_ERR_INVALID, std::string(fn) + ": span must be >= 1");
  if (!std::isfinite(eps) || eps < 0.0) return fail(ADMM_ERR_INVALID, std::string(fn) + ": eps must be finite and >= 0");
  if (h->pinst) return fail(ADMM_ERR_UNSUPPORTED, std::string(fn) + ": not available with per-instance dynamics (time_varying = 2)");
  if (h->ts_n) return fail(ADMM_ERR_UNSUPPORTED, std::string(fn) + ": not available on a time-sharded handle");
  if (h->cons_G)
    return fail(ADMM_ERR_UNSUPPORTED, std::string(fn) + ": not available on a scenario-consensus handle (a per-QP Farkas certificate is not the coupled problem's)");
  if (h->hs_nh)
    return fail(ADMM_ERR_UNSUPPORTED, std::string(fn) + ": not available on a handle with half-spaces (the Farkas certificate is written for boxes and the thrust ball)");
  if (h->opt.precision_mode == ADMM_PRECISION_MIXED)
    return fail(ADMM_ERR_UNSUPPORTED, std::string(fn) + ": not available with precision_mode MIXED (the fp32 phase would put rounding "
                "noise into the dual's difference)");
  HIP_TRY(hipSetDevice(h->device));
  CallerIO io(h, fn, mem, hip_stream);
  int rc;
  const size_t bsz = sizeof(double) * (size_t)h->batch, nusz = bsz * (size_t)h->N * h->n, fsz = sizeof(int32_t) * (size_t)h->batch;
  if ((rc = io.check_ptr(sep, bsz, "sep")) || (rc = io.check_ptr(drift, bsz, "drift")) || (rc = io.check_ptr(defect, bsz, "defect")) ||
      (rc = io.check_ptr(infeasible, fsz, "infeasible", sizeof(int32_t), "int32 entries")) || (rc = io.check_ptr(nu, nusz, "nu")))
    return rc;
  admm::InfeasLaunch l{};
  l.n = h->n; l.m = h->m;
  if (!admm::launch_infeas(l, /*query_only=*/true))
    return fail(ADMM_ERR_UNSUPPORTED, std::string(fn) + ": no infeasibility kernel for this (n, m)");
  if ((rc = infeas_prepare(h, nu != nullptr, infeasible != nullptr))) return rc;
  // the state as the (z, y) pair, as admm_get reads it; y kept; span iterations as admm_run(h, span, 0) runs them; (z, y) again
  if ((rc = ensure_zy(h))) return rc;
  HIP_TRY(hipMemcpyAsync(h->infeas_y0, h->y, sizeof(double) * (size_t)h->L * h->pitch, hipMemcpyDeviceToDevice, h->stream));
  if ((rc = admm_run(h, span, 0))) return rc;
  if ((rc = ensure_zy(h))) return rc;
  if ((rc = io.begin())) return rc;
  l.stream = h->stream;
  l.N = h->N; l.S = h->S; l.pitch = h->pitch;
  l.span = (double)span; l.eps = eps;
  l.y = h->y; l.y0 = h->infeas_y0; l.x0 = h->x0;
  l.AB = h->certAB; l.Phi = h->certPhi; l.bnd = h->infeas_bnd;
  l.seg_start = h->seg_start;
  l.cseg = h->cert_cseg; l.cin = h->cert_cin; l.part = h->infeas_part; l.out = h->infeas_out;
  l.nu = nu ? h->cert_nu : nullptr;
  admm::launch_infeas(l, false);
  HIP_TRY(hipGetLastError());
  double* dst[3] = {sep, drift, defect};
  for (int v = 0; v < 3; ++v)
    if (dst[v] && (rc = io.copy_out(dst[v], h->infeas_out + (size_t)v * h->pitch, bsz))) return rc;
  if (infeasible) {                                     // the flag as int32
    admm::launch_infeas_flags(h->stream, h->infeas_out + (size_t)3 * h->pitch, h->infeas_flag, h->batch);
    HIP_TRY(hipGetLastError());
    if ((rc = io.copy_out(infeasible, h->infeas_flag, fsz))) return rc;
  }
  if (nu && (rc = download_transposed(h, mem, h->cert_nu, nu, h->N * h->n))) return rc;
  return io.finish();
}

int admm_probe_infeasibility(admm_handle* h, int32_t span, double eps, double* sep, double* drift, double* defect,
                             int32_t* infeasible, double* nu) {
  return infeasibility_common(h, span, eps, sep, drift, defect, infeasible, nu, Mem::Host, nullptr);
}

// The device-memory form: the rules of admm_get_certificate_device.
int admm_probe_infeasibility_device(admm_handle* h, int32_t span, double eps, double* sep, double* drift, double* defect,
                                    int32_t* infeasible, double* nu, void* hip_stream) {
  return infeasibility_common(h, span, eps, sep, drift, defect, infeasible, nu, Mem::Device, hip_stream);
}

int admm_get_info(admm_handle* h, int32_t* iters, int32_t* status, double* r, double* s) {
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (iters) HIP_TRY(hipMemcpy(iters, h->iters, sizeof(int32_t) * h->batch, hipMemcpyDeviceToHost));
  if (status) HIP_TRY(hipMemcpy(status, h->status, sizeof(int32_t) * h->batch, hipMemcpyDeviceToHost));
  if (r) HIP_TRY(hipMemcpy(r, h->resid, sizeof(double) * h->batch, hipMemcpyDeviceToHost));
  if (s) HIP_TRY(hipMemcpy(s, h->resid + h->pitch, sizeof(double) * h->batch, hipMemcpyDeviceToHost));
  return ADMM_OK;
}


int admm_get_rho(admm_handle* h, double* rho) {
  if (!h || !rho) return fail(ADMM_ERR_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(h->device));
  if (!h->pinst) {
    for (int b = 0; b < h->batch; ++b) rho[b] = h->opt.rho;
    return ADMM_OK;
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(rho, h->rho_d, sizeof(double) * h->batch, hipMemcpyDeviceToHost));
  return ADMM_OK;
}

int admm_get_geometry(admm_handle* h, int32_t* pitch, int32_t* segs, int32_t* zrows, int32_t* zchunks) {
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  if (pitch) *pitch = h->pitch;
  if (segs) *segs = h->S;
  if (zrows) *zrows = h->zrows;
  if (zchunks) *zchunks = h->zchunks;
  return ADMM_OK;
}

int admm_get_scan_geometry(admm_handle* h, int32_t* split, int32_t* M, int32_t* K, int32_t* groups) {
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  if (split) *split = h->pinst ? 1 : h->scan_split;
  if (M) *M = h->pinst ? 0 : h->fac.scanM;
  if (K) *K = h->pinst ? 0 : h->fac.scanK;
  if (groups) *groups = h->pinst ? 0 : h->fac.scanM / 16 / admm::SCAN_MT;
  return ADMM_OK;
}

int admm_get_path(admm_handle* h, admm_path_info* info) {
  if (!h || !info) return fail(ADMM_ERR_INVALID, "NULL argument");
  std::memset(info, 0, sizeof *info);
  info->alternating = h->alt ? 1 : 0;
  info->alt_requested = h->alt_requested ? 1 : 0;
  info->mfma = h->mfma_mode != 0 && (h->opt.precision_mode == ADMM_PRECISION_MIXED || h->alt) ? h->mfma_mode : 0;
  info->xfree = h->xfree ? 1 : 0;
  info->segments = h->S;
  info->auto_segments = h->auto_segments ? 1 : 0;
  info->scan_form = h->pinst ? 3 : (h->opt.flags & ADMM_FLAG_SCAN_CHAIN) ? 2 : h->scan_gemv ? 1 : 0;
  info->per_instance = h->pinst ? 1 : 0;
  info->alt_check = h->pinst ? -1.0 : h->fac.alt_check;
  info->alt_gate = ALT_GATE;
  info->scan_growth = h->pinst ? 0.0 : scan_growth(h->fac);
  return ADMM_OK;
}

void admm_free(admm_handle* h) { release(h); }


}  // extern "C"
