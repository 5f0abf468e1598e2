// admm_runtime.hpp -- internals shared by the translation units of the solver runtime (round 3: csrc/admm_api.hip used to hold
// all of it in 2.4 k lines):
//   admm_api.hip      the C ABI of state, iteration, solve and read-out
//   admm_setup.hip    set-up of a handle, step by step, and every admm_setup* entry point
//   admm_zext.hip     the entry points of the fuel term and of the z-update extensions (consensus, soft box, half-spaces, cones)
//   admm_launch.hip   kernel launches, the time-shard exchange, iteration forms and their schedule, graph capture
//   admm_hostio.hip   host <-> device transfers, validation, uploads of a factor, handle lifetime
//   admm_rho_update.hip rho changes and problem updates: background candidate factors, admm_set_rho, admm_update_problem
//   admm_pinst_rt.hip per-instance dynamics: device factorisation, trial factorisation, set-up
//   admm_profile.hip  admm_profile (per-kernel HIP-event timing)
//   admm_mpc.hip      the receding-horizon step: admm_mpc_advance, admm_mpc_advance_device
// Everything here is namespace admm::rt; nothing in this header is part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/admm_hip.h"
#include "admm_dispatch.hpp"
#include "admm_factor.hpp"
#include "admm_kernels.hpp"

// A factorisation for a rho the adaptive rule may ask for next, computed on a background thread while the GPU iterates
// (or the factor of the previous rho, kept).  See spec_start().
struct SpecFactor {
  double rho = 0.0;
  admm::Factor f;
  std::string err;
  int rc = 0;
  std::thread th;
  ~SpecFactor() { if (th.joinable()) th.join(); }
};

// Which standalone z kernel a handle runs: the per-QP box / thrust-ball prox, or ONE extension of it.  A fuel term
// and a thrust bound (has_fuel, has_soc) compose with every kind and are not one.
enum class ZKind { Box, Consensus, Soft, Halfspace, Cone };

// What the runtime says and decides per kind, once.  Every extension runs the unfused path of the one-lane fp64 kernels of
// batch-shared dynamics only: its set-up refuses time_varying = 2 and the MFMA precision modes and forces ADMM_FLAG_UNFUSED.
struct ZKindInfo {
  const char* setup;         // the set-up entry point, as the messages name it
  const char *needs, *is_not;   // the subject of set-up's refusals, with its verb: "... needs batch-shared dynamics", "... is not supported by ..."
  bool whole_blocks;         // a chunk of the z kernel is whole blocks (a block-structured walk)
  const char* handle;        // such a handle, as the refusals of calls on it name it
  const char* no_step;       // why the receding-horizon step refuses it; nullptr: it does not
  const char* no_probe;      // why the infeasibility probe refuses it; nullptr: it does not
  const char* payload;       // what a handle of another kind lacks: "the handle has no ..."
};
constexpr ZKindInfo ZKINDS[] = {
    {"admm_setup", nullptr, nullptr, false, nullptr, nullptr, nullptr, nullptr},
    {"admm_setup_consensus", "scenario consensus needs", "scenario consensus is not", true, "a scenario-consensus handle",
     "a per-QP plant step is not the coupled problem's", "a per-QP Farkas certificate is not the coupled problem's", "scenario groups"},
    {"admm_setup_soft", "soft constraints need", "soft constraints are not", false, "a handle with soft weights", nullptr, nullptr,
     "soft weights"},
    {"admm_setup_halfspace", "half-spaces need", "half-spaces are not", true, "a handle with half-spaces",
     "a per-QP plane is not window-relative: it would have to shift with the horizon",
     "the Farkas certificate is written for boxes and the thrust ball", "half-spaces"},
    {"admm_setup_cone", "approach cones need", "approach cones are not", true, "a handle with approach cones",
     "a per-QP cone is not window-relative: it would have to shift with the horizon",
     "the Farkas certificate is written for boxes and the thrust ball", "approach cones"},
};
constexpr const ZKindInfo& zkind_info(ZKind k) { return ZKINDS[static_cast<int>(k)]; }

struct admm_handle {
  int N = 0, n = 0, m = 0, nb = 0, batch = 0, pitch = 0, L = 0;
  int S = 0, zrows = 0, zchunks = 0;
  int scan_split = 1;            // split-K factor of the MFMA scan (small batches)
  int device = 0;
  int num_cus = 256;             // hipDeviceProp_t::multiProcessorCount of the handle's device
  bool xfree = false;            // every state row is unbounded at every stage (XFREE kernel forms, see xfze_kernel)
  int xfree_mode = 1;            // 2 while enqueue_one launches an iteration whose successor will not read those rows' v
  // Lean residual iterations (admm_kernels_alt.hpp, LEAN forms): side data of the last iterate and its validity
  double *wu = nullptr, *xbnd = nullptr;   // w_u [stage][m][pitch] (window and bias of mvec); end-of-segment states [S][n][pitch]
  int lean_mode = 0;             // ALT_LEAN_* bits while enqueue_one launches a lean form, else 0 (the full forms)
  bool side_valid = false;       // wu / xbnd describe the iterate in h->v: the last iteration was a residual alternating one that wrote them
  int side_dir = 0;              // ... and ran in this direction (ALT_FWD / ALT_BWD): a lean read needs the opposite one
  bool v_rows_stale = false;     // the last launch was an NW form: the next one must be NR (same call, enqueue_one)
  long long lean_count = 0;      // iterations launched with the no-read form since setup (admm_get_lean_iterations)
  bool auto_segments = false;    // the segment count was chosen by admm_setup (and is guarded by scan_growth)
  bool has_q = false;
  bool has_soc = false;          // some stage has a finite thrust-magnitude bound, or the handle has a fuel term
  bool has_fuel = false;         // set up by admm_setup_fuel with weights: cost term sum_k fuel[k] ||u_k||_2
  std::vector<double> fuel;      // its N per-stage weights (the records and h->kap hold fuel[k] / rho)
  ZKind zkind = ZKind::Box;      // the standalone z kernel (launch_z), set once by init_handle; only that kind's fields below are in use
  int cons_G = 0;                // scenario consensus (admm_setup_consensus): group size
  // soft box constraints (admm_setup_soft): the weights per stacked row (+inf = hard), their device copy, weight / rho
  // beside it (refreshed wherever h->kap is: upload_kappa), and the report's results, allocated on the first admm_get_soft_report* call
  std::vector<double> soft;      // [L]
  double *soft_d = nullptr, *skap_d = nullptr, *soft_out = nullptr;      // [L], [L], [2][pitch] penalty | max violation
  int* soft_cnt = nullptr;       // [pitch] violated rows
  // one half-space per stage (admm_setup_halfspace): a' xi <= b on the first hs_nh state rows of a block.  The planes
  // live on the device only -- shared [N][nh] | [N], or per QP batch-minor [N][nh][pitch] | [N][pitch] --, at addresses that never
  // change (captured graphs hold them); the host keeps which stages have a plane for some QP (the open-box rule).  The report's
  // results and the scan's flags are allocated on first use.
  int hs_nh = 0;
  bool hs_perqp = false;
  double *hs_a = nullptr, *hs_b = nullptr;
  std::vector<char> hs_any;      // [N] some QP has a plane at the stage
  double *hs_out = nullptr, *hs_lam = nullptr;     // [pitch] max violation; [N][pitch] multipliers
  int *hs_cnt = nullptr, *hs_flags = nullptr;      // [pitch] active stages; [2][N] findings of halfspace_scan_kernel
  // one approach cone per stage (admm_setup_cone): axis, apex and slope on the first cone_nh state rows of a block,
  // kept as the half-spaces are -- on the device only, shared [N][nh] | [N][nh] | [N] or per QP batch-minor [N][nh][pitch] twice |
  // [N][pitch], at addresses that never change; the host keeps which stages have a cone for some QP (the open-box rule)
  int cone_nh = 0;
  bool cone_perqp = false;
  double *cone_c = nullptr, *cone_p = nullptr, *cone_g = nullptr;
  std::vector<char> cone_any;    // [N] some QP has a cone at the stage
  double *cone_out = nullptr, *cone_lam = nullptr; // [pitch] max violation; [N][pitch] rho |y_xi|
  int *cone_cnt = nullptr, *cone_flags = nullptr;  // [pitch] active stages; [3][N] findings of cone_scan_kernel
  admm_options opt{};
  admm::Factor fac;
  // host copy of the shared problem data (the caller's pointers are never kept): admm_set_rho refactors from it
  std::vector<double> pA, pB, pQ, pR, pQN, plo, phi, pun;
  int time_varying = 0, stage_bounds = 0;
  int rho_updates = 0;
  std::vector<std::unique_ptr<SpecFactor>> spec;        // candidates of the adaptive rule (rho tau, rho / tau)
  std::vector<std::unique_ptr<SpecFactor>> spec_stale;  // no longer candidates; their threads are joined lazily
  int spec_hits = 0, spec_misses = 0;
  // time-sharded handle (admm_setup_timeshard): this rank runs segments [ts_s0, ts_s0 + ts_sl) of the S the horizon is cut into
  int ts_n = 0, ts_rank = 0, ts_s0 = 0, ts_sl = 0;      // ts_n = 0: an ordinary handle
  admm_exchange_fn ts_fn = nullptr;
  // Stage window [wk0, wk1) of the big per-stage arrays (w, z, y, v, q: (n + m) rows per stage; dbuf, mvec: m rows per stage):
  // the whole horizon for an ordinary handle; a time shard of several ranks ALLOCATES only its own stages.  The pointers
  // h->w ... are biased by the window's first row (allocation - wk0 * rows_per_stage * pitch), so the kernels, which address
  // rows by their global stage index, run unchanged; only the window's rows are ever touched (admm::rt::win_* below).
  int wk0 = 0, wk1 = 0;
  void* ts_ctx = nullptr;
  bool solve_active = false;     // between admm_solve_begin and admm_solve_end: only then are candidate factors kept / started
  // ADMM_FLAG_HISTORY: one record per stopping test of the last admm_solve
  struct HistoryEntry { int32_t it, nconv; double max_r, max_s, rho; };
  std::vector<HistoryEntry> history;
  int solve_it = 0, solve_nconv = 0;     // admm_solve_begin / _step / _end state
  std::chrono::steady_clock::time_point solve_t0;
  hipStream_t stream = nullptr;
  // batch-minor state and work buffers
  double *w = nullptr, *z = nullptr, *y = nullptr, *v = nullptr, *q = nullptr, *x0 = nullptr;
  double *dbuf = nullptr, *tseg = nullptr, *eseg = nullptr, *tin = nullptr, *xin = nullptr;
  double *part = nullptr, *resid = nullptr, *lo = nullptr, *hi = nullptr, *ub = nullptr;
  double* kap = nullptr;         // [N] fuel weight / rho per stage beside ub (zeros without a fuel term): block-structured z kernels
  double *recB = nullptr, *recF = nullptr, *recS = nullptr;
  double *scan_in = nullptr, *scan_out = nullptr, *scanWp = nullptr;   // tseg|x0|eseg and t_in|x_in live inside these
  int* scan_range = nullptr;
  // batches of up to SCAN_GEMV_MAXCOLS QPs: the scan as a matrix-vector product per column (xscan_gemv_kernel) on the
  // dense row-major matrices, with each row's non-zero column range
  bool scan_gemv = false;
  double *scanWd = nullptr, *scanWBd = nullptr;
  int *scan_rows = nullptr, *scan_rowsB = nullptr;
  // alternating-direction iteration
  double *recFE = nullptr, *recBE = nullptr, *mvec = nullptr, *scanWpB = nullptr;
  size_t recFE_bytes = 0, recBE_bytes = 0;     // allocated, incl. the slack of the LDS-DMA copy (check_record_alloc below)
  int* scan_rangeB = nullptr;
  // MFMA form of the fused kernels: fragment records, mode (0 = not in use, 1 mixed, 2 fp64), and whether
  // launch_x currently routes to it (the fp64 refinement phase of a MIXED solve turns it off)
  unsigned char *recMF = nullptr, *recMB = nullptr;
  unsigned char *recMF64 = nullptr, *recMB64 = nullptr;    // MIXED only: all-fp64 records of the refinement phase
  int mfma_mode = 0;
  bool mfma_on = false;
  bool mfma_refine = false;      // MIXED, refinement phase: the fp64 MFMA kernels on recMF64 / recMB64
  bool alt_allowed = false;      // alternation permitted by the options / compiled kernels (before the precision mode)
  bool alt_requested = false;    // ... whether or not the forward-elimination form passed its host check (admm_get_path)
  // MIXED solve: phase 1 (fp32) checks the stopping rule with raised tolerances on scratch status arrays
  bool mixed_phase1 = false;
  int mixed_iters = 0;
  int *status1 = nullptr, *iters1 = nullptr;
  // per-instance dynamics (csrc/admm_pinst.hpp): device-side factor, operands per QP in HBM
  bool pinst = false, pbounds = false;
  double *Ad = nullptr, *Bd = nullptr, *Kd = nullptr, *Sd = nullptr, *lod = nullptr, *hid = nullptr;
  double *lodT = nullptr, *hidT = nullptr;   // wide shapes: a second, TILED copy of the per-instance box for the sweeps (csrc/admm_pinst.hpp, Operand)
  double *Qd = nullptr, *Rd = nullptr, *QNd = nullptr;
  int* pfail = nullptr;
  // TRIAL buffers of the per-instance path (allocated on first use): a change of rho or of the problem data is factorised
  // into these first and only then committed by swapping pointers, so that a refused change leaves the handle untouched
  double *Ad2 = nullptr, *Bd2 = nullptr, *Kd2 = nullptr, *Sd2 = nullptr, *Qd2 = nullptr, *Rd2 = nullptr, *QNd2 = nullptr;
  double *rho2_d = nullptr;      // [pitch] candidate rho (admm_set_rho) / the rho being left (per-QP adaptive rule)
  int *qflag_d = nullptr, *nveto_d = nullptr;      // [pitch] per-QP verdict of a trial factorisation; [1] refused changes
  // segments in time of the per-instance path (S > 1; csrc/admm_pinst.hpp, pseg_kernel): per-QP transfer matrices
  double *Omd = nullptr, *Psd = nullptr, *Segd = nullptr;
  int* pgrow = nullptr;
  bool pi_rows = false;          // small batches: sweeps with a QP's rows spread over lanes (csrc/admm_pinst_rows.hpp)
  bool pi_tiled = false;         // wide shapes: operand arrays A, B, K, S^-1, Omega, Psi in the tiled layout (csrc/admm_pinst.hpp, Operand)
  bool pi_rows_factor = false;   // (6, 3), ADMM_PI_ROWS_FACTOR=1: factorisation / transfer matrices through the wide shapes' kernels
  // per-QP rho (every QP of a per-instance problem has its own factor, so the adaptive rule runs QP by QP on the device)
  double *rho_d = nullptr, *cscale_d = nullptr;     // [pitch]
  int *nupd_d = nullptr, *todo_d = nullptr, *nchanged_d = nullptr;
  size_t stage_rows = 0;         // rows the staging buffer holds (L, or N n^2 for the per-instance upload of A)
  bool alt = false;              // the alternating kernels exist for this problem and are enabled
  // what the last kernel left behind for the next x-update:
  //   ALT_NONE  nothing (the next iteration starts with xb_kernel)
  //   ALT_FWD   xfze ran: db rows | mseg | ebseg -> next: scan (WB) + xbze
  //   ALT_BWD   xbze ran: dbuf | tseg | eseg    -> next: scan (W)  + xfze   (w of that iteration cannot be
  //             re-materialised, so no API call ever returns in this state)
  enum { ALT_NONE = 0, ALT_FWD = 1, ALT_BWD = 2 };
  int alt_state = ALT_NONE;
  int *seg_start = nullptr, *status = nullptr, *iters = nullptr, *nconv = nullptr;
  double* stage = nullptr;      // QP-major staging buffer, L * batch
  int* h_nconv = nullptr;       // pinned
  // pinned bounce buffers of large host-to-device uploads (allocated on first use; upload_h2d)
  unsigned char* pin[2] = {nullptr, nullptr};
  hipEvent_t pin_ev[2] = {nullptr, nullptr};
  // the *_device entry points (ABI v9): ordering against the caller's stream, result slots of the device-side checks
  hipEvent_t ext_ev = nullptr;
  unsigned long long* chk_d = nullptr;
  // certificate (admm_cert_kernels.hpp): raw problem operands and work buffers, allocated and uploaded on the first
  // admm_get_certificate* call; keep_shared() (admm_setup, admm_update_problem) invalidates the operands
  double *certAB = nullptr, *certQR = nullptr, *certPhi = nullptr, *cert_fuel = nullptr;
  double *cert_cseg = nullptr, *cert_cin = nullptr, *cert_part = nullptr, *cert_out = nullptr, *cert_nu = nullptr;
  bool cert_valid = false;       // certAB / certQR / certPhi describe the handle's current problem
  std::vector<double> cert_fuel_h;   // the weights cert_fuel holds (compared with h->fuel at call time)
  // infeasibility probe (admm_infeas_kernels.hpp): snapshot of y, the box and thrust bounds per stage, work buffers,
  // allocated on the first admm_probe_infeasibility* call; the probe shares certAB, certPhi, cert_cseg, cert_cin and cert_nu
  double *infeas_y0 = nullptr, *infeas_bnd = nullptr, *infeas_part = nullptr, *infeas_out = nullptr;
  int* infeas_flag = nullptr;    // [pitch] the flag row of infeas_out as int32 (read-out)
  bool infeas_valid = false;     // infeas_bnd describes the handle's current problem (keep_shared() invalidates it)
  // receding-horizon step (admm_mpc.hip), allocated on the first admm_mpc_advance* call: first blocks of the shift's
  // chunks [arrays][chunks - 1][nb][pitch], work rows of x+ [n][pitch], and the host form's per-QP inputs and outputs
  double *mpc_edge = nullptr, *mpc_xn = nullptr, *mpc_io = nullptr;
  size_t mpc_edge_count = 0;
  int iters_run = 0;
  bool resid_valid = false;
  // A residual-evaluating alternating iteration leaves its finalise to the NEXT scan launch (finalise
  // role of xscan_mfma_kernel); flush_finalize() runs it standalone when no scan follows.
  bool fin_pending = false;
  bool w_stale = false;         // fused iterations do not store w; admm_get re-materialises it
  // State form: the fused path keeps v = z + y only; z, y are rebuilt on demand.
  bool v_valid = false;         // h->v holds the current state
  bool zy_valid = true;         // h->z, h->y hold the current state
  // captured iterations, replayed by admm_run / admm_solve:
  //   [r]: plain iteration, r = 1 with residuals + finalise (it = 0);
  //   [4 t + 2 r + p] (t = IT_FWD_START .. IT_BWD): alternating forms, p = 1 if the scan launch also
  //   finalises the previous iteration's residuals
  hipGraph_t graph[16] = {};
  hipGraphExec_t graph_exec[16] = {};
  // Every device and pinned-host allocation made for this handle, as handle_alloc() returned it (the fields above may hold it
  // biased by the stage window, or swapped with another field): release() frees these and nothing else
  struct Owned { void* ptr; size_t bytes; bool pinned; };
  std::vector<Owned> owned;
};

// live handle-owned device allocations of the process and their bytes (tests/test_gpu_handle_memory.py; not part of the ABI)
extern "C" void admm_debug_handle_memory(int64_t* count, int64_t* bytes);

namespace admm {
namespace rt {

using admm::Z_THREADS;

extern thread_local std::string g_err;       // admm_last_error()
extern thread_local std::string g_warn;      // admm_last_warning(): a call succeeded but changed the kernels a handle runs

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// A call that some kinds cannot serve: ADMM_OK, or the refusal with the reason the table gives in column `why` (no_step / no_probe).
inline int refuse_on_kind(const admm_handle* h, const char* fn, const char* ZKindInfo::*why) {
  const ZKindInfo& k = zkind_info(h->zkind);
  if (!(k.*why)) return ADMM_OK;
  return fail(ADMM_ERR_UNSUPPORTED, std::string(fn) + ": not available on " + k.handle + " (" + k.*why + ")");
}
// A call on one kind's payload: ADMM_OK on a handle of that kind, else that the handle has none (adding: that none can be added).
inline int require_kind(const admm_handle* h, ZKind want, const char* fn, bool adding = false) {
  if (h->zkind == want) return ADMM_OK;
  const ZKindInfo& k = zkind_info(want);
  return fail(ADMM_ERR_INVALID, std::string(fn) + ": " + (adding ? std::string(k.payload) + " cannot be added to a handle"
                                                                 : std::string("the handle has no ") + k.payload) +
                                    " (set it up with " + k.setup + ")");
}

#define HIP_TRY(expr)                                                                         \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return ::admm::rt::fail(ADMM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_) + " (" +     \
                                    __FILE__ + ":" + std::to_string(__LINE__) + ")");          \
  } while (0)

constexpr double ALT_GATE = 5e-12;      // the bound build_alternating applies (csrc/admm_factor.cpp)
constexpr double SCAN_GROWTH_MAX = 100.0;

// Iteration forms.  IT_PLAIN is always available; the others need h->alt and
// the state in v-form.
enum IterForm {
  IT_PLAIN = 0,     // xb + scan + xfz                    leaves ALT_NONE
  IT_FWD_START = 1, // xb + scan + xfze                   leaves ALT_FWD
  IT_FWD = 2,       // scan + xfze        (needs ALT_BWD) leaves ALT_FWD
  IT_BWD = 3        // scan (WB) + xbze   (needs ALT_FWD) leaves ALT_BWD
};

// Host threads for the O(problem size) host loops of the API (finiteness checks, copies into pinned memory): at most 16, never
// more than the work is worth (one per 4 MB).  fn(begin, end) over a partition of [0, count); results are combined by the caller.
template <class F>
void host_parallel(size_t count, size_t bytes_per_item, F&& fn) {
  size_t nt = std::min<size_t>(std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency())),
                               count * bytes_per_item / ((size_t)4 << 20));
  if (nt <= 1) { fn((size_t)0, count); return; }
  std::vector<std::thread> th;
  size_t started = 1;
  try {
    for (size_t t = 1; t < nt; ++t) {
      th.emplace_back([&fn, t, nt, count] { fn(count * t / nt, count * (t + 1) / nt); });
      started = t + 1;
    }
  } catch (...) {                                // no more threads to be had: the remaining slices run here
  }
  fn((size_t)0, count / nt);
  for (size_t t = started; t < nt; ++t) fn(count * t / nt, count * (t + 1) / nt);
  for (auto& x : th) x.join();
}

// device memory that belongs to no handle (the scratch slots of admm_setup_device, the SCvx counter): freed by whoever allocates it
template <typename T>
int dalloc(T** p, size_t count) {
  hipError_t e = hipMalloc((void**)p, sizeof(T) * (count ? count : 1));
  if (e != hipSuccess) return fail(ADMM_ERR_ALLOC, std::string("hipMalloc failed: ") + hipGetErrorString(e));
  return ADMM_OK;
}

// ---- memory of a handle (admm_hostio.hip): every allocation is recorded in h->owned and freed by release().
// zeroed: filled with zeros on the handle's stream (before the stream exists: at once).  The fill is asynchronous, and the handle's
// stream is non-blocking: synchronise it before a null-stream copy into the same array.
int handle_alloc(admm_handle* h, void** p, size_t bytes, bool zeroed, bool pinned);
void handle_free(admm_handle* h, void* p);       // a recorded allocation, before release() (nullptr: nothing)
template <typename T>
int dalloc(admm_handle* h, T** field, size_t count, bool zeroed = false) {
  return handle_alloc(h, (void**)field, sizeof(T) * (count ? count : 1), zeroed, false);
}
template <typename T>
int halloc(admm_handle* h, T** field, size_t count) {      // pinned host memory
  return handle_alloc(h, (void**)field, sizeof(T) * count, false, true);
}
template <typename T>
void dfree(admm_handle* h, T** field) {          // (a field that holds the allocation's own address)
  handle_free(h, *field);
  *field = nullptr;
}

// Device arrays of stage records that a kernel stages by LDS-DMA (glds_chunk, admm_kernels.hpp: recFE / recBE, recMF / recMB):
// a chunk is copied in whole KiB pieces, so its last piece reads up to 1008 bytes past the chunk -- past the ARRAY for the
// last chunk.  Such an array is allocated with a KiB of (zeroed) slack, and every set-up and every upload checks that the
// allocation covers stages x stage_bytes rounded up to the next KiB (admm_record_alloc_check: the same test, host only).
constexpr size_t REC_SLACK_BYTES = 1024;
inline size_t rec_alloc_needed(size_t stages, size_t stage_bytes) { return (stages * stage_bytes + 1023) / 1024 * 1024; }
inline int check_record_alloc(const char* what, size_t alloc_bytes, size_t stages, size_t stage_bytes) {
  if (alloc_bytes >= rec_alloc_needed(stages, stage_bytes)) return ADMM_OK;
  return fail(ADMM_ERR_INVALID, std::string(what) + ": " + std::to_string(alloc_bytes) + " bytes allocated for " + std::to_string(stages) +
              " stage records of " + std::to_string(stage_bytes) + " bytes; the KiB-wise LDS-DMA copy reads up to " +
              std::to_string(rec_alloc_needed(stages, stage_bytes)));
}
// such an array for `payload` bytes of records: allocated with the slack, zeroed; *alloc_bytes = what check_record_alloc is given
template <typename T>
int dalloc_records(admm_handle* h, T** field, size_t payload, size_t* alloc_bytes = nullptr) {
  if (alloc_bytes) *alloc_bytes = payload + REC_SLACK_BYTES;
  return handle_alloc(h, (void**)field, payload + REC_SLACK_BYTES, true, false);
}

// ---- launches, exchange and iteration forms (admm_launch.hip)
admm::XLaunch xlaunch_of(const admm_handle* h);
admm::PLaunch plaunch_of(const admm_handle* h);
int launch_p(admm_handle* h, admm::PKernel k, bool vform, bool resid);
bool dispatch_x(const admm::XLaunch& l, admm::XKernel k, bool a, bool b, bool query_only);
bool dims_supported(int n, int m);
std::string supported_list();
int launch_x(admm_handle* h, admm::XKernel k, bool a, bool b);
admm::FinArgs fin_args(const admm_handle* h, int it, int nchunks);
int ts_allgather(admm_handle* h, double* base, size_t count_per_rank);
int ts_exchange_summaries(admm_handle* h);
int ts_exchange_partials(admm_handle* h);
int launch_xscan_mfma(admm_handle* h, bool forward_form = false, bool with_finalize = false);
int launch_xscan(admm_handle* h);
int ensure_zy(admm_handle* h);
int launch_z(admm_handle* h, bool resid);
int launch_finalize(admm_handle* h, int it, int nchunks);
int flush_finalize(admm_handle* h, int it = 0);
IterForm next_form(const admm_handle* h, int remaining);
int enqueue_form(admm_handle* h, IterForm f, bool resid, bool fin_prev);
void after_form(admm_handle* h, IterForm f);
int enqueue_iteration(admm_handle* h, bool resid, bool use_v);
void after_iterations(admm_handle* h, int count);
int ensure_w(admm_handle* h);
int step_x(admm_handle* h);
int capture_iterations(admm_handle* h);
int enqueue_one(admm_handle* h, bool resid, bool use_graph, int remaining, int it_number = 0, bool next_plain = false,
                bool next_resid = false);

// ---- host <-> device transfers, validation, uploads of the factor, handle lifetime (admm_hostio.hip)
int upload_h2d(admm_handle* h, void* dst, const void* src, size_t bytes);
int download_d2h(admm_handle* h, void* dst, const void* src, size_t bytes);   // ... and back; returns with the copy complete
// Where the caller's array (src of an upload, dst of a download) lives.  Mem::Device: memory of the handle's GPU; it is then read /
// written by the layout kernels directly, and a download returns with its kernel queued on the handle's stream
enum class Mem { Host, Device };
int upload_tiled(admm_handle* h, Mem mem, const double* src, double* dst, int E, int nr = 0, int nc = 0);   // per-instance operand (batch x N x E) -> tiled layout; nr x nc: row-major source blocks
int upload_transposed(admm_handle* h, Mem mem, const double* src, double* dst, int rows, int nr = 0, int nc = 0);   // nr x nc: the rows are stacks of row-major blocks
int download_transposed(admm_handle* h, Mem mem, const double* src, double* dst, int rows);
bool finite_all(const double* a, size_t cnt);
int validate_options(const admm_options* o);
// What the device-side checks of a *_device call found in the caller's large arrays; validate_problem reads these instead of
// the arrays themselves (which it cannot dereference), so both forms refuse the same data with the same status and message.
struct DeviceScan {
  bool ab_bad = false;               // a non-finite entry in per-instance A or B
  size_t bnd_bad = SIZE_MAX;         // per-instance box: smallest offending index ...
  double bnd_lo = 0.0, bnd_hi = 0.0; // ... and its lo, hi
  size_t un_stage = SIZE_MAX;        // per-instance box: smallest stage whose finite unorm meets a bounded control row of some QP
  bool x0_bad = false, q_bad = false;
};
// A problem whose arrays are device memory, as the library uses it: the small arrays (Q, R, QN, unorm; batch-shared A, B and box)
// copied to the host, the per-instance ones (per-instance A, B and box, x0, q) still the caller's device pointers.
struct DeviceProblem {
  admm_problem hp{};
  std::vector<double> A, B, Q, R, QN, lo, hi, un;
  DeviceScan scan;
};
int validate_dims(const admm_problem* p);
int validate_problem(const admm_problem* p, const DeviceScan* d = nullptr);
int check_device_ptr(int device, const void* ptr, size_t bytes, const char* fn, const char* name, size_t elem = sizeof(double),
                     const char* unit = "doubles");   // elem, unit: the array's element (alignment, the count the message names)
// The device-side finite check: CHK_SLOTS result slots (admm_handle::chk_d), slot i the smallest offending index of arrays[i] or
// CHK_NONE.  finite_scan_begin sets every slot to CHK_NONE and queues one pass per array given (ptr = NULL: none); a caller may queue checks
// of its own into free slots; finite_scan_end copies the slots back and synchronises s: one synchronisation for all of them.
struct FiniteArg { const double* ptr; size_t count; const char* name; };
constexpr int CHK_SLOTS = 8;
constexpr unsigned long long CHK_NONE = ~0ull;
int finite_scan_begin(hipStream_t s, unsigned long long* slots, const FiniteArg* arrays, size_t count);
int finite_scan_end(hipStream_t s, const unsigned long long* slots, unsigned long long (&found)[CHK_SLOTS]);
int prepare_device_problem(int device, hipStream_t s, const admm_problem* p, const char* fn, unsigned long long* scratch,
                           DeviceProblem& d);
int check_scratch(admm_handle* h);

// The caller-array contract of a handle call that exists in a host and a *_device form: both forms are ONE body
// that goes through this object wherever the caller's arrays are named.  Mem::Host: the arrays are host memory, hip_stream is
// ignored.  Mem::Device: they are memory of the handle's GPU, written / read in the order of hip_stream (NULL: the caller vouches
// for its data, and a call with results returns with them complete).
struct CallerIO {
  admm_handle* h;
  const char* fn;                // the entry point, as the messages name it
  Mem mem;
  CallerIO(admm_handle* h_, const char* fn_, Mem mem_, void* hip_stream)
      : h(h_), fn(fn_), mem(mem_), asked(mem_ == Mem::Device ? static_cast<hipStream_t>(hip_stream) : nullptr) {}
  bool dev() const { return mem == Mem::Device; }
  // device call: ptr (NULL: not given) is memory of the handle's GPU, aligned to elem, its allocation at least `bytes` long
  int check_ptr(const void* ptr, size_t bytes, const char* name, size_t elem = sizeof(double), const char* unit = "doubles") const;
  // the handle's stream waits for what the caller has queued on its stream so far
  int begin();
  // *bad = index of the first array given (ptr != NULL) that holds a non-finite entry, -1 if none does.  Host call: finite_all.
  // Device call, after begin(): one pass per array on the handle's stream and one synchronisation; none at all with no array given.
  int check_finite(std::initializer_list<FiniteArg> arrays, int* bad);
  // a device-resident result to the caller's array, queued on the handle's stream (a host copy is complete after finish())
  int copy_out(void* dst, const void* src, size_t bytes);
  // Host call, or no stream given: returns with the handle's stream idle.  Otherwise the caller's stream waits for what the handle's
  // stream holds, without a host synchronisation.
  int finish();
 private:
  hipStream_t asked;             // the caller's stream of a device call
  hipStream_t ordered = nullptr; // ... once begin() has ordered the handle's stream after it (and h->ext_ev exists): finish() hands over to this one only
};
void set_mixed_form(admm_handle* h, bool fp32);
void warn_alt_gate(const admm::Factor& f, double rho, const char* when);
double scan_growth(const admm::Factor& f);
void destroy_graph(admm_handle* h);
void release(admm_handle* h);
// a handle under construction: released when set-up returns early, with the message of the failure kept
struct HandleReleaser {
  void operator()(admm_handle* h) const { std::string keep = g_err; release(h); g_err = keep; }
};
using HandleGuard = std::unique_ptr<admm_handle, HandleReleaser>;
int upload_scan_dense(const std::vector<double>& W, int M, int K, double* Wd, int* rows_d);
int upload_factor(admm_handle* h, const char* when = "refactor");   // when: the call, as the messages and the warning name it
int upload_bounds(admm_handle* h, const admm_problem* p);
void keep_shared(admm_handle* h, const admm_problem* p);
bool problem_has_soc(const admm_problem* p);
int validate_fuel(const admm_problem* p, const double* fuel, bool per_stage);
int upload_kappa(admm_handle* h);
// soft weights against a validated problem: cnt entries, >= 0, no NaN (+inf = hard), and +inf on the control rows of a stage with a
// finite thrust bound or a positive fuel weight.  expanded = false: `soft` has lo's shape (nb entries with stage_bounds = 0, else nb N);
// true: L entries (a handle's own copy).  fuel: N per-stage weights or NULL.
int validate_soft(const admm_problem* p, const double* soft, bool expanded, const double* fuel);
inline const double* fuel_of(const admm_handle* h) { return h->has_fuel ? h->fuel.data() : nullptr; }
// half-spaces against a validated problem.  halfspace_stages: a, b as the caller gives them (a[b][k][i], b[b][k]; one "QP" in the
// shared form) must be finite and every a_k'a_k of a stage with a plane a normal number; any[k] = some QP has a plane at stage k.
// halfspace_box_open: the state rows 0 .. nh - 1 of every stage in `any` have the box (-inf, inf) in p (a batch-shared box).
int halfspace_stages(const char* fn, const double* a, const double* b, int count, int N, int nh, std::vector<char>& any);
int halfspace_box_open(const char* fn, const admm_problem* p, const std::vector<char>& any, int nh, const char* what = "a half-space");
// the planes of a half-space handle into h->hs_a / h->hs_b (admm_zext.hip); returns with the copies complete
int upload_halfspace(admm_handle* h, Mem mem, const double* a, const double* b);
// approach cones against a validated problem: c, apex, gamma as the caller gives them (c[b][k][i], apex[b][k][i], gamma[b][k]; one
// "QP" in the shared form) must be finite, and where c_k != 0 c_k'c_k a normal number and gamma a positive normal number with
// 1 + gamma^2 finite; any[k] = some QP has a cone at stage k.  The open-box rule is halfspace_box_open's.
int cone_stages(const char* fn, const double* c, const double* apex, const double* gamma, int count, int N, int nh, std::vector<char>& any);
// the cones of such a handle into h->cone_c / cone_p / cone_g (admm_zext.hip); returns with the copies complete
int upload_cone(admm_handle* h, Mem mem, const double* c, const double* apex, const double* gamma);

// ---- per-instance dynamics (admm_pinst_rt.hip)
int pinst_factor(admm_handle* h, bool only_marked = false);
int pinst_fill_rho(admm_handle* h, double rho);
int pinst_upload_dynamics(admm_handle* h, const admm_problem* p, double* Ad, double* Bd, double* Qd, double* Rd, double* QNd,
                          Mem mem);   // mem: where A, B live (the weights are host arrays either way)
int pinst_upload_bounds(admm_handle* h, const admm_problem* p, Mem mem);   // mem: where a per-instance box lives
int pinst_upload(admm_handle* h, const admm_problem* p, Mem mem);
int pinst_alloc_trial(admm_handle* h, bool dynamics);
int pinst_try(admm_handle* h, const double* Ad, const double* Bd, const double* Qd, const double* Rd, const double* QNd,
              const double* rhov, const int* todo, int* n_not_pd, int* n_grown);
int pinst_segments(admm_handle* h);
int setup_pinst(admm_handle* h, const admm_problem* p, Mem mem);
void choose_zchunks(admm_handle* h, int zrows);   // admm_setup.hip; zrows = 0: one workgroup per CU

// ---- refactors: background candidates of the adaptive rule, rho changes (admm_rho_update.hip)
admm_problem shared_problem(const admm_handle* h);
bool spec_enabled(const admm_handle* h);
void spec_reap(admm_handle* h, bool all);
std::unique_ptr<SpecFactor> spec_take(admm_handle* h, double rho);
void spec_start(admm_handle* h);
int set_rho_internal(admm_handle* h, double rho_new);
int update_problem_checked(admm_handle* h, const admm_problem* p, Mem mem);

// ---- the stage window of the big per-stage arrays (see admm_handle::wk0)
inline size_t win_row0(const admm_handle* h) { return (size_t)h->wk0 * h->nb; }                       // first stacked row held
inline size_t win_rows(const admm_handle* h) { return (size_t)(h->wk1 - h->wk0) * h->nb; }            // stacked rows held
inline size_t win_bias(const admm_handle* h) { return win_row0(h) * (size_t)h->pitch; }               // elements the state pointers are biased by
inline size_t win_bias_m(const admm_handle* h) { return (size_t)h->wk0 * h->m * (size_t)h->pitch; }   // ... dbuf / mvec
inline bool windowed(const admm_handle* h) { return h->wk0 != 0 || h->wk1 != h->N; }

// ---- one-line helpers
// vform: read the state from h->v (z = clip(v), y = v - z rebuilt in registers)
inline int launch_xb(admm_handle* h, bool vform) { return launch_x(h, admm::XKernel::XB, vform, false); }
inline int launch_xf(admm_handle* h) { return launch_x(h, admm::XKernel::XF, false, false); }
// fused forward rollout + z/dual (+ residual partials per segment); writes v+ into h->v.
// vin: previous state read from h->v, otherwise from h->z / h->y.
inline int launch_xfz(admm_handle* h, bool resid, bool vin) { return launch_x(h, admm::XKernel::XFZ, vin, resid); }
inline bool fused(const admm_handle* h) { return !(h->opt.flags & ADMM_FLAG_UNFUSED); }
// whatever changes the state, the factor or the instance data outside enqueue_one drops the lean forms' side data
inline void drop_side_data(admm_handle* h) { h->side_valid = false; h->lean_mode = 0; }
bool lean_capable(const admm_handle* h);
inline int chunks_of_iteration(const admm_handle* h) { return fused(h) ? h->S : h->zchunks; }

}  // namespace rt
}  // namespace admm
