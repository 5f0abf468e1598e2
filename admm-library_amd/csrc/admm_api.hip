// admm_api.hip -- C ABI of libadmm_hip.so (include/admm_hip.h): state, iteration, solve, read-out.  Set-up is admm_setup.hip, the fuel term's
// and the z-update extensions' entry points admm_zext.hip; the runtime behind them is split over admm_launch.hip, admm_hostio.hip,
// admm_rho_update.hip, admm_pinst_rt.hip, admm_profile.hip (admm_runtime.hpp).  No CPU fallback: without a HIP device every compute entry
// point returns ADMM_ERR_NO_DEVICE.
#include "admm_runtime.hpp"
#include "admm_cert.hpp"
#include "admm_infeas.hpp"

using namespace admm::rt;

extern "C" {

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
      if (h->zkind == ZKind::Soft)          // a row with a finite weight can be violated at a price: open for feasibility
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
  int rc;
  if ((rc = refuse_on_kind(h, fn, &ZKindInfo::no_probe))) return rc;
  if (h->opt.precision_mode == ADMM_PRECISION_MIXED)
    return fail(ADMM_ERR_UNSUPPORTED, std::string(fn) + ": not available with precision_mode MIXED (the fp32 phase would put rounding "
                "noise into the dual's difference)");
  HIP_TRY(hipSetDevice(h->device));
  CallerIO io(h, fn, mem, hip_stream);
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
