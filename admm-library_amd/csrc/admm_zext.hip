// admm_zext.hip -- entry points of what extends the z-update of a handle (admm_runtime.hpp): the fuel term, which
// composes with every kind, and the payload of each ZKind -- scenario groups, soft weights, half-spaces, approach cones: set, get,
// report.  Their set-up entry points are in admm_setup.hip, their kernels behind admm_consensus.hpp, admm_soft.hpp,
// admm_halfspace.hpp and admm_cone.hpp.
#include "admm_runtime.hpp"
#include "admm_consensus.hpp"
#include "admm_soft.hpp"
#include "admm_halfspace.hpp"
#include "admm_cone.hpp"

using namespace admm::rt;

namespace admm {
namespace rt {

// the planes of a half-space handle into h->hs_a / h->hs_b (their addresses never change): the shared form as it is, the per-QP
// form through the transposing upload.  Returns with the copies complete.
int upload_halfspace(admm_handle* h, Mem mem, const double* a, const double* b) {
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

// the cones of a cone handle into h->cone_c / cone_p / cone_g (their addresses never change), as upload_halfspace does the planes
int upload_cone(admm_handle* h, Mem mem, const double* c, const double* apex, const double* gamma) {
  int rc;
  const int rows = h->N * h->cone_nh;
  if (h->cone_perqp) {
    if ((rc = upload_transposed(h, mem, c, h->cone_c, rows)) || (rc = upload_transposed(h, mem, apex, h->cone_p, rows)) ||
        (rc = upload_transposed(h, mem, gamma, h->cone_g, h->N)))
      return rc;
    return ADMM_OK;
  }
  const hipMemcpyKind kind = mem == Mem::Device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HIP_TRY(hipMemcpyAsync(h->cone_c, c, sizeof(double) * (size_t)rows, kind, h->stream));
  HIP_TRY(hipMemcpyAsync(h->cone_p, apex, sizeof(double) * (size_t)rows, kind, h->stream));
  HIP_TRY(hipMemcpyAsync(h->cone_g, gamma, sizeof(double) * (size_t)h->N, kind, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return ADMM_OK;
}

}  // namespace rt
}  // namespace admm

// penalty, largest violation and violated rows of every QP at the handle's z (soft_report_kernel)
static int soft_report_common(admm_handle* h, double* penalty, double* max_violation, int32_t* n_violated, Mem mem, void* hip_stream) {
  const char* fn = mem == Mem::Device ? "admm_get_soft_report_device" : "admm_get_soft_report";
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  if (!penalty && !max_violation && !n_violated) return fail(ADMM_ERR_INVALID, std::string(fn) + ": at least one output must be given");
  int rc;
  if ((rc = require_kind(h, ZKind::Soft, fn))) return rc;
  HIP_TRY(hipSetDevice(h->device));
  CallerIO io(h, fn, mem, hip_stream);
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

// New planes on a half-space handle, same form and nh: nothing of the handle is written before every check has passed.  The
// state is the (z, y) pair already (such a handle never enters the v-form) and the factor does not depend on the planes.
static int set_halfspace_common(admm_handle* h, const double* a, const double* b, Mem mem, void* hip_stream) {
  const char* fn = mem == Mem::Device ? "admm_set_halfspace_device" : "admm_set_halfspace";
  if (!h || !a || !b) return fail(ADMM_ERR_INVALID, "NULL argument");
  g_warn.clear();
  int rc;
  if ((rc = require_kind(h, ZKind::Halfspace, fn, /*adding=*/true))) return rc;
  HIP_TRY(hipSetDevice(h->device));
  CallerIO io(h, fn, mem, hip_stream);
  const int cnt = h->hs_perqp ? h->batch : 1, N = h->N, nh = h->hs_nh;
  const size_t na = (size_t)cnt * N * nh, nbv = (size_t)cnt * N;
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

// largest violation of a plane by w, the stages with a positive multiplier, and the multipliers (halfspace_report_kernel)
static int halfspace_report_common(admm_handle* h, double* max_violation, int32_t* n_active, double* lam, Mem mem, void* hip_stream) {
  const char* fn = mem == Mem::Device ? "admm_get_halfspace_report_device" : "admm_get_halfspace_report";
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  if (!max_violation && !n_active && !lam) return fail(ADMM_ERR_INVALID, std::string(fn) + ": at least one output must be given");
  int rc;
  if ((rc = require_kind(h, ZKind::Halfspace, fn))) return rc;
  HIP_TRY(hipSetDevice(h->device));
  CallerIO io(h, fn, mem, hip_stream);
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

// New cones on a cone handle, same form and nh: set_halfspace_common's order -- nothing of the handle is written before every
// check has passed; the state is the (z, y) pair already and the factor does not depend on the cones.
static int set_cone_common(admm_handle* h, const double* c, const double* apex, const double* gamma, Mem mem, void* hip_stream) {
  const char* fn = mem == Mem::Device ? "admm_set_cone_device" : "admm_set_cone";
  if (!h || !c || !apex || !gamma) return fail(ADMM_ERR_INVALID, "NULL argument");
  g_warn.clear();
  int rc;
  if ((rc = require_kind(h, ZKind::Cone, fn, /*adding=*/true))) return rc;
  HIP_TRY(hipSetDevice(h->device));
  CallerIO io(h, fn, mem, hip_stream);
  const int cnt = h->cone_perqp ? h->batch : 1, N = h->N, nh = h->cone_nh;
  const size_t nc = (size_t)cnt * N * nh, ng = (size_t)cnt * N;
  if ((rc = io.check_ptr(c, nc * sizeof(double), "c")) || (rc = io.check_ptr(apex, nc * sizeof(double), "apex")) ||
      (rc = io.check_ptr(gamma, ng * sizeof(double), "gamma")))
    return rc;
  std::vector<char> any;
  if (!io.dev()) {
    if ((rc = cone_stages(fn, c, apex, gamma, cnt, N, nh, any))) return rc;
  } else {
    int bad;
    if ((rc = io.begin()) || (rc = io.check_finite({{c, nc, "c"}, {apex, nc, "apex"}, {gamma, ng, "gamma"}}, &bad))) return rc;
    if (bad >= 0) return fail(ADMM_ERR_INVALID, std::string(fn) + ": non-finite entry in c, apex or gamma");
    if (h->cone_perqp) {            // the device-side findings: which stages have a cone for some QP, and whether a c'c or a slope is unusable
      if (!h->cone_flags && (rc = dalloc(h, &h->cone_flags, (size_t)3 * N))) return rc;
      std::vector<int> fl((size_t)3 * N);
      HIP_TRY(hipMemsetAsync(h->cone_flags, 0, sizeof(int) * fl.size(), h->stream));
      admm::launch_cone_scan(h->stream, c, gamma, h->batch, N, nh, h->cone_flags);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(fl.data(), h->cone_flags, sizeof(int) * fl.size(), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(hipStreamSynchronize(h->stream));
      any.assign(N, 0);
      for (int k = 0; k < N; ++k) {
        if (fl[N + k]) return fail(ADMM_ERR_INVALID, std::string(fn) + ": c'c of stage " + std::to_string(k) + " is not a normal number (scale the axis)");
        if (fl[2 * N + k])
          return fail(ADMM_ERR_INVALID, std::string(fn) + ": gamma of stage " + std::to_string(k) + " must be a positive normal number with 1 + gamma^2 finite");
        any[k] = fl[k] != 0;
      }
    } else {                        // the shared form is N (2 nh + 1) doubles: checked on the host, as a DeviceProblem's small arrays are
      std::vector<double> ch(nc), ph(nc), gh(ng);
      HIP_TRY(hipMemcpyAsync(ch.data(), c, sizeof(double) * nc, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(hipMemcpyAsync(ph.data(), apex, sizeof(double) * nc, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(hipMemcpyAsync(gh.data(), gamma, sizeof(double) * ng, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(hipStreamSynchronize(h->stream));
      if ((rc = cone_stages(fn, ch.data(), ph.data(), gh.data(), 1, N, nh, any))) return rc;
    }
  }
  const admm_problem p = shared_problem(h);
  if ((rc = halfspace_box_open(fn, &p, any, nh, "a cone"))) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));   // kernels of the old cones are done before they change
  if ((rc = upload_cone(h, mem, c, apex, gamma))) return rc;
  h->cone_any = any;
  return io.finish();
}

// largest violation of a cone by w, the stages whose y_xi is not zero, and rho |y_xi| (cone_report_kernel)
static int cone_report_common(admm_handle* h, double* max_violation, int32_t* n_active, double* lam, Mem mem, void* hip_stream) {
  const char* fn = mem == Mem::Device ? "admm_get_cone_report_device" : "admm_get_cone_report";
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  if (!max_violation && !n_active && !lam) return fail(ADMM_ERR_INVALID, std::string(fn) + ": at least one output must be given");
  int rc;
  if ((rc = require_kind(h, ZKind::Cone, fn))) return rc;
  HIP_TRY(hipSetDevice(h->device));
  CallerIO io(h, fn, mem, hip_stream);
  const size_t bsz = sizeof(double) * (size_t)h->batch, csz = sizeof(int32_t) * (size_t)h->batch;
  if ((rc = io.check_ptr(max_violation, bsz, "max_violation")) ||
      (rc = io.check_ptr(n_active, csz, "n_active", sizeof(int32_t), "int32 entries")) || (rc = io.check_ptr(lam, bsz * h->N, "lam")))
    return rc;
  if (!h->cone_out && (rc = dalloc(h, &h->cone_out, (size_t)h->pitch))) return rc;
  if (!h->cone_cnt && (rc = dalloc(h, &h->cone_cnt, (size_t)h->pitch))) return rc;
  if (lam && !h->cone_lam && (rc = dalloc(h, &h->cone_lam, (size_t)h->N * h->pitch, true))) return rc;
  if ((rc = ensure_w(h)) || (rc = ensure_zy(h))) return rc;      // w of the last x-update; the state as the (z, y) pair
  if ((rc = io.begin())) return rc;
  admm::launch_cone_report(h->stream, h->w, h->y, h->cone_c, h->cone_p, h->cone_g, h->cone_out, h->cone_cnt, lam ? h->cone_lam : nullptr,
                           h->fac.rho, h->N, h->nb, h->m, h->cone_nh, h->pitch, h->batch, h->cone_perqp);
  HIP_TRY(hipGetLastError());
  if (max_violation && (rc = io.copy_out(max_violation, h->cone_out, bsz))) return rc;
  if (n_active && (rc = io.copy_out(n_active, h->cone_cnt, csz))) return rc;
  if (lam && (rc = download_transposed(h, mem, h->cone_lam, lam, h->N))) return rc;
  return io.finish();
}

// the control rows of each group's z, (ngroups, N, m): column g * G of the rows j < m of every block (consensus_gather_kernel)
static int consensus_common(admm_handle* h, double* ubar, Mem mem, void* hip_stream) {
  const char* fn = mem == Mem::Device ? "admm_get_consensus_device" : "admm_get_consensus";
  if (!h || !ubar) return fail(ADMM_ERR_INVALID, "NULL argument");
  int rc;
  if ((rc = require_kind(h, ZKind::Consensus, fn))) return rc;
  HIP_TRY(hipSetDevice(h->device));
  CallerIO io(h, fn, mem, hip_stream);
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

extern "C" {

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
  if (h->zkind == ZKind::Soft) {              // a stage that gains a fuel weight must not hold a finite soft weight on its control rows
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

int admm_get_consensus(admm_handle* h, double* ubar) { return consensus_common(h, ubar, Mem::Host, nullptr); }
int admm_get_consensus_device(admm_handle* h, double* ubar, void* hip_stream) { return consensus_common(h, ubar, Mem::Device, hip_stream); }

int admm_get_soft(admm_handle* h, double* soft) {
  if (!h || !soft) return fail(ADMM_ERR_INVALID, "NULL argument");
  for (int e = 0; e < h->L; ++e) soft[e] = h->zkind == ZKind::Soft ? h->soft[e] : INFINITY;
  return ADMM_OK;
}

// New weights on a soft handle: nothing of the handle is written before every check has passed.  The state is the (z, y) pair
// already (such a handle never enters the v-form); the factor does not depend on the weights, so only kappa is refreshed.
int admm_set_soft(admm_handle* h, const double* soft) {
  if (!h || !soft) return fail(ADMM_ERR_INVALID, "NULL argument");
  g_warn.clear();
  int rc;
  if ((rc = require_kind(h, ZKind::Soft, "admm_set_soft", /*adding=*/true))) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const admm_problem p = shared_problem(h);
  if ((rc = validate_soft(&p, soft, false, fuel_of(h)))) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));   // kernels of the old weights are done before kappa changes
  for (int e = 0; e < h->L; ++e) h->soft[e] = soft[(h->stage_bounds ? (size_t)(e / h->nb) * h->nb : 0) + e % h->nb];
  h->infeas_valid = false;                    // the probe's bound table opens the rows with a finite weight
  return upload_kappa(h);
}

int admm_get_soft_report(admm_handle* h, double* penalty, double* max_violation, int32_t* n_violated) {
  return soft_report_common(h, penalty, max_violation, n_violated, Mem::Host, nullptr);
}
int admm_get_soft_report_device(admm_handle* h, double* penalty, double* max_violation, int32_t* n_violated, void* hip_stream) {
  return soft_report_common(h, penalty, max_violation, n_violated, Mem::Device, hip_stream);
}

int admm_set_halfspace(admm_handle* h, const double* a, const double* b) { return set_halfspace_common(h, a, b, Mem::Host, nullptr); }
int admm_set_halfspace_device(admm_handle* h, const double* a, const double* b, void* hip_stream) {
  return set_halfspace_common(h, a, b, Mem::Device, hip_stream);
}

// the planes in force, in the caller's order (a[b][k][i], b[b][k]; one "QP" in the shared form)
int admm_get_halfspace(admm_handle* h, double* a, double* b) {
  if (!h || !a || !b) return fail(ADMM_ERR_INVALID, "NULL argument");
  int rc;
  if ((rc = require_kind(h, ZKind::Halfspace, "admm_get_halfspace"))) return rc;
  HIP_TRY(hipSetDevice(h->device));
  if (h->hs_perqp) {
    if ((rc = download_transposed(h, Mem::Host, h->hs_a, a, h->N * h->hs_nh))) return rc;
    return download_transposed(h, Mem::Host, h->hs_b, b, h->N);
  }
  HIP_TRY(hipMemcpyAsync(a, h->hs_a, sizeof(double) * (size_t)h->N * h->hs_nh, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(b, h->hs_b, sizeof(double) * (size_t)h->N, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return ADMM_OK;
}

int admm_get_halfspace_report(admm_handle* h, double* max_violation, int32_t* n_active, double* lam) {
  return halfspace_report_common(h, max_violation, n_active, lam, Mem::Host, nullptr);
}
int admm_get_halfspace_report_device(admm_handle* h, double* max_violation, int32_t* n_active, double* lam, void* hip_stream) {
  return halfspace_report_common(h, max_violation, n_active, lam, Mem::Device, hip_stream);
}

int admm_set_cone(admm_handle* h, const double* c, const double* apex, const double* gamma) {
  return set_cone_common(h, c, apex, gamma, Mem::Host, nullptr);
}
int admm_set_cone_device(admm_handle* h, const double* c, const double* apex, const double* gamma, void* hip_stream) {
  return set_cone_common(h, c, apex, gamma, Mem::Device, hip_stream);
}

// the cones in force, in the caller's order (c[b][k][i], apex[b][k][i], gamma[b][k]; one "QP" in the shared form)
int admm_get_cone(admm_handle* h, double* c, double* apex, double* gamma) {
  if (!h || !c || !apex || !gamma) return fail(ADMM_ERR_INVALID, "NULL argument");
  int rc;
  if ((rc = require_kind(h, ZKind::Cone, "admm_get_cone"))) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const int rows = h->N * h->cone_nh;
  if (h->cone_perqp) {
    if ((rc = download_transposed(h, Mem::Host, h->cone_c, c, rows)) || (rc = download_transposed(h, Mem::Host, h->cone_p, apex, rows)))
      return rc;
    return download_transposed(h, Mem::Host, h->cone_g, gamma, h->N);
  }
  HIP_TRY(hipMemcpyAsync(c, h->cone_c, sizeof(double) * (size_t)rows, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(apex, h->cone_p, sizeof(double) * (size_t)rows, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(gamma, h->cone_g, sizeof(double) * (size_t)h->N, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return ADMM_OK;
}

int admm_get_cone_report(admm_handle* h, double* max_violation, int32_t* n_active, double* lam) {
  return cone_report_common(h, max_violation, n_active, lam, Mem::Host, nullptr);
}
int admm_get_cone_report_device(admm_handle* h, double* max_violation, int32_t* n_active, double* lam, void* hip_stream) {
  return cone_report_common(h, max_violation, n_active, lam, Mem::Device, hip_stream);
}

}  // extern "C"
