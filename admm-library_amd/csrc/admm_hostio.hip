// admm_hostio.hip -- solver runtime: host <-> device transfers, validation, uploads of a factor, handle lifetime (admm_runtime.hpp)
#include "admm_runtime.hpp"
#include "admm_halfspace.hpp"
#include "admm_cone.hpp"

namespace admm {
namespace rt {


// Host -> device copy of a caller's (pageable) array.  Large ones go through two pinned bounce buffers: host threads fill one
// while the DMA engine drains the other -- hipMemcpy from pageable memory alone ran at a few GB/s and made
// admm_update_problem of 4096 x 1000 per-instance stages a 0.7 s call (round 2).
constexpr size_t PIN_BYTES = (size_t)32 << 20;
int upload_h2d(admm_handle* h, void* dst, const void* src, size_t bytes) {
  if (bytes < 2 * PIN_BYTES) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    return ADMM_OK;
  }
  int rc;
  for (int i = 0; i < 2; ++i) {
    if (!h->pin[i] && (rc = halloc(h, &h->pin[i], PIN_BYTES))) return rc;
    if (!h->pin_ev[i]) HIP_TRY(hipEventCreateWithFlags(&h->pin_ev[i], hipEventDisableTiming));
  }
  int slot = 0;
  for (size_t off = 0; off < bytes; off += PIN_BYTES, slot ^= 1) {
    const size_t len = std::min(PIN_BYTES, bytes - off);
    HIP_TRY(hipEventSynchronize(h->pin_ev[slot]));            // the copy that last read this buffer is done (no-op if never recorded)
    unsigned char* pb = h->pin[slot];
    const unsigned char* sb = static_cast<const unsigned char*>(src) + off;
    host_parallel(len, 1, [pb, sb](size_t b, size_t e) { std::memcpy(pb + b, sb + b, e - b); });
    HIP_TRY(hipMemcpyAsync(static_cast<unsigned char*>(dst) + off, pb, len, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipEventRecord(h->pin_ev[slot], h->stream));
  }
  return ADMM_OK;
}

// Device -> host copy into a caller's (pageable) array, the mirror of upload_h2d: the DMA engine fills one pinned buffer while host
// threads empty the other into the caller's memory (admm_get of three 295 MB vectors: 57 ms through pageable copies).
int download_d2h(admm_handle* h, void* dst, const void* src, size_t bytes) {
  if (bytes < 2 * PIN_BYTES) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return ADMM_OK;
  }
  int slot = 0, rc;
  for (int i = 0; i < 2; ++i) {
    if (!h->pin[i] && (rc = halloc(h, &h->pin[i], PIN_BYTES))) return rc;
    if (!h->pin_ev[i]) HIP_TRY(hipEventCreateWithFlags(&h->pin_ev[i], hipEventDisableTiming));
  }
  HIP_TRY(hipEventSynchronize(h->pin_ev[0]));                 // (an upload may have been the buffers' last user)
  HIP_TRY(hipEventSynchronize(h->pin_ev[1]));
  auto drain = [&](int slot, size_t off, size_t len) -> int {
    HIP_TRY(hipEventSynchronize(h->pin_ev[slot]));            // the DMA into this buffer is done
    const unsigned char* pb = h->pin[slot];
    unsigned char* db = static_cast<unsigned char*>(dst) + off;
    host_parallel(len, 1, [pb, db](size_t b, size_t e) { std::memcpy(db + b, pb + b, e - b); });
    return ADMM_OK;
  };
  size_t prev_off = 0, prev_len = 0;
  for (size_t off = 0; off < bytes; off += PIN_BYTES, slot ^= 1) {
    const size_t len = std::min(PIN_BYTES, bytes - off);
    HIP_TRY(hipMemcpyAsync(h->pin[slot], static_cast<const unsigned char*>(src) + off, len, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipEventRecord(h->pin_ev[slot], h->stream));
    if (prev_len && (rc = drain(slot ^ 1, prev_off, prev_len))) return rc;     // the previous chunk, while this one is in flight
    prev_off = off;
    prev_len = len;
  }
  return drain(slot ^ 1, prev_off, prev_len);
}

// QP-major host array (batch x rows) -> batch-minor device array (rows x pitch)
int upload_transposed(admm_handle* h, Mem mem, const double* src, double* dst, int rows, int nr, int nc) {
  const bool dev = mem == Mem::Device;
  if (rows == h->L && windowed(h)) {
    if (dev) return fail(ADMM_ERR_UNSUPPORTED, "internal: device-memory source on a time-sharded handle");
    // a state-sized array of a handle that holds a stage window only: rows [r0, r0 + Lw) of every QP's vector (a strided 2-D
    // copy out of the caller's L x batch array), transposed into the window (dst is the biased pointer)
    const size_t r0 = win_row0(h), Lw = win_rows(h);
    HIP_TRY(hipMemcpy2DAsync(h->stage, Lw * sizeof(double), src + r0, (size_t)h->L * sizeof(double), Lw * sizeof(double), h->batch,
                             hipMemcpyHostToDevice, h->stream));
    dim3 gridw(((int)Lw + admm::T_TILE - 1) / admm::T_TILE, (h->pitch + admm::T_TILE - 1) / admm::T_TILE), blockw(admm::T_TILE * 8);
    hipLaunchKernelGGL(admm::to_batch_minor_kernel, gridw, blockw, 0, h->stream, h->stage, dst + win_bias(h), h->batch, (int)Lw, h->pitch, 0, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    return ADMM_OK;
  }
  const double* staged = src;                 // (a device-memory source is read by the kernel where it is)
  if (!dev) {
    if ((size_t)rows > h->stage_rows) return fail(ADMM_ERR_INVALID, "internal: staging buffer too small");
    int rc_up;
    if ((rc_up = upload_h2d(h, h->stage, src, sizeof(double) * (size_t)rows * h->batch))) return rc_up;
    staged = h->stage;
  }
  dim3 grid((rows + admm::T_TILE - 1) / admm::T_TILE, (h->pitch + admm::T_TILE - 1) / admm::T_TILE), block(admm::T_TILE * 8);
  hipLaunchKernelGGL(admm::to_batch_minor_kernel, grid, block, 0, h->stream, staged, dst, h->batch, rows, h->pitch, nr, nc);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  return ADMM_OK;
}

// QP-major host operand (batch x N x E) -> the wide shapes' tiled device layout
int upload_tiled(admm_handle* h, Mem mem, const double* src, double* dst, int E, int nr, int nc) {
  const bool dev = mem == Mem::Device;
  const size_t rows = (size_t)h->N * E;
  const double* staged = src;
  if (!dev) {
    if (rows > h->stage_rows) return fail(ADMM_ERR_INVALID, "internal: staging buffer too small");
    int rc_up;
    if ((rc_up = upload_h2d(h, h->stage, src, sizeof(double) * rows * h->batch))) return rc_up;
    staged = h->stage;
  }
  admm::launch_to_tiled(h->stream, staged, dst, h->batch, h->N, E, h->n, h->pitch, nr, nc);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  return ADMM_OK;
}

int download_transposed(admm_handle* h, Mem mem, const double* src, double* dst, int rows) {
  const bool dev = mem == Mem::Device;
  if (rows == h->L && windowed(h)) {          // the window's rows only; the caller's other rows are left alone
    if (dev) return fail(ADMM_ERR_UNSUPPORTED, "internal: device-memory destination on a time-sharded handle");
    const size_t r0 = win_row0(h), Lw = win_rows(h);
    dim3 gridw(((int)Lw + admm::T_TILE - 1) / admm::T_TILE, (h->pitch + admm::T_TILE - 1) / admm::T_TILE), blockw(admm::T_TILE * 8);
    hipLaunchKernelGGL(admm::from_batch_minor_kernel, gridw, blockw, 0, h->stream, src + win_bias(h), h->stage, h->batch, (int)Lw, h->pitch);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy2DAsync(dst + r0, (size_t)h->L * sizeof(double), h->stage, Lw * sizeof(double), Lw * sizeof(double), h->batch,
                             hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return ADMM_OK;
  }
  dim3 grid((rows + admm::T_TILE - 1) / admm::T_TILE, (h->pitch + admm::T_TILE - 1) / admm::T_TILE), block(admm::T_TILE * 8);
  hipLaunchKernelGGL(admm::from_batch_minor_kernel, grid, block, 0, h->stream, src, dev ? dst : h->stage, h->batch, rows, h->pitch);
  HIP_TRY(hipGetLastError());
  if (dev) return ADMM_OK;                    // (the caller of a device-memory read-out orders it against its own stream)
  return download_d2h(h, dst, h->stage, sizeof(double) * (size_t)rows * h->batch);
}

bool finite_all(const double* a, size_t cnt) {          // (threaded from ~1 M entries: 2.7 GB of problem data at 4096 x 1000 stages)
  std::atomic<bool> ok{true};
  host_parallel(cnt, sizeof(double), [a, &ok](size_t b, size_t e) {
    // |x| < inf  <=>  finite; the exponent test on the bit pattern vectorises (isfinite in a loop with an early exit does not)
    uint64_t bad = 0;
    for (size_t i = b; i < e; ++i) {
      uint64_t u;
      std::memcpy(&u, a + i, sizeof u);
      bad |= ((u >> 52) & 0x7ff) == 0x7ff;
    }
    if (bad) ok.store(false, std::memory_order_relaxed);
  });
  return ok.load();
}

int validate_options(const admm_options* o) {
  if (!(o->rho > 0.0) || !std::isfinite(o->rho)) return fail(ADMM_ERR_INVALID, "rho must be positive and finite");
  if (!(o->alpha > 0.0 && o->alpha < 2.0)) return fail(ADMM_ERR_INVALID, "alpha must lie in (0, 2)");
  if (!(o->eps_abs >= 0.0) || !(o->eps_rel >= 0.0)) return fail(ADMM_ERR_INVALID, "eps_abs / eps_rel must be >= 0");
  if (o->max_iter < 1) return fail(ADMM_ERR_INVALID, "max_iter must be >= 1");
  if (o->check_interval < 1) return fail(ADMM_ERR_INVALID, "check_interval must be >= 1");
  if (o->segments < 0 || o->zrows < 0) return fail(ADMM_ERR_INVALID, "segments / zrows must be >= 0");
  if (o->adapt_interval < 0 || o->adapt_max < 0) return fail(ADMM_ERR_INVALID, "adapt_interval / adapt_max must be >= 0");
  if (o->precision_mode < 0 || o->precision_mode > 2) return fail(ADMM_ERR_INVALID, "precision_mode must be ADMM_PRECISION_FP64, _MIXED or _FP64_MFMA");
  if (o->reserved != 0) return fail(ADMM_ERR_INVALID, "options.reserved must be 0");
  if (o->adapt_interval > 0) {
    if (o->adapt_interval % o->check_interval != 0)
      return fail(ADMM_ERR_INVALID, "adapt_interval must be a multiple of check_interval");
    if (!(o->adapt_mu > 1.0) || !(o->adapt_tau > 1.0) || !std::isfinite(o->adapt_mu) || !std::isfinite(o->adapt_tau))
      return fail(ADMM_ERR_INVALID, "adapt_mu and adapt_tau must be finite and > 1");
  }
  return ADMM_OK;
}

// sizes, NULL pointers, modes: what can be checked without reading an array
int validate_dims(const admm_problem* p) {
  if (p->N < 1 || p->n < 1 || p->m < 1 || p->batch < 1) return fail(ADMM_ERR_INVALID, "N, n, m, batch must be positive");
  if (!p->A || !p->B || !p->Q || !p->R || !p->QN || !p->x0 || !p->lo || !p->hi)
    return fail(ADMM_ERR_INVALID, "A, B, Q, R, QN, x0, lo, hi must be non-NULL");
  const int nb = p->n + p->m;
  const size_t L = (size_t)p->N * nb;
  if (L * (size_t)p->batch > ((size_t)1 << 40)) return fail(ADMM_ERR_INVALID, "problem too large");
  if (L > (size_t)0x7fffffff) return fail(ADMM_ERR_INVALID, "L = N (n + m) exceeds 2^31 - 1");
  if (p->time_varying < 0 || p->time_varying > 2 || p->stage_bounds < 0 || p->stage_bounds > 2)
    return fail(ADMM_ERR_INVALID, "time_varying / stage_bounds must be 0, 1 or 2");
  if (p->stage_bounds == 2 && p->time_varying != 2)
    return fail(ADMM_ERR_INVALID, "per-instance bounds (stage_bounds = 2) need per-instance dynamics (time_varying = 2)");
  return ADMM_OK;
}

// d != NULL: p describes a problem of the *_device entry points (DeviceProblem::hp): the findings of the device-side checks
// stand in for the per-instance arrays, which are device memory; everything else is checked here, in the same order.
int validate_problem(const admm_problem* p, const DeviceScan* d) {
  int rc;
  if ((rc = validate_dims(p))) return rc;
  const int nb = p->n + p->m;
  const size_t L = (size_t)p->N * nb;
  if (p->time_varying == 2) {
    if (!p->Q || !p->R || !p->QN) return fail(ADMM_ERR_INVALID, "Q, R, QN must be non-NULL");
    const bool ab_bad = d ? d->ab_bad
                          : !finite_all(p->A, (size_t)p->n * p->n * p->N * p->batch) || !finite_all(p->B, (size_t)p->n * p->m * p->N * p->batch);
    if (ab_bad || !finite_all(p->Q, (size_t)p->n * p->n) || !finite_all(p->R, (size_t)p->m * p->m) || !finite_all(p->QN, (size_t)p->n * p->n))
      return fail(ADMM_ERR_INVALID, "non-finite entry in A, B, Q, R or QN");
  }
  const bool dev_box = d && p->stage_bounds == 2;
  const size_t nbnd = (size_t)nb * (p->stage_bounds ? p->N : 1) * (p->stage_bounds == 2 ? p->batch : 1);
  {
    std::atomic<size_t> first_bad{SIZE_MAX};         // smallest offending index (threads take disjoint ranges)
    const double *lo = p->lo, *hi = p->hi;
    if (dev_box)
      first_bad = d->bnd_bad;
    else
      host_parallel(nbnd, 2 * sizeof(double), [lo, hi, &first_bad](size_t b, size_t e) {
        for (size_t i = b; i < e; ++i)
          if (!(lo[i] <= hi[i]) || lo[i] == INFINITY || hi[i] == -INFINITY) {      // (!(<=) also catches NaN)
            size_t cur = first_bad.load();
            while (i < cur && !first_bad.compare_exchange_weak(cur, i)) {}
            return;
          }
      });
    const size_t i = first_bad.load();
    if (i != SIZE_MAX) {
      const double lo_i = dev_box ? d->bnd_lo : p->lo[i], hi_i = dev_box ? d->bnd_hi : p->hi[i];
      if (std::isnan(lo_i) || std::isnan(hi_i)) return fail(ADMM_ERR_INVALID, "NaN in bounds");
      if (lo_i > hi_i) return fail(ADMM_ERR_INVALID, "lo > hi at bound index " + std::to_string(i));
      return fail(ADMM_ERR_INVALID, "lo = +inf or hi = -inf");
    }
  }
  if (p->unorm) {
    const int cnt = p->stage_bounds ? p->N : 1;
    for (int k = 0; k < cnt; ++k) {
      const double ub = p->unorm[k];
      if (std::isnan(ub) || !(ub > 0.0)) return fail(ADMM_ERR_INVALID, "unorm entries must be positive (inf = off)");
      if (std::isfinite(ub) && dev_box) {
        if ((size_t)k == d->un_stage) return fail(ADMM_ERR_INVALID, "control rows must be unbounded (-inf, inf) where unorm is finite");
      } else if (std::isfinite(ub))
        for (int b = 0; b < (p->stage_bounds == 2 ? p->batch : 1); ++b)       // (per-instance box: every QP's)
          for (int j = 0; j < p->m; ++j) {
            const size_t o = ((size_t)b * cnt + k) * nb + j;
            if (std::isfinite(p->lo[o]) || std::isfinite(p->hi[o]))
              return fail(ADMM_ERR_INVALID, "control rows must be unbounded (-inf, inf) where unorm is finite");
          }
    }
  }
  if (d ? d->x0_bad : !finite_all(p->x0, (size_t)p->n * p->batch)) return fail(ADMM_ERR_INVALID, "non-finite entry in x0");
  if (p->q && (d ? d->q_bad : !finite_all(p->q, L * p->batch))) return fail(ADMM_ERR_INVALID, "non-finite entry in q");
  return ADMM_OK;
}


// ---- caller arrays in device memory (the *_device entry points, ABI v9) ----

// `ptr` must be device memory of `device` (not pageable or pinned host memory, not another GPU's), holding at least `bytes`
// where the runtime reports the allocation's extent.  `fn` / `name` name the entry point and the argument in the message.
int check_device_ptr(int device, const void* ptr, size_t bytes, const char* fn, const char* name, size_t elem, const char* unit) {
  hipPointerAttribute_t a{};
  const hipError_t e = hipPointerGetAttributes(&a, ptr);
  if (e != hipSuccess) (void)hipGetLastError();          // (pageable host memory: some ROCm versions fail the query itself)
  if (e != hipSuccess || a.type != hipMemoryTypeDevice || a.device != device)
    return fail(ADMM_ERR_INVALID, std::string(fn) + ": " + name + " is not device memory of the handle's GPU (device " + std::to_string(device) + ")");
  if (reinterpret_cast<uintptr_t>(ptr) % elem)
    return fail(ADMM_ERR_INVALID, std::string(fn) + ": " + name + " is not " + std::to_string(elem) + "-byte aligned");
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void*>(ptr)) == hipSuccess) {
    if (static_cast<const char*>(ptr) + bytes > static_cast<const char*>(base) + size)
      return fail(ADMM_ERR_INVALID, std::string(fn) + ": " + name + " ends before its " + std::to_string(bytes / elem) + " " + unit);
  } else {
    (void)hipGetLastError();
  }
  return ADMM_OK;
}

// check_finite_kernel over every array given, on s: slot i receives the smallest offending index of arrays[i] (admm_runtime.hpp)
int finite_scan_begin(hipStream_t s, unsigned long long* slots, const FiniteArg* arrays, size_t count) {
  if (count > (size_t)CHK_SLOTS) return fail(ADMM_ERR_INVALID, "internal: more arrays than result slots of the finite check");
  HIP_TRY(hipMemsetAsync(slots, 0xff, CHK_SLOTS * sizeof(unsigned long long), s));
  for (size_t i = 0; i < count; ++i) {
    const FiniteArg& a = arrays[i];
    const size_t blocks = std::min<size_t>((a.count + admm::CHECK_THREADS - 1) / admm::CHECK_THREADS, 8192);
    if (a.ptr && blocks) {
      hipLaunchKernelGGL(admm::check_finite_kernel, dim3((unsigned)blocks), dim3(admm::CHECK_THREADS), 0, s, a.ptr, a.count, slots + i);
      HIP_TRY(hipGetLastError());
    }
  }
  return ADMM_OK;
}

int finite_scan_end(hipStream_t s, const unsigned long long* slots, unsigned long long (&found)[CHK_SLOTS]) {
  HIP_TRY(hipMemcpyAsync(found, slots, sizeof found, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return ADMM_OK;
}

// The checks of a problem whose arrays are device memory of `device`, on stream s (ordered after the caller's writes): the pointers,
// then the small arrays copied to the host and the per-instance ones read once on the device (result slots of scratch: Slot below).  Fills d; returns with s synchronised.  The data checks themselves are validate_problem(&d.hp,
// &d.scan): the caller's.
int prepare_device_problem(int device, hipStream_t s, const admm_problem* p, const char* fn, unsigned long long* scratch,
                           DeviceProblem& d) {
  enum Slot { SLOT_A, SLOT_B, SLOT_BOX, SLOT_UN, SLOT_X0, SLOT_Q, SLOT_COUNT };      // (BOX, UN: check_bounds_kernel writes both)
  static_assert(SLOT_COUNT <= CHK_SLOTS && SLOT_UN == SLOT_BOX + 1, "result slots of the device-side checks");
  int rc;
  if ((rc = validate_dims(p))) return rc;
  const size_t n = p->n, m = p->m, N = p->N, B = p->batch, nb = n + m, L = N * nb;
  const size_t stages = p->time_varying ? N : 1, per = p->time_varying == 2 ? B : 1;
  const size_t nA = n * n * stages * per, nB = n * m * stages * per;
  const size_t nbnd = nb * (p->stage_bounds ? N : 1) * (p->stage_bounds == 2 ? B : 1), nun = p->stage_bounds ? N : 1;
  const struct { const double* ptr; size_t count; const char* name; } arrays[] = {
      {p->A, nA, "A"}, {p->B, nB, "B"}, {p->Q, n * n, "Q"}, {p->R, m * m, "R"}, {p->QN, n * n, "QN"}, {p->x0, n * B, "x0"},
      {p->lo, nbnd, "lo"}, {p->hi, nbnd, "hi"}, {p->q, L * B, "q"}, {p->unorm, nun, "unorm"}};
  for (const auto& a : arrays)
    if (a.ptr && (rc = check_device_ptr(device, a.ptr, a.count * sizeof(double), fn, a.name))) return rc;
  d.hp = *p;
  auto to_host = [&](const double* src, size_t count, std::vector<double>& v, const double** field) -> int {
    v.resize(count);
    HIP_TRY(hipMemcpyAsync(v.data(), src, sizeof(double) * count, hipMemcpyDeviceToHost, s));
    *field = v.data();
    return ADMM_OK;
  };
  if ((rc = to_host(p->Q, n * n, d.Q, &d.hp.Q)) || (rc = to_host(p->R, m * m, d.R, &d.hp.R)) || (rc = to_host(p->QN, n * n, d.QN, &d.hp.QN)))
    return rc;
  if (p->time_varying != 2 && ((rc = to_host(p->A, nA, d.A, &d.hp.A)) || (rc = to_host(p->B, nB, d.B, &d.hp.B)))) return rc;
  if (p->stage_bounds != 2 && ((rc = to_host(p->lo, nbnd, d.lo, &d.hp.lo)) || (rc = to_host(p->hi, nbnd, d.hi, &d.hp.hi)))) return rc;
  if (p->unorm && (rc = to_host(p->unorm, nun, d.un, &d.hp.unorm))) return rc;
  FiniteArg scans[SLOT_COUNT] = {};
  if (p->time_varying == 2) { scans[SLOT_A] = {p->A, nA, "A"}; scans[SLOT_B] = {p->B, nB, "B"}; }
  scans[SLOT_X0] = {p->x0, n * B, "x0"};
  scans[SLOT_Q] = {p->q, L * B, "q"};
  if ((rc = finite_scan_begin(s, scratch, scans, SLOT_COUNT))) return rc;
  if (p->stage_bounds == 2) {
    const size_t blocks = std::min<size_t>((nbnd + admm::CHECK_THREADS - 1) / admm::CHECK_THREADS, 8192);
    hipLaunchKernelGGL(admm::check_bounds_kernel, dim3((unsigned)blocks), dim3(admm::CHECK_THREADS), 0, s, p->lo, p->hi, nbnd, p->unorm,
                       (int)nb, (int)m, (int)N, scratch + SLOT_BOX);
    HIP_TRY(hipGetLastError());
  }
  unsigned long long found[CHK_SLOTS];
  if ((rc = finite_scan_end(s, scratch, found))) return rc;
  const unsigned long long none = CHK_NONE;
  d.scan = DeviceScan{};
  d.scan.ab_bad = found[SLOT_A] != none || found[SLOT_B] != none;
  if (found[SLOT_BOX] != none) {
    d.scan.bnd_bad = (size_t)found[SLOT_BOX];
    HIP_TRY(hipMemcpy(&d.scan.bnd_lo, p->lo + found[SLOT_BOX], sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&d.scan.bnd_hi, p->hi + found[SLOT_BOX], sizeof(double), hipMemcpyDeviceToHost));
  }
  if (found[SLOT_UN] != none) d.scan.un_stage = (size_t)found[SLOT_UN];
  d.scan.x0_bad = found[SLOT_X0] != none;
  d.scan.q_bad = found[SLOT_Q] != none;
  return ADMM_OK;
}

int check_scratch(admm_handle* h) {
  return h->chk_d ? ADMM_OK : dalloc(h, &h->chk_d, CHK_SLOTS);
}

// ---- CallerIO: the caller-array contract of the host and *_device forms of a handle call (admm_runtime.hpp) ----

int CallerIO::check_ptr(const void* ptr, size_t bytes, const char* name, size_t elem, const char* unit) const {
  return dev() && ptr ? check_device_ptr(h->device, ptr, bytes, fn, name, elem, unit) : ADMM_OK;
}

int CallerIO::begin() {
  if (!asked) return ADMM_OK;                    // (a host call; no stream given: the caller vouches for its data)
  if (!h->ext_ev) HIP_TRY(hipEventCreateWithFlags(&h->ext_ev, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(h->ext_ev, asked));
  HIP_TRY(hipStreamWaitEvent(h->stream, h->ext_ev, 0));
  ordered = asked;
  return ADMM_OK;
}

int CallerIO::check_finite(std::initializer_list<FiniteArg> arrays, int* bad) {
  *bad = -1;
  bool any = false;
  for (const FiniteArg& a : arrays) any = any || a.ptr;
  if (!any) return ADMM_OK;
  unsigned long long found[CHK_SLOTS];
  int rc;
  if (dev() && ((rc = check_scratch(h)) || (rc = finite_scan_begin(h->stream, h->chk_d, arrays.begin(), arrays.size())) ||
                (rc = finite_scan_end(h->stream, h->chk_d, found))))
    return rc;
  int i = 0;
  for (const FiniteArg& a : arrays) {
    if (a.ptr && (dev() ? found[i] != CHK_NONE : !finite_all(a.ptr, a.count))) { *bad = i; break; }
    ++i;
  }
  return ADMM_OK;
}

int CallerIO::copy_out(void* dst, const void* src, size_t bytes) {
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, dev() ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
  return ADMM_OK;
}

int CallerIO::finish() {
  if (!ordered) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    return ADMM_OK;
  }
  HIP_TRY(hipEventRecord(h->ext_ev, h->stream));
  HIP_TRY(hipStreamWaitEvent(ordered, h->ext_ev, 0));
  return ADMM_OK;
}


// MIXED precision: fp32 = the mixed MFMA kernels; otherwise (the fp64 refinement phase of
// admm_solve) the all-fp64 MFMA kernels on their own records.  Both forms share every other device array and the
// alternation schedule; what an alternating iteration left pending is dropped at the switch (the next iteration
// starts with a backward sweep).
void set_mixed_form(admm_handle* h, bool fp32) {
  if (h->opt.precision_mode != ADMM_PRECISION_MIXED) return;
  h->mfma_on = fp32;
  h->mfma_refine = !fp32;
  drop_side_data(h);
  h->alt_state = admm_handle::ALT_NONE;
}

// admm_last_warning(): the forward-elimination form of a factor failed its host check, so the handle runs (or falls back
// to) the plain fused path.  `when` names the call.
void warn_alt_gate(const admm::Factor& f, double rho, const char* when) {
  char buf[512];
  if (f.alt_check >= 0.0)
    std::snprintf(buf, sizeof buf, "%s: the forward-elimination form failed its host check at rho = %g (relative mismatch %.3g > %.1g): "
                  "the handle runs the plain fused path (xb + xfz kernels, no alternation: ~8 B per stacked element and iteration more)",
                  when, rho, f.alt_check, ALT_GATE);
  else
    std::snprintf(buf, sizeof buf, "%s: the forward-elimination form could not be built at rho = %g (a singular A_k or filter covariance): "
                  "the handle runs the plain fused path (xb + xfz kernels, no alternation)", when, rho);
  g_warn = buf;
}

// Conditioning guard of the parallel-in-time form (see admm_setup): largest entry of the dense scan matrices.
double scan_growth(const admm::Factor& f) {
  double g = 0.0;
  for (double v : f.scanW) g = std::max(g, std::fabs(v));
  return g;
}

void destroy_graph(admm_handle* h) {
  for (int v = 0; v < 16; ++v) {
    if (h->graph_exec[v]) { (void)hipGraphExecDestroy(h->graph_exec[v]); h->graph_exec[v] = nullptr; }
    if (h->graph[v]) { (void)hipGraphDestroy(h->graph[v]); h->graph[v] = nullptr; }
  }
}

// ---- memory of a handle (admm_runtime.hpp): one function allocates and records, release() frees what is recorded ----

static std::atomic<int64_t> g_owned_count{0}, g_owned_bytes{0};     // device allocations only (admm_debug_handle_memory)

int handle_alloc(admm_handle* h, void** p, size_t bytes, bool zeroed, bool pinned) {
  void* a = nullptr;
  const hipError_t e = pinned ? hipHostMalloc(&a, bytes, hipHostMallocDefault) : hipMalloc(&a, bytes);
  if (e != hipSuccess)
    return pinned ? fail(ADMM_ERR_HIP, std::string("hipHostMalloc failed: ") + hipGetErrorString(e))
                  : fail(ADMM_ERR_ALLOC, std::string("hipMalloc failed: ") + hipGetErrorString(e));
  h->owned.push_back({a, bytes, pinned});
  if (!pinned) { g_owned_count += 1; g_owned_bytes += (int64_t)bytes; }
  *p = a;
  if (zeroed) HIP_TRY(h->stream ? hipMemsetAsync(a, 0, bytes, h->stream) : hipMemset(a, 0, bytes));
  return ADMM_OK;
}

static void free_owned(const admm_handle::Owned& o) {
  if (o.pinned) { (void)hipHostFree(o.ptr); return; }
  (void)hipFree(o.ptr);
  g_owned_count -= 1;
  g_owned_bytes -= (int64_t)o.bytes;
}

void handle_free(admm_handle* h, void* p) {
  auto it = std::find_if(h->owned.begin(), h->owned.end(), [p](const admm_handle::Owned& o) { return o.ptr == p; });
  if (it == h->owned.end()) return;
  free_owned(*it);
  h->owned.erase(it);
}

void release(admm_handle* h) {
  if (!h) return;
  h->spec.clear();               // joins the background factorisations (they read the handle's problem copy)
  h->spec_stale.clear();
  (void)hipSetDevice(h->device);
  destroy_graph(h);
  for (const admm_handle::Owned& o : h->owned) free_owned(o);
  for (hipEvent_t ev : {h->pin_ev[0], h->pin_ev[1], h->ext_ev})
    if (ev) (void)hipEventDestroy(ev);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}


// device copies of everything in h->fac (records, scan matrices; the alternating set if enabled)
// dense scan matrix + each row's non-zero column range [begin, end) for xscan_gemv_kernel
int upload_scan_dense(const std::vector<double>& W, int M, int K, double* Wd, int* rows_d) {
  std::vector<int32_t> rr((size_t)2 * M);
  for (int r = 0; r < M; ++r) {
    int kb = K, ke = 0;
    const double* row = &W[(size_t)r * K];
    for (int k = 0; k < K; ++k)
      if (row[k] != 0.0) { if (k < kb) kb = k; ke = k + 1; }
    if (ke < kb) { kb = 0; ke = 0; }
    rr[2 * r] = kb; rr[2 * r + 1] = ke;
  }
  HIP_TRY(hipMemcpy(Wd, W.data(), sizeof(double) * W.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(rows_d, rr.data(), sizeof(int32_t) * rr.size(), hipMemcpyHostToDevice));
  return ADMM_OK;
}

int upload_factor(admm_handle* h, const char* when) {
  HIP_TRY(hipMemcpy(h->recB, h->fac.recB.data(), sizeof(double) * h->fac.recB.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->recF, h->fac.recF.data(), sizeof(double) * h->fac.recF.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->recS, h->fac.recS.data(), sizeof(double) * h->fac.recS.size(), hipMemcpyHostToDevice));
  if (!h->scan_gemv) HIP_TRY(hipMemcpy(h->scanWp, h->fac.scanWp.data(), sizeof(double) * h->fac.scanWp.size(), hipMemcpyHostToDevice));
  if (!h->scan_gemv) HIP_TRY(hipMemcpy(h->scan_range, h->fac.scanRange.data(), sizeof(int32_t) * h->fac.scanRange.size(), hipMemcpyHostToDevice));
  int rc;
  if (h->scan_gemv && (rc = upload_scan_dense(h->fac.scanW, h->fac.scanM, h->fac.scanK, h->scanWd, h->scan_rows))) return rc;
  drop_side_data(h);
  h->alt_state = admm_handle::ALT_NONE;
  if (!h->fac.alt_ok) {                                             // the forward-elimination form did not survive the refactor
    if (h->alt_allowed) warn_alt_gate(h->fac, h->fac.rho, when);
    h->alt = false; h->alt_allowed = false;
  }
  if (h->mfma_mode) {
    HIP_TRY(hipMemcpy(h->recMF, h->fac.recMF.data(), h->fac.recMF.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->recMB, h->fac.recMB.data(), h->fac.recMB.size(), hipMemcpyHostToDevice));
    if (h->recMF64) {
      HIP_TRY(hipMemcpy(h->recMF64, h->fac.recMF64.data(), h->fac.recMF64.size(), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(h->recMB64, h->fac.recMB64.data(), h->fac.recMB64.size(), hipMemcpyHostToDevice));
    }
  }
  if ((h->has_fuel || h->zkind == ZKind::Soft) && (rc = upload_kappa(h))) return rc;   // kappa = weight / rho follows every refactor
  if (h->alt_allowed) {
    // (the refactored records go into the allocation of admm_setup: its slack stays zero, and still covers them)
    const std::string who(when);
    if ((rc = check_record_alloc((who + ", recFE").c_str(), h->recFE_bytes, h->fac.recFE.size() / h->fac.RFE, sizeof(double) * h->fac.RFE))) return rc;
    if ((rc = check_record_alloc((who + ", recBE").c_str(), h->recBE_bytes, h->fac.recBE.size() / h->fac.RBE, sizeof(double) * h->fac.RBE))) return rc;
    HIP_TRY(hipMemcpy(h->recFE, h->fac.recFE.data(), sizeof(double) * h->fac.recFE.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->recBE, h->fac.recBE.data(), sizeof(double) * h->fac.recBE.size(), hipMemcpyHostToDevice));
    if (!h->scan_gemv) HIP_TRY(hipMemcpy(h->scanWpB, h->fac.scanWpB.data(), sizeof(double) * h->fac.scanWpB.size(), hipMemcpyHostToDevice));
    if (!h->scan_gemv) HIP_TRY(hipMemcpy(h->scan_rangeB, h->fac.scanRangeB.data(), sizeof(int32_t) * h->fac.scanRangeB.size(), hipMemcpyHostToDevice));
    if (h->scan_gemv && (rc = upload_scan_dense(h->fac.scanWB, h->fac.scanM, h->fac.scanK, h->scanWBd, h->scan_rowsB))) return rc;
  }
  return ADMM_OK;
}

// bounds expanded to one entry per stacked row (standalone z kernels), thrust-magnitude bound per stage
int upload_bounds(admm_handle* h, const admm_problem* p) {
  const size_t L = h->L;
  std::vector<double> lo(L), hi(L);
  for (size_t e = 0; e < L; ++e) {
    const size_t blk = e / h->nb, row = e % h->nb;
    lo[e] = p->lo[(p->stage_bounds ? blk * h->nb : 0) + row];
    hi[e] = p->hi[(p->stage_bounds ? blk * h->nb : 0) + row];
  }
  // (on the handle's stream -- it is non-blocking, a null-stream copy would not be ordered with what is queued on it)
  HIP_TRY(hipMemcpyAsync(h->lo, lo.data(), sizeof(double) * L, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(h->hi, hi.data(), sizeof(double) * L, hipMemcpyHostToDevice, h->stream));
  std::vector<double> ub(h->N, INFINITY);
  if (p->unorm)
    for (int k = 0; k < h->N; ++k) ub[k] = p->unorm[p->stage_bounds ? k : 0];
  HIP_TRY(hipMemcpyAsync(h->ub, ub.data(), sizeof(double) * h->N, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return upload_kappa(h);
}

// kappa_k = fuel weight / rho per stage (zeros without a fuel term), for the block-structured z kernels: the same quotient as
// in the records (admm::fill_fuel)
int upload_kappa(admm_handle* h) {
  std::vector<double> kap(h->N, 0.0);
  if (h->has_fuel)
    for (int k = 0; k < h->N; ++k) kap[k] = h->fuel[k] / h->fac.rho;
  HIP_TRY(hipMemcpyAsync(h->kap, kap.data(), sizeof(double) * h->N, hipMemcpyHostToDevice, h->stream));
  std::vector<double> skap;                   // soft box: weight / rho per stacked row, an IEEE division (inf / rho = inf, 0 / rho = 0)
  if (h->zkind == ZKind::Soft) {
    skap.resize(h->L);
    for (int e = 0; e < h->L; ++e) skap[e] = h->soft[e] / h->fac.rho;
    HIP_TRY(hipMemcpyAsync(h->skap_d, skap.data(), sizeof(double) * h->L, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->soft_d, h->soft.data(), sizeof(double) * h->L, hipMemcpyHostToDevice, h->stream));
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  return ADMM_OK;
}

// host copy of the shared problem data (the caller's pointers are never kept): admm_set_rho refactors from it
void keep_shared(admm_handle* h, const admm_problem* p) {
  const size_t nst = p->time_varying ? (size_t)p->N : 1, nbd = (size_t)h->nb * (p->stage_bounds ? p->N : 1);
  h->pA.assign(p->A, p->A + nst * p->n * p->n);
  h->pB.assign(p->B, p->B + nst * p->n * p->m);
  h->pQ.assign(p->Q, p->Q + (size_t)p->n * p->n);
  h->pR.assign(p->R, p->R + (size_t)p->m * p->m);
  h->pQN.assign(p->QN, p->QN + (size_t)p->n * p->n);
  h->plo.assign(p->lo, p->lo + nbd);
  h->phi.assign(p->hi, p->hi + nbd);
  h->pun.clear();
  if (p->unorm) h->pun.assign(p->unorm, p->unorm + (p->stage_bounds ? p->N : 1));
  h->time_varying = p->time_varying;
  h->stage_bounds = p->stage_bounds;
  h->cert_valid = false;           // the certificate's device copy of A, B, Q, R, QN is of the old problem
  h->infeas_valid = false;         // ... and the infeasibility probe's copy of the box and the thrust bounds
  // every STATE row unbounded at EVERY stage: its dual is identically zero, which lets the non-residual kernel forms
  // skip reading its v (XFREE, xfze_kernel)
  bool open = std::getenv("ADMM_NO_SKIPV") == nullptr;
  for (size_t k = 0; open && k < (p->stage_bounds ? (size_t)p->N : 1); ++k)
    for (int r = h->m; open && r < h->nb; ++r)
      open = p->lo[k * h->nb + r] == -INFINITY && p->hi[k * h->nb + r] == INFINITY;
  h->xfree = open;
}

// The weights of the minimum-fuel term sum_k f_k ||u_k||_2 (admm_setup_fuel) against a validated problem:
// per_stage = false: `fuel` has unorm's shape (1 entry with stage_bounds = 0, else N); true: N entries (a handle's own copy).
int validate_fuel(const admm_problem* p, const double* fuel, bool per_stage) {
  const int cnt = (per_stage || p->stage_bounds) ? p->N : 1;
  for (int k = 0; k < cnt; ++k)
    if (!std::isfinite(fuel[k]) || !(fuel[k] >= 0.0)) return fail(ADMM_ERR_INVALID, "fuel entries must be finite and >= 0");
  if (p->stage_bounds == 2) return ADMM_OK;         // (per-instance box: refused with per-instance dynamics by the caller)
  const int nb = p->n + p->m;
  for (int k = 0; k < p->N; ++k) {
    if (!(fuel[cnt == 1 ? 0 : k] > 0.0)) continue;
    const size_t o = p->stage_bounds ? (size_t)k * nb : 0;
    for (int j = 0; j < p->m; ++j)
      if (std::isfinite(p->lo[o + j]) || std::isfinite(p->hi[o + j]))
        return fail(ADMM_ERR_INVALID, "control rows must be unbounded (-inf, inf) where fuel is positive");
  }
  return ADMM_OK;
}

int validate_soft(const admm_problem* p, const double* soft, bool expanded, const double* fuel) {
  const int nb = p->n + p->m;
  const size_t cnt = (size_t)nb * ((expanded || p->stage_bounds) ? p->N : 1);
  for (size_t e = 0; e < cnt; ++e)
    if (!(soft[e] >= 0.0)) return fail(ADMM_ERR_INVALID, "soft entries must be >= 0 (+inf = a hard row) and not NaN");
  for (int k = 0; k < p->N; ++k) {
    const bool ball = p->unorm && std::isfinite(p->unorm[p->stage_bounds ? k : 0]);
    if (!ball && !(fuel && fuel[k] > 0.0)) continue;
    const size_t o = (expanded || p->stage_bounds) ? (size_t)k * nb : 0;
    for (int j = 0; j < p->m; ++j)
      if (soft[o + j] != INFINITY)
        return fail(ADMM_ERR_INVALID, "soft entries of the control rows must be +inf where unorm is finite or fuel is positive");
  }
  return ADMM_OK;
}

int halfspace_stages(const char* fn, const double* a, const double* b, int count, int N, int nh, std::vector<char>& any) {
  if (!finite_all(a, (size_t)count * N * nh) || !finite_all(b, (size_t)count * N))
    return fail(ADMM_ERR_INVALID, std::string(fn) + ": non-finite entry in a or b");
  any.assign(N, 0);
  for (size_t s = 0; s < (size_t)count * N; ++s) {
    const double* as = a + s * nh;
    double nn = 0.0;
    bool nz = false;
    for (int i = 0; i < nh; ++i) {
      nn = std::fma(as[i], as[i], nn);
      nz = nz || as[i] != 0.0;
    }
    if (!nz) continue;
    if (!admm::halfspace_norm_ok(nn))
      return fail(ADMM_ERR_INVALID, std::string(fn) + ": a'a of stage " + std::to_string(s % N) + " is not a normal number (scale the row)");
    any[s % N] = 1;
  }
  return ADMM_OK;
}

int halfspace_box_open(const char* fn, const admm_problem* p, const std::vector<char>& any, int nh, const char* what) {
  const int nb = p->n + p->m;
  for (int k = 0; k < p->N; ++k) {
    if (!any[k]) continue;
    const size_t o = (p->stage_bounds ? (size_t)k * nb : 0) + p->m;
    for (int i = 0; i < nh; ++i)
      if (p->lo[o + i] != -INFINITY || p->hi[o + i] != INFINITY)
        return fail(ADMM_ERR_INVALID, std::string(fn) + ": state rows 0 .. nh - 1 must be unbounded (-inf, inf) at a stage with " + what +
                                          " (stage " + std::to_string(k) + ")");
  }
  return ADMM_OK;
}

int cone_stages(const char* fn, const double* c, const double* apex, const double* gamma, int count, int N, int nh, std::vector<char>& any) {
  if (!finite_all(c, (size_t)count * N * nh) || !finite_all(apex, (size_t)count * N * nh) || !finite_all(gamma, (size_t)count * N))
    return fail(ADMM_ERR_INVALID, std::string(fn) + ": non-finite entry in c, apex or gamma");
  any.assign(N, 0);
  for (size_t s = 0; s < (size_t)count * N; ++s) {
    const double* cs = c + s * nh;
    double nn = 0.0;
    bool nz = false;
    for (int i = 0; i < nh; ++i) {
      nn = std::fma(cs[i], cs[i], nn);
      nz = nz || cs[i] != 0.0;
    }
    if (!nz) continue;
    if (!admm::halfspace_norm_ok(nn))
      return fail(ADMM_ERR_INVALID, std::string(fn) + ": c'c of stage " + std::to_string(s % N) + " is not a normal number (scale the axis)");
    if (!admm::cone_slope_ok(gamma[s]))
      return fail(ADMM_ERR_INVALID, std::string(fn) + ": gamma of stage " + std::to_string(s % N) +
                                        " must be a positive normal number with 1 + gamma^2 finite");
    any[s % N] = 1;
  }
  return ADMM_OK;
}

bool problem_has_soc(const admm_problem* p) {
  bool soc = false;
  if (p->unorm)
    for (int k = 0; k < (p->stage_bounds ? p->N : 1); ++k) soc = soc || std::isfinite(p->unorm[k]);
  return soc;
}



}  // namespace rt
}  // namespace admm

extern "C" void admm_debug_handle_memory(int64_t* count, int64_t* bytes) {
  if (count) *count = admm::rt::g_owned_count.load();
  if (bytes) *bytes = admm::rt::g_owned_bytes.load();
}
