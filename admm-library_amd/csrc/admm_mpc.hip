// admm_mpc.hip -- host side of the receding-horizon step (ADMM_HIP_HAS_MPC; kernels: admm_mpc_kernels.hpp):
// admm_mpc_advance / admm_mpc_advance_device.  Every check -- arguments first, without a HIP call; then the pointers; then the
// data -- comes before the first launch that changes the handle.
#include "admm_runtime.hpp"
#include "admm_mpc_kernels.hpp"

using namespace admm::rt;

namespace {

// The chunk count aims the shift's grid at 3/4 of the compute units (one 256-lane block each): at 4096 x 1000, (6, 3), that is 8
// chunks, the fastest of the counts 2 .. 128 measured on the MI355X (DESIGN.md §2.11 has the table; 4 blocks per CU, the first
// guess, was 10 % slower).  A chunk holds at least MPC_MIN_BLOCKS_PER_CHUNK blocks: a horizon of a few blocks is one chunk, with
// no scratch and no edge copies.
constexpr int MPC_GRID_CU_NUM = 3, MPC_GRID_CU_DEN = 4;
constexpr int MPC_MIN_BLOCKS_PER_CHUNK = 4;

int column_blocks(const admm_handle* h) { return (h->pitch / 2 + admm::MPC_THREADS - 1) / admm::MPC_THREADS; }

// ADMM_MPC_CHUNKS (tests and tools/mpc_time.py only) overrides the count; it is read per call and clamped to [1, N].
int chunk_count(const admm_handle* h, int arrays) {
  if (const char* e = std::getenv("ADMM_MPC_CHUNKS")) {
    const int v = std::atoi(e);
    if (v >= 1) return std::min(v, h->N);
  }
  const int per_chunk = column_blocks(h) * arrays;
  const int want = (h->num_cus * MPC_GRID_CU_NUM / MPC_GRID_CU_DEN + per_chunk - 1) / per_chunk;
  return std::max(1, std::min(want, h->N / MPC_MIN_BLOCKS_PER_CHUNK));
}

int bad(const char* fn, const std::string& what) { return fail(ADMM_ERR_INVALID, std::string(fn) + ": " + what); }

// what can be checked without a HIP call and without reading a per-QP array
int check_step(const char* fn, const admm_handle* h, const admm_mpc_step* s) {
  if (!h) return fail(ADMM_ERR_INVALID, "NULL handle");
  if (!s) return bad(fn, "step is NULL");
  if (h->ts_n) return fail(ADMM_ERR_UNSUPPORTED, std::string(fn) + ": not available on a time-sharded handle (a rank holds a stage window only)");
  if (int rc = refuse_on_kind(h, fn, &ZKindInfo::no_step)) return rc;
  if (h->pinst || h->time_varying == 2)
    return fail(ADMM_ERR_UNSUPPORTED, std::string(fn) + ": not available with per-instance dynamics (time_varying = 2): the per-QP operands and factors would have to shift too");
  if (h->n > admm::MPC_MAX_N || h->m > admm::MPC_MAX_M) return fail(ADMM_ERR_UNSUPPORTED, std::string(fn) + ": (n, m) beyond (12, 6)");
  if (s->tail != ADMM_MPC_TAIL_COPY && s->tail != ADMM_MPC_TAIL_ZERO) return bad(fn, "step.tail must be ADMM_MPC_TAIL_COPY or ADMM_MPC_TAIL_ZERO");
  if (s->reserved != 0) return bad(fn, "step.reserved must be 0");
  if (s->x_meas && (s->Ap || s->Bp || s->dx)) return bad(fn, "step.x_meas replaces the plant: Ap, Bp and dx must be NULL with it");
  if (s->q_tail && !h->has_q) return bad(fn, "step.q_tail on a handle that was set up without q");
  if (s->Ap && !finite_all(s->Ap, (size_t)h->n * h->n)) return bad(fn, "non-finite entry in Ap");
  if (s->Bp && !finite_all(s->Bp, (size_t)h->n * h->m)) return bad(fn, "non-finite entry in Bp");
  return ADMM_OK;
}

// the step itself on the handle's stream; every per-QP array of `s`, u and x are device memory (or NULL)
int advance(admm_handle* h, const admm_mpc_step* s, double* u, double* x) {
  int rc;
  admm::MpcArrays arr{};
  const int wzy_tail = s->tail == ADMM_MPC_TAIL_ZERO ? admm::MPC_ZERO : admm::MPC_KEEP;
  arr.count = h->has_q ? 4 : 3;
  const int chunks = chunk_count(h, arr.count);
  const size_t P = h->pitch, edge_count = (size_t)arr.count * (chunks - 1) * h->nb * P;
  if (edge_count > h->mpc_edge_count) {          // (first call, or a larger chunk count asked for since)
    dfree(h, &h->mpc_edge);                      // (hipFree waits for the kernels that still read it)
    h->mpc_edge_count = 0;
    if ((rc = dalloc(h, &h->mpc_edge, edge_count))) return rc;
    h->mpc_edge_count = edge_count;
  }
  if (!h->mpc_xn && (rc = dalloc(h, &h->mpc_xn, (size_t)h->n * P))) return rc;
  // the state as (w, z, y) in memory, as admm_get brings it there (w of the last x-update belongs to the old x0)
  if ((rc = ensure_w(h)) || (rc = ensure_zy(h))) return rc;
  double* const arrays[4] = {h->w, h->z, h->y, h->q};
  for (int a = 0; a < arr.count; ++a) { arr.a[a] = arrays[a]; arr.tail[a] = wzy_tail; }
  if (s->q_tail) arr.tail[3] = admm::MPC_FILL;
  const admm::MpcGeom g{h->N, h->n, h->m, h->nb, h->batch, h->pitch, chunks};
  admm::MpcPlant plant{};
  if (!s->x_meas) {
    std::memcpy(plant.A, s->Ap ? s->Ap : h->pA.data(), sizeof(double) * h->n * h->n);      // (stage 0 of time-varying dynamics)
    std::memcpy(plant.B, s->Bp ? s->Bp : h->pB.data(), sizeof(double) * h->n * h->m);
  }
  const admm::MpcStep step{h->x0, h->mpc_xn, s->du, s->dx, s->x_meas, u, x};
  const unsigned step_blocks = (unsigned)((h->pitch + admm::MPC_THREADS - 1) / admm::MPC_THREADS);
  hipLaunchKernelGGL(admm::mpc_edges_kernel, dim3(step_blocks, 1 + (unsigned)(arr.count * (chunks - 1))), dim3(admm::MPC_THREADS), 0,
                     h->stream, arr, g, step, plant, h->mpc_edge);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(admm::mpc_shift_kernel, dim3((unsigned)column_blocks(h), (unsigned)chunks, (unsigned)arr.count),
                     dim3(admm::MPC_THREADS), 0, h->stream, arr, g, (const double*)h->mpc_edge, s->q_tail);
  HIP_TRY(hipGetLastError());
  // the flags admm_update_instances and admm_set_state(w, z, y) leave
  h->w_stale = false;
  h->zy_valid = true;
  h->v_valid = false;
  drop_side_data(h);
  h->alt_state = admm_handle::ALT_NONE;
  return ADMM_OK;
}

// Both forms.  The host form stages its inputs into mpc_io; from there on it is the device form on the staged pointers.
int advance_common(admm_handle* h, const admm_mpc_step* s, double* u_applied, double* x_next, Mem mem, void* hip_stream) {
  const char* fn = mem == Mem::Device ? "admm_mpc_advance_device" : "admm_mpc_advance";
  int rc, bad_in;
  if ((rc = check_step(fn, h, s))) return rc;
  HIP_TRY(hipSetDevice(h->device));
  CallerIO io(h, fn, mem, hip_stream);
  const size_t B = h->batch, nu = B * h->m, nx = B * h->n, nq = B * h->nb;
  const FiniteArg in[4] = {{s->du, nu, "du"}, {s->dx, nx, "dx"}, {s->x_meas, nx, "x_meas"}, {s->q_tail, nq, "q_tail"}};
  for (const FiniteArg& a : in)
    if ((rc = io.check_ptr(a.ptr, a.count * sizeof(double), a.name))) return rc;
  if ((rc = io.check_ptr(u_applied, nu * sizeof(double), "u_applied")) || (rc = io.check_ptr(x_next, nx * sizeof(double), "x_next"))) return rc;
  // one pass over each input, one synchronisation for all of them (device form: none without an input)
  if ((rc = io.begin()) || (rc = io.check_finite({in[0], in[1], in[2], in[3]}, &bad_in))) return rc;
  if (bad_in >= 0) return bad(fn, std::string("non-finite entry in ") + in[bad_in].name);
  admm_mpc_step d = *s;                          // the step with its per-QP arrays in device memory
  double *u = u_applied, *x = x_next;
  if (!io.dev()) {
    // the small per-QP arrays cross through one device buffer: du | dx or x_meas | q_tail | u_applied | x_next
    if (!h->mpc_io && (rc = dalloc(h, &h->mpc_io, 2 * nu + 2 * nx + nq))) return rc;
    double *du_d = h->mpc_io, *dx_d = du_d + nu, *qt_d = dx_d + nx, *u_d = qt_d + nq, *x_d = u_d + nu;
    const double* xin = s->x_meas ? s->x_meas : s->dx;
    if ((s->du && (rc = upload_h2d(h, du_d, s->du, sizeof(double) * nu))) || (xin && (rc = upload_h2d(h, dx_d, xin, sizeof(double) * nx))) ||
        (s->q_tail && (rc = upload_h2d(h, qt_d, s->q_tail, sizeof(double) * nq))))
      return rc;
    d.du = s->du ? du_d : nullptr; d.dx = s->dx ? dx_d : nullptr; d.x_meas = s->x_meas ? dx_d : nullptr; d.q_tail = s->q_tail ? qt_d : nullptr;
    u = u_applied ? u_d : nullptr; x = x_next ? x_d : nullptr;
  }
  if ((rc = advance(h, &d, u, x))) return rc;
  if (!io.dev()) {
    if (u && (rc = download_d2h(h, u_applied, u, sizeof(double) * nu))) return rc;
    if (x && (rc = download_d2h(h, x_next, x, sizeof(double) * nx))) return rc;
  }
  return io.finish();
}

}  // namespace

extern "C" {

int admm_mpc_advance(admm_handle* h, const admm_mpc_step* s, double* u_applied, double* x_next) {
  return advance_common(h, s, u_applied, x_next, Mem::Host, nullptr);
}

// The device-memory form: du, dx, x_meas, q_tail, u_applied, x_next are device memory of the handle's GPU (Ap, Bp stay host arrays),
// under the rules of admm_update_instances_device for the inputs and of admm_get_device for the outputs.
int admm_mpc_advance_device(admm_handle* h, const admm_mpc_step* s, double* u_applied, double* x_next, void* hip_stream) {
  return advance_common(h, s, u_applied, x_next, Mem::Device, hip_stream);
}

}  // extern "C"
