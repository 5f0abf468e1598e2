// admm_mpc_kernels.hpp -- the receding-horizon step on the device (ADMM_HIP_HAS_MPC; host side: admm_mpc.hip).
//
// One step = apply the first control, propagate the plant, move every stacked array (w, z, y and q) one block of nb = n + m rows
// towards row 0.  The arrays are batch-minor [L][pitch] and stay where they are (captured graphs and launch structs hold their
// addresses), so the move is in place and overlapping.  It is cut into `chunks` runs of whole blocks along the row axis -- chunk c
// holds blocks [c N / chunks, (c + 1) N / chunks) -- and takes two launches:
//   mpc_edges_kernel   before anything is overwritten: the first block of every chunk but the first goes to a scratch (the chunk
//                      before it needs it after its owner has overwritten it); in the same launch one lane per QP reads block 0 of z
//                      and x0 and writes u, x+ and the new x0
//   mpc_shift_kernel   grid (column block, chunk, array): a lane owns two adjacent columns for its whole chunk and walks it forward,
//                      MPC_ROWS rows in flight; the chunk's last block comes from the scratch, the last chunk's from the tail rule
// Neither kernel uses LDS or a barrier.  Columns between batch and pitch are shifted like the rest (they stay finite); the tail and
// x0 get zeros there, as an upload would write.
#pragma once

#include <hip/hip_runtime.h>

namespace admm {

constexpr int MPC_THREADS = 256;
constexpr int MPC_ROWS = 8;            // rows in flight per lane of the shift (16 B each)
constexpr int MPC_MAX_ARRAYS = 4;      // w, z, y, q
constexpr int MPC_MAX_N = 12, MPC_MAX_M = 6;      // the widest compiled shape
// 16-byte accesses as a first-class vector value (a double2 STRUCT copied through a local array went through scratch memory)
typedef double mpc_d2 __attribute__((ext_vector_type(2)));
enum { MPC_KEEP = 0, MPC_ZERO = 1, MPC_FILL = 2 };    // what the last block of an array becomes (FILL: q_tail)

struct MpcArrays {
  double* a[MPC_MAX_ARRAYS];
  int tail[MPC_MAX_ARRAYS];
  int count;
};

struct MpcGeom {
  int N, n, m, nb, batch, pitch, chunks;
};

struct MpcPlant {                      // column-major, leading dimension n
  double A[MPC_MAX_N * MPC_MAX_N];
  double B[MPC_MAX_N * MPC_MAX_M];
};

struct MpcStep {
  double* x0;                          // [n][pitch], read and then overwritten
  double* xn;                          // [n][pitch] work rows: x+ until every row of it is known
  const double *du, *dx, *x_meas;      // QP-major (batch x m, batch x n, batch x n), NULL = absent
  double *u_out, *x_out;               // QP-major, NULL = not asked for
};

// (constant indices only: a by-value struct indexed by a run-time value is copied to scratch memory first)
__device__ inline double* mpc_array(const MpcArrays& arr, int a) { return a == 0 ? arr.a[0] : a == 1 ? arr.a[1] : a == 2 ? arr.a[2] : arr.a[3]; }
__device__ inline int mpc_tail(const MpcArrays& arr, int a) { return a == 0 ? arr.tail[0] : a == 1 ? arr.tail[1] : a == 2 ? arr.tail[2] : arr.tail[3]; }

__device__ __host__ inline int mpc_chunk_begin(int c, int N, int chunks) { return (int)((long long)c * N / chunks); }

// blockIdx.y = 0: the step, one lane per column.  blockIdx.y = 1 + a (chunks - 1) + (c - 1): block k0(c) of array a -> scratch.
static __global__ __launch_bounds__(MPC_THREADS) void mpc_edges_kernel(MpcArrays arr, MpcGeom g, MpcStep s, MpcPlant p, double* edge) {
  const size_t P = (size_t)g.pitch;
  if (blockIdx.y != 0) {
    const int col = (blockIdx.x * MPC_THREADS + threadIdx.x) * 2;
    if (col >= g.pitch) return;
    const int e = blockIdx.y - 1, a = e / (g.chunks - 1), c = 1 + e % (g.chunks - 1);
    const double* src = mpc_array(arr, a) + (size_t)mpc_chunk_begin(c, g.N, g.chunks) * g.nb * P + col;
    double* dst = edge + (size_t)e * g.nb * P + col;
    for (int i = 0; i < g.nb; ++i) *reinterpret_cast<mpc_d2*>(dst + i * P) = *reinterpret_cast<const mpc_d2*>(src + i * P);
    return;
  }
  const int b = blockIdx.x * MPC_THREADS + threadIdx.x;
  if (b >= g.pitch) return;
  if (b >= g.batch) {                  // padding columns: what an upload of x0 writes
    for (int i = 0; i < g.n; ++i) s.x0[i * P + b] = 0.0;
    return;
  }
  const double* zu = arr.a[1] + b;     // block 0 of z: rows 0 .. m-1 are u_0
  if (s.u_out)
    for (int j = 0; j < g.m; ++j) s.u_out[(size_t)b * g.m + j] = s.du ? zu[j * P] + s.du[(size_t)b * g.m + j] : zu[j * P];
  // This lane is the only reader of column b of x0, so the old x0 is safe until the second loop; x+ waits in xn meanwhile
  // (a register array indexed by a runtime n would live in scratch memory).
  for (int i = 0; i < g.n; ++i) {
    double acc;
    if (s.x_meas) {
      acc = s.x_meas[(size_t)b * g.n + i];
    } else {
      acc = s.dx ? s.dx[(size_t)b * g.n + i] : 0.0;
      for (int j = 0; j < g.n; ++j) acc = fma(p.A[i + j * g.n], s.x0[j * P + b], acc);
      for (int j = 0; j < g.m; ++j) {
        const double u = s.du ? zu[j * P] + s.du[(size_t)b * g.m + j] : zu[j * P];
        acc = fma(p.B[i + j * g.n], u, acc);
      }
    }
    s.xn[i * P + b] = acc;
  }
  for (int i = 0; i < g.n; ++i) {
    const double v = s.xn[i * P + b];
    s.x0[i * P + b] = v;
    if (s.x_out) s.x_out[(size_t)b * g.n + i] = v;
  }
}

// grid (column block, chunk, array).  Row r of the chunk takes row r + nb: loads run ahead of stores by nb rows and a lane touches
// its own two columns only, so walking forward never reads a row this launch has written -- except across a chunk boundary, which
// is what the scratch is for.  (No __restrict__: loads and stores go through one pointer on purpose.)
static __global__ __launch_bounds__(MPC_THREADS) void mpc_shift_kernel(MpcArrays arr, MpcGeom g, const double* edge,
                                                                       const double* q_tail) {
  const int col = (blockIdx.x * MPC_THREADS + threadIdx.x) * 2;
  if (col >= g.pitch) return;
  const size_t P = (size_t)g.pitch;
  const int c = blockIdx.y, a = blockIdx.z;
  double* p = mpc_array(arr, a) + col;
  const size_t nbP = (size_t)g.nb * P;
  size_t r = (size_t)mpc_chunk_begin(c, g.N, g.chunks) * g.nb;
  const size_t r_end = (size_t)(mpc_chunk_begin(c + 1, g.N, g.chunks) - 1) * g.nb;     // first row of the chunk's last block
  for (; r + MPC_ROWS <= r_end; r += MPC_ROWS) {
    mpc_d2 v[MPC_ROWS];
#pragma unroll
    for (int i = 0; i < MPC_ROWS; ++i) v[i] = *reinterpret_cast<const mpc_d2*>(p + (r + i) * P + nbP);
#pragma unroll
    for (int i = 0; i < MPC_ROWS; ++i) *reinterpret_cast<mpc_d2*>(p + (r + i) * P) = v[i];
  }
  for (; r < r_end; ++r) {
    const mpc_d2 v = *reinterpret_cast<const mpc_d2*>(p + r * P + nbP);
    *reinterpret_cast<mpc_d2*>(p + r * P) = v;
  }
  p += r_end * P;
  if (c + 1 < g.chunks) {
    const double* src = edge + ((size_t)a * (g.chunks - 1) + c) * nbP + col;
    for (int i = 0; i < g.nb; ++i) *reinterpret_cast<mpc_d2*>(p + i * P) = *reinterpret_cast<const mpc_d2*>(src + i * P);
    return;
  }
  const int tail = mpc_tail(arr, a);
  if (tail == MPC_ZERO) {
    for (int i = 0; i < g.nb; ++i) *reinterpret_cast<mpc_d2*>(p + i * P) = mpc_d2{0.0, 0.0};
  } else if (tail == MPC_FILL) {
    for (int i = 0; i < g.nb; ++i) {
      mpc_d2 v;
      v.x = col < g.batch ? q_tail[(size_t)col * g.nb + i] : 0.0;
      v.y = col + 1 < g.batch ? q_tail[(size_t)(col + 1) * g.nb + i] : 0.0;
      *reinterpret_cast<mpc_d2*>(p + i * P) = v;
    }
  }
}

}  // namespace admm
