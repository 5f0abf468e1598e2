// admm_consensus_kernels.hpp -- the z-update of a scenario-consensus handle: zdual_kernel / zdual_soc_kernel
// with the control rows of a stage projected ONCE per group of G adjacent QPs, on the group's mean:
//     state rows     z = clip(v),  y = v - z                                               (per QP, unchanged)
//     control rows   vbar_j = (sum_{b in g} v_{j,b}) / G,  zbar = prox(vbar),  z_{j,b} = zbar_j,  y_{j,b} = v_{j,b} - zbar_j
// prox = the box clip, or soc_factor(||vbar||, ub_k, kap_k) vbar on a stage with a thrust bound or a fuel weight: the pieces of
// admm_prox.hpp, composed as zdual_soc_kernel composes them, so G = 1 gives that kernel's bits (vbar = v / 1 = v).
//
// GEOMETRY.  One lane = one QP per slot (8-byte accesses; a wave's access is 64 adjacent columns, 512 B): a group may start at
// any column, odd ones included.  A workgroup owns WHOLE groups, so no sum crosses workgroups and the update stays in place:
//   route A, G <= T (T = consensus_tile(m): 512 columns for m <= 3, 256 above -- the LDS budget):  floor(T / G) adjacent
//       groups per workgroup.  v of the block's control rows goes to LDS (with w and the old z where residuals are formed),
//       is summed there and applied from there: every element is read from memory once -- 40 B per stacked element with
//       RESID / RELAX, 32 B without, as zdual_kernel.
//   route B, G > T:  one group per workgroup, walked in tiles of 512 columns, twice per block: once over the control rows for
//       the sum, once to apply (that second read of 3 m G doubles hits L2).  The five residual sums of a column cannot stay
//       in registers across the blocks of a chunk here; they continue through part[] (same fma chain, same bits).
// blockIdx.y = row chunk, a whole number of blocks (zrows % nb == 0), as zdual_soc_kernel.
//
// SUMMATION ORDER.  A radix-8 tree over the column index i RELATIVE to the group's first column:
//     S_0[i] = v[i];   S_{l+1}[i] = S_l[i] + S_l[i + 8^l] + ... + S_l[i + 7 * 8^l]   for i % 8^(l+1) == 0,
// added left to right, terms with i + k 8^l >= G left out; the group's sum is S_top[0].  It depends on G and on i only, not on
// the group's place in the batch, on the batch size or on the pitch.  Levels 0..2 (512 = 8^3 columns) run in LDS; route B
// carries the tile sums up the same tree one tile at a time (tree_carry).  No atomics: results are bitwise repeatable.
//
// PAD COLUMNS (batch .. pitch-1) belong to no group: they are neither read nor written.
// BARRIERS.  Every lane of the workgroup reaches every __syncthreads: no return before the end, every loop around a barrier has
// workgroup-uniform bounds, lanes without a column skip the work, not the barrier (as cert_pass_kernel documents).
#pragma once

#include "admm_consensus.hpp"
#include "admm_kernels.hpp"

namespace admm {

constexpr int CONS_TILE = 2 * Z_THREADS;       // columns of a tile: two slots per lane
constexpr int CONS_LEVELS = 10;                // route B: tree levels above a tile (8^10 tiles)
constexpr int CONS_MAXM = 8;

// columns a workgroup holds in LDS on route A: four arrays of m rows with residuals, 48 KiB at m = 3 and at m = 6, plus the 704 B of
// zbar and the upper levels -- 49 856 B per workgroup, under the 64 KiB a workgroup may ask for, and two workgroups fit a CU
__host__ __device__ constexpr int consensus_tile(int m) { return m <= 3 ? CONS_TILE : CONS_TILE / 2; }
constexpr size_t consensus_lds_bytes(int m, int G, bool resid) {
  const int T = consensus_tile(m);
  return sizeof(double) * ((size_t)CONS_MAXM * (1 + CONS_LEVELS) + (G > T ? (size_t)m * CONS_TILE : (size_t)m * T * (resid ? 4 : 2)));
}
static_assert(CONS_MAX_M <= CONS_MAXM, "zbar and the level sums hold CONS_MAXM rows");
static_assert(consensus_lds_bytes(3, 1, true) <= 65536 && consensus_lds_bytes(CONS_MAX_M, 1, true) <= 65536 &&
              consensus_lds_bytes(CONS_MAX_M, 1 << 20, true) <= 65536, "a workgroup's LDS request stays under 64 KiB for every m <= CONS_MAX_M");

// level d = 1, 8, 64 of the tree, in place on the m rows of sr (row stride `stride`); rel / lim: the element's index in its
// group (route A) or tile (route B) and that group's / tile's size.  Ends with a barrier per level.
__device__ __forceinline__ void cons_tree_levels(double* sr, int stride, int m, int top, const int (&e)[2], const int (&rel)[2],
                                                 const bool (&valid)[2], int lim) {
  for (int d = 1; d < top; d *= 8) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (valid[s] && rel[s] % (8 * d) == 0) {
        for (int j = 0; j < m; ++j) {
          double* p = sr + j * stride + e[s];
          double sum = p[0];
#pragma unroll
          for (int k = 1; k < 8; ++k)
            if (rel[s] + k * d < lim) sum += p[k * d];
          p[0] = sum;
        }
      }
    }
    __syncthreads();
  }
}

// zbar of a stage's control rows from the group's sums (m doubles at stride `stride`), in place
__device__ __forceinline__ void cons_prox(double* s, int stride, int m, double Gd, bool soc, double ub, double kap, cdouble_p lo,
                                          cdouble_p hi, int rb) {
  if (soc) {
    double ss = 0.0;
    for (int j = 0; j < m; ++j) {
      const double mu = s[j * stride] / Gd;
      ss = fma(mu, mu, ss);
    }
    const double c = soc_factor(sqrt(ss), ub, kap);
    for (int j = 0; j < m; ++j) s[j * stride] = (s[j * stride] / Gd) * c;
  } else {
    for (int j = 0; j < m; ++j) s[j * stride] = clip(s[j * stride] / Gd, lo[rb + j], hi[rb + j]);
  }
}

// A batch of up to U rows r0 .. of the lane's (up to) two columns in registers: every load of the batch is issued before the
// first is used (a row-at-a-time loop is one round trip to memory per row).  CONS_CU control rows and CONS_SU state rows per batch:
// a (6, 3) block is two batches, the second of which rides over the reduction of the first.
constexpr int CONS_CU = 3, CONS_SU = 6;

template <bool RESID, bool RELAX, int U>
__device__ __forceinline__ void cons_rows_load(const double* __restrict__ w, const double* z, const double* y, size_t P, int r0, int r1,
                                               const size_t (&col)[2], const bool (&valid)[2], double (&wv)[U][2], double (&yv)[U][2],
                                               double (&zv)[U][2]) {
#pragma unroll
  for (int i = 0; i < U; ++i)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      wv[i][s] = yv[i][s] = zv[i][s] = 0.0;
      if (r0 + i < r1 && valid[s]) {
        const size_t o = (size_t)(r0 + i) * P + col[s];
        wv[i][s] = w[o];
        yv[i][s] = y[o];
        if (RESID || RELAX) zv[i][s] = z[o];
      }
    }
}

// the per-QP z-update of zdual_kernel on a loaded batch of state rows
template <bool RESID, bool RELAX, int U>
__device__ __forceinline__ void cons_state_apply(double* __restrict__ z, double* __restrict__ y, cdouble_p lo, cdouble_p hi, double alpha,
                                                 size_t P, int r0, int r1, const size_t (&col)[2], const bool (&valid)[2],
                                                 const double (&wv)[U][2], const double (&yv)[U][2], const double (&zv)[U][2],
                                                 ResidSums (&acc)[2]) {
#pragma unroll
  for (int i = 0; i < U; ++i)
#pragma unroll
    for (int s = 0; s < 2; ++s)
      if (r0 + i < r1 && valid[s]) {
        const size_t o = (size_t)(r0 + i) * P + col[s];
        const double v = relaxed<RELAX>(alpha, wv[i][s], zv[i][s]) + yv[i][s];
        const double zn = clip(v, lo[r0 + i], hi[r0 + i]);
        const double yn = v - zn;
        z[o] = zn;
        y[o] = yn;
        if (RESID) acc[s].add(wv[i][s], zn, zv[i][s], yn);
      }
}

// state rows beyond the first batch
template <bool RESID, bool RELAX>
__device__ __forceinline__ void cons_state_rest(const double* __restrict__ w, double* __restrict__ z, double* __restrict__ y,
                                                cdouble_p lo, cdouble_p hi, double alpha, size_t P, int r0, int r1,
                                                const size_t (&col)[2], const bool (&valid)[2], ResidSums (&acc)[2]) {
  for (int r = r0; r < r1; r += CONS_SU) {
    double wv[CONS_SU][2], yv[CONS_SU][2], zv[CONS_SU][2];
    cons_rows_load<RESID, RELAX, CONS_SU>(w, z, y, P, r, r1, col, valid, wv, yv, zv);
    cons_state_apply<RESID, RELAX, CONS_SU>(z, y, lo, hi, alpha, P, r, r1, col, valid, wv, yv, zv, acc);
  }
}

template <bool RESID, bool RELAX>
__global__ __launch_bounds__(Z_THREADS) void zdual_consensus_kernel(
    const double* __restrict__ w, double* __restrict__ z, double* __restrict__ y,
    const double* __restrict__ lo_, const double* __restrict__ hi_, const double* __restrict__ ub_, const double* __restrict__ kap_,
    double* __restrict__ part, double alpha, int L, int zrows, int pitch, int nb, int m, int G, int batch) {
  extern __shared__ double cons_lds[];
  const int t = threadIdx.x;
  const int chunk = blockIdx.y;
  const int r_begin = chunk * zrows;
  const int r_end = (r_begin + zrows < L) ? r_begin + zrows : L;
  const size_t P = (size_t)pitch;
  cdouble_p lo = as_const(lo_);
  cdouble_p hi = as_const(hi_);
  cdouble_p ubv = as_const(ub_);
  cdouble_p kapv = as_const(kap_);
  const double Gd = (double)G;
  const int T = consensus_tile(m);
  double* const zb = cons_lds;                               // [CONS_MAXM]              route B: zbar
  double* const lv = cons_lds + CONS_MAXM;                   // [CONS_LEVELS][CONS_MAXM] route B: running sums of the upper levels
  double* const sr = lv + CONS_LEVELS * CONS_MAXM;           // [m][stride]              sums, then zbar at a group's first column
  const int e[2] = {t, t + Z_THREADS};

  if (G <= T) {
    // ---- route A: floor(T / G) whole groups, everything between the one read and the one write in LDS
    double* const sv = sr + (size_t)m * T;                   // [m][T] v
    double* const sw = sv + (size_t)m * T;                   // [m][T] w      (RESID)
    double* const so = sw + (size_t)m * T;                   // [m][T] old z  (RESID)
    const int gpw = T / G;
    const size_t c0 = (size_t)blockIdx.x * gpw * G;
    const int cnt = (size_t)gpw * G < (size_t)batch - c0 ? gpw * G : (int)((size_t)batch - c0);
    const bool valid[2] = {e[0] < cnt, e[1] < cnt};
    const int rel[2] = {e[0] % G, e[1] % G};
    const size_t col[2] = {c0 + e[0], c0 + e[1]};
    ResidSums acc[2];
    for (int rb = r_begin; rb < r_end; rb += nb) {
      const double ub = ubv[rb / nb], kap = kapv[rb / nb];
      const bool soc = ub < INFINITY || kap > 0.0;
      for (int j0 = 0; j0 < m; j0 += CONS_CU) {
        double wv[CONS_CU][2], yv[CONS_CU][2], zv[CONS_CU][2];
        cons_rows_load<RESID, RELAX, CONS_CU>(w, z, y, P, rb + j0, rb + m, col, valid, wv, yv, zv);
#pragma unroll
        for (int i = 0; i < CONS_CU; ++i)
#pragma unroll
          for (int s = 0; s < 2; ++s)
            if (j0 + i < m && valid[s]) {
              const int q = (j0 + i) * T + e[s];
              const double v = relaxed<RELAX>(alpha, wv[i][s], zv[i][s]) + yv[i][s];
              sv[q] = v;
              sr[q] = v;
              if (RESID) { sw[q] = wv[i][s]; so[q] = zv[i][s]; }
            }
      }
      // the first batch of state rows is loaded now and used after the reduction: its round trip to memory hides the barriers
      double pw[CONS_SU][2], py[CONS_SU][2], pz[CONS_SU][2];
      cons_rows_load<RESID, RELAX, CONS_SU>(w, z, y, P, rb + m, rb + nb, col, valid, pw, py, pz);
      __syncthreads();
      cons_tree_levels(sr, T, m, G, e, rel, valid, G);
#pragma unroll
      for (int s = 0; s < 2; ++s)
        if (valid[s] && rel[s] == 0) cons_prox(sr + e[s], T, m, Gd, soc, ub, kap, lo, hi, rb);
      __syncthreads();
      for (int j = 0; j < m; ++j)
#pragma unroll
        for (int s = 0; s < 2; ++s)
          if (valid[s]) {
            const size_t o = (size_t)(rb + j) * P + col[s];
            const double zn = sr[j * T + e[s] - rel[s]];
            const double yn = sv[j * T + e[s]] - zn;
            z[o] = zn;
            y[o] = yn;
            if (RESID) acc[s].add(sw[j * T + e[s]], zn, so[j * T + e[s]], yn);
          }
      cons_state_apply<RESID, RELAX, CONS_SU>(z, y, lo, hi, alpha, P, rb + m, rb + nb, col, valid, pw, py, pz, acc);
      cons_state_rest<RESID, RELAX>(w, z, y, lo, hi, alpha, P, rb + m + CONS_SU, rb + nb, col, valid, acc);
      __syncthreads();                  // the next block's v overwrites zbar, which other lanes of the group have just read
    }
    if (RESID) {
#pragma unroll
      for (int s = 0; s < 2; ++s)
        if (valid[s]) {
          double* p = part + (size_t)chunk * 5 * P + col[s];
          p[0 * P] = acc[s].r; p[1 * P] = acc[s].s; p[2 * P] = acc[s].w; p[3 * P] = acc[s].z; p[4 * P] = acc[s].y;
        }
    }
  } else {
    // ---- route B: one group, tiles of 512 columns; pass 1 sums the control rows, pass 2 applies
    const size_t c0 = (size_t)blockIdx.x * G;
    const int ntiles = (G + CONS_TILE - 1) / CONS_TILE;
    for (int rb = r_begin; rb < r_end; rb += nb) {
      const double ub = ubv[rb / nb], kap = kapv[rb / nb];
      const bool soc = ub < INFINITY || kap > 0.0;
      for (int tile = 0; tile < ntiles; ++tile) {
        const int cnt = G - tile * CONS_TILE < CONS_TILE ? G - tile * CONS_TILE : CONS_TILE;
        const bool valid[2] = {e[0] < cnt, e[1] < cnt};
        const size_t col[2] = {c0 + (size_t)tile * CONS_TILE + e[0], c0 + (size_t)tile * CONS_TILE + e[1]};
        for (int j0 = 0; j0 < m; j0 += CONS_CU) {
          double wv[CONS_CU][2], yv[CONS_CU][2], zv[CONS_CU][2];
          cons_rows_load<false, RELAX, CONS_CU>(w, z, y, P, rb + j0, rb + m, col, valid, wv, yv, zv);
#pragma unroll
          for (int i = 0; i < CONS_CU; ++i)
#pragma unroll
            for (int s = 0; s < 2; ++s)
              if (j0 + i < m && valid[s]) sr[(j0 + i) * CONS_TILE + e[s]] = relaxed<RELAX>(alpha, wv[i][s], zv[i][s]) + yv[i][s];
        }
        __syncthreads();
        cons_tree_levels(sr, CONS_TILE, m, CONS_TILE, e, e, valid, cnt);
        if (t < m) {
          // the tile's sum is node `tile` of level 3: carry it up the tree (a node is complete when its eighth child, or the
          // last node of the level below, has arrived)
          double x = sr[t * CONS_TILE];
          int tt = tile, nn = ntiles, l = 0;
          bool root = true;
          while (nn > 1) {
            const double run = (tt & 7) ? lv[l * CONS_MAXM + t] + x : x;
            if ((tt & 7) == 7 || tt == nn - 1) { x = run; tt >>= 3; nn = (nn + 7) >> 3; ++l; }
            else { lv[l * CONS_MAXM + t] = run; root = false; break; }
          }
          if (root) zb[t] = x;
        }
        __syncthreads();
      }
      if (t == 0) cons_prox(zb, 1, m, Gd, soc, ub, kap, lo, hi, rb);
      __syncthreads();
      for (int tile = 0; tile < ntiles; ++tile) {
        const int cnt = G - tile * CONS_TILE < CONS_TILE ? G - tile * CONS_TILE : CONS_TILE;
        const bool valid[2] = {e[0] < cnt, e[1] < cnt};
        const size_t col[2] = {c0 + (size_t)tile * CONS_TILE + e[0], c0 + (size_t)tile * CONS_TILE + e[1]};
        ResidSums acc[2];
        if (RESID && rb > r_begin) {
#pragma unroll
          for (int s = 0; s < 2; ++s)
            if (valid[s]) {
              const double* p = part + (size_t)chunk * 5 * P + col[s];
              acc[s].r = p[0 * P]; acc[s].s = p[1 * P]; acc[s].w = p[2 * P]; acc[s].z = p[3 * P]; acc[s].y = p[4 * P];
            }
        }
        double pw[CONS_SU][2], py[CONS_SU][2], pz[CONS_SU][2];
        cons_rows_load<RESID, RELAX, CONS_SU>(w, z, y, P, rb + m, rb + nb, col, valid, pw, py, pz);
        for (int j0 = 0; j0 < m; j0 += CONS_CU) {
          double wv[CONS_CU][2], yv[CONS_CU][2], zv[CONS_CU][2];
          cons_rows_load<RESID, RELAX, CONS_CU>(w, z, y, P, rb + j0, rb + m, col, valid, wv, yv, zv);
#pragma unroll
          for (int i = 0; i < CONS_CU; ++i)
#pragma unroll
            for (int s = 0; s < 2; ++s)
              if (j0 + i < m && valid[s]) {
                const size_t o = (size_t)(rb + j0 + i) * P + col[s];
                const double zn = zb[j0 + i];
                const double yn = (relaxed<RELAX>(alpha, wv[i][s], zv[i][s]) + yv[i][s]) - zn;
                z[o] = zn;
                y[o] = yn;
                if (RESID) acc[s].add(wv[i][s], zn, zv[i][s], yn);
              }
        }
        cons_state_apply<RESID, RELAX, CONS_SU>(z, y, lo, hi, alpha, P, rb + m, rb + nb, col, valid, pw, py, pz, acc);
        cons_state_rest<RESID, RELAX>(w, z, y, lo, hi, alpha, P, rb + m + CONS_SU, rb + nb, col, valid, acc);
        if (RESID) {
#pragma unroll
          for (int s = 0; s < 2; ++s)
            if (valid[s]) {
              double* p = part + (size_t)chunk * 5 * P + col[s];
              p[0 * P] = acc[s].r; p[1 * P] = acc[s].s; p[2 * P] = acc[s].w; p[3 * P] = acc[s].z; p[4 * P] = acc[s].y;
            }
        }
      }
      __syncthreads();                  // zbar is read above and rewritten by the next block's pass 1
    }
  }
}

}  // namespace admm
