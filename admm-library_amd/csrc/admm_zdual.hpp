// admm_zdual.hpp -- the standalone z-update and read-out kernels: zdual_kernel, zdual_soc_kernel,
// v_to_zy_kernel, v_to_zy_soc_kernel, and the walks that zdual_soft_kernel (admm_soft_kernels.hpp), zdual_halfspace_kernel
// (admm_halfspace_kernels.hpp) and zdual_cone_kernel (admm_cone_kernels.hpp) share with them.  Part of
// admm_kernels.hpp, which includes it inside namespace admm after the declarations it uses (Z_THREADS, cdouble_p, as_const).
//
// A kernel here is a WALK over the rows of a chunk, a SOURCE that says what a row is loaded from, and a PROX that says which
// (z, y) the row gets from its v and its row index.  The arithmetic is admm_prox.hpp's; the walk is written here once.
//
//   walks    z_walk_rows     one lane = two adjacent QPs (16-byte accesses), a workgroup = 512 columns x `zrows` rows, blockIdx.y
//                            = row chunk; ADMM_Z_UNROLL rows in flight per lane, then the tail of the chunk
//            z_walk_blocks   the same columns and chunks, a chunk being a whole number of blocks (zrows % nb == 0): the control
//                            rows of a stage with a thrust bound or a fuel weight need their joint norm, so such a block is
//                            visited twice -- its m control rows for ||v_u|| (the re-read hits L1/L2), then all rows to apply
//   sources  StateSource     (w, y, and z where RESID || RELAX), v+ = relaxed(w, z) + y; with RESID the five residual sums
//                            (zdual_kernel itself reads the same but keeps a walk of its own: see there)
//            VSource         v itself (read-out and mode switches of the v-form, §4.4); no sums
//   proxes   BoxProx         clip to [lo[r], hi[r]]; SoftBoxProx (admm_soft_kernels.hpp) is the other one
//   planes   NoPlane         z_walk_blocks only: a constraint that couples state rows of a stage; HalfspacePlane
//                            (admm_halfspace_kernels.hpp) and ConePlane (admm_cone_kernels.hpp) are the ones there are
//
// The row index is wave-uniform, so the bounds of a row are scalar loads through the constant address space and the per-QP sums
// need no cross-lane step at all: each lane owns its QPs' accumulators.  Pad columns (batch .. pitch - 1) are computed like any
// other: their state is zero and stays finite.
// (No include guard of its own and no includes: it is not a header to use alone.)

#ifndef ADMM_Z_UNROLL
#define ADMM_Z_UNROLL 4                // rows in flight per lane (a row-at-a-time loop ran at 3.5 TB/s: 250 us at configs[2])
#endif

// One row of two adjacent QPs, 16-byte pairs: (z, y) from v by the box, or -- the control rows of a thrust stage -- z = c v
// without the clip (their box is (-inf, inf): admm_prox.hpp).
struct ZY2 { double2 z, y; };
__device__ __forceinline__ ZY2 zy2_box(double2 v, double lo, double hi) {
  const double2 z = make_double2(clip(v.x, lo, hi), clip(v.y, lo, hi));
  return ZY2{z, make_double2(v.x - z.x, v.y - z.y)};
}
__device__ __forceinline__ ZY2 zy2_scaled(double2 v, double2 c) {
  const double2 z = make_double2(v.x * c.x, v.y * c.y);
  return ZY2{z, make_double2(v.x - z.x, v.y - z.y)};
}
__device__ __forceinline__ double2 soc_scale2(double2 ss, double ub, double kap) {
  return make_double2(soc_factor(sqrt(ss.x), ub, kap), soc_factor(sqrt(ss.y), ub, kap));
}
__device__ __forceinline__ double2 load2(const double* p) { return *reinterpret_cast<const double2*>(p); }

// ---- sources: Row load(o) gives the row at element offset o; v(row) is what the prox is applied to --------------------------
// The state source keeps the loaded (w, z, y) and forms v+ where the row is applied, as the kernels did before the walks were
// shared (forming it in the load step frees y early; it measured no faster: DESIGN.md §4.3).
template <bool RESID, bool RELAX>
struct StateSource {
  const double* w; const double* z; const double* y;
  double alpha;
  struct Row {
    static constexpr bool resid = RESID;
    double2 w, zo, y;                  // (zo is not loaded where nothing reads it)
  };
  __device__ __forceinline__ Row load(size_t o) const {
    Row r{load2(w + o), make_double2(0.0, 0.0), load2(y + o)};
    if (RESID || RELAX) r.zo = load2(z + o);
    return r;
  }
  __device__ __forceinline__ double2 v(const Row& r) const {
    return make_double2(relaxed<RELAX>(alpha, r.w.x, r.zo.x) + r.y.x, relaxed<RELAX>(alpha, r.w.y, r.zo.y) + r.y.y);
  }
};
struct VSource {
  const double* p;
  struct Row {
    static constexpr bool resid = false;
    double2 v;
  };
  __device__ __forceinline__ Row load(size_t o) const { return Row{load2(p + o)}; }
  __device__ __forceinline__ double2 v(const Row& r) const { return r.v; }
};

// ---- proxes: ZY2 operator()(v, r) of row r ---------------------------------------------------------------------------------------
struct BoxProx {
  cdouble_p lo, hi;
  __device__ __forceinline__ ZY2 operator()(double2 v, int r) const { return zy2_box(v, lo[r], hi[r]); }
};

// ---- the walks ---------------------------------------------------------------------------------------------------------------
// The columns and the row chunk of this lane; acc and its store are the walks' own
struct ZChunk {
  int col, r_begin, r_end;
  size_t P;
  __device__ __forceinline__ ZChunk(int L, int zrows, int pitch)
      : col((blockIdx.x * Z_THREADS + threadIdx.x) * 2), r_begin(blockIdx.y * zrows),
        r_end((r_begin + zrows < L) ? r_begin + zrows : L), P((size_t)pitch) {}
};

// One row, in place: store (z, y) = p; RESID: the sums of either QP, (w - z+)^2, (z+ - z)^2, w^2, z+^2, y+^2
template <class Row>
__device__ __forceinline__ void z_row_store(const Row& row, const ZY2& p, double* z, double* y, ResidSums (&acc)[2]) {
  *reinterpret_cast<double2*>(z) = p.z;
  *reinterpret_cast<double2*>(y) = p.y;
  if constexpr (Row::resid) {
    acc[0].add(row.w.x, p.z.x, row.zo.x, p.y.x);
    acc[1].add(row.w.y, p.z.y, row.zo.y, p.y.y);
  }
}

// the sums of a chunk -> part[chunk][5][pitch]
__device__ __forceinline__ void store_sums2(double* part, size_t P, const ResidSums (&acc)[2]) {
  *reinterpret_cast<double2*>(part + 0 * P) = make_double2(acc[0].r, acc[1].r);
  *reinterpret_cast<double2*>(part + 1 * P) = make_double2(acc[0].s, acc[1].s);
  *reinterpret_cast<double2*>(part + 2 * P) = make_double2(acc[0].w, acc[1].w);
  *reinterpret_cast<double2*>(part + 3 * P) = make_double2(acc[0].z, acc[1].z);
  *reinterpret_cast<double2*>(part + 4 * P) = make_double2(acc[0].y, acc[1].y);
}

template <class Source, class Prox>
__device__ __forceinline__ void z_walk_rows(const Source& src, const Prox& prox, double* z, double* y, double* part, int L, int zrows,
                                            int pitch) {
  const ZChunk c(L, zrows, pitch);
  if (c.col >= pitch) return;
  ResidSums acc[2];
  constexpr int U = ADMM_Z_UNROLL;
  int r = c.r_begin;
  for (; r + U <= c.r_end; r += U) {
    typename Source::Row row[U];
#pragma unroll
    for (int i = 0; i < U; ++i) row[i] = src.load((size_t)(r + i) * c.P + c.col);
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const size_t o = (size_t)(r + i) * c.P + c.col;
      z_row_store(row[i], prox(src.v(row[i]), r + i), z + o, y + o, acc);
    }
  }
  for (; r < c.r_end; ++r) {
    const size_t o = (size_t)r * c.P + c.col;
    const typename Source::Row row = src.load(o);
    z_row_store(row, prox(src.v(row), r), z + o, y + o, acc);
  }
  if (Source::Row::resid) store_sums2(part + (size_t)blockIdx.y * 5 * c.P + c.col, c.P, acc);
}

// A constraint on the state rows of a stage, carried by z_walk_blocks beside the thrust ball of its control rows.  NoPlane: none
// (the walk of zdual_soc_kernel, v_to_zy_soc_kernel, zdual_soft_kernel as it was); the others are HalfspacePlane
// (admm_halfspace_kernels.hpp) and ConePlane (admm_cone_kernels.hpp).  A plane says, per block,
//     Step step(src, k, rb, c)      what it needs from the block's rows before they are applied (a second read, as the norm's)
//     bool covers(step, r)          wave-uniform: row r of the block may be the plane's
//     ZY2 row(step, v, r, box, P)   (z, y) of such a row; box = the row's own prox, for the QPs whose stage has no plane
// and `soc` whether the walk reads ub / kap at all.
struct NoPlane {
  static constexpr bool enabled = false, soc = true;
};

template <class Source, class Prox, class Plane = NoPlane>
__device__ __forceinline__ void z_walk_blocks(const Source& src, const Prox& prox, double* z, double* y, const double* ub_,
                                              const double* kap_, double* part, int L, int zrows, int pitch, int nb, int m,
                                              const Plane& plane = Plane{}) {
  const ZChunk c(L, zrows, pitch);
  if (c.col >= pitch) return;
  cdouble_p ubv = as_const(ub_);
  cdouble_p kapv = as_const(kap_);
  ResidSums acc[2];
  for (int rb = c.r_begin; rb < c.r_end; rb += nb) {
    bool soc = false;
    double2 cs = {1.0, 1.0};
    if constexpr (Plane::soc) {
      const double ub = ubv[rb / nb], kap = kapv[rb / nb];
      soc = ub < INFINITY || kap > 0.0;               // a finite thrust bound or a fuel weight (else the control rows use their prox)
      if (soc) {
        double2 ss = {0.0, 0.0};
        for (int j = 0; j < m; ++j) {
          const double2 vn = src.v(src.load((size_t)(rb + j) * c.P + c.col));
          ss.x = fma(vn.x, vn.x, ss.x);
          ss.y = fma(vn.y, vn.y, ss.y);
        }
        cs = soc_scale2(ss, ub, kap);
      }
    }
    if constexpr (Plane::enabled) {
      // (ADMM_Z_UNROLL rows of the block in flight, as z_walk_rows: a workgroup per CU is one wave per SIMD, and a row at a time
      //  leaves it waiting on every load)
      const auto step = plane.step(src, rb / nb, rb, c);
      auto apply = [&](const typename Source::Row& row, int r) {
        const int row_i = rb + r;
        const size_t o = (size_t)row_i * c.P + c.col;
        const double2 v = src.v(row);
        z_row_store(row, soc && r < m ? zy2_scaled(v, cs) : plane.covers(step, r) ? plane.row(step, v, r, prox(v, row_i), c.P) : prox(v, row_i),
                    z + o, y + o, acc);
      };
      constexpr int U = ADMM_Z_UNROLL;
      int r = 0;
      for (; r + U <= nb; r += U) {
        typename Source::Row row[U];
#pragma unroll
        for (int i = 0; i < U; ++i) row[i] = src.load((size_t)(rb + r + i) * c.P + c.col);
#pragma unroll
        for (int i = 0; i < U; ++i) apply(row[i], r + i);
      }
      for (; r < nb; ++r) apply(src.load((size_t)(rb + r) * c.P + c.col), r);
    } else {
      for (int r = 0; r < nb; ++r) {
        const int row_i = rb + r;
        const size_t o = (size_t)row_i * c.P + c.col;
        const typename Source::Row row = src.load(o);
        const double2 v = src.v(row);
        z_row_store(row, soc && r < m ? zy2_scaled(v, cs) : prox(v, row_i), z + o, y + o, acc);
      }
    }
  }
  if (Source::Row::resid) store_sums2(part + (size_t)blockIdx.y * 5 * c.P + c.col, c.P, acc);
}

// ---- the kernels ---------------------------------------------------------------------------------------------------------------
// Fused z-update + dual ascent + residual partial sums -- the HBM-bound kernel the project is graded on.
//     wh = alpha w + (1 - alpha) z        (RELAX only)
//     v  = wh + y;  z+ = min(max(v, lo), hi);  y+ = v - z+       (in place)
//     RESID: per-QP partial sums over the chunk's rows -> part[chunk][5][pitch]
// Algorithmic HBM bytes per stacked element: RESID/RELAX: 3 reads + 2 writes = 40 B; plain: 2 reads + 2 writes = 32 B.
// zdual_kernel keeps a row walk of its own, the text it had before the walks were shared: built on z_walk_rows it gives the same
// bits and needs no more registers, but zdual_kernel<true, false> measured 2 % slower (261 - 267 us against 256 - 261 us, three
// alternated runs each), with v+ formed in the load step or at the apply step alike.
__device__ __forceinline__ void zy2_store(const ZY2& p, double* z, double* y, size_t o = 0) {
  *reinterpret_cast<double2*>(z + o) = p.z;
  *reinterpret_cast<double2*>(y + o) = p.y;
}
// v+ = w^ + y of one row of two adjacent QPs, from the loaded (z, y)
template <bool RELAX>
__device__ __forceinline__ double2 v_plus2(double alpha, double2 w, double2 z, double2 y) {
  return make_double2(relaxed<RELAX>(alpha, w.x, z.x) + y.x, relaxed<RELAX>(alpha, w.y, z.y) + y.y);
}
// One row of the unfused z-update for two adjacent QPs, in place: (z, y) <- z-update of (w, z, y); acc: the sums of either QP
template <bool RESID, bool RELAX>
__device__ __forceinline__ void zdual_row(double2 wv, double2 zv, double2 yv, double lo, double hi, double alpha,
                                          double* z, double* y, ResidSums (&acc)[2]) {
  const double2 v = v_plus2<RELAX>(alpha, wv, zv, yv);
  const ZY2 p = zy2_box(v, lo, hi);
  zy2_store(p, z, y);
  if (RESID) {
    acc[0].add(wv.x, p.z.x, zv.x, p.y.x);
    acc[1].add(wv.y, p.z.y, zv.y, p.y.y);
  }
}
template <bool RESID, bool RELAX>
__global__ __launch_bounds__(Z_THREADS) void zdual_kernel(
    const double* __restrict__ w, double* __restrict__ z, double* __restrict__ y,
    const double* __restrict__ lo_, const double* __restrict__ hi_,
    double* __restrict__ part, double alpha, int L, int zrows, int pitch) {
  const int col = (blockIdx.x * Z_THREADS + threadIdx.x) * 2;
  if (col >= pitch) return;
  const int chunk = blockIdx.y;
  const int r_begin = chunk * zrows;
  const int r_end = (r_begin + zrows < L) ? r_begin + zrows : L;
  const size_t P = (size_t)pitch;
  cdouble_p lo = as_const(lo_);
  cdouble_p hi = as_const(hi_);
  ResidSums acc[2];
  constexpr int U = ADMM_Z_UNROLL;
  int r = r_begin;
  for (; r + U <= r_end; r += U) {
    double2 wv[U], yv[U], zv[U];
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const size_t o = (size_t)(r + i) * P + col;
      wv[i] = *reinterpret_cast<const double2*>(w + o);
      yv[i] = *reinterpret_cast<const double2*>(y + o);
      zv[i] = make_double2(0.0, 0.0);
      if (RESID || RELAX) zv[i] = *reinterpret_cast<const double2*>(z + o);
    }
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const size_t o = (size_t)(r + i) * P + col;
      zdual_row<RESID, RELAX>(wv[i], zv[i], yv[i], lo[r + i], hi[r + i], alpha, z + o, y + o, acc);
    }
  }
  for (; r < r_end; ++r) {
    const size_t o = (size_t)r * P + col;
    const double2 wv = *reinterpret_cast<const double2*>(w + o);
    const double2 yv = *reinterpret_cast<const double2*>(y + o);
    double2 zv = {0, 0};
    if (RESID || RELAX) zv = *reinterpret_cast<const double2*>(z + o);
    zdual_row<RESID, RELAX>(wv, zv, yv, lo[r], hi[r], alpha, z + o, y + o, acc);
  }
  if (RESID) store_sums2(part + (size_t)chunk * 5 * P + col, P, acc);
}

// v -> (z, y): z = clip(v), y = v - z.  Read-out / mode switches only.
static __global__ __launch_bounds__(Z_THREADS) void v_to_zy_kernel(
    const double* __restrict__ v, double* __restrict__ z, double* __restrict__ y,
    const double* __restrict__ lo_, const double* __restrict__ hi_, int L, int zrows, int pitch) {
  z_walk_rows(VSource{v}, BoxProx{as_const(lo_), as_const(hi_)}, z, y, nullptr, L, zrows, pitch);
}

// Their forms for problems with a thrust-magnitude bound.  Unfused path and read-out only; the fused xfz / xb
// kernels do the same work on register-resident blocks.
template <bool RESID, bool RELAX>
__global__ __launch_bounds__(Z_THREADS) void zdual_soc_kernel(
    const double* __restrict__ w, double* __restrict__ z, double* __restrict__ y,
    const double* __restrict__ lo_, const double* __restrict__ hi_, const double* __restrict__ ub_, const double* __restrict__ kap_,
    double* __restrict__ part, double alpha, int L, int zrows, int pitch, int nb, int m) {
  z_walk_blocks(StateSource<RESID, RELAX>{w, z, y, alpha}, BoxProx{as_const(lo_), as_const(hi_)}, z, y, ub_, kap_, part, L, zrows,
                pitch, nb, m);
}

static __global__ __launch_bounds__(Z_THREADS) void v_to_zy_soc_kernel(
    const double* __restrict__ v, double* __restrict__ z, double* __restrict__ y,
    const double* __restrict__ lo_, const double* __restrict__ hi_, const double* __restrict__ ub_, const double* __restrict__ kap_,
    int L, int zrows, int pitch, int nb, int m) {
  z_walk_blocks(VSource{v}, BoxProx{as_const(lo_), as_const(hi_)}, z, y, ub_, kap_, nullptr, L, zrows, pitch, nb, m);
}
