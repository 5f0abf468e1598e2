/* admm_hip.h -- C ABI of libadmm_hip.so: batched ADMM for box-constrained
 * optimal-control QPs on MI355X (gfx950).
 *
 * Reference interface replaced: NONE EXISTS.  The reference snapshot is
 * /root/reference/README.md:1-2 ("Implementation of Alternating Direction
 * Method of Multipliers for astrodynamics problems") plus a LICENSE; it defines
 * no MATLAB entry point, MEX gateway or FFI for this path.
 * Every entry point below is therefore this repository's own specification of
 * the "problem-setup / solver entry-point surface" BASELINE.json's north_star
 * asks for; INTEGRATION.md shows the MEX and ctypes bindings over it.
 *
 * Conventions
 *   - Plain C, no C++ or torch types cross this boundary.
 *   - All real arrays are fp64.  Matrices are column-major (MATLAB-native).
 *   - Per-QP vectors are "L x batch column-major": QP b occupies
 *     [b*L, (b+1)*L).  The stacked variable of one QP is
 *       w = (u_0, x_1, u_1, x_2, ..., u_{N-1}, x_N),  L = N*(n+m),
 *     block k = (u_k, x_{k+1}).
 *   - Every function returns an admm_status (0 = ok); admm_last_error() gives
 *     a thread-local message for the last non-zero return.  No exceptions, no
 *     exit().
 *   - The library never keeps caller pointers after a call returns.
 *   - A handle is bound to one GPU and is not thread-safe; distinct handles are.
 */
#ifndef ADMM_HIP_H
#define ADMM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADMM_HIP_ABI_VERSION 9

typedef enum admm_status {
  ADMM_OK = 0,
  ADMM_ERR_INVALID = 1,      /* bad argument / problem data (NaN, lo > hi, sizes) */
  ADMM_ERR_UNSUPPORTED = 2,  /* (n, m) outside the compiled kernel set, etc. */
  ADMM_ERR_NO_DEVICE = 3,    /* no HIP device: the product path has no CPU fallback */
  ADMM_ERR_HIP = 4,          /* a HIP runtime call failed */
  ADMM_ERR_NUMERIC = 5,      /* factorisation failed (S_k not SPD) */
  ADMM_ERR_ALLOC = 6
} admm_status;

/* minimise  1/2 sum_k [u_k' R u_k + x_{k+1}' Q_{k+1} x_{k+1}] + q' w
 * s.t.      x_{k+1} = A_k x_k + B_k u_k,  x_0 given,   lo <= w <= hi   [and/or ||u_k||_2 <= unorm_k]
 * Dynamics, weights and the box are shared by the whole batch; x0 and q are
 * per instance.  (time_varying = 2 / stage_bounds = 2: dynamics / box per instance as well; weights stay shared.) */
typedef struct admm_problem {
  int32_t N;              /* horizon (stages) */
  int32_t n;              /* state dimension */
  int32_t m;              /* control dimension */
  int32_t batch;          /* number of independent QPs */
  int32_t time_varying;   /* 0: A is n*n, B is n*m;  1: A is n*n*N, B is n*m*N;
                             2: PER-INSTANCE dynamics, A is n*n*N*batch, B is n*m*N*batch (QP b's stages are contiguous):
                                the KKT system of every QP is factored on the device and the sweeps stream their stage
                                operators from HBM per QP (the (n, m) pairs of csrc/admm_pinst.hip and
                                admm_pinst_g1.hip, n <= 6; precision_mode FP64 only) */
  int32_t stage_bounds;   /* 0: lo/hi are (m+n);     1: lo/hi are (m+n)*N;   2 (with time_varying = 2 only): per
                             instance, lo/hi are (m+n)*N*batch */
  const double* A;
  const double* B;
  const double* Q;        /* n*n symmetric PSD */
  const double* R;        /* m*m symmetric PSD (R + rho I must be PD) */
  const double* QN;       /* n*n symmetric PSD, terminal weight */
  const double* x0;       /* n*batch */
  const double* lo;       /* block order (u then x); -inf allowed */
  const double* hi;       /* +inf allowed */
  const double* q;        /* L*batch linear cost, or NULL for q = 0 */
  /* Optional thrust-magnitude (second-order-cone) constraint ||u_k||_2 <= unorm_k on the control
   * rows, replacing their box: NULL = off; otherwise 1 entry (stage_bounds = 0) or N entries
   * (stage_bounds = 1), +inf = no constraint at that stage.  Where it is finite the box of the
   * control rows must be (-inf, +inf); the state rows keep their box. */
  const double* unorm;
} admm_problem;

typedef struct admm_options {
  double rho;             /* > 0 */
  double alpha;           /* over-relaxation in (0, 2); 1 = none */
  double eps_abs;
  double eps_rel;
  int32_t max_iter;
  int32_t check_interval; /* residuals + stop test every this many iterations */
  int32_t segments;       /* parallel-in-time segments of the x-update; 0 = auto (per-instance dynamics: at most 64) */
  int32_t device;         /* HIP device ordinal; -1 = current device */
  int32_t zrows;          /* rows per workgroup chunk in the z/dual kernel; 0 = auto */
  int32_t flags;          /* ADMM_FLAG_* */
  /* Adaptive rho by residual balancing (Boyd et al. 2011 §3.4.1), batch-level because the KKT
   * factor is shared by the batch.  At a checked iteration it with it % adapt_interval == 0, with
   * R = sum r_b^2 and S = sum s_b^2 over the QPs that have not converged yet:
   *   R > adapt_mu^2 S  ->  rho *= adapt_tau;     S > adapt_mu^2 R  ->  rho /= adapt_tau
   * then the scaled dual is rescaled (y *= rho_old / rho_new), the KKT system is refactored on
   * the host and the records re-uploaded.  adapt_interval = 0 disables (default).
   * With per-instance dynamics (time_varying = 2) every QP has its own factor, and the rule runs PER QP, on the
   * device (ABI v5): QP b compares R = r_b^2 with S = s_b^2, its rho, dual rescale and refactor are its own, adapt_max
   * counts its changes; admm_info.rho is then the largest rho in force, admm_info.rho_updates the number of changes
   * summed over the batch, and admm_get_rho returns every QP's rho. */
  int32_t adapt_interval; /* iterations between adaptation tests; 0 = fixed rho; must be a multiple of check_interval */
  int32_t adapt_max;      /* at most this many rho changes per admm_solve */
  double adapt_mu;        /* > 1 */
  double adapt_tau;       /* > 1 */
  /* Arithmetic of the x-update (ABI v4; BASELINE.json configs[4]).  ADMM_PRECISION_*:
   *   FP64       fp64 throughout; the library picks the kernel form: one lane per QP with fp64 vector FMAs (every
   *              compiled (n, m), q, thrust-magnitude bound), or FP64_MFMA's kernels where those are faster -- the
   *              smallest batches (ADMM_FLAG_NO_MFMA).
   *   FP64_MFMA  the fused stage operators as chains of v_mfma_f64_16x16x4_f64 over 16-QP panels, always: the same
   *              fp64 iteration (iterates equal to the one-lane kernels' to rounding).
   *   MIXED      as FP64_MFMA, but the two products of the Riccati form (forward rollout, backward elimination:
   *              operators O(1)) run in fp32 on v_mfma_f32_16x16x4_f32, at half the matrix-pipe cycles; the two of
   *              the forward-elimination form (gains up to 2.5e4) stay fp64, as do the state v, the z-update, the
   *              dual and the residuals.  Iterates then carry ~1e-6 relative error.  admm_solve refines in fp64: it
   *              iterates in this form until the stopping rule holds with eps_abs, eps_rel raised to at least 1e-4,
   *              then continues with the FP64_MFMA kernels until it holds as given (admm_info.mixed_iters = length
   *              of the first phase).  admm_run / admm_iterate always run the mixed form.
   * The two MFMA forms exist for the (n, m) pairs of csrc/admm_mfma.hip, without a thrust-magnitude bound and without q
   * (except FP64 / FP64_MFMA at (6, 3) with a batch of up to 128 QPs, where q is supported): ADMM_ERR_UNSUPPORTED otherwise. */
  int32_t precision_mode;
  int32_t reserved;       /* must be 0 */
} admm_options;

#define ADMM_PRECISION_FP64 0
#define ADMM_PRECISION_MIXED 1
#define ADMM_PRECISION_FP64_MFMA 2

#define ADMM_FLAG_NONE 0
#define ADMM_FLAG_NO_GRAPH 1   /* accepted, no effect: direct launches are the default (see ADMM_FLAG_GRAPH) */
#define ADMM_FLAG_GRAPH 16     /* replay captured hipGraphs (one per iteration form) instead of launching
                                  the 2-4 kernels of an iteration directly.  Off by default: on ROCm 7.2 /
                                  MI355X a graph launch per iteration costs ~5 us MORE than the direct
                                  launches it replaces, at every problem size measured */
#define ADMM_FLAG_SCAN_CHAIN 4 /* segment scan as the sequential per-QP chain (xscan_kernel) instead of
                                  the fp64-MFMA GEMM form (xscan_mfma_kernel) */
#define ADMM_FLAG_UNFUSED 2    /* iterate with separate forward-rollout and z/dual kernels (w stored
                                  every iteration) instead of the fused xfz kernel */

#define ADMM_FLAG_NO_MFMA 32    /* ADMM_PRECISION_FP64 only: always the one-lane-per-QP kernels.  By default FP64 takes the
                                  fp64 MFMA form of the fused kernels (same iteration, iterates equal to rounding;
                                  DESIGN.md §4.9) where it is compiled for (n, m), the problem has no q and no
                                  thrust-magnitude bound, and it is the faster of the two -- measured (tools/family_time.py):
                                  batches of at most 64 QPs, or at most 128 with n >= 9 (one wave per segment runs a chain
                                  of ~15 MFMAs per stage instead of a few hundred dependent vector FMAs).  Larger batches
                                  run the one-lane kernels, whose stage operators are distributed over the lanes of a row
                                  and applied with v_fmac_f64_dpp (round 3): faster than the MFMA form at every shape
                                  from 256 QPs on, n = 12 included */

#define ADMM_FLAG_HISTORY 64     /* admm_solve records, at every stopping test, (iteration, converged QPs, max primal residual, max dual
                                   residual, rho in force) for admm_get_history; costs one read-back of the per-QP residuals per test */
#define ADMM_FLAG_ROW_MAJOR 128   /* per-instance dynamics only (time_varying = 2; ABI v8): every n x n block of A and n x m block of B is
                                   ROW-major (C / NumPy order) instead of column-major.  The caller's arrays are then uploaded as they
                                   are and the blocks are transposed on the device on the way into the library's layout -- a NumPy or C
                                   caller otherwise transposes 7 GB on the host per admm_update_problem at n = 12, 4096 x 1000.  Fixed at
                                   admm_setup: admm_update_problem of the handle reads A, B the same way.  Q, R, QN are symmetric;
                                   ADMM_ERR_UNSUPPORTED with batch-shared dynamics (their small A, B are cheap to transpose). */
#define ADMM_FLAG_NO_ALTERNATE 8 /* always eliminate backward / substitute forward (xb + xfz kernels); by
                                  default (unless the forward form fails its host check for the problem),
                                  consecutive iterations alternate the elimination direction so that each
                                  substitution sweep is fused with the next elimination sweep.
                                  ACCURACY: with this flag the iterates stay within 1e-10 of the sequential Riccati
                                  loop's on every stage at any iteration count (measured <= 7e-13 through 400
                                  iterations at N = 1000).  The default path holds 1e-10 on the stages past the
                                  early-gain zone of the forward form (stage 64 on: measured <= 2e-11) at any
                                  count, and on every stage through the first 16 iterations of a fresh handle;
                                  the controls of the first few stages then drift -- at N = 1000, n = 6, rho = 0.8 ... 2
                                  they leave 1e-10 between iterations 80 and 200 and reach 3e-10 by 400 (2e-9 at
                                  rho = 16); 1.3e-11 at rho = 0.05, 4e-12 at N = 200 (measured; DESIGN.md §4.8, §5;
                                  tests/test_gpu_alt_drift.py holds them to a NumPy emulation of the form).  A caller
                                  that needs 1e-10 on u_0 at any count sets this flag (29.33 instead of 21.33 B per
                                  stacked element and iteration at n = 6, m = 3). */

typedef struct admm_info {
  int32_t iters_run;      /* batch iterations executed by the last admm_solve */
  int32_t n_converged;    /* QPs that met the stopping rule */
  double  max_r;          /* max over the batch of the last checked primal residual */
  double  max_s;          /* ... dual residual */
  double  solve_ms;       /* wall time of the last admm_solve (host clock) */
  double  rho;            /* rho in force at the end of the solve */
  int32_t rho_updates;    /* rho changes made by the adaptive rule during the solve */
  int32_t mixed_iters;    /* ADMM_PRECISION_MIXED: iterations run in fp32 before the fp64 refinement phase (else 0) */
} admm_info;

typedef struct admm_handle admm_handle;

/* Defaults: rho 0.1, alpha 1, eps 1e-6/1e-6, max_iter 4000, check_interval 10, fixed rho
 * (adapt_interval 0, adapt_max 16, adapt_mu 10, adapt_tau 2). */
void admm_default_options(admm_options* o);

/* Validate, factor the x-update's KKT system on the host (fp64 Riccati sweep),
 * allocate device memory, upload.  State starts at z = y = w = 0. */
int admm_setup(admm_handle** out, const admm_problem* p, const admm_options* o);

/* Replace the per-instance data (x0: n*batch, q: L*batch or NULL = keep) of an
 * existing handle without refactoring.  Both arrays are checked before anything is written; on
 * ADMM_ERR_INVALID the handle is unchanged. */
int admm_update_instances(admm_handle* h, const double* x0, const double* q);

/* Change rho on an existing handle: refactors the KKT system on the host, re-uploads the
 * records and rescales the scaled dual (y *= rho_old / rho_new) so that the unscaled multiplier
 * rho y is unchanged.  If the handle's segment count was chosen by admm_setup (options.segments = 0), the
 * conditioning bound applied there (largest entry of the segment-scan matrix <= 100) is re-checked on the new
 * factor: a rho that breaks it is refused with ADMM_ERR_NUMERIC and the handle is unchanged (the segment count
 * of a live handle is frozen).  The adaptive rule of admm_solve treats such a refusal as "keep rho and stop
 * adapting". */
int admm_set_rho(admm_handle* h, double rho);

/* New shared problem data on an existing handle: dynamics, weights, box, thrust-magnitude bounds, x0 and
 * q of *p replace those of admm_setup (same N, n, m, batch; q present iff it was; a thrust-magnitude
 * bound present iff one was).  The KKT system is refactored with the current rho and segment count and
 * everything re-uploaded; device buffers, the state (kept as the (z, y) pair) and per-QP results are left
 * alone.  This is what a successive-convexification caller does between outer iterations instead of
 * admm_free + admm_setup.  The conditioning bound of admm_set_rho applies here too.  On failure the handle is
 * unchanged. */
int admm_update_problem(admm_handle* h, const admm_problem* p);

/* Minimum-fuel cost (new symbols of ABI v9, announced by ADMM_HIP_HAS_FUEL -- no struct or signature changed):
 *
 *     ... + sum_k fuel_k ||u_k||_2,   fuel_k >= 0
 *
 * the propellant of a single gimballed thruster, usually together with the thrust bound ||u_k||_2 <= unorm_k.  Its solutions
 * coast and burn: where the term wins, the control rows of z are exactly zero.  Only the z-update changes: the control rows of a
 * stage are shrunk by fuel_k / rho, then scaled onto the ball (with fuel_k = 0 the thrust-bound projection, bit for bit).
 *
 * admm_setup_fuel: admm_setup with the weights `fuel`, in unorm's shape -- 1 entry with stage_bounds = 0, N entries with
 *   stage_bounds = 1; finite and >= 0, and where an entry is positive the box of that stage's control rows must be (-inf, +inf)
 *   (ADMM_ERR_INVALID otherwise, checked before a device is looked for).  fuel = NULL is exactly admm_setup.  Needs batch-shared
 *   dynamics (time_varying 0 or 1) and ADMM_PRECISION_FP64; per-instance dynamics, the MFMA precision modes and time-sharded
 *   handles are refused with ADMM_ERR_UNSUPPORTED.  The handle runs the one-lane fp64 kernels (thrust-magnitude forms) whether
 *   or not unorm is given; all of the solver -- adaptive rho, over-relaxation, q, warm starts, admm_update_instances,
 *   admm_update_problem (which keeps the weights and checks the new box against them), admm_set_rho -- works on it.
 * admm_set_fuel: replace the weights (same shape) of such a handle between iterations -- continuation in the weight with a warm
 *   start.  The state is kept as the (z, y) pair; on failure nothing has changed.  ADMM_ERR_INVALID on a handle that was not set
 *   up with weights: a fuel term cannot be added to a handle.
 * admm_get_fuel: the N per-stage weights in force (zeros on a handle without the term). */
#define ADMM_HIP_HAS_FUEL 1
int admm_setup_fuel(admm_handle** out, const admm_problem* p, const admm_options* o, const double* fuel);
int admm_set_fuel(admm_handle* h, const double* fuel);
int admm_get_fuel(admm_handle* h, double* fuel);

/* Scenario consensus (new symbols, announced by ADMM_HIP_HAS_CONSENSUS -- no struct or signature changed, ABI
 * version unchanged): the batch is batch / group_size consecutive groups of group_size QPs (QP b belongs to group b / group_size),
 * and the QPs of a group share ONE control profile:
 *
 *     minimise  sum_{b in g} [ 1/2 w_b'P w_b + q_b'w_b + sum_k fuel_k ||u_{b,k}|| ]
 *     s.t.      each b's dynamics from its own x0,  lo <= w_b <= hi (and ||u|| <= unorm_k),  u_{b,k} = ubar_{g,k} for all b in g
 *
 * -- open-loop robust guidance over a cloud of initial conditions: the state box holds for EVERY scenario, not for their mean.
 * Global-consensus ADMM: only the z-update changes; the control rows of a stage are projected once per group, on the group's
 * mean of v (box clip, or the shrink-and-scale of the thrust bound / fuel term), and written to every QP of the group.
 *
 * admm_setup_consensus: admm_setup_fuel (fuel may be NULL) with the group size.  ADMM_ERR_INVALID: group_size < 1 or not a divisor
 *   of batch.  ADMM_ERR_UNSUPPORTED: time_varying = 2, precision_mode other than ADMM_PRECISION_FP64, m > 6.  (A time-sharded form
 *   cannot be asked for: admm_setup_timeshard takes no group size.)  Refused before a device is looked for, nothing allocated.  The handle runs the unfused one-lane fp64 path
 *   (ADMM_FLAG_UNFUSED is set internally: admm_get_path reports alternating = alt_requested = 0).  Everything else works as on any
 *   handle -- admm_solve*, admm_run / admm_iterate, admm_step_z, the adaptive rule and admm_set_rho, admm_update_problem*,
 *   admm_update_instances*, admm_set_state* / admm_get*, admm_set_fuel, admm_get_certificate* (per QP, mu_b = rho y_b),
 *   ADMM_FLAG_GRAPH, admm_profile with fused_path = 0 -- except admm_probe_infeasibility* and admm_mpc_advance* (a per-QP Farkas
 *   certificate and a per-QP plant step are not the coupled problem's) and admm_profile with fused_path != 0 (the fused kernels
 *   carry the per-QP z-update): ADMM_ERR_UNSUPPORTED, the handle unchanged.
 * admm_get_consensus: the control rows of each group's z, (batch / group_size) x N x m doubles, group-major.  Brings the state into
 *   the (z, y) pair first, as admm_get does.  ADMM_ERR_INVALID on a handle without groups.
 * admm_get_consensus_device: ubar is device memory of the handle's GPU, under the rules of admm_get_certificate_device. */
#define ADMM_HIP_HAS_CONSENSUS 1
int admm_setup_consensus(admm_handle** out, const admm_problem* p, const admm_options* o, const double* fuel, int32_t group_size);
int admm_get_consensus(admm_handle* h, double* ubar);
int admm_get_consensus_device(admm_handle* h, double* ubar, void* hip_stream);

/* Soft box constraints (new symbols, announced by ADMM_HIP_HAS_SOFT -- no struct or signature changed, ABI version
 * unchanged): the box of chosen rows is enforced by an exact L1 penalty instead of absolutely.  `soft` has the shape of lo / hi --
 * nb entries with stage_bounds = 0, nb N with stage_bounds = 1 --, every entry s >= 0; +inf keeps the row hard, 0 ignores its box.
 * The cost gains
 *
 *     sum_rows s_i max(lo_i - w_i, 0, w_i - hi_i)
 *
 * and only the z-update changes: with v = w^ + y and kap_i = s_i / rho,  c = clip(v, lo, hi), e = v - c,
 * z = |e| <= kap ? c : (e > 0 ? v - kap : v + kap), y = v - z.  The penalty is exact: for s above the row's multiplier in the hard
 * problem the solutions coincide; where the hard problem has no solution the soft one is the least-violating at that price.
 * mu = rho y keeps its meaning (rho y in s d dist(z)).  The control rows of a stage with a finite unorm or a positive fuel weight
 * keep their shrink-and-scale projection: their entries must be +inf.
 *
 * admm_setup_soft: admm_setup_fuel (fuel may be NULL) with the weights.  ADMM_ERR_INVALID: soft = NULL, a negative or NaN entry, a
 *   finite entry on such a control row.  ADMM_ERR_UNSUPPORTED: time_varying = 2, precision_mode other than ADMM_PRECISION_FP64.
 *   (Time-sharded and consensus forms cannot be asked for: neither set-up call takes weights.)  Refused before a device is looked
 *   for, nothing allocated.  The handle runs the unfused one-lane fp64 path (ADMM_FLAG_UNFUSED is set internally); the state is
 *   always the (z, y) pair.  Everything else works as on any handle -- admm_solve*, admm_run / admm_iterate, admm_step_z, the
 *   adaptive rule and admm_set_rho, q, over-relaxation, admm_update_instances*, admm_set_state* / admm_get*, admm_set_fuel,
 *   admm_get_certificate*, ADMM_FLAG_GRAPH, admm_mpc_advance* (the weights are window-relative like the per-stage box: nothing
 *   shifts), admm_profile with fused_path = 0 (fused_path != 0: ADMM_ERR_UNSUPPORTED).  admm_update_problem* keeps the weights, per
 *   stacked row, and re-checks the control-row rule against the new problem.  admm_probe_infeasibility* treats a row with a finite
 *   weight as open: a feasible QP is still never flagged.
 * admm_set_soft: replace the weights (same shape) between iterations -- continuation in the penalty from a warm start.  Every check
 *   comes first: a refused call changes nothing.  ADMM_ERR_INVALID on a handle set up without weights.
 * admm_get_soft: the weights in force, one per stacked row (L doubles; +inf everywhere on a handle without weights).
 * admm_get_soft_report: per QP, on the handle's z and over the rows with a finite weight: penalty = sum s_i dist_i (an fma chain in
 *   row order), max_violation = max dist_i, n_violated = rows with dist_i > 0.  batch entries each; any pointer may be NULL, not all.
 *   obj of admm_get_certificate does NOT include the penalty: the total objective is obj + penalty.
 * admm_get_soft_report_device: the outputs are device memory of the handle's GPU, under the rules of admm_get_certificate_device
 *   (n_violated: 4-byte alignment). */
#define ADMM_HIP_HAS_SOFT 1
int admm_setup_soft(admm_handle** out, const admm_problem* p, const admm_options* o, const double* fuel, const double* soft);
int admm_set_soft(admm_handle* h, const double* soft);
int admm_get_soft(admm_handle* h, double* soft);
int admm_get_soft_report(admm_handle* h, double* penalty, double* max_violation, int32_t* n_violated);
int admm_get_soft_report_device(admm_handle* h, double* penalty, double* max_violation, int32_t* n_violated, void* hip_stream);

/* One half-space per stage (new symbols, announced by ADMM_HIP_HAS_HALFSPACE -- no struct or signature changed,
 * ABI version unchanged): stage k constrains xi_k, the first nh state rows of block k = (u_k, x_{k+1}), 1 <= nh <= n, by
 *
 *     a_k' xi_k <= b_k
 *
 * -- the tangent plane of a keep-out sphere, re-linearised about the last trajectory by the caller.  a, b are C order, a[b][k][i]
 * and b[b][k]: shared by the batch (per_instance = 0: N nh and N doubles) or one set per QP (per_instance != 0: batch N nh and
 * batch N).  a_k = 0 exactly: the stage has no half-space and its rows keep their box.  Where a stage has a plane for any QP, state
 * rows 0 .. nh - 1 of that stage must have the box (-inf, inf) (with stage_bounds = 0: of the one block); a, b must be finite and
 * a_k'a_k of a stage with a plane a normal number.  Only the z-update changes: with v = w^ + y on those rows,
 *     nn = a'a, d = a'v - b (fma chains in row order), t = d > 0 ? d / nn : 0, z_i = fma(-t, a_i, v_i), y_i = v_i - z_i,
 * the Euclidean projection, independent of rho.  The other state rows and the control rows keep what they have (box, ball, fuel).
 *
 * admm_setup_halfspace: admm_setup_fuel (fuel may be NULL) with the planes.  ADMM_ERR_INVALID: nh out of range, NULL a or b, a
 *   non-finite entry, a closed box under a plane.  ADMM_ERR_UNSUPPORTED: time_varying = 2, precision_mode other than
 *   ADMM_PRECISION_FP64.  (Time-sharded, consensus and soft forms cannot be asked for: none of those set-up calls takes planes.)
 *   Refused before a device is looked for, nothing allocated.  The handle runs the unfused one-lane fp64 path (ADMM_FLAG_UNFUSED is
 *   set internally); the state is always the (z, y) pair.  Everything else works as on a soft handle -- admm_solve*, admm_run /
 *   admm_iterate, admm_step_z, the adaptive rule and admm_set_rho, q, over-relaxation, admm_update_instances*, admm_set_state* /
 *   admm_get*, admm_set_fuel, admm_get_certificate* (none of its quantities involves the constraint set), ADMM_FLAG_GRAPH (the
 *   planes keep their device addresses across admm_set_halfspace*), admm_profile with fused_path = 0.  admm_update_problem* keeps
 *   the planes and re-checks the open-box rule against the new box.  ADMM_ERR_UNSUPPORTED on such a handle: admm_mpc_advance* (a
 *   per-QP plane is not window-relative), admm_probe_infeasibility* (its certificate is written for boxes and the ball),
 *   admm_profile with fused_path != 0.
 * admm_set_halfspace: replace a, b (same form, same nh) between iterations; the state is kept as a warm start.  Every check comes
 *   first: a refused call changes nothing.  ADMM_ERR_INVALID on a handle set up without half-spaces.
 * admm_set_halfspace_device: a, b are device memory of the handle's GPU, under the rules of admm_set_state_device; the per-QP
 *   arrays are checked on the device.
 * admm_get_halfspace: the planes in force, in the caller's order and form.
 * admm_get_halfspace_report: per QP (batch entries; any pointer may be NULL, not all):
 *     max_violation = max_k (a_k' w_xi - b_k)+ / sqrt(a_k'a_k)  on w, the dynamics-feasible iterate of the last x-update
 *     n_active      = number of stages with lam_k > 0
 *     lam[b][k]     = rho (a_k' y_xi) / a_k'a_k  (batch N doubles), the multiplier of the stage's inequality: the sensitivity of
 *                     the cost to b_k -- for a keep-out plane, to the radius.  0 at a stage without a plane.
 * admm_get_halfspace_report_device: the outputs are device memory of the handle's GPU, under the rules of
 *   admm_get_certificate_device (n_active: 4-byte alignment). */
#define ADMM_HIP_HAS_HALFSPACE 1
int admm_setup_halfspace(admm_handle** out, const admm_problem* p, const admm_options* o, const double* fuel,
                         const double* a, const double* b, int32_t nh, int32_t per_instance);
int admm_set_halfspace(admm_handle* h, const double* a, const double* b);
int admm_set_halfspace_device(admm_handle* h, const double* a, const double* b, void* hip_stream);
int admm_get_halfspace(admm_handle* h, double* a, double* b);
int admm_get_halfspace_report(admm_handle* h, double* max_violation, int32_t* n_active, double* lam);
int admm_get_halfspace_report_device(admm_handle* h, double* max_violation, int32_t* n_active, double* lam, void* hip_stream);

/* One approach cone per stage (new symbols, announced by ADMM_HIP_HAS_CONE -- no struct or signature changed, ABI
 * version unchanged): stage k constrains xi_k, the first nh state rows of block k = (u_k, x_{k+1}), 1 <= nh <= n, to the second-order
 * cone of axis c_k, apex p_k and slope gamma_k > 0 (the tangent of the half-angle):
 *
 *     r <= gamma s,     e = c / |c|,   s = e'(xi - p),   r = |(xi - p) - s e|_2
 *
 * c, apex, gamma are C order, c[b][k][i], apex[b][k][i], gamma[b][k]: shared by the batch (per_instance = 0: N nh, N nh and N
 * doubles) or one set per QP (per_instance != 0: batch N nh, batch N nh and batch N).  c_k = 0 exactly: the stage has no cone and its
 * rows keep their box.  Where a stage has a cone for any QP, state rows 0 .. nh - 1 of that stage must have the box (-inf, inf) (with
 * stage_bounds = 0: of the one block).  Every entry must be finite; where c_k != 0, c_k'c_k must be a normal number and gamma_k a
 * positive normal number with 1 + gamma_k^2 finite.  Only the z-update changes: the rows v = w^ + y of a stage with a cone get their
 * Euclidean projection onto it -- v itself inside, the apex where v lies in the polar cone, else the nearest point of the surface
 * (csrc/admm_prox.hpp, cone_project) -- independent of rho.  The cone is convex: no re-linearisation.  The other state rows and the
 * control rows keep what they have (box, ball, fuel).
 *
 * admm_setup_cone: admm_setup_fuel (fuel may be NULL) with the cones, under the rules of admm_setup_halfspace: ADMM_ERR_INVALID for
 *   nh out of range, a NULL array, a non-finite entry, an unusable c'c or gamma, a closed box under a cone; ADMM_ERR_UNSUPPORTED for
 *   time_varying = 2 or a precision_mode other than ADMM_PRECISION_FP64; refused before a device is looked for.  The handle runs the
 *   unfused one-lane fp64 path, the state is always the (z, y) pair, and everything that works on a half-space handle works on it.
 *   admm_update_problem* keeps the cones and re-checks the open-box rule.  ADMM_ERR_UNSUPPORTED on such a handle: admm_mpc_advance*,
 *   admm_probe_infeasibility*, admm_profile with fused_path != 0.
 * admm_set_cone: replace c, apex, gamma (same form, same nh) between iterations; the state is kept as a warm start.  Every check
 *   comes first: a refused call changes nothing.  ADMM_ERR_INVALID on a handle set up without cones.
 * admm_set_cone_device: the arrays are device memory of the handle's GPU, under the rules of admm_set_state_device; the per-QP arrays
 *   are checked on the device.  A captured graph survives either call: the cones keep their device addresses.
 * admm_get_cone: the cones in force, in the caller's order and form.
 * admm_get_cone_report: per QP (batch entries; any pointer may be NULL, not all):
 *     max_violation = max_k (r_k - gamma_k s_k)+ / sqrt(1 + gamma_k^2)  on w, the dynamics-feasible iterate of the last x-update
 *     n_active      = number of stages with a cone whose y_xi has a nonzero entry
 *     lam[b][k]     = rho |y_xi|_2  (batch N doubles), the size of the stage's multiplier.  0 at a stage without a cone.
 * admm_get_cone_report_device: the outputs are device memory of the handle's GPU, under the rules of admm_get_certificate_device
 *   (n_active: 4-byte alignment). */
#define ADMM_HIP_HAS_CONE 1
int admm_setup_cone(admm_handle** out, const admm_problem* p, const admm_options* o, const double* fuel, const double* c,
                    const double* apex, const double* gamma, int32_t nh, int32_t per_instance);
int admm_set_cone(admm_handle* h, const double* c, const double* apex, const double* gamma);
int admm_set_cone_device(admm_handle* h, const double* c, const double* apex, const double* gamma, void* hip_stream);
int admm_get_cone(admm_handle* h, double* c, double* apex, double* gamma);
int admm_get_cone_report(admm_handle* h, double* max_violation, int32_t* n_active, double* lam);
int admm_get_cone_report_device(admm_handle* h, double* max_violation, int32_t* n_active, double* lam, void* hip_stream);

/* Warm start / test hook: overwrite device state.  Any pointer may be NULL
 * (left unchanged).  Each is L*batch and must be finite (ADMM_ERR_INVALID otherwise, nothing uploaded). */
int admm_set_state(admm_handle* h, const double* w, const double* z, const double* y);

/* Run until every QP met the rule at a checked iteration, or max_iter.
 * z0/y0 (L*batch) may be NULL: continue from the handle's current state. */
int admm_solve(admm_handle* h, const double* z0, const double* y0, admm_info* info);

/* admm_solve in pieces, for callers that need a decision between checks -- in particular a
 * multi-GPU solve, where each rank owns a shard of the batch and the stop decision (and the
 * adaptive-rho sums) must be global:
 *   admm_solve_begin(h, z0, y0);
 *   loop: admm_solve_step(h, &it, &nconv, &R, &S);       // runs up to and including the next check
 *         [all-reduce  batch - nconv  (SUM),  R, S (SUM)  over the ranks]
 *         stop if nothing is left unconverged or it >= max_iter;
 *         admm_solve_adapt(h, R_global, S_global, &changed);   // no-op unless an adaptation is due
 *   admm_solve_end(h, &info);
 * admm_solve is exactly this loop with local values.  R, S = sums of r^2, s^2 over the QPs that
 * have not converged (NULL to skip the read-back). */
int admm_solve_begin(admm_handle* h, const double* z0, const double* y0);
int admm_solve_step(admm_handle* h, int32_t* iters_done, int32_t* n_converged, double* R, double* S);
int admm_solve_adapt(admm_handle* h, double R, double S, int32_t* changed);
int admm_solve_end(admm_handle* h, admm_info* info);

/* Run exactly `iters` iterations, no residuals, no stop test (benchmark and
 * iterate-parity path).  Asynchronous on the handle's stream; admm_sync waits. */
int admm_iterate(admm_handle* h, int32_t iters);
/* As admm_iterate, but every `residual_every`-th iteration (0 = never) runs the
 * residual-evaluating form of the fused z kernel plus the residual finalise
 * kernel on the device; still no host synchronisation and no early exit.
 * residual_every = 1 is the benchmark's "step": x-update + fused
 * z/dual/residual-partials + finalise, every iteration. */
int admm_run(admm_handle* h, int32_t iters, int32_t residual_every);
/* Iterations launched since setup in the lean residual form: consecutive residual-evaluating iterations of admm_run on a
 * handle whose state rows are unbounded at every stage neither read nor write v of those rows.
 * Diagnostic: 0 on every handle the form does not apply to, and with ADMM_NO_LEAN_RESID=1 in the environment. */
int admm_get_lean_iterations(admm_handle* h, int64_t* count);
int admm_sync(admm_handle* h);

/* Single steps, for kernel-level parity tests. */
int admm_step_x(admm_handle* h);                    /* w <- x-update(z, y) */
int admm_step_z(admm_handle* h, int32_t residuals); /* (z, y) <- z/dual update; residual partials if != 0 */

/* Residual norms of the last residual-evaluating z-step: each array is `batch`
 * long and may be NULL.  r = |w - z+|, s = rho |z+ - z|, nw = |w|, nz = |z+|,
 * ny = rho |y+|. */
int admm_get_residuals(admm_handle* h, double* r, double* s, double* nw, double* nz, double* ny);

/* Copy out the state; any pointer may be NULL.  Each is L*batch. */
int admm_get(admm_handle* h, double* w, double* z, double* y);

/* DEVICE-MEMORY forms (ABI v9): the same calls with every array pointer in device memory of the handle's GPU
 * (admm_setup_device: of options.device, or of the current device if that is -1) -- for callers that hold their data on the GPU
 * already (torch tensors, hipMalloc'd arrays): nothing crosses PCIe but the small arrays below.  Sizes, layouts, NULL rules, flags
 * (ADMM_FLAG_ROW_MAJOR included) and the data checks are those of the host forms, with the same status and message for the same
 * data; on failure nothing of the handle has changed.  Any alignment of 8 bytes or more is accepted (a view at an offset).
 *   - Every non-NULL pointer is checked with hipPointerGetAttributes: pageable or pinned host memory, another GPU's memory, or an
 *     allocation shorter than the array gives ADMM_ERR_INVALID with a message naming the argument.
 *   - hip_stream is the caller's stream (a hipStream_t).  The library's stream waits for what the caller has queued on it before
 *     reading (or, admm_get_device, writing) the caller's arrays.  hip_stream = NULL: the caller vouches that its data are ready.
 *   - The input calls (setup, update_problem, update_instances, set_state) return once the caller's arrays have been consumed:
 *     the caller may overwrite or free them then.  admm_get_device returns WITHOUT a host synchronisation: hip_stream waits for the
 *     library's writes (work queued on it afterwards sees the state); with hip_stream = NULL it returns with the writes complete.
 *   - The per-instance arrays (A, B of time_varying = 2, the box of stage_bounds = 2, x0, q, w, z, y) are read on the device, the
 *     large ones checked there in one pass; the small ones (Q, R, QN, unorm, batch-shared A, B and box) are copied to the host
 *     (the host factorisation of batch-shared dynamics needs them there).
 *   - Time-sharded handles (admm_setup_timeshard): ADMM_ERR_UNSUPPORTED from each of the four calls on a handle. */
int admm_setup_device(admm_handle** out, const admm_problem* p, const admm_options* o, void* hip_stream);
int admm_update_problem_device(admm_handle* h, const admm_problem* p, void* hip_stream);
int admm_update_instances_device(admm_handle* h, const double* x0, const double* q, void* hip_stream);
int admm_set_state_device(admm_handle* h, const double* w, const double* z, const double* y, void* hip_stream);
int admm_get_device(admm_handle* h, double* w, double* z, double* y, void* hip_stream);

/* Certificate of a handle's current point (new symbols, announced by ADMM_HIP_HAS_CERTIFICATE -- no struct or
 * signature changed): costates of the dynamics, objective and optimality measures of every QP, computed on the device from the
 * (z, y) pair with mu = rho y (rho: the value in force) and g = P z + q + mu:
 *   nu        nu_N = -g^x_N,  nu_k = A_k' nu_{k+1} - g^x_k  (k = N-1 .. 1): nu_{k+1} is the multiplier of stage k's dynamics row, and
 *             the state rows of g + G'nu are zero by construction; B_k' nu_{k+1} is the primer vector
 *   stat      max_k |g^u_k - B_k' nu_{k+1}|_inf: the whole stationarity defect of the original QP (not of the ADMM splitting)
 *   feas_dyn  max_k |x_{k+1} - A_k x_k - B_k u_k|_inf on z
 *   obj       1/2 z'Pz + q'z + sum_k fuel_k ||z_u,k||_2  (the weights of admm_get_fuel; NOT the penalty of a soft box: admm_get_soft_report)
 * Any output pointer may be NULL; obj, feas_dyn, stat: batch entries; nu: N*n*batch, QP b at [b*N*n, (b+1)*N*n), stage-major
 * (nu_1 .. nu_N).  The call brings the state into the (z, y) pair exactly as admm_get does and changes nothing else: iterating
 * on gives the same bits as after admm_get.  Only what was asked for is copied out (batch doubles per scalar output).
 * admm_get_certificate_device: the outputs are device memory of the handle's GPU, under the rules of admm_get_device (pointer
 * checks naming the argument, hip_stream ordering, no host synchronisation, 8-byte alignment).
 * Batch-shared dynamics (time_varying 0 or 1) on every iteration path; ADMM_ERR_UNSUPPORTED, before anything is launched, with
 * per-instance dynamics (time_varying = 2) and on time-sharded handles. */
#define ADMM_HIP_HAS_CERTIFICATE 1
int admm_get_certificate(admm_handle* h, double* obj, double* feas_dyn, double* stat, double* nu);
int admm_get_certificate_device(admm_handle* h, double* obj, double* feas_dyn, double* stat, double* nu, void* hip_stream);

/* Infeasibility probe (new symbols, announced by ADMM_HIP_HAS_INFEASIBILITY -- no struct or signature
 * changed): a Farkas certificate of every QP from the drift of the scaled dual.  The call brings the state into the (z, y) pair as
 * admm_get does, keeps y, runs `span` iterations as admm_run(h, span, 0) does and brings the state into (z, y) again; the state
 * afterwards is, bit for bit, that of admm_get; admm_run(span, 0); admm_get, and per-QP iters and status are untouched.  With
 * lambda = (y_after - y_before) / span in block order (u_k, x_{k+1}), on the device:
 *   nu          nu_N = -lambda^x_N,  nu_k = A_k' nu_{k+1} - lambda^x_k  (k = N-1 .. 1): the ray costates
 *   mu          -G'nu: the state rows are lambda's by construction, the control rows are REPLACED by B_k' nu_{k+1}
 *   drift       |lambda|_inf (tends to 0 on a feasible QP)
 *   defect      |mu - lambda|_inf / |mu|_inf (diagnostic: how far the drift is from a pure ray)
 *   sep         (x0' A_0' nu_1 + sigma_C(mu)) / |mu|_inf, sigma_C the support function of the box (the ball ||u_k|| <= unorm_k on
 *               the control rows of a stage with a finite thrust bound); +inf if mu = 0 or if a row whose needed bound is infinite
 *               has |mu_i| > eps |mu|_inf.  A feasible QP has sep >= 0 in exact arithmetic whatever the iterates are.
 *   infeasible  1 iff sep < -eps: a proof, up to rounding and the eps of the open rule, that no w meets the dynamics and the bounds
 * Any output pointer may be NULL; sep, drift, defect, infeasible: batch entries; nu: N*n*batch, laid out as admm_get_certificate's.
 * admm_probe_infeasibility_device: the outputs are device memory of the handle's GPU, under the rules of
 * admm_get_certificate_device (infeasible: 4-byte aligned).
 * ADMM_ERR_INVALID: span < 1, eps not finite or negative.  ADMM_ERR_UNSUPPORTED: per-instance dynamics (time_varying = 2),
 * time-sharded handles, precision_mode MIXED, an (n, m) without a compiled kernel.  Everything is checked before anything is
 * launched or allocated: a refused call leaves the handle as it was.  Fuel weights change the cost, not feasibility: they do not
 * enter. */
#define ADMM_HIP_HAS_INFEASIBILITY 1
int admm_probe_infeasibility(admm_handle* h, int32_t span, double eps, double* sep, double* drift, double* defect,
                             int32_t* infeasible, double* nu);
int admm_probe_infeasibility_device(admm_handle* h, int32_t span, double eps, double* sep, double* drift, double* defect,
                                    int32_t* infeasible, double* nu, void* hip_stream);

/* Outer step of the batched successive-convexification loop on the device (new symbols, announced by
 * ADMM_HIP_HAS_SCVX -- no struct or signature changed): the device counterparts of scvx.rollout, scvx.linearise,
 * scvx.correction_qp_batch and the decision block of scvx.scvx_batch for the shipped model (exact relative motion about a circular
 * orbit, classical RK4 with `substeps` sub-intervals per stage; n = 6, m = 3).  The calls need no solver handle: they take a device
 * ordinal and the caller's stream (a hipStream_t; NULL: the null stream), on which all their work is queued -- ordered after what
 * the caller queued there, before what it queues next.  Every array is device memory of `device` in QP-major C order:
 *   x0 (batch, 6);  u, ub, u_cand (batch, N, 3);  x, xb, x_cand (batch, N, 6): x_1 .. x_N
 *   A (batch, N, 6, 6), B (batch, N, 6, 3): ROW-major blocks (what ADMM_FLAG_ROW_MAJOR takes)
 *   lo, hi, q, z (batch, N, 9) in block order (u_k, x_{k+1});  J, tr_u, tr_x, active, converged, accepted, outer, take: (batch)
 *   history (history_capacity, batch, 9): cost, cost_candidate, predicted, actual, ratio, tr_u, tr_x, du_max, accepted of the
 *   outer iteration a trajectory was active in (record outer[b] of trajectory b)
 * Q, R, QN of admm_scvx_params are row-major (symmetric in use).
 *   admm_scvx_rollout_device  x = the nonlinear trajectory from x0 under u
 *   admm_scvx_init_device     the loop's start: ub = 0, xb = rollout, J = its cost, radii (tr_u, tr_x), active = 1, the rest 0
 *   admm_scvx_prepare_device  the correction QPs about (ub, xb): A, B by central differences (step fd_eps), q = (R ub_k, Q xb_k)
 *                             (QN at the last stage), lo = max(u_lo - ub, -tr_u) | -tr_x, hi = min(u_hi - ub, tr_u) | tr_x; a
 *                             trajectory that is not active gets radii 0 (a zero-width box)
 *   admm_scvx_advance_device  from the QPs' solutions z: the candidate (u_cand = clip(ub + du), x_cand = its rollout), predicted and
 *                             actual decrease, and per ACTIVE trajectory the decision of scvx.scvx_batch -- stop if predicted <=
 *                             tol max(1, |J|); else accept if ratio >= rho_reject (radii doubled if ratio >= rho_expand), else radii
 *                             halved; stop if accepted and |du|_inf <= tol --, one history record, and the accepted candidates
 *                             copied into (ub, xb).  A trajectory that is not active on entry is left as it is (take = 0).
 *                             *n_active (host): trajectories still active; the call returns once it is there -- the loop's one
 *                             synchronisation per outer iteration.
 * ADMM_ERR_INVALID, naming the argument, before anything is launched: N, batch or substeps < 1; dt, rc or fd_eps not finite or not
 * positive; a NULL pointer; a pointer that is not device memory of `device`, or whose allocation ends before the array does; an
 * active trajectory whose record would not fit in history_capacity. */
#define ADMM_HIP_HAS_SCVX 1
typedef struct { int32_t N, batch, substeps; double dt, rc; } admm_scvx_model;
typedef struct { double Q[36], R[9], QN[36], u_lo[3], u_hi[3], fd_eps, tol, rho_reject, rho_expand; } admm_scvx_params;
typedef struct {   /* device pointers */
  double *ub, *xb, *u_cand, *x_cand, *J, *tr_u, *tr_x;
  int32_t *active, *converged, *accepted, *outer, *take;
  double* history;
  int32_t history_capacity;
} admm_scvx_state;
int admm_scvx_rollout_device(int32_t device, const admm_scvx_model* model, const double* x0, const double* u, double* x, void* hip_stream);
int admm_scvx_init_device(int32_t device, const admm_scvx_model* model, const admm_scvx_params* params, const double* x0,
                          admm_scvx_state* state, double tr_u, double tr_x, void* hip_stream);
int admm_scvx_prepare_device(int32_t device, const admm_scvx_model* model, const admm_scvx_params* params, const double* x0,
                             const admm_scvx_state* state, double* A, double* B, double* lo, double* hi, double* q, void* hip_stream);
int admm_scvx_advance_device(int32_t device, const admm_scvx_model* model, const admm_scvx_params* params, const double* x0,
                             const double* z, admm_scvx_state* state, int32_t* n_active, void* hip_stream);

/* The model of the device outer step as an argument (new symbols, announced by ADMM_HIP_HAS_SCVX_MODELS --
 * no struct or signature changed, ABI version unchanged).  admm_scvx_dynamics names a model compiled into the library (`kind`) and
 * gives its parameters; n = 6, m = 3 for every kind:
 *   ADMM_SCVX_RELATIVE_CIRCULAR  the model of admm_scvx_model: par[0] = rc
 *   ADMM_SCVX_CRTBP              circular restricted three-body problem, nondimensional rotating frame, primaries at X = -mu and
 *                                X = 1 - mu; s = (x, y, z, vx, vy, vz) with the position measured from (x_ref, 0, 0), u a thrust
 *                                acceleration: par[0] = mu, par[1] = x_ref.  With X = x_ref + x, d1 = X + mu, d2 = X - 1 + mu,
 *                                r_i = d_i^2 + y^2 + z^2, k1 = (1 - mu) / r1^(3/2), k2 = mu / r2^(3/2):
 *                                  ax = 2 vy + X - k1 d1 - k2 d2 + ux,  ay = -2 vx + y - (k1 + k2) y + uy,  az = -(k1 + k2) z + uz
 *                                Nothing is special near a primary: inf / NaN propagate into the cost and the candidate is rejected.
 * Unused par entries and `reserved` are 0.  The four calls are admm_scvx_{rollout,init,prepare,advance}_device with the dynamics in
 * place of the model: same array layouts, admm_scvx_params, admm_scvx_state, stream rules, and every check before the first HIP call
 * and before any launch.  ADMM_ERR_INVALID names the field: dynamics.N, .batch, .substeps < 1; .dt not finite and positive; an unknown
 * .kind; .reserved != 0; a non-zero unused .par entry; kind 0: par[0] (rc) not finite and positive; kind 1: par[0] (mu) not finite or
 * not in (0, 1), par[1] (x_ref) not finite.  admm_scvx_model_name: "relative_circular", "crtbp"; NULL for an unknown kind. */
#define ADMM_HIP_HAS_SCVX_MODELS 1
enum { ADMM_SCVX_RELATIVE_CIRCULAR = 0, ADMM_SCVX_CRTBP = 1 };
typedef struct { int32_t N, batch, substeps, kind; double dt; double par[4]; int32_t reserved; } admm_scvx_dynamics;
const char* admm_scvx_model_name(int32_t kind);
int admm_scvx_rollout_model_device(int32_t device, const admm_scvx_dynamics* dynamics, const double* x0, const double* u, double* x,
                                   void* hip_stream);
int admm_scvx_init_model_device(int32_t device, const admm_scvx_dynamics* dynamics, const admm_scvx_params* params, const double* x0,
                                admm_scvx_state* state, double tr_u, double tr_x, void* hip_stream);
int admm_scvx_prepare_model_device(int32_t device, const admm_scvx_dynamics* dynamics, const admm_scvx_params* params, const double* x0,
                                   const admm_scvx_state* state, double* A, double* B, double* lo, double* hi, double* q,
                                   void* hip_stream);
int admm_scvx_advance_model_device(int32_t device, const admm_scvx_dynamics* dynamics, const admm_scvx_params* params, const double* x0,
                                   const double* z, admm_scvx_state* state, int32_t* n_active, void* hip_stream);

/* Time-dependent models of the device outer step (new symbols, announced by
 * ADMM_HIP_HAS_SCVX_STAGE_MODELS -- no struct or signature changed, ABI version unchanged).  A stage is integrated by classical RK4
 * over `substeps` sub-intervals of h = dt / substeps, so the right-hand side is evaluated at the times t0 + g h / 2 of the global
 * nodes g = 0 .. 2 substeps N: sub-interval i of stage k, g0 = 2 (substeps k + i), reads node g0 (k1), g0 + 1 (k2, k3) and g0 + 2
 * (k4).  The model reads ADMM_SCVX_NODE_PAR doubles per node from `nodes` (n_nodes rows, row-major, GPU memory of the call's device,
 * shared by all trajectories; n_nodes = 2 substeps N + 1).  The library computes no epoch: a caller who moves the window passes a
 * pointer further into a longer table.  n = 6, m = 3:
 *   ADMM_SCVX_STAGE_RELATIVE_TABULATED  exact relative motion in the rotating frame of a chief that moves in a plane, x radial,
 *                                       y along-track, z cross-track; the node's row (rc, w, wd, g) = chief radius, angular rate,
 *                                       angular acceleration, the chief's radial gravity mu / rc^2; par[0] = mu.  With xr = rc + x,
 *                                       r2 = xr^2 + y^2 + z^2, k = mu / r2^(3/2):
 *                                         ax =  2 w vy + wd y + w^2 x + g - k xr + ux
 *                                         ay = -2 w vx - wd x + w^2 y     - k y  + uy
 *                                         az =                            - k z  + uz
 * The four calls are admm_scvx_{rollout,init,prepare,advance}_model_device with this struct in place of admm_scvx_dynamics: same
 * array layouts, admm_scvx_params, admm_scvx_state and stream rules.  ADMM_ERR_INVALID names the field, before the first HIP call:
 * dynamics.N, .batch, .substeps < 1; .dt not finite and positive; an unknown .kind; .reserved != 0; par[0] (mu) not finite and
 * positive; par[1..3] != 0; .nodes NULL; .n_nodes != 2 substeps N + 1.  Then `nodes` is checked like every other array: memory of
 * that device, 4 n_nodes doubles long.  Its values are not scanned: a NaN or inf propagates into the cost and the candidate is
 * rejected.  admm_scvx_stage_model_name: "relative_tabulated"; NULL for an unknown kind. */
#define ADMM_HIP_HAS_SCVX_STAGE_MODELS 1
#define ADMM_SCVX_NODE_PAR 4
enum { ADMM_SCVX_STAGE_RELATIVE_TABULATED = 0 };
typedef struct { int32_t N, batch, substeps, kind; double dt; double par[4];
                 const double* nodes; int64_t n_nodes; int32_t reserved; } admm_scvx_stage_dynamics;
const char* admm_scvx_stage_model_name(int32_t kind);
int admm_scvx_rollout_stage_device(int32_t device, const admm_scvx_stage_dynamics* dynamics, const double* x0, const double* u, double* x,
                                   void* hip_stream);
int admm_scvx_init_stage_device(int32_t device, const admm_scvx_stage_dynamics* dynamics, const admm_scvx_params* params, const double* x0,
                                admm_scvx_state* state, double tr_u, double tr_x, void* hip_stream);
int admm_scvx_prepare_stage_device(int32_t device, const admm_scvx_stage_dynamics* dynamics, const admm_scvx_params* params, const double* x0,
                                   const admm_scvx_state* state, double* A, double* B, double* lo, double* hi, double* q,
                                   void* hip_stream);
int admm_scvx_advance_stage_device(int32_t device, const admm_scvx_stage_dynamics* dynamics, const admm_scvx_params* params, const double* x0,
                                   const double* z, admm_scvx_state* state, int32_t* n_active, void* hip_stream);

/* Costates and a first-order optimality certificate of the NONLINEAR problem the SCvx loop works on (new
 * symbols, announced by ADMM_HIP_HAS_SCVX_ADJOINT -- no struct or signature changed, ABI version unchanged): one backward sweep
 * over ub and the A, B, q that admm_scvx_prepare_device (any model) wrote about the reference (ub, xb) -- q = (qu_k, qx_k) =
 * (R ub_k, Q xb_{k+1}).  It needs no handle and no model.  Per trajectory b (device arrays, layouts as above; any output may be
 * NULL, not all; a NULL output is neither computed into memory nor stored):
 *   nu      (batch, N, 6)  nu[b, k] = nu_{k+1}, the costate of stage k's dynamics: nu_N = -qx_{N-1},
 *                          nu_{k+1} = A_{k+1}' nu_{k+2} - qx_k for k = N-2 .. 0
 *   primer  (batch, N, 3)  B_k' nu_{k+1}
 *   grad    (batch, N, 3)  qu_k - primer_k = dJ/du_k at fixed x0 (J: the cost of scvx.trajectory_cost; symmetric weights)
 *   dJdx0   (batch, 6)     -A_0' nu_1 = dJ/dx_0 at fixed u
 *   stat    (batch)        the maximum over (k, j) of the violation of component (k, j), with exact comparisons: 0 if
 *                          u_lo_j == u_hi_j; max(-g, 0) if ub == u_lo_j; max(g, 0) if ub == u_hi_j; |g| otherwise (g = grad).
 *                          NaN if any entry of the trajectory's grad is a NaN
 *   n_bound (batch) int32  the number of components with ub == u_lo_j or ub == u_hi_j
 * Every dot product is one fma chain in ascending index whose accumulator starts from the subtracted term (0 where there is none).
 * Of params only u_lo and u_hi are read.  Queued on the caller's stream, no host synchronisation.  ADMM_ERR_INVALID names the
 * argument, before the first HIP call or launch: N or batch < 1; NULL params, ub, A, B, q or out; every field of out NULL; a pointer
 * that is not memory of `device` or whose allocation ends early.  Values are not scanned. */
#define ADMM_HIP_HAS_SCVX_ADJOINT 1
typedef struct { double *nu, *primer, *grad, *dJdx0, *stat; int32_t* n_bound; } admm_scvx_adjoint_out; /* device; any may be NULL, not all */
int admm_scvx_adjoint_device(int32_t device, int32_t N, int32_t batch, const admm_scvx_params* params,
                             const double* ub, const double* A, const double* B, const double* q,
                             const admm_scvx_adjoint_out* out, void* hip_stream);

/* Receding-horizon (MPC) step on the device (new symbols, announced by ADMM_HIP_HAS_MPC -- no struct or
 * signature changed): apply the first control, propagate the plant, move the window one stage.  Per QP b, in this order:
 *   1. the state is brought into the (z, y) pair and w into memory, as admm_get does
 *   2. u = z_u,0 + du            (rows 0 .. m-1 of block 0 of z; one addition per row, none with du = NULL)
 *   3. x+ = x_meas if given; else row i: acc = dx_i (or 0), acc = fma(Ap[i,j], x0_j, acc) for j ascending, then
 *      acc = fma(Bp[i,j], u_j, acc) for j ascending
 *   4. x0 <- x+, with the effect of admm_update_instances(h, x+, NULL)
 *   5. w, z, y, and q if the handle has one: block k <- block k+1 (k = 0 .. N-2); block N-1 keeps its content (TAIL_COPY) or
 *      becomes 0 (TAIL_ZERO); q's block N-1 is q_tail if given
 *   6. the flags are those admm_set_state(h, w', z', y') leaves; per-QP iters, status, residuals, rho, the factor and the
 *      certificate / infeasibility caches are untouched
 * The call equals, bit for bit in the state and in every later iterate, admm_get; that shift on the host;
 * admm_update_instances(x+, q'); admm_set_state(w', z', y').  The problem data are window-relative: time_varying = 1 and
 * stage_bounds = 1 are served as they are (a shifted z may lie outside its new stage's box, as admm_set_state allows).
 * Ap (n*n) and Bp (n*m) are HOST memory in both forms, column-major like admm_problem.A; NULL = the handle's A_0 / B_0.
 * du (m*batch), dx, x_meas (n*batch), q_tail (nb*batch), u_applied (m*batch), x_next (n*batch) are QP-major; each may be NULL.
 * admm_mpc_advance_device: those six are device memory of the handle's GPU -- pointer checks, finite scans and stream hand-over as
 * admm_update_instances_device (inputs) and admm_get_device (outputs): hip_stream waits for the library's writes; the only host
 * synchronisation is the finite scan's, and with no input array the call queues its work and returns (hip_stream = NULL: it
 * returns with the work complete).
 * ADMM_ERR_UNSUPPORTED (nothing launched, the handle unchanged): per-instance dynamics (time_varying = 2), time-sharded handles.
 * ADMM_ERR_INVALID (likewise): s = NULL, an unknown tail, reserved != 0, x_meas together with Ap / Bp / dx, q_tail on a handle
 * without q, a non-finite entry in any input. */
#define ADMM_HIP_HAS_MPC 1
#define ADMM_MPC_TAIL_COPY 0   /* the last block keeps its old content (the old block N-1 appears twice) */
#define ADMM_MPC_TAIL_ZERO 1   /* the last block of w, z, y becomes 0 */
typedef struct admm_mpc_step {
  const double* Ap;      /* plant, n*n column-major like admm_problem.A; NULL = the handle's A_0 */
  const double* Bp;      /* n*m; NULL = the handle's B_0.  Ap, Bp are HOST memory in both forms */
  const double* du;      /* m*batch, added to the commanded control (actuation error); NULL = 0 */
  const double* dx;      /* n*batch, added to the propagated state (process noise); NULL = 0 */
  const double* x_meas;  /* n*batch: if given, the new x0 is this and the plant is not evaluated; Ap, Bp, dx must then be NULL */
  const double* q_tail;  /* nb*batch: the new last block of q; NULL = q's tail follows `tail` */
  int32_t tail;          /* ADMM_MPC_TAIL_* */
  int32_t reserved;      /* 0 */
} admm_mpc_step;
int admm_mpc_advance(admm_handle* h, const admm_mpc_step* s, double* u_applied, double* x_next);
int admm_mpc_advance_device(admm_handle* h, const admm_mpc_step* s, double* u_applied, double* x_next, void* hip_stream);

/* Per-QP results of the last admm_solve: first checked iteration at which the
 * rule held (max_iter if never), status (1 converged / 0 not), last r and s. */
int admm_get_info(admm_handle* h, int32_t* iters, int32_t* status, double* r, double* s);

/* Timing hook for bench.py: runs `iters` iterations with HIP events recorded
 * on the handle's stream around each kernel launch and returns average
 * durations in ms.  fused_path == 1 (the plain fused path, ADMM_FLAG_NO_ALTERNATE):
 *   ms = {xb, xscan, xfz, 0, finalise, whole iteration}
 * fused_path == 0 (ADMM_FLAG_UNFUSED path):
 *   ms = {xb, xscan, xf, zdual, finalise, whole iteration}
 * fused_path == 2 (the default alternating-direction path; ADMM_ERR_UNSUPPORTED if the
 * handle does not run it): `iters` PAIRS of iterations,
 *   ms = {xscan, xfze, xscan (+ finalise role), xbze, 0, whole pair}
 * fused_path == 3 (the same path, BACK-TO-BACK cross-check: no event between launches): `iters` consecutive
 * (xfze, xbze) pairs without the scans, then each scan form `iters` times in a row,
 *   ms = {xscan (W), mean of xfze and xbze, xscan (WB) (+ finalise role), the same mean, 0, sum of the four}
 * (not ADMM iterates: the state is parked, restored, and ONE plain iteration is applied to leave the handle consistent).
 * fused_path == 4: as 2, with the pair in its lean residual forms (admm_get_lean_iterations; residuals must be set;
 * ADMM_ERR_UNSUPPORTED where the forms do not apply).  Modes 2 and 3 always time the full-read / full-write forms.
 * xb = x-update backward sweep, xscan = segment scan, xf = forward rollout,
 * zdual = standalone fused z/dual/residual kernel, xfz = forward rollout fused
 * with z/dual/residual.  `residuals` selects the residual-evaluating kernel
 * forms (+ the finalise kernel).
 * The call ADVANCES the state, by ordinary ADMM iterations: `iters` of them in modes 0 and 1, 2 iters + 1 in modes 2 and 4 (the
 * pairs, then one forward form: a call never returns after a backward form), one in mode 3.  Modes 2, 3 and 4 start from the
 * state as v = z + y: when the handle holds it as the (z, y) pair -- after admm_setup, admm_set_state with z or y, admm_set_rho,
 * admm_update_problem, admm_set_fuel, admm_step_z, a rho change of admm_solve_adapt, or iterations of an ADMM_FLAG_UNFUSED
 * handle or of mode 0 -- ONE plain iteration is applied first (2 iters + 2, or 2, in all).  With `residuals` the last iteration
 * applied leaves its norms for admm_get_residuals. */
int admm_profile(admm_handle* h, int32_t iters, int32_t residuals, int32_t fused_path, double ms[6]);

/* Residual history of the last admm_solve (ADMM_FLAG_HISTORY; ABI v5): one entry per stopping test, oldest first.  *count =
 * number of entries recorded; at most `capacity` of them are copied into each non-NULL array.  max_r / max_s are maxima over
 * the real QPs of the batch (converged or not) of the residuals of that iteration; rho is the one in force during it (the
 * largest one with per-instance dynamics). */
int admm_get_history(admm_handle* h, int32_t capacity, int32_t* count, int32_t* iteration, int32_t* n_converged,
                     double* max_r, double* max_s, double* rho);

/* rho of every QP (batch entries): the handle's rho for batch-shared dynamics, each QP's own with per-instance
 * dynamics (where the adaptive rule moves them apart; admm_set_rho sets them all).  ABI v5. */
int admm_get_rho(admm_handle* h, double* rho);

/* Geometry chosen at setup, for roofline accounting: pitch = padded batch,
 * segs = x-update segments, zrows = rows per z-kernel chunk, zchunks. */
int admm_get_geometry(admm_handle* h, int32_t* pitch, int32_t* segs, int32_t* zrows, int32_t* zchunks);

/* Which kernels the handle runs, and the measured margin of the default path (ABI v6).  The default iteration alternates
 * the elimination direction; its forward-elimination factor carries large early-stage gains, so admm_setup
 * (and every refactor: admm_set_rho, the adaptive rule, admm_update_problem) verifies it on the host -- one x-update with a
 * random linear term through both forms -- and falls back to the plain fused path (29.33 instead of 21.33 B per stacked
 * element and iteration at n = 6, m = 3) when the relative mismatch alt_check exceeds alt_gate.  That fallback is reported
 * here and through admm_last_warning(), never silently.  The gate bounds ONE x-update; what it implies for the iterates is
 * stated at ADMM_FLAG_NO_ALTERNATE: 1e-10 past the first stages at any iteration count and everywhere through 16 iterations,
 * not 1e-10 on the controls of the first stages of a long run at rho >= 0.2 on a long horizon. */
typedef struct admm_path_info {
  int32_t alternating;     /* 1: the alternating-direction fused kernels run; 0: the plain fused (or unfused) path */
  int32_t alt_requested;   /* 1: options / compiled kernels allow alternation for this problem class (0: ADMM_FLAG_NO_ALTERNATE,
                              _UNFUSED, _SCAN_CHAIN, per-instance dynamics, (n, m) without the fused kernels) */
  int32_t mfma;            /* kernel family of the fused sweeps: 0 one lane per QP (fp64 VALU), 1 MIXED, 2 fp64 MFMA */
  int32_t xfree;           /* 1: every state row is unbounded at every stage: iterations without residuals neither read nor
                              write v of those rows (XFREE forms) */
  int32_t segments;        /* parallel-in-time segments of the x-update */
  int32_t auto_segments;   /* 1: chosen by admm_setup (and guarded by the conditioning bound on every refactor) */
  int32_t scan_form;       /* segment scan: 0 fp64-MFMA GEMM, 1 matrix-vector (batches <= 4), 2 sequential chain, 3 per-QP (per-instance) */
  int32_t per_instance;    /* 1: time_varying = 2 (device factor, operands per QP from HBM) */
  double  alt_check;       /* relative mismatch of the forward-elimination form on the host verification vector; -1: not run
                              (alternation not requested, or the form could not be built: a singular A_k or covariance) */
  double  alt_gate;        /* the bound alt_check must meet (5e-12, on one x-update: see above for the iterates) */
  double  scan_growth;     /* largest |entry| of the segment-scan matrices (conditioning bound: <= 100 with automatic segments) */
} admm_path_info;
int admm_get_path(admm_handle* h, admm_path_info* info);

/* Geometry of the segment scan as a dense product: the split-K factor the handle runs (1, 2, 4 or 8; chosen at
 * admm_setup from the grid size, 1 on the matrix-vector form), the padded shape M x K of the scan matrix and the number of row
 * groups of xscan_mfma_kernel (M / 64), each with its own k-step range.  Handles with per-instance dynamics scan per QP: they
 * report split 1 and M = K = groups = 0.  Any output pointer may be NULL.  (New symbols of ABI v9 -- this one and
 * admm_host_scan_packed --, announced by ADMM_HIP_HAS_SCAN_GEOMETRY: no struct or signature changed.) */
#define ADMM_HIP_HAS_SCAN_GEOMETRY 1
int admm_get_scan_geometry(admm_handle* h, int32_t* split, int32_t* M, int32_t* K, int32_t* groups);

/* Thread-local diagnostic of the last admm_setup / admm_set_rho / admm_update_problem / admm_solve* call on this thread that
 * SUCCEEDED but changed the kernels a handle runs (the forward-elimination gate above; the adaptive rule refused a rho); ""
 * if there was nothing to report.  Cleared at the start of each of those calls. */
const char* admm_last_warning(void);

/* TIME-SHARDED handles: one batch of QPs whose horizon is cut into segments that live on DIFFERENT ranks (ABI v7).
 * The parallel-in-time x-update couples its segments EXACTLY through 2 n numbers per segment and QP (the segment summaries the
 * elimination sweeps leave, and the boundary values the scan returns) -- so the "shooting segments" of one horizon can sit on
 * different GPUs and exchange just those: every rank factorises the whole horizon on the host, runs the fused kernels of its own
 * S / nranks consecutive segments, and before each segment scan the summaries are completed by an ALL-GATHER over the ranks (the
 * only data-path collective of this library; the residual partial sums of the segments travel the same way before each stopping
 * test, so every rank takes the same decisions).  The iterates are those of one handle holding every segment (up to the rounding
 * of the scan product).
 *
 * The transport is the caller's: `exchange` is called from inside admm_run / admm_iterate / admm_solve* at those points, with
 *   op = ADMM_EXCHANGE_ALLGATHER: `buf` holds nranks slices of `count` doubles in rank order, this rank's slice (at
 *        buf + rank * count) is complete; when the function's work on `hip_stream` is done every slice must be.
 * buf is DEVICE memory.  The function either enqueues the collective on hip_stream (RCCL: nothing waits on the host) or
 * synchronises the stream and moves the data itself (any other transport); it returns 0 on success (anything else fails the
 * calling entry point with ADMM_ERR_HIP).
 *
 * admm_setup_timeshard takes the GLOBAL problem on every rank.  options.segments = total segment count (0 = automatic), a
 * multiple of nranks.  Shared dynamics only, fused paths only (no ADMM_FLAG_UNFUSED / _GRAPH / _SCAN_CHAIN).  A rank ALLOCATES
 * the state (w, z, y, v, q and the feed-forward rows) of its own stages only: admm_set_state / admm_solve(z0, y0) /
 * admm_update_instances(q) take the usual L x batch arrays and use the rows [stage_lo, stage_hi) * (n + m) of every QP,
 * admm_get writes those rows of the caller's arrays and leaves the others alone; the host side assembles the windows
 * (admm_get_window). */
#define ADMM_EXCHANGE_ALLGATHER 0
typedef int (*admm_exchange_fn)(void* ctx, void* hip_stream, int32_t op, double* buf, int64_t count);
int admm_setup_timeshard(admm_handle** out, const admm_problem* p, const admm_options* o, int32_t rank, int32_t nranks,
                         admm_exchange_fn exchange, void* ctx);
/* The rank's window: stages [stage_lo, stage_hi), segments [seg_lo, seg_lo + segs_local) of segs_total.  An ordinary handle
 * reports the whole horizon and rank 0 of 1. */
int admm_get_window(admm_handle* h, int32_t* stage_lo, int32_t* stage_hi, int32_t* seg_lo, int32_t* segs_local, int32_t* segs_total);

void admm_free(admm_handle* h);

/* Host-only helpers (no GPU needed): the fp64 pre-factorisation exactly as
 * admm_setup uploads it, exposed so that the host logic can be tested on a
 * CPU-only machine.  admm_record_sizes gives the per-stage / per-segment record
 * lengths in doubles; admm_host_factor fills K (N*m*n), Sinv (N*m*m), both
 * row-major, the packed backward / forward / segment records (N*rb, N*rf,
 * segments*rs doubles; layouts in csrc/admm_factor.hpp) and seg_start
 * (segments + 1).  Any output pointer may be NULL. */
int admm_record_sizes(int32_t n, int32_t m, int32_t* rb, int32_t* rf, int32_t* rs);
int admm_host_factor(const admm_problem* p, double rho, int32_t segments, double* K, double* Sinv,
                     double* recB, double* recF, double* recS, int32_t* seg_start);
/* The dense segment-scan matrix W (row-major M x K) of the MFMA scan kernel:
 *   [t_in(0..S-1) | pad to Mt | x_in(0..S-1) | pad] = W [tseg(0..S-1) | x0 | eseg(0..S-1) | pad]
 * Call with W = NULL to query M, Mt, K first. */
int admm_host_scan_matrix(const admm_problem* p, double rho, int32_t segments, double* W, int32_t* M,
                          int32_t* Mt, int32_t* K);
/* The same matrix as xscan_mfma_kernel reads it: Wp = W in MFMA fragment order (k-step-major, M / 16 tiles of 64 doubles per
 * k-step, element `lane` of a tile = W[16 tile + (lane & 15)][4 kstep + (lane >> 4)]; M * K doubles) and range = the k-step range
 * [begin, end) of each group of 4 tiles (2 * groups entries) outside which the group's rows of W are zero.  backward != 0: the
 * pack and ranges of WB, the scan matrix of the forward-elimination form (admm_host_factor_alt).  sizes[4] = {M, K, groups, ok};
 * ok = 0: backward was asked for and that form could not be built (Wp and range are then untouched;
 * with sizes = NULL the call returns ADMM_ERR_NUMERIC instead, so that it cannot go unnoticed).  Call with Wp = range = NULL
 * to query the sizes first.  Any output pointer may be NULL. */
int admm_host_scan_packed(const admm_problem* p, double rho, int32_t segments, int32_t backward, double* Wp, int32_t* range,
                          int32_t* sizes);

/* The same two dense scan matrices (W, and WB if *ok) with their INPUT columns in the rank-by-rank layout of time-sharded handles
 * (admm_setup_timeshard): [rank 0: tseg of its segments | eseg of them][rank 1: ...] ... | x0 | pad.  Shapes as above. */
int admm_host_scan_matrices_timeshard(const admm_problem* p, double rho, int32_t segments, int32_t nranks, double* W, double* WB,
                                      int32_t* ok);

/* Alternating-direction iteration: per-stage records of the two fused kernels
 * (rfe / rbe doubles per stage; layouts in csrc/admm_layout.hpp) and the dense scan matrix WB of
 * the forward-elimination form (same M x K shape and row / column layout as W above:
 *   [m_in(0..S-1) | pad to Mt | lam_in(0..S-1) | pad] = WB [mseg(0..S-1) | x0 | epsseg(0..S-1) | pad]).
 * *ok = 0 if that form could not be built for this problem (outputs are then untouched).
 * Any output pointer may be NULL. */
int admm_record_sizes_alt(int32_t n, int32_t m, int32_t* rfe, int32_t* rbe);
int admm_host_factor_alt(const admm_problem* p, double rho, int32_t segments, double* recFE, double* recBE,
                         double* WB, int32_t* ok);
/* The fused kernels copy these records to on-chip memory in whole KiB pieces, so a device array of them is allocated with a
 * KiB of slack behind `stages` records of `stage_bytes` bytes.  This is the test admm_setup and every refactor apply to their
 * allocations (host only): ADMM_ERR_INVALID if alloc_bytes does not cover stages * stage_bytes rounded up to the next KiB
 * (*needed, may be NULL). */
int admm_record_alloc_check(int64_t alloc_bytes, int32_t stages, int32_t stage_bytes, int64_t* needed);

/* MFMA form (csrc/admm_mfma_layout.hpp): bytes per stage of the forward / backward fragment
 * records of mode ADMM_PRECISION_MIXED or ADMM_PRECISION_FP64_MFMA, and the records themselves (N * bytes each;
 * either pointer may be NULL).  *alt_ok = 0: the ELIM_F / SUB_B fragments are zero (no forward-elimination form). */
int admm_mfma_record_bytes(int32_t n, int32_t m, int32_t mode, int32_t* fwd, int32_t* bwd);
int admm_host_factor_mfma(const admm_problem* p, double rho, int32_t segments, int32_t mode, void* recMF,
                          void* recMB, int32_t* alt_ok);

const char* admm_last_error(void);
int admm_abi_version(void);
/* Number of HIP devices visible (0 if none / no driver). */
int admm_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* ADMM_HIP_H */
