/*
 * osqp_amd.h -- C ABI of the MI355X-native OSQP ADMM engine (libosqp_amd.so).
 *
 * This header is the drop-in boundary.  Part 1 declares exactly the symbols and
 * struct layouts that the reference wrapper osqp/OSQP.jl v0.8.1 binds with
 * `ccall` (every entry cites the reference call site as [REF file:line], paths
 * relative to the reference checkout).  An unmodified OSQP.jl pointed at
 * libosqp_amd.so instead of OSQP_jll's libosqp therefore keeps working
 * (see INTEGRATION.md).  Part 2 declares the extension entry points that have
 * no counterpart in the reference (device-resident problem generation, the
 * batched small-QP path, introspection for measurement).
 *
 * Conventions (same as the reference's FFI): plain pointers and sizes, no C++
 * or torch types; c_int is 64-bit [REF src/types.jl:5-9]; c_float is double;
 * return value 0 means success, anything else is an error that the Julia side
 * turns into `error(...)` [REF src/interface.jl:157-159].
 *
 * All pointers passed IN are borrowed for the duration of the call only (the
 * Julia side holds them under `@preserve` [REF src/interface.jl:132-155]); the
 * library deep-copies.  Everything reachable from an OSQPWorkspace* is owned
 * by the library and released by osqp_cleanup().
 */
#ifndef OSQP_AMD_H
#define OSQP_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef long long c_int;   /* [REF src/types.jl:5-9]  Cc_int = Clonglong */
typedef double    c_float; /* Cdouble everywhere in [REF src/types.jl]   */

/* ------------------------------------------------------------------------- */
/* Part 1a: constants  [REF src/constants.jl:1-21]                            */
/* ------------------------------------------------------------------------- */
#define OSQP_INFTY 1e30 /* [REF src/constants.jl:5] */

enum osqp_linsys_solver_type {
  QDLDL_SOLVER       = 0, /* [REF src/constants.jl:1]  direct LDL^T (default; "auto" here: falls back to PCG when the factor cannot fit) */
  MKL_PARDISO_SOLVER = 1, /* [REF src/constants.jl:2]  accepted, served by the same direct LDL^T back-end */
  AMD_PCG_SOLVER     = 2, /* extension: force the indirect (preconditioned CG) back-end */
  AMD_DIRECT_SOLVER  = 3  /* extension: force the direct back-end (never fall back) */
};

/* status_val codes [REF src/constants.jl:9-21] */
#define OSQP_DUAL_INFEASIBLE_INACCURATE    (4)
#define OSQP_PRIMAL_INFEASIBLE_INACCURATE  (3)
#define OSQP_SOLVED_INACCURATE             (2)
#define OSQP_SOLVED                        (1)
#define OSQP_MAX_ITER_REACHED             (-2)
#define OSQP_PRIMAL_INFEASIBLE            (-3)
#define OSQP_DUAL_INFEASIBLE              (-4)
#define OSQP_SIGINT                       (-5)
#define OSQP_TIME_LIMIT_REACHED           (-6)
#define OSQP_NON_CVX                      (-7)
#define OSQP_UNSOLVED                    (-10)

/* ------------------------------------------------------------------------- */
/* Part 1b: struct layouts read across the boundary                           */
/* ------------------------------------------------------------------------- */

/* Compressed-sparse-column matrix, 56 bytes. [REF src/types.jl:11-19]
 * nz == -1 marks compressed-column form [REF src/types.jl:46]; indices are
 * 0-based [REF src/types.jl:39-43]. */
typedef struct {
  c_int    nzmax;
  c_int    m;
  c_int    n;
  c_int   *p;
  c_int   *i;
  c_float *x;
  c_int    nz;
} csc;

/* 56 bytes. [REF src/types.jl:101-109] */
typedef struct {
  c_int    n;
  c_int    m;
  csc     *P; /* upper triangle only [REF src/interface.jl:102-104] */
  csc     *A;
  c_float *q;
  c_float *l;
  c_float *u;
} OSQPData;

/* 176 bytes, linsys_solver is a 32-bit enum followed by 4 bytes of padding.
 * [REF src/types.jl:111-134] */
typedef struct {
  c_float rho;
  c_float sigma;
  c_int   scaling;
  c_int   adaptive_rho;
  c_int   adaptive_rho_interval;
  c_float adaptive_rho_tolerance;
  c_float adaptive_rho_fraction;
  c_int   max_iter;
  c_float eps_abs;
  c_float eps_rel;
  c_float eps_prim_inf;
  c_float eps_dual_inf;
  c_float alpha;
  int     linsys_solver; /* enum osqp_linsys_solver_type */
  c_float delta;
  c_int   polish;
  c_int   polish_refine_iter;
  c_int   verbose;
  c_int   scaled_termination;
  c_int   check_termination;
  c_int   warm_start;
  c_float time_limit;
} OSQPSettings;

/* 136 bytes. [REF src/types.jl:81-99] */
typedef struct {
  c_int   iter;
  char    status[32];
  c_int   status_val;
  c_int   status_polish;
  c_float obj_val;
  c_float pri_res;
  c_float dua_res;
  c_float setup_time;
  c_float solve_time;
  c_float update_time;
  c_float polish_time;
  c_float run_time;
  c_int   rho_updates;
  c_float rho_estimate;
} OSQPInfo;

/* 16 bytes. [REF src/types.jl:74-77] */
typedef struct {
  c_float *x;
  c_float *y;
} OSQPSolution;

/* 30-field mirror. [REF src/types.jl:173-217]
 * The Julia side dereferences `data`, `solution`, `info`, `delta_y`, `delta_x`
 * as HOST pointers after osqp_solve [REF src/interface.jl:176-205, 744-746].
 * The iterates live in HBM; those five are host mirrors refreshed before
 * osqp_solve returns.  `rho_vec` .. `E_temp` other than delta_x/delta_y are
 * NULL in libosqp_amd.so (device-resident; no reference code reads them). */
typedef struct OSQPWorkspace {
  OSQPData     *data;          /*   0 */
  void         *linsys_solver; /*   8 */
  void         *pol;           /*  16 */
  c_float      *rho_vec;       /*  24 */
  c_float      *rho_inv_vec;   /*  32 */
  c_int        *constr_type;   /*  40 */
  c_float      *x;             /*  48 */
  c_float      *y;             /*  56 */
  c_float      *z;             /*  64 */
  c_float      *xz_tilde;      /*  72 */
  c_float      *x_prev;        /*  80 */
  c_float      *z_prev;        /*  88 */
  c_float      *Ax;            /*  96 */
  c_float      *Px;            /* 104 */
  c_float      *Aty;           /* 112 */
  c_float      *delta_y;       /* 120  host mirror: primal-infeasibility certificate */
  c_float      *Atdelta_y;     /* 128 */
  c_float      *delta_x;       /* 136  host mirror: dual-infeasibility certificate */
  c_float      *Pdelta_x;      /* 144 */
  c_float      *Adelta_x;      /* 152 */
  c_float      *D_temp;        /* 160 */
  c_float      *D_temp_A;      /* 168 */
  c_float      *E_temp;        /* 176 */
  OSQPSettings *settings;      /* 184 */
  void         *scaling;       /* 192 */
  OSQPSolution *solution;      /* 200  host mirror */
  OSQPInfo     *info;          /* 208  host mirror */
  void         *timer;         /* 216 */
  c_int         first_run;     /* 224 */
  c_int         summary_printed; /* 232 */
  void         *impl;          /* 240  library-private (engine handle) */
} OSQPWorkspace;

/* Layout contract, checked at compile time by every translation unit that includes this header (the library
 * itself and tests/c_harness.c): the byte offsets the Julia mirrors imply [REF src/types.jl:11-19, 74-77,
 * 81-99, 101-109, 111-134, 173-217] and that interface.jl reads through `unsafe_load`
 * [REF src/interface.jl:176-205, 744-746]. */
#if defined(__cplusplus)
#define OSQP_AMD_STATIC_ASSERT(c, msg) static_assert(c, msg)
#else
#define OSQP_AMD_STATIC_ASSERT(c, msg) _Static_assert(c, msg)
#endif
#define OSQP_AMD_OFFSET(T, f, o) OSQP_AMD_STATIC_ASSERT(offsetof(T, f) == (o), #T "." #f " must sit at byte " #o)
OSQP_AMD_STATIC_ASSERT(sizeof(c_int) == 8 && sizeof(c_float) == 8 && sizeof(void *) == 8, "64-bit c_int / c_float / pointers");
OSQP_AMD_STATIC_ASSERT(sizeof(csc) == 56, "csc is 56 bytes");
OSQP_AMD_OFFSET(csc, nzmax, 0); OSQP_AMD_OFFSET(csc, m, 8); OSQP_AMD_OFFSET(csc, n, 16); OSQP_AMD_OFFSET(csc, p, 24);
OSQP_AMD_OFFSET(csc, i, 32); OSQP_AMD_OFFSET(csc, x, 40); OSQP_AMD_OFFSET(csc, nz, 48);
OSQP_AMD_STATIC_ASSERT(sizeof(OSQPData) == 56, "OSQPData is 56 bytes");
OSQP_AMD_OFFSET(OSQPData, n, 0); OSQP_AMD_OFFSET(OSQPData, m, 8); OSQP_AMD_OFFSET(OSQPData, P, 16); OSQP_AMD_OFFSET(OSQPData, A, 24);
OSQP_AMD_OFFSET(OSQPData, q, 32); OSQP_AMD_OFFSET(OSQPData, l, 40); OSQP_AMD_OFFSET(OSQPData, u, 48);
OSQP_AMD_STATIC_ASSERT(sizeof(OSQPSettings) == 176, "OSQPSettings is 176 bytes");
OSQP_AMD_OFFSET(OSQPSettings, rho, 0); OSQP_AMD_OFFSET(OSQPSettings, sigma, 8); OSQP_AMD_OFFSET(OSQPSettings, scaling, 16);
OSQP_AMD_OFFSET(OSQPSettings, adaptive_rho, 24); OSQP_AMD_OFFSET(OSQPSettings, adaptive_rho_interval, 32);
OSQP_AMD_OFFSET(OSQPSettings, adaptive_rho_tolerance, 40); OSQP_AMD_OFFSET(OSQPSettings, adaptive_rho_fraction, 48);
OSQP_AMD_OFFSET(OSQPSettings, max_iter, 56); OSQP_AMD_OFFSET(OSQPSettings, eps_abs, 64); OSQP_AMD_OFFSET(OSQPSettings, eps_rel, 72);
OSQP_AMD_OFFSET(OSQPSettings, eps_prim_inf, 80); OSQP_AMD_OFFSET(OSQPSettings, eps_dual_inf, 88); OSQP_AMD_OFFSET(OSQPSettings, alpha, 96);
OSQP_AMD_OFFSET(OSQPSettings, linsys_solver, 104); OSQP_AMD_OFFSET(OSQPSettings, delta, 112); OSQP_AMD_OFFSET(OSQPSettings, polish, 120);
OSQP_AMD_OFFSET(OSQPSettings, polish_refine_iter, 128); OSQP_AMD_OFFSET(OSQPSettings, verbose, 136);
OSQP_AMD_OFFSET(OSQPSettings, scaled_termination, 144); OSQP_AMD_OFFSET(OSQPSettings, check_termination, 152);
OSQP_AMD_OFFSET(OSQPSettings, warm_start, 160); OSQP_AMD_OFFSET(OSQPSettings, time_limit, 168);
OSQP_AMD_STATIC_ASSERT(sizeof(OSQPInfo) == 136, "OSQPInfo is 136 bytes");
OSQP_AMD_OFFSET(OSQPInfo, iter, 0); OSQP_AMD_OFFSET(OSQPInfo, status, 8); OSQP_AMD_OFFSET(OSQPInfo, status_val, 40);
OSQP_AMD_OFFSET(OSQPInfo, status_polish, 48); OSQP_AMD_OFFSET(OSQPInfo, obj_val, 56); OSQP_AMD_OFFSET(OSQPInfo, pri_res, 64);
OSQP_AMD_OFFSET(OSQPInfo, dua_res, 72); OSQP_AMD_OFFSET(OSQPInfo, setup_time, 80); OSQP_AMD_OFFSET(OSQPInfo, solve_time, 88);
OSQP_AMD_OFFSET(OSQPInfo, update_time, 96); OSQP_AMD_OFFSET(OSQPInfo, polish_time, 104); OSQP_AMD_OFFSET(OSQPInfo, run_time, 112);
OSQP_AMD_OFFSET(OSQPInfo, rho_updates, 120); OSQP_AMD_OFFSET(OSQPInfo, rho_estimate, 128);
OSQP_AMD_STATIC_ASSERT(sizeof(OSQPSolution) == 16, "OSQPSolution is 16 bytes");
OSQP_AMD_OFFSET(OSQPSolution, x, 0); OSQP_AMD_OFFSET(OSQPSolution, y, 8);
OSQP_AMD_OFFSET(OSQPWorkspace, data, 0); OSQP_AMD_OFFSET(OSQPWorkspace, linsys_solver, 8); OSQP_AMD_OFFSET(OSQPWorkspace, pol, 16);
OSQP_AMD_OFFSET(OSQPWorkspace, rho_vec, 24); OSQP_AMD_OFFSET(OSQPWorkspace, rho_inv_vec, 32); OSQP_AMD_OFFSET(OSQPWorkspace, constr_type, 40);
OSQP_AMD_OFFSET(OSQPWorkspace, x, 48); OSQP_AMD_OFFSET(OSQPWorkspace, y, 56); OSQP_AMD_OFFSET(OSQPWorkspace, z, 64);
OSQP_AMD_OFFSET(OSQPWorkspace, xz_tilde, 72); OSQP_AMD_OFFSET(OSQPWorkspace, x_prev, 80); OSQP_AMD_OFFSET(OSQPWorkspace, z_prev, 88);
OSQP_AMD_OFFSET(OSQPWorkspace, Ax, 96); OSQP_AMD_OFFSET(OSQPWorkspace, Px, 104); OSQP_AMD_OFFSET(OSQPWorkspace, Aty, 112);
OSQP_AMD_OFFSET(OSQPWorkspace, delta_y, 120); OSQP_AMD_OFFSET(OSQPWorkspace, Atdelta_y, 128); OSQP_AMD_OFFSET(OSQPWorkspace, delta_x, 136);
OSQP_AMD_OFFSET(OSQPWorkspace, Pdelta_x, 144); OSQP_AMD_OFFSET(OSQPWorkspace, Adelta_x, 152); OSQP_AMD_OFFSET(OSQPWorkspace, D_temp, 160);
OSQP_AMD_OFFSET(OSQPWorkspace, D_temp_A, 168); OSQP_AMD_OFFSET(OSQPWorkspace, E_temp, 176); OSQP_AMD_OFFSET(OSQPWorkspace, settings, 184);
OSQP_AMD_OFFSET(OSQPWorkspace, scaling, 192); OSQP_AMD_OFFSET(OSQPWorkspace, solution, 200); OSQP_AMD_OFFSET(OSQPWorkspace, info, 208);
OSQP_AMD_OFFSET(OSQPWorkspace, timer, 216); OSQP_AMD_OFFSET(OSQPWorkspace, first_run, 224); OSQP_AMD_OFFSET(OSQPWorkspace, summary_printed, 232);
OSQP_AMD_OFFSET(OSQPWorkspace, impl, 240); /* past everything the reference mirror declares (240 bytes) */

/* ------------------------------------------------------------------------- */
/* Part 1c: the 30 symbols OSQP.jl binds                                      */
/* ------------------------------------------------------------------------- */

/* [REF src/types.jl:139] */
void osqp_set_default_settings(OSQPSettings *settings);

/* [REF src/interface.jl:147]  0 on success; non-zero (1 data, 2 settings,
 * 4 linsys init, 5 non-convex, 6 alloc) makes setup! throw.
 * data->A: the row indices inside every column must ascend without repeats -- what Julia's SparseMatrixCSC guarantees
 * and ManagedCcsc copies verbatim [REF src/types.jl:21-47]; the arrays serve as the CSR arrays of A' as they are.  A
 * caller that hands over unsorted columns gets exit flag 1, not a wrong answer.  data->P (upper triangle) may come in
 * any order inside its columns. */
c_int osqp_setup(OSQPWorkspace **workp, const OSQPData *data, const OSQPSettings *settings);

/* [REF src/interface.jl:171]  return value ignored by the caller; the outcome
 * is info->status_val. */
c_int osqp_solve(OSQPWorkspace *work);

/* [REF src/interface.jl:220] */
const char *osqp_version(void);

/* [REF src/interface.jl:225]  must accept NULL (finalizer of a never-set-up
 * Model [REF src/interface.jl:24-25]). */
c_int osqp_cleanup(OSQPWorkspace *work);

/* [REF src/interface.jl:241, 259, 277, 303] */
c_int osqp_update_lin_cost(OSQPWorkspace *work, const c_float *q_new);
c_int osqp_update_lower_bound(OSQPWorkspace *work, const c_float *l_new);
c_int osqp_update_upper_bound(OSQPWorkspace *work, const c_float *u_new);
c_int osqp_update_bounds(OSQPWorkspace *work, const c_float *l_new, const c_float *u_new);

/* [REF src/interface.jl:337, 358, 382]  idx are 0-based positions into the
 * setup-time nnz order (P: upper-triangular nnz order); NULL = all nnz. */
c_int osqp_update_P(OSQPWorkspace *work, const c_float *Px_new, const c_int *Px_new_idx, c_int P_new_n);
c_int osqp_update_A(OSQPWorkspace *work, const c_float *Ax_new, const c_int *Ax_new_idx, c_int A_new_n);
c_int osqp_update_P_A(OSQPWorkspace *work, const c_float *Px_new, const c_int *Px_new_idx, c_int P_new_n,
                      const c_float *Ax_new, const c_int *Ax_new_idx, c_int A_new_n);

/* [REF src/interface.jl:476, 580, 593, 606, 619, 632, 645] */
c_int osqp_update_max_iter(OSQPWorkspace *work, c_int max_iter_new);
c_int osqp_update_polish(OSQPWorkspace *work, c_int polish_new);
c_int osqp_update_polish_refine_iter(OSQPWorkspace *work, c_int polish_refine_iter_new);
c_int osqp_update_verbose(OSQPWorkspace *work, c_int verbose_new);
c_int osqp_update_scaled_termination(OSQPWorkspace *work, c_int scaled_termination_new);
c_int osqp_update_check_termination(OSQPWorkspace *work, c_int check_termination_new);
c_int osqp_update_warm_start(OSQPWorkspace *work, c_int warm_start_new);

/* [REF src/interface.jl:489, 502, 515, 528, 541, 554, 567, 658] */
c_int osqp_update_eps_abs(OSQPWorkspace *work, c_float eps_abs_new);
c_int osqp_update_eps_rel(OSQPWorkspace *work, c_float eps_rel_new);
c_int osqp_update_eps_prim_inf(OSQPWorkspace *work, c_float eps_prim_inf_new);
c_int osqp_update_eps_dual_inf(OSQPWorkspace *work, c_float eps_dual_inf_new);
c_int osqp_update_rho(OSQPWorkspace *work, c_float rho_new);
c_int osqp_update_alpha(OSQPWorkspace *work, c_float alpha_new);
c_int osqp_update_delta(OSQPWorkspace *work, c_float delta_new);
c_int osqp_update_time_limit(OSQPWorkspace *work, c_float time_limit_new);

/* [REF src/interface.jl:676, 690, 709] */
c_int osqp_warm_start_x(OSQPWorkspace *work, const c_float *x);
c_int osqp_warm_start_y(OSQPWorkspace *work, const c_float *y);
c_int osqp_warm_start(OSQPWorkspace *work, const c_float *x, const c_float *y);

/* ------------------------------------------------------------------------- */
/* Part 2: extensions (no counterpart in the reference)                       */
/* ------------------------------------------------------------------------- */

/* Synthetic problem families of SURVEY.md section 8d; generated by a
 * counter-based SplitMix64 stream keyed by (seed, stream, index), so the host
 * generator (oracle/gen.c) and the device generator produce identical bits. */
enum osqp_amd_problem_kind {
  OSQP_AMD_GEN_RANDOM_QP = 0, /* n=m, `per_row` nnz per row of A, P = M + M' + diag */
  OSQP_AMD_GEN_LASSO     = 1, /* P diagonal, A = [I; -I], m = 2n */
  OSQP_AMD_GEN_MPC       = 2  /* nx=6, nu=4, T=10: n=100, m=200 */
};

/* Build the problem directly in HBM (no host copy, no PCIe) and run setup on
 * it.  `n` is the number of variables, `per_row` the nnz per row of A (random
 * QP only), `seed` the generator key.  Same return codes as osqp_setup. */
c_int osqp_amd_setup_generated(OSQPWorkspace **workp, c_int kind, c_int n, c_int per_row,
                               unsigned long long seed, const OSQPSettings *settings);

/* Introspection for measurement (bench.py, tests).  Fills `out[0..count)`:
 *  0 back-end in use (0 direct, 2 pcg)      1 nnz(A)          2 nnz(P full symmetric)
 *  3 nnz(triu P)                             4 nnz(L) (direct) 5 levels of the trisolve schedule
 *  6 total CG iterations so far              7 total ADMM iterations so far
 *  8 numeric factorisations so far           9 device bytes allocated
 * 10 algorithmic bytes of one SpMV with A   11 algorithmic bytes of one forward+backward trisolve
 * 12 SpMV kernel used for A: 0 CSR (k_spmv), 2 LDS-staged column panels with sliced-ELL tiles (k_spmv_sell),
 *    3 the same tiles over wide panels gathered through L2 (n >> 1e6 at fixed nnz)
 * 13 ranks of the row partition (1: not sharded)   14 all-gathers issued so far   15 bytes received by them
 * 16, 17 rows of the local blocks (n, m)          18 compact mode (CSR column / value arrays released) 0 / 1
 * 19 levels of the supernode graph when the triangular solves run by supernodes (0: by the level schedule)
 * 20 high-water mark of the device bytes allocated by this process (a sharded setup stays near 1/ranks of the whole)
 * 21 solves that were run again from a cold start because a wait inside the one-launch supernodal solve timed out
 * 22 the numeric factorisation runs by supernodes (multifrontal, one launch per supernode level and size class) 0 / 1
 * 23 the factor's index arrays (CSC pattern of L, scatter maps, supernode lists) were built on the device from a lean host analysis 0 / 1
 * 24 bytes of device address space this process has reserved for mapped blocks and never handed back (ranges are not reused
 *    -- a ROCm 7 re-map defect, csrc/devmem.hip -- so a long-lived process grows this until reservations fail and blocks fall
 *    back to hipMalloc; 128 TiB per process)
 * 25 pivots of the dense top block of the direct back-end (its Schur complement is inverted explicitly: block sweeps on the
 *    fp64 matrix cores from 512 pivots on); 0: none
 * 26 whole-matrix products issued by residual evaluations so far (A x, P x and A' y per evaluation; osqp_amd_iterate evaluates
 *    every check_termination iterations and at its last iteration, once each)
 * Returns the number of entries written (at most OSQP_AMD_STATS_COUNT). */
#define OSQP_AMD_STATS_COUNT 27
c_int osqp_amd_get_stats(const OSQPWorkspace *work, c_float *out, c_int count);

/* Time `reps` launches of one hot-path kernel with HIP events on the engine's
 * own stream; returns the mean milliseconds per launch, <0 on error.
 * which: 0 SpMV A*x, 1 SpMV A'*y, 2 SpMV P*x, 3 forward+backward trisolve,
 *        4 fused ADMM vector update, 5 one whole ADMM iteration of the back-end in use without the residual
 *        evaluation (advances the iterate), 7 one all-gather of an n-vector (sharded workspaces), 8 the active-set check
 *        of osqp_amd_adjoint_retain on the kept derivative factor (<0 without one or with m = 0; changes nothing). */
c_float osqp_amd_time_kernel(OSQPWorkspace *work, c_int which, c_int reps);

/* ---- Row-sharded workspaces: ONE large QP over several GPUs, indirect back-end ----
 *
 * Rank r of R keeps rows [r*ceil(n/R), ...) of A', of the full symmetric P and of every n-vector, and rows
 * [r*ceil(m/R), ...) of A and of every m-vector.  Per product with A, P or A' the input vector is all-gathered
 * (n or m doubles); norms and dot products are all-gathered as scalars and combined in rank order, so all
 * ranks take identical decisions.  Every rank calls the same entry points in the same order with the same
 * arguments (full-length vectors; each rank reads its slice) and receives the full solution.  Setup walks the
 * problem column range by column range and keeps only the rank's row blocks, so the peak device memory of a rank is
 * about 1/R of the single-device workspace (stats[20]; the device generator never materialises the rest at all).  Not available on a
 * sharded workspace: the direct back-end, osqp_amd_apply.  (Round 4: polish runs in its iterative form; osqp_update_P / _A / _P_A
 * take the same full-length value arrays on every rank.)
 *
 * The communicator is one in-place all-gather of doubles; it must outlive the workspaces that use it.
 *   host:  `fn(ctx, host_buf, count)` is called with world*count doubles, chunk `rank` filled in, and fills in the
 *          other chunks (MPI_Allgather, gloo, ...); returns 0.
 *   rccl:  ncclAllGather on the engine's stream.  `unique_id` = the 128 bytes osqp_amd_comm_unique_id wrote on
 *          one rank, distributed by the caller; `librccl_path` (may be NULL) names the librccl to use when the
 *          process does not already hold one. */
typedef struct osqp_amd_comm osqp_amd_comm;
typedef int (*osqp_amd_allgather_fn)(void *ctx, double *host_buf, long long count);
c_int osqp_amd_comm_create_host(osqp_amd_comm **out, c_int rank, c_int world, osqp_amd_allgather_fn fn, void *ctx);
c_int osqp_amd_comm_unique_id(void *out128, const char *librccl_path);
c_int osqp_amd_comm_create_rccl(osqp_amd_comm **out, c_int rank, c_int world, const void *unique_id,
                                const char *librccl_path);
c_int osqp_amd_comm_destroy(osqp_amd_comm *comm);
/* The communicator's one primitive, exposed: in-place all-gather of `count` doubles per rank on a DEVICE buffer of
 * world*count doubles whose chunk `rank` is filled in; blocks until done. */
c_int osqp_amd_comm_all_gather(osqp_amd_comm *comm, c_float *dev_buf, c_int count);
/* rank / size as the communicator was created, and the size the transport itself reports (RCCL: ncclCommCount; the
 * host transport: the size it was created with; -1: the transport cannot say).  Any pointer may be NULL. */
c_int osqp_amd_comm_info(const osqp_amd_comm *comm, c_int *rank, c_int *world, c_int *transport_ranks);
/* as osqp_setup [REF src/interface.jl:147-162] / osqp_amd_setup_generated, keeping this rank's row block */
c_int osqp_amd_setup_sharded(OSQPWorkspace **workp, const OSQPData *data, const OSQPSettings *settings,
                             osqp_amd_comm *comm);
c_int osqp_amd_setup_generated_sharded(OSQPWorkspace **workp, c_int kind, c_int n, c_int per_row,
                                       unsigned long long seed, const OSQPSettings *settings, osqp_amd_comm *comm);

/* Run exactly `iters` ADMM iterations from the current iterate (no
 * termination test inside, residuals refreshed at the end); used by bench.py
 * to time K steps.  Returns 0 on success. */
c_int osqp_amd_iterate(OSQPWorkspace *work, c_int iters);

/* The current iterate in the caller's units (x = D x_scaled, y = E y_scaled / c -- what osqp_solve would store
 * [REF src/interface.jl:176-186]) copied to host buffers of n and m doubles, without touching the iterate: what the
 * headline-size parity record compares after osqp_amd_iterate on the engine and on the oracle.  Either pointer
 * may be NULL. */
c_int osqp_amd_get_iterate(OSQPWorkspace *work, c_float *x_out, c_float *y_out);

/* Element-wise kernel parity hooks (tests only): run one device kernel on
 * host-provided vectors and copy the result back.
 *  op 0: y = A*x (len n -> m)   op 1: y = A'*x (m -> n)   op 2: y = P*x (n -> n)
 *  op 3: y = K^{-1} x through the linear-system back-end (n+m -> n+m)        */
c_int osqp_amd_apply(OSQPWorkspace *work, c_int op, const c_float *in, c_float *out);

/* Which kernel and which layout the products of one matrix run on (tests only; read from what the host already
 * holds, no device work).  which: 0 A, 1 A', 2 P (full symmetric).  Fills out[0..count):
 *  0 kernel, as stats[12]: 0 CSR (k_spmv), 2 LDS-staged panels, 3 wide panels through L2
 *  1 lanes per row G of the CSR kernel (what k_spmv<G> would be launched with)
 *  2 panel shift (panels of 2^shift columns)   3 panels B   4 panels per group Gp   5 groups NG (the reduction depth)
 *  6 tiles   7 slices   8 padded entries of the sliced copy   9 stored entries (nnz)
 * 10 compact (the CSR column / value arrays of this matrix released) 0 / 1
 * 11 fused: the single product adds up its group sums inside the product launch (k_spmv_sell_fused) 0 / 1
 * 12 rshift: reduce blocks of 2^rshift rows (LDS-staged panels)
 * 13 products of this matrix that ran on k_spmv_sell_fused so far (a product onto its own input keeps two kernels and is not
 *    counted, nor is any launch of the two-kernel form)
 * Entries 2-8 and 11-13 are 0 when the matrix runs on the CSR kernel.  Returns the number of entries written (at most
 * OSQP_AMD_LAYOUT_COUNT), 0 on a bad argument. */
#define OSQP_AMD_LAYOUT_COUNT 14
c_int osqp_amd_spmv_layout(const OSQPWorkspace *work, c_int which, c_float *out, c_int count);

/* Which kernel the last batched solve of this process ran (tests, benchmarks): -1 the 512-thread kernel (one QP per eight
 * wavefronts, the factorisation through an n x n scratch in global memory), k >= 0 entry k of the table of instantiations of
 * the four-wavefront kernel (csrc/batch_common.hpp OQ_QUAD_ENTRIES; 0 = the MPC family with its shape compiled in), -2 none yet. */
c_int osqp_amd_batch_last_kernel(void);

/* The schedule of that launch (tests, diagnostics): fills out[0 .. min(count, 11)) with, in this order, the entry number as
 * osqp_amd_batch_last_kernel gives it, the pivots of the two-ended first phase taken from the top and from the bottom
 * (p1_top, p1_bot), the furthest such a pivot reaches (bw), the term slots per thread and assembly window (ns), the longest
 * row held by each of the four wavefronts (kew[0 .. 3]), the bytes of LDS of a workgroup, and the instances launched.  For the
 * 512-thread kernel the schedule numbers are 0 and the bytes are that kernel's; before any launch out[0] = -2 and the rest
 * is 0.  Returns the number of entries written. */
c_int osqp_amd_batch_last_schedule(c_int *out, c_int count);

/* Instances with 128 < n <= 256: an opt-in, process-wide switch, 0 at start; returns the previous
 * value.  While it is 0 nothing differs from a library without it: n > 128 is refused with the message that names 128.
 * While it is 1, osqp_amd_batch_solve and osqp_amd_batch_setup accept 128 < n <= 256 and serve it with k_batch_solve_large:
 * one QP per 512-thread workgroup and compute unit, the inverse of the reduced KKT matrix left in the instance's n x n
 * scratch in global memory and read from there every iteration -- several times slower per iteration than the register
 * kernels, hence a switch.  n > 256 is refused with a message that names 256; a pattern whose LDS need exceeds 160 KB with the
 * usual message; every pattern with n <= 128 goes where it went before, with the same bits.  A resident handle remembers at
 * setup which path it was built on; later changes of the switch do not touch it.  On such a handle every call of the
 * resident surface works; polish, adjoint and JVP work once osqp_amd_batch_large_factor (below) has been switched on for the
 * handle.  By default their capacity check refuses every such handle ("instance too large to polish ...": they keep M in LDS
 * and at most 128 variables per instance), before anything is launched or written; polish = 1 is refused at setup either way.  osqp_amd_batch_last_kernel and out[0] of osqp_amd_batch_last_schedule report -2 for this kernel (with its LDS
 * bytes in out[9]; before any launch they are 0). */
c_int osqp_amd_batch_large(c_int on);
/* What that kernel needs for a shape, on the host alone (no device is touched; the function the launcher uses): nnzF is the
 * number of stored entries of the FULL symmetric P (both triangles).  out[0] = bytes of LDS per workgroup, out[1] = bytes of
 * scratch per instance (8 n^2: the inverse every iteration reads), out[2] = 16 x 16 tiles per wavefront of the inversion.
 * Returns 0 when the shape is accepted; otherwise 1 with the reason in osqp_amd_last_error (n <= 128, n > 256, too much
 * LDS) and out untouched.  It does not look at the switch. */
c_int osqp_amd_batch_large_plan(c_int n, c_int m, c_int nnzA, c_int nnzF, c_int *out);

/* Batched path: `count` independent QPs that
 * share one sparsity pattern.  P (upper triangle) and A are given once as
 * patterns; values are [count x nnz] row-major; q,l,u are [count x n|m].
 * Outputs: x [count x n], y [count x m], info [count] (host pointers).
 * The instances are solved one per workgroup with the reduced KKT system
 * factorised in LDS.  `device` selects the HIP device (one process per GPU). */
c_int osqp_amd_batch_solve(c_int count, c_int n, c_int m,
                           const c_int *Pp, const c_int *Pi, const c_float *Px_all,
                           const c_int *Ap, const c_int *Ai, const c_float *Ax_all,
                           const c_float *q_all, const c_float *l_all, const c_float *u_all,
                           const OSQPSettings *settings,
                           c_float *x_out, c_float *y_out, OSQPInfo *info_out, c_int device);

/* Generate `count` MPC instances [first, first+count) of the mpc-batch family
 * on the device and solve them there; outputs as above but DEVICE pointers
 * (so that the caller can hand them to an RCCL gather without a host hop).
 * info_out is [count x 4] doubles: iter, status_val, pri_res, dua_res. */
c_int osqp_amd_batch_solve_generated(c_int first, c_int count, unsigned long long seed,
                                     const OSQPSettings *settings,
                                     c_float *x_dev, c_float *y_dev, c_float *info_dev, c_int device);

/* The batched path over several GPUs (SURVEY.md 8e, rows K11 + K12): `total` MPC instances of the mpc-batch family
 * (seed `seed`) cut into contiguous equal blocks, instance i -> rank floor(i / (total / world)); one process per GPU.
 * create(): this rank's block is generated in HBM (`comm` NULL = a single rank owning everything; `total` must be
 * divisible by the communicator's size).  solve(): one workgroup per instance writes its row
 * [x (100) | y (200) | iter, status_val, pri_res, dua_res] straight into the packed DEVICE array
 * `packed_dev` [total x 304], then ONE in-place all-gather of the rank blocks over the communicator (RCCL over xGMI,
 * or the host callback) fills in the other ranks' rows; returns when the whole array is valid on this rank.  No other
 * communication. */
typedef struct osqp_amd_batch osqp_amd_batch;
c_int osqp_amd_batch_mpc_create(osqp_amd_batch **out, c_int total, unsigned long long seed, const OSQPSettings *settings,
                                osqp_amd_comm *comm, c_int device);
c_int osqp_amd_batch_mpc_solve(osqp_amd_batch *batch, c_float *packed_dev);
c_int osqp_amd_batch_destroy(osqp_amd_batch *batch);

/* A resident batch of the caller's own QPs (one shared sparsity pattern): set up once, then the life cycle of
 * osqp_setup / osqp_update_* / osqp_warm_start / osqp_solve, instance by instance, without leaving HBM.
 *   setup():  arguments and validation as osqp_amd_batch_solve (host pointers; return codes 1 = data, 2 = settings).  The
 *             handle keeps the RAW data and, per instance, a state record [c, rho, flag, - | D[n] | x[n] | E[m] | z[m] | y[m]]:
 *             the Ruiz factors D, E, c are computed HERE from the setup data and kept; no solve is run.
 *   update_lin_cost() / update_bounds(): replace q / l and-or u of every instance ([count x n] / [count x m]); the stored
 *             factors are applied to the new vectors, nothing is re-equilibrated.  update_bounds refuses l > u in any instance
 *             (return 1, "lower bound greater than upper bound") and then leaves the handle unchanged.
 *   update_matrices(): replace the values of P and-or A ([count x nnz], the pattern stays) and re-run the equilibration from
 *             scratch on the raw data with the current q, l, u; the stored (scaled) iterate is left as it is, as
 *             osqp_update_P_A leaves it.
 *   warm_start(): x [count x n] and-or y [count x m] in the caller's units, stored as x / D, c y / E, z = A x; x alone sets
 *             y = 0, y alone sets x = 0 and z = 0; switches the handle's warm_start setting on.
 *   resolve(): solves every instance.  With settings.warm_start = 1 (the default) a solve starts from the iterate the last
 *             one ended on (the first from zero; so does the solve after one that ended without a solution -- primal / dual
 *             infeasible, non-convex -- as osqp_solve resets the iterate then); with 0 every solve starts from zero.  rho is kept per
 *             instance: a solve that adapted it hands the adapted value on.  The constraint classes are derived from the
 *             current bounds at the start of each solve.  x_out [count x n], y_out [count x m] (NaN rows for instances
 *             without a solution), info_out [count x 6] doubles: iter, status_val, pri_res, dua_res, obj_val, rho_updates.
 *             With settings.polish = 1 a second launch then polishes every instance whose status is Solved, as osqp_solve
 *             does (settings.delta, settings.polish_refine_iter): an accepted polish overwrites the instance's x, y, pri_res,
 *             dua_res, obj_val and the stored iterate (the next warm solve starts from the polished point); a refused one
 *             and every instance that is not Solved keep exactly what the solve left.  With where = 0 the results are
 *             downloaded after the polish launch.
 *   polish_status(): status_out [count] doubles, status_polish of every instance from the handle's last resolve: 1 accepted,
 *             -1 refused (the acceptance rule of osqp_solve, or a failed factorisation), 0 not polished (not Solved, or
 *             polish off).  All 0 before the first resolve.
 *   update_polish(): the batch form of osqp_update_polish + osqp_update_polish_refine_iter: polish_new in {0, 1},
 *             polish_refine_iter_new >= 0, otherwise return 1 and the handle is unchanged.  A pattern whose polish working
 *             set (the n x n condensed KKT matrix as a packed triangle, the values of A and P, 5 n + 6 m doubles) exceeds
 *             160 KB of LDS is refused with return 1 and a message naming the bytes -- here and by setup() with polish = 1;
 *             polish is never skipped silently.
 *   adjoint(): derivatives of a scalar loss through the solutions of the last resolve.  dx [count x n], dy [count x m]: the
 *             gradients of the loss with respect to x and y as resolve returned them (NULL = zero; both NULL: return 1).
 *             Per instance, with L / U the rows active at the lower / upper bound, a = L u U and K = [P, Aa'; Aa, 0], one solve
 *             K [r_x; r_a] = [dx; dy restricted to a] (dy on inactive rows does not enter: the multiplier there is locally
 *             constant at 0), r_y = r_a scattered to length m, gives
 *               dq [count x n] = -r_x;  dl, du [count x m]: r_y,i on the rows of L (dl) / U (du), 0 elsewhere;
 *               dPx [count x nnz(P upper)], in the setup's pattern order: -r_x,i x_i for a stored diagonal entry (i, i),
 *                   -(r_x,i x_j + r_x,j x_i) for a stored entry (i, j), i < j (it stands for both halves of P);
 *               dAx [count x nnz(A)]: -(y_i r_x,j + r_y,i x_j) for entry (i, j);
 *               act_out [count x m] doubles: -1 lower, 1 upper, 0 inactive;  status_out [count] doubles.
 *             Any output may be NULL (not wanted); a y-sized or A-sized pointer is ignored when m = 0 or nnz(A) = 0.
 *             The active rows are those the polish step takes from the stored iterate (lower if z - l < -y, else upper if
 *             u - z < y, scaled space), and a row with l == u is always active and counts as lower: for such a row only
 *             dl + du is meaningful (the derivative with respect to moving both bounds together), and it is returned in dl.
 *             The solve is the polish solve with another right-hand side, in its own kernel launch: the condensed matrix
 *             regularised with settings.delta, a Cholesky factor, settings.polish_refine_iter refinement steps against the
 *             unregularised K (polish itself need not be on).  Where K is singular -- dependent active rows, more active
 *             rows than variables -- the derivative does not exist; the call does not detect this and returns the refined
 *             regularised answer.  status: 1 differentiated; 0 the instance had no solution at the last resolve (its
 *             gradient rows and its act_out row are zeros); -1 the Cholesky factor met a non-positive pivot (zeros).
 *             Refused with return 1 and a message: a handle that has not been resolved, or whose data or iterate changed
 *             since (any update_* or warm_start; update_polish does not count), and a pattern whose working set exceeds
 *             the polish LDS limit.  The call changes nothing on the handle: a resolve after it is bit-identical to one
 *             without it.
 *   adjoint_multi(): adjoint() for ncot >= 1 pairs (dx, dy) per instance in ONE launch.  Every array of the call but act_out
 *             and status_out is cotangent-major: dx [ncot x count x n], dy [ncot x count x m], and dq, dl, du, dPx, dAx
 *             [ncot x count x cols]; cotangent c of every array is a contiguous [count x cols] block.  act_out [count x m] and
 *             status_out [count] are written once per instance.  The matrix is assembled and factorised ONCE per instance
 *             and solved once per cotangent; nothing is carried from one cotangent to the next, so cotangent c of an ncot
 *             call has the bits of adjoint() with that pair, and ncot = 1 is adjoint().  An instance with status 0 or -1 has
 *             zeros in the rows of every cotangent.  ncot < 1 is refused with return 1 and a message; every other rule is
 *             adjoint()'s.  adjoint_multi_rows() is to it what adjoint_rows() is to adjoint(): [ncot x k x cols] arrays.
 *   jvp():    forward sensitivities (Jacobian-vector products) of the solutions of the last resolve: the transpose of
 *             adjoint().  A direction of the data is (tq [n], tl, tu [m], tPx [nnz(P upper)], tAx [nnz(A)]) per instance, in
 *             the setup's pattern order; tP is the symmetric matrix of tPx (a stored off-diagonal entry stands for both
 *             halves of P).  With the active rows a = L u U and K = [P, Aa'; Aa, 0] of adjoint(), one solve per direction
 *               K [tx; ty_a] = [-(tq + tP x + tA' y); (tb - tA x) restricted to a],   tb_i = tl_i on L, tu_i on U,
 *             gives tx_out (the tangent of x) and ty_out = ty_a scattered to length m, zero on the inactive rows.  On a row
 *             with l == u (always active, counts as lower) only tl is read -- the mirror of "returned in dl" of adjoint();
 *             a tangent of an inactive bound has no effect.  x, y are the values resolve returned.
 *             ndir >= 1 directions per call, direction-major: every tangent is [ndir x count x cols] and so are tx_out
 *             [ndir x count x n] and ty_out [ndir x count x m]; direction d of every array is a contiguous [count x cols]
 *             block.  act_out [count x m] and status_out [count], once per call, are those of adjoint().  The matrix is
 *             assembled and factorised ONCE per instance and solved once per direction (the polish solve: regularised with
 *             settings.delta, settings.polish_refine_iter refinement steps against the unregularised K); nothing is carried
 *             from one direction to the next, so direction d of an ndir-direction call has the bits of a one-direction call
 *             with that tangent, and a NULL tangent gives the bits of a tangent of zeros.
 *             A NULL tangent is zero and never read (all five NULL: return 1); tx_out or ty_out may be NULL (not wanted;
 *             both NULL: return 1), as may act_out and status_out.  With m = 0, tl / tu / tAx / ty_out / act_out are
 *             ignored, and a zero-width tPx or tAx is ignored.  status: 1 differentiated; 0 the instance had no solution at
 *             the last resolve (its rows of every direction and its act_out row are zeros); -1 non-positive pivot (zeros).
 *             Refused with return 1 and a message, without a launch and with the handle unchanged: ndir < 1, a handle that
 *             has not been resolved or whose data or iterate changed since (the rules and the message of adjoint(): every
 *             instance must be current, the first stale one is named; setting changes do not count), and a pattern whose
 *             working set exceeds the polish LDS limit.  Singular K: as adjoint().  The call only reads the handle: a
 *             resolve after it is bit-identical to one without it.
 *   certificates(): the directions that prove the infeasibilities of the handle's last resolve -- results.prim_inf_cert /
 *             dual_inf_cert of a single model.  Row i of prim_inf_cert_out [count x m], for an instance whose status is
 *             primal infeasible (or its inaccurate form), is the projected delta_y of the terminating check, multiplied
 *             element-wise by E when scaling is on and scaled_termination off, then divided by its infinity norm: its largest
 *             entry is exactly +-1.  Row i of dual_inf_cert_out [count x n] is the same with delta_x and D for the two dual
 *             infeasible statuses.  Every other row is NaN; before the first resolve all rows are.  Like polish_status they
 *             are results of the last resolve: update_* and warm_start leave them readable, the next resolve replaces them.
 *             Either pointer may be NULL (not wanted; both NULL: return 1); with m = 0 the first is ignored.  The call only
 *             copies: every resolve makes one extra small launch (k_batch_cert) after its ADMM launch, which normalises
 *             the directions that launch left in the records and puts the records back as they were -- the one-shot
 *             entries and the MPC handle make none and have no certificates.
 *   update_setting(): the batch form of osqp_update_<name>, by name: max_iter, eps_abs, eps_rel, eps_prim_inf, eps_dual_inf,
 *             time_limit, rho, alpha, delta, polish, polish_refine_iter, verbose, scaled_termination, check_termination,
 *             warm_start.  The value must pass the rule of the single-model function of that name, and an integer setting
 *             must be given an integral value; otherwise return 1 with a message naming the setting, and the handle is
 *             unchanged.  Any other name (sigma, scaling, adaptive_rho*, linsys_solver, ...) returns 1 with "<name> cannot
 *             be updated or is not recognized".  The value acts from the next resolve.  rho also replaces the stored rho of
 *             EVERY instance, adapted or not, as osqp_update_rho rebuilds rho_vec (the iterate stays); polish and
 *             polish_refine_iter go the way of update_polish, with its LDS refusal; time_limit and verbose are stored and
 *             have no effect (below).  No setting change makes the stored solution stale for adjoint(), and the certificates
 *             and polish_status of the last resolve stay as they are.
 *   *_rows(): update_lin_cost, update_bounds, update_matrices, warm_start and resolve for a SELECTION of the instances.
 *             rows [k]: k distinct instance numbers in [0, count), 1 <= k <= count, in any order; always a HOST pointer.  The
 *             array arguments and results are compact, [k x .]: row j belongs to instance rows[j].  A selected instance
 *             behaves exactly as under the whole-batch call of the same name, bit for bit (x, y, info, record, certificates,
 *             polish status).  An instance that is not selected is neither read nor written nor launched: its data, its
 *             record (D, E, c, rho, iterate), its certificate rows, its polish status and its info row stay as they were.
 *             update_bounds_rows compares a new bound with the stored other bound of the same instance when only one is
 *             given; update_matrices_rows re-equilibrates the selected instances only; resolve_rows launches k workgroups
 *             in its ADMM launch, in k_batch_cert and (polish = 1) in k_batch_polish; x_out [k x n], y_out [k x m],
 *             info_out [k x 6].  A bad selection -- k < 1, k > count, an entry out of range, a repeated entry (the message
 *             names it) -- returns 1 with a message and leaves the handle unchanged.
 *             Row i of the whole-batch polish_status(), certificates(), adjoint() and jvp() is of instance i's OWN last
 *             resolve, whole or selected (polish status 0 when polish was off at that resolve).  The whole-batch adjoint() and
 *             jvp() need every instance current: a *_rows update or warm start makes its rows stale, resolve_rows makes them
 *             current, and the refusal names the first stale instance.
 *   adjoint_rows() / jvp_rows() / polish_status_rows() / certificates_rows(): the four reading calls for a SELECTION, with
 *             rows and k as above.  Every array of the call is compact: dx, dy and the gradients [k x .], the tangents and
 *             tx_out / ty_out [ndir x k x cols] (direction d is a contiguous [k x cols] block), act_out [k x m], status_out
 *             [k], the certificates [k x m] / [k x n]; row j is of instance rows[j] and has the bits of row rows[j] of the
 *             whole-batch call.  adjoint_rows and jvp_rows launch k workgroups and need only the SELECTED instances
 *             current: the refusal names the first stale one in the order of rows, and nothing is launched.  Every other
 *             rule is the whole-batch call's (NULL arguments, m = 0, status values, the LDS limit; polish_status_rows gives
 *             zeros before the first resolve and after a whole resolve without polish; certificates_rows ignores the
 *             first pointer with m = 0 and returns 1 when no certificate was asked for).  A bad selection returns 1
 *             before anything else is looked at.  The calls only read the handle: a resolve after them is bit-identical
 *             to one without them.
 * where: 0 = the array arguments are host pointers, 1 = device pointers on the handle's device (no host hop: a controller
 * whose state estimate lives in HBM).  A NULL array means "keep" (update_*) / "none" (warm_start).  Every call blocks until
 * done.  Single rank.  The handle is freed by osqp_amd_batch_destroy; it is not interchangeable with the handle of
 * osqp_amd_batch_mpc_create: each family's calls return 1 with a message on the other's handle. */
c_int osqp_amd_batch_setup(osqp_amd_batch **out, c_int count, c_int n, c_int m,
                           const c_int *Pp, const c_int *Pi, const c_float *Px_all,
                           const c_int *Ap, const c_int *Ai, const c_float *Ax_all,
                           const c_float *q_all, const c_float *l_all, const c_float *u_all,
                           const OSQPSettings *settings, c_int device);
c_int osqp_amd_batch_update_lin_cost(osqp_amd_batch *batch, const c_float *q_all, c_int where);
c_int osqp_amd_batch_update_bounds(osqp_amd_batch *batch, const c_float *l_all, const c_float *u_all, c_int where);
c_int osqp_amd_batch_update_matrices(osqp_amd_batch *batch, const c_float *Px_all, const c_float *Ax_all, c_int where);
c_int osqp_amd_batch_warm_start(osqp_amd_batch *batch, const c_float *x_all, const c_float *y_all, c_int where);
c_int osqp_amd_batch_resolve(osqp_amd_batch *batch, c_float *x_out, c_float *y_out, c_float *info_out, c_int where);
c_int osqp_amd_batch_update_lin_cost_rows(osqp_amd_batch *batch, const c_int *rows, c_int k, const c_float *q_rows, c_int where);
c_int osqp_amd_batch_update_bounds_rows(osqp_amd_batch *batch, const c_int *rows, c_int k, const c_float *l_rows,
                                        const c_float *u_rows, c_int where);
c_int osqp_amd_batch_update_matrices_rows(osqp_amd_batch *batch, const c_int *rows, c_int k, const c_float *Px_rows,
                                          const c_float *Ax_rows, c_int where);
c_int osqp_amd_batch_warm_start_rows(osqp_amd_batch *batch, const c_int *rows, c_int k, const c_float *x_rows,
                                     const c_float *y_rows, c_int where);
c_int osqp_amd_batch_resolve_rows(osqp_amd_batch *batch, const c_int *rows, c_int k, c_float *x_out, c_float *y_out,
                                  c_float *info_out, c_int where);
c_int osqp_amd_batch_polish_status(osqp_amd_batch *batch, c_float *status_out, c_int where);
/* status_polish of the k selected instances: status_out [k] doubles, entry j of instance rows[j]. */
c_int osqp_amd_batch_polish_status_rows(osqp_amd_batch *batch, const c_int *rows, c_int k, c_float *status_out /* [k] */, c_int where);
c_int osqp_amd_batch_update_polish(osqp_amd_batch *batch, c_int polish_new, c_int polish_refine_iter_new);
c_int osqp_amd_batch_update_setting(osqp_amd_batch *batch, const char *name, c_float value);
c_int osqp_amd_batch_certificates(osqp_amd_batch *batch, c_float *prim_inf_cert_out /* [count x m] */,
                                  c_float *dual_inf_cert_out /* [count x n] */, c_int where);
/* The certificate rows of the k selected instances, gathered on the device: row j is row rows[j] of the whole call. */
c_int osqp_amd_batch_certificates_rows(osqp_amd_batch *batch, const c_int *rows, c_int k, c_float *prim_inf_cert_out /* [k x m] */,
                                       c_float *dual_inf_cert_out /* [k x n] */, c_int where);
c_int osqp_amd_batch_adjoint(osqp_amd_batch *batch, const c_float *dx, const c_float *dy,
                             c_float *dq, c_float *dl, c_float *du, c_float *dPx, c_float *dAx,
                             c_float *act_out, c_float *status_out, c_int where);
/* adjoint() of the k selected instances in a launch of k workgroups; all arrays [k x .]; only they must be current. */
c_int osqp_amd_batch_adjoint_rows(osqp_amd_batch *batch, const c_int *rows, c_int k, const c_float *dx, const c_float *dy,
                                  c_float *dq, c_float *dl, c_float *du, c_float *dPx, c_float *dAx,
                                  c_float *act_out, c_float *status_out, c_int where);
/* adjoint() / adjoint_rows() for ncot pairs (dx, dy) per instance in one launch: cotangent-major arrays [ncot x count x cols]
 * ([ncot x k x cols]); act_out and status_out once per instance. */
c_int osqp_amd_batch_adjoint_multi(osqp_amd_batch *batch, c_int ncot, const c_float *dx, const c_float *dy,
                                   c_float *dq, c_float *dl, c_float *du, c_float *dPx, c_float *dAx,
                                   c_float *act_out, c_float *status_out, c_int where);
c_int osqp_amd_batch_adjoint_multi_rows(osqp_amd_batch *batch, const c_int *rows, c_int k, c_int ncot, const c_float *dx, const c_float *dy,
                                        c_float *dq, c_float *dl, c_float *du, c_float *dPx, c_float *dAx,
                                        c_float *act_out, c_float *status_out, c_int where);
c_int osqp_amd_batch_jvp(osqp_amd_batch *batch, c_int ndir,
                         const c_float *tq, const c_float *tl, const c_float *tu, const c_float *tPx, const c_float *tAx,
                         c_float *tx_out, c_float *ty_out, c_float *act_out, c_float *status_out, c_int where);
/* jvp() of the k selected instances in a launch of k workgroups; direction-major arrays [ndir x k x cols]; only they must
 * be current. */
c_int osqp_amd_batch_jvp_rows(osqp_amd_batch *batch, const c_int *rows, c_int k, c_int ndir,
                              const c_float *tq, const c_float *tl, const c_float *tu, const c_float *tPx, const c_float *tAx,
                              c_float *tx_out, c_float *ty_out, c_float *act_out, c_float *status_out, c_int where);
/* Diagnostic, like osqp_amd_batch_last_kernel: how many polish launches this process has made so far.  A resolve with
 * polish = 0 makes none -- its launch sequence is the one of a library without the polish kernel. */
c_int osqp_amd_batch_polish_launches(void);
/* The same for the adjoint kernel: one launch per osqp_amd_batch_adjoint / _adjoint_rows / _adjoint_multi /
 * _adjoint_multi_rows that passed its checks, whatever ncot, none otherwise. */
c_int osqp_amd_batch_adjoint_launches(void);
/* The same for the sensitivity kernel: one launch per osqp_amd_batch_jvp / _jvp_rows that passed its checks, whatever ndir, none
 * otherwise. */
c_int osqp_amd_batch_jvp_launches(void);
/* The same for the certificate kernel: one launch per osqp_amd_batch_resolve / _resolve_rows, none by osqp_amd_batch_certificates or by the
 * one-shot entries. */
c_int osqp_amd_batch_cert_launches(void);
/* Primal objective, dual objective and duality gap of every instance of a resident handle (definitions: "Dual objective,
 * duality gap and a gap stopping rule" below): out [count x 3] doubles (host or device by `where`), row
 * i = prim_obj, dual_obj, gap of the pair (x, y) instance i's last resolve returned (the polished pair where polish was
 * accepted), in the caller's units; a NaN row where that resolve left no solution (infeasible, non-convex).  A launch of
 * a kernel of its own (one workgroup per instance, sums in a fixed order) that reads the records, the raw data and the
 * pattern: the handle is only read, a resolve after the call has the bits of one without it.  Every instance must be
 * current (resolved after its last update or warm start), as for osqp_amd_batch_adjoint: otherwise 1, and the message
 * names the first that is not.  _rows: the k selected instances, out [k x 3], row j of instance rows[j], equal to row
 * rows[j] of the whole call; only they must be current.  Returns 0; 1 NULL or foreign handle, NULL out, a bad selection, a
 * stale instance.
 * Out of scope: the one-shot entries (osqp_amd_batch_solve, _solve_generated) and osqp_amd_batch_mpc_*: they return x and
 * y, from which the caller can form the three numbers. */
c_int osqp_amd_batch_duality(osqp_amd_batch *batch, c_float *out /* [count x 3] */, c_int where);
c_int osqp_amd_batch_duality_rows(osqp_amd_batch *batch, const c_int *rows, c_int k, c_float *out /* [k x 3] */, c_int where);
/* The gap as a stopping rule of the resident batch (the rule of osqp_amd_duality_gap_check below, inside
 * the batched solve kernels).  on = 1: from the next osqp_amd_batch_resolve / _resolve_rows an instance ends Solved
 * (Solved_inaccurate in the approximate pass at the iteration limit, at 10 eps) only where, next to the two residual tests,
 * |gap| < eps_abs + eps_rel max(|x'Px|, |q'x|, |SC|) holds, in the units of the residual tests (the caller's unless
 * scaled_termination); a NaN fails it.  The test is evaluated only at checks where both residual tests hold; a check that
 * it alone refuses goes on iterating (the infeasibility tests did not run at that check; adaptive rho proceeds as at any
 * other) and adds one to the instance's refusal count.  Instances whose gap holds where their residuals do stop where they
 * stopped before, with the same bits.  on = 0, the default: the solve of a handle that never had the rule.  The call drops
 * nothing -- iterate, rho, which instances are current, certificates and polish status stay -- and sets every refusal count
 * to zero.  Polish, certificates, adjoint, JVP and osqp_amd_batch_duality work on whatever point a solve stopped at.
 * osqp_amd_batch_gap_refusals: out [count] doubles (host or device by `where`), out[i] = the checks of instance i's own last
 * resolve that the gap test alone refused; zeros while the rule is off.  _rows: out [k], out[j] of instance rows[j].
 * The one-shot entries (osqp_amd_batch_solve, _solve_generated) and osqp_amd_batch_mpc_* run without the rule.
 * Return 0; 1 NULL or foreign (non-resident) handle, NULL out, a bad selection. */
c_int osqp_amd_batch_duality_gap_check(osqp_amd_batch *batch, c_int on);

/* Polish, adjoint and JVP on a resident handle with 128 < n <= 256: an opt-in switch PER HANDLE, 0
 * after setup; returns the previous value, or -1 with the reason in osqp_amd_last_error for a NULL handle, a handle that
 * osqp_amd_batch_setup did not create, or a handle with n <= 128.  While it is 1 the three kernels run forms that keep the
 * Cholesky factor of M in the instance's n x n block of the handle's global scratch (blocked factorisation, panels of
 * out[2] columns in LDS) instead of in LDS; everything else they do -- ncot cotangents, ndir directions, *_rows, host and
 * device forms, statuses, acceptance rule -- is what they do for n <= 128.  The shape is checked against the LDS need of that
 * layout wherever polish is asked for and at every adjoint / JVP call, before anything is launched or written ("instance too
 * large to polish ... (needs N bytes of LDS ...").  The call launches nothing and touches nothing on the device.  To polish:
 * set up with polish = 0, switch on, osqp_amd_batch_update_polish(handle, 1, ...).  Switching off puts the refusals back and
 * sets the handle's polish to 0. */
c_int osqp_amd_batch_large_factor(osqp_amd_batch *batch, c_int on);
/* What those forms need for a shape, on the host alone (the function their launchers ask): out[0] = bytes of LDS per workgroup,
 * out[1] = bytes of scratch per launched instance (8 n^2), out[2] = NB, the columns per panel.  Returns 0 when the shape is
 * accepted; otherwise 1 with the reason in osqp_amd_last_error (n <= 128, n > 256, too much LDS) and out untouched. */
c_int osqp_amd_batch_large_factor_plan(c_int n, c_int m, c_int nnzA, c_int nnzF, c_int *out);
c_int osqp_amd_batch_gap_refusals(osqp_amd_batch *batch, c_float *out /* [count] */, c_int where);
c_int osqp_amd_batch_gap_refusals_rows(osqp_amd_batch *batch, const c_int *rows, c_int k, c_float *out /* [k] */, c_int where);

/* Device memory for callers without an allocator of their own (the packed result array above): plain hipMalloc / hipFree /
 * hipMemcpy on `device`.  copy kind: 0 device -> host, 1 host -> device, 2 device -> device; blocking. */
void *osqp_amd_device_alloc(c_int bytes, c_int device);
c_int osqp_amd_device_free(void *ptr, c_int device);
c_int osqp_amd_device_copy(void *dst, const void *src, c_int bytes, c_int kind, c_int device);

/* Differences between the batched path and osqp_setup / osqp_solve: instances share one sparsity pattern, n <= 128
 * (n <= 256 while osqp_amd_batch_large is on),
 * fewer than 65536 rows and non-zeros, everything must fit 160 KB of LDS; `adaptive_rho_interval` = 0 (automatic) means
 * every 100 iterations (there is no per-instance clock); `time_limit`, `verbose` and `linsys_solver` are ignored (the
 * reduced KKT system is factorised on chip); data and settings are validated as by osqp_setup (1 = data, 2 = settings).
 * The one-shot entries (osqp_amd_batch_solve, _solve_generated, _mpc_create / _mpc_solve) also ignore `warm_start` and
 * `polish` (with `polish_refine_iter` and `delta`): they equilibrate, start from zero every time and return the ADMM
 * iterate.  The resident handle (osqp_amd_batch_setup) honours all of them: it keeps scaling, iterate and rho between
 * solves and polishes the Solved instances after the ADMM launch when `polish` = 1, as described above; the per-instance
 * status_polish is read with osqp_amd_batch_polish_status (the six info columns do not change).  Only the resident handle
 * returns infeasibility certificates (osqp_amd_batch_certificates) and takes settings updates after setup
 * (osqp_amd_batch_update_setting: the names of osqp_update_*; `time_limit` and `verbose` are stored and ignored as above). */

/* ---- Adjoint derivatives of the solution of a single model (upstream OSQP 1.0:
 * adjoint_derivative_compute / _get_mat / _get_vec) ----
 *
 * osqp_amd_adjoint differentiates a scalar loss through the solution the last osqp_solve left in `work`: from ncot
 * pairs g_x = dloss/dx (dx, [ncot x n]) and g_y = dloss/dy (dy, [ncot x m]; either may be NULL = 0) it returns per pair
 * dloss/dq (dq [ncot x n]), dloss/dl and dloss/du (dl, du [ncot x m]) and the gradients of the stored values of P and A
 * (dPx [ncot x nnz(triu P)], dAx [ncot x nnz(A)]) indexed by the caller's nnz index -- the index space of osqp_update_P /
 * _A, the setup-time order also where the columns of A came unsorted.  Any of the five may be NULL: not wanted, not
 * computed.  act ([m], or NULL) receives the active set: -1 lower, 0 inactive, 1 upper.  All pointers are host pointers.
 *
 *   With L / U the rows active at the lower / upper bound, a = L u U and K = [P, Aa'; Aa, 0], one solve
 *   K [r_x; r_a] = [g_x; (g_y)_a] per pair gives, with r_y = r_a scattered to length m (0 on inactive rows),
 *     dq = -r_x;   dl_i = r_y,i on L, du_i = r_y,i on U, 0 elsewhere;
 *     dPx(i, i) = -r_x,i x_i;   dPx(i, j) = -(r_x,i x_j + r_x,j x_i) for i < j (the stored entry stands for both halves);
 *     dAx(i, j) = -(y_i r_x,j + r_y,i x_j).
 *   Active rows: polish's rule on the workspace's scaled (z, y, l, u) -- z - l < -y lower, u - z < y upper -- and a row with
 *   l == u is always active and counts as lower.  The solve runs on the scaled data through the factorisation of
 *   [P + delta I, Aa'; Aa, -delta I], followed by `polish_refine_iter` refinement steps against the unregularised matrix
 *   (0 steps: the regularised answer, made accurate by one step against the REGULARISED matrix -- the factorisation does not
 *   pivot and its solve alone is good to ~1e-8).  A singular K is not detected: the refined regularised answer is returned.
 *
 *   The factor is KEPT: the first call after a solve classifies the rows, analyses and factorises (the work
 *   of a polish; measured: DESIGN.md section 14); later calls on the same solution reuse it, ncot pairs in one call are ncot solve-and-refine passes on it, and
 *   pair c of a call has the bits of a call with that pair alone.  osqp_solve, every osqp_update_* (settings included: delta
 *   is inside the matrix), every osqp_warm_start*, osqp_amd_iterate, osqp_cleanup and osqp_amd_adjoint_release drop it; the
 *   factor is as large as a polish's, so a caller who is done with a solution releases it.  The call changes nothing else:
 *   not info, not the solution, not the iterate, rho or the ADMM factor -- solve, adjoint, solve gives the bits and the
 *   iteration count of solve, solve.
 *
 *   Returns 0, or non-zero with the reason in osqp_amd_last_error and no output written: 7 NULL workspace; 1 ncot < 1, a
 *   gradient wanted with dx and dy both NULL, nothing wanted at all, no current solution (no osqp_solve yet, or a data
 *   update, warm start or osqp_amd_iterate after the last one: call osqp_solve), the last solve did not end with status
 *   OSQP_SOLVED (solved inaccurate is refused too); 6 a compact or a row-sharded workspace (no CSR arrays, no reduced KKT
 *   matrix) and a reduced factor that is too large -- under the default method; osqp_amd_derivative_method(work, 1, 0, 0)
 *   serves the compact workspace and the factor that does not fit with the iterative adjoint on the operator of the indirect
 *   back-end (below), a row-sharded workspace stays refused --; 4 a failed numeric factorisation, or an iterative solve that
 *   did not converge. */
c_int osqp_amd_adjoint(OSQPWorkspace *work, c_int ncot,
                       const c_float *dx /* [ncot x n] or NULL = 0 */, const c_float *dy /* [ncot x m] or NULL = 0 */,
                       c_float *dq /* [ncot x n] */, c_float *dl /* [ncot x m] */, c_float *du /* [ncot x m] */,
                       c_float *dPx /* [ncot x nnz(triu P)] */, c_float *dAx /* [ncot x nnz(A)] */,
                       c_float *act /* [m] or NULL */);
/* ---- Forward sensitivities of the solution of a single model ----
 *
 * osqp_amd_jvp pushes ndir directions of the data forward to the solution the last osqp_solve left in `work`: a direction is
 * (tq [n], tl, tu [m], tPx [nnz(triu P)], tAx [nnz(A)]), the matrix tangents as value arrays in the caller's nnz order (the
 * index space of osqp_update_P / _A, also where the columns of A came unsorted); the arrays are direction-major
 * ([ndir x cols]) and any of the five may be NULL = zero.  tx [ndir x n] and ty [ndir x m] receive dx/dtheta . t and
 * dy/dtheta . t; either may be NULL (not wanted); act as for osqp_amd_adjoint.  All pointers are host pointers.
 *
 *   With a = L u U and K = [P, Aa'; Aa, 0] of osqp_amd_adjoint, one solve per direction
 *     K [tx; ty_a] = [-(tq + tP x + tA' y); (tb - tA x)_a],   tb_i = tl_i on L, tu_i on U,   ty = 0 off a,
 *   tP the symmetric matrix of the stored upper triangle (a diagonal entry counts once), x and y the solution.  On a row with
 *   l == u (always active, counts as lower) only tl is read.  The solve is osqp_amd_adjoint's: the same kept factor, the same
 *   refinement (and the same rule at polish_refine_iter = 0).  Direction d of a call has the bits of a call with that
 *   direction alone, and a NULL tangent those of a tangent of zeros.
 *
 *   The kept state is osqp_amd_adjoint's, created by whichever of the two is called first after a solve and used by both: a
 *   jvp after an adjoint on the same solution (or the other way round) builds nothing; what drops the factor is unchanged,
 *   and so is "the call changes nothing else".  The first call with tPx or tAx adds two maps of 4 bytes per stored entry of
 *   the full P and of A to the workspace (until osqp_cleanup).
 *
 *   Returns 0, or non-zero with the reason in osqp_amd_last_error and no output written, with osqp_amd_adjoint's codes: 7
 *   NULL workspace; 1 ndir < 1, tx or ty wanted with all five tangents NULL, nothing wanted at all, no current solution, a
 *   status other than OSQP_SOLVED; 6 a compact or a row-sharded workspace, a reduced factor that is too large (the default
 *   method; osqp_amd_derivative_method(work, 1, 0, 0) serves the first and the last iteratively, with tq, tl, tu on a compact
 *   workspace: tPx / tAx are refused with 6 there, their products on the sliced copy are not built); 4 a failed numeric
 *   factorisation, or an iterative solve that did not converge. */
c_int osqp_amd_jvp(OSQPWorkspace *work, c_int ndir,
                   const c_float *tq /* [ndir x n] or NULL = 0 */, const c_float *tl /* [ndir x m] */, const c_float *tu /* [ndir x m] */,
                   const c_float *tPx /* [ndir x nnz(triu P)] */, const c_float *tAx /* [ndir x nnz(A)] */,
                   c_float *tx /* [ndir x n] or NULL */, c_float *ty /* [ndir x m] or NULL */, c_float *act /* [m] or NULL */);
/* Drop the kept factor now.  0, also when none is kept; 7 on a NULL workspace. */
c_int osqp_amd_adjoint_release(OSQPWorkspace *work);
/* Entries 0 and 1 count the builds and the KKT solves of osqp_amd_adjoint and of osqp_amd_jvp together (one factor serves both).
 * Fills out[0..count): 0 factor builds so far, 1 KKT solves so far (1 + polish_refine_iter per pair or direction; 2 at polish_refine_iter = 0), 2, 3 n_low and
 * n_upp of the kept factor (0 if none), 4 1 if a factor is kept, 5 device bytes the kept factor holds with its index
 * arrays and scratch.  Like osqp_amd_get_stats it returns the number of entries written (at most
 * OSQP_AMD_ADJOINT_STATS_COUNT), 0 on a NULL argument.  Under osqp_amd_adjoint_retain(work, 1) a state that is stale
 * (held over from the previous solution, awaiting its check) is still a kept factor: entry 4 is 1 and entries 2, 3 and 5
 * are those of what is held. */
#define OSQP_AMD_ADJOINT_STATS_COUNT 6
c_int osqp_amd_adjoint_stats(const OSQPWorkspace *work, c_float *out, c_int count);

/* ---- Keep the derivative factor while the active set holds ----
 *
 * By default the kept factor belongs to ONE solution.  osqp_amd_adjoint_retain(work, 1) lets it outlive the solution, for
 * the loop update - solve - differentiate: the calls that move the model on -- osqp_solve, osqp_update_lin_cost /
 * _bounds / _lower_bound / _upper_bound / _P / _A / _P_A, osqp_warm_start*, osqp_amd_iterate, osqp_amd_time_kernel id 5 and
 * the _dev forms of these -- no longer drop a kept FACTOR, they mark it stale.  osqp_update_P / _A / _P_A and
 * osqp_amd_update_values_dev also mark its values dirty, and they do so also when they return non-zero.  The first
 * osqp_amd_adjoint / _jvp (or _dev form) that passes its checks on the next solution classifies the rows on the device
 * against the kept side of every row (one pass over z, y, l, u and the kept side; the host reads one word, no m-vector comes
 * to the host) and then
 *   - no row changed side, values clean: the factor is reused as it is; only the caller-unit solution is refreshed;
 *   - no row changed side, values dirty: the kept structure is factorised numerically again (no classification on the
 *     host, no analysis); a factorisation that returns non-zero (a failed probe of the dense top block included) falls
 *     back to a full build;
 *   - otherwise: the state is dropped and built as by default, with the default's refusals and codes.
 * The results have the bits of the default life cycle: the same kernels on the same values in the same structure.
 *
 *   What still drops the state, stale or not: every settings update (delta is inside the matrix), osqp_amd_derivative_method,
 *   osqp_amd_adjoint_release, osqp_cleanup.  The iterative state of osqp_amd_derivative_method is never retained (it is cheap
 *   to build).  A derivative call that is refused for want of a current solution, or after a solve that did not end
 *   OSQP_SOLVED, is refused exactly as by default and leaves a stale state where it is.  mode 0 (the default) drops a stale
 *   state at once and leaves a current one alone.  With the mode never set nothing changes: not a launch, not a bit.
 *
 *   Returns 0; 1 on another mode; 7 on a NULL workspace. */
c_int osqp_amd_adjoint_retain(OSQPWorkspace *work, c_int mode);
/* Fills out[0..count): 0 the mode, 1 checks made (derivative calls that found a stale kept factor and classified the new
 * solution against it), 2 reused as it was, 3 reused after a numeric refactorisation, 4 rebuilt because the active set
 * differed, 5 rebuilt because the numeric refactorisation of the kept structure returned non-zero, 6 rows whose side
 * differed at the last check, 7 1 while the kept state is stale (awaiting a check; osqp_amd_adjoint_stats reports it as
 * kept, with its bytes, n_low and n_upp).  Full builds stay in entry 0 of osqp_amd_adjoint_stats.  Returns the number of
 * entries written (at most OSQP_AMD_ADJOINT_RETAIN_STATS_COUNT), 0 on a NULL argument. */
#define OSQP_AMD_ADJOINT_RETAIN_STATS_COUNT 8
c_int osqp_amd_adjoint_retain_stats(const OSQPWorkspace *work, c_float *out, c_int count);

/* ---- The KKT solve behind osqp_amd_adjoint / _jvp and their _dev forms: factor or iteration ----
 *
 * osqp_amd_derivative_method chooses per workspace.  method 0, direct (the default): the kept factor, with the refusals
 * above.  1, auto: the kept factor wherever method 0 builds one; the iterative form on a compact workspace and where the
 * reduced factor is too large.  2, iterative: always the iterative form.  The iterative form needs the indirect back-end
 * (linsys_solver = pcg) on one device, with OSQP_AMD_PCG_ASYNC and OSQP_AMD_PCG_SR at their defaults: method 2 on another
 * workspace returns 6 and says what is missing (a row-sharded workspace stays refused under every method).
 *
 *   The iterative form solves K [s_x; s_a] = [b1; b2] on the scaled data as polish does on such a workspace: conjugate
 *   gradients on (P + d I + Aa' Aa / d) with d = max(delta, 1e-3), relative tolerance 1e-6, start vector zero, the
 *   multipliers s_a = (Aa s_x - r2) / d, and outer steps on the residual of the UNREGULARISED system until it has dropped by
 *   rel_drop (0: 1e-10), after more than polish_refine_iter and at most max_outer (0: 40) steps.  Its kept state holds no
 *   factor: the side of every row (classified on the device), the caller-unit solution and scratch of n + m doubles; it is
 *   created by the first adjoint or jvp after a solve, used by both, dropped by what drops the factor, and reported by
 *   osqp_amd_adjoint_stats (entries 0 and 1 then count builds and outer steps).  Pair c (direction d) of a call has the bits
 *   of a call with it alone, a NULL tangent those of zeros, the device form those of the host form.  "The call changes
 *   nothing else" holds: rho, sigma, the preconditioner, the CG settings, start vectors, carried products and the iteration
 *   total of the indirect back-end are saved and put back, also when a launch throws; the derivative's CG iterations are
 *   counted below and not in osqp_amd_get_stats.  On a compact workspace dPx / dAx are computed on the sliced copy (scratch
 *   of one double per stored slot of one matrix for the length of the call) and the matrix tangents tPx / tAx are refused.
 *
 *   A solve that does not reach rel_drop in max_outer steps (or whose CG refuses) makes the call return 4 with the reached
 *   rn / first_norm in osqp_amd_last_error.  Host form: nothing has been delivered.  Device form: the outputs of earlier
 *   pairs / directions of the same call may already have been written.
 *
 *   The call drops the derivative state the current solution keeps (as osqp_amd_adjoint_release).  Returns 0; 7 NULL
 *   workspace; 1 method outside 0..2, max_outer < 0, rel_drop outside [0, 1); 6 as above. */
c_int osqp_amd_derivative_method(OSQPWorkspace *work, c_int method, c_int max_outer, c_float rel_drop);
/* Fills out[0..count): 0 iterative states built so far, 1 outer steps so far, 2 CG iterations so far (the derivative's own),
 * 3 outer steps of the last pass, 4 rn / first_norm of the last pass, 5 1 if the kept state is the iterative one, 6 device
 * bytes it holds.  Returns the number of entries written (at most OSQP_AMD_DERIVATIVE_ITER_STATS_COUNT), 0 on a NULL argument. */
#define OSQP_AMD_DERIVATIVE_ITER_STATS_COUNT 7
c_int osqp_amd_derivative_iter_stats(const OSQPWorkspace *work, c_float *out, c_int count);

/* ---- Device-pointer forms of a single model's life cycle ----
 *
 * The calls above take host arrays.  Each call below is the twin of one of them with every array argument a DEVICE pointer
 * on the workspace's device (fp64, contiguous): update and warm start from HBM, read the solution into HBM, differentiate
 * HBM to HBM.  Nothing passes through the host but return codes and, for a bounds update, one flag word.
 *
 *   Bit contract.  A device-form call leaves the workspace in exactly the state its host twin leaves it in for the same
 *   numbers -- data, iterate, info reset, rho vector, the dropped kept factor -- and writes the numbers the twin would have
 *   returned, bit for bit: it runs the twin's kernels in the twin's order on the same operands, and only the upload is
 *   replaced by a device-to-device copy (or the array is read where it lies).  The forms mix freely on one workspace.
 *
 *   Stream rule (as for `where = 1` of the resident batch).  The library runs on its own stream and blocks until it is done:
 *   the caller must have finished producing the inputs before the call (synchronise the producing stream), and may read the
 *   outputs as soon as the call returns.
 *
 *   Every call returns 7 on a NULL workspace and 6, with a message, on a row-sharded workspace (a rank holds a row block).
 *   A compact workspace is served by the four life-cycle calls as by their host twins; osqp_amd_adjoint_dev / _jvp_dev
 *   refuse it with the host twins' code 6 and a message that says "compact".
 *
 * osqp_amd_update_vectors_dev: osqp_update_lin_cost (q) followed by osqp_update_bounds / _lower_bound / _upper_bound (l, u;
 *   NULL = keep).  The rule on the bounds is theirs -- any l_i > u_i, a new l against the STORED u where only l is given and
 *   the reverse: return 1, nothing changed, q included -- and it is decided on the device, by a kernel that reduces the
 *   comparison to one word.  The workspace's host copy of the raw bounds stays truthful across the two forms: a host-form
 *   one-sided update after a device-form update validates against the device-given bound, and the reverse.  A lower bound below
 *   -OSQP_INFTY and an upper bound above OSQP_INFTY are stored as -OSQP_INFTY / OSQP_INFTY (what the wrappers of the host
 *   forms do on the host before the call is part of this call, as in the resident batch); within that range the numbers are
 *   taken as given.
 * osqp_amd_update_values_dev: osqp_update_P / _A / _P_A with full value arrays in the caller's nnz order (NULL = keep; a
 *   call that gives indices stays with the host forms).  Where the columns of A came unsorted at setup the values are
 *   permuted on the device.  Returns what the host form returns on a failed refactorisation or an indefinite P.
 * osqp_amd_warm_start_dev: osqp_warm_start (both given), osqp_warm_start_x (y NULL: the stored y is zeroed) or
 *   osqp_warm_start_y (x NULL).
 *   These three end the solution's being current and drop the factor osqp_amd_adjoint keeps, as their twins do; all NULL is
 *   a call that does nothing and returns 0.
 * osqp_amd_solution_dev: x = D x~ [n] and y = E y~ / c [m] of the solution of the last osqp_solve with the operations that
 *   fill solution->x / ->y (either may be NULL); NaN where that solve ended without a solution (infeasible, non-convex), as
 *   the host mirrors are filled.  Returns 1 before any osqp_solve has run, and when an update or a warm start since the
 *   last one has ended the solution's being current (the iterate is then no longer that solution).  Changes nothing.
 * osqp_amd_adjoint_dev / osqp_amd_jvp_dev: the arguments, the mathematics, the kept factor, the counters and the refusals of
 *   osqp_amd_adjoint / osqp_amd_jvp; cotangents and tangents are read in place, the output kernels write the caller's arrays
 *   (no staging array, no download) and act [m] is a copy of the kept array of doubles.  A device-form call after a
 *   host-form call on one solution builds nothing, and the reverse; osqp_amd_adjoint_stats counts both forms together.
 *   Every refusal (7, 1, 6 compact or too large, 4) is decided before the first kernel that writes to a caller's array: a
 *   refused call has written nothing.  The one exception is an internal error: when a wait inside the one-launch
 *   supernodal solve times out the passes run again by levels and overwrite the outputs; a second fault (code 6) may leave
 *   partial output behind.
 * osqp_amd_device_form_calls: out[0..count) (a HOST array) = the device-form calls that returned 0 on this workspace so
 *   far: 0 updates of vectors, 1 updates of values, 2 warm starts, 3 solution reads, 4 adjoints, 5 jvps.  Returns the number
 *   of entries written (at most OSQP_AMD_DEVICE_FORM_COUNT), 0 on a NULL argument. */
c_int osqp_amd_update_vectors_dev(OSQPWorkspace *work, const c_float *q /* [n] or NULL */, const c_float *l /* [m] or NULL */,
                                  const c_float *u /* [m] or NULL */);
c_int osqp_amd_update_values_dev(OSQPWorkspace *work, const c_float *Px /* [nnz(triu P)] or NULL */, const c_float *Ax /* [nnz(A)] or NULL */);
c_int osqp_amd_warm_start_dev(OSQPWorkspace *work, const c_float *x /* [n] or NULL */, const c_float *y /* [m] or NULL */);
c_int osqp_amd_solution_dev(OSQPWorkspace *work, c_float *x_out /* [n] or NULL */, c_float *y_out /* [m] or NULL */);
c_int osqp_amd_adjoint_dev(OSQPWorkspace *work, c_int ncot,
                           const c_float *dx /* [ncot x n] or NULL = 0 */, const c_float *dy /* [ncot x m] or NULL = 0 */,
                           c_float *dq /* [ncot x n] */, c_float *dl /* [ncot x m] */, c_float *du /* [ncot x m] */,
                           c_float *dPx /* [ncot x nnz(triu P)] */, c_float *dAx /* [ncot x nnz(A)] */,
                           c_float *act /* [m] or NULL */);
c_int osqp_amd_jvp_dev(OSQPWorkspace *work, c_int ndir,
                       const c_float *tq /* [ndir x n] or NULL = 0 */, const c_float *tl /* [ndir x m] */, const c_float *tu /* [ndir x m] */,
                       const c_float *tPx /* [ndir x nnz(triu P)] */, const c_float *tAx /* [ndir x nnz(A)] */,
                       c_float *tx /* [ndir x n] or NULL */, c_float *ty /* [ndir x m] or NULL */, c_float *act /* [m] or NULL */);
#define OSQP_AMD_DEVICE_FORM_COUNT 6
c_int osqp_amd_device_form_calls(const OSQPWorkspace *work, c_float *out, c_int count);

/* ---- Dual objective, duality gap and a gap stopping rule (after OSQP 1.0's check_dualgap) ----
 *
 * For min 1/2 x'Px + q'x s.t. l <= Ax <= u and a pair (x, y): yh is y projected onto the polar of the recession cone of
 * [l, u] (0 where both bounds are infinite, min(y, 0) where only u is, max(y, 0) where only l is, y otherwise; "infinite"
 * is the test of the primal-infeasibility check on the scaled bound; y itself is not modified),
 *   SC       = sum_i u_i max(yh_i, 0) + l_i min(yh_i, 0)     (an infinite bound adds 0; 0 when m = 0)
 *   prim_obj = 1/2 x'Px + q'x        dual_obj = -1/2 x'Px - SC        gap = x'Px + q'x + SC = prim_obj - dual_obj
 *   eps_gap  = eps_abs + eps_rel max(|x'Px|, |q'x|, |SC|)              rule: |gap| < eps_gap.
 *
 * osqp_amd_duality_gap_check(work, on): on = 1 adds the rule to the termination test of every later osqp_solve: Solved and
 *   Solved inaccurate (there with 10 eps, as for the residuals) then need the primal-residual, the dual-residual and the gap
 *   test to hold.  The gap and the three magnitudes are taken in the units of the residual tests: the caller's with
 *   scaling && !scaled_termination, the scaled problem's otherwise.  The infeasibility tests, Non_convex, adaptive rho and
 *   the tolerance rule of the indirect back-end stay as they are.  With the rule on every residual evaluation makes one more
 *   pass over y, l, u, and SC comes back in the read-back of the residual norms; off (the default) a solve launches exactly
 *   what it launched before.  Callable any time after setup; it does not move the iterate, rho, the ADMM factor or a kept
 *   derivative factor.  Returns 0; 7 NULL workspace; 1 `on` other than 0 or 1; 6 row-sharded workspace.
 * osqp_amd_duality(work, out, count) fills out[0..min(count, OSQP_AMD_DUALITY_COUNT)), caller's units:
 *   0 prim_obj, 1 dual_obj, 2 gap -- of the (x, y) the workspace holds: what the last osqp_solve returned (the polished pair
 *     when polish was accepted, the final iterate at Max_iter / Time_limit), or the current iterate after osqp_amd_iterate.
 *     Computed by the call, rule on or off: one product with P, two dots, the support pass, in scratch of its own.  Where
 *     the status carries no solution (infeasible, non-convex) 1 and 2 are NaN and 0 is info->obj_val.
 *   3 eps_gap of the last termination check the rule took part in (units of that check; NaN if there was none),
 *   4 1 if the rule is on, 5 checks so far at which both residual tests held and the gap alone refused.
 *   The call changes nothing: solve, duality, solve has the bits and counts of solve, solve.  Returns 0; 7 NULL workspace;
 *   1 before any osqp_solve / osqp_amd_iterate or NULL out; 6 row-sharded workspace.
 * Both serve the direct and the indirect back-end, compact workspaces included. */
#define OSQP_AMD_DUALITY_COUNT 6
c_int osqp_amd_duality_gap_check(OSQPWorkspace *work, c_int on);
c_int osqp_amd_duality(OSQPWorkspace *work, c_float *out, c_int count);

/* ---- The shared batch: ONE MODEL, MANY RIGHT-HAND SIDES on a shared KKT inverse --------------------
 * A shared batch is one model (P, A, base vectors q0, l0, u0, settings) and `count` instances that differ in q, l and u
 * only: MPC of one plant from many states, scenario trees, a QP layer with fixed matrices.  Instance i is, by definition,
 *   osqp_setup(P, q0, A, l0, u0, settings); osqp_update_lin_cost(q_i); osqp_update_bounds(l_i, u_i); osqp_solve
 * on a fresh model, and later updates and re-solves act on that same model.  Three rules make one inverse serve all:
 *   scaling  D, E and c come from setup (P, A, q0) and are not recomputed on vector updates, as in libosqp;
 *   rho      settings->adaptive_rho must be 0 (setup returns 2 with a message otherwise); rho is settings->rho and changes
 *            through update_setting("rho") at the cost of one re-factorisation;
 *   kinds    every row of every instance must have the kind it has under (l0, u0) on the SCALED bounds: loose where
 *            l < -OSQP_INFTY * 1e-4 and u > OSQP_INFTY * 1e-4, an equality where u - l < 1e-4, an inequality otherwise (the
 *            rule osqp_update_bounds re-derives rho by).  An update that breaks this, or has l > u, is refused before
 *            anything is written; the message names the first offending instance and row.
 * plan()     host only: out[0] = T, the instances per workgroup, chosen from the shape alone (never from count); out[1] the LDS
 *            bytes of a workgroup; out[2] the bytes of the model block (scaling, scaled values, the padded inverse); out[3] the
 *            bytes of device state per instance.  nnzF counts the stored entries of the full symmetric P.  n <= 256; a shape
 *            whose layout exceeds 160 KB of LDS is refused ("needs N bytes of LDS").
 * setup()    one scaling and one inversion (k_shared_factor, one workgroup); every instance then holds (q0, l0, u0) and a zero
 *            iterate.  A reduced KKT matrix that is not positive definite ends setup with the OSQP_NON_CVX message.
 * update_lin_cost() / update_bounds()  q_all [count x n]; l_all, u_all [count x m], both given.
 * warm_start()  x_all [count x n] and / or y_all [count x m] in the caller's units, NULL = zero; sets warm_start = 1.
 * resolve()  ONE launch of k_batch_solve_shared: T instances per workgroup, the dense step on the fp64 matrix cores.  x_out
 *            [count x n], y_out [count x m], info_out [count x 6] (iter, status_val, pri_res, dua_res, obj_val, 0): the columns
 *            of the resident batch.  An instance stops at ITS OWN check and reports its own iteration count; its bits do not
 *            depend on count, on its position or on the other instances.  Instances without a solution get NaN rows and
 *            restart from zero.  With warm_start = 1 (the default) a resolve starts from the iterate the last one left.
 *            osqp_amd_batch_last_kernel reports -3 afterwards; osqp_amd_shared_batch_launches counts these launches.
 * update_setting()  max_iter, eps_abs, eps_rel, eps_prim_inf, eps_dual_inf, alpha, check_termination, scaled_termination, rho
 *            (one k_shared_factor launch; the carried iterates stay, as with osqp_update_rho).  Any other name is refused.
 * device_bytes()  the device memory the handle holds, staging included.
 * where: 0 host pointers, 1 device pointers on the handle's device.  Every call blocks until done; 0 = success, otherwise
 * osqp_amd_last_error has the reason.
 * adjoint()  gradients of a scalar loss with respect to the data through the solutions of the last resolve (DESIGN.md section
 *            13.4): the mathematics and the five-gradient table of osqp_amd_batch_adjoint, the rules of
 *            osqp_amd_batch_adjoint_multi -- `ncot` pairs (dx, dy) per instance in cotangent-major arrays [ncot x count x n],
 *            [ncot x count x m], NULL = zeros (not both); dq, dl, du, dPx, dAx [ncot x count x cols], NULL = not wanted; act_out
 *            [count x m] (-1 lower, 1 upper, 0 inactive; a row with l == u is active and lower) and status_out [count] once per
 *            instance.  Status 1: differentiated; 0: the instance's last status is not OSQP_SOLVED; -1: the factorisation
 *            failed; rows with status != 1 are zeros.  Instance i is differentiated as the shared instance it is: the scaling
 *            is that of the base data.
 *            dPx_sum [ncot x nnzP], dAx_sum [ncot x nnzA] (NULL = not wanted): the gradients of the SHARED values, the sums
 *            over the instances of the per-instance rows r_i, formed on the device in a fixed order that depends on count alone:
 *              s_b = ((r_16b + r_16b+1) + ...) + r_16b+15   over each block of 16 consecutive instances (the last one shorter),
 *              sum = ((s_0 + s_1) + s_2) + ...,
 *            plain IEEE additions, no atomics -- a loop in that order reproduces the bits, and they are the same whether or not
 *            dPx / dAx were asked for (then the rows go through a bounded scratch of the handle).  The gradients of
 *            (instance, cotangent) have the same bits whatever count, ncot, the position, the neighbours or the outputs wanted.
 *            The form of the kernel follows from the shape: the factor in LDS where that layout fits 160 KB (n <= 128),
 *            otherwise in a fixed number of n x n blocks of global scratch, allocated at the first such call and counted by
 *            device_bytes() -- never count x n x n.  A shape neither form serves is refused ("instance too large ...").
 *            CURRENCY: the call is refused (1, a message, nothing launched) before the first resolve and after any
 *            update_lin_cost, update_bounds, warm_start or update_setting("rho") that followed the last resolve.  It only
 *            reads the handle: a resolve after it has the bits of one without it.  One call counts once in
 *            osqp_amd_shared_batch_adjoint_launches, whatever ncot is; a refused call does not count.
 * jvp()      forward sensitivities of the solutions of the last resolve along `ndir` directions of the data (DESIGN.md section
 *            13.5): the mathematics of osqp_amd_batch_jvp -- per instance i with solution (x_i, y_i) and active rows a_i, ONE
 *            solve per direction with [P, Aa'; Aa, 0] [tx; ty_a] = [-(tq_i + tP x_i + tA' y_i); (tb_i - tA x_i)_a], tb = tl on the
 *            lower rows, tu on the upper ones, ty zero on the inactive rows.  tq, tl, tu are PER INSTANCE, direction-major
 *            [ndir x count x n], [ndir x count x m].  tPx [ndir x nnzP] and tAx [ndir x nnzA] are ONE tangent per direction
 *            for the whole batch, as P and A are shared: tPx on the stored upper triangle (an off-diagonal entry stands for
 *            both halves), tAx in the order of the Ax given at setup -- the index spaces of dPx_sum / dAx_sum.  A NULL tangent
 *            is zero and gives the bits of an explicit zero array; not all five may be NULL (arrays of width 0 are dropped
 *            first).  On a row with l == u (scaled, as the handle stores it) only tl is read.  tx [ndir x count x n], ty
 *            [ndir x count x m], NULL = not wanted (not both); act_out [count x m] and status_out [count] as the adjoint's,
 *            with the same values.  The sensitivities of (instance, direction) have the same bits whatever count, ndir, the
 *            position, the neighbours or the outputs wanted.  The form of the kernel and its factor blocks are the adjoint's:
 *            the same blocks, allocated by whichever call comes first.  ndir < 1 is refused.  CURRENCY and reading only: as
 *            the adjoint.  One call counts once in osqp_amd_shared_batch_jvp_launches, whatever ndir is; a refused call does
 *            not count.
 * The handle has no polish, certificates, duality or `rows` entries, and its matrices cannot be
 * updated: a new model is a new handle. */
typedef struct osqp_amd_shared_batch osqp_amd_shared_batch;
c_int osqp_amd_shared_batch_plan(c_int n, c_int m, c_int nnzA, c_int nnzF, c_int *out /* [4] */);
c_int osqp_amd_shared_batch_setup(osqp_amd_shared_batch **out, c_int count, c_int n, c_int m,
                                  const c_int *Pp, const c_int *Pi, const c_float *Px,
                                  const c_int *Ap, const c_int *Ai, const c_float *Ax,
                                  const c_float *q0, const c_float *l0, const c_float *u0,
                                  const OSQPSettings *settings, c_int device);
c_int osqp_amd_shared_batch_update_lin_cost(osqp_amd_shared_batch *batch, const c_float *q_all, c_int where);
c_int osqp_amd_shared_batch_update_bounds(osqp_amd_shared_batch *batch, const c_float *l_all, const c_float *u_all, c_int where);
c_int osqp_amd_shared_batch_warm_start(osqp_amd_shared_batch *batch, const c_float *x_all, const c_float *y_all, c_int where);
c_int osqp_amd_shared_batch_resolve(osqp_amd_shared_batch *batch, c_float *x_out, c_float *y_out, c_float *info_out, c_int where);
c_int osqp_amd_shared_batch_update_setting(osqp_amd_shared_batch *batch, const char *name, c_float value);
c_int osqp_amd_shared_batch_adjoint(osqp_amd_shared_batch *batch, c_int ncot, const c_float *dx, const c_float *dy,
                                    c_float *dq, c_float *dl, c_float *du, c_float *dPx, c_float *dAx, /* [ncot x count x cols] or NULL */
                                    c_float *dPx_sum, c_float *dAx_sum,                                /* [ncot x nnzP], [ncot x nnzA] or NULL */
                                    c_float *act_out, c_float *status_out, c_int where);
c_int osqp_amd_shared_batch_adjoint_launches(void);
c_int osqp_amd_shared_batch_jvp(osqp_amd_shared_batch *batch, c_int ndir,
                                const c_float *tq, const c_float *tl, const c_float *tu,   /* [ndir x count x n | m | m] or NULL */
                                const c_float *tPx, const c_float *tAx,                    /* [ndir x nnzP], [ndir x nnzA] or NULL: shared */
                                c_float *tx, c_float *ty,                                  /* [ndir x count x n | m] or NULL */
                                c_float *act_out, c_float *status_out, c_int where);       /* [count x m], [count] or NULL */
c_int osqp_amd_shared_batch_jvp_launches(void);
c_int osqp_amd_shared_batch_device_bytes(osqp_amd_shared_batch *batch);
c_int osqp_amd_shared_batch_launches(void);
c_int osqp_amd_shared_batch_destroy(osqp_amd_shared_batch *batch);

/* Select the HIP device for workspaces created afterwards by this process
 * (one process per GPU: pass LOCAL_RANK). */
c_int osqp_amd_set_device(c_int device);

/* Host-only: the symbolic analysis of the direct back-end on the pattern of a QP (triu(P) and A in CSC form), no
 * device needed -- what the CPU tests of the ordering / level schedule / supernode partition call.
 * ordering: 0 minimum degree, 1 nested dissection, 2 minimum degree with queued ties; smax: largest supernode.
 * out[0..12]: N, nnz(L), pivot levels, supernodes, supernode levels, entries outside the diagonal blocks,
 *            doubles in the inverted blocks, largest supernode, 1 if every structural invariant holds, nnz in blocks,
 *            modelled microseconds of a solve by levels / by supernodes, 1 if the engine would take supernodes;
 * out[13] (when count >= 14): depth of a breadth-first level structure of the KKT graph (>= 400 on a problem of >= 2e5
 *            pivots sends nested dissection first) */
c_int osqp_amd_symbolic_probe(c_int n, c_int m, const c_int *Pp, const c_int *Pi, const c_int *Ap, const c_int *Ai,
                              c_int ordering, c_int smax, c_float *out, c_int count);

/* Last error message of the calling thread ("" if none). */
const char *osqp_amd_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* OSQP_AMD_H */
