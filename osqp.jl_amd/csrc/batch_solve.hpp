// batch_solve.hpp -- the batched small-QP kernel of rounds 1-3: ONE QP PER 512-THREAD WORKGROUP, two per compute unit, for
// every pattern with n <= 128 that the four-wavefront kernel (batch_quad.hpp) does not take (run-time shapes, dense P,
// long rows).  Stands on batch_common.hpp; launch_batch (batch.hip) dispatches to it.
//   - LDS (~75 KB at n = 100, m = 200): the instance's values of A (shared sparsity pattern, CSC order) and of the full
//     symmetric P, q, l, u, the Ruiz scalings, all ADMM iterates, and the thread's share of the pattern of A in both
//     orientations as packed (value offset, operand offset) words;
//   - REGISTERS: the inverse of the reduced KKT matrix M = P + sigma I + A' diag(rho) A -- thread 4 i + c of the 512
//     holds M^-1[i, c*n/4 .. (c+1)*n/4) (25 doubles at n = 100): the four column parts of a row sit in neighbouring
//     lanes, so the dense product ends in two DPP adds instead of a trip through LDS;
//   - M is assembled from host-precomputed term lists in a per-instance n x n scratch in GLOBAL memory (L2-resident) and
//     inverted there by Gauss-Jordan block sweeps on the fp64 matrix cores (invert_mfma), then loaded into the register
//     tiles.  (The on-chip variant of this factorisation was built in round 3 and measured slower for this
//     decomposition: profiles/r03_batch_experiments.md.)
// Per iteration, three barrier-separated phases: b = sigma x - q + A'(rho z - y) (4 lanes per column of A);
// x~ = M^-1 b (registers x LDS broadcast) with the x update; z~ = A x~ consumed row by row by the z / y update (2 lanes
// per row); every `check_termination` iterations the same residual / infeasibility tests as the large-problem path.
// The 512-thread kernel is issue-bound, not latency-bound (round 3: 16 waves per CU, every vector instruction of a wavefront is four
// cycles of its SIMD): the iteration is written for instruction count -- operand addresses come ready-made out of one
// packed word (two instructions per entry), short columns / rows are padded with a zero-valued entry instead of
// branching, nothing the loop needs lives in spilled registers.
#pragma once
#include "batch_common.hpp"

namespace oq {
namespace {

#ifndef OQ_BATCH_NT
#define OQ_BATCH_NT 512
#endif
constexpr int NT = OQ_BATCH_NT;  // threads per workgroup = per QP
constexpr int NW = NT / 64;

constexpr int KT = 4, KR = 6;  // entries per lane: 4 lanes per column of A (A' v), 2 lanes per row (A v)
constexpr int KRW = 8;         // dwords per thread of the row-side words (6 used: a 16-byte and an 8-byte read)

// The pivot buffers of the MFMA inversion (Lds::gjc) as a layout: GW doubles per pivot row -- 128 for the kernels of this file,
// 256 for k_batch_solve_large (batch_large.hpp) -- and what sits behind them.  Every user takes its offsets from here.
constexpr int kPivotW = 128;
__host__ __device__ constexpr int gjc_pivot(int gw) { return 2 * 4 * gw; }    // where the 2 x 32 of the pivot block start
__host__ __device__ constexpr int gjc_parked(int gw) { return 2 * 4 * gw + 56; }  // the parked record pointer; + 1: the gap refusals
__host__ __device__ constexpr int gjc_doubles(int gw) { return 2 * 4 * gw + 64; }

struct Lds {
  ldouble *gjc;  // 2 x (4 x GW): the four pivot rows of a block step of the MFMA inversion, double-buffered; behind them
                 // 2 x 32: the inverse of the 4 x 4 pivot block and its positive-definite flag
  ldouble *bb, *Av, *Pv, *q, *l, *u, *D, *E, *rho, *rhoi, *x, *z, *y, *xp, *zp, *xt, *zt, *dx, *dy, *Ax, *Px, *Aty, *tn, *tm, *red, *ldinv, *nrm;
  lint *ctype;
  lshort *Ap, *Ai, *Rp, *Rc, *Rmap, *Fp, *Fc;  // shared pattern, staged into LDS as 16-bit indices
  luint *cw, *rw;  // the thread's entries of A, column side (KT words per thread) and row side (KRW per thread): (byte offset of
                   // the value in Av) << 16 | byte offset of the operand; only when the pattern fits (sparse_fits)
  int ld;
};
// Av carries one more double than A has entries: a zero that padded entries point at
__host__ __device__ inline size_t lds_doubles(int n, int m, int nnzA, int nnzF, int gw = kPivotW) {
  return (size_t)n + nnzA + 1 + nnzF + 10 * (size_t)n + 12 * (size_t)m + 16 * NW + 24 + gjc_doubles(gw) + 1;  // + 1: alignment slack
}
__host__ __device__ inline size_t lds_shorts(int n, int m, int nnzA, int nnzF) {
  return 2 * ((size_t)n + 1) + ((size_t)m + 1) + 3 * (size_t)nnzA + (size_t)nnzF + 8;
}
__host__ __device__ inline size_t lds_bytes(int n, int m, int nnzA, int nnzF, bool words, int gw = kPivotW) {
  return lds_doubles(n, m, nnzA, nnzF, gw) * 8 + (((size_t)m * 4 + 15) / 16) * 16 + (words ? (size_t)NT * (KT + KRW) * 4 : 0) +
         lds_shorts(n, m, nnzA, nnzF) * 2 + 16;
}
template <int GW = kPivotW>
__device__ __forceinline__ Lds carve(ldouble *base, const Pattern &P, bool words) {
  Lds s;
  const int n = P.n, m = P.m;
  s.ld = n + 1;
  ldouble *p = base;
  s.bb = p; p += n;  // the right-hand side of the reduced system
  s.Av = p; p += P.nnzA + 1; s.Pv = p; p += P.nnzF;
  s.q = p; p += n; s.D = p; p += n; s.x = p; p += n; s.xp = p; p += n; s.xt = p; p += n; s.dx = p; p += n;
  s.Px = p; p += n; s.Aty = p; p += n; s.tn = p; p += n; s.ldinv = p; p += n;
  s.l = p; p += m; s.u = p; p += m; s.E = p; p += m; s.rho = p; p += m; s.rhoi = p; p += m; s.z = p; p += m; s.y = p; p += m;
  s.zp = p; p += m; s.zt = p; p += m; s.dy = p; p += m; s.Ax = p; p += m; s.tm = p; p += m;
  s.red = p; p += 16 * NW;  // NW * K doubles of block_reduce, K <= 14
  s.nrm = p; p += 24;
  s.gjc = p; p += gjc_doubles(GW);
  p += (p - base) & 1;  // what follows starts on a 16-byte boundary
  s.ctype = (lint *)p;
  luint *w = (luint *)((lchar *)p + (((size_t)m * 4 + 15) / 16) * 16);  // 16-byte aligned: the words are read four at a time
  s.cw = w; s.rw = w + (words ? NT * KT : 0);
  lshort *h = (lshort *)(w + (words ? NT * (KT + KRW) : 0));
  s.Ap = h; h += n + 1; s.Fp = h; h += n + 1; s.Rp = h; h += m + 1;
  s.Ai = h; h += P.nnzA; s.Rc = h; h += P.nnzA; s.Rmap = h; h += P.nnzA; s.Fc = h;
  return s;
}

// y = A x (CSR), y = A' x (CSC), y = P x (full symmetric CSR); no barriers inside.  L lanes share a row (the index ->
// value -> operand chain of LDS reads is latency-bound: 8 entries walked by one lane cost 8 round trips, by 4 lanes 2)
// and add up with xor shuffles, so every thread of the workgroup reaches the shuffles whether it has a row or not.
// finish(r, sum) runs on one lane per row.
template <int L, typename F, typename G>
__device__ __forceinline__ void rows_dot(int rows, const lshort *ptr, F term, G finish) {
  const int lane = mytid() & (L - 1);
  for (int base = 0; base < rows; base += NT / L) {
    const int r = base + mytid() / L;
    double a = 0.0;
    if (r < rows)
      for (int q = ptr[r] + lane; q < ptr[r + 1]; q += L) a += term(q);
#pragma unroll
    for (int o = L >> 1; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (lane == 0 && r < rows) finish(r, a);
  }
}
__device__ __forceinline__ void mul_P(const Pattern &P, const Lds &s, const ldouble *x, ldouble *y) {
  rows_dot<4>(P.n, s.Fp, [&](int q) { return s.Pv[q] * x[s.Fc[q]]; }, [&](int r, double a) { y[r] = a; });
}

__device__ __forceinline__ void set_rho(const Pattern &P, const Lds &s, double rho, bool classify) {
  for (int i = mytid(); i < P.m; i += NT) {
    int t;
    if (classify) {
      if (s.l[i] < -B_INF && s.u[i] > B_INF) t = -1;
      else if (s.u[i] - s.l[i] < 1e-4) t = 1;
      else t = 0;
      s.ctype[i] = t;
    } else t = s.ctype[i];
    double r = t == -1 ? B_RHO_MIN : (t == 1 ? 1e3 * rho : rho);
    s.rho[i] = r; s.rhoi[i] = 1.0 / r;
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------
// The reduced KKT matrix and its inverse, in registers.
//
// Thread t = 4 * row + part owns row `row` (rows >= n idle) and the NC = ceil(n / PARTS) columns
// [part * NC, (part + 1) * NC) of the n x n array: T.v[u] = M^-1[row, j0 + u].  NCT is the compile-time bound of NC.
// The four parts of a row are neighbouring lanes: the dense product M^-1 b ends in two quad-permute adds.
//
// Why an explicit inverse: it is applied to thousands of right-hand sides (one per ADMM iteration) between two rho
// updates, and a dense product M^-1 b keeps every row independent while a triangular solve is a chain of 2n dependent
// steps.  Why Gauss-Jordan sweeps (Goodnight's sweep operator): a block sweep is a rank-4 update of the whole array on the
// matrix cores (invert_mfma below) -- no serial column loop anywhere.  The pivots are the Schur complements of M, so the
// positive-definiteness test of the Cholesky factorisation carries over unchanged.
// ---------------------------------------------------------------------------------------------------------
constexpr int PARTS = 4;
static_assert(NT == 512, "the register tiles assume 128 rows x 4 column parts");

template <int NCT>
struct MTile {
  double v[NCT];
};

// Addressing rule of the routines below: ONE base register per array and compile-time offsets u / u ld.  (Written with the
// global column j = j0 + u, the 25 column ids and 25 clamped addresses are loop invariants that the compiler precomputes
// and then has to keep in -- or spill from -- registers across the whole ADMM loop.)  EXACT: PARTS * NCT == n, no
// column of a tile lies outside the matrix; otherwise columns u >= ncv of the last part are masked.
// the thread's tile (row = tid >> 2, NCT columns of part tid & 3) of the n x n array in the instance's scratch
template <int NCT, bool EXACT>
__device__ __forceinline__ void load_tile(int n, const double *scratch, MTile<NCT> &T) {
  scratch = opaque(scratch);
  const int ld = n;
  const int row = mytid() >> 2, part = mytid() & 3;
  const int nc = EXACT ? NCT : (n + PARTS - 1) / PARTS, j0 = part * nc;
  const int ncv = EXACT ? NCT : max(0, min(nc, n - j0));
  const bool live = row < n;
  const double *src = scratch + (live ? row : 0) + (size_t)min(j0, n - 1) * ld;
#pragma unroll
  for (int u = 0; u < NCT; u++) T.v[u] = (live && (EXACT || u < ncv)) ? src[(size_t)u * ld] : 0.0;
}
// M = P + sigma I + A' diag(rho) A: the lower triangle from the host-precomputed term lists (the intersections of the
// columns of A do not depend on the instance), both triangles into the instance's scratch (global memory, n x n,
// column-major)
__device__ __forceinline__ void assemble_scratch(const Pattern &P, const Lds &s, double sigma, double *__restrict__ scratch) {
  const int n = P.n, ld = n;
  scratch = opaque(scratch);
  for (int e = mytid(); e < n * ld; e += NT) scratch[e] = 0.0;
  __syncthreads();
  for (int t = mytid(); t < P.npair; t += NT) {
    double acc = 0.0;
    const int q1 = P.Tp[t + 1];
    int q = P.Tp[t];
    for (; q + 4 <= q1; q += 4) {  // the index triples of four terms first (global memory), then their LDS operands, then the sum in order
      unsigned short tr[4], ta[4], tb[4];
#pragma unroll
      for (int u = 0; u < 4; u++) { tr[u] = P.Tr[q + u]; ta[u] = P.Ta[q + u]; tb[u] = P.Tb[q + u]; }
      double r[4], a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; u++) { r[u] = s.rho[tr[u]]; a[u] = s.Av[ta[u]]; b[u] = s.Av[tb[u]]; }
#pragma unroll
      for (int u = 0; u < 4; u++) acc += r[u] * a[u] * b[u];
    }
    for (; q < q1; q++) acc += s.rho[P.Tr[q]] * s.Av[P.Ta[q]] * s.Av[P.Tb[q]];
    const int i = P.Ti[t], j = P.Tj[t];
    scratch[i + j * ld] = acc;
    scratch[j + i * ld] = acc;
  }
  __syncthreads();
  for (int i = mytid(); i < n; i += NT) scratch[i + i * ld] += sigma;
  __syncthreads();
  for (int r = mytid(); r < n; r += NT)
    for (int q = s.Fp[r]; q < s.Fp[r + 1]; q++) scratch[r + s.Fc[q] * ld] += s.Pv[q];  // full symmetric P: both triangles
  __syncthreads();
}


// ---- the same inverse by block sweeps on the matrix cores ---------------------------------------------------------
// Four pivots at a time: with K the pivot indices, C = M[K, :] (4 x n) and G = M[K, K]^-1 the sweep operator is
//   M <- M - C' (G C),  then  M[K, R] <- G C (and its mirror),  M[K, K] <- -G,
// i.e. one rank-4 update of the whole array -- v_mfma_f64_16x16x4_f64 per 16 x 16 tile -- and a patch of four rows and
// columns, instead of four rank-1 updates whose pivot row has to be broadcast element by element (invert_tile: 50
// v_readlane per 25 multiply-adds, ~10 % of the fp64 rate).  The array stays symmetric, so only the tiles on and below
// the diagonal are kept, TPW per wavefront in accumulator layout (lane: column lane & 15, rows (lane >> 4) + 4 r);
// indices >= n are padded with the identity and never swept.  One barrier per block step: the pivot rows go through two
// alternating 4 x GW LDS buffers (GW >= 16 ceil(n / 16)).  In: M in the instance's scratch (both triangles, ld = n); out: M^-1 there.
typedef double d4_t __attribute__((ext_vector_type(4)));
template <int TPW, int GW = kPivotW>
__device__ __forceinline__ bool invert_mfma(int n, double *scratch, ldouble *cb) {
  scratch = opaque(scratch);
  const int lane = mytid() & 63, wave = uni(mytid() >> 6);
  const int lr = lane >> 4, lc = lane & 15;
  const int NB = (n + 15) >> 4, ntiles = NB * (NB + 1) / 2, steps = (n + 3) >> 2;
  d4_t acc[TPW];
  int TI[TPW], TJ[TPW];
#pragma unroll
  for (int s = 0; s < TPW; s++) {
    const int t = wave + s * NW;
    int I = -1, J = -1;
    if (t < ntiles) { I = 0; while ((I + 1) * (I + 2) / 2 <= t) I++; J = t - I * (I + 1) / 2; }
    TI[s] = uni(I); TJ[s] = uni(J);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = I * 16 + lr + 4 * r, col = J * 16 + lc;
      double v = (row == col) ? 1.0 : 0.0;
      if (I >= 0 && row < n && col < n) v = scratch[row + (size_t)col * n];
      acc[s][r] = v;
    }
  }
  bool ok = true;
  for (int tb = 0; tb < NB; tb++) {
#pragma unroll
    for (int tq = 0; tq < 4; tq++) {
      const int step = tb * 4 + tq;
      if (step < steps) {
        ldouble *C = cb + (step & 1) * (4 * GW);  // C[a][j] at a * GW + j
        ldouble *Gs = cb + gjc_pivot(GW) + (step & 1) * 32;
        // publish rows k0 .. k0 + 3: left of and inside block tb from the tiles of row block tb (register tq of every
        // lane), right of it from column k0 + a of the tiles below (the array is symmetric).  The wavefront that owns the
        // diagonal tile also inverts the 4 x 4 pivot block -- it sits in register tq of its lanes 16 a + 4 tq + b -- while
        // the others wait at the barrier: one Gauss-Jordan per block step instead of one per wavefront.
#pragma unroll
        for (int s = 0; s < TPW; s++) {
          if (TI[s] == tb) C[lr * GW + TJ[s] * 16 + lc] = acc[s][tq];
          if (TJ[s] == tb && TI[s] > tb && (lc >> 2) == tq) {
#pragma unroll
            for (int r = 0; r < 4; r++) C[(lc & 3) * GW + TI[s] * 16 + lr + 4 * r] = acc[s][r];
          }
          if (TI[s] == tb && TJ[s] == tb) {
            double g[4][4];
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
              for (int b = 0; b < 4; b++) g[a][b] = lane_bcast(acc[s][tq], 16 * a + 4 * tq + b);
            bool pd = true;
#pragma unroll
            for (int p = 0; p < 4; p++) {
              if (!(g[p][p] > 0.0)) pd = false;
              double d = __builtin_amdgcn_rcp(g[p][p]);                 // v_rcp_f64 and two Newton steps instead of the
              d = __builtin_fma(__builtin_fma(-g[p][p], d, 1.0), d, d);  // ~40-instruction chain of the IEEE division
              d = __builtin_fma(__builtin_fma(-g[p][p], d, 1.0), d, d);
#pragma unroll
              for (int j = 0; j < 4; j++) if (j != p) g[p][j] *= d;
#pragma unroll
              for (int i = 0; i < 4; i++) if (i != p) {
                const double f = g[i][p];
#pragma unroll
                for (int j = 0; j < 4; j++) if (j != p) g[i][j] = __builtin_fma(-f, g[p][j], g[i][j]);
                g[i][p] = -f * d;
              }
              g[p][p] = d;
            }
            if (lane == 0) {
#pragma unroll
              for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) Gs[a * 4 + b] = g[a][b];
              Gs[16] = pd ? 1.0 : 0.0;
            }
          }
        }
        __syncthreads();
        if (Gs[16] == 0.0) ok = false;
        double gl[4], gc[4];  // rows lane >> 4 and lane & 3 of G
#pragma unroll
        for (int b = 0; b < 4; b++) { gl[b] = Gs[lr * 4 + b]; gc[b] = Gs[(lc & 3) * 4 + b]; }
        const double gdiag = Gs[lr * 4 + (lc & 3)];
#pragma unroll
        for (int s = 0; s < TPW; s++) {
          if (TI[s] < 0) continue;
          const double aop = -C[lr * GW + TI[s] * 16 + lc];  // A[i = lane & 15][k = lane >> 4] = -C[k][row i of block I]
          const ldouble *cj = C + TJ[s] * 16 + lc;
          double bop = gl[0] * cj[0];                          // B[k = lane >> 4][j = lane & 15] = (G C)[k][column j of block J]
          bop = __builtin_fma(gl[1], cj[GW], bop);
          bop = __builtin_fma(gl[2], cj[2 * GW], bop);
          bop = __builtin_fma(gl[3], cj[3 * GW], bop);
          acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop, bop, acc[s], 0, 0, 0);
          if (TI[s] == tb) acc[s][tq] = (TJ[s] == tb && (lc >> 2) == tq) ? -gdiag : bop;  // rows K: G C, and -G inside the block
          if (TJ[s] == tb && (lc >> 2) == tq) {                                              // columns K: the mirror
#pragma unroll
            for (int r = 0; r < 4; r++) {
              if (TI[s] == tb && r == tq) continue;  // rows K of the diagonal tile were set above
              const ldouble *ci = C + TI[s] * 16 + lr + 4 * r;
              double w = gc[0] * ci[0];
              w = __builtin_fma(gc[1], ci[GW], w);
              w = __builtin_fma(gc[2], ci[2 * GW], w);
              w = __builtin_fma(gc[3], ci[3 * GW], w);
              acc[s][r] = w;
            }
          }
        }
      }
    }
  }
  // the sweeps leave -M^-1; both triangles back into the scratch
  // (the wide instantiations take the pointer and the lane afresh: the 4 TPW addresses of the load above are otherwise kept
  // for this loop -- spilled before the sweeps and fetched back after them)
  int sr = lr, sc = lc;
  if constexpr (GW > kPivotW) { scratch = opaque(scratch); const int l2 = mytid() & 63; sr = l2 >> 4; sc = l2 & 15; }
#pragma unroll
  for (int s = 0; s < TPW; s++) {
    if (TI[s] < 0) continue;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = TI[s] * 16 + sr + 4 * r, col = TJ[s] * 16 + sc;
      if (row < n && col < n) {
        const double v = -acc[s][r];
        scratch[row + (size_t)col * n] = v;
        scratch[col + (size_t)row * n] = v;
      }
    }
  }
  __syncthreads();
  return ok;
}

// LDS through a byte offset: with the arrays at compile-time addresses (the shape-specialised kernel) the base is an
// immediate of the ds_read and the offset register goes in as it comes out of the packed word
__device__ __forceinline__ double lds_at(const ldouble *base, unsigned byte_off) {
  return *(const ldouble *)((const lchar *)base + byte_off);
}

// x~ = M^-1 b with b in s.bb: the thread's NCT entries of row `row` against its stretch of b (every lane of a quad reads
// its own part: four addresses per wavefront, each a broadcast), then the four parts of the row add up inside the quad.
// The lane of part 0 finishes the row on the spot: x~ to s.xt (the row-side product reads it), x and delta_x.
template <int NCT, bool EXACT>
__device__ __forceinline__ void apply_tile(int n, const MTile<NCT> &T, const Lds &s, double alpha, const ldouble *xp, ldouble *x) {
  const int row = mytid() >> 2, part = mytid() & 3;
  const int nc = EXACT ? NCT : (n + PARTS - 1) / PARTS, j0 = part * nc;
  const int ncv = EXACT ? NCT : max(0, min(nc, n - j0));
  const ldouble *bp = s.bb + j0;
  double bj[NCT];
#pragma unroll
  for (int u = 0; u < NCT; u++) bj[u] = (EXACT || u < ncv) ? bp[u] : 0.0;
  const double xo = xp[row < n ? row : 0];
  double a0 = 0.0, a1 = 0.0;
#pragma unroll
  for (int u = 0; u < NCT; u++) {
    if (u & 1) a1 = __builtin_fma(T.v[u], bj[u], a1); else a0 = __builtin_fma(T.v[u], bj[u], a0);
  }
  double a = a0 + a1;
  a += quad_xor<2>(a);
  a += quad_xor<1>(a);
  if (part == 0 && row < n) {
    s.xt[row] = a;
    const double xn = alpha * a + (1.0 - alpha) * xo;
    x[row] = xn;
    s.dx[row] = xn - xo;
  }
}

// ---------------------------------------------------------------------------------------------------------
// The thread's share of the pattern of A, both orientations, as packed words in LDS (s.cw, s.rw):
//   column side (A' v):  4 lanes per column, lane l of column c walks entries Ap[c] + l, + 4, ...   (KT per lane)
//   row side    (A v):   2 lanes per row,    lane l of row r    walks entries Rp[r] + l, + 2, ...   (KR per lane)
// A word holds (byte offset of the value inside Av) << 16 | (byte offset of the operand inside its vector): both LDS reads
// of an entry take their address from one shift / one mask, where the walk through the pattern arrays is a chain of three
// dependent reads.  A lane with fewer entries than KT / KR is padded with words that point at the zero behind the values
// of A (and at operand 0): the loops have no tails and no predicates, the padded terms add +0.0 and change nothing.
// The words live in LDS, not in registers: the hot loop fetches them with one 16-byte read (two on the row side) -- held
// in registers across the ADMM loop they were the first thing the allocator spilled, and a spilled word came back from
// scratch memory once per entry and iteration (round 2: ~10 dependent round trips to memory per iteration).
// Same lane-strided order and the same quad reduction as rows_dot<4> / rows_dot<2>: bit-identical sums.  Used when the
// pattern fits (at most 4 KT per column, 2 KR per row, 4 n and 2 m threads); rows_dot on the LDS copy otherwise.
// ---------------------------------------------------------------------------------------------------------
__host__ __device__ inline bool sparse_fits(const Pattern &P) {
  // m > 0: a padded entry reads operand 0 of the vector it is multiplied into -- there has to be one (0 x garbage is not 0)
  return P.m > 0 && P.nnzA > 0 && 4 * P.n <= NT && 2 * P.m <= NT && P.max_col <= 4 * KT && P.max_row <= 2 * KR && (size_t)(P.nnzA + 1) * 8 < 65536;
}
__device__ __forceinline__ void store_sparse(const Pattern &P, const Lds &s) {
  const int t = mytid();
  const unsigned pad = (unsigned)(P.nnzA * 8) << 16;  // the zero behind the values, operand 0
  const int col = (t >> 2) < P.n ? (t >> 2) : -1, row = (t >> 1) < P.m ? (t >> 1) : -1;
#pragma unroll
  for (int e = 0; e < KT; e++) {
    unsigned w = pad;
    if (col >= 0) {
      const int k = s.Ap[col] + (t & 3) + 4 * e;
      if (k < s.Ap[col + 1]) w = ((unsigned)(k * 8) << 16) | (unsigned)(s.Ai[k] * 8);
    }
    s.cw[t * KT + e] = w;
  }
#pragma unroll
  for (int e = 0; e < KRW; e++) {
    unsigned w = pad;
    if (row >= 0 && e < KR) {
      const int q = s.Rp[row] + (t & 1) + 2 * e;
      if (q < s.Rp[row + 1]) w = ((unsigned)(s.Rmap[q] * 8) << 16) | (unsigned)(s.Rc[q] * 8);
    }
    s.rw[t * KRW + e] = w;
  }
}
struct ColWords { unsigned w[KT]; };
struct RowWords { unsigned w[KR]; };
__device__ __forceinline__ ColWords col_words(const Lds &s) {
  const uint4_t v = *(const luint4 *)(s.cw + mytid() * KT);
  ColWords c;
  c.w[0] = v.x; c.w[1] = v.y; c.w[2] = v.z; c.w[3] = v.w;
  return c;
}
__device__ __forceinline__ RowWords row_words(const Lds &s) {
  const luint *p = s.rw + mytid() * KRW;
  const uint4_t v = *(const luint4 *)p;
  const uint2_t v2 = *(const luint2 *)(p + 4);
  RowWords r;
  r.w[0] = v.x; r.w[1] = v.y; r.w[2] = v.z; r.w[3] = v.w; r.w[4] = v2.x; r.w[5] = v2.y;
  return r;
}
// sum over the lane's entries of value * v[operand]; the value is read through `val(byte offset)` so that the scaling
// passes can look at |value| with the same walk
// finish(col, sum over the column of A of value * v[row]) on one lane per column
// All LDS reads of a phase are issued before the first one is consumed (values and operands into arrays first, the
// arithmetic in a second loop, in entry order): one round trip to LDS per phase instead of one per entry.
// pre(index) reads what finish() will need about the column / row (every lane: the reads join the batch above, clamped
// index for lanes without one); finish(index, sum, what pre returned) runs on one lane per column / row.
template <typename PRE, typename G>
__device__ __forceinline__ void col_dot(const Lds &s, const ldouble *v, int n, PRE pre, G finish) {
  const ColWords c = col_words(s);
  const int t = mytid(), j = t >> 2;
  double av[KT], ov[KT];
#pragma unroll
  for (int e = 0; e < KT; e++) { av[e] = lds_at(s.Av, c.w[e] >> 16); ov[e] = lds_at(v, c.w[e] & 0xFFFFu); }
  const auto ops = pre(j < n ? j : 0);
  double a = 0.0;
#pragma unroll
  for (int e = 0; e < KT; e++) a += av[e] * ov[e];
  a += quad_xor<2>(a);
  a += quad_xor<1>(a);
  if ((t & 3) == 0 && j < n) finish(j, a, ops);
}
template <typename PRE, typename G>
__device__ __forceinline__ void row_dot(const Lds &s, const ldouble *v, int m, PRE pre, G finish) {
  const RowWords r = row_words(s);
  const int t = mytid(), i = t >> 1;
  double av[KR], ov[KR];
#pragma unroll
  for (int e = 0; e < KR; e++) { av[e] = lds_at(s.Av, r.w[e] >> 16); ov[e] = lds_at(v, r.w[e] & 0xFFFFu); }
  const auto ops = pre(i < m ? i : 0);
  double a = 0.0;
#pragma unroll
  for (int e = 0; e < KR; e++) a += av[e] * ov[e];
  a += quad_xor<1>(a);
  if ((t & 1) == 0 && i < m) finish(i, a, ops);
}
struct Ops2 { double a, b; };
struct Ops6 { double a, b, c, d, e, f; };

#ifdef OQ_BATCH_PROFILE
#define PROF_DECL long long pt0 = clock64(), pacc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#define PROF(k) { long long pt1 = clock64(); pacc[k] += pt1 - pt0; pt0 = pt1; }
#define PROF_PRINT if (inst == 0 && tid == 0) printf("cycles: load %lld scale %lld assemble %lld invert %lld rhs %lld solve %lld mulA+upd %lld check %lld rho %lld iters %d\n", pacc[0], pacc[1], pacc[8], pacc[2], pacc[3], pacc[4], pacc[5], pacc[6], pacc[7], iter);
#else
#define PROF_DECL
#define PROF(k)
#define PROF_PRINT
#endif

// ---------------------------------------------------------------------------------------------------------
// Residual evaluation + termination tests, every `check_termination` iterations.  NOT inlined on purpose: the ADMM
// loop holds the inverse in registers; as a separate function this phase gets its own register allocation (the call
// saves / restores what is live around it -- once per 25 iterations) instead of dragging 100+ temporaries into the
// allocation of the hot loop.  Everything it needs is in LDS (products walk the LDS copy of A); results go back through
// the nrm[] block: the 14 norms (Slot order of the large-problem path), then pri_res, dua_res, obj and the status code
// (0: keep iterating).
// ---------------------------------------------------------------------------------------------------------
struct CheckArgs {
  int n, m, nnzA, nnzF, swapped, uns, passes, last, words;
  double ea, er, epi, edi, c, cinv;
};

// K values per thread -> K block results in out[0..K) (max for op 0, sum for op 1); two barriers, a few registers
template <int K>
__device__ __forceinline__ void block_reduce_to(double *v, int op, ldouble *red, ldouble *out) {
#pragma unroll
  for (int k = 0; k < K; k++) {
    double a = v[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { double b = __shfl_xor(a, o, 64); a = op ? a + b : nmax(a, b); }
    v[k] = a;
  }
  __syncthreads();
  const int t = mytid();
  if ((t & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; k++) red[(t >> 6) * K + k] = v[k];
  }
  __syncthreads();
  if (t < K) {
    double a = red[t];
#pragma unroll 1
    for (int w = 1; w < NW; w++) a = op ? a + red[w * K + t] : nmax(a, red[w * K + t]);
    out[t] = a;
  }
  __syncthreads();
}

template <int CN, int CM, int CA, int CF, int GW = kPivotW>
__device__ __noinline__ void residual_phase(CheckArgs a) {
  Pattern P;
  P.n = CN ? CN : a.n; P.m = CN ? CM : a.m; P.nnzA = CN ? CA : a.nnzA; P.nnzF = CN ? CF : a.nnzF;
  const Lds s = carve<GW>((ldouble *)lds_raw, P, a.words != 0);
  const int n = P.n, m = P.m, tid = mytid();
  ldouble *x = a.swapped ? s.xp : s.x, *z = a.swapped ? s.zp : s.z;
  ldouble *nrm = s.nrm, *tmp = s.nrm + 18;  // tmp: 6 scratch results of the small reductions
  const bool uns = a.uns;
  const double c = a.c, cinv = a.cinv;
  auto a_rows = [&](const ldouble *v, auto finish) {
    rows_dot<2>(m, s.Rp, [&](int q) { return s.Av[s.Rmap[q]] * v[s.Rc[q]]; }, finish);
  };
  auto a_cols = [&](const ldouble *v, auto finish) {
    rows_dot<4>(n, s.Ap, [&](int k) { return s.Av[k] * v[s.Ai[k]]; }, finish);
  };
  // ---- residual evaluation (K8): nrm[0..14), pri_res, dua_res, obj ----
  {
    a_rows(x, [&](int r, double v) { s.Ax[r] = v; });
    mul_P(P, s, x, s.Px);
    a_cols(s.y, [&](int j, double v) { s.Aty[j] = v; });
    __syncthreads();
    double v[14];
#pragma unroll
    for (int k = 0; k < 14; k++) v[k] = 0.0;
    double sm[2] = {0.0, 0.0};
    for (int i = tid; i < m; i += NT) {
      double ax = s.Ax[i], zi = z[i], e = 1.0 / s.E[i], r = ax - zi;
      v[0] = nmax(v[0], fabs(r)); v[1] = nmax(v[1], fabs(e * r)); v[2] = nmax(v[2], fabs(zi)); v[3] = nmax(v[3], fabs(ax));
      v[4] = nmax(v[4], fabs(e * zi)); v[5] = nmax(v[5], fabs(e * ax));
    }
    for (int j = tid; j < n; j += NT) {
      double px = s.Px[j], qj = s.q[j], at = s.Aty[j], d = 1.0 / s.D[j], xj = x[j], r = (qj + px) + at;
      v[6] = nmax(v[6], fabs(r)); v[7] = nmax(v[7], fabs(d * r)); v[8] = nmax(v[8], fabs(qj)); v[9] = nmax(v[9], fabs(at));
      v[10] = nmax(v[10], fabs(px)); v[11] = nmax(v[11], fabs(d * qj)); v[12] = nmax(v[12], fabs(d * at)); v[13] = nmax(v[13], fabs(d * px));
      sm[0] += xj * px; sm[1] += qj * xj;
    }
    block_reduce_to<14>(v, 0, s.red, nrm);
    block_reduce_to<2>(sm, 1, s.red, tmp);
    if (tid == 0) {
      nrm[N_PRI] = m == 0 ? 0.0 : (uns ? nrm[1] : nrm[0]);
      nrm[N_DUA] = uns ? cinv * nrm[7] : nrm[6];
      nrm[N_OBJ] = cinv * (0.5 * tmp[0] + tmp[1]);
      nrm[N_STATUS] = 0.0;
    }
    __syncthreads();
  }
  const double pri_res = nrm[N_PRI], dua_res = nrm[N_DUA];
  // RES_GAP (batch_common.hpp): the duality gap as a third test, only where both residual tests hold.  The bit rides in the
  // parked record pointer; the two sums of the objective are taken out of tmp[] here, before the infeasibility tests of a
  // first pass reuse the slots
  const bool gap_rule = parked_gap(*(const lu64 *)(s.gjc + gjc_parked(GW)));
  const double sxpx = tmp[0], sqx = tmp[1];
  // ---- termination tests: the requested accuracy when a check is due or the iteration limit is reached,
  //      then -- at the limit only -- the 10x-relaxed ones ----
  int status = 0;
  for (int pass = 0; pass < a.passes && status == 0; pass++) {
    const bool approx = pass == 1;
    double ea = a.ea, er = a.er, epi = a.epi, edi = a.edi;
    if (!(pri_res <= OSQP_INFTY) || !(dua_res <= OSQP_INFTY)) { status = OSQP_NON_CVX; break; }
    if (approx) { ea *= 10; er *= 10; epi *= 10; edi *= 10; }
    bool pc = false, dc = false, pinf = false, dinf = false;
    if (m == 0) pc = true;
    else {
      double eps_p = ea + er * (uns ? nmax(nrm[4], nrm[5]) : nmax(nrm[2], nrm[3]));
      if (pri_res < eps_p) pc = true;
      else {  // primal infeasibility on delta_y
        double v[1] = {0.0}, sm[1] = {0.0};
        for (int i = tid; i < m; i += NT) {
          double d = s.dy[i];
          if (s.u[i] > B_INF) { if (s.l[i] < -B_INF) d = 0.0; else d = fmin(d, 0.0); }
          else if (s.l[i] < -B_INF) d = fmax(d, 0.0);
          s.dy[i] = d;
          v[0] = nmax(v[0], fabs(uns ? s.E[i] * d : d));
          sm[0] += s.u[i] * fmax(d, 0.0) + s.l[i] * fmin(d, 0.0);
        }
        block_reduce_to<1>(v, 0, s.red, tmp);
        block_reduce_to<1>(sm, 1, s.red, tmp + 1);
        const double nv = tmp[0], lhs = tmp[1];
        if (nv > epi && lhs < -epi * nv) {
          a_cols(s.dy, [&](int j, double t) { s.tn[j] = t; });
          __syncthreads();
          double w[1] = {0.0};
          for (int j = tid; j < n; j += NT) w[0] = nmax(w[0], fabs(uns ? s.tn[j] / s.D[j] : s.tn[j]));
          block_reduce_to<1>(w, 0, s.red, tmp + 2);
          pinf = tmp[2] < epi * nv;
        }
      }
    }
    double eps_d = ea + er * (uns ? cinv * nmax(nrm[11], nmax(nrm[12], nrm[13])) : nmax(nrm[8], nmax(nrm[9], nrm[10])));
    if (dua_res < eps_d) dc = true;
    else {  // dual infeasibility on delta_x
      double v[1] = {0.0}, sm[1] = {0.0};
      for (int j = tid; j < n; j += NT) { v[0] = nmax(v[0], fabs(uns ? s.D[j] * s.dx[j] : s.dx[j])); sm[0] += s.q[j] * s.dx[j]; }
      block_reduce_to<1>(v, 0, s.red, tmp + 3);
      block_reduce_to<1>(sm, 1, s.red, tmp + 4);
      const double nv = tmp[3], qdx = tmp[4];
      double cs = uns ? c : 1.0;
      if (nv > edi && qdx < -cs * edi * nv) {
        mul_P(P, s, s.dx, s.tn);
        __syncthreads();
        double w[1] = {0.0};
        for (int j = tid; j < n; j += NT) w[0] = nmax(w[0], fabs(uns ? s.tn[j] / s.D[j] : s.tn[j]));
        block_reduce_to<1>(w, 0, s.red, tmp + 5);
        if (tmp[5] < cs * edi * nv) {
          a_rows(s.dx, [&](int r, double t) { s.tm[r] = t; });
          __syncthreads();
          double bad[1] = {0.0};
          for (int i = tid; i < m; i += NT) {
            double t = uns ? s.tm[i] / s.E[i] : s.tm[i];
            if ((s.u[i] < B_INF && t > edi * nv) || (s.l[i] > -B_INF && t < -edi * nv) || t != t) bad[0] = 1.0;
          }
          block_reduce_to<1>(bad, 0, s.red, tmp + 5);
          dinf = tmp[5] == 0.0;
        }
      }
    }
    bool gc = true;
    if (pc && dc && gap_rule) {  // SC: every thread its rows in index order, then the fixed order of block_reduce_to
      double sm[1] = {0.0};
      for (int i = tid; i < m; i += NT) sm[0] += support_term(s.l[i], s.u[i], s.y[i], s.l[i], s.u[i]);
      block_reduce_to<1>(sm, 1, s.red, tmp + 2);
      gc = gap_test(sxpx, sqx, tmp[2], uns ? cinv : 1.0, ea, er);
      // a refusal means "go on" (neither infeasibility test ran at this check); counted behind the parked pointer
      if (!gc && tid == 0) s.gjc[gjc_parked(GW) + 1] += 1.0;
    }
    if (pc && dc) { if (gc) status = approx ? OSQP_SOLVED_INACCURATE : OSQP_SOLVED; }
    else if (pinf) status = approx ? OSQP_PRIMAL_INFEASIBLE_INACCURATE : OSQP_PRIMAL_INFEASIBLE;
    else if (dinf) status = approx ? OSQP_DUAL_INFEASIBLE_INACCURATE : OSQP_DUAL_INFEASIBLE;
  }
  if (a.last && a.passes && status == 0) status = OSQP_MAX_ITER_REACHED;
  __syncthreads();
  if (tid == 0) nrm[N_STATUS] = (double)status;
  __syncthreads();
}

// RES_CERT (batch_common.hpp), the last step of the epilogue: the direction that proves an infeasibility passes through the
// record slot it belongs to on its way to k_batch_cert, which puts the zero back.  Every thread overwrites the zeros it has
// just written itself (the same thread-to-entry map as the store before it).  A call like residual_phase, and for its
// reason: everything it needs is in LDS -- the parked record pointer with the RES_CERT bit, the status code where the
// residual phase left it (a loop that ended on a failed factorisation left 0 there: no certificate), delta_y and delta_x --
// so the kernel keeps no register for it and its own code stays what it was.
template <int CN, int CM, int CA, int CF, int GW = kPivotW>
__device__ __noinline__ void leave_certificate(int n_, int m_, int nnzA, int nnzF, int words) {
  Pattern P;
  P.n = CN ? CN : n_; P.m = CN ? CM : m_; P.nnzA = CN ? CA : nnzA; P.nnzF = CN ? CF : nnzF;
  const Lds s = carve<GW>((ldouble *)lds_raw, P, words != 0);
  const unsigned long long parked = *(const lu64 *)(s.gjc + gjc_parked(GW));
  if (!parked_cert(parked)) return;
  double *const rec = parked_ptr(parked);
  const int n = P.n, m = P.m, code = uni((int)s.nrm[N_STATUS]);
  if (status_prim_inf(code)) for (int i = mytid(); i < m; i += NT) rec[rec_y(n, m) + i] = s.dy[i];
  else if (status_dual_inf(code)) for (int j = mytid(); j < n; j += NT) rec[rec_x(n, m) + j] = s.dx[j];
}

// CN > 0: the instance shape (n, m, nnz(A), nnz(P full)) = (CN, CM, CA, CF) is known at compile time -- every LDS address
// becomes an immediate and every vector loop a fixed trip count (the registers otherwise spent on ~35 LDS pointers are
// what the inverse needs); CN = 0: the same source with the shape read from the pattern at run time.
template <int NCT, int CN, int CM, int CA, int CF, bool SEL>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_batch_solve(Pattern Pin, OSQPSettings st, int count, double *__restrict__ scratch_all,
                                                    const double *__restrict__ Px_all,
                                                    const double *__restrict__ Ax_all, const double *__restrict__ q_all,
                                                    const double *__restrict__ l_all, const double *__restrict__ u_all,
                                                    double *__restrict__ x_out, double *__restrict__ y_out,
                                                    double *__restrict__ info_out, int x_stride, int y_stride, int info_stride,
                                                    int info_cols, double *__restrict__ rec_all, int rec_stride, int res_mode,
                                                    const int *__restrict__ sel) {
  // the workgroup's position in the launch and the instance it serves (BatchIO::sel): the data and the record are the
  // instance's; the x / y / info rows and the scratch are the position's, taken from blockIdx.x again where they are used.
  // SEL: a template argument, as in k_batch_quad -- without a selection the kernel is the code it was before there was one
  const int pos = blockIdx.x;
  if (pos >= count) return;
  const int inst = SEL ? uni(sel[pos]) : pos;
  const bool res_solve = (res_mode & RES_SOLVE) != 0, res_warm = (res_mode & RES_WARM) != 0;
  double *const rec = res_mode ? rec_all + (size_t)inst * rec_stride : nullptr;  // the instance's state record (resident mode)
  Pattern P = Pin;
  if (CN > 0) { P.n = CN; P.m = CM; P.nnzA = CA; P.nnzF = CF; }
  constexpr bool EXACT = CN > 0 && PARTS * NCT == CN;
  const int n = P.n, m = P.m, tid = mytid();
  // the thread's share of the entries of A as packed words in LDS (both orientations; the positions do not change under
  // scaling, so the walks of the scaling passes use them too: 4 lanes per column, 2 per row)
  const bool regs = sparse_fits(P);
  Lds s = carve((ldouble *)lds_raw, P, regs);
  PROF_DECL
  // ---- stage the shared pattern (16-bit) and load the instance -----------------
  for (int k = tid; k <= n; k += NT) { s.Ap[k] = (unsigned short)P.Ap[k]; s.Fp[k] = (unsigned short)P.Fp[k]; }
  for (int k = tid; k <= m; k += NT) s.Rp[k] = (unsigned short)P.Rp[k];
  for (int k = tid; k < P.nnzA; k += NT) { s.Ai[k] = (unsigned short)P.Ai[k]; s.Rc[k] = (unsigned short)P.Rc[k]; s.Rmap[k] = (unsigned short)P.Rmap[k]; }
  for (int k = tid; k < P.nnzF; k += NT) s.Fc[k] = (unsigned short)P.Fc[k];
  for (int k = tid; k < P.nnzA; k += NT) s.Av[k] = Ax_all[(size_t)inst * P.nnzA + k];
  if (tid == 0) s.Av[P.nnzA] = 0.0;  // what padded entries of the packed words point at
  for (int k = tid; k < P.nnzF; k += NT) s.Pv[k] = Px_all[(size_t)inst * P.nnzP + P.Fmap[k]];
  for (int j = tid; j < n; j += NT) {
    const double x0 = res_warm ? rec[rec_x(n, m) + j] : 0.0;  // the scaled iterate the last solve left (or warm_start wrote)
    s.q[j] = q_all[(size_t)inst * n + j]; s.D[j] = res_solve ? rec[rec_D(n, m) + j] : 1.0; s.x[j] = x0; s.xp[j] = x0; s.dx[j] = 0.0;
  }
  for (int i = tid; i < m; i += NT) {
    s.l[i] = fmax(l_all[(size_t)inst * m + i], -OSQP_INFTY); s.u[i] = fmin(u_all[(size_t)inst * m + i], OSQP_INFTY);
    const double z0 = res_warm ? rec[rec_z(n, m) + i] : 0.0;
    s.E[i] = res_solve ? rec[rec_E(n, m) + i] : 1.0; s.z[i] = z0; s.y[i] = res_warm ? rec[rec_y(n, m) + i] : 0.0; s.zp[i] = z0; s.dy[i] = 0.0;
  }
  // where the epilogue finds the record (0: nothing to leave behind): parked behind the pivot buffers of the inversion
  // instead of scalar registers that would stay live across the whole ADMM loop
  // (and a defined status code for the RES_CERT block of the epilogue, should the loop end before its first residual phase)
  // (behind it, slot 57: the checks the gap test refused, RES_GAP only)
  if (tid == 0) { *(lu64 *)(s.gjc + gjc_parked(kPivotW)) = park_rec(rec, res_mode); s.gjc[gjc_parked(kPivotW) + 1] = 0.0; s.nrm[N_STATUS] = 0.0; }
  __syncthreads();
  PROF(0)
  // ---- K0: Ruiz equilibration + cost scaling --------------------------------
  if (regs) store_sparse(P, s);
  __syncthreads();
  double c = 1.0;
  const int nscale = res_solve ? 0 : (int)st.scaling;  // a resident solve applies the factors of its record instead (below)
  for (int it = 0; it < nscale; it++) {
    if (regs) {
      const ColWords cwd = col_words(s);
      double mx = 0.0;
#pragma unroll
      for (int e = 0; e < KT; e++) mx = fmax(mx, fabs(lds_at(s.Av, cwd.w[e] >> 16)));  // padded entries: |0|
      mx = fmax(mx, quad_xor<2>(mx));
      mx = fmax(mx, quad_xor<1>(mx));
      if ((tid & 3) == 0 && (tid >> 2) < n) {
        const int j = tid >> 2;
        for (int q = s.Fp[j]; q < s.Fp[j + 1]; q++) mx = fmax(mx, fabs(s.Pv[q]));
        s.tn[j] = 1.0 / sqrt(lim(mx));
      }
      const RowWords rwd = row_words(s);
      double mr = 0.0;
#pragma unroll
      for (int e = 0; e < KR; e++) mr = fmax(mr, fabs(lds_at(s.Av, rwd.w[e] >> 16)));
      mr = fmax(mr, quad_xor<1>(mr));
      if ((tid & 1) == 0 && (tid >> 1) < m) s.tm[tid >> 1] = 1.0 / sqrt(lim(mr));
    } else {
    for (int j = tid; j < n; j += NT) {
      double mx = 0.0;
      for (int q = s.Fp[j]; q < s.Fp[j + 1]; q++) mx = fmax(mx, fabs(s.Pv[q]));
      for (int k = s.Ap[j]; k < s.Ap[j + 1]; k++) mx = fmax(mx, fabs(s.Av[k]));
      s.tn[j] = 1.0 / sqrt(lim(mx));
    }
    for (int i = tid; i < m; i += NT) {
      double mx = 0.0;
      for (int q = s.Rp[i]; q < s.Rp[i + 1]; q++) mx = fmax(mx, fabs(s.Av[s.Rmap[q]]));
      s.tm[i] = 1.0 / sqrt(lim(mx));
    }
    }
    __syncthreads();
    for (int r = tid; r < n; r += NT)
      for (int q = s.Fp[r]; q < s.Fp[r + 1]; q++) {
        int cc = s.Fc[q];
        int lo = cc < r ? cc : r, hi = cc < r ? r : cc;
        s.Pv[q] = (s.Pv[q] * s.tn[lo]) * s.tn[hi];
      }
    if (regs) {
      if ((tid >> 2) < n) {
        const double tj = s.tn[tid >> 2];
        const ColWords cwd = col_words(s);
        const unsigned padw = (unsigned)(P.nnzA * 8);
#pragma unroll
        for (int e = 0; e < KT; e++) {
          const unsigned vo = cwd.w[e] >> 16;
          if (vo != padw) *(ldouble *)((lchar *)s.Av + vo) = (lds_at(s.Av, vo) * lds_at(s.tm, cwd.w[e] & 0xFFFFu)) * tj;
        }
      }
      for (int j = tid; j < n; j += NT) { s.q[j] *= s.tn[j]; s.D[j] *= s.tn[j]; }
    } else {
    for (int j = tid; j < n; j += NT) {
      for (int k = s.Ap[j]; k < s.Ap[j + 1]; k++) s.Av[k] = (s.Av[k] * s.tm[s.Ai[k]]) * s.tn[j];
      s.q[j] *= s.tn[j];
      s.D[j] *= s.tn[j];
    }
    }
    for (int i = tid; i < m; i += NT) s.E[i] *= s.tm[i];
    __syncthreads();
    double v[2] = {0.0, 0.0}, w[1] = {0.0};
    for (int j = tid; j < n; j += NT) {
      double mx = 0.0;
      for (int q = s.Fp[j]; q < s.Fp[j + 1]; q++) mx = fmax(mx, fabs(s.Pv[q]));
      w[0] += mx;
      v[0] = fmax(v[0], fabs(s.q[j]));
    }
    {  // the sum and the maximum in one exchange: wavefront reductions, one barrier, the two halves of the upper part of
       // s.red taken in turn so that the pass after next may overwrite what this one reads
      double sm = w[0], mq = v[0];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { sm += __shfl_xor(sm, o, 64); mq = nmax(mq, __shfl_xor(mq, o, 64)); }
      ldouble *rr = s.red + 8 * NW + (it & 1) * 2 * NW;
      if ((tid & 63) == 0) { rr[2 * (tid >> 6)] = sm; rr[2 * (tid >> 6) + 1] = mq; }
      __syncthreads();
      sm = rr[0]; mq = rr[1];
#pragma unroll
      for (int wv = 1; wv < NW; wv++) { sm += rr[2 * wv]; mq = nmax(mq, rr[2 * wv + 1]); }
      w[0] = sm; v[0] = mq;
    }
    double c_temp = w[0] / (double)n;
    c_temp = lim(fmax(c_temp, lim(v[0])));
    c_temp = 1.0 / c_temp;
    for (int k = tid; k < P.nnzF; k += NT) s.Pv[k] *= c_temp;
    for (int j = tid; j < n; j += NT) s.q[j] *= c_temp;
    c *= c_temp;
    __syncthreads();
  }
  if (res_mode & RES_SCALE_ONLY) {  // setup / after a matrix update: D, E, c of this data into the record, no solve
    for (int j = tid; j < n; j += NT) rec[rec_D(n, m) + j] = s.D[j];
    for (int i = tid; i < m; i += NT) rec[rec_E(n, m) + i] = s.E[i];
    if (tid == 0) { rec[REC_C] = c; rec[REC_FLAG] = 1.0; }
    return;
  }
  if (res_solve) {  // the stored factors in one pass over the raw data: P <- c D P D, A <- E A D, q <- c D q
    c = uni(rec[REC_C]);
    for (int r = tid; r < n; r += NT)
      for (int q = s.Fp[r]; q < s.Fp[r + 1]; q++) {
        const int cc = s.Fc[q];
        const int lo = cc < r ? cc : r, hi = cc < r ? r : cc;
        s.Pv[q] = c * ((s.Pv[q] * s.D[lo]) * s.D[hi]);
      }
    for (int j = tid; j < n; j += NT) {
      for (int k = s.Ap[j]; k < s.Ap[j + 1]; k++) s.Av[k] = (s.Av[k] * s.E[s.Ai[k]]) * s.D[j];
      s.q[j] = c * (s.q[j] * s.D[j]);
    }
    __syncthreads();
  }
  const double cinv = 1.0 / c;
  for (int i = tid; i < m; i += NT) { s.l[i] *= s.E[i]; s.u[i] *= s.E[i]; }
  __syncthreads();
  PROF(1)
  // ---- K1, K2 (a resident solve goes on with the rho its last solve ended on) ---
  double rho = uni(fmin(fmax(res_solve ? rec[REC_RHO] : st.rho, B_RHO_MIN), B_RHO_MAX));
  set_rho(P, s, rho, true);
  int status = OSQP_UNSOLVED;
  double *scratch = scratch_all + (size_t)(SEL ? (int)blockIdx.x : inst) * n * n;
  MTile<NCT> Minv;
  // y = A v / y = A' v through whichever walk of A applies
  auto a_rows = [&](const ldouble *v, auto pre, auto finish) {
    if (regs) row_dot(s, v, m, pre, finish);
    else rows_dot<2>(m, s.Rp, [&](int q) { return s.Av[s.Rmap[q]] * v[s.Rc[q]]; }, [&](int r, double a) { finish(r, a, pre(r)); });
  };
  auto a_cols = [&](const ldouble *v, auto pre, auto finish) {
    if (regs) col_dot(s, v, n, pre, finish);
    else rows_dot<4>(n, s.Ap, [&](int k) { return s.Av[k] * v[s.Ai[k]]; }, [&](int r, double a) { finish(r, a, pre(r)); });
  };
  PROF(2)
  const bool uns = st.scaling && !st.scaled_termination;
  const int check = (int)st.check_termination;
  const int rho_interval = st.adaptive_rho ? (st.adaptive_rho_interval ? (int)st.adaptive_rho_interval : 100) : 0;
  const double alpha = st.alpha, sigma = st.sigma;
  double pri_res = 0.0, dua_res = 0.0, obj = 0.0;
  ldouble *nrm = s.nrm;  // the 14 norms of the last residual evaluation (the same in every thread: kept in LDS, not in registers)
  int iter = 0, rho_updates = 0;
  ldouble *x = s.x, *xp = s.xp, *z = s.z, *zp = s.zp;

  // Every phase below appears ONCE in the code (the loop is arranged around that): the kernel is one long function
  // whose register allocation has to hold the inverse (2 NCT registers) across all of it.
  // ---- ADMM loop --------------------------------------------------------------
  const int max_iter = (int)st.max_iter;
  bool need_factor = true;
  for (int i = tid; i < m; i += NT) s.zt[i] = s.rho[i] * z[i] - s.y[i];
  __syncthreads();
  for (iter = 1; iter <= max_iter; iter++) {
    if (need_factor) {  // first iteration and after every rho update
      assemble_scratch(P, s, st.sigma, scratch);
      PROF(8)
      const bool pd = invert_mfma<(NCT <= 16 ? 2 : (NCT <= 25 ? 4 : 5))>(n, scratch, s.gjc);
      load_tile<NCT, EXACT>(n, scratch, Minv);
      if (!pd) { status = OSQP_NON_CVX; iter--; break; }
      need_factor = false;
      PROF(2)
    }
    { ldouble *t = x; x = xp; xp = t; t = z; z = zp; zp = t; }
    // b = sigma x_prev - q + A'(rho z_prev - y); s.zt = rho z_prev - y was left behind by the previous z / y update
    a_cols(s.zt, [&](int j) { return Ops2{xp[j], s.q[j]}; }, [&](int j, double a, const Ops2 &o) { s.bb[j] = sigma * o.a - o.b + a; });
    __syncthreads();
    PROF(3)
    // x~ = M^-1 b: the thread's tile of the inverse against its stretch of b, the four parts of a row add up inside a
    // quad of lanes; the lane that ends up with the row writes x~, x and delta_x
    apply_tile<NCT, EXACT>(n, Minv, s, opaque_s(alpha), xp, x);
    __syncthreads();
    PROF(4)
    // z~ = A x~ row by row, each row finished on the spot: z, y, delta_y and s.zt = rho z - y for the next right-hand side
    a_rows(s.xt, [&](int i) { return Ops6{zp[i], s.y[i], s.rhoi[i], s.l[i], s.u[i], s.rho[i]}; },
           [&](int i, double zt, const Ops6 &o) {
      const double al = opaque_s(alpha);
      const double zh = al * zt + (1.0 - al) * o.a;
      const double yo = o.b;
      const double zn = fmin(fmax(zh + o.c * yo, o.d), o.e);
      z[i] = zn;
      const double d = o.f * (zh - zn);
      s.dy[i] = d; s.y[i] = yo + d;
      s.zt[i] = o.f * zn - (yo + d);
    });
    __syncthreads();
    PROF(5)
    const bool last = iter == max_iter;
    const bool due = check && (iter % check == 0);
    const bool rho_due = rho_interval && (iter % rho_interval == 0);
    if (!(due || rho_due || last)) continue;

    // ---- residual evaluation (K8) and termination tests: a call, not inlined (see residual_phase) ----
    {
      CheckArgs ca;
      ca.n = n; ca.m = m; ca.nnzA = P.nnzA; ca.nnzF = P.nnzF;
      ca.swapped = (x != s.x); ca.uns = uns; ca.words = regs; ca.passes = (due || last) ? (last ? 2 : 1) : 0; ca.last = last;
      ca.ea = st.eps_abs; ca.er = st.eps_rel; ca.epi = st.eps_prim_inf; ca.edi = st.eps_dual_inf; ca.c = c; ca.cinv = cinv;
      residual_phase<CN, CM, CA, CF>(ca);
    }
    bool done = false;
    {
      const int code = (int)nrm[N_STATUS];
      if (code != 0) { status = code; done = true; }
      pri_res = uni(nrm[N_PRI]); dua_res = uni(nrm[N_DUA]); obj = uni(nrm[N_OBJ]);
    }
    PROF(6)
    if (done) break;
    // ---- adaptive rho ----
    if (rho_due) {
      double pr = m == 0 ? 0.0 : nrm[0] / (nmax(nrm[2], nrm[3]) + 1e-10);
      double du = nrm[6] / (nmax(nmax(nrm[8], nrm[9]), nrm[10]) + 1e-10);
      double est = uni(fmin(fmax(rho * sqrt(pr / (du + 1e-10)), B_RHO_MIN), B_RHO_MAX));
      if (est > rho * st.adaptive_rho_tolerance || est < rho / st.adaptive_rho_tolerance) {
        rho = est; rho_updates++;
        set_rho(P, s, rho, false);
        for (int i = mytid(); i < m; i += NT) s.zt[i] = s.rho[i] * z[i] - s.y[i];  // the carried vector follows rho
        __syncthreads();
        need_factor = true;  // picked up at the top of the next iteration
      }
    }
    PROF(7)
  }
  if (iter > max_iter) iter = max_iter;
  PROF_PRINT
  // ---- store -----------------------------------------------------
  const bool has_sol = status == OSQP_SOLVED || status == OSQP_SOLVED_INACCURATE || status == OSQP_MAX_ITER_REACHED;
  const int row = SEL ? (int)blockIdx.x : inst;  // the position (without a selection the same number, and the code as it was)
  for (int j = tid; j < n; j += NT) x_out[(size_t)row * x_stride + j] = has_sol ? s.D[j] * x[j] : NAN;
  for (int i = tid; i < m; i += NT) y_out[(size_t)row * y_stride + i] = has_sol ? cinv * s.E[i] * s.y[i] : NAN;
  if (tid == 0) {
    double *o = info_out + (size_t)row * info_stride;
    o[0] = (double)iter; o[1] = (double)status; o[2] = pri_res; o[3] = dua_res;
    if (info_cols > 4) { o[4] = status == OSQP_NON_CVX ? NAN : obj; o[5] = (double)rho_updates; }
  }
  if (double *const rec = parked_ptr(*(const lu64 *)(s.gjc + gjc_parked(kPivotW)))) {  // the scaled iterate and rho stay: the next solve starts from them
    // (an instance without a solution -- infeasible, non-convex -- starts its next solve from zero, as the oracle's
    // store_solution cold-starts it; rho stays)
    for (int j = tid; j < n; j += NT) rec[rec_x(n, m) + j] = has_sol ? x[j] : 0.0;
    for (int i = tid; i < m; i += NT) { rec[rec_z(n, m) + i] = has_sol ? z[i] : 0.0; rec[rec_y(n, m) + i] = has_sol ? s.y[i] : 0.0; }
    if (tid == 0) { rec[REC_RHO] = rho; rec[REC_FLAG] = 3.0; }
    if (parked_gap(*(const lu64 *)(s.gjc + gjc_parked(kPivotW))) && tid == 0) rec[REC_GAPREF] = s.gjc[gjc_parked(kPivotW) + 1];  // the checks the gap alone refused
  }
  leave_certificate<CN, CM, CA, CF>(n, m, P.nnzA, P.nnzF, regs);
}

}  // namespace
}  // namespace oq
