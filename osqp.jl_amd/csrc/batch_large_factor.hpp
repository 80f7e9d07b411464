// batch_large_factor.hpp -- the second home of the factor of M = P + delta I + Aa' Aa / delta for the polish, adjoint and JVP
// kernels of the resident batch (batch_polish.hpp, batch_adjoint.hpp, batch_jvp.hpp): THE INSTANCE'S n x n BLOCK OF GLOBAL SCRATCH,
// for handles with 128 < n <= 256 whose switch osqp_amd_batch_large_factor is on.  The n <= 128 forms keep M
// in LDS as a packed triangle (263 KB at n = 256: it does not fit); the large forms differ from them in three calls only --
// assemble / cholesky / solve below in place of assemble_M / cholesky / factor_solve -- and in the LDS layout, where the slot of
// M holds the panel instead.  The block is the one k_batch_solve_large inverts M in; nothing reads it after that launch has ended,
// and every launch of these kernels builds its factor anew, so the two never meet.
//
// The block G (column-major, leading dimension n, indexed by LAUNCH POSITION as the solve kernel indexes it):
//   assembly       the LOWER triangle only (entry (i, j), i >= j, at G[i + j n]); the upper triangle is not read before it is
//                  written below;
//   factorisation  BOTH triangles: with L the Cholesky factor and b a block of NB columns starting at j0,
//                    below the diagonal block:  G[i + j n] = L(i, j),  and the mirror G[j + i n] = L(i, j)  (i >= j0 + nb > j >= j0),
//                    the diagonal block:        W = L_bb^-1 (lower triangular) as a symmetric block: G[(j0 + r) + (j0 + c) n] =
//                                               W(max(r, c), min(r, c)) -- L_bb itself is not kept;
//                  so that BOTH substitutions walk columns of G with one thread per row: consecutive lanes on consecutive doubles.
//
// Factorisation: blocked, right-looking.  A panel of NB columns (rows j0 .. n) is staged in LDS and factorised there column by
// column (two LDS barriers per column, as cholesky of batch_polish.hpp does for the whole matrix); then, out of the LDS panel
// and without a barrier between them, NB threads invert the diagonal block, all threads write the panel and its mirror back,
// and all threads update the trailing lower triangle in global memory: entry (i, j) by ONE thread, its NB products summed in
// column order and taken off G once -- a fixed order, the same bits in every call.  One barrier ends the block.  Global memory
// is touched n / NB times per entry instead of once per column.
//
// Substitutions (solve): t <- M^-1 t in n / NB block steps per direction.  A block step is w_b = W t_b (a thread per row of the
// block, NB multiply-adds on loads that do not depend on each other), a barrier, then t_i -= sum_c G[i + (j0 + c) n] w_c for every
// row i beyond the block (forward) or before it (backward; the mirror), a thread per row, and a barrier.  The dependent chain of
// one solve is 2 ceil(n / NB) block steps = 4 ceil(n / NB) barriers (32 at n = 256), each behind one round of global loads, in
// place of 2 n scalar steps.
#pragma once
#include "batch_common.hpp"

namespace oq {
namespace {
namespace polish {
namespace lf {

constexpr int LT = 256;  // threads per workgroup: PT of batch_polish.hpp (asserted there); one thread per row of G
constexpr int NB = 32;   // columns per panel
constexpr int kMaxN = 256;
static_assert(kMaxN <= LT, "a thread per row");

// LDS, in doubles, in the slot M has in the n <= 128 layout: the panel [NB columns x ld], ld = n | 1 (odd: the write-back of the
// mirror walks a row of the panel, and an even stride would put it on one bank), the pivots of the panel [NB], the inverse of
// the diagonal block while it is formed [NB x NB], the block result of a substitution step [NB]
__host__ __device__ constexpr int panel_ld(int n) { return n | 1; }
__host__ __device__ constexpr int lds_doubles(int n) { return NB * panel_ld(n) + NB + NB * NB + NB; }
struct Work { ldouble *panel, *dg, *inv, *wb; int ld; };
__device__ __forceinline__ Work make_work(ldouble *base, int n) {
  const int ld = panel_ld(n);
  return Work{base, base + NB * ld, base + NB * ld + NB, base + NB * ld + NB + NB * NB, ld};
}

// M = P + delta I + Aa' Aa / delta into the lower triangle of G: the formulas and the order of assemble_M (batch_polish.hpp).
// Av, Pv and act are written but not yet synchronised on entry.
__device__ __forceinline__ void assemble(const Pattern &P, const ldouble *Av, const ldouble *Pv, const ldouble *act, double delta, double *G) {
  const int tid = threadIdx.x, n = P.n;
  for (int j = 0; j < n; j++)
    for (int i = j + tid; i < n; i += LT) G[i + (size_t)j * n] = 0.0;
  __syncthreads();
  for (int p = tid; p < P.npair; p += LT) {
    double acc = 0.0;
    for (int s = P.Tp[p]; s < P.Tp[p + 1]; s++) acc += (act[P.Tr[s]] != 0.0 ? 1.0 : 0.0) * Av[P.Ta[s]] * Av[P.Tb[s]];
    G[P.Ti[p] + (size_t)P.Tj[p] * n] = acc / delta;
  }
  __syncthreads();  // (the read-modify-writes below meet entries other threads wrote: see VISIBILITY in cholesky)
  for (int r = tid; r < n; r += LT) {
    for (int f = P.Fp[r]; f < P.Fp[r + 1]; f++) {
      const int cc = P.Fc[f];
      if (cc <= r) G[r + (size_t)cc * n] += Pv[f];
    }
    G[r + (size_t)r * n] += delta;
  }
  __syncthreads();
}

// The blocked Cholesky of G, as the file header lays it out.  false: a non-positive pivot (the same value in every thread: a
// uniform exit; G is left half-way, nobody reads it).
__device__ __forceinline__ bool cholesky(int n, double *G, const Work &w) {
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, ld = w.ld;
  ldouble *const pn = w.panel;
  for (int j0 = 0; j0 < n; j0 += NB) {
    const int nb = n - j0 < NB ? n - j0 : NB, end = j0 + nb;
    // ---- stage rows j0 .. n of the block's columns (lower part).  VISIBILITY: these are plain vector loads (a per-lane
    // address: never a scalar load, whose cache vector stores do not reach; G is not const, not __restrict__, nothing is marked
    // invariant or non-temporal) of what the trailing update of the block before -- or assemble -- stored: vector stores of
    // the four wavefronts of THIS workgroup, which run on one compute unit and go through its one write-through vector cache,
    // where a store updates the line it hits on its way to L2.  Between those stores and these loads stands a __syncthreads():
    // a workgroup-scope release (every store acknowledged), the barrier, a workgroup-scope acquire.  Nothing outside the
    // workgroup writes the block during a launch ("Visibility of a new inverse").
    {
      const int i = j0 + tid;
      if (i < n)
        for (int c = 0; c < nb; c++)
          if (i >= j0 + c) pn[i + c * ld] = G[i + (size_t)(j0 + c) * n];
    }
    __syncthreads();
    // ---- the panel, column by column, in LDS ----
    for (int k = 0; k < nb; k++) {
      const double d = pn[(j0 + k) + k * ld];  // final since the barrier that ended step k - 1; not written in step k
      if (!(d > 0.0)) return false;
      const double piv = sqrt(d);
      if (tid == 0) w.dg[k] = piv;
      for (int i = j0 + k + 1 + tid; i < n; i += LT) pn[i + k * ld] = pn[i + k * ld] / piv;
      __syncthreads();
      {
        const int i = j0 + tid;  // a thread per row: its entries of the columns k + 1 .. nb
        if (i > j0 + k && i < n) {
          const double ci = pn[i + k * ld];
          const int cmax = i - j0 < nb - 1 ? i - j0 : nb - 1;
          for (int c = k + 1; c <= cmax; c++) pn[i + c * ld] -= ci * pn[(j0 + c) + k * ld];
        }
      }
      __syncthreads();
    }
    // ---- out of the finished panel, no barrier between the three: (a) W = L_bb^-1, a thread per column, into the diagonal
    // block of G (both halves); (b) the panel below the block and its mirror into G; (c) the trailing update ----
    if (tid < nb) {
      const int c = tid;
      ldouble *const col = w.inv + c * NB;  // this thread's column: it reads back only what it wrote itself
      for (int r = c; r < nb; r++) {
        double v;
        if (r == c) v = 1.0 / w.dg[c];
        else {
          double s = 0.0;
          for (int k = c; k < r; k++) s = __builtin_fma(pn[(j0 + r) + k * ld], col[k], s);
          v = -s / w.dg[r];
        }
        col[r] = v;
        G[(j0 + r) + (size_t)(j0 + c) * n] = v;
        G[(j0 + c) + (size_t)(j0 + r) * n] = v;
      }
    }
    if (end < n) {
      {
        const int i = end + tid;
        if (i < n)
          for (int c = 0; c < nb; c++) G[i + (size_t)(j0 + c) * n] = pn[i + c * ld];
      }
      for (int e = tid; e < (n - end) * nb; e += LT) {  // the mirror: row j0 + c of column i, nb consecutive doubles
        const int c = e % nb, i = end + e / nb;
        G[(j0 + c) + (size_t)i * n] = pn[i + c * ld];
      }
      // (c) entry (i, j), end <= j <= i < n, by one thread: 64 x 64 tiles, a thread takes rows ib + tx + 16 a and columns
      // jb + ty + 16 b (a, b < 4).  Indices beyond n are clamped for the loads and dropped at the store.
      for (int jb = end; jb < n; jb += 64)
        for (int ib = jb; ib < n; ib += 64) {
          int ri[4], rj[4];
#pragma unroll
          for (int a = 0; a < 4; a++) {
            const int i = ib + tx + 16 * a, j = jb + ty + 16 * a;
            ri[a] = i < n ? i : n - 1; rj[a] = j < n ? j : n - 1;
          }
          double acc[4][4];
#pragma unroll
          for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) acc[a][b] = 0.0;
          for (int k = 0; k < nb; k++) {
            double va[4], vb[4];
#pragma unroll
            for (int a = 0; a < 4; a++) { va[a] = pn[ri[a] + k * ld]; vb[a] = pn[rj[a] + k * ld]; }
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
              for (int b = 0; b < 4; b++) acc[a][b] = __builtin_fma(va[a], vb[b], acc[a][b]);
          }
#pragma unroll
          for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
              const int i = ib + tx + 16 * a, j = jb + ty + 16 * b;
              if (i < n && j <= i) G[i + (size_t)j * n] -= acc[a][b];
            }
        }
    }
    __syncthreads();
  }
  return true;
}

// t <- M^-1 t (t: n doubles of LDS, complete and synchronised on entry; complete and synchronised on return) through the factor
// in G: forward L w = t over the blocks upwards, then backward L' x = w over them downwards.
__device__ __forceinline__ void solve(int n, const double *G, const Work &w, ldouble *t) {
  const int tid = threadIdx.x;
  const int nblk = (n + NB - 1) / NB;
  for (int pass = 0; pass < 2; pass++)
    for (int s = 0; s < nblk; s++) {
      const int j0 = (pass == 0 ? s : nblk - 1 - s) * NB;
      const int nb = n - j0 < NB ? n - j0 : NB, end = j0 + nb;
      // VISIBILITY of the factor (written by cholesky above, in this launch, by the wavefronts of THIS workgroup): plain
      // vector loads with a per-lane address -- not scalar, not invariant, not non-temporal -- behind the __syncthreads() that
      // ended cholesky; the argument is the one stated at the panel stage there and in DESIGN.md section 13.1.
      if (tid < nb) {  // w_b = W t_b (forward: the lower half of the symmetric block, backward: its upper half = W')
        const double *const row = G + (j0 + tid) + (size_t)j0 * n;
        const int c0 = pass == 0 ? 0 : tid, c1 = pass == 0 ? tid : nb - 1;
        double a = 0.0;
        for (int c = 0; c < nb; c += 8) {  // eight loads in flight, then the multiply-adds of this lane's columns in index order
          double v[8], tc[8];
#pragma unroll
          for (int u = 0; u < 8; u++) {
            const bool on = c + u >= c0 && c + u <= c1;
            v[u] = on ? row[(size_t)(c + u) * n] : 0.0;
            tc[u] = on ? t[j0 + c + u] : 0.0;
          }
#pragma unroll
          for (int u = 0; u < 8; u++)
            if (c + u >= c0 && c + u <= c1) a = __builtin_fma(v[u], tc[u], a);
        }
        w.wb[tid] = a;
      }
      __syncthreads();
      if (tid < n) {
        const int i = tid;
        if (i >= j0 && i < end) t[i] = w.wb[i - j0];
        else if (pass == 0 ? i >= end : i < j0) {
          const double *const row = G + i + (size_t)j0 * n;
          double a = t[i];
          int c = 0;
          for (; c + 8 <= nb; c += 8) {  // eight loads in flight; the sum stays in column order
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = row[(size_t)(c + u) * n];
#pragma unroll
            for (int u = 0; u < 8; u++) a = __builtin_fma(-v[u], w.wb[c + u], a);
          }
          for (; c < nb; c++) a = __builtin_fma(-row[(size_t)c * n], w.wb[c], a);
          t[i] = a;
        }
      }
      __syncthreads();
    }
}

}  // namespace lf
}  // namespace polish
}  // namespace
}  // namespace oq
