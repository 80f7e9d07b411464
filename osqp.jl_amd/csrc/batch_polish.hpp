// batch_polish.hpp -- solution polishing for the resident batch (osqp_amd_batch_resolve with settings.polish = 1): a kernel
// of its own, launched after the ADMM launch.  The semantics are polish() / form_Ared() of oracle/osqp_oracle.c, instance by
// instance, in the SCALED space: the record row (batch_common.hpp) holds c, D, E and the scaled x, z, y the solve left, the
// handle holds the raw data, and D, E, c are applied on the fly exactly as the solve kernels' prologue applies them.
//
// One workgroup (PT threads) per instance; only instances whose ADMM status is Solved do anything.  The regularised KKT
// system [P + delta I, Aa'; Aa, -delta I] (Aa: the active rows) is solved in its condensed form -- the constraint block
// eliminated exactly:
//     M = P + delta I + (1 / delta) Aa' Aa     (n x n, symmetric positive definite)
//     d_x = M^-1 (r_x + Aa' r_y / delta),   d_y = (Aa d_x - r_y) / delta
// which is the matrix the batched path assembles for ADMM with sigma -> delta and rho_i -> 1 / delta on the active rows, 0
// elsewhere: the term lists of A' diag(.) A and the full-P CSR of the shared pattern are reused.  The full (n + m_act)-square
// matrix would not fit the LDS (the MPC family has >= 60 active rows on n = 100); M does for every n <= 128.
//
// LDS (doubles; make_layout): M as a packed lower triangle, row-major (entry (i, j), i >= j, at i (i + 1) / 2 + j: a row of
// the factor is contiguous -- the backward substitution and the trailing update walk rows with consecutive lanes on
// consecutive words), the scaled values of A and of the full P, 1 / pivot [n], the pivot column [n], q, x, t (right-hand side
// / correction) [n each], l, u, y, r_y, z, act [m each], and a small block for reductions.  Nothing of an instance touches
// global scratch.  tests/batch_polish_ref.py is the numpy model of this file.
//
// LARGE (a template argument of the three kernels and of kkt_step; handles with 128 < n <= 256 and osqp_amd_batch_large_factor
// on): M and its factor live in the n x n block of global scratch of the launch position instead
// (batch_large_factor.hpp: lf::assemble, lf::cholesky, lf::solve in place of assemble_M, cholesky, factor_solve), and the slot
// of M in the layout holds that file's panel.  Everything else is this file's code, instantiated twice.
#pragma once
#include "batch_common.hpp"
#include "batch_large_factor.hpp"

namespace oq {
namespace {
namespace polish {

constexpr int PT = 256;  // threads per workgroup
constexpr int PW = PT / 64;
static_assert(PT == lf::LT, "batch_large_factor.hpp deals its rows to the threads of these kernels");

struct Layout { int M, Av, Pv, rdg, col, q, x, t, l, u, y, ry, z, act, red, total; };  // offsets in doubles; total in bytes
inline Layout make_layout(int n, int m, int nnzA, int nnzF, bool large = false) {  // large: the panel of lf:: in the slot of M
  Layout L;
  int o = 0;
  auto take = [&o](int k) { const int at = o; o += (k + 1) & ~1; return at; };
  L.M = take(large ? lf::lds_doubles(n) : n * (n + 1) / 2); L.Av = take(nnzA); L.Pv = take(nnzF);
  L.rdg = take(n); L.col = take(n); L.q = take(n); L.x = take(n); L.t = take(n);
  L.l = take(m); L.u = take(m); L.y = take(m); L.ry = take(m); L.z = take(m); L.act = take(m);
  L.red = take(4 * PW);
  L.total = o * (int)sizeof(double);
  return L;
}
constexpr int kLdsLimit = 160 * 1024;

struct Args {
  const double *Px, *Ax, *q, *l, *u;
  double *x, *y, *info, *rec, *status;
  int x_stride, y_stride, info_stride, rec_stride;
  int refine, unscaled;  // unscaled: scaling on and scaled_termination off (residuals in the caller's units)
  double delta;
  const int *sel;  // the instance of each workgroup (nullptr: its own number); the x / y / info rows are the workgroups'
  double *scratch = nullptr;  // LARGE: n x n doubles per launch position (the handle's solve scratch)
};

__device__ __forceinline__ int tri(int i, int j) { return ((i * (i + 1)) >> 1) + j; }  // i >= j

// max / max / sum over the workgroup of (a, b, c); every thread gets the results.  NaN propagates through the maxima.
__device__ __forceinline__ void reduce3(ldouble *red, double &a, double &b, double &c) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { a = nmax(a, __shfl_xor(a, o, 64)); b = nmax(b, __shfl_xor(b, o, 64)); c += __shfl_xor(c, o, 64); }
  __syncthreads();  // whoever still reads the block of an earlier reduction
  if ((tid & 63) == 0) { red[3 * (tid >> 6)] = a; red[3 * (tid >> 6) + 1] = b; red[3 * (tid >> 6) + 2] = c; }
  __syncthreads();
  a = red[0]; b = red[1]; c = red[2];
#pragma unroll
  for (int w = 1; w < PW; w++) { a = nmax(a, red[3 * w]); b = nmax(b, red[3 * w + 1]); c += red[3 * w + 2]; }
}

// t <- M^-1 t through the Cholesky factor in LDS, by the first wavefront: lane L holds entries L and L + 64 of the vector in
// registers; step k hands the finished entry round (one cross-lane read) and takes one column (forward: L w = t) or one row
// (backward: L' x = w) of the factor out of the rest.  The other wavefronts wait at the caller's barrier.
__device__ __forceinline__ void factor_solve(int n, const ldouble *M, const ldouble *rdg, ldouble *t) {
  const int lane = threadIdx.x;
  if (lane >= 64) return;
  const int i0 = lane, i1 = lane + 64;
  double b0 = i0 < n ? t[i0] : 0.0, b1 = i1 < n ? t[i1] : 0.0;
  for (int k = 0; k < n; k++) {
    const double m0 = (i0 > k && i0 < n) ? M[tri(i0, k)] : 0.0, m1 = (i1 > k && i1 < n) ? M[tri(i1, k)] : 0.0;
    const double wk = __shfl(k < 64 ? b0 : b1, k & 63, 64) * rdg[k];
    if (lane == (k & 63)) { if (k < 64) b0 = wk; else b1 = wk; }
    b0 -= m0 * wk; b1 -= m1 * wk;
  }
  for (int k = n - 1; k >= 0; k--) {
    const double m0 = i0 < k ? M[tri(k, i0)] : 0.0, m1 = i1 < k ? M[tri(k, i1)] : 0.0;
    const double xk = __shfl(k < 64 ? b0 : b1, k & 63, 64) * rdg[k];
    if (lane == (k & 63)) { if (k < 64) b0 = xk; else b1 = xk; }
    b0 -= m0 * xk; b1 -= m1 * xk;
  }
  if (i0 < n) t[i0] = b0;
  if (i1 < n) t[i1] = b1;
}

// ---- what k_batch_polish and k_batch_adjoint (batch_adjoint.hpp) share: the views of the LDS slots, the scaled matrices, the
// classification of a row, the assembly of M, its factorisation and one solve / refinement step ----
struct Slots { ldouble *M, *Av, *Pv, *rdg, *col, *q, *x, *t, *l, *u, *y, *ry, *z, *act, *red; double *G; };  // G: LARGE only
__device__ __forceinline__ Slots make_slots(const Layout &L) {
  ldouble *const lds = (ldouble *)lds_raw;
  return Slots{lds + L.M, lds + L.Av, lds + L.Pv, lds + L.rdg, lds + L.col, lds + L.q, lds + L.x, lds + L.t,
               lds + L.l, lds + L.u, lds + L.y, lds + L.ry, lds + L.z, lds + L.act, lds + L.red, nullptr};
}

// column j of the scaled A and row j of the scaled full P (as the solve prologue forms them) into Av / Pv
__device__ __forceinline__ void stage_matrices(const Pattern &P, const Slots &S, int j, const double *Axi, const double *Pxi, const double *D,
                                               const double *E, double c) {
  const double dj = D[j];
  for (int k = P.Ap[j]; k < P.Ap[j + 1]; k++) S.Av[k] = (Axi[k] * E[P.Ai[k]]) * dj;
  for (int f = P.Fp[j]; f < P.Fp[j + 1]; f++) {
    const int cc = P.Fc[f];
    const int lo = cc < j ? cc : j, hi = cc < j ? j : cc;
    S.Pv[f] = c * ((Pxi[P.Fmap[f]] * D[lo]) * D[hi]);
  }
}
// -1 lower, 1 upper, 0 inactive, on the scaled iterate: lower first, as form_Ared
__device__ __forceinline__ double classify(double zi, double yi, double li, double ui) {
  return (zi - li < -yi) ? -1.0 : ((ui - zi < yi) ? 1.0 : 0.0);
}

// M = P + delta I + Aa' Aa / delta, lower triangle; Av, Pv and act are written but not yet synchronised on entry
__device__ __forceinline__ void assemble_M(const Pattern &P, const Slots &S, double delta) {
  const int tid = threadIdx.x, n = P.n;
  ldouble *const M = S.M;
  for (int e = tid; e < n * (n + 1) / 2; e += PT) M[e] = 0.0;
  __syncthreads();
  for (int p = tid; p < P.npair; p += PT) {
    double acc = 0.0;
    for (int s = P.Tp[p]; s < P.Tp[p + 1]; s++) acc += (S.act[P.Tr[s]] != 0.0 ? 1.0 : 0.0) * S.Av[P.Ta[s]] * S.Av[P.Tb[s]];
    M[tri(P.Ti[p], P.Tj[p])] = acc / delta;
  }
  __syncthreads();
  for (int r = tid; r < n; r += PT) {
    for (int f = P.Fp[r]; f < P.Fp[r + 1]; f++) {
      const int cc = P.Fc[f];
      if (cc <= r) M[tri(r, cc)] += S.Pv[f];
    }
    M[tri(r, r)] += delta;
  }
  __syncthreads();
}

// Cholesky, right-looking, in place (the diagonal of M keeps the pivot's square; 1 / pivot goes to rdg); false: a
// non-positive pivot (the same value in every thread: a uniform exit)
__device__ __forceinline__ bool cholesky(int n, ldouble *M, ldouble *rdg, ldouble *col) {
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  for (int k = 0; k < n; k++) {
    const double d = M[tri(k, k)];  // final since the barrier that ended step k - 1; not written in step k
    if (!(d > 0.0)) return false;
    const double piv = sqrt(d);
    if (tid == 0) rdg[k] = 1.0 / piv;
    for (int i = k + 1 + tid; i < n; i += PT) { const double v = M[tri(i, k)] / piv; M[tri(i, k)] = v; col[i] = v; }
    __syncthreads();
    for (int i = k + 1 + ty; i < n; i += 16) {
      const double ci = col[i];
      for (int j = k + 1 + tx; j <= i; j += 16) M[tri(i, j)] -= ci * col[j];
    }
    __syncthreads();
  }
  return true;
}
// M and its factor where the instantiation keeps them: false as cholesky
template <bool LARGE>
__device__ __forceinline__ bool assemble_and_factor(const Pattern &P, const Slots &S, double delta) {
  if constexpr (LARGE) {
    lf::assemble(P, S.Av, S.Pv, S.act, delta, S.G);
    return lf::cholesky(P.n, S.G, lf::make_work(S.M, P.n));
  } else {
    assemble_M(P, S, delta);
    return cholesky(P.n, S.M, S.rdg, S.col);
  }
}

// One solve with the factor: step `it` = 0 solves [P + delta I, Aa'; Aa, -delta I] [x; y] = [g; b] from the ry the caller
// staged (b on the active rows, zero elsewhere); a step it > 0 refines x, y against the unregularised [P, Aa'; Aa, 0].
// POLISH: g = -q and b = l on the lower rows, u on the upper ones; otherwise (the adjoint) g = q and b = l on every active row.
template <bool POLISH, bool LARGE>
__device__ __forceinline__ void kkt_step(const Pattern &P, const Slots &S, int it, double delta) {
  const int tid = threadIdx.x, n = P.n, m = P.m;
  ldouble *const Av = S.Av, *const Pv = S.Pv, *const x = S.x, *const y = S.y, *const t = S.t, *const ry = S.ry, *const act = S.act;
  if (it > 0) {  // r_y = b - Aa x on the active rows (zero elsewhere, so the column walks need no mask)
    for (int i = tid; i < m; i += PT) {
      const double on = act[i];
      double ax = 0.0;
      if (on != 0.0) for (int s = P.Rp[i]; s < P.Rp[i + 1]; s++) ax += Av[P.Rmap[s]] * x[P.Rc[s]];
      ry[i] = on != 0.0 ? ((on < 0.0 || !POLISH) ? S.l[i] : S.u[i]) - ax : 0.0;
    }
    __syncthreads();
  }
  for (int j = tid; j < n; j += PT) {  // t = r_x + Aa' r_y / delta,  r_x = g - P x - Aa' y (first solve: g)
    double rx = POLISH ? -S.q[j] : S.q[j], ar = 0.0;
    if (it > 0) {
      double px = 0.0, ay = 0.0;
      for (int f = P.Fp[j]; f < P.Fp[j + 1]; f++) px += Pv[f] * x[P.Fc[f]];
      for (int k = P.Ap[j]; k < P.Ap[j + 1]; k++) ay += Av[k] * y[P.Ai[k]];
      rx = (rx - px) - ay;
    }
    for (int k = P.Ap[j]; k < P.Ap[j + 1]; k++) ar += Av[k] * ry[P.Ai[k]];
    t[j] = rx + ar / delta;
  }
  __syncthreads();
  if constexpr (LARGE) lf::solve(n, S.G, lf::make_work(S.M, n), t);
  else factor_solve(n, S.M, S.rdg, t);
  __syncthreads();
  for (int i = tid; i < m; i += PT) {  // d_y = (Aa d_x - r_y) / delta
    if (act[i] == 0.0) continue;
    double ad = 0.0;
    for (int s = P.Rp[i]; s < P.Rp[i + 1]; s++) ad += Av[P.Rmap[s]] * t[P.Rc[s]];
    const double dy = (ad - ry[i]) / delta;
    y[i] = it > 0 ? y[i] + dy : dy;
  }
  for (int j = tid; j < n; j += PT) x[j] = it > 0 ? x[j] + t[j] : t[j];
  __syncthreads();
}

template <bool LARGE>
__global__ __launch_bounds__(PT) void k_batch_polish(Pattern P, int count, Layout L, Args a) {
  const int pos = blockIdx.x, tid = threadIdx.x, n = P.n, m = P.m;
  if (pos >= count) return;
  const int inst = a.sel ? a.sel[pos] : pos;
  double *const info = a.info + (size_t)pos * a.info_stride;
  if ((int)info[1] != OSQP_SOLVED) {  // nothing to polish: x, y, info and the record stay as the solve left them
    if (tid == 0) a.status[inst] = 0.0;
    return;
  }
  Slots S = make_slots(L);
  if constexpr (LARGE) S.G = a.scratch + (size_t)pos * n * n;
  ldouble *const Av = S.Av, *const Pv = S.Pv, *const q = S.q, *const x = S.x, *const l = S.l, *const u = S.u;
  ldouble *const y = S.y, *const ry = S.ry, *const z = S.z, *const act = S.act, *const red = S.red;
  double *const rec = a.rec + (size_t)inst * a.rec_stride;
  const double *const D = rec + rec_D(n, m), *const E = rec + rec_E(n, m);
  const double c = rec[REC_C], cinv = 1.0 / c, delta = a.delta;
  const double pri0 = info[2], dua0 = info[3];

  // ---- the scaled data (as the solve prologue forms them), the iterate of the record, the active sets ----
  const double *const Axi = a.Ax + (size_t)inst * P.nnzA, *const Pxi = a.Px + (size_t)inst * P.nnzP;
  for (int j = tid; j < n; j += PT) {
    stage_matrices(P, S, j, Axi, Pxi, D, E, c);
    q[j] = c * (a.q[(size_t)inst * n + j] * D[j]);
    x[j] = rec[rec_x(n, m) + j];
  }
  for (int i = tid; i < m; i += PT) {
    const double e = E[i];
    const double li = fmax(a.l[(size_t)inst * m + i], -OSQP_INFTY) * e, ui = fmin(a.u[(size_t)inst * m + i], OSQP_INFTY) * e;
    const double zi = rec[rec_z(n, m) + i], yi = rec[rec_y(n, m) + i];
    l[i] = li; u[i] = ui;
    const double on = classify(zi, yi, li, ui);
    act[i] = on;
    ry[i] = on < 0.0 ? li : (on > 0.0 ? ui : 0.0);  // the right-hand side of the first solve: [-q; l_low; u_upp]
    y[i] = 0.0;
  }
  if (!assemble_and_factor<LARGE>(P, S, delta)) {  // as a failed direct_init in the oracle
    if (tid == 0) a.status[inst] = -1.0;
    return;
  }

  // ---- solve with [-q; b_act], then `refine` steps against the unregularised [P, Aa'; Aa, 0] ----
  for (int it = 0; it <= a.refine; it++) kkt_step<true, LARGE>(P, S, it, delta);

  // ---- z = A x, (z, y) onto the normal cone of [l, u]; residuals and objective as the termination check defines them ----
  double pri = 0.0, dua = 0.0, obj = 0.0;
  for (int i = tid; i < m; i += PT) {
    double ax = 0.0;
    for (int s = P.Rp[i]; s < P.Rp[i + 1]; s++) ax += Av[P.Rmap[s]] * x[P.Rc[s]];
    const double sum = ax + y[i];
    const double zc = fmin(fmax(sum, l[i]), u[i]);
    z[i] = zc; y[i] = sum - zc;
    const double rp = ax - zc;
    pri = nmax(pri, fabs(a.unscaled ? rp / E[i] : rp));
  }
  __syncthreads();
  for (int j = tid; j < n; j += PT) {
    double px = 0.0, ay = 0.0;
    for (int f = P.Fp[j]; f < P.Fp[j + 1]; f++) px += Pv[f] * x[P.Fc[f]];
    for (int k = P.Ap[j]; k < P.Ap[j + 1]; k++) ay += Av[k] * y[P.Ai[k]];
    const double rd = (px + q[j]) + ay;
    dua = nmax(dua, fabs(a.unscaled ? rd / D[j] : rd));
    obj += x[j] * (0.5 * px + q[j]);
  }
  reduce3(red, pri, dua, obj);
  if (a.unscaled) dua *= cinv;
  obj *= cinv;

  // ---- acceptance: lines 635-637 of the oracle ----
  const bool ok = (pri < pri0 && dua < dua0) || (pri < pri0 && dua0 < 1e-10) || (dua < dua0 && pri0 < 1e-10);
  if (!ok) {
    if (tid == 0) a.status[inst] = -1.0;
    return;
  }
  for (int j = tid; j < n; j += PT) { a.x[(size_t)pos * a.x_stride + j] = D[j] * x[j]; rec[rec_x(n, m) + j] = x[j]; }
  for (int i = tid; i < m; i += PT) {
    a.y[(size_t)pos * a.y_stride + i] = cinv * E[i] * y[i];
    rec[rec_z(n, m) + i] = z[i]; rec[rec_y(n, m) + i] = y[i];
  }
  if (tid == 0) { info[2] = pri; info[3] = dua; info[4] = obj; a.status[inst] = 1.0; }
}

}  // namespace polish
}  // namespace
}  // namespace oq
