// batch_shared.hpp -- the shared batch (osqp_amd_shared_batch_*): ONE MODEL (P, A, settings) AND MANY
// RIGHT-HAND SIDES.  Instance i is osqp_setup(P, q0, A, l0, u0), osqp_update_lin_cost(q_i), osqp_update_bounds(l_i, u_i),
// osqp_solve: the scaling D, E, c comes from the base data, rho is fixed (adaptive_rho = 0) and every row of every instance has
// the kind (loose / equality / inequality) it has under (l0, u0) -- so M = P + sigma I + A' diag(rho) A and its inverse are the
// same for all instances, and x~ = M^-1 b for T instances is a product M^-1 [n x n] . B [n x T] on the fp64 matrix cores.
//   k_shared_factor        one workgroup, at setup and after a rho update: the Ruiz passes and the cost scaling of
//                          k_batch_solve_large's K0 on the base data, set_rho, assemble_scratch, invert_mfma (the existing
//                          device functions, GW = kLargeW), then the MODEL BLOCK in global memory (ModelLayout below);
//   k_batch_solve_shared   the whole ADMM solve of a TILE of T instances per 512-thread workgroup: phases, formulas and order
//                          of k_batch_solve_large, the per-instance vectors as [. x T] arrays (entry idx of column c at
//                          idx T + c), the dense step v_mfma_f64_16x16x4_f64 on 16-row tiles of M^-1 read from the model block;
//   k_shared_put / _warm / _check_bounds   the small kernels of the updates.
// The adjoint of the handle (k_shared_adjoint, k_shared_reduce_rows) reads the model block and the tile records laid out here:
// batch_shared_adjoint.hpp, DESIGN.md section 13.4.
// WHERE THE VECTORS LIVE.  LDS holds what an iteration reads more than once or with scattered addresses: the scaled values
// of A, rho and 1 / rho (shared), and per tile b (padded to a multiple of 16 rows, the padding zero), x~, x, z, y and
// zt = rho z - y.  q, l and u are read once per iteration, entry idx T + c by the thread that owns it: they stay in the TILE
// RECORD in global memory (TileLayout), which also keeps the iterate x, z, y between solves and delta_x / delta_y, written
// at the iterations that end in a check only.  P is needed by the checks alone and is read from the model block there.
// INDEPENDENCE.  Every sum that belongs to one instance is formed by one thread (a row or a column of A walked in index
// order), by the matrix cores over k = 0, 1, ... in that order, or by one wavefront (lane l takes entries l, l + 64, ...; then
// an xor butterfly): the column index c enters addresses only, never an order.  An instance has the same bits whatever
// `count` is, wherever it sits in the batch and whatever its neighbours hold.
#pragma once
#include "batch_large.hpp"

namespace oq {
namespace {
namespace shared {

constexpr int kMaxN = kLargeMaxN;
constexpr int kTileSizes[3] = {16, 8, 4};  // T: the largest whose LDS layout fits (shared_plan in batch.hip)
constexpr int kLastKernel = -3;            // osqp_amd_batch_last_kernel after a shared launch

// ---- the model block, in doubles: [ c | rho | pd | - x 5 | D[n] | E[m] | rho[m] | 1 / rho[m] | Av[nnzA + 1] (CSC order, a zero
// behind) | Pv[nnzF] (full symmetric, CSR order) | M^-1 [ldm x ldm] column-major, both triangles, ldm = 16 ceil(n / 16), rows
// and columns >= n zero | ctype[m] (ints: -1 loose, 1 equality, 0 inequality) ]
enum { MB_C = 0, MB_RHO = 1, MB_PD = 2, MB_HDR = 8 };
struct ModelLayout { size_t D, E, rho, rhoi, Av, Pv, Minv, ctype, total; int ldm; };
__host__ __device__ inline ModelLayout model_layout(int n, int m, int nnzA, int nnzF) {
  ModelLayout L;
  size_t o = MB_HDR;
  L.ldm = (n + 15) & ~15;
  L.D = o; o += n; L.E = o; o += m; L.rho = o; o += m; L.rhoi = o; o += m;
  L.Av = o; o += (size_t)nnzA + 1; L.Pv = o; o += nnzF; o += o & 1;
  L.Minv = o; o += (size_t)L.ldm * L.ldm;
  L.ctype = o; o += ((size_t)m + 1) / 2;
  L.total = o;
  return L;
}
// ---- the record of a tile, in doubles: q, l, u (scaled), the scaled iterate x, z, y, delta_x, delta_y -- each [len x T]
struct TileLayout { size_t q, l, u, x, z, y, dx, dy, total; };
__host__ __device__ inline TileLayout tile_layout(int n, int m, int T) {
  TileLayout L;
  const size_t nt = (size_t)n * T, mt = (size_t)m * T;
  L.q = 0; L.l = nt; L.u = nt + mt; L.x = nt + 2 * mt; L.z = 2 * nt + 2 * mt; L.y = 2 * nt + 3 * mt; L.dx = 2 * nt + 4 * mt; L.dy = 3 * nt + 4 * mt;
  L.total = 3 * nt + 5 * mt;
  return L;
}
// ---- LDS of k_batch_solve_shared: doubles (Av, rho, rhoi | bb, xt, x, z, y, zt | res[16 x 4]), then the 16-bit pattern
__host__ __device__ inline size_t lds_doubles(int n, int m, int nnzA, int T) {
  const int ldm = (n + 15) & ~15;
  return (size_t)nnzA + 1 + 2 * (size_t)m + (size_t)T * ((size_t)ldm + 2 * (size_t)n + 3 * (size_t)m) + 64;
}
__host__ __device__ inline size_t lds_bytes(int n, int m, int nnzA, int T) {
  return lds_doubles(n, m, nnzA, T) * 8 + 2 * ((size_t)n + 1 + (size_t)m + 1 + 3 * (size_t)nnzA) + 16;
}
__host__ __device__ constexpr int log2_tile(int T) { return T == 16 ? 4 : (T == 8 ? 3 : 2); }

// =====================================================================================================================
// k_shared_factor: the scaling of the base data and the shared inverse, into the model block.  The LDS layout and the
// passes are those of k_batch_solve_large up to its first factorisation (batch_large.hpp), for the one instance (P, A, q0).
// =====================================================================================================================
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_shared_factor(
    Pattern Pin, OSQPSettings st, const double *__restrict__ Px, const double *__restrict__ Ax, const double *__restrict__ q0,
    const double *__restrict__ l0, const double *__restrict__ u0, double *scratch, double *model) {
  constexpr int GW = kLargeW;
  const Pattern P = Pin;
  const int n = P.n, m = P.m, tid = mytid();
  Lds s = carve<GW>((ldouble *)lds_raw, P, false);
  for (int k = tid; k <= n; k += NT) { s.Ap[k] = (unsigned short)P.Ap[k]; s.Fp[k] = (unsigned short)P.Fp[k]; }
  for (int k = tid; k <= m; k += NT) s.Rp[k] = (unsigned short)P.Rp[k];
  for (int k = tid; k < P.nnzA; k += NT) { s.Ai[k] = (unsigned short)P.Ai[k]; s.Rc[k] = (unsigned short)P.Rc[k]; s.Rmap[k] = (unsigned short)P.Rmap[k]; }
  for (int k = tid; k < P.nnzF; k += NT) s.Fc[k] = (unsigned short)P.Fc[k];
  for (int k = tid; k < P.nnzA; k += NT) s.Av[k] = Ax[k];
  if (tid == 0) s.Av[P.nnzA] = 0.0;
  for (int k = tid; k < P.nnzF; k += NT) s.Pv[k] = Px[P.Fmap[k]];
  for (int j = tid; j < n; j += NT) { s.q[j] = q0[j]; s.D[j] = 1.0; }
  for (int i = tid; i < m; i += NT) { s.l[i] = fmax(l0[i], -OSQP_INFTY); s.u[i] = fmin(u0[i], OSQP_INFTY); s.E[i] = 1.0; }
  __syncthreads();
  // ---- K0: Ruiz equilibration + cost scaling, pass by pass as in k_batch_solve_large ----
  double c = 1.0;
  const int nscale = (int)st.scaling;
  for (int it = 0; it < nscale; it++) {
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
    __syncthreads();
    for (int r = tid; r < n; r += NT)
      for (int q = s.Fp[r]; q < s.Fp[r + 1]; q++) {
        const int cc = s.Fc[q];
        const int lo = cc < r ? cc : r, hi = cc < r ? r : cc;
        s.Pv[q] = (s.Pv[q] * s.tn[lo]) * s.tn[hi];
      }
    for (int j = tid; j < n; j += NT) {
      for (int k = s.Ap[j]; k < s.Ap[j + 1]; k++) s.Av[k] = (s.Av[k] * s.tm[s.Ai[k]]) * s.tn[j];
      s.q[j] *= s.tn[j];
      s.D[j] *= s.tn[j];
    }
    for (int i = tid; i < m; i += NT) s.E[i] *= s.tm[i];
    __syncthreads();
    double sm = 0.0, mq = 0.0;
    for (int j = tid; j < n; j += NT) {
      double mx = 0.0;
      for (int q = s.Fp[j]; q < s.Fp[j + 1]; q++) mx = fmax(mx, fabs(s.Pv[q]));
      sm += mx;
      mq = fmax(mq, fabs(s.q[j]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sm += __shfl_xor(sm, o, 64); mq = nmax(mq, __shfl_xor(mq, o, 64)); }
    ldouble *rr = s.red + 8 * NW + (it & 1) * 2 * NW;
    if ((tid & 63) == 0) { rr[2 * (tid >> 6)] = sm; rr[2 * (tid >> 6) + 1] = mq; }
    __syncthreads();
    sm = rr[0]; mq = rr[1];
#pragma unroll
    for (int wv = 1; wv < NW; wv++) { sm += rr[2 * wv]; mq = nmax(mq, rr[2 * wv + 1]); }
    double c_temp = sm / (double)n;
    c_temp = lim(fmax(c_temp, lim(mq)));
    c_temp = 1.0 / c_temp;
    for (int k = tid; k < P.nnzF; k += NT) s.Pv[k] *= c_temp;
    for (int j = tid; j < n; j += NT) s.q[j] *= c_temp;
    c *= c_temp;
    __syncthreads();
  }
  for (int i = tid; i < m; i += NT) { s.l[i] *= s.E[i]; s.u[i] *= s.E[i]; }
  __syncthreads();
  // ---- the row kinds of the base bounds, rho per row, M and its inverse ----
  const double rho = uni(fmin(fmax(st.rho, B_RHO_MIN), B_RHO_MAX));
  set_rho(P, s, rho, true);
  assemble_scratch(P, s, st.sigma, scratch);
  const bool pd = invert_large(n, scratch, s.gjc);
  // ---- the model block ----
  const ModelLayout L = model_layout(n, m, P.nnzA, P.nnzF);
  if (tid == 0) { model[MB_C] = c; model[MB_RHO] = rho; model[MB_PD] = pd ? 1.0 : 0.0; }
  for (int j = tid; j < n; j += NT) model[L.D + j] = s.D[j];
  int *const ctype = (int *)(model + L.ctype);
  for (int i = tid; i < m; i += NT) { model[L.E + i] = s.E[i]; model[L.rho + i] = s.rho[i]; model[L.rhoi + i] = s.rhoi[i]; ctype[i] = s.ctype[i]; }
  for (int k = tid; k <= P.nnzA; k += NT) model[L.Av + k] = s.Av[k];
  for (int k = tid; k < P.nnzF; k += NT) model[L.Pv + k] = s.Pv[k];
  // M^-1 out of the scratch (vector stores of this workgroup, behind the barrier that ends invert_mfma: section 13.1) into
  // the padded array; the padding is written as zeros so that no 0 x NaN ever enters an accumulator of the solve kernel
  const int ldm = L.ldm;
  for (int e = tid; e < ldm * ldm; e += NT) {
    const int row = e % ldm, col = e / ldm;
    model[L.Minv + e] = (pd && row < n && col < n) ? scratch[row + (size_t)col * n] : 0.0;
  }
}

// =====================================================================================================================
// The termination tests of one instance (column c of the tile) by ONE WAVEFRONT: the residuals, the primal- and the dual-
// infeasibility tests of residual_phase (batch_solve.hpp) in its order -- the requested accuracy, then at the iteration limit
// the 10x-relaxed pass -- with every product formed on the fly by the lane that needs it.  No workgroup barrier inside: the
// wavefronts of a tile run their instances side by side.  Result: res[4 c ..] = status code (0: go on), pri_res, dua_res, obj.
// Not inlined, for the reason residual_phase is not: the ADMM loop keeps its own register allocation.
// =====================================================================================================================
struct CheckCtx {
  int n, m, T, uns, passes, last;
  double ea, er, epi, edi, c, cinv;
  const ldouble *Av, *x, *z, *y;
  ldouble *res;
  const lshort *Ap, *Ai, *Rp, *Rc, *Rmap;
  const int *Fp, *Fc;
  const double *Pv, *D, *E;  // model block
  const double *q, *l, *u, *dx, *dy;  // tile record
};
__device__ __forceinline__ double wave_max(double a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a = nmax(a, __shfl_xor(a, o, 64));
  return uni(a);
}
__device__ __forceinline__ double wave_sum(double a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  return uni(a);
}
__device__ __noinline__ void shared_check(CheckCtx k, int c) {
  const int n = k.n, m = k.m, T = k.T, lane = mytid() & 63;
  const bool uns = k.uns != 0;
  const double cinv = k.cinv;
  auto a_row = [&](int i, auto v) { double a = 0.0; for (int q = k.Rp[i]; q < k.Rp[i + 1]; q++) a += k.Av[k.Rmap[q]] * v(k.Rc[q]); return a; };
  auto a_col = [&](int j, auto v) { double a = 0.0; for (int e = k.Ap[j]; e < k.Ap[j + 1]; e++) a += k.Av[e] * v(k.Ai[e]); return a; };
  auto p_row = [&](int j, auto v) { double a = 0.0; for (int f = k.Fp[j]; f < k.Fp[j + 1]; f++) a += k.Pv[f] * v(k.Fc[f]); return a; };
  auto xv = [&](int j) { return (double)k.x[j * T + c]; };
  auto yv = [&](int i) { return (double)k.y[i * T + c]; };
  auto dxv = [&](int j) { return k.dx[(size_t)j * T + c]; };
  auto dyv = [&](int i) {  // delta_y projected onto the polar of the recession cone of [l, u]
    double d = k.dy[(size_t)i * T + c];
    const double us = k.u[(size_t)i * T + c], ls = k.l[(size_t)i * T + c];
    if (us > B_INF) { if (ls < -B_INF) d = 0.0; else d = fmin(d, 0.0); }
    else if (ls < -B_INF) d = fmax(d, 0.0);
    return d;
  };
  double v[14];
#pragma unroll
  for (int t = 0; t < 14; t++) v[t] = 0.0;
  double sxpx = 0.0, sqx = 0.0;
  for (int i = lane; i < m; i += 64) {
    const double ax = a_row(i, xv), zi = k.z[i * T + c], e = 1.0 / k.E[i], r = ax - zi;
    v[0] = nmax(v[0], fabs(r)); v[1] = nmax(v[1], fabs(e * r)); v[2] = nmax(v[2], fabs(zi)); v[3] = nmax(v[3], fabs(ax));
    v[4] = nmax(v[4], fabs(e * zi)); v[5] = nmax(v[5], fabs(e * ax));
  }
  for (int j = lane; j < n; j += 64) {
    const double px = p_row(j, xv), qj = k.q[(size_t)j * T + c], at = a_col(j, yv), d = 1.0 / k.D[j], xj = xv(j), r = (qj + px) + at;
    v[6] = nmax(v[6], fabs(r)); v[7] = nmax(v[7], fabs(d * r)); v[8] = nmax(v[8], fabs(qj)); v[9] = nmax(v[9], fabs(at));
    v[10] = nmax(v[10], fabs(px)); v[11] = nmax(v[11], fabs(d * qj)); v[12] = nmax(v[12], fabs(d * at)); v[13] = nmax(v[13], fabs(d * px));
    sxpx += xj * px; sqx += qj * xj;
  }
#pragma unroll
  for (int t = 0; t < 14; t++) v[t] = wave_max(v[t]);
  sxpx = wave_sum(sxpx); sqx = wave_sum(sqx);
  const double pri_res = m == 0 ? 0.0 : (uns ? v[1] : v[0]);
  const double dua_res = uns ? cinv * v[7] : v[6];
  const double obj = cinv * (0.5 * sxpx + sqx);
  int status = 0;
  for (int pass = 0; pass < k.passes && status == 0; pass++) {
    const bool approx = pass == 1;
    double ea = k.ea, er = k.er, epi = k.epi, edi = k.edi;
    if (!(pri_res <= OSQP_INFTY) || !(dua_res <= OSQP_INFTY)) { status = OSQP_NON_CVX; break; }
    if (approx) { ea *= 10; er *= 10; epi *= 10; edi *= 10; }
    bool pc = false, dc = false, pinf = false, dinf = false;
    if (m == 0) pc = true;
    else {
      const double eps_p = ea + er * (uns ? nmax(v[4], v[5]) : nmax(v[2], v[3]));
      if (pri_res < eps_p) pc = true;
      else {  // primal infeasibility on delta_y
        double mv = 0.0, sm = 0.0;
        for (int i = lane; i < m; i += 64) {
          const double d = dyv(i);
          mv = nmax(mv, fabs(uns ? k.E[i] * d : d));
          sm += k.u[(size_t)i * T + c] * fmax(d, 0.0) + k.l[(size_t)i * T + c] * fmin(d, 0.0);
        }
        const double nv = wave_max(mv), lhs = wave_sum(sm);
        if (nv > epi && lhs < -epi * nv) {
          double w = 0.0;
          for (int j = lane; j < n; j += 64) { const double t = a_col(j, dyv); w = nmax(w, fabs(uns ? t / k.D[j] : t)); }
          pinf = wave_max(w) < epi * nv;
        }
      }
    }
    const double eps_d = ea + er * (uns ? cinv * nmax(v[11], nmax(v[12], v[13])) : nmax(v[8], nmax(v[9], v[10])));
    if (dua_res < eps_d) dc = true;
    else {  // dual infeasibility on delta_x
      double mv = 0.0, sm = 0.0;
      for (int j = lane; j < n; j += 64) { const double d = dxv(j); mv = nmax(mv, fabs(uns ? k.D[j] * d : d)); sm += k.q[(size_t)j * T + c] * d; }
      const double nv = wave_max(mv), qdx = wave_sum(sm);
      const double cs = uns ? k.c : 1.0;
      if (nv > edi && qdx < -cs * edi * nv) {
        double w = 0.0;
        for (int j = lane; j < n; j += 64) { const double t = p_row(j, dxv); w = nmax(w, fabs(uns ? t / k.D[j] : t)); }
        if (wave_max(w) < cs * edi * nv) {
          double bad = 0.0;
          for (int i = lane; i < m; i += 64) {
            const double r = a_row(i, dxv), t = uns ? r / k.E[i] : r;
            if ((k.u[(size_t)i * T + c] < B_INF && t > edi * nv) || (k.l[(size_t)i * T + c] > -B_INF && t < -edi * nv) || t != t) bad = 1.0;
          }
          dinf = wave_max(bad) == 0.0;
        }
      }
    }
    if (pc && dc) status = approx ? OSQP_SOLVED_INACCURATE : OSQP_SOLVED;
    else if (pinf) status = approx ? OSQP_PRIMAL_INFEASIBLE_INACCURATE : OSQP_PRIMAL_INFEASIBLE;
    else if (dinf) status = approx ? OSQP_DUAL_INFEASIBLE_INACCURATE : OSQP_DUAL_INFEASIBLE;
  }
  if (k.last && k.passes && status == 0) status = OSQP_MAX_ITER_REACHED;
  if (lane == 0) { k.res[4 * c] = (double)status; k.res[4 * c + 1] = pri_res; k.res[4 * c + 2] = dua_res; k.res[4 * c + 3] = obj; }
}

// =====================================================================================================================
// k_batch_solve_shared: workgroup b solves instances b T .. b T + T - 1 (those below count).  `tiles` is read AND written by
// the launch (q, l, u read; the iterate read at the start and written where an instance stops; delta_x / delta_y written at a
// check iteration and read back by the check behind a barrier: plain vector stores and loads of this workgroup, the argument
// of section 13.1) -- neither const nor __restrict__.  The model block was written by an earlier launch.
// =====================================================================================================================
__global__ __launch_bounds__(NT) void k_batch_solve_shared(Pattern Pin, OSQPSettings st, int count, int T, int warm,
                                                           const double *__restrict__ model, double *tiles, double *__restrict__ x_out,
                                                           double *__restrict__ y_out, double *__restrict__ info_out) {
  const Pattern P = Pin;
  const int n = P.n, m = P.m, nnzA = P.nnzA, tid = mytid();
  const int lgT = log2_tile(T), first = blockIdx.x * T;
  if (first >= count) return;
  const int ncol = count - first < T ? count - first : T;
  const ModelLayout ML = model_layout(n, m, nnzA, P.nnzF);
  const TileLayout TL = tile_layout(n, m, T);
  const int ldm = ML.ldm, nT = n * T, mT = m * T;
  double *const rec = tiles + (size_t)blockIdx.x * TL.total;
  // ---- LDS ----
  ldouble *p = (ldouble *)lds_raw;
  ldouble *const Av = p; p += nnzA + 1;
  ldouble *const rho = p; p += m;
  ldouble *const rhoi = p; p += m;
  ldouble *const bb = p; p += ldm * T;
  ldouble *const xt = p; p += nT;
  ldouble *const x = p; p += nT;
  ldouble *const z = p; p += mT;
  ldouble *const y = p; p += mT;
  ldouble *const zt = p; p += mT;
  ldouble *const res = p; p += 64;
  lshort *h = (lshort *)p;
  lshort *const sAp = h; h += n + 1;
  lshort *const sRp = h; h += m + 1;
  lshort *const sAi = h; h += nnzA;
  lshort *const sRc = h; h += nnzA;
  lshort *const sRmap = h;
  // ---- stage the pattern (16-bit), the shared scaled values and the tile's iterate ----
  for (int k = tid; k <= n; k += NT) sAp[k] = (unsigned short)P.Ap[k];
  for (int k = tid; k <= m; k += NT) sRp[k] = (unsigned short)P.Rp[k];
  for (int k = tid; k < nnzA; k += NT) { sAi[k] = (unsigned short)P.Ai[k]; sRc[k] = (unsigned short)P.Rc[k]; sRmap[k] = (unsigned short)P.Rmap[k]; }
  for (int k = tid; k <= nnzA; k += NT) Av[k] = model[ML.Av + k];
  for (int i = tid; i < m; i += NT) { rho[i] = model[ML.rho + i]; rhoi[i] = model[ML.rhoi + i]; }
  for (int e = tid; e < ldm * T; e += NT) bb[e] = 0.0;
  for (int e = tid; e < nT; e += NT) { x[e] = (warm && (e & (T - 1)) < ncol) ? rec[TL.x + e] : 0.0; xt[e] = 0.0; }
  for (int e = tid; e < mT; e += NT) {
    const bool on = warm && (e & (T - 1)) < ncol;
    const double z0 = on ? rec[TL.z + e] : 0.0, y0 = on ? rec[TL.y + e] : 0.0;
    z[e] = z0; y[e] = y0; zt[e] = model[ML.rho + (e >> lgT)] * z0 - y0;
  }
  if (tid < 64) res[tid] = 0.0;
  __syncthreads();
  const double c = uni(model[MB_C]), cinv = 1.0 / c;
  const bool uns = st.scaling && !st.scaled_termination;
  const int check = (int)st.check_termination, max_iter = (int)st.max_iter;
  const double alpha = st.alpha, sigma = st.sigma;
  const int lane = tid & 63, wave = uni(tid >> 6), lr = lane >> 4, lc = lane & 15;
  const int ntile = ldm >> 4;
  const double *const Minv = model + ML.Minv;
  const double *const qg = rec + TL.q, *const lg = rec + TL.l, *const ug = rec + TL.u;
  double *const dxg = rec + TL.dx, *const dyg = rec + TL.dy;
  unsigned mask = (1u << ncol) - 1u;  // the columns still iterating: the same value in every thread
  // ---- ADMM loop ----
  for (int iter = 1; iter <= max_iter && mask; iter++) {
    const bool last = iter == max_iter;
    const bool chk = last || (check && (iter % check == 0));
    // b = sigma x_prev - q + A' zt: one thread per (column j of A, instance c), the column walked in index order
    for (int e = tid; e < nT; e += NT) {
      const int cc = e & (T - 1), j = e >> lgT;
      if (!((mask >> cc) & 1u)) continue;
      double a = 0.0;
      for (int k = sAp[j]; k < sAp[j + 1]; k++) a += Av[k] * zt[(sAi[k] << lgT) + cc];
      bb[e] = sigma * x[e] - qg[e] + a;
    }
    __syncthreads();
    // x~ = M^-1 B on the matrix cores: the 16-row tiles of M^-1 dealt to the wavefronts; per step of four columns the A
    // operand (lane: row lane & 15, column lane >> 4) is 16 x 4 doubles of M^-1 from the model block, the B operand (row
    // lane >> 4, column lane & 15) 4 x 16 right-hand sides from LDS -- zero for columns >= T and for stopped instances.
    // k runs 0, 4, 8, ... in every solve.  Result: lane holds rows (lane >> 4) + 4 r of column lane & 15.
    {
      const bool on = lc < T && ((mask >> lc) & 1u);
      const ldouble *const bp = bb + lr * T + (on ? lc : 0);
      // A wavefront has at most two tiles (ntile <= 16 = 2 NW): I0 = wave and I1 = wave + 8.  Both go through k together -- one
      // B operand serves both -- in chunks of eight steps (sixteen loads of M^-1 in flight per lane: the loads come from L2 and
      // the phase is bound by their latency), then a last chunk of four where ldm is an odd multiple of 16.
      const int I0 = wave, I1 = wave + NW;
      const bool two = I1 < ntile;
      if (I0 < ntile) {
        const double *const ap0 = Minv + (I0 * 16 + lc) + (size_t)lr * ldm;
        const double *const ap1 = Minv + ((two ? I1 : I0) * 16 + lc) + (size_t)lr * ldm;
        d4_t acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
        int k0 = 0;
        for (; k0 + 32 <= ldm; k0 += 32) {
          double a0[8], a1[8], b[8];
#pragma unroll
          for (int u = 0; u < 8; u++) a0[u] = ap0[(size_t)(k0 + 4 * u) * ldm];
          if (two) {
#pragma unroll
            for (int u = 0; u < 8; u++) a1[u] = ap1[(size_t)(k0 + 4 * u) * ldm];
          }
#pragma unroll
          for (int u = 0; u < 8; u++) b[u] = on ? (double)bp[(k0 + 4 * u) * T] : 0.0;
#pragma unroll
          for (int u = 0; u < 8; u++) acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[u], b[u], acc0, 0, 0, 0);
          if (two) {
#pragma unroll
            for (int u = 0; u < 8; u++) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[u], b[u], acc1, 0, 0, 0);
          }
        }
        if (k0 < ldm) {  // sixteen columns left
          double a0[4], a1[4], b[4];
#pragma unroll
          for (int u = 0; u < 4; u++) a0[u] = ap0[(size_t)(k0 + 4 * u) * ldm];
          if (two) {
#pragma unroll
            for (int u = 0; u < 4; u++) a1[u] = ap1[(size_t)(k0 + 4 * u) * ldm];
          }
#pragma unroll
          for (int u = 0; u < 4; u++) b[u] = on ? (double)bp[(k0 + 4 * u) * T] : 0.0;
#pragma unroll
          for (int u = 0; u < 4; u++) acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[u], b[u], acc0, 0, 0, 0);
          if (two) {
#pragma unroll
            for (int u = 0; u < 4; u++) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[u], b[u], acc1, 0, 0, 0);
          }
        }
        if (on) {
          for (int s = 0; s < (two ? 2 : 1); s++) {
            const d4_t acc = s ? acc1 : acc0;
            const int I = s ? I1 : I0;
#pragma unroll
            for (int r = 0; r < 4; r++) {
              const int row = I * 16 + lr + 4 * r;
              if (row < n) {
                const int e = (row << lgT) + lc;
                const double xo = x[e], a = acc[r];
                xt[e] = a;
                const double xn = alpha * a + (1.0 - alpha) * xo;
                x[e] = xn;
                if (chk) dxg[e] = xn - xo;
              }
            }
          }
        }
      }
    }
    __syncthreads();
    // z~ = A x~ row by row, each row finished on the spot: z, y, delta_y and zt = rho z - y for the next right-hand side
    for (int e = tid; e < mT; e += NT) {
      const int cc = e & (T - 1), i = e >> lgT;
      if (!((mask >> cc) & 1u)) continue;
      double a = 0.0;
      for (int q = sRp[i]; q < sRp[i + 1]; q++) a += Av[sRmap[q]] * xt[(sRc[q] << lgT) + cc];
      const double r = rho[i], zh = alpha * a + (1.0 - alpha) * z[e], yo = y[e];
      const double zn = fmin(fmax(zh + rhoi[i] * yo, lg[e]), ug[e]);
      z[e] = zn;
      const double d = r * (zh - zn);
      y[e] = yo + d;
      zt[e] = r * zn - (yo + d);
      if (chk) dyg[e] = d;
    }
    __syncthreads();
    if (!chk) continue;
    // ---- the termination tests: wavefront w takes the instances w, w + 8 of the tile ----
    {
      CheckCtx k;
      k.n = n; k.m = m; k.T = T; k.uns = uns; k.passes = last ? 2 : 1; k.last = last;
      k.ea = st.eps_abs; k.er = st.eps_rel; k.epi = st.eps_prim_inf; k.edi = st.eps_dual_inf; k.c = c; k.cinv = cinv;
      k.Av = Av; k.x = x; k.z = z; k.y = y; k.res = res;
      k.Ap = sAp; k.Ai = sAi; k.Rp = sRp; k.Rc = sRc; k.Rmap = sRmap;
      k.Fp = P.Fp; k.Fc = P.Fc; k.Pv = model + ML.Pv; k.D = model + ML.D; k.E = model + ML.E;
      k.q = qg; k.l = lg; k.u = ug; k.dx = dxg; k.dy = dyg;
      for (int cc = wave; cc < T; cc += NW)
        if ((mask >> cc) & 1u) shared_check(k, cc);
    }
    __syncthreads();
    // ---- an instance that stops here leaves its results and its scaled iterate; its column is masked from now on ----
    for (int cc = 0; cc < T; cc++) {
      if (!((mask >> cc) & 1u)) continue;
      const int status = uni((int)res[4 * cc]);
      if (status == 0) continue;
      const bool has_sol = status == OSQP_SOLVED || status == OSQP_SOLVED_INACCURATE || status == OSQP_MAX_ITER_REACHED;
      const size_t inst = (size_t)first + cc;
      for (int j = tid; j < n; j += NT) {
        const double xj = x[(j << lgT) + cc];
        x_out[inst * n + j] = has_sol ? model[ML.D + j] * xj : NAN;
        rec[TL.x + (j << lgT) + cc] = has_sol ? xj : 0.0;
      }
      for (int i = tid; i < m; i += NT) {
        const double yi = y[(i << lgT) + cc];
        y_out[inst * m + i] = has_sol ? cinv * model[ML.E + i] * yi : NAN;
        rec[TL.z + (i << lgT) + cc] = has_sol ? (double)z[(i << lgT) + cc] : 0.0;
        rec[TL.y + (i << lgT) + cc] = has_sol ? yi : 0.0;
      }
      if (tid == 0) {
        double *o = info_out + inst * 6;
        o[0] = (double)iter; o[1] = (double)status; o[2] = res[4 * cc + 1]; o[3] = res[4 * cc + 2];
        o[4] = status == OSQP_NON_CVX ? NAN : (double)res[4 * cc + 3]; o[5] = 0.0;
      }
      mask &= ~(1u << cc);
    }
    __syncthreads();  // res is rewritten by the next check
  }
}

// =====================================================================================================================
// The small kernels of the updates.  One thread per (instance, entry); instance i is column i % T of tile i / T.
// =====================================================================================================================
// dst[entry idx of instance i] = mult * (clamp(src[i stride + idx]) * scale[idx]): q -> c (q D) (no clamp), l -> max(l, -INFTY) E,
// u -> min(u, INFTY) E.  stride 0: every instance takes the same vector (the base data at setup).
__global__ __launch_bounds__(256) void k_shared_put(int count, int len, int T, const double *__restrict__ src, int stride,
                                                    const double *__restrict__ scale, double mult, int clamp, double *__restrict__ tiles,
                                                    size_t off, size_t tile_total) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (size_t)count * len) return;
  const int inst = (int)(g / len), idx = (int)(g - (size_t)inst * len);
  double v = src[(size_t)inst * stride + idx];
  if (clamp < 0) v = fmax(v, -OSQP_INFTY);
  if (clamp > 0) v = fmin(v, OSQP_INFTY);
  tiles[(size_t)(inst / T) * tile_total + off + (size_t)idx * T + inst % T] = mult * (v * scale[idx]);
}
// zeros into the iterate of every tile (setup)
__global__ __launch_bounds__(256) void k_shared_zero(size_t total, double *__restrict__ tiles) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g < total) tiles[g] = 0.0;
}
// the iterate of osqp_amd_shared_batch_warm_start, as k_batch_warm has it: x <- x / D, z <- E (A_raw x_raw), y <- c y / E; a
// missing vector is zero (and z with x).  One thread per (instance, row or variable).
__global__ __launch_bounds__(256) void k_shared_warm(Pattern P, int count, int T, const double *__restrict__ Ax_raw, const double *__restrict__ model,
                                                     const double *__restrict__ x_all, const double *__restrict__ y_all, double *__restrict__ tiles) {
  const int n = P.n, m = P.m;
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (size_t)count * (n + m)) return;
  const int inst = (int)(g / (n + m)), k = (int)(g - (size_t)inst * (n + m));
  const ModelLayout ML = model_layout(n, m, P.nnzA, P.nnzF);
  const TileLayout TL = tile_layout(n, m, T);
  double *const rec = tiles + (size_t)(inst / T) * TL.total;
  const int cc = inst % T;
  if (k < n) { rec[TL.x + (size_t)k * T + cc] = x_all ? x_all[(size_t)inst * n + k] / model[ML.D + k] : 0.0; return; }
  const int i = k - n;
  const double e = model[ML.E + i];
  double ax = 0.0;
  if (x_all)
    for (int q = P.Rp[i]; q < P.Rp[i + 1]; q++) ax += Ax_raw[P.Rmap[q]] * x_all[(size_t)inst * n + P.Rc[q]];
  rec[TL.z + (size_t)i * T + cc] = e * ax;
  rec[TL.y + (size_t)i * T + cc] = y_all ? model[MB_C] * y_all[(size_t)inst * m + i] / e : 0.0;
}
// The check of an update of the bounds, reduced to ONE WORD as k_bounds_crossed does for the single model: the smallest
// ((instance m + row) << 2 | reason) over the offending rows -- reason 1: l > u, 2: the kind of the row under the scaled bounds
// (set_rho's rule) is not the kind it has under (l0, u0).  ~0: the update is fine.
__global__ __launch_bounds__(256) void k_shared_check_bounds(int count, int m, const double *__restrict__ l_all, const double *__restrict__ u_all,
                                                             const double *__restrict__ E, const int *__restrict__ ctype, unsigned long long *flag) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (size_t)count * m) return;
  const int i = (int)(g % m);
  const double l = l_all[g], u = u_all[g];
  unsigned long long reason = 0;
  if (l > u) reason = 1;
  else {
    const double ls = fmax(l, -OSQP_INFTY) * E[i], us = fmin(u, OSQP_INFTY) * E[i];
    const int t = (ls < -B_INF && us > B_INF) ? -1 : (us - ls < 1e-4 ? 1 : 0);
    if (t != ctype[i]) reason = 2;
  }
  if (reason) atomicMin(flag, ((unsigned long long)g << 2) | reason);
}

}  // namespace shared
}  // namespace
}  // namespace oq
