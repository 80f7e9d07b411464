// batch_adjoint.hpp -- adjoint derivatives of the solutions of the resident batch (osqp_amd_batch_adjoint): a kernel of its
// own, launched on request after a resolve; the solve kernels and k_batch_polish know nothing of it.
//
// For an instance with solution x, multipliers y and active rows a (L at the lower bound, U at the upper), the gradients of a
// scalar loss with respect to the data follow from ONE solve with the KKT matrix of the active set (caller's units):
//     [P, Aa'; Aa, 0] [r_x; r_a] = [g_x; (g_y)_a],     r_y = r_a scattered to length m, zero on the inactive rows
//     dq = -r_x,   dl_i = r_y,i (i in L),   du_i = r_y,i (i in U),
//     dPx(i, j) = -r_x,i x_i (i = j), -(r_x,i x_j + r_x,j x_i) (i < j),     dAx(i, j) = -(y_i r_x,j + r_y,i x_j).
// The kernel works in the SCALED space, on the record row and the raw data, exactly as k_batch_polish does: with
// P~ = c D P D, A~ = E A D it solves [P~, A~a'; A~a, 0] [r~_x; s] = [c D g_x; (E g_y)_a], then r_x = D r~_x, r_y = E s / c; the
// x and y of the two matrix gradients are the caller-unit values D x~, E y~ / c of the record (what the resolve returned).
// The solve is the polish solve with another right-hand side: the condensed M = P~ + delta I + A~a' A~a / delta, its
// Cholesky factor, one solve and `refine` refinement steps against the unregularised matrix -- the device functions of
// batch_polish.hpp, shared with that kernel.  Active rows: the classification of polish on the record's iterate, and a row
// with l == u (scaled, after clipping) is always active and counts as lower.
//
// A call carries `ncot` pairs (g_x, g_y) per instance (osqp_amd_batch_adjoint_multi; 1 for osqp_amd_batch_adjoint).  The factor
// is kept for every cotangent of a call, as k_batch_jvp keeps it for its directions: stage_matrices, the classification,
// assemble_M and cholesky run once per instance, the right-hand side, the solve, its `refine` refinement steps, the unscaling
// and the five gradients once per cotangent.  Nothing is carried from one cotangent to the next, so cotangent c of an ncot
// call has the bits of a one-cotangent call with that pair.
//
// LDS: the polish Layout as it stands.  col holds the caller-unit x (after the factorisation, which is done with it; t is the
// work vector of every solve), z the caller-unit y; per cotangent q holds c D g_x, l the masked E g_y, x and y the solution
// r~_x and s (after the solves: r_x and, in ry, r_y); u is not used.  y is zeroed once: the solves write it on the active rows
// only.  Nothing of an instance touches global scratch; the record, the data and the info of the handle are only read.
// tests/batch_adjoint_ref.py (model) is the numpy model of this file.
#pragma once
#include "batch_polish.hpp"

namespace oq {
namespace {
namespace polish {

struct AdjointArgs {
  const double *Px, *Ax, *l, *u, *info, *rec;  // of the handle: raw data, the info rows and the records of the last resolve
  const double *gx, *gy;                        // of the call: incoming gradients, cotangent-major [ncot x k x n], [ncot x k x m]; nullptr: zero
  double *dq, *dl, *du, *dPx, *dAx;             // of the call: outputs, cotangent-major [ncot x k x cols]; nullptr: not wanted
  double *act, *status;                         // of the call: act [k x m], status [k], once per instance; nullptr: not wanted
  int ncot, info_stride, rec_stride, refine;
  double delta;
  // a selection (osqp_amd_batch_adjoint_rows): the workgroup at position p of the k launched serves instance sel[p]; what is
  // "of the handle" above is addressed with the instance, what is "of the call" with the position (row c * k + p of a
  // cotangent-major array).  nullptr: the identity
  const int *sel = nullptr;
  double *scratch = nullptr;  // LARGE (batch_polish.hpp): n x n doubles per launch position, the handle's solve scratch
};

// the rows of the call (at position pos of the `count` launched) of an instance that is not differentiated: zeros in every
// cotangent
__device__ __forceinline__ void adjoint_zero_rows(const Pattern &P, const AdjointArgs &a, int count, int pos) {
  const int tid = threadIdx.x, n = P.n, m = P.m;
  for (int c = 0; c < a.ncot; c++) {
    const size_t row = (size_t)c * count + pos;
    for (int j = tid; j < n; j += PT) if (a.dq) a.dq[row * n + j] = 0.0;
    for (int i = tid; i < m; i += PT) {
      if (a.dl) a.dl[row * m + i] = 0.0;
      if (a.du) a.du[row * m + i] = 0.0;
    }
    if (a.dPx) for (int k = tid; k < P.nnzP; k += PT) a.dPx[row * P.nnzP + k] = 0.0;
    if (a.dAx) for (int k = tid; k < P.nnzA; k += PT) a.dAx[row * P.nnzA + k] = 0.0;
  }
  if (a.act) for (int i = tid; i < m; i += PT) a.act[(size_t)pos * m + i] = 0.0;
}

template <bool LARGE>
__global__ __launch_bounds__(PT) void k_batch_adjoint(Pattern P, int count, Layout L, AdjointArgs a) {
  const int pos = blockIdx.x, tid = threadIdx.x, n = P.n, m = P.m;
  if (pos >= count) return;
  const int inst = a.sel ? a.sel[pos] : pos;  // wave-uniform; `count` is the launch's: k workgroups
  if ((int)a.info[(size_t)inst * a.info_stride + 1] != OSQP_SOLVED) {  // no solution to differentiate
    adjoint_zero_rows(P, a, count, pos);
    if (tid == 0 && a.status) a.status[pos] = 0.0;
    return;
  }
  Slots S = make_slots(L);
  if constexpr (LARGE) S.G = a.scratch + (size_t)pos * n * n;
  ldouble *const q = S.q, *const x = S.x, *const xc = S.col, *const l = S.l, *const y = S.y, *const ry = S.ry, *const z = S.z, *const act = S.act;
  const double *const rec = a.rec + (size_t)inst * a.rec_stride;
  const double *const D = rec + rec_D(n, m), *const E = rec + rec_E(n, m);
  const double c = rec[REC_C], cinv = 1.0 / c, delta = a.delta;

  // ---- the scaled matrices, the active sets, the caller-unit multipliers ----
  const double *const Axi = a.Ax + (size_t)inst * P.nnzA, *const Pxi = a.Px + (size_t)inst * P.nnzP;
  for (int j = tid; j < n; j += PT) stage_matrices(P, S, j, Axi, Pxi, D, E, c);
  for (int i = tid; i < m; i += PT) {
    const double e = E[i];
    const double li = fmax(a.l[(size_t)inst * m + i], -OSQP_INFTY) * e, ui = fmin(a.u[(size_t)inst * m + i], OSQP_INFTY) * e;
    const double yi = rec[rec_y(n, m) + i];
    const double on = li == ui ? -1.0 : classify(rec[rec_z(n, m) + i], yi, li, ui);  // an equality row is always active
    act[i] = on;
    if (a.act) a.act[(size_t)pos * m + i] = on;
    y[i] = 0.0;  // the inactive rows stay zero through every cotangent
    z[i] = cinv * e * yi;
  }
  if (!assemble_and_factor<LARGE>(P, S, delta)) {
    adjoint_zero_rows(P, a, count, pos);
    if (tid == 0 && a.status) a.status[pos] = -1.0;
    return;
  }
  // ---- the factor is done with col: the caller-unit x = D x~ of the record goes there ----
  for (int j = tid; j < n; j += PT) xc[j] = D[j] * rec[rec_x(n, m) + j];

  for (int cot = 0; cot < a.ncot; cot++) {
    const size_t row = (size_t)cot * count + pos;
    // ---- the right-hand side [c D g_x; (E g_y)_a] of this cotangent.  The output stage of the cotangent before reads x, ry
    // of OTHER threads' entries (dPx, dAx): the barrier that ends the loop body stands between it and these writes ----
    for (int j = tid; j < n; j += PT) q[j] = a.gx ? c * (a.gx[row * n + j] * D[j]) : 0.0;
    for (int i = tid; i < m; i += PT) {
      const double g = (act[i] != 0.0 && a.gy) ? a.gy[row * m + i] * E[i] : 0.0;
      l[i] = g; ry[i] = g;
    }
    __syncthreads();  // kkt_step's first loop reads the ry of other threads' rows (and xc is complete for the output stage)
    for (int it = 0; it <= a.refine; it++) kkt_step<false, LARGE>(P, S, it, delta);

    // ---- back to the caller's units: x <- r_x = D r~_x, ry <- r_y = E s / c (y is zero on the inactive rows) ----
    for (int j = tid; j < n; j += PT) x[j] = D[j] * x[j];
    for (int i = tid; i < m; i += PT) ry[i] = cinv * E[i] * y[i];
    __syncthreads();

    // ---- the gradients: a thread per row (dl, du), a thread per column (dq, its stored entries of P, its entries of A) ----
    for (int i = tid; i < m; i += PT) {
      const double on = act[i], r = ry[i];
      if (a.dl) a.dl[row * m + i] = on < 0.0 ? r : 0.0;
      if (a.du) a.du[row * m + i] = on > 0.0 ? r : 0.0;
    }
    for (int j = tid; j < n; j += PT) {
      const double rj = x[j], xj = xc[j];
      if (a.dq) a.dq[row * n + j] = -rj;
      if (a.dPx) {
        double *const dP = a.dPx + row * P.nnzP;
        for (int f = P.Fp[j]; f < P.Fp[j + 1]; f++) {  // row j of the full P; its entries cc <= j are column j of the stored triangle
          const int cc = P.Fc[f];
          if (cc == j) dP[P.Fmap[f]] = -(rj * xj);
          else if (cc < j) dP[P.Fmap[f]] = -(x[cc] * xj + rj * xc[cc]);
        }
      }
      if (a.dAx) {
        double *const dA = a.dAx + row * P.nnzA;
        for (int k = P.Ap[j]; k < P.Ap[j + 1]; k++) { const int i = P.Ai[k]; dA[k] = -(z[i] * rj + ry[i] * xj); }
      }
    }
    if (cot + 1 < a.ncot) __syncthreads();  // uniform: the next right-hand side overwrites ry, its solve x
  }
  if (tid == 0 && a.status) a.status[pos] = 1.0;
}

}  // namespace polish
}  // namespace
}  // namespace oq
