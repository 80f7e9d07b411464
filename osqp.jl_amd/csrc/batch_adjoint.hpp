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
// LDS: the polish Layout as it stands.  q holds c D g_x, l the masked E g_y, x and y the solution r~_x and s (after the
// solves: r_x and, in ry, r_y), t the caller-unit x after the solves, z the caller-unit y; u is not used.  Nothing of an
// instance touches global scratch; the record, the data and the info of the handle are only read.
// tests/batch_adjoint_ref.py (model) is the numpy model of this file.
#pragma once
#include "batch_polish.hpp"

namespace oq {
namespace {
namespace polish {

struct AdjointArgs {
  const double *Px, *Ax, *l, *u, *info, *rec;  // of the handle: raw data, the info rows and the records of the last resolve
  const double *gx, *gy;                        // of the call: incoming gradients [k x n], [k x m]; nullptr: zero
  double *dq, *dl, *du, *dPx, *dAx, *act, *status;  // of the call: outputs, [k x .]; nullptr: not wanted
  int info_stride, rec_stride, refine;
  double delta;
  // a selection (osqp_amd_batch_adjoint_rows): the workgroup at position p of the k launched serves instance sel[p]; what is
  // "of the handle" above is addressed with the instance, what is "of the call" with the position.  nullptr: the identity
  const int *sel = nullptr;
};

// the rows of the call (at position pos) of an instance that is not differentiated: zeros
__device__ __forceinline__ void adjoint_zero_rows(const Pattern &P, const AdjointArgs &a, int pos) {
  const int tid = threadIdx.x, n = P.n, m = P.m;
  for (int j = tid; j < n; j += PT) if (a.dq) a.dq[(size_t)pos * n + j] = 0.0;
  for (int i = tid; i < m; i += PT) {
    if (a.dl) a.dl[(size_t)pos * m + i] = 0.0;
    if (a.du) a.du[(size_t)pos * m + i] = 0.0;
    if (a.act) a.act[(size_t)pos * m + i] = 0.0;
  }
  if (a.dPx) for (int k = tid; k < P.nnzP; k += PT) a.dPx[(size_t)pos * P.nnzP + k] = 0.0;
  if (a.dAx) for (int k = tid; k < P.nnzA; k += PT) a.dAx[(size_t)pos * P.nnzA + k] = 0.0;
}

__global__ __launch_bounds__(PT) void k_batch_adjoint(Pattern P, int count, Layout L, AdjointArgs a) {
  const int pos = blockIdx.x, tid = threadIdx.x, n = P.n, m = P.m;
  if (pos >= count) return;
  const int inst = a.sel ? a.sel[pos] : pos;  // wave-uniform; `count` is the launch's: k workgroups
  if ((int)a.info[(size_t)inst * a.info_stride + 1] != OSQP_SOLVED) {  // no solution to differentiate
    adjoint_zero_rows(P, a, pos);
    if (tid == 0 && a.status) a.status[pos] = 0.0;
    return;
  }
  const Slots S = make_slots(L);
  ldouble *const q = S.q, *const x = S.x, *const t = S.t, *const l = S.l, *const y = S.y, *const ry = S.ry, *const z = S.z, *const act = S.act;
  const double *const rec = a.rec + (size_t)inst * a.rec_stride;
  const double *const D = rec + rec_D(n, m), *const E = rec + rec_E(n, m);
  const double c = rec[REC_C], cinv = 1.0 / c, delta = a.delta;

  // ---- the scaled matrices, the right-hand side [c D g_x; (E g_y)_a], the active sets, the caller-unit multipliers ----
  const double *const Axi = a.Ax + (size_t)inst * P.nnzA, *const Pxi = a.Px + (size_t)inst * P.nnzP;
  for (int j = tid; j < n; j += PT) {
    stage_matrices(P, S, j, Axi, Pxi, D, E, c);
    q[j] = a.gx ? c * (a.gx[(size_t)pos * n + j] * D[j]) : 0.0;
  }
  for (int i = tid; i < m; i += PT) {
    const double e = E[i];
    const double li = fmax(a.l[(size_t)inst * m + i], -OSQP_INFTY) * e, ui = fmin(a.u[(size_t)inst * m + i], OSQP_INFTY) * e;
    const double yi = rec[rec_y(n, m) + i];
    const double on = li == ui ? -1.0 : classify(rec[rec_z(n, m) + i], yi, li, ui);  // an equality row is always active
    const double g = (on != 0.0 && a.gy) ? a.gy[(size_t)pos * m + i] * e : 0.0;
    act[i] = on;
    l[i] = g; ry[i] = g;
    y[i] = 0.0;
    z[i] = cinv * e * yi;
  }
  assemble_M(P, S, delta);
  if (!cholesky(n, S.M, S.rdg, S.col)) {
    adjoint_zero_rows(P, a, pos);
    if (tid == 0 && a.status) a.status[pos] = -1.0;
    return;
  }
  for (int it = 0; it <= a.refine; it++) kkt_step<false>(P, S, it, delta);

  // ---- back to the caller's units: x <- r_x = D r~_x, ry <- r_y = E s / c, t <- the solution x = D x~ of the record ----
  for (int j = tid; j < n; j += PT) { const double dj = D[j]; x[j] = dj * x[j]; t[j] = dj * rec[rec_x(n, m) + j]; }
  for (int i = tid; i < m; i += PT) ry[i] = cinv * E[i] * y[i];
  __syncthreads();

  // ---- the gradients: a thread per row (dl, du, act), a thread per column (dq, its stored entries of P, its entries of A) ----
  for (int i = tid; i < m; i += PT) {
    const double on = act[i], r = ry[i];
    if (a.dl) a.dl[(size_t)pos * m + i] = on < 0.0 ? r : 0.0;
    if (a.du) a.du[(size_t)pos * m + i] = on > 0.0 ? r : 0.0;
    if (a.act) a.act[(size_t)pos * m + i] = on;
  }
  for (int j = tid; j < n; j += PT) {
    const double rj = x[j], xj = t[j];
    if (a.dq) a.dq[(size_t)pos * n + j] = -rj;
    if (a.dPx) {
      double *const dP = a.dPx + (size_t)pos * P.nnzP;
      for (int f = P.Fp[j]; f < P.Fp[j + 1]; f++) {  // row j of the full P; its entries cc <= j are column j of the stored triangle
        const int cc = P.Fc[f];
        if (cc == j) dP[P.Fmap[f]] = -(rj * xj);
        else if (cc < j) dP[P.Fmap[f]] = -(x[cc] * xj + rj * t[cc]);
      }
    }
    if (a.dAx) {
      double *const dA = a.dAx + (size_t)pos * P.nnzA;
      for (int k = P.Ap[j]; k < P.Ap[j + 1]; k++) { const int i = P.Ai[k]; dA[k] = -(z[i] * rj + ry[i] * xj); }
    }
  }
  if (tid == 0 && a.status) a.status[pos] = 1.0;
}

}  // namespace polish
}  // namespace
}  // namespace oq
