// batch_jvp.hpp -- forward sensitivities (Jacobian-vector products) of the solutions of the resident batch
// (osqp_amd_batch_jvp): a kernel of its own, launched on request after a resolve; the solve kernels, k_batch_polish and
// k_batch_adjoint know nothing of it.
//
// For an instance with solution x, multipliers y and active rows a (L at the lower bound, U at the upper), the tangents of
// the solution along a direction (tq, tl, tu, tP, tA) of the data follow from ONE solve with the KKT matrix of the active set
// (caller's units; the transpose of what batch_adjoint.hpp does, and the matrix is symmetric):
//     [P, Aa'; Aa, 0] [tx; ty_a] = [-(tq + tP x + tA' y); (tb - tA x)_a],     tb_i = tl_i (i in L), tu_i (i in U)
//     ty = ty_a scattered to length m, zero on the inactive rows.
// tP is the symmetric matrix of the stored triangle tPx (a stored off-diagonal entry stands for both halves).  On a row with
// l == u only tl is read; a tangent of an inactive bound has no effect.  The kernel works in the SCALED space, as
// k_batch_adjoint does: with P~ = c D P D, A~ = E A D it solves [P~, A~a'; A~a, 0] [x~; s] = [c D rhs_x; (E rhs_a)_a], then
// tx = D x~, ty = E s / c.  rhs_x and rhs_a are formed in the caller's units from the raw tangents and the caller-unit
// x = D x~, y = E y~ / c of the record (what the resolve returned), through the full-P CSR, A's CSC and A's CSR of the Pattern.
//
// The factor is kept for every direction of a call: assemble_M and cholesky run once per instance, the right-hand side, the
// solve, its `refine` refinement steps and the output stage once per direction.  Nothing is carried from one direction to the
// next, so direction d of an ndir-direction call has the bits of a one-direction call with that tangent.
//
// LDS: the polish Layout as it stands.  col holds the caller-unit x (after the factorisation, which is done with it), z the
// caller-unit y; per direction q holds c D rhs_x, l the masked E rhs_a, x and y the solution x~ and s; u is not used.  Nothing
// of an instance touches global scratch; the record, the data and the info of the handle are only read.
// tests/batch_jvp_ref.py (model) is the numpy model of this file.
#pragma once
#include "batch_polish.hpp"

namespace oq {
namespace {
namespace polish {

struct JvpArgs {
  const double *Px, *Ax, *l, *u, *info, *rec;  // of the handle: raw data, the info rows and the records of the last resolve
  const double *tq, *tl, *tu, *tPx, *tAx;      // of the call: tangents, direction-major [ndir x k x cols]; nullptr: zero
  double *tx, *ty, *act, *status;               // of the call: tx, ty direction-major, act [k x m], status [k]; nullptr: not wanted
  int ndir, info_stride, rec_stride, refine;
  double delta;
  // a selection (osqp_amd_batch_jvp_rows): the workgroup at position p of the k launched serves instance sel[p]; what is
  // "of the handle" above is addressed with the instance, what is "of the call" with the position (row d * k + p of a
  // direction-major array).  nullptr: the identity
  const int *sel = nullptr;
  double *scratch = nullptr;  // LARGE (batch_polish.hpp): n x n doubles per launch position, the handle's solve scratch
};

// the rows of the call (at position pos of the `count` launched) of an instance that is not differentiated: zeros in every
// direction
__device__ __forceinline__ void jvp_zero_rows(const Pattern &P, const JvpArgs &a, int count, int pos) {
  const int tid = threadIdx.x, n = P.n, m = P.m;
  for (int d = 0; d < a.ndir; d++) {
    const size_t row = (size_t)d * count + pos;
    if (a.tx) for (int j = tid; j < n; j += PT) a.tx[row * n + j] = 0.0;
    if (a.ty) for (int i = tid; i < m; i += PT) a.ty[row * m + i] = 0.0;
  }
  if (a.act) for (int i = tid; i < m; i += PT) a.act[(size_t)pos * m + i] = 0.0;
}

template <bool LARGE>
__global__ __launch_bounds__(PT) void k_batch_jvp(Pattern P, int count, Layout L, JvpArgs a) {
  const int pos = blockIdx.x, tid = threadIdx.x, n = P.n, m = P.m;
  if (pos >= count) return;
  const int inst = a.sel ? a.sel[pos] : pos;  // wave-uniform; `count` is the launch's: k workgroups
  if ((int)a.info[(size_t)inst * a.info_stride + 1] != OSQP_SOLVED) {  // no solution to differentiate
    jvp_zero_rows(P, a, count, pos);
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
    act[i] = li == ui ? -1.0 : classify(rec[rec_z(n, m) + i], yi, li, ui);  // an equality row is always active
    y[i] = 0.0;  // the inactive rows stay zero through every direction
    z[i] = cinv * e * yi;
  }
  if (!assemble_and_factor<LARGE>(P, S, delta)) {
    jvp_zero_rows(P, a, count, pos);
    if (tid == 0 && a.status) a.status[pos] = -1.0;
    return;
  }
  // ---- the factor is done with col: the caller-unit x = D x~ of the record goes there ----
  for (int j = tid; j < n; j += PT) xc[j] = D[j] * rec[rec_x(n, m) + j];
  for (int i = tid; i < m; i += PT) if (a.act) a.act[(size_t)pos * m + i] = act[i];
  __syncthreads();

  for (int d = 0; d < a.ndir; d++) {
    const size_t row = (size_t)d * count + pos;
    // ---- the right-hand side [c D rhs_x; (E rhs_a)_a] of this direction; xc and z are complete (the barrier above, or the one
    // that ends the last kkt_step), and the x, y, q, l, ry of the direction before are read by nobody any more ----
    const double *const tP = a.tPx ? a.tPx + row * P.nnzP : nullptr, *const tA = a.tAx ? a.tAx + row * P.nnzA : nullptr;
    for (int j = tid; j < n; j += PT) {
      double px = 0.0, ay = 0.0;
      if (tP) for (int f = P.Fp[j]; f < P.Fp[j + 1]; f++) px += tP[P.Fmap[f]] * xc[P.Fc[f]];
      if (tA) for (int k = P.Ap[j]; k < P.Ap[j + 1]; k++) ay += tA[k] * z[P.Ai[k]];
      const double r = -(((a.tq ? a.tq[row * n + j] : 0.0) + px) + ay);
      q[j] = c * (r * D[j]);
    }
    for (int i = tid; i < m; i += PT) {
      const double on = act[i];
      double g = 0.0;
      if (on != 0.0) {
        double ax = 0.0;
        if (tA) for (int s = P.Rp[i]; s < P.Rp[i + 1]; s++) ax += tA[P.Rmap[s]] * xc[P.Rc[s]];
        const double *const tb = on < 0.0 ? a.tl : a.tu;
        g = ((tb ? tb[row * m + i] : 0.0) - ax) * E[i];
      }
      l[i] = g; ry[i] = g;
    }
    __syncthreads();
    for (int it = 0; it <= a.refine; it++) kkt_step<false, LARGE>(P, S, it, delta);

    // ---- back to the caller's units: tx = D x~, ty = E s / c (y is zero on the inactive rows) ----
    if (a.tx) for (int j = tid; j < n; j += PT) a.tx[row * n + j] = D[j] * x[j];
    // (no barrier: the next direction writes q, l, ry, which nobody reads here, and x, y only after kkt_step's own barriers)
    if (a.ty) for (int i = tid; i < m; i += PT) a.ty[row * m + i] = cinv * E[i] * y[i];
  }
  if (tid == 0 && a.status) a.status[pos] = 1.0;
}

}  // namespace polish
}  // namespace
}  // namespace oq
