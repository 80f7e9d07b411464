// batch_shared_jvp.hpp -- forward sensitivities of the solutions of the shared batch (osqp_amd_shared_batch_jvp, DESIGN.md
// section 13.5): the mathematics, the LDS slots and the loop over the directions of k_batch_jvp (batch_jvp.hpp: one solve with
// [P~, A~a'; A~a, 0] per direction on the factor of M = P~ + delta I + A~a' A~a / delta and `refine` refinement steps), fed the way
// k_shared_adjoint (batch_shared_adjoint.hpp) is fed: the scaled Av / Pv, c, D, E from the model block, the scaled iterate and the
// ALREADY SCALED l, u of instance i from the tile record, the status from the handle's status array.
//
// THE TANGENTS.  tq, tl, tu are per instance, direction-major [ndir x count x n | m]: row d * count + i.  tPx [ndir x nnzP] and
// tAx [ndir x nnzA] are SHARED, as P and A are: row d, the same for every instance -- one direction of the values of the model
// moves all `count` solutions.  tPx is the stored upper triangle (an off-diagonal entry stands for both halves), tAx is in the
// order of the Ax given at setup: the index spaces of the adjoint's dPx_sum / dAx_sum.  nullptr: zero.  On a row with l == u
// (scaled, as the record holds them) only tl is read: the row counts as lower, as in k_shared_adjoint.
//
// WHICH INSTANCES A WORKGROUP SERVES, the factor block of the LARGE form and the barrier at the head of the instance loop: as
// k_shared_adjoint, word for word -- the same W, the same buffer (the handle's adj_factor).  Nothing is carried from one instance
// or one direction to the next: the bits of (instance, direction) do not depend on count, ndir, W, the position, the neighbours
// or the outputs asked for.  An instance whose status is not OSQP_SOLVED gets zero rows and status 0, a failed Cholesky zero rows
// and status -1: both exits are workgroup-uniform.  Every store is a plain vector store; the handle is only read.
// tests/batch_jvp_ref.py (model) is the numpy model of the per-direction part.
#pragma once
#include "batch_jvp.hpp"
#include "batch_shared_adjoint.hpp"

namespace oq {
namespace {
namespace shared {

struct SharedJvpArgs {
  const double *model, *tiles, *status_in;  // of the handle
  const double *tq, *tl, *tu;               // of the call: direction-major [ndir x count x n | m | m]; nullptr: zero
  const double *tPx, *tAx;                  // of the call: [ndir x nnzP], [ndir x nnzA], shared by the instances; nullptr: zero
  double *tx, *ty;                          // outputs, direction-major [ndir x count x n | m]; nullptr: not wanted
  double *act, *status;                     // [count x m], [count]; nullptr: not wanted
  double *scratch;                          // LARGE: W blocks of n x n doubles
  int count, first, cnt, T, ndir, refine;
  double delta;
};

// the rows of an instance that is not differentiated: zeros in every direction
__device__ __forceinline__ void shared_jvp_zero_rows(const Pattern &P, const SharedJvpArgs &a, int inst) {
  const int tid = threadIdx.x, n = P.n, m = P.m;
  for (int d = 0; d < a.ndir; d++) {
    const size_t row = (size_t)d * a.count + inst;
    if (a.tx) for (int j = tid; j < n; j += polish::PT) a.tx[row * n + j] = 0.0;
    if (a.ty) for (int i = tid; i < m; i += polish::PT) a.ty[row * m + i] = 0.0;
  }
  if (a.act) for (int i = tid; i < m; i += polish::PT) a.act[(size_t)inst * m + i] = 0.0;
}

template <bool LARGE>
__global__ __launch_bounds__(polish::PT) void k_shared_jvp(Pattern P, polish::Layout L, SharedJvpArgs a) {
  using namespace polish;
  const int tid = threadIdx.x, n = P.n, m = P.m, T = a.T;
  const ModelLayout ML = model_layout(n, m, P.nnzA, P.nnzF);
  const TileLayout TL = tile_layout(n, m, T);
  Slots S = make_slots(L);
  if constexpr (LARGE) S.G = a.scratch + (size_t)blockIdx.x * n * n;
  ldouble *const q = S.q, *const x = S.x, *const xc = S.col, *const l = S.l, *const y = S.y, *const ry = S.ry, *const z = S.z, *const act = S.act;
  const double *const D = a.model + ML.D, *const E = a.model + ML.E;
  const double c = a.model[MB_C], cinv = 1.0 / c, delta = a.delta;

  // ---- the scaled matrices of the model: the same for every instance of this workgroup (synchronised by the first barrier of
  // assemble_and_factor, and never written again) ----
  for (int k = tid; k < P.nnzA; k += PT) S.Av[k] = a.model[ML.Av + k];
  for (int f = tid; f < P.nnzF; f += PT) S.Pv[f] = a.model[ML.Pv + f];

  bool again = false;
  for (int inst = a.first + blockIdx.x; inst < a.first + a.cnt; inst += gridDim.x) {  // wave-uniform
    if (again) __syncthreads();  // the instance before is done with the slots and, LARGE, with the factor block
    again = true;
    if ((int)a.status_in[inst] != OSQP_SOLVED) {  // no solution to differentiate
      shared_jvp_zero_rows(P, a, inst);
      if (tid == 0 && a.status) a.status[inst] = 0.0;
      continue;
    }
    const double *const rec = a.tiles + (size_t)(inst / T) * TL.total + inst % T;

    // ---- the active sets on the scaled iterate and the scaled bounds of the record, the caller-unit multipliers ----
    for (int i = tid; i < m; i += PT) {
      const double li = rec[TL.l + (size_t)i * T], ui = rec[TL.u + (size_t)i * T], yi = rec[TL.y + (size_t)i * T];
      const double on = li == ui ? -1.0 : classify(rec[TL.z + (size_t)i * T], yi, li, ui);  // an equality row is always active
      act[i] = on;
      if (a.act) a.act[(size_t)inst * m + i] = on;
      y[i] = 0.0;  // the inactive rows stay zero through every direction
      z[i] = cinv * E[i] * yi;
    }
    if (!assemble_and_factor<LARGE>(P, S, delta)) {
      shared_jvp_zero_rows(P, a, inst);
      if (tid == 0 && a.status) a.status[inst] = -1.0;
      continue;
    }
    // ---- the factor is done with col: the caller-unit x = D x~ of the record goes there ----
    for (int j = tid; j < n; j += PT) xc[j] = D[j] * rec[TL.x + (size_t)j * T];
    __syncthreads();  // the right-hand sides read the xc of other threads' entries

    for (int d = 0; d < a.ndir; d++) {
      const size_t row = (size_t)d * a.count + inst;
      // ---- the right-hand side [c D rhs_x; (E rhs_a)_a] of this direction; xc and z are complete (the barrier above, or the one
      // that ends the last kkt_step), and the x, y, q, l, ry of the direction before are read by nobody any more.  tP, tA: row d
      // of the shared tangents, whatever the instance ----
      const double *const tP = a.tPx ? a.tPx + (size_t)d * P.nnzP : nullptr, *const tA = a.tAx ? a.tAx + (size_t)d * P.nnzA : nullptr;
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
    if (tid == 0 && a.status) a.status[inst] = 1.0;
  }
}

}  // namespace shared
}  // namespace
}  // namespace oq
