// batch_shared_adjoint.hpp -- adjoint derivatives of the solutions of the shared batch (osqp_amd_shared_batch_adjoint, DESIGN.md
// section 13.4): the mathematics, the LDS slots and the loop over the cotangents of k_batch_adjoint (batch_adjoint.hpp: one solve
// with [P~, A~a'; A~a, 0] per cotangent through M = P~ + delta I + A~a' A~a / delta, its Cholesky factor and `refine` refinement
// steps -- stage / classify / assemble_and_factor / kkt_step of batch_polish.hpp, the factor of batch_large_factor.hpp), fed from
// the SHARED layout instead of a record row and raw data:
//   the model block (ModelLayout)   c, D, E and the scaled values -- Av in CSC order, Pv in full-symmetric CSR order, which ARE the
//                                   index spaces of Slots::Av / Slots::Pv (k_shared_factor writes model[L.Av + k] = s.Av[k], k the
//                                   CSC position, and model[L.Pv + f] = s.Pv[f], f the position in the full CSR): a plain copy, not
//                                   stage_matrices, and once per workgroup -- the values are the same for every instance;
//   the tile record (TileLayout)    the scaled iterate x, z, y and the ALREADY SCALED l, u of instance i: entry idx at
//                                   (i / T) TL.total + off + idx T + i % T;
//   the handle's status array       [count], the status_val of the last resolve (k_shared_status below).
// A row with l == u (scaled) is always active and counts as lower, as there.  An instance whose status is not OSQP_SOLVED gets
// zero rows and status 0, a failed Cholesky zero rows and status -1: both exits are workgroup-uniform.
//
// WHICH INSTANCES A WORKGROUP SERVES.  A launch covers the instances first .. first + cnt - 1; workgroup w takes first + w,
// first + w + gridDim.x, ... in a loop, with a barrier between two instances (the LDS slots are reused).  LARGE = false: M as a
// packed triangle in LDS (n <= 128).  LARGE = true: the factor in block w of the handle's factor scratch (W blocks of n x n doubles,
// W from the shape alone whatever `count` is: the host launches at most W workgroups) -- written and read by that ONE workgroup
// only, by plain vector stores and loads with the barriers of lf::assemble / lf::cholesky / lf::solve between them: the
// VISIBILITY argument stated in lf::cholesky holds instance after instance, the barrier at the head of the loop standing between
// the last loads of one instance's factor and the first stores of the next.  Nothing is carried from one instance or one cotangent to the next, and
// every sum of an instance is formed in an order its own shape fixes: the bits of (instance, cotangent) do not depend on count,
// ncot, W, the position, the neighbours or the outputs asked for.
//
// WHERE THE ROWS GO.  dq, dl, du, act, status: the call's arrays, row cot * count + i.  dPx / dAx: row cot * pcount + (i - pfirst)
// resp. cot * acount + (i - afirst) -- the call's array (pcount = count, pfirst = 0) or, where only the SUM is wanted, the
// handle's bounded row scratch, which holds the instances of one launch (pcount = cnt, pfirst = first).
//
// k_shared_reduce_rows: out[c, k] (+)= the sum over the instances of rows[c, ., k] in THE order of the contract -- blocks of 16
// consecutive instances, s_b = ((r_16b + r_16b+1) + ...) + r_16b+15, then ((s_0 + s_1) + ...) -- one thread per (c, k), plain adds
// (the library is built with -ffp-contract=off; there is no product to contract anyway), no atomics.  The order is a function
// of the number of instances alone: a launch continues the running sum of the launches before (`cont`), whose instances were
// a multiple of 16, so chunked and whole-batch calls give the same bits.
#pragma once
#include "batch_adjoint.hpp"
#include "batch_shared.hpp"

namespace oq {
namespace {
namespace shared {

constexpr int kAdjointBlocks = 256;  // the compute units of the MI355X; W, the factor blocks of the LARGE form = the workgroups of its
                                     // launch, is this or twice this, by the LDS of the shape (shared_adjoint_plan)
static_assert(kAdjointBlocks % 16 == 0, "a chunk of whole rounds of W workgroups is a multiple of the blocks of the summation order");
constexpr int kSumBlock = 16;        // instances per block of the summation order

struct SharedAdjointArgs {
  const double *model, *tiles, *status_in;  // of the handle
  const double *gx, *gy;                    // of the call: cotangent-major [ncot x count x n], [ncot x count x m]; nullptr: zero
  double *dq, *dl, *du, *dPx, *dAx;         // outputs (nullptr: not wanted); dPx / dAx by (pcount, pfirst) / (acount, afirst)
  double *act, *status;                     // [count x m], [count]; nullptr: not wanted
  double *scratch;                          // LARGE: W blocks of n x n doubles
  int count, first, cnt, T, ncot, refine;
  int pcount, pfirst, acount, afirst;
  double delta;
};

// status[i] = status_val of instance i from the info rows of the resolve that has just run
__global__ __launch_bounds__(256) void k_shared_status(int count, const double *__restrict__ info, double *__restrict__ status) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < count) status[i] = info[(size_t)i * 6 + 1];
}

// the rows of an instance that is not differentiated: zeros in every cotangent
__device__ __forceinline__ void shared_adjoint_zero_rows(const Pattern &P, const SharedAdjointArgs &a, int inst) {
  const int tid = threadIdx.x, n = P.n, m = P.m;
  for (int c = 0; c < a.ncot; c++) {
    const size_t row = (size_t)c * a.count + inst;
    if (a.dq) for (int j = tid; j < n; j += polish::PT) a.dq[row * n + j] = 0.0;
    for (int i = tid; i < m; i += polish::PT) {
      if (a.dl) a.dl[row * m + i] = 0.0;
      if (a.du) a.du[row * m + i] = 0.0;
    }
    if (a.dPx) {
      double *const dP = a.dPx + ((size_t)c * a.pcount + (inst - a.pfirst)) * P.nnzP;
      for (int k = tid; k < P.nnzP; k += polish::PT) dP[k] = 0.0;
    }
    if (a.dAx) {
      double *const dA = a.dAx + ((size_t)c * a.acount + (inst - a.afirst)) * P.nnzA;
      for (int k = tid; k < P.nnzA; k += polish::PT) dA[k] = 0.0;
    }
  }
  if (a.act) for (int i = tid; i < m; i += polish::PT) a.act[(size_t)inst * m + i] = 0.0;
}

template <bool LARGE>
__global__ __launch_bounds__(polish::PT) void k_shared_adjoint(Pattern P, polish::Layout L, SharedAdjointArgs a) {
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
      shared_adjoint_zero_rows(P, a, inst);
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
      y[i] = 0.0;  // the inactive rows stay zero through every cotangent
      z[i] = cinv * E[i] * yi;
    }
    if (!assemble_and_factor<LARGE>(P, S, delta)) {
      shared_adjoint_zero_rows(P, a, inst);
      if (tid == 0 && a.status) a.status[inst] = -1.0;
      continue;
    }
    // ---- the factor is done with col: the caller-unit x = D x~ of the record goes there ----
    for (int j = tid; j < n; j += PT) xc[j] = D[j] * rec[TL.x + (size_t)j * T];

    for (int cot = 0; cot < a.ncot; cot++) {
      const size_t row = (size_t)cot * a.count + inst;
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
      double *const dP = a.dPx ? a.dPx + ((size_t)cot * a.pcount + (inst - a.pfirst)) * P.nnzP : nullptr;
      double *const dA = a.dAx ? a.dAx + ((size_t)cot * a.acount + (inst - a.afirst)) * P.nnzA : nullptr;
      for (int j = tid; j < n; j += PT) {
        const double rj = x[j], xj = xc[j];
        if (a.dq) a.dq[row * n + j] = -rj;
        if (dP)
          for (int f = P.Fp[j]; f < P.Fp[j + 1]; f++) {  // row j of the full P; its entries cc <= j are column j of the stored triangle
            const int cc = P.Fc[f];
            if (cc == j) dP[P.Fmap[f]] = -(rj * xj);
            else if (cc < j) dP[P.Fmap[f]] = -(x[cc] * xj + rj * xc[cc]);
          }
        if (dA)
          for (int k = P.Ap[j]; k < P.Ap[j + 1]; k++) { const int i = P.Ai[k]; dA[k] = -(z[i] * rj + ry[i] * xj); }
      }
      if (cot + 1 < a.ncot) __syncthreads();  // uniform: the next right-hand side overwrites ry, its solve x
    }
    if (tid == 0 && a.status) a.status[inst] = 1.0;
  }
}

// out[c x cols + k] = (cont ? out[..] + : ) the block-of-16 sum over local instances 0 .. cnt - 1 of rows[(c rcount + i) cols + k]
__global__ __launch_bounds__(256) void k_shared_reduce_rows(int ncot, int cnt, int rcount, int cols, int cont, const double *__restrict__ rows,
                                                           double *__restrict__ out) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (size_t)ncot * cols) return;
  const int c = (int)(g / cols), k = (int)(g - (size_t)c * cols);
  const double *const r = rows + (size_t)c * rcount * cols + k;
  double total = cont ? out[g] : 0.0;
  for (int b = 0; b < cnt; b += kSumBlock) {
    double v[kSumBlock];
#pragma unroll
    for (int j = 0; j < kSumBlock; j++) v[j] = b + j < cnt ? r[(size_t)(b + j) * cols] : 0.0;
    double s = v[0];
#pragma unroll
    for (int j = 1; j < kSumBlock; j++)
      if (b + j < cnt) s = s + v[j];
    total = (b == 0 && !cont) ? s : total + s;
  }
  out[g] = total;
}

}  // namespace shared
}  // namespace
}  // namespace oq
