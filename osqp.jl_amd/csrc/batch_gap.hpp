// batch_gap.hpp -- primal objective, dual objective and duality gap of the resident batch (osqp_amd_batch_duality, DESIGN.md
// section 19): a kernel of its own, like k_batch_cert, launched by the reading call and by nothing else; nothing of it is
// inside the ADMM loop of k_batch_quad / k_batch_solve.
//
// One workgroup per instance.  It reads the instance's record (D, E, c and the scaled iterate a resolve -- or an accepted
// polish -- left there), its RAW data in the handle and the shared pattern, forms the caller's pair x = D x~, y = E y~ / c
// with the expressions that wrote the caller's rows, and sums, each thread its strided share in index order, then the
// wavefront tree, then the four wavefronts in order (the same bits on every call):
//   x'Px (rows of the full symmetric P), q'x, SC = sum_i u_i max(yh_i, 0) + l_i min(yh_i, 0)
// yh: y projected onto the polar of the recession cone of [l, u]; a bound is infinite by the test of the solve kernels on the
// scaled bound (B_INF) and then adds 0.  Row p of the output: prim_obj, dual_obj, gap; NaN where the instance's own last
// resolve left no solution.  The handle is only read.
#pragma once
#include "batch_common.hpp"

namespace oq {
namespace {
namespace gap {

constexpr int GT = 256;

struct Args {
  const double *Px, *q, *l, *u;  // the handle's raw data
  const double *info;            // info_all: [count x info_stride], the row of every instance's own last resolve
  const double *rec;             // the records
  double *out;                   // [launch x 3]
  int info_stride, rec_stride;
  const int *sel;                // the instance of each workgroup (nullptr: its own number)
};

// the sum over the workgroup in a fixed order, the same value in every thread; `red` holds one double per wavefront
__device__ __forceinline__ double block_sum(double v, double *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();  // the previous use of red is over
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__host__ __device__ inline bool status_no_solution(int s) { return status_prim_inf(s) || status_dual_inf(s) || s == OSQP_NON_CVX; }

__global__ __launch_bounds__(GT) void k_batch_gap(Pattern P, int count, Args a) {
  __shared__ double red[GT / 64];
  const int pos = blockIdx.x, tid = threadIdx.x, n = P.n, m = P.m;
  if (pos >= count) return;
  const int inst = a.sel ? a.sel[pos] : pos;
  double *const out = a.out + (size_t)pos * 3;
  if (status_no_solution((int)a.info[(size_t)inst * a.info_stride + 1])) {
    if (tid < 3) out[tid] = NAN;
    return;
  }
  const double *const rec = a.rec + (size_t)inst * a.rec_stride;
  const double *const D = rec + rec_D(n, m), *const E = rec + rec_E(n, m);
  const double *const xs = rec + rec_x(n, m), *const ys = rec + rec_y(n, m);
  const double cinv = 1.0 / rec[REC_C];
  const double *const Pxi = a.Px + (size_t)inst * P.nnzP, *const qi = a.q + (size_t)inst * n;
  double xpx = 0.0, qx = 0.0, sc = 0.0;
  for (int j = tid; j < n; j += GT) {
    const double xj = D[j] * xs[j];
    double px = 0.0;
    for (int f = P.Fp[j]; f < P.Fp[j + 1]; f++) { const int k = P.Fc[f]; px += Pxi[P.Fmap[f]] * (D[k] * xs[k]); }
    xpx += xj * px;
    qx += qi[j] * xj;
  }
  for (int i = tid; i < m; i += GT) {
    const double e = E[i], yi = cinv * e * ys[i];
    const double li = fmax(a.l[(size_t)inst * m + i], -OSQP_INFTY), ui = fmin(a.u[(size_t)inst * m + i], OSQP_INFTY);
    sc += support_term(li, ui, yi, li * e, ui * e);
  }
  xpx = block_sum(xpx, red);
  qx = block_sum(qx, red);
  sc = block_sum(sc, red);
  if (tid == 0) {
    out[0] = 0.5 * xpx + qx;
    out[1] = -0.5 * xpx - sc;
    out[2] = (xpx + qx) + sc;
  }
}

}  // namespace gap
}  // namespace
}  // namespace oq
