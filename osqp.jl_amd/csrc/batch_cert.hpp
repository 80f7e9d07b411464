// batch_cert.hpp -- infeasibility certificates of the resident batch (osqp_amd_batch_certificates): a kernel of its own,
// launched by osqp_amd_batch_resolve right after the solve launch; nothing of it is inside the ADMM loop.
//
// A solve launched with RES_CERT (batch_common.hpp) leaves, for an instance that ended primal infeasible, the scaled and
// projected delta_y in the y slot of its record, and for one that ended dual infeasible the scaled delta_x in the x slot
// (caller's numbering) -- the slots that hold zeros for an instance without a solution.  k_batch_cert reads the status from
// the info row and, for those instances, does what the oracle does between update_status and store_solution: multiply by E
// (delta_y) or D (delta_x) when the termination criteria are in the caller's units (scaling on, scaled_termination off),
// divide by the infinity norm, and write the row into the handle's certificate buffers; the slot gets its zeros back, so the
// records are what a solve without RES_CERT leaves.  Every other row of the two buffers is NaN.  One workgroup per instance.
#pragma once
#include "batch_common.hpp"

namespace oq {
namespace {
namespace cert {

constexpr int CT = 256;

struct Args {
  const double *info;  // the info rows the solve has just written
  double *rec;         // the records
  double *prim, *dual; // [count x m], [count x n] of the handle (prim nullptr when m = 0)
  int info_stride, rec_stride, unscaled;
  const int *sel;      // the instance of each workgroup (nullptr: its own number); the info rows are the workgroups'
};

// max over the workgroup, the same value in every thread; `red` holds one double per wavefront
__device__ __forceinline__ double block_max(double v, double *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  __syncthreads();  // the previous use of red is over
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = red[0];
#pragma unroll
  for (int w = 1; w < CT / 64; w++) v = fmax(v, red[w]);
  return v;
}

// slot[0 .. len) of the record times scale[] (when unscaled), over its infinity norm -> out[0 .. len); slot <- 0
__device__ __forceinline__ void normalise_row(double *slot, const double *scale, int len, bool unscaled, double *out, double *red) {
  double mx = 0.0;
  for (int k = threadIdx.x; k < len; k += CT) mx = fmax(mx, fabs(unscaled ? slot[k] * scale[k] : slot[k]));
  const double nrm = block_max(mx, red);
  for (int k = threadIdx.x; k < len; k += CT) {  // the same thread read slot[k] above: no other thread depends on it
    const double v = unscaled ? slot[k] * scale[k] : slot[k];
    out[k] = v / nrm;
    slot[k] = 0.0;
  }
}

__global__ __launch_bounds__(CT) void k_batch_cert(int n, int m, int count, Args a) {
  __shared__ double red[CT / 64];
  const int pos = blockIdx.x;
  if (pos >= count) return;
  const int inst = a.sel ? a.sel[pos] : pos;
  const int status = (int)a.info[(size_t)pos * a.info_stride + 1];
  double *const rec = a.rec + (size_t)inst * a.rec_stride;
  double *const prim = a.prim ? a.prim + (size_t)inst * m : nullptr, *const dual = a.dual + (size_t)inst * n;
  if (prim) {
    if (status_prim_inf(status)) normalise_row(rec + rec_y(n, m), rec + rec_E(n, m), m, a.unscaled != 0, prim, red);
    else for (int i = threadIdx.x; i < m; i += CT) prim[i] = NAN;
  }
  if (status_dual_inf(status)) normalise_row(rec + rec_x(n, m), rec + rec_D(n, m), n, a.unscaled != 0, dual, red);
  else for (int j = threadIdx.x; j < n; j += CT) dual[j] = NAN;
}

}  // namespace cert
}  // namespace
}  // namespace oq
