// direct_jvp.hpp -- forward sensitivities of the solution of a single model (osqp_amd_jvp)
// Part of the direct KKT back-end and of its one translation unit: included by direct.hip after direct_adjoint.hpp, whose kept
// state (AdjointKept: the factor of the reduced KKT matrix of the active set, the slot map, the caller-unit x and y) and whose
// build it uses as they are.  With a = L u U the active rows and K = [P, Aa'; Aa, 0], one solve per direction
//   K [tx; ty_a] = [-(tq + tP x + tA' y); (tb - tA x)_a],  tb = tl on L, tu on U,  ty = 0 off a
// on the scaled data: right-hand side [c D rhs_x; (E rhs_a)_a], tx = D r~, ty = E s / c.  The new device work is that
// right-hand side: products with tangent MATRICES given as value arrays in the caller's nnz order, read through two maps from
// CSR position back to the caller's entry.  G lanes per row as in k_spmv (kernels.hip), G from the pattern alone, no atomics:
// direction d of a call has the bits of a call with that direction alone, and a missing tangent those of a tangent of zeros.
// On the iterative kept state of section 17 (mr = m, identity act_rows / slot) the same kernels run over all m rows and the
// solve masks the inactive ones; a compact workspace has no CSR arrays for the tangent products: tPx / tAx are refused there.
#pragma once
#include "engine.hpp"

namespace oq {
namespace {

// sum over the entries [s, e) of one CSR row of tv[map ? map[k] : k] * x[ci[k]], lane-strided over the G lanes of the row's
// group, 4 accumulators per lane, xor-shuffle reduction: every lane of the group returns the sum
template <int G>
__device__ __forceinline__ double jvp_row_dot(int lane, int64_t s, int64_t e, const int *__restrict__ ci, const int *__restrict__ map,
                                              const double *__restrict__ tv, const double *__restrict__ x) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int64_t k = s + lane;
  if (map) {
    for (; k + 3 * G < e; k += 4 * G) {
      const int c0 = ci[k], c1 = ci[k + G], c2 = ci[k + 2 * G], c3 = ci[k + 3 * G];
      const int e0 = map[k], e1 = map[k + G], e2 = map[k + 2 * G], e3 = map[k + 3 * G];
      a0 += tv[e0] * x[c0]; a1 += tv[e1] * x[c1]; a2 += tv[e2] * x[c2]; a3 += tv[e3] * x[c3];
    }
    for (; k < e; k += G) a0 += tv[map[k]] * x[ci[k]];
  } else {
    for (; k + 3 * G < e; k += 4 * G) {
      const int c0 = ci[k], c1 = ci[k + G], c2 = ci[k + 2 * G], c3 = ci[k + 3 * G];
      const double v0 = tv[k], v1 = tv[k + G], v2 = tv[k + 2 * G], v3 = tv[k + 3 * G];
      a0 += v0 * x[c0]; a1 += v1 * x[c1]; a2 += v2 * x[c2]; a3 += v3 * x[c3];
    }
    for (; k < e; k += G) a0 += tv[k] * x[ci[k]];
  }
  double acc = (a0 + a1) + (a2 + a3);
#pragma unroll
  for (int o = G >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  return acc;
}

// the n variable rows: rhs[j] = c D[j] (-(tq[j] + (tP x)[j] + (tA' y)[j])).  Row j of Pf with the tangent values fetched
// through Ppos2k, row j of A' (the sorted CSC copy of A: its own order is tAx's) with tAx as it lies.  A missing tangent is a
// literal 0.0 in the same sum (a product with finite x, y adds +0.0 to an accumulator that starts at +0.0: the same bits).
template <int G>
__global__ __launch_bounds__(kBlock) void k_jvp_rhs_x(int n, double c, const double *__restrict__ D, const int64_t *__restrict__ Prp,
                                                      const int *__restrict__ Pci, const int *__restrict__ Ppos2k,
                                                      const double *__restrict__ tPx, const int64_t *__restrict__ Arp,
                                                      const int *__restrict__ Aci, const double *__restrict__ tAx,
                                                      const double *__restrict__ x, const double *__restrict__ y,
                                                      const double *__restrict__ tq, double *__restrict__ rhs) {
  const int lane = threadIdx.x & (G - 1);
  const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
  if (row >= n) return;  // G divides the block: a group leaves as a whole
  const double sP = tPx ? jvp_row_dot<G>(lane, Prp[row], Prp[row + 1], Pci, Ppos2k, tPx, x) : 0.0;
  const double sA = tAx ? jvp_row_dot<G>(lane, Arp[row], Arp[row + 1], Aci, nullptr, tAx, y) : 0.0;
  if (lane == 0) rhs[row] = c * (D[row] * -((tq ? tq[row] : 0.0) + sP + sA));
}

// the mr active rows, in the order of the reduced matrix: rhs[n + k] = E[i] (tb_i - (tA x)[i]), i = act_rows[k], tb by the
// side of the row (a row with l == u is lower: only tl is read).  Row i of A (CSR) with the tangent values through Apos2k.
// Inactive rows are never visited.
template <int G>
__global__ __launch_bounds__(kBlock) void k_jvp_rhs_a(int n, int mr, const double *__restrict__ E, const int *__restrict__ act_rows,
                                                      const double *__restrict__ side, const int64_t *__restrict__ rp,
                                                      const int *__restrict__ ci, const int *__restrict__ Apos2k,
                                                      const double *__restrict__ tAx, const double *__restrict__ x,
                                                      const double *__restrict__ tl, const double *__restrict__ tu,
                                                      double *__restrict__ rhs) {
  const int lane = threadIdx.x & (G - 1);
  const int64_t k = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
  if (k >= mr) return;
  const int i = act_rows[k];
  const double s = tAx ? jvp_row_dot<G>(lane, rp[i], rp[i + 1], ci, Apos2k, tAx, x) : 0.0;
  if (lane == 0) {
    const double *tb = side[i] < 0.0 ? tl : tu;
    rhs[n + k] = E[i] * ((tb ? tb[i] : 0.0) - s);
  }
}

// tx = D r~ (threads [0, n)); ty_i = E[i] s[slot[i]] / c on the active rows, 0 elsewhere (threads [n, n + m)): a gather through
// slot, one thread per output word.  tx, ty may be null (not wanted).
__global__ __launch_bounds__(kBlock) void k_jvp_out(int n, int m, double c, const double *__restrict__ D, const double *__restrict__ E,
                                                    const int *__restrict__ slot, const double *__restrict__ sol, double *__restrict__ tx,
                                                    double *__restrict__ ty) {
  const int o = blockIdx.x * kBlock + threadIdx.x;
  if (o < n) {
    if (tx) tx[o] = D[o] * sol[o];
  } else if (o < n + m) {
    const int i = o - n, k = slot[i];
    if (ty) ty[i] = k >= 0 ? E[i] * sol[n + k] / c : 0.0;
  }
}

// the two launches of one direction's right-hand side into K.rhs_red; tA_sorted: tAx in the order of the sorted CSC copy
void jvp_rhs(Engine &e, ModelAdjoint &A, const double *tq, const double *tl, const double *tu, const double *tPx, const double *tA_sorted) {
  AdjointKept &K = *A.kept;
  hipStream_t s = e.stream;
  const int n = e.n, mr = K.mr;
  // lanes per row from the pattern alone: the rows of Pf and of A' together for the variable rows, A's own for the active rows
  const int Gx = pick_group(n, e.Pf.nnz + e.nnzA), Ga = e.A.group;
  {
    dim3 grid(blocks_for((int64_t)n * Gx)), block(kBlock);
#define OQ_JVP_X(GG) \
  OQ_LAUNCH(k_jvp_rhs_x<GG>, grid, block, 0, s, n, e.c, e.D.get(), e.Pf.rowptr.get(), e.Pf.col.get(), A.Ppos2k.get(), tPx, e.At.rowptr.get(), \
            e.At.col.get(), tA_sorted, K.xc.get(), K.yc.get(), tq, K.rhs_red.get())
    switch (Gx) {
    case 1: OQ_JVP_X(1); break;
    case 2: OQ_JVP_X(2); break;
    case 4: OQ_JVP_X(4); break;
    case 8: OQ_JVP_X(8); break;
    case 16: OQ_JVP_X(16); break;
    case 32: OQ_JVP_X(32); break;
    default: OQ_JVP_X(64); break;
    }
#undef OQ_JVP_X
  }
  if (mr > 0) {  // (an empty grid is an error)
    dim3 grid(blocks_for((int64_t)mr * Ga)), block(kBlock);
#define OQ_JVP_A(GG) \
  OQ_LAUNCH(k_jvp_rhs_a<GG>, grid, block, 0, s, n, mr, e.E.get(), K.act_rows.get(), K.side.get(), e.A.rowptr.get(), e.A.col.get(), A.Apos2k.get(), \
            tA_sorted, K.xc.get(), tl, tu, K.rhs_red.get())
    switch (Ga) {
    case 1: OQ_JVP_A(1); break;
    case 2: OQ_JVP_A(2); break;
    case 4: OQ_JVP_A(4); break;
    case 8: OQ_JVP_A(8); break;
    case 16: OQ_JVP_A(16); break;
    case 32: OQ_JVP_A(32); break;
    default: OQ_JVP_A(64); break;
    }
#undef OQ_JVP_A
  }
}

}  // namespace

int model_jvp_run(Engine &e, const char *who, bool dev, int ndir, const double *tq, const double *tl, const double *tu,
                  const double *tPx, const double *tAx, double *tx, double *ty, double *act) {
  ModelAdjoint &A = kept_state(e, who, "form");
  AdjointKept &K = *A.kept;
  hipStream_t s = e.stream;
  const int n = e.n, m = e.m;
  // a tangent of an array without entries has nothing to say
  if (m == 0) { tl = tu = nullptr; }
  if (e.nnzPtriu == 0) tPx = nullptr;
  if (e.nnzA == 0) tAx = nullptr;
  // section 17: the products with tangent matrices read the CSR arrays through Ppos2k / Apos2k; on the slices they are not built
  if ((tPx && (e.Pf.compact || e.Pi_keep.n == 0)) || (tAx && (e.A.compact || e.At.compact)))
    throw Error(6, std::string(who) + ": matrix tangents (tPx, tAx) are not available on a compact workspace (its CSR arrays are released and the products on the "
                       "sliced copy are not built; tq, tl, tu are served, and osqp_amd_adjoint gives dPx / dAx there)");
  if ((tPx || tAx) && !A.jvp_maps) {
    A.Ppos2k.alloc(std::max<int64_t>(1, e.Pf.nnz)); A.Apos2k.alloc(std::max<int64_t>(1, e.nnzA));
    A.Ppos2k.zero(s); A.Apos2k.zero(s);  // (every position is written below; an index that is read is in range in any case)
    invert_map(e.nnzPtriu, e.P_k2lo.get(), 0, e.Pf.nnz, A.Ppos2k.get(), s);
    invert_map(e.nnzPtriu, e.P_k2up.get(), 0, e.Pf.nnz, A.Ppos2k.get(), s);  // -1 on the diagonal: outside [0, nnz), it counts once
    invert_map(e.nnzA, e.A_k2pos.get(), 0, e.nnzA, A.Apos2k.get(), s);
    e.device_A_to_sorted();
    e.sync();
    A.jvp_maps = true;
  }
  if (tx || ty) {
    const size_t nd = (size_t)ndir, nzP = (size_t)e.nnzPtriu, nzA = (size_t)e.nnzA;
    Staged st(e, dev);
    const double *pq = st.in(tq, nd * n), *pl = st.in(tl, nd * m), *pu = st.in(tu, nd * m), *pP = st.in(tPx, nd * nzP), *pA = st.in(tAx, nd * nzA);
    double *px = st.out(tx, nd * n), *py = st.out(m > 0 ? ty : nullptr, nd * m);
    const int64_t *to_sorted = tAx ? e.device_A_to_sorted() : nullptr;
    DevBuf<double> dAs;  // one direction's tAx in sorted order, for a caller whose columns came unsorted
    if (to_sorted) dAs.alloc(nzA);
    with_tree_retry(e, A, [&]() {
      for (size_t d = 0; d < nd; d++) {
        const double *tA_d = pA ? pA + d * nzA : nullptr;
        if (to_sorted) {
          permute_vals(e.nnzA, to_sorted, tA_d, dAs.get(), s);
          tA_d = dAs.get();
        }
        jvp_rhs(e, A, pq ? pq + d * n : nullptr, pl ? pl + d * m : nullptr, pu ? pu + d * m : nullptr, pP ? pP + d * nzP : nullptr, tA_d);
        kept_solve(e, A);
        OQ_LAUNCH(k_jvp_out, dim3(blocks_for((int64_t)n + m)), dim3(kBlock), 0, s, n, m, e.c, e.D.get(), e.E.get(), K.slot.get(), K.sol.get(),
                  px ? px + d * n : nullptr, py ? py + d * m : nullptr);
      }
    });
    st.deliver();
  }
  write_act(e, K, act, dev);
  return 0;
}

}  // namespace oq
