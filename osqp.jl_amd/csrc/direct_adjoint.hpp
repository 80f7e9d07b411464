// direct_adjoint.hpp -- adjoint derivatives of the solution of a single model (osqp_amd_adjoint)
// Part of the direct KKT back-end and of its one translation unit: included by direct.hip after polish_run (like the
// direct_*_kernels.hpp files it is a piece of that file, not a header for anybody else), whose factor object (LdlFactor,
// reduced_factor) and whose solve-and-refine loop (kkt_solve_refine: one function for both) it uses with another right-hand side.  With a = L u U the active rows and K = [P, Aa'; Aa, 0], one solve
// K [r_x; r_a] = [g_x; (g_y)_a] per cotangent gives dq = -r_x, dl / du = r_y on L / U, dPx(i, j) = -(r_x,i x_j + r_x,j x_i) (once
// on the diagonal), dAx(i, j) = -(y_i r_x,j + r_y,i x_j).  The solve runs on the scaled data: [P~ + delta I, A~a'; A~a, -delta I]
// factorised once per solution and KEPT, the right-hand side c D g_x and (E g_y)_a, r_x = D r~, r_y = E s / c.
// Every kernel is one thread per output word, consecutive lanes on consecutive words, gathers through L2, no atomics: two calls
// give the same bits.
#pragma once
#include "engine.hpp"

namespace oq {
namespace {

// rhs = [c (D g_x) ; (E g_y) on the active rows, in the order of the reduced matrix]; a missing cotangent is zero
__global__ __launch_bounds__(kBlock) void k_adj_rhs(int n, int mr, double c, const double *__restrict__ D, const double *__restrict__ E,
                                                    const int *__restrict__ act_rows, const double *__restrict__ gx,
                                                    const double *__restrict__ gy, double *__restrict__ rhs) {
  const int o = blockIdx.x * kBlock + threadIdx.x;
  if (o >= n + mr) return;
  if (o < n) rhs[o] = gx ? c * (D[o] * gx[o]) : 0.0;
  else {
    const int i = act_rows[o - n];
    rhs[o] = gy ? E[i] * gy[i] : 0.0;
  }
}

// the caller-unit solution the matrix gradients multiply by: x = D x~, y = E y~ / c (once per kept factor)
__global__ __launch_bounds__(kBlock) void k_adj_unscale(int n, int m, double c, const double *__restrict__ D, const double *__restrict__ E,
                                                        const double *__restrict__ xs, const double *__restrict__ ys,
                                                        double *__restrict__ x, double *__restrict__ y) {
  const int o = blockIdx.x * kBlock + threadIdx.x;
  if (o < n) x[o] = D[o] * xs[o];
  else if (o < n + m) { const int i = o - n; y[i] = E[i] * ys[i] / c; }
}

// vectors: r_x = D r~ and dq = -r_x (threads [0, n)); r_y = E s / c on the active rows, 0 elsewhere, dl / du by the side of the
// row (threads [n, n + m)).  Row i finds its multiplier through slot[i] (its position in the reduced matrix, -1: inactive):
// a gather, so no thread writes another's word.  dq, dl, du may be null (not wanted); rx, ry feed the matrix kernels.
__global__ __launch_bounds__(kBlock) void k_adj_vectors(int n, int m, double c, const double *__restrict__ D, const double *__restrict__ E,
                                                        const int *__restrict__ slot, const double *__restrict__ side,
                                                        const double *__restrict__ sol, double *__restrict__ rx, double *__restrict__ ry,
                                                        double *__restrict__ dq, double *__restrict__ dl, double *__restrict__ du) {
  const int o = blockIdx.x * kBlock + threadIdx.x;
  if (o < n) {
    const double r = D[o] * sol[o];
    rx[o] = r;
    if (dq) dq[o] = -r;
  } else if (o < n + m) {
    const int i = o - n, k = slot[i];
    const double r = k >= 0 ? E[i] * sol[n + k] / c : 0.0, sd = side[i];
    ry[i] = r;
    if (dl) dl[i] = sd < 0.0 ? r : 0.0;
    if (du) du[i] = sd > 0.0 ? r : 0.0;
  }
}

// dPx: entry k of the caller's triu(P), row Pi[k], column Pcol[k] (expanded once per workspace)
__global__ __launch_bounds__(kBlock) void k_adj_dP(int64_t nnz, const int *__restrict__ Pi, const int *__restrict__ Pcol,
                                                   const double *__restrict__ rx, const double *__restrict__ x, double *__restrict__ dP) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= nnz) return;
  const int i = Pi[k], j = Pcol[k];
  dP[k] = i == j ? -(rx[i] * x[i]) : -(rx[i] * x[j] + rx[j] * x[i]);
}

// dAx: entry k of the caller's A; to_sorted (may be null) translates a caller index into the sorted copy the workspace holds
__global__ __launch_bounds__(kBlock) void k_adj_dA(int64_t nnz, const int64_t *__restrict__ to_sorted, const int *__restrict__ Ai,
                                                   const int *__restrict__ Acol, const double *__restrict__ rx, const double *__restrict__ ry,
                                                   const double *__restrict__ x, const double *__restrict__ y, double *__restrict__ dA) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= nnz) return;
  const int64_t ks = to_sorted ? to_sorted[k] : k;
  const int i = Ai[ks], j = Acol[ks];
  dA[k] = -(y[i] * rx[j] + ry[i] * x[j]);
}

// what one solution keeps: the factor, the active set in its three forms, the caller-unit solution, the scratch of the solves
struct AdjointKept {
  std::unique_ptr<LdlFactor> F;
  int n_low = 0, n_upp = 0, mr = 0;
  std::vector<double> h_side;                   // [m] -1 lower, 0 inactive, 1 upper (the `act` output)
  DevBuf<int> act_rows, slot;                   // [mr] rows in the order of the reduced matrix; [m] row -> position, -1
  DevBuf<double> side, xc, yc;                  // [m], [n], [m]
  DevBuf<double> rhs_red, sol, rhs, yfull, Axv, px, ared_x, rx, ry;
  size_t bytes = 0;                             // device bytes held (factor, index arrays, scratch)
};

}  // namespace

struct ModelAdjoint {
  std::unique_ptr<AdjointKept> kept;
  DevBuf<int> Pcol, Acol;          // column of every entry of the caller's triu(P) / of A (sorted copy): once per workspace
  bool patterns = false;
  // osqp_amd_jvp (direct_jvp.hpp): for every position of Pf the entry of the caller's triu(P) it mirrors, for every position
  // of A (CSR) the entry of the sorted CSC copy -- P_k2lo / P_k2up / A_k2pos inverted, at the first call with tPx or tAx
  DevBuf<int> Ppos2k, Apos2k;
  bool jvp_maps = false;
  long long builds = 0, solves = 0;
};
void model_adjoint_destroy(ModelAdjoint *a) { delete a; }

void model_adjoint_release(Engine &e) {
  if (e.adj && e.adj->kept) { e.sync(); e.adj->kept.reset(); }
}

void model_adjoint_stats(const Engine &e, double out[6]) {
  const ModelAdjoint *a = e.adj.get();
  const AdjointKept *k = a ? a->kept.get() : nullptr;
  out[0] = a ? (double)a->builds : 0.0;
  out[1] = a ? (double)a->solves : 0.0;
  out[2] = k ? (double)k->n_low : 0.0;
  out[3] = k ? (double)k->n_upp : 0.0;
  out[4] = k ? 1.0 : 0.0;
  out[5] = k ? (double)k->bytes : 0.0;
}

namespace {

// classify the rows on the scaled (z, y, l, u) of the solution -- polish's rule, and a row with l == u is always active and
// counts as lower --, analyse and factorise the reduced matrix, set up what every later call on this solution reuses
void adjoint_build(Engine &e, ModelAdjoint &A, const char *who, const char *form) {
  hipStream_t s = e.stream;
  const int n = e.n, m = e.m;
  const size_t bytes0 = g_device_bytes;
  std::unique_ptr<AdjointKept> K(new AdjointKept());
  std::vector<double> hz(m), hy(m), hl(m), hu(m);
  e.z.download(hz.data(), m, s); e.y.download(hy.data(), m, s); e.l.download(hl.data(), m, s); e.u.download(hu.data(), m, s);
  e.sync();
  K->h_side.assign(m, 0.0);
  std::vector<int> row_map(m, -1), rows;
  for (int i = 0; i < m; i++) {
    const bool low = (hz[i] - hl[i] < -hy[i]) || hl[i] == hu[i];
    const bool upp = !low && (hu[i] - hz[i] < hy[i]);
    K->h_side[i] = low ? -1.0 : (upp ? 1.0 : 0.0);
    if (low) K->n_low++;
    if (upp) K->n_upp++;
  }
  const int mr = K->mr = K->n_low + K->n_upp;
  rows.resize(mr);
  for (int i = 0, kl = 0, ku = K->n_low; i < m; i++) {  // lower rows first, as polish orders its reduced matrix
    if (K->h_side[i] < 0.0) { row_map[i] = kl; rows[kl++] = i; }
    else if (K->h_side[i] > 0.0) { row_map[i] = ku; rows[ku++] = i; }
  }
  int frc = 0;
  K->F = reduced_factor(e, row_map, mr, &frc);
  if (frc == -1)
    throw Error(6, std::string(who) + ": the factor of the reduced KKT matrix of the active set is too large for the device (an iterative " + form + " is not built)");
  if (frc != 0)
    throw Error(4, std::string(who) + ": the numeric factorisation of the regularised KKT matrix of the active set failed");
  const int nr = n + mr;
  K->act_rows.alloc(mr ? mr : 1); K->act_rows.upload(rows.data(), mr, s);
  K->slot.alloc(m ? m : 1); K->slot.upload(row_map.data(), m, s);
  K->side.alloc(m ? m : 1); K->side.upload(K->h_side.data(), m, s);
  K->xc.alloc(n); K->yc.alloc(m ? m : 1);
  K->rhs_red.alloc(nr); K->sol.alloc(nr); K->rhs.alloc(nr); K->yfull.alloc(m ? m : 1); K->Axv.alloc(m ? m : 1); K->px.alloc(n);
  K->ared_x.alloc(mr ? mr : 1); K->rx.alloc(n); K->ry.alloc(m ? m : 1);
  OQ_LAUNCH(k_adj_unscale, dim3(blocks_for((int64_t)n + m)), dim3(kBlock), 0, s, n, m, e.c, e.D.get(), e.E.get(), e.x.get(), e.y.get(),
            K->xc.get(), K->yc.get());
  e.sync();  // (the uploads above read host vectors of this scope)
  K->bytes = g_device_bytes > bytes0 ? g_device_bytes - bytes0 : 0;
  A.kept = std::move(K);
  A.builds++;
}

// the solve on the kept factor from K.rhs_red to K.sol: the regularised solve, polish_refine_iter steps against the
// unregularised matrix (the loop of polish_run on scratch of its own: the engine's Ax / Px / Aty keep what the last residual
// evaluation left).  polish_refine_iter = 0 asks for the regularised answer itself.  The factorisation does not pivot and
// eliminates rows of -delta before their variables wherever the fill-reducing order says so: multipliers of 1 / delta, a solve
// accurate to ~1e-8 where the matrix has a condition of 1e3 (control(): 1.0e-8 against a dense solve; the steps against the
// unregularised matrix remove that as well, which is why polish never sees it).  So with 0 steps ONE step runs against
// the REGULARISED matrix: the answer is the regularised one, to working accuracy.
void kept_solve(Engine &e, ModelAdjoint &A) {
  AdjointKept &K = *A.kept;
  const bool regularised = e.st.polish_refine_iter == 0;
  A.solves += kkt_solve_refine(e, *K.F, K.act_rows.get(), K.mr, K.rhs_red.get(), K.sol.get(),
                               RefineScratch{K.rhs.get(), K.yfull.get(), K.Axv.get(), K.px.get(), K.ared_x.get()},
                               regularised ? 1 : (int)e.st.polish_refine_iter, regularised);
}

// one cotangent: right-hand side and solve
void adjoint_pass(Engine &e, ModelAdjoint &A, const double *gx, const double *gy) {
  AdjointKept &K = *A.kept;
  const int n = e.n, mr = K.mr;
  OQ_LAUNCH(k_adj_rhs, dim3(blocks_for(n + mr)), dim3(kBlock), 0, e.stream, n, mr, e.c, e.D.get(), e.E.get(), K.act_rows.get(), gx, gy, K.rhs_red.get());
  kept_solve(e, A);
}

// no CSR arrays and no reduced KKT matrix: what polish_run hands to its iterative form
void adjoint_needs_csr(const Engine &e, const char *who, const char *form) {
  if (e.comm)
    throw Error(6, std::string(who) + ": not available on a row-sharded workspace (a row block has no reduced KKT matrix; an iterative " + form + " is not built)");
  if (e.compact || e.A.compact || e.At.compact || e.Pf.compact || (e.nnzPtriu > 0 && e.Pi_keep.n == 0))
    throw Error(6, std::string(who) + ": not available on a compact workspace (its CSR arrays are released, there is no reduced KKT matrix to factorise; "
                   "an iterative " + form + " is not built; OSQP_AMD_COMPACT_NNZ=-1 at setup keeps the arrays)");
}

// ---- the driver model_adjoint_run and model_jvp_run (direct_jvp.hpp) share ----
// the workspace's derivative state with what the current solution keeps present (built by the first call after a solve);
// who: the exported symbol that was called, form: what its refusals say is not built
ModelAdjoint &kept_state(Engine &e, const char *who, const char *form) {
  adjoint_needs_csr(e, who, form);
  if (!e.adj) e.adj.reset(new ModelAdjoint());
  if (!e.adj->kept) adjoint_build(e, *e.adj, who, form);
  return *e.adj;
}

// The operands of one call as device arrays.  Device form: the caller's arrays themselves.  Host form: in() gives an uploaded
// copy, out() a fresh device array that deliver() downloads into the caller's; a null operand stays null and allocates nothing.
// Every refusal (the checks of the C boundary, kept_state) lies before the first kernel, and deliver() comes after the passes:
// a call that fails has written nothing (device form: the re-run of with_tree_retry overwrites what a faulted pass wrote; only a
// second tree fault, an internal error, leaves partial output behind).
struct Staged {
  Engine &e;
  bool dev;
  struct Out { double *host; size_t at, count; };
  std::vector<DevBuf<double>> held;
  std::vector<Out> outs;
  Staged(Engine &e_, bool dev_) : e(e_), dev(dev_) {}
  ~Staged() { while (!held.empty()) held.pop_back(); }  // released last-allocated first, as a function's local buffers are
  const double *in(const double *p, size_t count) {
    if (dev || !p) return p;
    held.emplace_back(count);
    held.back().upload(p, count, e.stream);
    return held.back().get();
  }
  double *out(double *p, size_t count) {
    if (dev || !p) return p;
    held.emplace_back(count);
    outs.push_back({p, held.size() - 1, count});
    return held.back().get();
  }
  void deliver() {
    if (dev) return;
    for (const Out &o : outs) held[o.at].download(o.host, o.count, e.stream);
    e.sync();
  }
};

// passes() with the one re-run a supernodal tree fault is answered with
template <typename F>
void with_tree_retry(Engine &e, ModelAdjoint &A, F &&passes) {
  AdjointKept &K = *A.kept;
  const long long solves0 = A.solves;
  passes();
  e.sync();
  if (K.F->faulted()) {  // a wait inside the one-launch supernodal solve timed out: one launch per level, and once more
    *K.F->sn_fault_host = 0;
    K.F->sn_tree = false;
    A.solves = solves0;
    passes();
    e.sync();
    if (K.F->faulted()) throw TreeFault();
  }
}

// the `act` output: [m] -1 lower, 0 inactive, 1 upper
void write_act(Engine &e, const AdjointKept &K, double *act, bool dev) {
  if (!act) return;
  if (dev) { e.copy_dev(act, K.side.get(), (size_t)e.m); e.sync(); }
  else std::copy(K.h_side.begin(), K.h_side.end(), act);
}

}  // namespace

int model_adjoint_run(Engine &e, const char *who, bool dev, int ncot, const double *dx, const double *dy, double *dq, double *dl,
                      double *du, double *dPx, double *dAx, double *act) {
  ModelAdjoint &A = kept_state(e, who, "adjoint");
  AdjointKept &K = *A.kept;
  hipStream_t s = e.stream;
  const int n = e.n, m = e.m;
  if ((dPx || dAx) && !A.patterns) {
    A.Pcol.alloc(std::max<int64_t>(1, e.nnzPtriu)); A.Acol.alloc(std::max<int64_t>(1, e.nnzA));
    expand_colptr(n, e.Pp_keep.get(), e.nnzPtriu, A.Pcol.get(), s);
    expand_colptr(n, e.At.rowptr.get(), e.nnzA, A.Acol.get(), s);
    e.device_A_to_sorted();
    e.sync();
    A.patterns = true;
  }
  if (dq || dl || du || dPx || dAx) {
    const size_t nc = (size_t)ncot, nzP = (size_t)e.nnzPtriu, nzA = (size_t)e.nnzA;
    Staged st(e, dev);
    const double *gx = st.in(dx, nc * n), *gy = st.in(m > 0 ? dy : nullptr, nc * m);
    double *oq_ = st.out(dq, nc * n), *ol = st.out(dl, nc * m), *ou = st.out(du, nc * m), *oP = st.out(dPx, nc * nzP), *oA = st.out(dAx, nc * nzA);
    const int64_t *to_sorted = dAx ? e.device_A_to_sorted() : nullptr;
    with_tree_retry(e, A, [&]() {
      for (size_t c = 0; c < nc; c++) {
        adjoint_pass(e, A, gx ? gx + c * n : nullptr, gy ? gy + c * m : nullptr);
        OQ_LAUNCH(k_adj_vectors, dim3(blocks_for((int64_t)n + m)), dim3(kBlock), 0, s, n, m, e.c, e.D.get(), e.E.get(), K.slot.get(), K.side.get(),
                  K.sol.get(), K.rx.get(), K.ry.get(), oq_ ? oq_ + c * n : nullptr, ol ? ol + c * m : nullptr, ou ? ou + c * m : nullptr);
        if (dPx && e.nnzPtriu > 0)
          OQ_LAUNCH(k_adj_dP, dim3(blocks_for(e.nnzPtriu)), dim3(kBlock), 0, s, e.nnzPtriu, e.Pi_keep.get(), A.Pcol.get(), K.rx.get(), K.xc.get(),
                    oP + c * nzP);
        if (dAx && e.nnzA > 0)
          OQ_LAUNCH(k_adj_dA, dim3(blocks_for(e.nnzA)), dim3(kBlock), 0, s, e.nnzA, to_sorted,
                    e.At.col.get(), A.Acol.get(), K.rx.get(), K.ry.get(), K.xc.get(), K.yc.get(), oA + c * nzA);
      }
    });
    st.deliver();
  }
  write_act(e, K, act, dev);
  return 0;
}

}  // namespace oq
