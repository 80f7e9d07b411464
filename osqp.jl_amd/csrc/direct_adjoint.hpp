// direct_adjoint.hpp -- adjoint derivatives of the solution of a single model (osqp_amd_adjoint)
// Part of the direct KKT back-end and of its one translation unit: included by direct.hip after polish_run (like the
// direct_*_kernels.hpp files it is a piece of that file, not a header for anybody else), whose factor object (LdlFactor,
// reduced_factor) and whose solve-and-refine loop (kkt_solve_refine: one function for both) it uses with another right-hand side.  With a = L u U the active rows and K = [P, Aa'; Aa, 0], one solve
// K [r_x; r_a] = [g_x; (g_y)_a] per cotangent gives dq = -r_x, dl / du = r_y on L / U, dPx(i, j) = -(r_x,i x_j + r_x,j x_i) (once
// on the diagonal), dAx(i, j) = -(y_i r_x,j + r_y,i x_j).  The solve runs on the scaled data: [P~ + delta I, A~a'; A~a, -delta I]
// factorised once per solution and KEPT, the right-hand side c D g_x and (E g_y)_a, r_x = D r~, r_y = E s / c.
// Every kernel is one thread per output word, consecutive lanes on consecutive words, gathers through L2, no atomics: two calls
// give the same bits.
// Section 17 (osqp_amd_derivative_method): the same drivers on a kept state WITHOUT a factor -- the solve is kkt_iter_solve of
// pcg.hip on the operator of the indirect back-end, the multipliers stay at full length m (act_rows / slot the identity), and
// the matrix gradients of a compact matrix come from a sampled outer product on its sliced copy (panel_outer) and a gather.
// Section 18 (osqp_amd_adjoint_retain): opt-in, the kept factor outlives its solution -- what moves the model on marks it
// stale, and the next derivative call counts on the device the rows that changed side (k_adj_side_changed) and reuses the
// factor, factorises the kept structure numerically again, or drops it and builds as ever.
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
  std::unique_ptr<LdlFactor> F;                 // null: the iterative state of section 17 -- no factor, multipliers at full length
  bool iterative = false;                       // (mr = m, act_rows and slot the identity: the kernels above serve both)
  bool h_side_current = true;                   // iterative: h_side is downloaded by the first host-form call that wants `act`
  int n_low = 0, n_upp = 0, mr = 0;
  std::vector<double> h_side;                   // [m] -1 lower, 0 inactive, 1 upper (the `act` output)
  DevBuf<int> act_rows, slot;                   // [mr] rows in the order of the reduced matrix; [m] row -> position, -1
  DevBuf<double> side, xc, yc;                  // [m], [n], [m]
  DevBuf<double> rhs_red, sol, rhs, yfull, Axv, px, ared_x, rx, ry;
  size_t bytes = 0;                             // device bytes held (factor, index arrays, scratch)
  // section 18 (osqp_amd_adjoint_retain): the model moved on and the state was kept for the next solution to be checked
  // against it; values_dirty: P or A changed meanwhile, the kept structure needs its numeric factorisation again
  bool stale = false, values_dirty = false;
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
  // the iterative form (osqp_amd_derivative_iter_stats): states built, outer steps, CG iterations of its own, the last pass
  long long it_builds = 0, it_outer = 0, it_cg = 0;
  int last_outer = 0;
  double last_drop = 0.0;
  const char *who = "";            // the exported symbol of the call in progress (kept_state)
  KktIter *session = nullptr;      // the indirect back-end is borrowed for the passes of the call in progress (IterSession)
  // osqp_amd_adjoint_retain (section 18): the mode, and what became of the stale states that were checked
  int retain = 0;
  long long rt_checks = 0, rt_reused = 0, rt_refactorised = 0, rt_rebuilt_set = 0, rt_rebuilt_failed = 0;
  int rt_last_changed = 0;
};
void model_adjoint_destroy(ModelAdjoint *a) { delete a; }

void model_adjoint_release(Engine &e) {
  if (e.adj && e.adj->kept) { e.sync(); e.adj->kept.reset(); }
}

// the model moved on (a solve, new data, a new iterate).  Default: the kept state goes.  Retain mode, and the state holds a
// factor: it stays, marked stale, and the first derivative call on the next solution decides what it is still good for
void model_adjoint_moved_on(Engine &e, bool values_changed) {
  ModelAdjoint *a = e.adj.get();
  if (!a || !a->kept) return;
  if (a->retain != 1 || !a->kept->F) { model_adjoint_release(e); return; }
  a->kept->stale = true;
  a->kept->values_dirty = a->kept->values_dirty || values_changed;
}

void model_adjoint_retain(Engine &e, int mode) {
  if (!e.adj) e.adj.reset(new ModelAdjoint());
  e.adj->retain = mode;
  if (mode == 0 && e.adj->kept && e.adj->kept->stale) model_adjoint_release(e);  // from here on the default's invariants hold
}

void model_adjoint_retain_stats(const Engine &e, double out[8]) {
  const ModelAdjoint *a = e.adj.get();
  const AdjointKept *k = a ? a->kept.get() : nullptr;
  out[0] = a ? (double)a->retain : 0.0;
  out[1] = a ? (double)a->rt_checks : 0.0;
  out[2] = a ? (double)a->rt_reused : 0.0;
  out[3] = a ? (double)a->rt_refactorised : 0.0;
  out[4] = a ? (double)a->rt_rebuilt_set : 0.0;
  out[5] = a ? (double)a->rt_rebuilt_failed : 0.0;
  out[6] = a ? (double)a->rt_last_changed : 0.0;
  out[7] = k && k->stale ? 1.0 : 0.0;
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

void model_adjoint_iter_stats(const Engine &e, double out[7]) {
  const ModelAdjoint *a = e.adj.get();
  const AdjointKept *k = a ? a->kept.get() : nullptr;
  out[0] = a ? (double)a->it_builds : 0.0;
  out[1] = a ? (double)a->it_outer : 0.0;
  out[2] = a ? (double)a->it_cg : 0.0;
  out[3] = a ? (double)a->last_outer : 0.0;
  out[4] = a ? a->last_drop : 0.0;
  out[5] = k && k->iterative ? 1.0 : 0.0;
  out[6] = k && k->iterative ? (double)k->bytes : 0.0;
}

namespace {

// classify the rows on the scaled (z, y, l, u) of the solution -- polish's rule, and a row with l == u is always active and
// counts as lower --, analyse and factorise the reduced matrix, set up what every later call on this solution reuses
// too_large (auto method): a factor that does not fit is reported there instead of refused, and nothing is built
void adjoint_build(Engine &e, ModelAdjoint &A, const char *who, const char *form, bool *too_large = nullptr) {
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
  if (frc == -1 && too_large) { *too_large = true; return; }
  if (frc == -1)
    throw Error(6, std::string(who) + ": the factor of the reduced KKT matrix of the active set is too large for the device (the iterative " + form +
                       " is opt-in: osqp_amd_derivative_method(work, 1, 0, 0) takes it where the factor does not fit)");
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
  if (K.iterative) {  // section 17: rhs_red = [b1; b2] and sol = [s_x; s_y] at full length n + m
    KktIterResult res;
    const int rc = kkt_iter_solve(A.session, K.rhs_red.get(), K.rhs_red.get() + e.n, K.sol.get(), K.sol.get() + e.n, e.deriv_max_outer,
                                  e.deriv_rel_drop, &res);
    A.solves += res.outer; A.it_outer += res.outer; A.it_cg += res.cg;
    A.last_outer = res.outer; A.last_drop = res.drop;
    if (rc) {
      char buf[64];
      snprintf(buf, sizeof buf, "%.3e", res.drop);
      throw Error(4, std::string(A.who) + ": the iterative KKT solve of the derivative did not converge: residual drop rn / first_norm = " + buf + " after " +
                         std::to_string(res.outer) + " outer steps (osqp_amd_derivative_method sets max_outer and rel_drop)");
    }
    return;
  }
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

bool workspace_compact(const Engine &e) {
  return e.compact || e.A.compact || e.At.compact || e.Pf.compact || (e.nnzPtriu > 0 && e.Pi_keep.n == 0);
}

// no CSR arrays and no reduced KKT matrix: what polish_run hands to its iterative form
void adjoint_needs_csr(const Engine &e, const char *who, const char *form) {
  if (e.comm)
    throw Error(6, std::string(who) + ": not available on a row-sharded workspace (a row block has no reduced KKT matrix; the iterative " + form +
                       " of osqp_amd_derivative_method runs on one device only)");
  if (workspace_compact(e))
    throw Error(6, std::string(who) + ": not available on a compact workspace (its CSR arrays are released, there is no reduced KKT matrix to factorise; "
                   "the iterative " + form + " is opt-in: osqp_amd_derivative_method(work, 1, 0, 0); OSQP_AMD_COMPACT_NNZ=-1 at setup keeps the arrays)");
}

// ---- the iterative kept state ----
// side by the rule of adjoint_build, on the device; low / upp: 1.0 where the row is lower / upper (summed for the counts)
__global__ __launch_bounds__(kBlock) void k_adj_classify(int m, const double *__restrict__ z, const double *__restrict__ y, const double *__restrict__ l,
                                                         const double *__restrict__ u, double *__restrict__ side, double *__restrict__ low_ind,
                                                         double *__restrict__ upp_ind, int *__restrict__ ident_a, int *__restrict__ ident_b) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= m) return;
  const bool low = (z[i] - l[i] < -y[i]) || l[i] == u[i];
  const bool upp = !low && (u[i] - z[i] < y[i]);
  side[i] = low ? -1.0 : (upp ? 1.0 : 0.0);
  low_ind[i] = low ? 1.0 : 0.0;
  upp_ind[i] = upp ? 1.0 : 0.0;
  ident_a[i] = i; ident_b[i] = i;
}

// no factor: the side array (classified and counted on the device: no m-vector comes to the host), the caller-unit solution,
// right-hand side and solution at full length n + m, act_rows and slot the identity
void adjoint_build_iter(Engine &e, ModelAdjoint &A) {
  hipStream_t s = e.stream;
  const int n = e.n, m = e.m;
  const size_t bytes0 = g_device_bytes, m1 = m ? m : 1;
  std::unique_ptr<AdjointKept> K(new AdjointKept());
  K->iterative = true;
  K->mr = m;
  K->act_rows.alloc(m1); K->slot.alloc(m1); K->side.alloc(m1);
  K->xc.alloc(n); K->yc.alloc(m1);
  K->rhs_red.alloc((size_t)n + m); K->sol.alloc((size_t)n + m); K->rx.alloc(n); K->ry.alloc(m1);
  if (m > 0) {
    // the indicator arrays live in scratch that the first pass overwrites (rhs_red is n + m long, ry m)
    double *low_ind = K->rhs_red.get() + n, *upp_ind = K->ry.get();
    OQ_LAUNCH(k_adj_classify, dim3(blocks_for(m)), dim3(kBlock), 0, s, m, e.z.get(), e.y.get(), e.l.get(), e.u.get(), K->side.get(), low_ind, upp_ind,
              K->act_rows.get(), K->slot.get());
    double h_keep[2] = {e.h_slots[S_T2], e.h_slots[S_T3]};
    reduce_sum(low_ind, m, e.partials.get(), e.slots.get() + S_T2, s);
    reduce_sum(upp_ind, m, e.partials.get(), e.slots.get() + S_T3, s);
    e.fetch_slots(S_T2, 2, 3u);
    K->n_low = (int)e.h_slots[S_T2]; K->n_upp = (int)e.h_slots[S_T3];
    e.h_slots[S_T2] = h_keep[0]; e.h_slots[S_T3] = h_keep[1];
  }
  K->h_side_current = m == 0;
  OQ_LAUNCH(k_adj_unscale, dim3(blocks_for((int64_t)n + m)), dim3(kBlock), 0, s, n, m, e.c, e.D.get(), e.E.get(), e.x.get(), e.y.get(),
            K->xc.get(), K->yc.get());
  e.sync();
  K->bytes = g_device_bytes > bytes0 ? g_device_bytes - bytes0 : 0;
  A.kept = std::move(K);
  A.builds++; A.it_builds++;
}

// the indirect back-end borrowed for the passes of one call and handed back at the end of the scope, whatever ends it
struct IterSession {
  ModelAdjoint &A;
  std::unique_ptr<KktIter, KktIterDeleter> it;
  IterSession(Engine &e, ModelAdjoint &A_) : A(A_) {
    if (!A.kept->iterative) return;
    it.reset(kkt_iter_begin(e, A.kept->side.get()));
    A.session = it.get();
  }
  ~IterSession() { A.session = nullptr; }
};

// ---- a kept factor that outlives its solution (osqp_amd_adjoint_retain) ----
// How many rows of the new solution lie on another side than the kept state was built for: the rule of adjoint_build to the
// letter (subtractions and comparisons only: the host and the device cannot disagree) against side[i].  A streaming pass over
// five m-vectors, consecutive lanes on consecutive doubles, grid-stride beyond kSideGrid workgroups; the count goes through
// the wavefront, then the four waves of the block, then ONE integer add per workgroup into a word the caller zeroed.
constexpr int kSideGrid = 2048;
__global__ __launch_bounds__(kBlock) void k_adj_side_changed(int m, const double *__restrict__ z, const double *__restrict__ y,
                                                             const double *__restrict__ l, const double *__restrict__ u,
                                                             const double *__restrict__ side, int *__restrict__ count) {
  int mine = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock) {
    const double zi = z[i], yi = y[i], li = l[i], ui = u[i];
    const bool low = (zi - li < -yi) || li == ui;
    const bool upp = !low && (ui - zi < yi);
    mine += (low ? -1.0 : (upp ? 1.0 : 0.0)) != side[i];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  __shared__ int sm[kBlock / 64];
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    if (total) atomicAdd(count, total);
  }
}

void launch_side_changed(Engine &e, const AdjointKept &K) {
  OQ_LAUNCH(k_adj_side_changed, dim3(std::min(blocks_for(e.m), kSideGrid)), dim3(kBlock), 0, e.stream, e.m, e.z.get(), e.y.get(), e.l.get(), e.u.get(),
            K.side.get(), e.flag.get());
}

// The stale kept state against the solution the workspace holds now; true: it serves (A.kept is current again), false: it
// is gone and the caller builds as ever.  The host reads one word (m > 0; m = 0 has nothing to classify).  An unchanged
// active set leaves the structure as it is -- act_rows, slot, side, h_side, the scratch, the factor's choice of solve -- and
// only the caller-unit solution is written again; where P or A changed meanwhile the kept structure is factorised
// numerically first (LdlFactor's constructor reads the pattern alone: every choice it takes holds for the new values, and
// the probe of a dense top block is part of refactor).
bool retained_state_serves(Engine &e, ModelAdjoint &A) {
  AdjointKept &K = *A.kept;
  hipStream_t s = e.stream;
  const int n = e.n, m = e.m;
  int changed = 0;
  A.rt_checks++;
  if (m > 0) {
    e.flag.zero(s);
    launch_side_changed(e, K);
    e.flag.download(&changed, 1, s);
    e.sync();
  }
  A.rt_last_changed = changed;
  if (changed > 0) { A.rt_rebuilt_set++; model_adjoint_release(e); return false; }
  if (K.values_dirty && K.F->refactor(nullptr) != 0) { A.rt_rebuilt_failed++; model_adjoint_release(e); return false; }
  OQ_LAUNCH(k_adj_unscale, dim3(blocks_for((int64_t)n + m)), dim3(kBlock), 0, s, n, m, e.c, e.D.get(), e.E.get(), e.x.get(), e.y.get(),
            K.xc.get(), K.yc.get());
  e.sync();
  if (K.values_dirty) A.rt_refactorised++; else A.rt_reused++;
  K.stale = K.values_dirty = false;
  return true;
}

// ---- the driver model_adjoint_run and model_jvp_run (direct_jvp.hpp) share ----
// the workspace's derivative state with what the current solution keeps present (built by the first call after a solve);
// who: the exported symbol that was called, form: what its refusals name.  The method of osqp_amd_derivative_method decides
// which state is built: 0 the factor (and today's refusals), 1 the factor where today's code builds one and the iterative
// state on a compact workspace or where the factor does not fit, 2 the iterative state always.
ModelAdjoint &kept_state(Engine &e, const char *who, const char *form) {
  if (!e.adj) e.adj.reset(new ModelAdjoint());
  ModelAdjoint &A = *e.adj;
  A.who = who;
  if (A.kept && !A.kept->stale) return A;
  if (A.kept && retained_state_serves(e, A)) return A;  // section 18 (only a state with a factor is ever stale)
  bool iterative = e.deriv_method == 2 || (e.deriv_method == 1 && !e.comm && workspace_compact(e));
  if (!iterative) {
    adjoint_needs_csr(e, who, form);
    bool too_large = false;
    adjoint_build(e, A, who, form, e.deriv_method == 1 ? &too_large : nullptr);
    iterative = too_large;
  }
  if (iterative) {
    kkt_iter_refuse(e, who);
    adjoint_build_iter(e, A);
  }
  return A;
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
  if (K.iterative) {  // no factor, no tree: the passes run inside a session on the borrowed indirect back-end
    IterSession session(e, A);
    passes();
    e.sync();
    return;
  }
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
void write_act(Engine &e, AdjointKept &K, double *act, bool dev) {
  if (!act) return;
  if (dev) { e.copy_dev(act, K.side.get(), (size_t)e.m); e.sync(); return; }
  if (!K.h_side_current) {  // the iterative state classified on the device: the one m-vector a host-form caller asks for
    K.h_side.resize((size_t)e.m);
    K.side.download(K.h_side.data(), (size_t)e.m, e.stream);
    e.sync();
    K.h_side_current = true;
  }
  std::copy(K.h_side.begin(), K.h_side.end(), act);
}

// the matrix gradients of a compact matrix (section 17): entry k of the caller's array gathers its slot of the sampled outer
// product g (panel_outer); a map entry of all ones is no slot (P_k2up on the diagonal), a slot beyond `padded` is not read
__global__ __launch_bounds__(kBlock) void k_adj_gather_A(int64_t nnz, const int64_t *__restrict__ to_sorted, const uint32_t *__restrict__ k2slot,
                                                         size_t padded, const double *__restrict__ g, double *__restrict__ dA) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= nnz) return;
  const uint32_t sl = k2slot[to_sorted ? to_sorted[k] : k];
  dA[k] = sl < padded ? g[sl] : 0.0;
}
__global__ __launch_bounds__(kBlock) void k_adj_gather_P(int64_t nnz, const uint32_t *__restrict__ k2lo, const uint32_t *__restrict__ k2up,
                                                         size_t padded, const double *__restrict__ g, double *__restrict__ dP) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= nnz) return;
  const uint32_t lo = k2lo[k], up = k2up[k];
  const bool has_lo = lo < padded, has_up = up < padded && up != lo;
  dP[k] = has_lo && has_up ? g[lo] + g[up] : (has_lo ? g[lo] : (has_up ? g[up] : 0.0));
}

// which statement of dPx / dAx this workspace can run; refusals before the first kernel
void matrix_gradient_paths(const Engine &e, const char *who, bool wantP, bool wantA, bool &slicedP, bool &slicedA) {
  slicedP = wantP && e.nnzPtriu > 0 && e.Pf.compact;
  slicedA = wantA && e.nnzA > 0 && e.A.compact;
  if (wantP && e.nnzPtriu > 0 && !slicedP && e.Pi_keep.n == 0)
    throw Error(6, std::string(who) + ": dPx is not available: the workspace released the pattern of P while its sliced copy keeps CSR arrays");
  if (wantA && e.nnzA > 0 && !slicedA && e.At.compact)
    throw Error(6, std::string(who) + ": dAx is not available: A' is compact while A keeps its CSR arrays");
}

}  // namespace

int model_adjoint_run(Engine &e, const char *who, bool dev, int ncot, const double *dx, const double *dy, double *dq, double *dl,
                      double *du, double *dPx, double *dAx, double *act) {
  ModelAdjoint &A = kept_state(e, who, "adjoint");
  AdjointKept &K = *A.kept;
  hipStream_t s = e.stream;
  const int n = e.n, m = e.m;
  bool slicedP = false, slicedA = false;
  matrix_gradient_paths(e, who, dPx != nullptr, dAx != nullptr, slicedP, slicedA);
  const bool csrP = dPx && e.nnzPtriu > 0 && !slicedP, csrA = dAx && e.nnzA > 0 && !slicedA;
  if ((dPx || dAx) && !A.patterns && !workspace_compact(e)) {
    A.Pcol.alloc(std::max<int64_t>(1, e.nnzPtriu)); A.Acol.alloc(std::max<int64_t>(1, e.nnzA));
    expand_colptr(n, e.Pp_keep.get(), e.nnzPtriu, A.Pcol.get(), s);
    expand_colptr(n, e.At.rowptr.get(), e.nnzA, A.Acol.get(), s);
    e.device_A_to_sorted();
    e.sync();
    A.patterns = true;
  }
  if (workspace_compact(e)) {  // some matrices compact, others not: the column arrays of those that still go the CSR way
    if (csrP && A.Pcol.n == 0) { A.Pcol.alloc((size_t)e.nnzPtriu); expand_colptr(n, e.Pp_keep.get(), e.nnzPtriu, A.Pcol.get(), s); }
    if (csrA && A.Acol.n == 0) { A.Acol.alloc((size_t)e.nnzA); expand_colptr(n, e.At.rowptr.get(), e.nnzA, A.Acol.get(), s); }
    e.sync();
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
        if (csrP)
          OQ_LAUNCH(k_adj_dP, dim3(blocks_for(e.nnzPtriu)), dim3(kBlock), 0, s, e.nnzPtriu, e.Pi_keep.get(), A.Pcol.get(), K.rx.get(), K.xc.get(),
                    oP + c * nzP);
        if (csrA)
          OQ_LAUNCH(k_adj_dA, dim3(blocks_for(e.nnzA)), dim3(kBlock), 0, s, e.nnzA, to_sorted,
                    e.At.col.get(), A.Acol.get(), K.rx.get(), K.ry.get(), K.xc.get(), K.yc.get(), oA + c * nzA);
        // compact matrices: the sampled outer product on the slices, then the gather through the slot maps; the scratch g
        // (panel.padded doubles) lives for one matrix of one cotangent
        if (slicedP) {
          DevBuf<double> g(e.Pf.panel.padded);
          panel_outer(e.Pf, K.rx.get(), K.xc.get(), false, g.get(), s);  // -(r_x,i x_j) at (i, j): the two halves add up in the gather
          OQ_LAUNCH(k_adj_gather_P, dim3(blocks_for(e.nnzPtriu)), dim3(kBlock), 0, s, e.nnzPtriu, (const uint32_t *)e.P_k2lo.get(),
                    (const uint32_t *)e.P_k2up.get(), e.Pf.panel.padded, (const double *)g.get(), oP + c * nzP);
          e.sync();
        }
        if (slicedA) {
          DevBuf<double> g(e.A.panel.padded);
          panel_outer(e.A, K.yc.get(), K.rx.get(), false, g.get(), s);  // -(y_i r_x,j)
          panel_outer(e.A, K.ry.get(), K.xc.get(), true, g.get(), s);   // - r_y,i x_j: the second pass (one staged vector at a time)
          OQ_LAUNCH(k_adj_gather_A, dim3(blocks_for(e.nnzA)), dim3(kBlock), 0, s, e.nnzA, to_sorted, (const uint32_t *)e.A_k2pos.get(), e.A.panel.padded,
                    (const double *)g.get(), oA + c * nzA);
          e.sync();
        }
      }
    });
    st.deliver();
  }
  write_act(e, K, act, dev);
  return 0;
}

// osqp_amd_time_kernel id 8: the check kernel of section 18 by itself on the kept state (stale or current), HIP events on the
// engine's stream; -1 without a kept factor or with m = 0.  It writes the engine's flag word only.
float model_adjoint_time_check(Engine &e, int reps) {
  const AdjointKept *K = e.adj ? e.adj->kept.get() : nullptr;
  if (!K || !K->F || e.m == 0) return -1.0f;
  hipStream_t s = e.stream;
  hipEvent_t a, b;
  HIP_CHECK(hipEventCreate(&a)); HIP_CHECK(hipEventCreate(&b));
  e.flag.zero(s);
  launch_side_changed(e, *K);  // warm
  HIP_CHECK(hipEventRecord(a, s));
  for (int i = 0; i < reps; i++) launch_side_changed(e, *K);
  HIP_CHECK(hipEventRecord(b, s));
  HIP_CHECK(hipEventSynchronize(b));
  float ms = 0;
  HIP_CHECK(hipEventElapsedTime(&ms, a, b));
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  e.flag.zero(s);
  e.sync();
  return ms / (float)reps;
}

}  // namespace oq
