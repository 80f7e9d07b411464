// batch.hip -- batched small-QP path (rows K11/K12 of SURVEY.md section 8a,
// BASELINE.json config 5: 4096 independent MPC QPs, n = 100, m = 200).  One translation unit:
//   batch_common.hpp  what everything below shares: the pattern as the kernels see it, LDS pointer types and small device
//                     helpers, the state record of resident mode, the argument block of a launch (BatchIO), and the ONE
//                     table of the instantiations of the four-wavefront kernel (OQ_QUAD_ENTRIES);
//   batch_quad.hpp    k_batch_quad (round 4) -- one QP per FOUR wavefronts, three QPs per compute unit, the inverse of the
//                     reduced KKT matrix in registers as four quadrants, formed there by Gauss-Jordan sweeps; nothing of a
//                     factorisation touches global memory.  Takes the patterns that fit the compile-time bounds of an entry
//                     of the table -- the MPC family of the benchmark among them;
//   batch_solve.hpp   k_batch_solve (rounds 1-3) -- one QP per 512-thread workgroup, two per compute unit, for every other
//                     pattern with n <= 128 (run-time shapes, dense P, long rows);
//   batch_large.hpp  k_batch_solve_large -- the same phases for 128 < n <= 256 with the inverse left in the instance's global
//                     scratch and read from there every iteration; only while osqp_amd_batch_large is on (opt-in: slower per
//                     iteration than the register kernels);
//   batch_sched.hpp   host side: the analysis of the shared pattern (HostPattern), its device copy and the schedule of the
//                     four-wavefront kernel for the first table entry it fits (DevicePattern);
//   batch_large_factor.hpp  the factor of the polish / adjoint / JVP kernels in the instance's global scratch, for handles with
//                     128 < n <= 256 and osqp_amd_batch_large_factor on: the LARGE instantiations of the three kernels below;
//   batch_polish.hpp  k_batch_polish -- solution polishing for the resident batch, a launch of its own after the ADMM launch
//                     when the handle's settings.polish is 1; the solve kernels know nothing of it;
//   batch_adjoint.hpp k_batch_adjoint -- adjoint derivatives of the solutions of the resident batch, a launch of its own on
//                     request (osqp_amd_batch_adjoint, _multi: ncot cotangents per launch); shares the factorisation and the
//                     solves of the polish kernel;
//   batch_jvp.hpp     k_batch_jvp -- forward sensitivities of the solutions of the resident batch along directions of the data, a
//                     launch of its own on request (osqp_amd_batch_jvp): one factorisation per instance, one solve per direction;
//   batch_cert.hpp    k_batch_cert -- the infeasibility certificates of the resident batch, a launch of its own after every
//                     ADMM launch of osqp_amd_batch_resolve: normalises the directions that launch left in the records (RES_CERT);
//   batch_gap.hpp     k_batch_gap -- primal objective, dual objective and duality gap of the resident batch, a launch of its own on
//                     request (osqp_amd_batch_duality); reads the records, the raw data and the pattern, writes three doubles;
//   batch_shared.hpp  the shared batch (osqp_amd_shared_batch_*): one model and many right-hand sides on ONE inverse --
//                     k_shared_factor (setup), k_batch_solve_shared (T instances per workgroup, the dense step on the fp64
//                     matrix cores) and their small kernels; a handle type of its own (SharedBatch below);
//   batch_shared_adjoint.hpp  k_shared_adjoint -- the adjoint of the shared batch from the model block and the tile records
//                     (osqp_amd_shared_batch_adjoint), and k_shared_reduce_rows, the summed matrix gradients in a fixed order;
//   batch_shared_jvp.hpp  k_shared_jvp -- the forward sensitivities of the shared batch on the same data path, with matrix
//                     tangents shared by the instances (osqp_amd_shared_batch_jvp);
//   this file         the small kernels (warm start, rho fill, bound check, the row scatter and gather of a selection, MPC generator), the
//                     launcher (launch_batch), the handle (BatchPlan) and the C ABI.  A resident call exists for every instance and
//                     for a selection (osqp_amd_batch_X, osqp_amd_batch_X_rows): ONE static body batch_X(handle, subset, rows, k, ...)
//                     each, the extern "C" entries forward.  What differs between the two forms is in `Served` (launch size,
//                     sel), put_rows / give_rows (copy vs. scatter / gather) and OutStage (host-pointer outputs through adj_out);
//                     launch_factor is the one launcher of the polish, adjoint and JVP kernels.
// Same algorithm as oracle/osqp_oracle.c with the KKT system in reduced form.
// Both kernels also run in RESIDENT mode (osqp_amd_batch_setup ... _resolve, "the state record" in batch_common.hpp):
// scaling, iterate and rho of every instance live in HBM between launches; a branch of the prologue and of the epilogue on
// a kernel argument, the ADMM loop is the same code.
// There is no communication between instances: the multi-GPU path shards the
// instance range over ranks and gathers the packed results once (batch.py).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "batch_adjoint.hpp"
#include "batch_jvp.hpp"
#include "batch_cert.hpp"
#include "batch_gap.hpp"
#include "batch_polish.hpp"
#include "batch_quad.hpp"
#include "batch_sched.hpp"
#include "batch_solve.hpp"
#include "batch_large.hpp"
#include "batch_shared.hpp"
#include "batch_shared_adjoint.hpp"
#include "batch_shared_jvp.hpp"
#include "rng.hpp"

namespace oq {
namespace {

int g_batch_polish_launches = 0;  // launches of k_batch_polish by this process (osqp_amd_batch_polish_launches)
int g_batch_jvp_launches = 0;      // launches of k_batch_jvp by this process (osqp_amd_batch_jvp_launches)
int g_batch_adjoint_launches = 0;  // launches of k_batch_adjoint by this process (osqp_amd_batch_adjoint_launches)
int g_batch_cert_launches = 0;  // launches of k_batch_cert by this process (osqp_amd_batch_cert_launches)
int g_batch_last_kernel = -2;  // what launch_batch launched last: -1 the 512-thread kernel, >= 0 the number of the entry of OQ_QUAD_ENTRIES,
                               // -2 k_batch_solve_large (also the value before any launch: the LDS bytes of the schedule are 0 then)
int g_batch_large = 0;         // osqp_amd_batch_large: 128 < n <= 256 is accepted and served by k_batch_solve_large
// the schedule of that launch (osqp_amd_batch_last_schedule): entry, p1_top, p1_bot, bw, ns, kew[0..3], LDS bytes, instances
constexpr int kSchedWords = 11;
int g_batch_last_schedule[kSchedWords] = {-2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
inline bool batch_quad_enabled() {  // OSQP_AMD_BATCH_QUAD=0: the MPC family on the 512-thread kernel (A/B runs, tests)
  const char *e = getenv("OSQP_AMD_BATCH_QUAD");
  return !e || atoi(e) != 0;
}

// the iterate of osqp_amd_batch_warm_start, caller's units in, the record's scaled units out: x <- x / D, y <- c y / E,
// z <- A x in scaled units = E (A_raw x_raw); a missing vector is zero (and z with x).  One workgroup per instance: the one
// at position p serves instance sel[p] (sel nullptr: p) with row p of x_all / y_all, as BatchIO::sel has it.
__global__ __launch_bounds__(256) void k_batch_warm(Pattern P, int count, const double *__restrict__ Ax_all, const double *__restrict__ x_all,
                                                    const double *__restrict__ y_all, double *__restrict__ rec_all, int rec_stride,
                                                    const int *__restrict__ sel) {
  const int pos = blockIdx.x, n = P.n, m = P.m;
  if (pos >= count) return;
  const int inst = sel ? sel[pos] : pos;
  double *rec = rec_all + (size_t)inst * rec_stride;
  const double c = rec[REC_C];
  for (int j = threadIdx.x; j < n; j += 256) rec[rec_x(n, m) + j] = x_all ? x_all[(size_t)pos * n + j] / rec[rec_D(n, m) + j] : 0.0;
  for (int i = threadIdx.x; i < m; i += 256) {
    const double e = rec[rec_E(n, m) + i];
    double ax = 0.0;
    if (x_all)
      for (int q = P.Rp[i]; q < P.Rp[i + 1]; q++) ax += Ax_all[(size_t)inst * P.nnzA + P.Rmap[q]] * x_all[(size_t)pos * n + P.Rc[q]];
    rec[rec_z(n, m) + i] = e * ax;
    rec[rec_y(n, m) + i] = y_all ? c * y_all[(size_t)pos * m + i] / e : 0.0;
  }
}

// one header slot of every record: the rho of osqp_amd_batch_update_setting("rho") into REC_RHO, as osqp_update_rho rebuilds
// rho_vec, or a zero into REC_GAPREF when the gap rule is switched (osqp_amd_batch_duality_gap_check); the iterate stays
__global__ __launch_bounds__(256) void k_batch_fill_hdr(int count, int slot, double value, double *__restrict__ rec_all, int rec_stride) {
  const int inst = blockIdx.x * 256 + threadIdx.x;
  if (inst < count) rec_all[(size_t)inst * rec_stride + slot] = value;
}
// out[p] = the refusal count in the record of instance sel[p] (sel == nullptr: p), or 0 while the rule is off
__global__ __launch_bounds__(256) void k_batch_gap_refusals(const int *__restrict__ sel, int k, int on, const double *__restrict__ rec_all,
                                                            int rec_stride, double *__restrict__ out) {
  const int pos = blockIdx.x * 256 + threadIdx.x;
  if (pos < k) out[pos] = on ? rec_all[(size_t)(sel ? sel[pos] : pos) * rec_stride + REC_GAPREF] : 0.0;
}

// rows with l > u, counted per launch (osqp_amd_batch_update_bounds refuses the update when there is one)
__global__ __launch_bounds__(256) void k_batch_check_bounds(size_t total, const double *__restrict__ l, const double *__restrict__ u, int *bad) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < total && l[i] > u[i]) atomicAdd(bad, 1);
}

// ---- a selection of instances (osqp_amd_batch_*_rows): sel[0 .. k) distinct instance numbers, checked on the host ----------
// row p of src [k x cols] into row sel[p] of dst [count x cols]: q, l, u, Px, Ax of an update, the info rows of a resolve.
// One workgroup per selected row.
__global__ __launch_bounds__(256) void k_batch_scatter_rows(const int *__restrict__ sel, int k, int cols, const double *__restrict__ src,
                                                            double *__restrict__ dst) {
  const int pos = blockIdx.x;
  if (pos >= k) return;
  const double *from = src + (size_t)pos * cols;
  double *to = dst + (size_t)sel[pos] * cols;
  for (int c = threadIdx.x; c < cols; c += 256) to[c] = from[c];
}
// the other way: row sel[p] of src [count x cols] into row p of dst [k x cols] -- the polish status and the certificates of a
// selection (osqp_amd_batch_polish_status_rows, _certificates_rows).  One workgroup per selected row.
__global__ __launch_bounds__(256) void k_batch_gather_rows(const int *__restrict__ sel, int k, int cols, const double *__restrict__ src,
                                                           double *__restrict__ dst) {
  const int pos = blockIdx.x;
  if (pos >= k) return;
  const double *from = src + (size_t)sel[pos] * cols;
  double *to = dst + (size_t)pos * cols;
  for (int c = threadIdx.x; c < cols; c += 256) to[c] = from[c];
}
// dst[sel[p]] = value (the polish status of instances re-solved without polish)
__global__ __launch_bounds__(256) void k_batch_fill_rows(const int *__restrict__ sel, int k, double value, double *__restrict__ dst) {
  const int pos = blockIdx.x * 256 + threadIdx.x;
  if (pos < k) dst[sel[pos]] = value;
}
// k_batch_check_bounds over the selected rows: a bound that is not given ([k x m], nullptr) is the stored one of the instance
__global__ __launch_bounds__(256) void k_batch_check_bounds_rows(const int *__restrict__ sel, int k, int m, const double *__restrict__ l_rows,
                                                                 const double *__restrict__ u_rows, const double *__restrict__ l_all,
                                                                 const double *__restrict__ u_all, int *bad) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)k * m) return;
  const size_t pos = i / m, at = (size_t)sel[pos] * m + (i - pos * m);
  const double l = l_rows ? l_rows[i] : l_all[at], u = u_rows ? u_rows[i] : u_all[at];
  if (l > u) atomicAdd(bad, 1);
}

// ---------------------------------------------------------------------------
// MPC instance generator (same statement as gen_mpc in oracle/gen.c); one
// thread fills one instance.  Also run on the host for instance 0 to obtain the
// shared sparsity pattern.
// ---------------------------------------------------------------------------
struct MpcValues { double *Ax, *Pd, *q, *l, *u; };  // of one instance: nnz(A), n, n, m, m doubles
__host__ __device__ inline void mpc_fill(long long inst, unsigned long long seed, int *Ap, int *Ai, MpcValues out) {
  double *const Ax = out.Ax, *const Pd = out.Pd, *const q = out.q, *const l = out.l, *const u = out.u;
  const int row_box = NX * TT, row_rate = NX * TT + MPC_N;
  double Ad[NX][NX], Bd[NX][NU], x0[NX], xref[NX];
  for (int r = 0; r < NX; r++) {
    for (int c = 0; c < NX; c++) {
      double base = (r == c ? 0.9 : 0.0) + ((r - c == 1 || c - r == 1) ? 0.05 : 0.0);
      Ad[r][c] = base + 0.02 * gauss(seed, G_MPC_A, (unsigned long long)(inst * 36 + r * 6 + c));
    }
    for (int c = 0; c < NU; c++)
      Bd[r][c] = ((r % 4) == c ? 0.5 : 0.0) + 0.1 * gauss(seed, G_MPC_B, (unsigned long long)(inst * 24 + r * 4 + c));
    x0[r] = gauss(seed, G_MPC_X0, (unsigned long long)(inst * 6 + r));
    xref[r] = 0.5 * gauss(seed, G_MPC_REF, (unsigned long long)(inst * 6 + r));
  }
  int pos = 0, j = 0;
  for (int t = 0; t < TT; t++) {
    for (int r = 0; r < NX; r++, j++) {
      Pd[j] = 1.0 + 0.1 * (double)r;
      q[j] = -(1.0 + 0.1 * (double)r) * xref[r];
      if (Ap) Ap[j] = pos;
      if (Ai) Ai[pos] = NX * t + r;
      Ax[pos++] = 1.0;
      if (t + 1 < TT) for (int c = 0; c < NX; c++) { if (Ai) Ai[pos] = NX * (t + 1) + c; Ax[pos++] = -Ad[c][r]; }
      if (Ai) Ai[pos] = row_box + j;
      Ax[pos++] = 1.0;
    }
    for (int c = 0; c < NU; c++, j++) {
      Pd[j] = 0.1;
      q[j] = 0.0;
      if (Ap) Ap[j] = pos;
      for (int r = 0; r < NX; r++) { if (Ai) Ai[pos] = NX * t + r; Ax[pos++] = -Bd[r][c]; }
      if (Ai) Ai[pos] = row_box + j;
      Ax[pos++] = 1.0;
      if (Ai) Ai[pos] = row_rate + NU * t + c;
      Ax[pos++] = 1.0;
      if (t + 1 < TT) { if (Ai) Ai[pos] = row_rate + NU * (t + 1) + c; Ax[pos++] = -1.0; }
    }
  }
  if (Ap) Ap[MPC_N] = pos;
  for (int r = 0; r < MPC_M; r++) { l[r] = 0.0; u[r] = 0.0; }
  for (int r = 0; r < NX; r++) {
    double sum = 0.0;
    for (int c = 0; c < NX; c++) sum += Ad[r][c] * x0[c];
    l[r] = sum; u[r] = sum;
  }
  for (int jj = 0; jj < MPC_N; jj++) {
    double b = (jj % NS) < NX ? 20.0 : 1.0;
    l[row_box + jj] = -b; u[row_box + jj] = b;
  }
  for (int r = 0; r < NU * TT; r++) { l[row_rate + r] = -0.5; u[row_rate + r] = 0.5; }
}
__global__ __launch_bounds__(64) void k_gen_mpc(long long first, int count, unsigned long long seed, int nnzA, double *Ax_all,
                                                double *Pd_all, double *q_all, double *l_all, double *u_all) {
  int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= count) return;
  mpc_fill(first + t, seed, nullptr, nullptr, MpcValues{Ax_all + (size_t)t * nnzA, Pd_all + (size_t)t * MPC_N, q_all + (size_t)t * MPC_N,
                                                        l_all + (size_t)t * MPC_M, u_all + (size_t)t * MPC_M});
}

// the pattern of the MPC family, from instance 0 on the host (mpc_fill writes the same Ap / Ai for every instance; P diagonal)
HostPattern mpc_host_pattern(unsigned long long seed) {
  std::vector<int> Ap(MPC_N + 1), Ai(kMpcNnzA), Pp(MPC_N + 1), Pi(MPC_N);
  std::vector<double> ax(kMpcNnzA), pd(MPC_N), q(MPC_N), l(MPC_M), u(MPC_M);
  mpc_fill(0, seed, Ap.data(), Ai.data(), MpcValues{ax.data(), pd.data(), q.data(), l.data(), u.data()});
  for (int j = 0; j <= MPC_N; j++) Pp[j] = j;
  for (int j = 0; j < MPC_N; j++) Pi[j] = j;
  return HostPattern(MPC_N, MPC_M, Pp, Pi, std::move(Ap), std::move(Ai));
}
// the caller's batch as osqp_amd_batch_solve and osqp_amd_batch_setup receive it (the arguments in their order)
struct BatchProblem {
  c_int count, n, m;
  const c_int *Pp, *Pi;
  const c_float *Px_all;
  const c_int *Ap, *Ai;
  const c_float *Ax_all, *q_all, *l_all, *u_all;
  const OSQPSettings *settings;
};
// its CSC patterns (validate_batch_data has seen them)
HostPattern host_pattern(const BatchProblem &p) {
  const c_int n = p.n;
  return HostPattern((int)n, (int)p.m, std::vector<int>(p.Pp, p.Pp + n + 1), std::vector<int>(p.Pi, p.Pi + p.Pp[n]),
                     std::vector<int>(p.Ap, p.Ap + n + 1), std::vector<int>(p.Ai, p.Ai + p.Ap[n]));
}

template <typename K>
void launch_kernel_solve(K kern, size_t bytes, const DevicePattern &dp, const OSQPSettings &st, int count, const BatchIO &io, hipStream_t s) {
  HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  OQ_LAUNCH(kern, dim3(count), dim3(NT), bytes, s, dp.P, st, count, dp.scratch.get(), io.Px, io.Ax, io.q, io.l, io.u, io.x, io.y, io.info,
            io.x_stride, io.y_stride, io.info_stride, io.info_cols, io.rec, io.rec_stride, io.res_mode, io.sel);
}
template <typename K>
void launch_kernel_quad(K kern, const DevicePattern &dp, const OSQPSettings &st, int count, const BatchIO &io, hipStream_t s) {
  const Pattern &P = dp.P;
  const quad::Layout L = quad::make_layout(P.n, P.m, P.nnzA, P.nnzF, dp.quad->NH, dp.quad->KC, dp.quad->KE, dp.quad->CH);
  HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, L.total));
  OQ_LAUNCH(kern, dim3(count), dim3(quad::QT), (size_t)L.total, s, dp.QS, st, count, io.Px, io.Ax, io.q, io.l, io.u, io.x, io.y, io.info,
            io.x_stride, io.y_stride, io.info_stride, io.info_cols, io.rec, io.rec_stride, io.res_mode, io.sel);
}

// What k_batch_solve_large needs for a shape (osqp_amd_batch_large_plan and the launcher both ask here); a shape it does not
// take is an Error with the reason.
struct LargePlan { size_t lds_bytes, scratch_bytes; int tiles_per_wave; };
LargePlan large_plan(long long n, long long m, long long nnzA, long long nnzF) {
  if (n > kLargeMaxN || m > 65535 || nnzA > 65535 || nnzF > 65535)
    throw Error(1, "the batched path supports n <= 256 (osqp_amd_batch_large on) and fewer than 65536 rows / non-zeros");
  if (n <= kPivotW || m < 0 || nnzA < 0 || nnzF < 0)
    throw Error(1, "k_batch_solve_large serves 128 < n <= 256; a pattern with n <= 128 runs the register kernels (n = " + std::to_string(n) + ")");
  const size_t bytes = large_lds_bytes((int)n, (int)m, (int)nnzA, (int)nnzF);
  if (bytes > 160 * 1024) throw Error(1, "instance too large for the LDS-resident batched path (needs " + std::to_string(bytes) + " bytes of LDS)");
  return LargePlan{bytes, (size_t)n * (size_t)n * sizeof(double), large_tiles_per_wave((int)n)};
}
void launch_batch_large(const DevicePattern &dp, const OSQPSettings &st, int count, const BatchIO &io, hipStream_t s) {
  const Pattern &P = dp.P;
  const LargePlan lp = large_plan(P.n, P.m, P.nnzA, P.nnzF);
  const size_t need = (size_t)count * P.n * P.n;  // M, then M^-1, of every position of the launch: read every iteration
  if (dp.scratch.n < need) { HIP_CHECK(hipStreamSynchronize(s)); dp.scratch.alloc(need); }
  g_batch_last_kernel = -2;
  const int sched[kSchedWords] = {-2, 0, 0, 0, 0, 0, 0, 0, 0, (int)lp.lds_bytes, count};
  std::copy(sched, sched + kSchedWords, g_batch_last_schedule);
  if (io.sel) launch_kernel_solve(k_batch_solve_large<true>, lp.lds_bytes, dp, st, count, io, s);
  else launch_kernel_solve(k_batch_solve_large<false>, lp.lds_bytes, dp, st, count, io, s);
}

void launch_batch(const DevicePattern &dp, const OSQPSettings &st, int count, const BatchIO &io, hipStream_t s) {
  const Pattern &P = dp.P;
  if (dp.large) { launch_batch_large(dp, st, count, io, s); return; }  // built while osqp_amd_batch_large was on, n > 128
  const size_t bytes = lds_bytes(P.n, P.m, P.nnzA, P.nnzF, sparse_fits(P));
  if (P.n > 128 || P.m > 65535 || P.nnzA > 65535 || P.nnzF > 65535) throw Error(1, "the batched path supports n <= 128 and fewer than 65536 rows / non-zeros");
  if (bytes > 160 * 1024) throw Error(1, "instance too large for the LDS-resident batched path (needs " + std::to_string(bytes) + " bytes of LDS)");
  if (dp.quad && batch_quad_enabled()) {
    // one QP per four wavefronts, the factorisation on chip, no global scratch: the instantiation the pattern's schedule
    // was built for.  FIXED entries get the shape of the MPC family as template arguments (DevicePattern::build tries
    // them for that family only).
    g_batch_last_kernel = dp.quad->number;
    {
      const quad::Sched &q = dp.QS;
      const int sched[kSchedWords] = {dp.quad->number, q.p1_top, q.p1_bot, q.bw, q.ns, q.kew[0], q.kew[1], q.kew[2], q.kew[3],
                                      quad::make_layout(P.n, P.m, P.nnzA, P.nnzF, dp.quad->NH, dp.quad->KC, dp.quad->KE, dp.quad->CH).total, count};
      std::copy(sched, sched + kSchedWords, g_batch_last_schedule);
    }
    switch (dp.quad->number) {
#define OQ_QUAD_CASE(NUMBER, NH, KC, KE, CH, FIXED, KERNEL)                                                                    \
  case NUMBER: {                                                                                                               \
    constexpr int CN = FIXED ? MPC_N : 0, CM = FIXED ? MPC_M : 0, CA = FIXED ? kMpcNnzA : 0, CF = FIXED ? MPC_N : 0;           \
    static_assert(quad_entry(NUMBER)->fixed == (CN > 0), "shape compiled in <=> CN > 0: the kernel's BWC and the host's guard"); \
    if (io.sel) launch_kernel_quad(quad::KERNEL<NH, KC, KE, CH, CN, CM, CA, CF, true>, dp, st, count, io, s);                 \
    else launch_kernel_quad(quad::KERNEL<NH, KC, KE, CH, CN, CM, CA, CF, false>, dp, st, count, io, s);                       \
  } break;
      OQ_QUAD_ENTRIES(OQ_QUAD_CASE)
#undef OQ_QUAD_CASE
    default: throw Error(6, "no instantiation of the four-wavefront kernel has number " + std::to_string(dp.quad->number));
    }
    return;
  }
  const size_t need = (size_t)count * P.n * P.n;  // where a workgroup assembles and inverts its reduced KKT matrix
  if (dp.scratch.n < need) { HIP_CHECK(hipStreamSynchronize(s)); dp.scratch.alloc(need); }
  const int nc = (P.n + PARTS - 1) / PARTS;  // columns of the inverse per thread: the register tile is sized at compile time
  g_batch_last_kernel = -1;
  {
    const int sched[kSchedWords] = {-1, 0, 0, 0, 0, 0, 0, 0, 0, (int)bytes, count};  // no schedule: the LDS bytes are this kernel's
    std::copy(sched, sched + kSchedWords, g_batch_last_schedule);
  }
  // shapes compiled in (same source, constants folded): the MPC family of BASELINE.json config 5
  // (the last argument: a launch over a selection, io.sel, has instantiations of its own)
#define OQ_SOLVE_LAUNCH(...)                                                                              \
  do {                                                                                                    \
    if (io.sel) launch_kernel_solve(k_batch_solve<__VA_ARGS__, true>, bytes, dp, st, count, io, s);       \
    else launch_kernel_solve(k_batch_solve<__VA_ARGS__, false>, bytes, dp, st, count, io, s);             \
  } while (0)
  if (dp.mpc) OQ_SOLVE_LAUNCH(25, MPC_N, MPC_M, kMpcNnzA, MPC_N);
  else if (nc <= 16) OQ_SOLVE_LAUNCH(16, 0, 0, 0, 0);
  else if (nc <= 25) OQ_SOLVE_LAUNCH(25, 0, 0, 0, 0);
  else OQ_SOLVE_LAUNCH(32, 0, 0, 0, 0);
#undef OQ_SOLVE_LAUNCH
}

// the five data arrays of `count` instances of pattern P on the device: allocated and filled in one step
struct BatchData {
  DevBuf<double> Px, Ax, q, l, u;
  void alloc(size_t count, const Pattern &P) {
    Px.alloc(count * P.nnzP); Ax.alloc(count * P.nnzA); q.alloc(count * P.n); l.alloc(count * P.m); u.alloc(count * P.m);
  }
  void upload(const BatchProblem &p, const Pattern &P, hipStream_t s) {
    alloc((size_t)p.count, P);
    Px.upload(p.Px_all, Px.n, s); Ax.upload(p.Ax_all, Ax.n, s); q.upload(p.q_all, q.n, s); l.upload(p.l_all, l.n, s); u.upload(p.u_all, u.n, s);
  }
  void generate_mpc(long long first, int count, unsigned long long seed, const Pattern &P, hipStream_t s) {
    alloc((size_t)count, P);
    OQ_LAUNCH(k_gen_mpc, dim3(blocks_for(count, 64)), dim3(64), 0, s, first, count, seed, kMpcNnzA, Ax.get(), Px.get(), q.get(), l.get(), u.get());
  }
  BatchIO inputs() const {  // a launch on these data; the caller names the outputs (and the records)
    BatchIO io;
    io.Px = Px.get(); io.Ax = Ax.get(); io.q = q.get(); io.l = l.get(); io.u = u.get();
    return io;
  }
};

// A batch of MPC instances resident in HBM, cut into contiguous equal blocks over the ranks of a communicator
// (instance i -> rank floor(i / (total / world))).  solve() = this rank's block, one workgroup per
// instance, results written straight into their rows of the packed [total x (n + m + 4)] array, then the one
// collective of the path: an in-place all-gather of the rank blocks (rows K11 + K12 in one library call).
struct BatchPlan : BatchData {
  int device = 0, total = 0, first = 0, count = 0;
  Comm *comm = nullptr;  // not owned; nullptr = one rank
  OSQPSettings st;
  DevicePattern dp;
  static constexpr int kRow = MPC_N + MPC_M + 4;
  // osqp_amd_batch_setup: the caller's own QPs (raw values in Px .. u above), their state records, staging for host-pointer
  // calls (updates and warm starts come in through in_a / in_b, results leave through x_out / y_out / info_out)
  bool resident = false;
  int n = 0, m = 0, nnzA = 0, nnzP = 0, rec_stride = 0;
  DevBuf<double> rec, in_a, in_b, x_out, y_out, info_out;
  DevBuf<int> bad;
  // polish (settings.polish = 1): status_polish of every instance from the last resolve (1, -1, 0); pstat_live = 0: the
  // last resolve did not polish (or there was none) and all are 0, whatever the buffer holds
  DevBuf<double> pstat;
  bool pstat_live = false;
  // adjoint (osqp_amd_batch_adjoint): current[i] = the record and the info row of instance i hold the solution of its current
  // data (set by a resolve that served it, cleared by every update_* and warm_start that touched it; host bookkeeping).
  // info_all [count x 6]: the info row of every instance's own last resolve, wherever the caller's went -- not the staging of
  // a host-pointer resolve of a selection, which is compact (info_out).  Staging of host-pointer calls: gradients in through
  // in_a / in_b, out through adj_out
  std::vector<char> current;
  DevBuf<double> info_all, adj_out;
  // forward sensitivities (osqp_amd_batch_jvp): the staging of host-pointer calls -- the five tangents come in through in_a,
  // in_b and these three, the wanted outputs leave through adj_out
  DevBuf<double> in_c, in_d, in_e;
  void mark(bool is_current) { std::fill(current.begin(), current.end(), (char)is_current); }
  void mark_rows(bool is_current) { for (int i : sel_host) current[(size_t)i] = (char)is_current; }
  // the selection of the running *_rows call, uploaded once per call (BatchIO::sel)
  std::vector<int> sel_host;
  DevBuf<int> sel;
  // certificates (osqp_amd_batch_certificates): [count x m] and [count x n], NaN from setup, then written by k_batch_cert
  // after every resolve
  DevBuf<double> pcert, dcert;
  bool rec_raw = false;  // a solve launched with RES_CERT whose k_batch_cert has not been launched (osqp_amd_batch_resolve)
  // osqp_amd_batch_duality_gap_check: every resolve carries RES_GAP, and slot REC_GAPREF of a record is the refusal count of
  // the instance's own last resolve since the rule was switched on (the switch zeroes the slot of every record)
  bool gap_rule = false;
  // osqp_amd_batch_large_factor (handles with n > 128 only): polish, adjoint and JVP run their LARGE instantiations, the factor
  // in dp.scratch; off: they are refused as a large handle always refused them
  bool large_factor = false;
};

// The checks osqp_setup makes [REF src/interface.jl:47-100 + the C side's validate_data / validate_settings], shared by the
// one-shot osqp_amd_batch_solve and osqp_amd_batch_setup.  outputs_ok: what the caller checked of its own output
// pointers; max_n: the size cap of the caller's path (kPivotW, or 256 for the opt-in large path and the shared batch).
// 0 = fine; otherwise the return code, the message is set.
c_int validate_batch_data(const BatchProblem &p, bool outputs_ok, c_int max_n) {
  const c_int count = p.count, n = p.n, m = p.m, *Pp = p.Pp, *Pi = p.Pi, *Ap = p.Ap, *Ai = p.Ai;
  const c_float *Px_all = p.Px_all, *Ax_all = p.Ax_all, *q_all = p.q_all, *l_all = p.l_all, *u_all = p.u_all;
  const OSQPSettings *settings = p.settings;
  if (count <= 0 || n <= 0 || m < 0 || !Pp || !Pi || !Ap || !Ai || !q_all || (m > 0 && (!l_all || !u_all)) || !settings || !outputs_ok) {
    set_last_error("invalid batch data"); return 1;
  }
  if (validate_settings(settings)) { set_last_error("invalid settings"); return 2; }
  if (n > max_n || m > 65535 || Pp[0] != 0 || Ap[0] != 0 || Pp[n] < 0 || Ap[n] < 0 || Pp[n] > 65535 || Ap[n] > 65535) {
    set_last_error(max_n > kPivotW ? "the batched path supports n <= 256 (osqp_amd_batch_large on) and fewer than 65536 rows / non-zeros"
                                 : "the batched path supports n <= 128 and fewer than 65536 rows / non-zeros");
    return 1;
  }
  for (c_int j = 0; j < n; j++) {
    if (Pp[j + 1] < Pp[j] || Ap[j + 1] < Ap[j]) { set_last_error("column pointers must not decrease"); return 1; }
    for (c_int k = Pp[j]; k < Pp[j + 1]; k++) if (Pi[k] < 0 || Pi[k] > j) { set_last_error("P must be upper triangular with row indices in range"); return 1; }
    for (c_int k = Ap[j]; k < Ap[j + 1]; k++) if (Ai[k] < 0 || Ai[k] >= m) { set_last_error("row index of A out of range"); return 1; }
    // the term lists of A' rho A are built by merging sorted columns (DevicePattern::build): unsorted or repeated rows
    // would silently drop terms
    for (c_int k = Ap[j] + 1; k < Ap[j + 1]; k++) if (Ai[k] <= Ai[k - 1]) { set_last_error("the rows of every column of A must be sorted and unique"); return 1; }
    for (c_int k = Pp[j] + 1; k < Pp[j + 1]; k++) if (Pi[k] <= Pi[k - 1]) { set_last_error("the rows of every column of P must be sorted and unique"); return 1; }
  }
  if ((Pp[n] > 0 && !Px_all) || (Ap[n] > 0 && !Ax_all)) { set_last_error("invalid batch data"); return 1; }
  for (c_int i = 0; i < count * m; i++) if (l_all[i] > u_all[i]) { set_last_error("lower bound greater than upper bound"); return 1; }
  return 0;
}

// the handle of a resident call, or nullptr with the message set
BatchPlan *resident_plan(osqp_amd_batch *handle) {
  if (!handle) { set_last_error("null batch handle"); return nullptr; }
  BatchPlan *b = (BatchPlan *)handle;
  if (!b->resident) { set_last_error("this batch handle was not created by osqp_amd_batch_setup"); return nullptr; }
  return b;
}
// `src` ([len] doubles, host or device pointer by `where`) as a device pointer: host data goes through `stage`
const double *device_ptr(const c_float *src, size_t len, c_int where, DevBuf<double> &stage, hipStream_t s) {
  if (where) return src;
  if (stage.n < len) stage.alloc(len);
  stage.upload(src, len, s);
  return stage.get();
}
void copy_d2d(double *dst, const double *src, size_t len, hipStream_t s) {
  HIP_CHECK(hipMemcpyAsync(dst, src, len * sizeof(double), hipMemcpyDeviceToDevice, s));
}
// D, E, c of the handle's current raw data into the records (one launch of the solve kernel in its scale-only mode)
// (`count` workgroups, instance by `sel`: nullptr = all of them)
void resident_equilibrate(BatchPlan &b, int count, const int *sel, hipStream_t s) {
  BatchIO io = b.inputs();
  io.rec = b.rec.get(); io.rec_stride = b.rec_stride; io.res_mode = RES_SCALE_ONLY; io.sel = sel;
  launch_batch(b.dp, b.st, count, io, s);
}
// The selection of a *_rows call, checked on the host before anything of the handle changes and uploaded into the handle's
// buffer: false with the message set when it is bad.
bool select_rows(BatchPlan &b, const c_int *rows, c_int k, hipStream_t s) {
  if (!rows) { set_last_error("invalid selection: rows is NULL"); return false; }
  if (k < 1 || k > b.count) {
    set_last_error("invalid selection: " + std::to_string(k) + " rows of a batch of " + std::to_string(b.count) + " instances (1 <= k <= count)");
    return false;
  }
  std::vector<char> seen((size_t)b.count, 0);
  for (c_int j = 0; j < k; j++) {
    const c_int i = rows[j];
    if (i < 0 || i >= b.count) {
      set_last_error("invalid selection: rows[" + std::to_string(j) + "] = " + std::to_string(i) + " is out of range [0, " + std::to_string(b.count) + ")");
      return false;
    }
    if (seen[(size_t)i]) { set_last_error("invalid selection: instance " + std::to_string(i) + " is repeated"); return false; }
    seen[(size_t)i] = 1;
  }
  b.sel_host.assign(rows, rows + k);
  if (b.sel.n < (size_t)b.count) b.sel.alloc((size_t)b.count);
  b.sel.upload(b.sel_host.data(), (size_t)k, s);
  return true;
}
void scatter_rows(const BatchPlan &b, int k, int cols, const double *src, double *dst, hipStream_t s) {
  if (cols) OQ_LAUNCH(k_batch_scatter_rows, dim3(k), dim3(256), 0, s, b.sel.get(), k, cols, src, dst);
}
void gather_rows(const BatchPlan &b, int k, int cols, const double *src, double *dst, hipStream_t s) {
  if (cols) OQ_LAUNCH(k_batch_gather_rows, dim3(k), dim3(256), 0, s, b.sel.get(), k, cols, src, dst);
}
// Whom a resident call serves: every instance (osqp_amd_batch_X) or the selection of the _rows form of the same call.
// launch: the workgroups of its launches and the rows of its arrays (count, or k: the arrays are then compact, row j for
// instance rows[j]); sel: what BatchIO::sel and the small kernels take (nullptr, or the handle's uploaded selection).
struct Served { bool subset; int launch; const int *sel; };
// that of the running call; a selection is checked and uploaded here (select_rows): false with the message set when it is bad
bool serve(BatchPlan &b, bool subset, const c_int *rows, c_int k, hipStream_t s, Served &v) {
  if (subset && !select_rows(b, rows, k, s)) return false;
  v = subset ? Served{true, (int)k, b.sel.get()} : Served{false, b.count, nullptr};
  return true;
}
void mark(BatchPlan &b, const Served &v, bool is_current) { if (v.subset) b.mark_rows(is_current); else b.mark(is_current); }
// The rows of the call (src [v.launch x cols], host or device pointer by `where`) into the handle's array dst [count x cols].
// Every instance: straight into dst, one upload or one d2d copy; a selection: through `stage` when they are host data, then
// scattered.
void put_rows(const BatchPlan &b, const Served &v, int cols, const c_float *src, c_int where, DevBuf<double> &stage, DevBuf<double> &dst, hipStream_t s) {
  const size_t len = (size_t)v.launch * cols;
  if (!len) return;
  if (v.subset) scatter_rows(b, v.launch, cols, device_ptr(src, len, where, stage, s), dst.get(), s);
  else if (where) copy_d2d(dst.get(), src, len, s);
  else dst.upload(src, len, s);
}
// The other way: the rows of the handle's array src [count x cols] out into dst [v.launch x cols].  Every instance: one
// download or one d2d copy by `where`; a selection: gathered on the device, so dst is device memory -- the caller's array or
// its slot of an OutStage.
void give_rows(const BatchPlan &b, const Served &v, int cols, const DevBuf<double> &src, c_float *dst, c_int where, hipStream_t s) {
  const size_t len = (size_t)v.launch * cols;
  if (v.subset) gather_rows(b, v.launch, cols, src.get(), dst, s);
  else if (where) copy_d2d(dst, src.get(), len, s);
  else src.download(dst, len, s);
}
// The outputs of a call as the device pointers its kernels write (nullptr: not wanted).  Not staged: the caller's own
// pointers.  Staged (host pointers): the wanted ones share the handle's adj_out at running offsets, in the order given, and
// download() issues their copies once the launches are on the stream.
struct OutStage {
  c_float *host[9];
  size_t len[9];
  double *dev[9];
  int count = 0;
  bool staged;
  template <typename Handle>  // BatchPlan or SharedBatch: whoever owns an adj_out
  OutStage(Handle &b, bool staged_, std::initializer_list<c_float *> outs, std::initializer_list<size_t> lens) : staged(staged_) {
    size_t total = 0, at = 0;
    for (c_float *h : outs) { host[count] = h; len[count] = lens.begin()[count]; if (h) total += len[count]; count++; }
    if (staged && b.adj_out.n < total) b.adj_out.alloc(total);
    for (int j = 0; j < count; j++) {
      dev[j] = staged && host[j] ? b.adj_out.get() + at : host[j];
      if (staged && host[j]) at += len[j];
    }
  }
  void download(int j, hipStream_t s) const {
    if (staged && host[j]) HIP_CHECK(hipMemcpyAsync(host[j], dev[j], len[j] * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  void download(hipStream_t s) const { for (int j = 0; j < count; j++) download(j, s); }
};
// The rule of the derivative calls: every instance they serve holds the solution of its current data.  rows nullptr: all of
// the batch (osqp_amd_batch_adjoint, _jvp); otherwise the selection (the *_rows forms), in its order.  false with the message
// set, naming the first instance that does not.
bool holds_current(const BatchPlan &b, const std::vector<int> *rows) {
  const size_t len = rows ? rows->size() : b.current.size();
  for (size_t j = 0; j < len; j++) {
    const size_t i = rows ? (size_t)(*rows)[j] : j;
    if (!b.current[i]) {
      set_last_error("instance " + std::to_string(i) + " of the batch holds no current solution: call osqp_amd_batch_resolve (or _resolve_rows "
                     "with this instance) after its last update or warm start");
      return false;
    }
  }
  return true;
}
// What the LARGE instantiations of k_batch_polish / _adjoint / _jvp need for a shape (osqp_amd_batch_large_factor_plan and
// polish_check_fits, which every launcher of the three asks, both ask here); a shape they do not take is an Error.
struct LargeFactorPlan { size_t lds_bytes, scratch_bytes; int nb; };
LargeFactorPlan large_factor_plan(long long n, long long m, long long nnzA, long long nnzF) {
  if (n <= kPivotW || n > polish::lf::kMaxN || m < 0 || m > 65535 || nnzA < 0 || nnzA > 65535 || nnzF < 0 || nnzF > 65535)
    throw Error(1, "the factor in global scratch serves 128 < n <= 256 and fewer than 65536 rows / non-zeros (n = " + std::to_string(n) + ")");
  const polish::Layout L = polish::make_layout((int)n, (int)m, (int)nnzA, (int)nnzF, true);
  if (L.total > polish::kLdsLimit)
    throw Error(1, "instance too large to polish on the LDS-resident batched path (needs " + std::to_string(L.total) + " bytes of LDS, " +
                       std::to_string(polish::kLdsLimit) + " available, with the factor in global scratch); set polish = 0");
  return LargeFactorPlan{(size_t)L.total, (size_t)n * (size_t)n * sizeof(double), polish::lf::NB};
}
// the LDS a polish launch of this pattern needs; a pattern it cannot serve is refused where polish is asked for (setup,
// osqp_amd_batch_update_polish), never skipped.  large_factor: the handle's switch (a handle with n <= 128 ignores it)
void polish_check_fits(const Pattern &P, bool large_factor = false) {
  if (large_factor && P.n > kPivotW) { large_factor_plan(P.n, P.m, P.nnzA, P.nnzF); return; }
  const polish::Layout L = polish::make_layout(P.n, P.m, P.nnzA, P.nnzF);
  if (L.total > polish::kLdsLimit)
    throw Error(1, "instance too large to polish on the LDS-resident batched path (needs " + std::to_string(L.total) + " bytes of LDS, " +
                       std::to_string(polish::kLdsLimit) + " available); set polish = 0");
  // a handle of the opt-in path for n > 128 whose M would still fit the LDS (n < ~190): the substitutions of the polish,
  // adjoint and JVP kernels hold the vector as two entries per lane of one wavefront (factor_solve, batch_polish.hpp)
  if (P.n > kPivotW)
    throw Error(1, "instance too large to polish on the LDS-resident batched path (n = " + std::to_string(P.n) +
                       ": the polish, adjoint and JVP kernels hold at most 128 variables); set polish = 0");
}
// the n x n block per launch position of the LARGE instantiations: the scratch of the handle's solve launches, grown as
// launch_batch_large grows it
double *large_factor_scratch(const DevicePattern &dp, int launch, hipStream_t s) {
  const size_t need = (size_t)launch * dp.P.n * dp.P.n;
  if (dp.scratch.n < need) { HIP_CHECK(hipStreamSynchronize(s)); dp.scratch.alloc(need); }
  return dp.scratch.get();
}
// One launch of k_batch_polish, k_batch_adjoint or k_batch_jvp (`lds` / `global`: its instantiation with the factor in LDS and
// its LARGE one; `a`: its argument block, filled by the caller but for the scratch), `launch` workgroups.  A pattern the
// kernels cannot serve is refused here; `launches` is the counter of the kernel.
template <typename A>
void launch_factor(BatchPlan &b, void (*lds)(Pattern, int, polish::Layout, A), void (*global)(Pattern, int, polish::Layout, A), A &a, int launch,
                   int &launches, hipStream_t s) {
  const Pattern &P = b.dp.P;
  const bool large = b.large_factor && b.dp.large;
  polish_check_fits(P, large);
  const polish::Layout L = polish::make_layout(P.n, P.m, P.nnzA, P.nnzF, large);
  if (large) a.scratch = large_factor_scratch(b.dp, launch, s);
  auto *const kern = large ? global : lds;
  HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, L.total));
  launches++;
  OQ_LAUNCH(kern, dim3(launch), dim3(polish::PT), (size_t)L.total, s, P, launch, L, a);
}
// polish() of the oracle on every Solved instance of the launch that has just written io.x / io.y / io.info and the records
// (`count` workgroups, instance by io.sel)
void launch_polish(BatchPlan &b, const BatchIO &io, int count, hipStream_t s) {
  polish::Args a;
  a.Px = io.Px; a.Ax = io.Ax; a.q = io.q; a.l = io.l; a.u = io.u;
  a.x = io.x; a.y = io.y; a.info = io.info; a.rec = io.rec; a.status = b.pstat.get();
  a.x_stride = io.x_stride; a.y_stride = io.y_stride; a.info_stride = io.info_stride; a.rec_stride = io.rec_stride;
  a.refine = (int)b.st.polish_refine_iter; a.unscaled = b.st.scaling && !b.st.scaled_termination;
  a.delta = b.st.delta; a.sel = io.sel;
  launch_factor(b, polish::k_batch_polish<false>, polish::k_batch_polish<true>, a, count, g_batch_polish_launches, s);
}
// the certificates of the launch that has just written io.info and, under RES_CERT, left the directions in the records
void launch_cert(BatchPlan &b, const BatchIO &io, int count, hipStream_t s) {
  cert::Args a;
  a.info = io.info; a.rec = io.rec; a.prim = b.m ? b.pcert.get() : nullptr; a.dual = b.dcert.get();
  a.info_stride = io.info_stride; a.rec_stride = io.rec_stride; a.unscaled = b.st.scaling && !b.st.scaled_termination;
  a.sel = io.sel;
  g_batch_cert_launches++;
  OQ_LAUNCH(cert::k_batch_cert, dim3(count), dim3(cert::CT), 0, s, b.n, b.m, count, a);
}
// polish / polish_refine_iter of a resident handle (osqp_amd_batch_update_polish, osqp_amd_batch_update_setting); the values
// have passed their rules
void set_polish(BatchPlan &b, c_int polish_new, c_int refine_new) {
  if (polish_new) polish_check_fits(b.dp.P, b.large_factor);
  b.st.polish = polish_new; b.st.polish_refine_iter = refine_new;
}
// `value` for the setting `name` into st, by the rule of the name from the table of the single-model updates (engine.hpp); an
// integer setting takes integral values.  known: the name is in the table; ok: the value passed its rule and is set
void parse_setting(const char *name, c_float value, OSQPSettings &st, bool &known, bool &ok) {
#define OQ_BATCH_SETTING(field, type, cond)                                                                                               \
  if (!known && !strcmp(name, #field)) {                                                                                                  \
    known = true;                                                                                                                         \
    const bool whole = std::is_floating_point<type>::value || (value == std::floor(value) && std::fabs(value) <= 9007199254740992.0);   \
    if (whole && setting_ok_##field((type)value)) { st.field = (type)value; ok = true; }                                                  \
  }
  OQ_UPDATABLE_SETTINGS(OQ_BATCH_SETTING)
#undef OQ_BATCH_SETTING
}
#define OQ_BATCH_CATCH                                                                          \
  catch (const Error &er) { set_last_error(er.what()); return er.code ? er.code : 6; }         \
  catch (const std::exception &ex) { set_last_error(ex.what()); return 6; }

// ---- the shared batch (batch_shared.hpp) ---------------------------------------------------------------
int g_shared_launches = 0;  // launches of k_batch_solve_shared by this process (osqp_amd_shared_batch_launches)
// What a shape needs, from the shape alone: T never depends on the number of instances.
struct SharedPlan { int T; size_t lds_bytes, model_bytes, inst_bytes, factor_lds; };
SharedPlan shared_plan(long long n, long long m, long long nnzA, long long nnzF) {
  if (n <= 0 || n > shared::kMaxN || m < 0 || m > 65535 || nnzA < 0 || nnzA > 65535 || nnzF < 0 || nnzF > 65535)
    throw Error(1, "a shared batch supports 1 <= n <= 256 and fewer than 65536 rows / non-zeros (n = " + std::to_string(n) + ")");
  const size_t fl = large_lds_bytes((int)n, (int)m, (int)nnzA, (int)nnzF);  // k_shared_factor: the layout of k_batch_solve_large
  if (fl > 160 * 1024) throw Error(1, "instance too large for the LDS-resident batched path (needs " + std::to_string(fl) + " bytes of LDS)");
  size_t bytes = 0;
  for (int T : shared::kTileSizes) {
    bytes = shared::lds_bytes((int)n, (int)m, (int)nnzA, T);
    if (bytes <= 160 * 1024)
      return SharedPlan{T, bytes, shared::model_layout((int)n, (int)m, (int)nnzA, (int)nnzF).total * sizeof(double),
                        shared::tile_layout((int)n, (int)m, 1).total * sizeof(double), fl};
  }
  throw Error(1, "instance too large for the LDS-resident batched path (needs " + std::to_string(bytes) + " bytes of LDS)");
}
struct SharedBatch {
  int device = 0, count = 0, n = 0, m = 0, nnzA = 0, nnzP = 0, nnzF = 0, ntiles = 0;
  SharedPlan plan{};
  OSQPSettings st;
  DevicePattern dp;
  shared::ModelLayout ML;
  shared::TileLayout TL;
  DevBuf<double> Px, Ax, q0, l0, u0;   // the raw base data: k_shared_factor runs on them again after a rho update
  DevBuf<double> model, scratch, tiles;
  DevBuf<double> in_a, in_b, x_out, y_out, info_out, adj_out;  // staging of host-pointer calls
  DevBuf<unsigned long long> flag;
  std::vector<double> hdr;  // c, rho, pd of the model block
  // the adjoint (osqp_amd_shared_batch_adjoint): status [count], the status_val of the last resolve; current: the tile records
  // hold the solutions of the current data; adj_factor: the W factor blocks of the form with the factor in global scratch,
  // adj_rows: the bounded row scratch of the summed matrix gradients -- both allocated at first use
  DevBuf<double> status, adj_factor, adj_rows;
  // forward sensitivities (osqp_amd_shared_batch_jvp): the staging of host-pointer calls -- the five tangents come in through
  // in_a, in_b and these three, the outputs leave through adj_out; the factor blocks are adj_factor, whichever call came first
  DevBuf<double> in_c, in_d, in_e;
  bool current = false;
  size_t device_bytes() const {
    return (Px.n + Ax.n + q0.n + l0.n + u0.n + model.n + scratch.n + tiles.n + in_a.n + in_b.n + x_out.n + y_out.n + info_out.n + adj_out.n + status.n +
            adj_factor.n + adj_rows.n + in_c.n + in_d.n + in_e.n + 1) * sizeof(double);
  }
};
SharedBatch *shared_handle(osqp_amd_shared_batch *h) {
  if (!h) { set_last_error("null shared batch handle"); return nullptr; }
  return (SharedBatch *)h;
}
// scaling, row kinds, rho per row and the inverse into the model block; a pivot block that is not positive definite is an Error
void shared_factor(SharedBatch &b, const OSQPSettings &st, hipStream_t s) {
  HIP_CHECK(hipFuncSetAttribute((const void *)shared::k_shared_factor, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b.plan.factor_lds));
  OQ_LAUNCH(shared::k_shared_factor, dim3(1), dim3(NT), b.plan.factor_lds, s, b.dp.P, st, b.Px.get(), b.Ax.get(), b.q0.get(), b.l0.get(), b.u0.get(),
            b.scratch.get(), b.model.get());
  b.hdr.assign(shared::MB_HDR, 0.0);
  b.model.download(b.hdr.data(), shared::MB_HDR, s);
  HIP_CHECK(hipStreamSynchronize(s));
  if (b.hdr[shared::MB_PD] == 0.0) throw Error(7, "problem non convex: the reduced KKT matrix is not positive definite (OSQP_NON_CVX)");
}
// one vector of every instance into the tile records (k_shared_put); stride 0: the same base vector for all
void shared_put(SharedBatch &b, const double *src, int stride, int len, const double *scale, double mult, int clamp, size_t off, hipStream_t s) {
  if (!len) return;
  OQ_LAUNCH(shared::k_shared_put, dim3(blocks_for((int64_t)b.count * len, 256)), dim3(256), 0, s, b.count, len, b.plan.T, src, stride, scale, mult, clamp,
            b.tiles.get(), off, b.TL.total);
}
// the check of new bounds (device pointers) against l <= u and the row kinds of the base: false with the message set
bool shared_bounds_ok(SharedBatch &b, const double *l, const double *u, hipStream_t s) {
  unsigned long long word = ~0ull;
  b.flag.upload(&word, 1, s);
  OQ_LAUNCH(shared::k_shared_check_bounds, dim3(blocks_for((int64_t)b.count * b.m, 256)), dim3(256), 0, s, b.count, b.m, l, u, b.model.get() + b.ML.E,
            (const int *)(b.model.get() + b.ML.ctype), b.flag.get());
  b.flag.download(&word, 1, s);
  HIP_CHECK(hipStreamSynchronize(s));
  if (word == ~0ull) return true;
  const unsigned long long g = word >> 2;
  const std::string at = "instance " + std::to_string(g / b.m) + ", row " + std::to_string(g % b.m);
  if ((word & 3) == 1) set_last_error("lower bound greater than upper bound (" + at + ")");
  else set_last_error("the bounds change the kind of a row (loose / equality / inequality) from the one it has under the base bounds, which the shared "
                      "inverse was built for (" + at + ")");
  return false;
}

// ---- the adjoint of the shared batch (batch_shared_adjoint.hpp) ----------------------------------------
int g_shared_adjoint_launches = 0;  // accepted calls of osqp_amd_shared_batch_adjoint by this process (_adjoint_launches)
constexpr size_t kSharedRowScratch = (size_t)64 << 20;  // bytes of the row scratch of the summed matrix gradients (at least one block of 16)
// The form of k_shared_adjoint a shape takes, from the shape alone: M as a packed triangle in LDS whenever that layout fits
// (n <= 128: factor_solve holds two entries per lane), otherwise the factor in global scratch; a shape neither serves is an Error.
// blocks: W, the factor blocks of the form with the factor in global scratch = the workgroups of its launches: one per compute
// unit, two where the LDS of the layout lets two workgroups share a compute unit (185 VGPRs allow no third) -- 0 for the LDS form
struct SharedAdjointPlan { bool large; polish::Layout L; int blocks; };
SharedAdjointPlan shared_adjoint_plan(const Pattern &P) {
  polish::Layout L = polish::make_layout(P.n, P.m, P.nnzA, P.nnzF, false);
  if (P.n <= kPivotW && L.total <= polish::kLdsLimit) return SharedAdjointPlan{false, L, 0};
  L = polish::make_layout(P.n, P.m, P.nnzA, P.nnzF, true);
  if (P.n > polish::lf::kMaxN || L.total > polish::kLdsLimit)
    throw Error(1, "instance too large to differentiate on the LDS-resident batched path (needs " + std::to_string(L.total) + " bytes of LDS, " +
                       std::to_string(polish::kLdsLimit) + " available, with the factor in global scratch)");
  return SharedAdjointPlan{true, L, shared::kAdjointBlocks * std::min(2, polish::kLdsLimit / L.total)};
}
// One launch of k_shared_adjoint over the instances a.first .. a.first + a.cnt - 1: a workgroup per instance, or at most W of them
// where each needs its factor block
void launch_shared_adjoint(SharedBatch &b, const SharedAdjointPlan &ap, shared::SharedAdjointArgs &a, hipStream_t s) {
  auto *const kern = ap.large ? shared::k_shared_adjoint<true> : shared::k_shared_adjoint<false>;
  const int grid = ap.large ? std::min(a.cnt, ap.blocks) : a.cnt;
  HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, ap.L.total));
  OQ_LAUNCH(kern, dim3(grid), dim3(polish::PT), (size_t)ap.L.total, s, b.dp.P, ap.L, a);
}
// The same for k_shared_jvp (batch_shared_jvp.hpp): the plan, the grid and the factor blocks of the adjoint
int g_shared_jvp_launches = 0;  // accepted calls of osqp_amd_shared_batch_jvp by this process (_jvp_launches)
void launch_shared_jvp(SharedBatch &b, const SharedAdjointPlan &ap, shared::SharedJvpArgs &a, hipStream_t s) {
  auto *const kern = ap.large ? shared::k_shared_jvp<true> : shared::k_shared_jvp<false>;
  const int grid = ap.large ? std::min(a.cnt, ap.blocks) : a.cnt;
  HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, ap.L.total));
  OQ_LAUNCH(kern, dim3(grid), dim3(polish::PT), (size_t)ap.L.total, s, b.dp.P, ap.L, a);
}
void launch_shared_reduce(int ncot, int cnt, int rcount, int cols, bool cont, const double *rows, double *out, hipStream_t s) {
  OQ_LAUNCH(shared::k_shared_reduce_rows, dim3(blocks_for((int64_t)ncot * cols, 256)), dim3(256), 0, s, ncot, cnt, rcount, cols, (int)cont, rows, out);
}

// osqp_amd_batch_adjoint, _multi (subset false: every instance, rows / k unused) and osqp_amd_batch_adjoint_rows, _multi_rows
// (subset true: the k instances of rows; every array of the call is compact, row j for instance rows[j]).  ncot pairs
// (dx, dy) per instance (1 for the two old entries): the cotangent-major arrays are [ncot x cnt x cols], act and status once
// per instance.  One launch of `cnt` workgroups, whatever ncot is.
c_int batch_adjoint(osqp_amd_batch *handle, bool subset, const c_int *rows, c_int k, c_int ncot, const c_float *dx, const c_float *dy,
                    c_float *dq, c_float *dl, c_float *du, c_float *dPx, c_float *dAx, c_float *act_out, c_float *status_out, c_int where) {
  BatchPlan *b = resident_plan(handle);
  if (!b) return 1;
  if (ncot < 1) { set_last_error("invalid batch data: the adjoint needs ncot >= 1"); return 1; }
  if (!dx && !dy) { set_last_error("invalid batch data: the adjoint needs dx or dy"); return 1; }
  if (!subset && !holds_current(*b, nullptr)) return 1;
  try {
    DeviceScope on_dev(b->device);
    hipStream_t s = nullptr;
    Served v;
    if (!serve(*b, subset, rows, k, s, v)) return 1;
    // only the selected instances must be current; nothing is launched when one is not
    if (v.subset && !holds_current(*b, &b->sel_host)) { HIP_CHECK(hipStreamSynchronize(s)); return 1; }
    const size_t cnt = (size_t)v.launch, nc = (size_t)ncot, ln = cnt * b->n, lm = cnt * b->m, lp = cnt * b->nnzP, la = cnt * b->nnzA;
    if (!lm) { dy = nullptr; dl = du = act_out = nullptr; }
    if (!la) dAx = nullptr;
    if (!lp) dPx = nullptr;
    const OutStage o(*b, !where, {dq, dl, du, dPx, dAx, act_out, status_out}, {nc * ln, nc * lm, nc * lm, nc * lp, nc * la, lm, cnt});
    polish::AdjointArgs a;
    a.Px = b->Px.get(); a.Ax = b->Ax.get(); a.l = b->l.get(); a.u = b->u.get(); a.info = b->info_all.get(); a.rec = b->rec.get();
    a.gx = dx ? device_ptr(dx, nc * ln, where, b->in_a, s) : nullptr;
    a.gy = dy ? device_ptr(dy, nc * lm, where, b->in_b, s) : nullptr;
    a.dq = o.dev[0]; a.dl = o.dev[1]; a.du = o.dev[2]; a.dPx = o.dev[3]; a.dAx = o.dev[4]; a.act = o.dev[5]; a.status = o.dev[6];
    a.ncot = (int)ncot; a.info_stride = 6; a.rec_stride = b->rec_stride; a.refine = (int)b->st.polish_refine_iter; a.delta = b->st.delta;
    a.sel = v.sel;
    launch_factor(*b, polish::k_batch_adjoint<false>, polish::k_batch_adjoint<true>, a, v.launch, g_batch_adjoint_launches, s);
    o.download(s);
    HIP_CHECK(hipStreamSynchronize(s));
    return 0;
  } OQ_BATCH_CATCH
}

// osqp_amd_batch_jvp and osqp_amd_batch_jvp_rows, as batch_adjoint above; the direction-major arrays are [ndir x cnt x cols]
c_int batch_jvp(osqp_amd_batch *handle, bool subset, const c_int *rows, c_int k, c_int ndir, const c_float *tq, const c_float *tl,
                const c_float *tu, const c_float *tPx, const c_float *tAx, c_float *tx_out, c_float *ty_out, c_float *act_out,
                c_float *status_out, c_int where) {
  BatchPlan *b = resident_plan(handle);
  if (!b) return 1;
  if (ndir < 1) { set_last_error("invalid batch data: the sensitivities need ndir >= 1"); return 1; }
  if (!tq && !tl && !tu && !tPx && !tAx) { set_last_error("invalid batch data: the sensitivities need a tangent"); return 1; }
  if (!tx_out && !ty_out) { set_last_error("invalid batch data: the sensitivities need tx_out or ty_out"); return 1; }
  if (!subset && !holds_current(*b, nullptr)) return 1;
  try {
    DeviceScope on_dev(b->device);
    hipStream_t s = nullptr;
    Served v;
    if (!serve(*b, subset, rows, k, s, v)) return 1;
    if (v.subset && !holds_current(*b, &b->sel_host)) { HIP_CHECK(hipStreamSynchronize(s)); return 1; }
    const size_t cnt = (size_t)v.launch, nd = (size_t)ndir, ln = cnt * b->n, lm = cnt * b->m, lp = cnt * b->nnzP, la = cnt * b->nnzA;
    if (!lm) { tl = tu = nullptr; ty_out = act_out = nullptr; }
    if (!la) tAx = nullptr;
    if (!lp) tPx = nullptr;
    const OutStage o(*b, !where, {tx_out, ty_out, act_out, status_out}, {nd * ln, nd * lm, lm, cnt});
    polish::JvpArgs a;
    a.Px = b->Px.get(); a.Ax = b->Ax.get(); a.l = b->l.get(); a.u = b->u.get(); a.info = b->info_all.get(); a.rec = b->rec.get();
    a.tq = tq ? device_ptr(tq, nd * ln, where, b->in_a, s) : nullptr;
    a.tl = tl ? device_ptr(tl, nd * lm, where, b->in_b, s) : nullptr;
    a.tu = tu ? device_ptr(tu, nd * lm, where, b->in_c, s) : nullptr;
    a.tPx = tPx ? device_ptr(tPx, nd * lp, where, b->in_d, s) : nullptr;
    a.tAx = tAx ? device_ptr(tAx, nd * la, where, b->in_e, s) : nullptr;
    a.tx = o.dev[0]; a.ty = o.dev[1]; a.act = o.dev[2]; a.status = o.dev[3];
    a.ndir = (int)ndir; a.info_stride = 6; a.rec_stride = b->rec_stride; a.refine = (int)b->st.polish_refine_iter; a.delta = b->st.delta;
    a.sel = v.sel;
    launch_factor(*b, polish::k_batch_jvp<false>, polish::k_batch_jvp<true>, a, v.launch, g_batch_jvp_launches, s);
    o.download(s);
    HIP_CHECK(hipStreamSynchronize(s));
    return 0;
  } OQ_BATCH_CATCH
}

}  // namespace
}  // namespace oq

using namespace oq;

extern "C" {

c_int osqp_amd_batch_last_kernel(void) { return g_batch_last_kernel; }
c_int osqp_amd_batch_last_schedule(c_int *out, c_int count) {
  if (!out || count <= 0) return 0;
  const c_int k = std::min<c_int>(count, kSchedWords);
  for (c_int i = 0; i < k; i++) out[i] = g_batch_last_schedule[i];
  return k;
}
c_int osqp_amd_batch_large(c_int on) {
  const c_int before = g_batch_large;
  g_batch_large = on ? 1 : 0;
  return before;
}
c_int osqp_amd_batch_large_plan(c_int n, c_int m, c_int nnzA, c_int nnzF, c_int *out) {
  try {
    const LargePlan lp = large_plan(n, m, nnzA, nnzF);
    if (out) { out[0] = (c_int)lp.lds_bytes; out[1] = (c_int)lp.scratch_bytes; out[2] = lp.tiles_per_wave; }
    return 0;
  } OQ_BATCH_CATCH
}
c_int osqp_amd_batch_large_factor_plan(c_int n, c_int m, c_int nnzA, c_int nnzF, c_int *out) {
  try {
    const LargeFactorPlan lp = large_factor_plan(n, m, nnzA, nnzF);
    if (out) { out[0] = (c_int)lp.lds_bytes; out[1] = (c_int)lp.scratch_bytes; out[2] = lp.nb; }
    return 0;
  } OQ_BATCH_CATCH
}
// The switch of a handle with n > 128: host state that the next polish / adjoint / JVP launch reads; nothing is launched,
// nothing of the handle changes.  Switching off while settings.polish is 1 would leave a handle whose next resolve refuses: the
// polish setting goes off with it.
c_int osqp_amd_batch_large_factor(osqp_amd_batch *handle, c_int on) {
  BatchPlan *b = resident_plan(handle);
  if (!b) return -1;
  if (!b->dp.large) {
    set_last_error("osqp_amd_batch_large_factor is for handles with 128 < n <= 256 (n = " + std::to_string(b->n) + " keeps its factor in LDS)");
    return -1;
  }
  const c_int before = b->large_factor ? 1 : 0;
  b->large_factor = on != 0;
  if (!b->large_factor) b->st.polish = 0;
  return before;
}
c_int osqp_amd_batch_polish_launches(void) { return g_batch_polish_launches; }
c_int osqp_amd_batch_adjoint_launches(void) { return g_batch_adjoint_launches; }
c_int osqp_amd_batch_jvp_launches(void) { return g_batch_jvp_launches; }
c_int osqp_amd_batch_cert_launches(void) { return g_batch_cert_launches; }

c_int osqp_amd_batch_solve(c_int count, c_int n, c_int m, const c_int *Pp, const c_int *Pi, const c_float *Px_all, const c_int *Ap,
                           const c_int *Ai, const c_float *Ax_all, const c_float *q_all, const c_float *l_all, const c_float *u_all,
                           const OSQPSettings *settings, c_float *x_out, c_float *y_out, OSQPInfo *info_out, c_int device) {
  try {
    const BatchProblem prob{count, n, m, Pp, Pi, Px_all, Ap, Ai, Ax_all, q_all, l_all, u_all, settings};
    if (c_int bad = validate_batch_data(prob, x_out && info_out && (m <= 0 || y_out), g_batch_large ? kLargeMaxN : kPivotW)) return bad;
    DeviceScope on_device((int)device);
    hipStream_t s = nullptr;
    DevicePattern dp;
    dp.build(host_pattern(prob), s);
    dp.large = n > kPivotW;  // past validate_batch_data only while osqp_amd_batch_large is on
    BatchData d;
    d.upload(prob, dp.P, s);
    DevBuf<double> dx((size_t)count * n), dy((size_t)count * m), dinfo((size_t)count * 6);
    BatchIO io = d.inputs();
    io.x = dx.get(); io.y = dy.get(); io.info = dinfo.get();
    io.x_stride = (int)n; io.y_stride = (int)m; io.info_stride = io.info_cols = 6;
    auto t0 = std::chrono::steady_clock::now();
    launch_batch(dp, *settings, (int)count, io, s);
    HIP_CHECK(hipDeviceSynchronize());
    double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::vector<double> hinfo((size_t)count * 6);
    dx.download(x_out, (size_t)count * n, s); dy.download(y_out, (size_t)count * m, s); dinfo.download(hinfo.data(), hinfo.size(), s);
    HIP_CHECK(hipDeviceSynchronize());
    for (c_int i = 0; i < count; i++) {
      OSQPInfo &o = info_out[i];
      memset(&o, 0, sizeof(OSQPInfo));
      o.iter = (c_int)hinfo[i * 6 + 0];
      update_status(&o, (c_int)hinfo[i * 6 + 1]);
      o.pri_res = hinfo[i * 6 + 2]; o.dua_res = hinfo[i * 6 + 3]; o.obj_val = hinfo[i * 6 + 4];
      o.rho_updates = (c_int)hinfo[i * 6 + 5];
      o.solve_time = secs; o.run_time = secs;
      o.rho_estimate = settings->rho;
    }
    return 0;
  } OQ_BATCH_CATCH
}

c_int osqp_amd_batch_solve_generated(c_int first, c_int count, unsigned long long seed, const OSQPSettings *settings, c_float *x_dev,
                                     c_float *y_dev, c_float *info_dev, c_int device) {
  try {
    if (count <= 0 || first < 0) return 1;
    if (validate_settings(settings)) { set_last_error("invalid settings"); return 2; }
    DeviceScope on_device((int)device);
    hipStream_t s = nullptr;
    DevicePattern dp;
    dp.build(mpc_host_pattern(seed), s);
    BatchData d;
    d.generate_mpc((long long)first, (int)count, seed, dp.P, s);
    BatchIO io = d.inputs();
    io.x = x_dev; io.y = y_dev; io.info = info_dev;
    io.x_stride = MPC_N; io.y_stride = MPC_M; io.info_stride = io.info_cols = 4;
    launch_batch(dp, *settings, (int)count, io, s);
    HIP_CHECK(hipDeviceSynchronize());
    return 0;
  } OQ_BATCH_CATCH
}

// ---- sharded MPC batch: K11 + K12 behind one handle -------------------------------------------------------
c_int osqp_amd_batch_mpc_create(osqp_amd_batch **out, c_int total, unsigned long long seed, const OSQPSettings *settings,
                                osqp_amd_comm *comm, c_int device) {
  if (!out) return 1;
  *out = nullptr;
  try {
    if (total <= 0) { set_last_error("empty batch"); return 1; }
    if (validate_settings(settings)) { set_last_error("invalid settings"); return 2; }
    Comm *c = (Comm *)comm;
    const int world = c ? c->world : 1, rank = c ? c->rank : 0;
    if (total % world != 0) { set_last_error("instance count must be divisible by the number of ranks"); return 1; }
    DeviceScope on_device((int)device);
    std::unique_ptr<BatchPlan> b(new BatchPlan());
    b->device = (int)device; b->total = (int)total; b->count = (int)(total / world); b->first = rank * b->count;
    b->comm = c; b->st = *settings;
    hipStream_t s = nullptr;
    b->dp.build(mpc_host_pattern(seed), s);
    b->generate_mpc((long long)b->first, b->count, seed, b->dp.P, s);
    HIP_CHECK(hipDeviceSynchronize());
    *out = (osqp_amd_batch *)b.release();
    return 0;
  } OQ_BATCH_CATCH
}

c_int osqp_amd_batch_mpc_solve(osqp_amd_batch *handle, c_float *packed_dev) {
  if (!handle || !packed_dev) return 1;
  BatchPlan &b = *(BatchPlan *)handle;
  if (b.resident) { set_last_error("this batch handle was not created by osqp_amd_batch_mpc_create"); return 1; }
  try {
    DeviceScope on_device(b.device);
    hipStream_t s = nullptr;
    double *mine = packed_dev + (size_t)b.first * BatchPlan::kRow;
    BatchIO io = b.inputs();
    io.x = mine; io.y = mine + MPC_N; io.info = mine + MPC_N + MPC_M;
    io.x_stride = io.y_stride = io.info_stride = BatchPlan::kRow; io.info_cols = 4;
    launch_batch(b.dp, b.st, b.count, io, s);
    if (b.comm && b.comm->world > 1) b.comm->all_gather(packed_dev, (size_t)b.count * BatchPlan::kRow, s);
    HIP_CHECK(hipStreamSynchronize(s));
    return 0;
  } OQ_BATCH_CATCH
}

// ---- resident batch of the caller's own QPs: setup once, update vectors / values in place, re-solve warm ---------------------
c_int osqp_amd_batch_setup(osqp_amd_batch **out, c_int count, c_int n, c_int m, const c_int *Pp, const c_int *Pi, const c_float *Px_all,
                           const c_int *Ap, const c_int *Ai, const c_float *Ax_all, const c_float *q_all, const c_float *l_all,
                           const c_float *u_all, const OSQPSettings *settings, c_int device) {
  if (!out) { set_last_error("invalid batch data"); return 1; }
  *out = nullptr;
  try {
    const BatchProblem prob{count, n, m, Pp, Pi, Px_all, Ap, Ai, Ax_all, q_all, l_all, u_all, settings};
    if (c_int bad = validate_batch_data(prob, true, g_batch_large ? kLargeMaxN : kPivotW)) return bad;
    DeviceScope on_device((int)device);
    hipStream_t s = nullptr;
    std::unique_ptr<BatchPlan> b(new BatchPlan());
    b->resident = true; b->device = (int)device; b->total = b->count = (int)count; b->st = *settings;
    b->n = (int)n; b->m = (int)m; b->nnzP = (int)Pp[n]; b->nnzA = (int)Ap[n]; b->rec_stride = rec_doubles((int)n, (int)m);
    b->dp.build(host_pattern(prob), s);
    b->dp.large = n > kPivotW;  // the handle stays on the path it was built on, whatever the switch does later
    if (settings->polish) polish_check_fits(b->dp.P);
    const size_t cnt = (size_t)count;
    b->upload(prob, b->dp.P, s);
    b->x_out.alloc(cnt * n); b->y_out.alloc(cnt * m); b->info_out.alloc(cnt * 6); b->bad.alloc(1); b->pstat.alloc(cnt);
    b->info_all.alloc(cnt * 6); b->current.assign(cnt, 0);
    {
      const std::vector<double> nan(cnt * std::max(n, m), NAN);
      b->pcert.alloc(cnt * m); b->dcert.alloc(cnt * n);
      b->pcert.upload(nan.data(), cnt * m, s); b->dcert.upload(nan.data(), cnt * n, s);
      HIP_CHECK(hipStreamSynchronize(s));  // nan leaves scope
    }
    // the records: a zero iterate (the first solve starts from zero either way), the rho of the settings
    std::vector<double> hrec(cnt * b->rec_stride, 0.0);
    for (size_t i = 0; i < cnt; i++) hrec[i * b->rec_stride + REC_RHO] = settings->rho;
    b->rec.alloc(hrec.size()); b->rec.upload(hrec.data(), hrec.size(), s);
    resident_equilibrate(*b, b->count, nullptr, s);  // D, E, c come from the setup data and stay until the matrices change
    HIP_CHECK(hipDeviceSynchronize());
    *out = (osqp_amd_batch *)b.release();
    return 0;
  } OQ_BATCH_CATCH
}

// The calls below serve every instance (osqp_amd_batch_X: subset false, rows / k unused, arrays [count x .]) or a selection
// (osqp_amd_batch_X_rows, include/osqp_amd.h: subset true, arrays compact [k x .], row j for instance rows[j]): one body each,
// the entries forward.  The handle and the required arrays are checked first; a whole call with nothing to do returns before
// any device call; a selection is checked and uploaded before anything else (`serve`), so a bad one is refused even when
// there is nothing to do.
static c_int batch_update_lin_cost(osqp_amd_batch *handle, bool subset, const c_int *rows, c_int k, const c_float *q, c_int where) {
  BatchPlan *b = resident_plan(handle);
  if (!b) return 1;
  if (!q) { set_last_error("invalid batch data"); return 1; }
  try {
    DeviceScope on_dev(b->device);
    hipStream_t s = nullptr;
    Served v;
    if (!serve(*b, subset, rows, k, s, v)) return 1;
    mark(*b, v, false);
    put_rows(*b, v, b->n, q, where, b->in_a, b->q, s);
    HIP_CHECK(hipStreamSynchronize(s));
    return 0;
  } OQ_BATCH_CATCH
}
c_int osqp_amd_batch_update_lin_cost(osqp_amd_batch *handle, const c_float *q_all, c_int where) {
  return batch_update_lin_cost(handle, false, nullptr, 0, q_all, where);
}
c_int osqp_amd_batch_update_lin_cost_rows(osqp_amd_batch *handle, const c_int *rows, c_int k, const c_float *q_rows, c_int where) {
  return batch_update_lin_cost(handle, true, rows, k, q_rows, where);
}

static c_int batch_update_bounds(osqp_amd_batch *handle, bool subset, const c_int *rows, c_int k, const c_float *l, const c_float *u, c_int where) {
  BatchPlan *b = resident_plan(handle);
  if (!b) return 1;
  const bool nothing = b->m == 0 || (!l && !u);
  if (nothing && !subset) return 0;
  try {
    DeviceScope on_dev(b->device);
    hipStream_t s = nullptr;
    Served v;
    if (!serve(*b, subset, rows, k, s, v)) return 1;
    if (nothing) { HIP_CHECK(hipStreamSynchronize(s)); return 0; }
    const size_t len = (size_t)v.launch * b->m;
    // checked on the device against the bound that stays (of the same instance), before anything of the handle changes
    const double *ln = l ? device_ptr(l, len, where, b->in_a, s) : nullptr;
    const double *un = u ? device_ptr(u, len, where, b->in_b, s) : nullptr;
    int bad = 0;
    HIP_CHECK(hipMemsetAsync(b->bad.get(), 0, sizeof(int), s));
    if (v.subset)
      OQ_LAUNCH(k_batch_check_bounds_rows, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s, v.sel, v.launch, b->m, ln, un, b->l.get(), b->u.get(),
                b->bad.get());
    else
      OQ_LAUNCH(k_batch_check_bounds, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s, len, ln ? ln : b->l.get(), un ? un : b->u.get(), b->bad.get());
    b->bad.download(&bad, 1, s);
    HIP_CHECK(hipStreamSynchronize(s));
    if (bad) { set_last_error("lower bound greater than upper bound"); return 1; }
    mark(*b, v, false);
    if (ln) put_rows(*b, v, b->m, ln, 1, b->in_a, b->l, s);  // on the device by now
    if (un) put_rows(*b, v, b->m, un, 1, b->in_b, b->u, s);
    HIP_CHECK(hipStreamSynchronize(s));
    return 0;
  } OQ_BATCH_CATCH
}
c_int osqp_amd_batch_update_bounds(osqp_amd_batch *handle, const c_float *l_all, const c_float *u_all, c_int where) {
  return batch_update_bounds(handle, false, nullptr, 0, l_all, u_all, where);
}
c_int osqp_amd_batch_update_bounds_rows(osqp_amd_batch *handle, const c_int *rows, c_int k, const c_float *l_rows, const c_float *u_rows,
                                        c_int where) {
  return batch_update_bounds(handle, true, rows, k, l_rows, u_rows, where);
}

static c_int batch_update_matrices(osqp_amd_batch *handle, bool subset, const c_int *rows, c_int k, const c_float *Px, const c_float *Ax, c_int where) {
  BatchPlan *b = resident_plan(handle);
  if (!b) return 1;
  const bool nothing = !Px && !Ax;
  if (nothing && !subset) return 0;
  try {
    DeviceScope on_dev(b->device);
    hipStream_t s = nullptr;
    Served v;
    if (!serve(*b, subset, rows, k, s, v)) return 1;
    if (nothing) { HIP_CHECK(hipStreamSynchronize(s)); return 0; }
    mark(*b, v, false);
    if (Px) put_rows(*b, v, b->nnzP, Px, where, b->in_a, b->Px, s);
    if (Ax) put_rows(*b, v, b->nnzA, Ax, where, b->in_b, b->Ax, s);
    // from scratch on the raw data with the current q, l, u, the served instances only; the scaled iterate stays as it is
    resident_equilibrate(*b, v.launch, v.sel, s);
    HIP_CHECK(hipStreamSynchronize(s));
    return 0;
  } OQ_BATCH_CATCH
}
c_int osqp_amd_batch_update_matrices(osqp_amd_batch *handle, const c_float *Px_all, const c_float *Ax_all, c_int where) {
  return batch_update_matrices(handle, false, nullptr, 0, Px_all, Ax_all, where);
}
c_int osqp_amd_batch_update_matrices_rows(osqp_amd_batch *handle, const c_int *rows, c_int k, const c_float *Px_rows, const c_float *Ax_rows,
                                          c_int where) {
  return batch_update_matrices(handle, true, rows, k, Px_rows, Ax_rows, where);
}

static c_int batch_warm_start(osqp_amd_batch *handle, bool subset, const c_int *rows, c_int k, const c_float *x, const c_float *y, c_int where) {
  BatchPlan *b = resident_plan(handle);
  if (!b) return 1;
  const bool nothing = !x && !y;
  if (nothing && !subset) return 0;
  try {
    DeviceScope on_dev(b->device);
    hipStream_t s = nullptr;
    Served v;
    if (!serve(*b, subset, rows, k, s, v)) return 1;
    if (nothing) { HIP_CHECK(hipStreamSynchronize(s)); return 0; }
    mark(*b, v, false);
    const double *xd = x ? device_ptr(x, (size_t)v.launch * b->n, where, b->in_a, s) : nullptr;
    const double *yd = y && b->m ? device_ptr(y, (size_t)v.launch * b->m, where, b->in_b, s) : nullptr;
    OQ_LAUNCH(k_batch_warm, dim3(v.launch), dim3(256), 0, s, b->dp.P, v.launch, b->Ax.get(), xd, yd, b->rec.get(), b->rec_stride, v.sel);
    HIP_CHECK(hipStreamSynchronize(s));
    b->st.warm_start = 1;  // a setting of the handle, as osqp_warm_start does
    return 0;
  } OQ_BATCH_CATCH
}
c_int osqp_amd_batch_warm_start(osqp_amd_batch *handle, const c_float *x_all, const c_float *y_all, c_int where) {
  return batch_warm_start(handle, false, nullptr, 0, x_all, y_all, where);
}
c_int osqp_amd_batch_warm_start_rows(osqp_amd_batch *handle, const c_int *rows, c_int k, const c_float *x_rows, const c_float *y_rows,
                                     c_int where) {
  return batch_warm_start(handle, true, rows, k, x_rows, y_rows, where);
}

static c_int batch_resolve(osqp_amd_batch *handle, bool subset, const c_int *rows, c_int k, c_float *x_out, c_float *y_out, c_float *info_out,
                           c_int where) {
  BatchPlan *b = resident_plan(handle);
  if (!b) return 1;
  if (!x_out || !info_out || (b->m > 0 && !y_out)) { set_last_error("invalid batch data"); return 1; }
  try {
    DeviceScope on_dev(b->device);
    hipStream_t s = nullptr;
    Served v;
    if (!serve(*b, subset, rows, k, s, v)) return 1;
    // host pointers: through the first v.launch rows of the staging.  The info rows of every instance go straight into
    // info_all; those of a selection are compact (info_out) and scattered into it below
    DevBuf<double> &info_stage = v.subset ? b->info_out : b->info_all;
    BatchIO io = b->inputs();
    io.x = where ? x_out : b->x_out.get(); io.y = where ? y_out : b->y_out.get(); io.info = where ? info_out : info_stage.get();
    io.x_stride = b->n; io.y_stride = b->m; io.info_stride = io.info_cols = 6;
    // (a resolve that failed between its solve launch and k_batch_cert may have left directions where the records of
    // infeasible instances hold zeros: the next one starts every instance it serves from zero and rewrites their records)
    io.rec = b->rec.get(); io.rec_stride = b->rec_stride; io.sel = v.sel;
    io.res_mode = RES_SOLVE | RES_CERT | (b->st.warm_start && !b->rec_raw ? RES_WARM : 0) | (b->gap_rule ? RES_GAP : 0);
    b->rec_raw = true;
    launch_batch(b->dp, b->st, v.launch, io, s);
    launch_cert(*b, io, v.launch, s);  // before anything else reads the records: it puts them back as a solve without RES_CERT leaves them
    b->rec_raw = false;
    // the polish status is of every instance's own last resolve: after a selection the others keep theirs (all 0 while the
    // buffer is not live), and the selected ones read 0 when polish is off
    const bool was_live = b->pstat_live;
    if (v.subset && !was_live) b->pstat.zero(s);
    b->pstat_live = v.subset || b->st.polish != 0;
    if (b->st.polish) launch_polish(*b, io, v.launch, s);
    else if (v.subset && was_live) OQ_LAUNCH(k_batch_fill_rows, dim3(blocks_for(v.launch, 256)), dim3(256), 0, s, v.sel, v.launch, 0.0, b->pstat.get());
    // the statuses, for osqp_amd_batch_adjoint: after the polish launch, which rewrites the residuals
    if (v.subset) scatter_rows(*b, v.launch, 6, io.info, b->info_all.get(), s);
    else if (where) copy_d2d(b->info_all.get(), info_out, (size_t)v.launch * 6, s);
    if (!where) {
      b->x_out.download(x_out, (size_t)v.launch * b->n, s);
      if (b->m) b->y_out.download(y_out, (size_t)v.launch * b->m, s);
      info_stage.download(info_out, (size_t)v.launch * 6, s);
    }
    HIP_CHECK(hipStreamSynchronize(s));
    mark(*b, v, true);
    return 0;
  } OQ_BATCH_CATCH
}
c_int osqp_amd_batch_resolve(osqp_amd_batch *handle, c_float *x_out, c_float *y_out, c_float *info_out, c_int where) {
  return batch_resolve(handle, false, nullptr, 0, x_out, y_out, info_out, where);
}
c_int osqp_amd_batch_resolve_rows(osqp_amd_batch *handle, const c_int *rows, c_int k, c_float *x_out, c_float *y_out, c_float *info_out,
                                  c_int where) {
  return batch_resolve(handle, true, rows, k, x_out, y_out, info_out, where);
}

c_int osqp_amd_batch_adjoint(osqp_amd_batch *handle, const c_float *dx, const c_float *dy, c_float *dq, c_float *dl, c_float *du,
                             c_float *dPx, c_float *dAx, c_float *act_out, c_float *status_out, c_int where) {
  return batch_adjoint(handle, false, nullptr, 0, 1, dx, dy, dq, dl, du, dPx, dAx, act_out, status_out, where);
}
c_int osqp_amd_batch_adjoint_rows(osqp_amd_batch *handle, const c_int *rows, c_int k, const c_float *dx, const c_float *dy, c_float *dq,
                                  c_float *dl, c_float *du, c_float *dPx, c_float *dAx, c_float *act_out, c_float *status_out, c_int where) {
  return batch_adjoint(handle, true, rows, k, 1, dx, dy, dq, dl, du, dPx, dAx, act_out, status_out, where);
}
c_int osqp_amd_batch_adjoint_multi(osqp_amd_batch *handle, c_int ncot, const c_float *dx, const c_float *dy, c_float *dq, c_float *dl,
                                   c_float *du, c_float *dPx, c_float *dAx, c_float *act_out, c_float *status_out, c_int where) {
  return batch_adjoint(handle, false, nullptr, 0, ncot, dx, dy, dq, dl, du, dPx, dAx, act_out, status_out, where);
}
c_int osqp_amd_batch_adjoint_multi_rows(osqp_amd_batch *handle, const c_int *rows, c_int k, c_int ncot, const c_float *dx, const c_float *dy,
                                        c_float *dq, c_float *dl, c_float *du, c_float *dPx, c_float *dAx, c_float *act_out,
                                        c_float *status_out, c_int where) {
  return batch_adjoint(handle, true, rows, k, ncot, dx, dy, dq, dl, du, dPx, dAx, act_out, status_out, where);
}

c_int osqp_amd_batch_jvp(osqp_amd_batch *handle, c_int ndir, const c_float *tq, const c_float *tl, const c_float *tu, const c_float *tPx,
                         const c_float *tAx, c_float *tx_out, c_float *ty_out, c_float *act_out, c_float *status_out, c_int where) {
  return batch_jvp(handle, false, nullptr, 0, ndir, tq, tl, tu, tPx, tAx, tx_out, ty_out, act_out, status_out, where);
}
c_int osqp_amd_batch_jvp_rows(osqp_amd_batch *handle, const c_int *rows, c_int k, c_int ndir, const c_float *tq, const c_float *tl,
                              const c_float *tu, const c_float *tPx, const c_float *tAx, c_float *tx_out, c_float *ty_out, c_float *act_out,
                              c_float *status_out, c_int where) {
  return batch_jvp(handle, true, rows, k, ndir, tq, tl, tu, tPx, tAx, tx_out, ty_out, act_out, status_out, where);
}

static c_int batch_polish_status(osqp_amd_batch *handle, bool subset, const c_int *rows, c_int k, c_float *status_out, c_int where) {
  BatchPlan *b = resident_plan(handle);
  if (!b) return 1;
  if (!status_out) { set_last_error("invalid batch data"); return 1; }
  try {
    DeviceScope on_dev(b->device);
    hipStream_t s = nullptr;
    Served v;
    if (!serve(*b, subset, rows, k, s, v)) return 1;
    const size_t len = (size_t)v.launch;
    if (!b->pstat_live) {  // no resolve yet, or the last one did not polish: all 0, whatever the buffer holds
      if (where) HIP_CHECK(hipMemsetAsync(status_out, 0, len * sizeof(double), s));
      else std::fill(status_out, status_out + len, 0.0);
    } else {  // a selection with a host pointer: gathered into the staging, then down
      const OutStage o(*b, v.subset && !where, {status_out}, {len});
      give_rows(*b, v, 1, b->pstat, o.dev[0], where, s);
      o.download(s);
    }
    HIP_CHECK(hipStreamSynchronize(s));
    return 0;
  } OQ_BATCH_CATCH
}
c_int osqp_amd_batch_polish_status(osqp_amd_batch *handle, c_float *status_out, c_int where) {
  return batch_polish_status(handle, false, nullptr, 0, status_out, where);
}
c_int osqp_amd_batch_polish_status_rows(osqp_amd_batch *handle, const c_int *rows, c_int k, c_float *status_out, c_int where) {
  return batch_polish_status(handle, true, rows, k, status_out, where);
}

c_int osqp_amd_batch_update_polish(osqp_amd_batch *handle, c_int polish_new, c_int polish_refine_iter_new) {
  BatchPlan *b = resident_plan(handle);
  if (!b) return 1;
  if (!setting_ok_polish(polish_new)) { set_last_error("polish must be 0 or 1"); return 1; }
  if (!setting_ok_polish_refine_iter(polish_refine_iter_new)) { set_last_error("polish_refine_iter must be nonnegative"); return 1; }
  try {
    set_polish(*b, polish_new, polish_refine_iter_new);
    return 0;
  } OQ_BATCH_CATCH
}

c_int osqp_amd_batch_update_setting(osqp_amd_batch *handle, const char *name, c_float value) {
  BatchPlan *b = resident_plan(handle);
  if (!b) return 1;
  if (!name) { set_last_error("invalid batch data"); return 1; }
  try {
    OSQPSettings st = b->st;
    bool known = false, ok = false;
    parse_setting(name, value, st, known, ok);
    if (!known) { set_last_error(std::string(name) + " cannot be updated or is not recognized"); return 1; }
    if (!ok) { set_last_error(std::string("invalid value for the setting ") + name); return 1; }
    if (!strcmp(name, "polish") || !strcmp(name, "polish_refine_iter")) { set_polish(*b, st.polish, st.polish_refine_iter); return 0; }
    if (!strcmp(name, "rho")) {  // also the stored rho of every instance, as osqp_update_rho rebuilds rho_vec from it
      DeviceScope on_dev(b->device);
      hipStream_t s = nullptr;
      st.rho = std::min(std::max(st.rho, (c_float)B_RHO_MIN), (c_float)B_RHO_MAX);
      OQ_LAUNCH(k_batch_fill_hdr, dim3(blocks_for(b->count, 256)), dim3(256), 0, s, b->count, (int)REC_RHO, (double)st.rho, b->rec.get(), b->rec_stride);
      HIP_CHECK(hipStreamSynchronize(s));
    }
    b->st = st;  // acts from the next resolve; data and iterate are unchanged: `current`, the certificates and polish_status stay
    return 0;
  } OQ_BATCH_CATCH
}

static c_int batch_certificates(osqp_amd_batch *handle, bool subset, const c_int *rows, c_int k, c_float *prim_inf_cert_out,
                                c_float *dual_inf_cert_out, c_int where) {
  BatchPlan *b = resident_plan(handle);
  if (!b) return 1;
  if (b->m == 0) prim_inf_cert_out = nullptr;
  if (!prim_inf_cert_out && !dual_inf_cert_out) { set_last_error("invalid batch data: no certificate was asked for"); return 1; }
  try {
    DeviceScope on_dev(b->device);
    hipStream_t s = nullptr;
    Served v;
    if (!serve(*b, subset, rows, k, s, v)) return 1;
    const DevBuf<double> *const src[2] = {&b->pcert, &b->dcert};
    const int cols[2] = {b->m, b->n};
    // a selection with host pointers: the two are gathered into the shared staging, in this order
    const OutStage o(*b, v.subset && !where, {prim_inf_cert_out, dual_inf_cert_out}, {(size_t)v.launch * b->m, (size_t)v.launch * b->n});
    for (int j = 0; j < 2; j++) {
      if (!o.host[j]) continue;
      give_rows(*b, v, cols[j], *src[j], o.dev[j], where, s);
      o.download(j, s);  // each behind its own gather, as the copies always were issued
    }
    HIP_CHECK(hipStreamSynchronize(s));
    return 0;
  } OQ_BATCH_CATCH
}
c_int osqp_amd_batch_certificates(osqp_amd_batch *handle, c_float *prim_inf_cert_out, c_float *dual_inf_cert_out, c_int where) {
  return batch_certificates(handle, false, nullptr, 0, prim_inf_cert_out, dual_inf_cert_out, where);
}
c_int osqp_amd_batch_certificates_rows(osqp_amd_batch *handle, const c_int *rows, c_int k, c_float *prim_inf_cert_out,
                                       c_float *dual_inf_cert_out, c_int where) {
  return batch_certificates(handle, true, rows, k, prim_inf_cert_out, dual_inf_cert_out, where);
}

// osqp_amd_batch_duality (subset false) and osqp_amd_batch_duality_rows: one launch of k_batch_gap (batch_gap.hpp), one
// workgroup per served instance; row j of out is of instance j, or of rows[j].  Only reads the handle (the selection and the
// staging of a host-pointer call are per-call scratch, as for the certificates).
static c_int batch_duality(osqp_amd_batch *handle, bool subset, const c_int *rows, c_int k, c_float *out, c_int where) {
  BatchPlan *b = resident_plan(handle);
  if (!b) return 1;
  if (!out) { set_last_error("invalid batch data: no output array"); return 1; }
  if (!subset && !holds_current(*b, nullptr)) return 1;
  try {
    DeviceScope on_dev(b->device);
    hipStream_t s = nullptr;
    Served v;
    if (!serve(*b, subset, rows, k, s, v)) return 1;
    // only the selected instances must be current; nothing is launched when one is not
    if (v.subset && !holds_current(*b, &b->sel_host)) { HIP_CHECK(hipStreamSynchronize(s)); return 1; }
    const OutStage o(*b, !where, {out}, {(size_t)v.launch * 3});
    gap::Args a;
    a.Px = b->Px.get(); a.q = b->q.get(); a.l = b->l.get(); a.u = b->u.get(); a.info = b->info_all.get(); a.rec = b->rec.get();
    a.out = o.dev[0];
    a.info_stride = 6; a.rec_stride = b->rec_stride; a.sel = v.sel;
    OQ_LAUNCH(gap::k_batch_gap, dim3(v.launch), dim3(gap::GT), 0, s, b->dp.P, v.launch, a);
    o.download(s);
    HIP_CHECK(hipStreamSynchronize(s));
    return 0;
  } OQ_BATCH_CATCH
}
c_int osqp_amd_batch_duality(osqp_amd_batch *handle, c_float *out, c_int where) { return batch_duality(handle, false, nullptr, 0, out, where); }
c_int osqp_amd_batch_duality_rows(osqp_amd_batch *handle, const c_int *rows, c_int k, c_float *out, c_int where) {
  return batch_duality(handle, true, rows, k, out, where);
}

// The gap stopping rule of the resident batch: the switch is host state that the next resolve, whole
// or _rows, turns into RES_GAP; the iterate, rho, `current`, the certificates and the polish status stay.  The refusal counts
// start from zero at every switch.
c_int osqp_amd_batch_duality_gap_check(osqp_amd_batch *handle, c_int on) {
  BatchPlan *b = resident_plan(handle);
  if (!b) return 1;
  try {
    DeviceScope on_dev(b->device);
    hipStream_t s = nullptr;
    OQ_LAUNCH(k_batch_fill_hdr, dim3(blocks_for(b->count, 256)), dim3(256), 0, s, b->count, (int)REC_GAPREF, 0.0, b->rec.get(), b->rec_stride);
    HIP_CHECK(hipStreamSynchronize(s));
    b->gap_rule = on != 0;
    return 0;
  } OQ_BATCH_CATCH
}

// osqp_amd_batch_gap_refusals (subset false) and _rows: out[j] = the checks of the own last resolve of instance j (rows[j])
// that the gap test alone refused; zeros while the rule is off.  Only reads the handle.
static c_int batch_gap_refusals(osqp_amd_batch *handle, bool subset, const c_int *rows, c_int k, c_float *out, c_int where) {
  BatchPlan *b = resident_plan(handle);
  if (!b) return 1;
  if (!out) { set_last_error("invalid batch data: no output array"); return 1; }
  try {
    DeviceScope on_dev(b->device);
    hipStream_t s = nullptr;
    Served v;
    if (!serve(*b, subset, rows, k, s, v)) return 1;
    const OutStage o(*b, !where, {out}, {(size_t)v.launch});
    OQ_LAUNCH(k_batch_gap_refusals, dim3(blocks_for(v.launch, 256)), dim3(256), 0, s, v.sel, v.launch, (int)b->gap_rule, (const double *)b->rec.get(),
              b->rec_stride, o.dev[0]);
    o.download(s);
    HIP_CHECK(hipStreamSynchronize(s));
    return 0;
  } OQ_BATCH_CATCH
}
c_int osqp_amd_batch_gap_refusals(osqp_amd_batch *handle, c_float *out, c_int where) { return batch_gap_refusals(handle, false, nullptr, 0, out, where); }
c_int osqp_amd_batch_gap_refusals_rows(osqp_amd_batch *handle, const c_int *rows, c_int k, c_float *out, c_int where) {
  return batch_gap_refusals(handle, true, rows, k, out, where);
}

c_int osqp_amd_batch_destroy(osqp_amd_batch *handle) {
  if (!handle) return 0;
  BatchPlan *b = (BatchPlan *)handle;
  try { DeviceScope on_device(b->device); delete b; } catch (...) { return 1; }
  return 0;
}

// ---- the shared batch: one model, many right-hand sides on one inverse (include/osqp_amd.h) ------------
c_int osqp_amd_shared_batch_plan(c_int n, c_int m, c_int nnzA, c_int nnzF, c_int *out) {
  try {
    const SharedPlan sp = shared_plan(n, m, nnzA, nnzF);
    if (out) { out[0] = sp.T; out[1] = (c_int)sp.lds_bytes; out[2] = (c_int)sp.model_bytes; out[3] = (c_int)sp.inst_bytes; }
    return 0;
  } OQ_BATCH_CATCH
}
c_int osqp_amd_shared_batch_launches(void) { return g_shared_launches; }

c_int osqp_amd_shared_batch_setup(osqp_amd_shared_batch **out, c_int count, c_int n, c_int m, const c_int *Pp, const c_int *Pi, const c_float *Px,
                                  const c_int *Ap, const c_int *Ai, const c_float *Ax, const c_float *q0, const c_float *l0, const c_float *u0,
                                  const OSQPSettings *settings, c_int device) {
  if (!out) { set_last_error("invalid batch data"); return 1; }
  *out = nullptr;
  try {
    if (count <= 0 || count > 16777216) { set_last_error("invalid batch data"); return 1; }
    if (n > shared::kMaxN) { set_last_error("a shared batch supports 1 <= n <= 256 and fewer than 65536 rows / non-zeros (n = " + std::to_string(n) + ")"); return 1; }
    // the data checks of the batched path, for ONE instance and with the cap of this path
    const BatchProblem prob{1, n, m, Pp, Pi, Px, Ap, Ai, Ax, q0, l0, u0, settings};
    if (c_int bad = validate_batch_data(prob, true, shared::kMaxN)) return bad;
    if (settings->adaptive_rho) {
      set_last_error("adaptive_rho must be 0 for a shared batch: all instances share one inverse of the reduced KKT matrix, which is built for one rho "
                     "(change it with osqp_amd_shared_batch_update_setting(\"rho\"))");
      return 2;
    }
    const HostPattern hp = host_pattern(prob);
    std::unique_ptr<SharedBatch> b(new SharedBatch());
    b->plan = shared_plan(n, m, hp.nnzA, hp.nnzF);
    DeviceScope on_device((int)device);
    hipStream_t s = nullptr;
    b->device = (int)device; b->count = (int)count; b->st = *settings;
    b->n = (int)n; b->m = (int)m; b->nnzA = hp.nnzA; b->nnzP = hp.nnzP; b->nnzF = hp.nnzF;
    b->ML = shared::model_layout(b->n, b->m, b->nnzA, b->nnzF); b->TL = shared::tile_layout(b->n, b->m, b->plan.T);
    b->ntiles = (b->count + b->plan.T - 1) / b->plan.T;
    b->dp.build(hp, s);
    b->Px.alloc(b->nnzP); b->Ax.alloc(b->nnzA); b->q0.alloc(n); b->l0.alloc(m); b->u0.alloc(m);
    b->Px.upload(Px, b->nnzP, s); b->Ax.upload(Ax, b->nnzA, s); b->q0.upload(q0, n, s); b->l0.upload(l0, m, s); b->u0.upload(u0, m, s);
    b->model.alloc(b->ML.total); b->scratch.alloc((size_t)n * n); b->tiles.alloc((size_t)b->ntiles * b->TL.total); b->flag.alloc(1);
    const size_t cnt = (size_t)count;
    b->x_out.alloc(cnt * n); b->y_out.alloc(cnt * m); b->info_out.alloc(cnt * 6); b->status.alloc(cnt);
    shared_factor(*b, b->st, s);
    // every instance holds (q0, l0, u0) and a zero iterate
    OQ_LAUNCH(shared::k_shared_zero, dim3(blocks_for((int64_t)b->tiles.n, 256)), dim3(256), 0, s, b->tiles.n, b->tiles.get());
    shared_put(*b, b->q0.get(), 0, b->n, b->model.get() + b->ML.D, b->hdr[shared::MB_C], 0, b->TL.q, s);
    shared_put(*b, b->l0.get(), 0, b->m, b->model.get() + b->ML.E, 1.0, -1, b->TL.l, s);
    shared_put(*b, b->u0.get(), 0, b->m, b->model.get() + b->ML.E, 1.0, 1, b->TL.u, s);
    HIP_CHECK(hipDeviceSynchronize());
    *out = (osqp_amd_shared_batch *)b.release();
    return 0;
  } OQ_BATCH_CATCH
}

c_int osqp_amd_shared_batch_update_lin_cost(osqp_amd_shared_batch *handle, const c_float *q_all, c_int where) {
  SharedBatch *b = shared_handle(handle);
  if (!b) return 1;
  if (!q_all) { set_last_error("invalid batch data"); return 1; }
  try {
    DeviceScope on_dev(b->device);
    hipStream_t s = nullptr;
    const double *qd = device_ptr(q_all, (size_t)b->count * b->n, where, b->in_a, s);
    b->current = false;
    shared_put(*b, qd, b->n, b->n, b->model.get() + b->ML.D, b->hdr[shared::MB_C], 0, b->TL.q, s);
    HIP_CHECK(hipStreamSynchronize(s));
    return 0;
  } OQ_BATCH_CATCH
}

c_int osqp_amd_shared_batch_update_bounds(osqp_amd_shared_batch *handle, const c_float *l_all, const c_float *u_all, c_int where) {
  SharedBatch *b = shared_handle(handle);
  if (!b) return 1;
  if (b->m == 0) return 0;
  if (!l_all || !u_all) { set_last_error("a shared batch updates both bounds in one call"); return 1; }
  try {
    DeviceScope on_dev(b->device);
    hipStream_t s = nullptr;
    const size_t len = (size_t)b->count * b->m;
    const double *ld = device_ptr(l_all, len, where, b->in_a, s), *ud = device_ptr(u_all, len, where, b->in_b, s);
    if (!shared_bounds_ok(*b, ld, ud, s)) return 1;  // before anything of the handle is written
    b->current = false;
    shared_put(*b, ld, b->m, b->m, b->model.get() + b->ML.E, 1.0, -1, b->TL.l, s);
    shared_put(*b, ud, b->m, b->m, b->model.get() + b->ML.E, 1.0, 1, b->TL.u, s);
    HIP_CHECK(hipStreamSynchronize(s));
    return 0;
  } OQ_BATCH_CATCH
}

c_int osqp_amd_shared_batch_warm_start(osqp_amd_shared_batch *handle, const c_float *x_all, const c_float *y_all, c_int where) {
  SharedBatch *b = shared_handle(handle);
  if (!b) return 1;
  if (!x_all && !y_all) return 0;
  try {
    DeviceScope on_dev(b->device);
    hipStream_t s = nullptr;
    const double *xd = x_all ? device_ptr(x_all, (size_t)b->count * b->n, where, b->in_a, s) : nullptr;
    const double *yd = y_all && b->m ? device_ptr(y_all, (size_t)b->count * b->m, where, b->in_b, s) : nullptr;
    b->current = false;
    OQ_LAUNCH(shared::k_shared_warm, dim3(blocks_for((int64_t)b->count * (b->n + b->m), 256)), dim3(256), 0, s, b->dp.P, b->count, b->plan.T, b->Ax.get(),
              b->model.get(), xd, yd, b->tiles.get());
    HIP_CHECK(hipStreamSynchronize(s));
    b->st.warm_start = 1;  // as osqp_warm_start does
    return 0;
  } OQ_BATCH_CATCH
}

c_int osqp_amd_shared_batch_resolve(osqp_amd_shared_batch *handle, c_float *x_out, c_float *y_out, c_float *info_out, c_int where) {
  SharedBatch *b = shared_handle(handle);
  if (!b) return 1;
  if (!x_out || !info_out || (b->m > 0 && !y_out)) { set_last_error("invalid batch data"); return 1; }
  try {
    DeviceScope on_dev(b->device);
    hipStream_t s = nullptr;
    double *xd = where ? x_out : b->x_out.get(), *yd = where ? y_out : b->y_out.get(), *id = where ? info_out : b->info_out.get();
    HIP_CHECK(hipFuncSetAttribute((const void *)shared::k_batch_solve_shared, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b->plan.lds_bytes));
    g_batch_last_kernel = shared::kLastKernel;
    g_shared_launches++;
    OQ_LAUNCH(shared::k_batch_solve_shared, dim3(b->ntiles), dim3(NT), b->plan.lds_bytes, s, b->dp.P, b->st, b->count, b->plan.T, (int)(b->st.warm_start != 0),
              (const double *)b->model.get(), b->tiles.get(), xd, yd, id);
    // the statuses, for osqp_amd_shared_batch_adjoint: a copy of the handle's own, whoever owns the info rows
    OQ_LAUNCH(shared::k_shared_status, dim3(blocks_for((int64_t)b->count, 256)), dim3(256), 0, s, b->count, (const double *)id, b->status.get());
    if (!where) {
      b->x_out.download(x_out, (size_t)b->count * b->n, s);
      if (b->m) b->y_out.download(y_out, (size_t)b->count * b->m, s);
      b->info_out.download(info_out, (size_t)b->count * 6, s);
    }
    HIP_CHECK(hipStreamSynchronize(s));
    b->current = true;
    return 0;
  } OQ_BATCH_CATCH
}

c_int osqp_amd_shared_batch_update_setting(osqp_amd_shared_batch *handle, const char *name, c_float value) {
  SharedBatch *b = shared_handle(handle);
  if (!b) return 1;
  if (!name) { set_last_error("invalid batch data"); return 1; }
  try {
    static const char *const kNames[] = {"max_iter", "eps_abs", "eps_rel", "eps_prim_inf", "eps_dual_inf", "alpha", "check_termination", "scaled_termination", "rho"};
    bool listed = false;
    for (const char *k : kNames) listed = listed || !strcmp(name, k);
    if (!listed) { set_last_error(std::string(name) + " cannot be updated on a shared batch or is not recognized"); return 1; }
    OSQPSettings st = b->st;
    bool known = false, ok = false;  // known: every listed name is in the table
    parse_setting(name, value, st, known, ok);
    if (!ok) { set_last_error(std::string("invalid value for the setting ") + name); return 1; }
    if (!strcmp(name, "rho")) {  // one re-factorisation; the carried iterates stay, as with osqp_update_rho
      DeviceScope on_dev(b->device);
      hipStream_t s = nullptr;
      st.rho = std::min(std::max(st.rho, (c_float)B_RHO_MIN), (c_float)B_RHO_MAX);
      b->current = false;  // the carried iterates are those of the old rho: a resolve comes first
      try { shared_factor(*b, st, s); }
      catch (...) { shared_factor(*b, b->st, s); throw; }  // the model block of the rho that stays
    }
    b->st = st;
    return 0;
  } OQ_BATCH_CATCH
}

c_int osqp_amd_shared_batch_adjoint_launches(void) { return g_shared_adjoint_launches; }

c_int osqp_amd_shared_batch_adjoint(osqp_amd_shared_batch *handle, c_int ncot, const c_float *dx, const c_float *dy, c_float *dq, c_float *dl,
                                    c_float *du, c_float *dPx, c_float *dAx, c_float *dPx_sum, c_float *dAx_sum, c_float *act_out,
                                    c_float *status_out, c_int where) {
  SharedBatch *b = shared_handle(handle);
  if (!b) return 1;
  if (ncot < 1) { set_last_error("invalid batch data: the adjoint needs ncot >= 1"); return 1; }
  if (!dx && !dy) { set_last_error("invalid batch data: the adjoint needs dx or dy"); return 1; }
  if (!b->current) {
    set_last_error("the shared batch holds no current solution: call osqp_amd_shared_batch_resolve after the last update, warm start or rho update");
    return 1;
  }
  try {
    DeviceScope on_dev(b->device);
    hipStream_t s = nullptr;
    const Pattern &P = b->dp.P;
    const SharedAdjointPlan ap = shared_adjoint_plan(P);  // a refusal comes before anything is allocated or launched
    const int count = b->count;
    const size_t cnt = (size_t)count, nc = (size_t)ncot, ln = cnt * b->n, lm = cnt * b->m, lp = cnt * b->nnzP, la = cnt * b->nnzA;
    if (!lm) { dy = nullptr; dl = du = act_out = nullptr; }
    if (!la) dAx = dAx_sum = nullptr;
    if (!lp) dPx = dPx_sum = nullptr;
    if (!dx && !dy) { set_last_error("invalid batch data: the adjoint needs dx or dy"); return 1; }
    const OutStage o(*b, !where, {dq, dl, du, dPx, dAx, dPx_sum, dAx_sum, act_out, status_out},
                     {nc * ln, nc * lm, nc * lm, nc * lp, nc * la, nc * (size_t)b->nnzP, nc * (size_t)b->nnzA, lm, cnt});
    shared::SharedAdjointArgs a;
    a.model = b->model.get(); a.tiles = b->tiles.get(); a.status_in = b->status.get();
    a.gx = dx ? device_ptr(dx, nc * ln, where, b->in_a, s) : nullptr;
    a.gy = dy ? device_ptr(dy, nc * lm, where, b->in_b, s) : nullptr;
    a.dq = o.dev[0]; a.dl = o.dev[1]; a.du = o.dev[2]; a.act = o.dev[7]; a.status = o.dev[8];
    a.count = count; a.T = b->plan.T; a.ncot = (int)ncot; a.refine = (int)b->st.polish_refine_iter; a.delta = b->st.delta;
    a.scratch = nullptr;
    if (ap.large) {
      const size_t need = (size_t)ap.blocks * b->n * b->n;
      if (b->adj_factor.n < need) b->adj_factor.alloc(need);
      a.scratch = b->adj_factor.get();
    }
    // a sum whose rows the caller does not take: the rows of one launch go to the handle's scratch, `chunk` instances (a multiple
    // of 16, or all of them) at a time, and are added to the running sum in the order of the contract
    const bool psum = dPx_sum && !dPx, asum = dAx_sum && !dAx;
    const size_t per_inst = nc * ((psum ? (size_t)b->nnzP : 0) + (asum ? (size_t)b->nnzA : 0));
    int chunk = count;
    if (per_inst) {
      const size_t fit = std::max<size_t>(shared::kSumBlock, (kSharedRowScratch / sizeof(double) / per_inst) & ~(size_t)(shared::kSumBlock - 1));
      if (fit < cnt) chunk = (int)fit;
      if (ap.large && chunk < count && chunk > ap.blocks) chunk -= chunk % ap.blocks;  // whole rounds of the W workgroups: no short last round per chunk
      if (b->adj_rows.n < per_inst * chunk) { HIP_CHECK(hipStreamSynchronize(s)); b->adj_rows.alloc(per_inst * chunk); }
    }
    g_shared_adjoint_launches++;
    for (int first = 0; first < count; first += chunk) {
      const int now = std::min(chunk, count - first);
      double *const rowsP = psum ? b->adj_rows.get() : nullptr;
      double *const rowsA = asum ? b->adj_rows.get() + (psum ? nc * (size_t)now * b->nnzP : 0) : nullptr;
      a.first = first; a.cnt = now;
      a.dPx = psum ? rowsP : o.dev[3]; a.pcount = psum ? now : count; a.pfirst = psum ? first : 0;
      a.dAx = asum ? rowsA : o.dev[4]; a.acount = asum ? now : count; a.afirst = asum ? first : 0;
      launch_shared_adjoint(*b, ap, a, s);
      if (psum) launch_shared_reduce((int)ncot, now, now, b->nnzP, first > 0, rowsP, o.dev[5], s);
      if (asum) launch_shared_reduce((int)ncot, now, now, b->nnzA, first > 0, rowsA, o.dev[6], s);
    }
    if (dPx_sum && dPx) launch_shared_reduce((int)ncot, count, count, b->nnzP, false, o.dev[3], o.dev[5], s);
    if (dAx_sum && dAx) launch_shared_reduce((int)ncot, count, count, b->nnzA, false, o.dev[4], o.dev[6], s);
    o.download(s);
    HIP_CHECK(hipStreamSynchronize(s));
    return 0;
  } OQ_BATCH_CATCH
}

c_int osqp_amd_shared_batch_jvp_launches(void) { return g_shared_jvp_launches; }

c_int osqp_amd_shared_batch_jvp(osqp_amd_shared_batch *handle, c_int ndir, const c_float *tq, const c_float *tl, const c_float *tu,
                                const c_float *tPx, const c_float *tAx, c_float *tx_out, c_float *ty_out, c_float *act_out, c_float *status_out,
                                c_int where) {
  SharedBatch *b = shared_handle(handle);
  if (!b) return 1;
  if (ndir < 1) { set_last_error("invalid batch data: the sensitivities need ndir >= 1"); return 1; }
  const size_t cnt = (size_t)b->count, nd = (size_t)ndir, ln = cnt * b->n, lm = cnt * b->m;
  if (!lm) { tl = tu = nullptr; ty_out = act_out = nullptr; }  // arrays of width 0 are dropped first
  if (!b->nnzA) tAx = nullptr;
  if (!b->nnzP) tPx = nullptr;
  if (!tq && !tl && !tu && !tPx && !tAx) { set_last_error("invalid batch data: the sensitivities need a tangent"); return 1; }
  if (!tx_out && !ty_out) { set_last_error("invalid batch data: the sensitivities need tx_out or ty_out"); return 1; }
  if (!b->current) {
    set_last_error("the shared batch holds no current solution: call osqp_amd_shared_batch_resolve after the last update, warm start or rho update");
    return 1;
  }
  try {
    DeviceScope on_dev(b->device);
    hipStream_t s = nullptr;
    const Pattern &P = b->dp.P;
    const SharedAdjointPlan ap = shared_adjoint_plan(P);  // a refusal comes before anything is allocated or launched
    const OutStage o(*b, !where, {tx_out, ty_out, act_out, status_out}, {nd * ln, nd * lm, lm, cnt});
    shared::SharedJvpArgs a;
    a.model = b->model.get(); a.tiles = b->tiles.get(); a.status_in = b->status.get();
    a.tq = tq ? device_ptr(tq, nd * ln, where, b->in_a, s) : nullptr;
    a.tl = tl ? device_ptr(tl, nd * lm, where, b->in_b, s) : nullptr;
    a.tu = tu ? device_ptr(tu, nd * lm, where, b->in_c, s) : nullptr;
    a.tPx = tPx ? device_ptr(tPx, nd * b->nnzP, where, b->in_d, s) : nullptr;  // one row per direction: shared by the instances
    a.tAx = tAx ? device_ptr(tAx, nd * b->nnzA, where, b->in_e, s) : nullptr;
    a.tx = o.dev[0]; a.ty = o.dev[1]; a.act = o.dev[2]; a.status = o.dev[3];
    a.count = b->count; a.first = 0; a.cnt = b->count; a.T = b->plan.T; a.ndir = (int)ndir;
    a.refine = (int)b->st.polish_refine_iter; a.delta = b->st.delta;
    a.scratch = nullptr;
    if (ap.large) {  // the factor blocks of the adjoint: allocated by whichever call comes first
      const size_t need = (size_t)ap.blocks * b->n * b->n;
      if (b->adj_factor.n < need) b->adj_factor.alloc(need);
      a.scratch = b->adj_factor.get();
    }
    g_shared_jvp_launches++;
    launch_shared_jvp(*b, ap, a, s);
    o.download(s);
    HIP_CHECK(hipStreamSynchronize(s));
    return 0;
  } OQ_BATCH_CATCH
}

c_int osqp_amd_shared_batch_device_bytes(osqp_amd_shared_batch *handle) {
  SharedBatch *b = shared_handle(handle);
  return b ? (c_int)b->device_bytes() : -1;
}

c_int osqp_amd_shared_batch_destroy(osqp_amd_shared_batch *handle) {
  if (!handle) return 0;
  SharedBatch *b = (SharedBatch *)handle;
  try { DeviceScope on_device(b->device); delete b; } catch (...) { return 1; }
  return 0;
}

}  // extern "C"
