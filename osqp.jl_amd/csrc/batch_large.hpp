// batch_large.hpp -- k_batch_solve_large: the batched kernel for instances with 128 < n <= 256 (opt-in: osqp_amd_batch_large,
// DESIGN.md section 13.1).  ONE QP PER 512-THREAD WORKGROUP, ONE WORKGROUP PER COMPUTE UNIT.  The phases, their order and
// their formulas are those of k_batch_solve (batch_solve.hpp), whose generic device functions it calls: the Ruiz passes, the
// rows_dot walks over the LDS copy of the pattern, set_rho, assemble_scratch, residual_phase, leave_certificate.  What differs
// is the home of the inverse of the reduced KKT matrix M = P + sigma I + A' diag(rho) A:
//   - k_batch_solve keeps M^-1 in registers, thread 4 row + part of 512: that is where n <= 128 comes from;
//   - here M^-1 STAYS IN THE INSTANCE'S n x n SCRATCH in global memory (column-major, symmetric, both triangles -- where
//     assemble_scratch builds M and invert_mfma inverts it anyway) and x~ = M^-1 b reads it every iteration: 8 n^2 bytes per
//     instance and iteration (512 KB at n = 256), served by the caches, not by registers.  That is several times slower per
//     iteration than the register kernels, which is why a caller has to ask for this path.
// Inversion: the block sweeps of invert_mfma with pivot-row buffers of 4 x 256 (kLargeW) and up to 17 tiles per wavefront (136
// lower 16 x 16 tiles over 8 wavefronts at n = 256: 136 accumulator registers per lane).  The kernel asks for two wavefronts per
// SIMD -- its eight wavefronts and nothing else, the LDS of an instance does not leave room for a second workgroup anyway --
// which gives every lane 256 registers of the unified file; the accumulators stay in registers through all sweeps.
// LDS: the layout of k_batch_solve (carve) with the wider pivot buffers, without the packed words (sparse_fits needs 4 n <= 512).
#pragma once
#include "batch_solve.hpp"

namespace oq {
namespace {

constexpr int kLargeW = 256;    // pivot-row width of the inversion = the largest n of this kernel
constexpr int kLargeMaxN = 256;
// tiles on and below the diagonal of a 16 x 16 tiling, dealt round-robin to the NW wavefronts
__host__ __device__ constexpr int large_tiles_per_wave(int n) { return (((n + 15) / 16) * ((n + 15) / 16 + 1) / 2 + NW - 1) / NW; }
constexpr int kLargeTpwSmall = 10, kLargeNSmall = 192;  // n <= 192: 12 tile blocks, 78 tiles, 10 per wavefront
static_assert(large_tiles_per_wave(kLargeNSmall) == kLargeTpwSmall && large_tiles_per_wave(kLargeMaxN) == 17, "the two instantiations of the inversion");
__host__ __device__ inline size_t large_lds_bytes(int n, int m, int nnzA, int nnzF) { return lds_bytes(n, m, nnzA, nnzF, false, kLargeW); }

// The inversion, by n: 10 or 17 accumulator tiles per wavefront.  false: a pivot block was not positive definite (OSQP_NON_CVX).
__device__ __forceinline__ bool invert_large(int n, double *scratch, ldouble *cb) {
  return n <= kLargeNSmall ? invert_mfma<kLargeTpwSmall, kLargeW>(n, scratch, cb) : invert_mfma<large_tiles_per_wave(kLargeMaxN), kLargeW>(n, scratch, cb);
}

// x~ = M^-1 b with M^-1 in the instance's scratch and b in s.bb.  Wavefront w serves the 64 rows 64 (w & 3) + lane and the
// column half w >> 2 ([0, ceil(n / 2)) or the rest): the 64 lanes of a wavefront read 64 consecutive doubles of one column, one
// contiguous 512-byte load, and b[j] is one LDS broadcast.  A thread adds its columns in index order into four sums (column
// offset mod 4) and closes them as (a0 + a1) + (a2 + a3); the row is (half 0) + (half 1): a fixed split and a fixed order,
// the same bits in every solve.  Returns the thread's partial sum; half 1 also leaves it in `part` (n doubles of LDS).
__device__ __forceinline__ double apply_large_partial(int n, const double *scratch, const ldouble *bb, ldouble *part) {
  scratch = opaque(scratch);
  const int t = mytid(), w = t >> 6, row = 64 * (w & 3) + (t & 63), half = w >> 2;
  const int nh = (n + 1) >> 1, j0 = half * nh, j1 = half ? n : nh;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (row < n) {
    // VISIBILITY of a new inverse (after the first factorisation and after every rho update).  These are plain vector loads
    // (global_load_dwordx2, a per-lane address: never a scalar load, whose cache the stores below do not reach; not marked
    // invariant or non-temporal: the kernel writes the array).  The values were written by the last loop of invert_mfma --
    // vector stores of the eight wavefronts of THIS workgroup, which all run on one compute unit and go through its one
    // write-through vector cache: a store updates the line it hits there on its way to L2, so no line of the old inverse
    // survives in the only vector cache these loads look into.  Between those stores and these loads stands the
    // __syncthreads() that ends invert_mfma: a workgroup-scope release (s_waitcnt vmcnt(0): every store of the wavefront has
    // been acknowledged), the s_barrier, and a workgroup-scope acquire (no load of this function is issued early).  Nothing
    // outside the workgroup ever writes the instance's scratch during a launch.
    const double *src = scratch + row + (size_t)j0 * n;
    const ldouble *bp = bb + j0;
    const int len = j1 - j0;
    int j = 0;
    for (; j + 8 <= len; j += 8) {  // eight loads in flight, then eight multiply-adds (column offset mod 4 picks the sum)
      double v[8], b[8];
#pragma unroll
      for (int u = 0; u < 8; u++) v[u] = src[(size_t)(j + u) * n];
#pragma unroll
      for (int u = 0; u < 8; u++) b[u] = bp[j + u];
      a0 = __builtin_fma(v[0], b[0], a0); a1 = __builtin_fma(v[1], b[1], a1); a2 = __builtin_fma(v[2], b[2], a2); a3 = __builtin_fma(v[3], b[3], a3);
      a0 = __builtin_fma(v[4], b[4], a0); a1 = __builtin_fma(v[5], b[5], a1); a2 = __builtin_fma(v[6], b[6], a2); a3 = __builtin_fma(v[7], b[7], a3);
    }
    for (; j < len; j++) {  // at most seven: j is a multiple of 8 here, so j & 3 is the column offset mod 4
      const double v = src[(size_t)j * n], b = bp[j];
      if ((j & 3) == 0) a0 = __builtin_fma(v, b, a0);
      else if ((j & 3) == 1) a1 = __builtin_fma(v, b, a1);
      else if ((j & 3) == 2) a2 = __builtin_fma(v, b, a2);
      else a3 = __builtin_fma(v, b, a3);
    }
  }
  const double a = (a0 + a1) + (a2 + a3);
  if (half && row < n) part[row] = a;
  return a;
}
// the second step, after a barrier: the thread of half 0 closes its row and updates x on the spot, as apply_tile does
__device__ __forceinline__ void apply_large_finish(int n, double a, const Lds &s, const ldouble *part, double alpha, const ldouble *xp, ldouble *x) {
  const int t = mytid(), w = t >> 6, row = 64 * (w & 3) + (t & 63);
  if ((w >> 2) == 0 && row < n) {
    a += part[row];
    const double xo = xp[row];
    s.xt[row] = a;
    const double xn = alpha * a + (1.0 - alpha) * xo;
    x[row] = xn;
    s.dx[row] = xn - xo;
  }
}

// The argument list of k_batch_solve.  Two wavefronts per SIMD: 256 registers per lane (the 17 accumulator tiles of the
// inversion are 136 of them).
template <bool SEL>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_batch_solve_large(
    Pattern Pin, OSQPSettings st, int count, double *__restrict__ scratch_all, const double *__restrict__ Px_all, const double *__restrict__ Ax_all,
    const double *__restrict__ q_all, const double *__restrict__ l_all, const double *__restrict__ u_all, double *__restrict__ x_out,
    double *__restrict__ y_out, double *__restrict__ info_out, int x_stride, int y_stride, int info_stride, int info_cols,
    double *__restrict__ rec_all, int rec_stride, int res_mode, const int *__restrict__ sel) {
  constexpr int GW = kLargeW;
  const int pos = blockIdx.x;
  if (pos >= count) return;
  const int inst = SEL ? uni(sel[pos]) : pos;
  const bool res_solve = (res_mode & RES_SOLVE) != 0, res_warm = (res_mode & RES_WARM) != 0;
  double *const rec = res_mode ? rec_all + (size_t)inst * rec_stride : nullptr;  // the instance's state record (resident mode)
  const Pattern P = Pin;
  const int n = P.n, m = P.m, tid = mytid();
  Lds s = carve<GW>((ldouble *)lds_raw, P, false);
  // ---- stage the shared pattern (16-bit) and load the instance -----------------
  for (int k = tid; k <= n; k += NT) { s.Ap[k] = (unsigned short)P.Ap[k]; s.Fp[k] = (unsigned short)P.Fp[k]; }
  for (int k = tid; k <= m; k += NT) s.Rp[k] = (unsigned short)P.Rp[k];
  for (int k = tid; k < P.nnzA; k += NT) { s.Ai[k] = (unsigned short)P.Ai[k]; s.Rc[k] = (unsigned short)P.Rc[k]; s.Rmap[k] = (unsigned short)P.Rmap[k]; }
  for (int k = tid; k < P.nnzF; k += NT) s.Fc[k] = (unsigned short)P.Fc[k];
  for (int k = tid; k < P.nnzA; k += NT) s.Av[k] = Ax_all[(size_t)inst * P.nnzA + k];
  if (tid == 0) s.Av[P.nnzA] = 0.0;
  for (int k = tid; k < P.nnzF; k += NT) s.Pv[k] = Px_all[(size_t)inst * P.nnzP + P.Fmap[k]];
  for (int j = tid; j < n; j += NT) {
    const double x0 = res_warm ? rec[rec_x(n, m) + j] : 0.0;  // the scaled iterate the last solve left (or warm_start wrote)
    s.q[j] = q_all[(size_t)inst * n + j]; s.D[j] = res_solve ? rec[rec_D(n, m) + j] : 1.0; s.x[j] = x0; s.xp[j] = x0; s.dx[j] = 0.0;
  }
  for (int i = tid; i < m; i += NT) {
    s.l[i] = fmax(l_all[(size_t)inst * m + i], -OSQP_INFTY); s.u[i] = fmin(u_all[(size_t)inst * m + i], OSQP_INFTY);
    const double z0 = res_warm ? rec[rec_z(n, m) + i] : 0.0;
    s.E[i] = res_solve ? rec[rec_E(n, m) + i] : 1.0; s.z[i] = z0; s.y[i] = res_warm ? rec[rec_y(n, m) + i] : 0.0; s.zp[i] = z0; s.dy[i] = 0.0;
  }
  // the record pointer with its RES_CERT / RES_GAP bits, the refusal count and a defined status code, parked where
  // residual_phase and leave_certificate look for them: behind the pivot buffers of THIS layout
  if (tid == 0) { *(lu64 *)(s.gjc + gjc_parked(GW)) = park_rec(rec, res_mode); s.gjc[gjc_parked(GW) + 1] = 0.0; s.nrm[N_STATUS] = 0.0; }
  __syncthreads();
  // ---- K0: Ruiz equilibration + cost scaling (the walks of k_batch_solve without the packed words) ----------------
  double c = 1.0;
  const int nscale = res_solve ? 0 : (int)st.scaling;  // a resident solve applies the factors of its record instead (below)
  for (int it = 0; it < nscale; it++) {
    for (int j = tid; j < n; j += NT) {
      double mx = 0.0;
      for (int q = s.Fp[j]; q < s.Fp[j + 1]; q++) mx = fmax(mx, fabs(s.Pv[q]));
      for (int k = s.Ap[j]; k < s.Ap[j + 1]; k++) mx = fmax(mx, fabs(s.Av[k]));
      s.tn[j] = 1.0 / sqrt(lim(mx));
    }
    for (int i = tid; i < m; i += NT) {
      double mx = 0.0;
      for (int q = s.Rp[i]; q < s.Rp[i + 1]; q++) mx = fmax(mx, fabs(s.Av[s.Rmap[q]]));
      s.tm[i] = 1.0 / sqrt(lim(mx));
    }
    __syncthreads();
    for (int r = tid; r < n; r += NT)
      for (int q = s.Fp[r]; q < s.Fp[r + 1]; q++) {
        int cc = s.Fc[q];
        int lo = cc < r ? cc : r, hi = cc < r ? r : cc;
        s.Pv[q] = (s.Pv[q] * s.tn[lo]) * s.tn[hi];
      }
    for (int j = tid; j < n; j += NT) {
      for (int k = s.Ap[j]; k < s.Ap[j + 1]; k++) s.Av[k] = (s.Av[k] * s.tm[s.Ai[k]]) * s.tn[j];
      s.q[j] *= s.tn[j];
      s.D[j] *= s.tn[j];
    }
    for (int i = tid; i < m; i += NT) s.E[i] *= s.tm[i];
    __syncthreads();
    double v[2] = {0.0, 0.0}, w[1] = {0.0};
    for (int j = tid; j < n; j += NT) {
      double mx = 0.0;
      for (int q = s.Fp[j]; q < s.Fp[j + 1]; q++) mx = fmax(mx, fabs(s.Pv[q]));
      w[0] += mx;
      v[0] = fmax(v[0], fabs(s.q[j]));
    }
    {  // the sum and the maximum in one exchange, as in k_batch_solve
      double sm = w[0], mq = v[0];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { sm += __shfl_xor(sm, o, 64); mq = nmax(mq, __shfl_xor(mq, o, 64)); }
      ldouble *rr = s.red + 8 * NW + (it & 1) * 2 * NW;
      if ((tid & 63) == 0) { rr[2 * (tid >> 6)] = sm; rr[2 * (tid >> 6) + 1] = mq; }
      __syncthreads();
      sm = rr[0]; mq = rr[1];
#pragma unroll
      for (int wv = 1; wv < NW; wv++) { sm += rr[2 * wv]; mq = nmax(mq, rr[2 * wv + 1]); }
      w[0] = sm; v[0] = mq;
    }
    double c_temp = w[0] / (double)n;
    c_temp = lim(fmax(c_temp, lim(v[0])));
    c_temp = 1.0 / c_temp;
    for (int k = tid; k < P.nnzF; k += NT) s.Pv[k] *= c_temp;
    for (int j = tid; j < n; j += NT) s.q[j] *= c_temp;
    c *= c_temp;
    __syncthreads();
  }
  if (res_mode & RES_SCALE_ONLY) {  // setup / after a matrix update: D, E, c of this data into the record, no solve
    for (int j = tid; j < n; j += NT) rec[rec_D(n, m) + j] = s.D[j];
    for (int i = tid; i < m; i += NT) rec[rec_E(n, m) + i] = s.E[i];
    if (tid == 0) { rec[REC_C] = c; rec[REC_FLAG] = 1.0; }
    return;
  }
  if (res_solve) {  // the stored factors in one pass over the raw data: P <- c D P D, A <- E A D, q <- c D q
    c = uni(rec[REC_C]);
    for (int r = tid; r < n; r += NT)
      for (int q = s.Fp[r]; q < s.Fp[r + 1]; q++) {
        const int cc = s.Fc[q];
        const int lo = cc < r ? cc : r, hi = cc < r ? r : cc;
        s.Pv[q] = c * ((s.Pv[q] * s.D[lo]) * s.D[hi]);
      }
    for (int j = tid; j < n; j += NT) {
      for (int k = s.Ap[j]; k < s.Ap[j + 1]; k++) s.Av[k] = (s.Av[k] * s.E[s.Ai[k]]) * s.D[j];
      s.q[j] = c * (s.q[j] * s.D[j]);
    }
    __syncthreads();
  }
  const double cinv = 1.0 / c;
  for (int i = tid; i < m; i += NT) { s.l[i] *= s.E[i]; s.u[i] *= s.E[i]; }
  __syncthreads();
  // ---- K1, K2 (a resident solve goes on with the rho its last solve ended on) ---
  double rho = uni(fmin(fmax(res_solve ? rec[REC_RHO] : st.rho, B_RHO_MIN), B_RHO_MAX));
  set_rho(P, s, rho, true);
  int status = OSQP_UNSOLVED;
  double *scratch = scratch_all + (size_t)(SEL ? (int)blockIdx.x : inst) * n * n;
  auto a_rows = [&](const ldouble *v, auto pre, auto finish) {
    rows_dot<2>(m, s.Rp, [&](int q) { return s.Av[s.Rmap[q]] * v[s.Rc[q]]; }, [&](int r, double a) { finish(r, a, pre(r)); });
  };
  auto a_cols = [&](const ldouble *v, auto pre, auto finish) {
    rows_dot<4>(n, s.Ap, [&](int k) { return s.Av[k] * v[s.Ai[k]]; }, [&](int r, double a) { finish(r, a, pre(r)); });
  };
  const bool uns = st.scaling && !st.scaled_termination;
  const int check = (int)st.check_termination;
  const int rho_interval = st.adaptive_rho ? (st.adaptive_rho_interval ? (int)st.adaptive_rho_interval : 100) : 0;
  const double alpha = st.alpha, sigma = st.sigma;
  double pri_res = 0.0, dua_res = 0.0, obj = 0.0;
  ldouble *nrm = s.nrm;
  int iter = 0, rho_updates = 0;
  ldouble *x = s.x, *xp = s.xp, *z = s.z, *zp = s.zp;
  // ---- ADMM loop --------------------------------------------------------------
  const int max_iter = (int)st.max_iter;
  bool need_factor = true;
  for (int i = tid; i < m; i += NT) s.zt[i] = s.rho[i] * z[i] - s.y[i];
  __syncthreads();
  for (iter = 1; iter <= max_iter; iter++) {
    if (need_factor) {  // first iteration and after every rho update: M into the scratch, M^-1 in its place
      assemble_scratch(P, s, st.sigma, scratch);
      const bool pd = invert_large(n, scratch, s.gjc);
      if (!pd) { status = OSQP_NON_CVX; iter--; break; }
      need_factor = false;
    }
    { ldouble *t = x; x = xp; xp = t; t = z; z = zp; zp = t; }
    // b = sigma x_prev - q + A'(rho z_prev - y); s.zt = rho z_prev - y was left behind by the previous z / y update
    a_cols(s.zt, [&](int j) { return Ops2{xp[j], s.q[j]}; }, [&](int j, double a, const Ops2 &o) { s.bb[j] = sigma * o.a - o.b + a; });
    __syncthreads();
    // x~ = M^-1 b out of the scratch (s.tn is free between two residual phases: the partial sums of column half 1)
    const double part = apply_large_partial(n, scratch, s.bb, s.tn);
    __syncthreads();
    apply_large_finish(n, part, s, s.tn, opaque_s(alpha), xp, x);
    __syncthreads();
    // z~ = A x~ row by row, each row finished on the spot: z, y, delta_y and s.zt = rho z - y for the next right-hand side
    a_rows(s.xt, [&](int i) { return Ops6{zp[i], s.y[i], s.rhoi[i], s.l[i], s.u[i], s.rho[i]}; },
           [&](int i, double zt, const Ops6 &o) {
      const double al = opaque_s(alpha);
      const double zh = al * zt + (1.0 - al) * o.a;
      const double yo = o.b;
      const double zn = fmin(fmax(zh + o.c * yo, o.d), o.e);
      z[i] = zn;
      const double d = o.f * (zh - zn);
      s.dy[i] = d; s.y[i] = yo + d;
      s.zt[i] = o.f * zn - (yo + d);
    });
    __syncthreads();
    const bool last = iter == max_iter;
    const bool due = check && (iter % check == 0);
    const bool rho_due = rho_interval && (iter % rho_interval == 0);
    if (!(due || rho_due || last)) continue;
    // ---- residual evaluation (K8) and termination tests: the function of k_batch_solve on this kernel's layout ----
    {
      CheckArgs ca;
      ca.n = n; ca.m = m; ca.nnzA = P.nnzA; ca.nnzF = P.nnzF;
      ca.swapped = (x != s.x); ca.uns = uns; ca.words = 0; ca.passes = (due || last) ? (last ? 2 : 1) : 0; ca.last = last;
      ca.ea = st.eps_abs; ca.er = st.eps_rel; ca.epi = st.eps_prim_inf; ca.edi = st.eps_dual_inf; ca.c = c; ca.cinv = cinv;
      residual_phase<0, 0, 0, 0, GW>(ca);
    }
    bool done = false;
    {
      const int code = (int)nrm[N_STATUS];
      if (code != 0) { status = code; done = true; }
      pri_res = uni(nrm[N_PRI]); dua_res = uni(nrm[N_DUA]); obj = uni(nrm[N_OBJ]);
    }
    if (done) break;
    // ---- adaptive rho ----
    if (rho_due) {
      double pr = m == 0 ? 0.0 : nrm[0] / (nmax(nrm[2], nrm[3]) + 1e-10);
      double du = nrm[6] / (nmax(nmax(nrm[8], nrm[9]), nrm[10]) + 1e-10);
      double est = uni(fmin(fmax(rho * sqrt(pr / (du + 1e-10)), B_RHO_MIN), B_RHO_MAX));
      if (est > rho * st.adaptive_rho_tolerance || est < rho / st.adaptive_rho_tolerance) {
        rho = est; rho_updates++;
        set_rho(P, s, rho, false);
        for (int i = mytid(); i < m; i += NT) s.zt[i] = s.rho[i] * z[i] - s.y[i];  // the carried vector follows rho
        __syncthreads();
        need_factor = true;  // picked up at the top of the next iteration: the scratch is rebuilt and re-inverted there
      }
    }
  }
  if (iter > max_iter) iter = max_iter;
  // ---- store -----------------------------------------------------
  const bool has_sol = status == OSQP_SOLVED || status == OSQP_SOLVED_INACCURATE || status == OSQP_MAX_ITER_REACHED;
  const int row = SEL ? (int)blockIdx.x : inst;
  for (int j = tid; j < n; j += NT) x_out[(size_t)row * x_stride + j] = has_sol ? s.D[j] * x[j] : NAN;
  for (int i = tid; i < m; i += NT) y_out[(size_t)row * y_stride + i] = has_sol ? cinv * s.E[i] * s.y[i] : NAN;
  if (tid == 0) {
    double *o = info_out + (size_t)row * info_stride;
    o[0] = (double)iter; o[1] = (double)status; o[2] = pri_res; o[3] = dua_res;
    if (info_cols > 4) { o[4] = status == OSQP_NON_CVX ? NAN : obj; o[5] = (double)rho_updates; }
  }
  const unsigned long long parked = *(const lu64 *)(s.gjc + gjc_parked(GW));
  if (double *const rec = parked_ptr(parked)) {  // the scaled iterate and rho stay: the next solve starts from them
    for (int j = tid; j < n; j += NT) rec[rec_x(n, m) + j] = has_sol ? x[j] : 0.0;
    for (int i = tid; i < m; i += NT) { rec[rec_z(n, m) + i] = has_sol ? z[i] : 0.0; rec[rec_y(n, m) + i] = has_sol ? s.y[i] : 0.0; }
    if (tid == 0) { rec[REC_RHO] = rho; rec[REC_FLAG] = 3.0; }
    if (parked_gap(parked) && tid == 0) rec[REC_GAPREF] = s.gjc[gjc_parked(GW) + 1];  // the checks the gap alone refused
  }
  leave_certificate<0, 0, 0, 0, GW>(n, m, P.nnzA, P.nnzF, 0);
}

}  // namespace
}  // namespace oq
