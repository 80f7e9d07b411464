// batch_common.hpp -- what the two kernels of the batched small-QP path (batch_quad.hpp: one QP per four wavefronts;
// batch_solve.hpp: one QP per 512 threads), their host scheduling (batch_sched.hpp) and the launcher (batch.hip) share:
// the device view of the shared pattern, the LDS pointer types and the small device helpers, the layout of the state
// record of resident mode, the shape of the MPC family, the argument block of a batched launch (BatchIO) and THE table of
// the instantiations of the four-wavefront kernel (OQ_QUAD_ENTRIES).
// One translation unit (batch.hip) includes these headers: everything is in oq::{anonymous}, as it was in that file.
#pragma once
#include "engine.hpp"

namespace oq {
namespace {

#define B_RHO_MIN 1e-6
#define B_RHO_MAX 1e6
#define B_MIN_SCALING 1e-4
#define B_MAX_SCALING 1e4
#define B_INF (OSQP_INFTY * B_MIN_SCALING)

struct Pattern {        // shared by all instances; device pointers
  int n, m, nnzA, nnzP, nnzF;
  const int *Ap, *Ai;               // A, CSC
  const int *Rp, *Rc, *Rmap;        // A, CSR; Rmap -> position in the CSC value array
  const int *Fp, *Fc, *Fmap;        // full symmetric P, CSR; Fmap -> position in the triu(P) value array
  // structure of A' diag(rho) A (lower triangle), pre-computed once for the shared pattern: non-zero pair t is
  // entry (Ti[t], Tj[t]) = sum over terms q in [Tp[t], Tp[t+1]) of rho[Tr[q]] * Av[Ta[q]] * Av[Tb[q]]
  int npair;
  const int *Tp;
  const unsigned short *Ti, *Tj, *Tr, *Ta, *Tb;
  int max_col, max_row;             // longest column / row of A
};

// LDS pointers carry their address space in the type: a plain `double *` into LDS is a 64-bit generic pointer whose
// accesses compile to flat_load / flat_store (the slow path into LDS, and two registers per pointer) -- with these
// every access is a ds_read / ds_write on a 32-bit offset.
typedef __attribute__((address_space(3))) double ldouble;
typedef __attribute__((address_space(3))) unsigned short lshort;
typedef __attribute__((address_space(3))) int lint;
typedef __attribute__((address_space(3))) char lchar;
typedef __attribute__((address_space(3))) unsigned luint;
typedef unsigned uint4_t __attribute__((ext_vector_type(4)));
typedef unsigned uint2_t __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) uint4_t luint4;
typedef __attribute__((address_space(3))) uint2_t luint2;

__device__ __forceinline__ double nmax(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double lim(double v) { v = v < B_MIN_SCALING ? 1.0 : v; return v > B_MAX_SCALING ? B_MAX_SCALING : v; }

// a value every lane holds identically, moved to scalar registers (the compiler cannot see that an LDS broadcast is uniform)
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double uni(double v) {
  union { double d; int i[2]; } u;
  u.d = v;
  u.i[0] = __builtin_amdgcn_readfirstlane(u.i[0]);
  u.i[1] = __builtin_amdgcn_readfirstlane(u.i[1]);
  return u.d;
}

// Hides where a (wave-uniform) pointer comes from: address arithmetic on it cannot be hoisted out of the enclosing loop.
// The rarely taken phases of the ADMM loop (factorisation, residual evaluation) would otherwise park dozens of
// precomputed addresses in registers -- or spill them -- across the iterations that never use them.
template <typename T>
__device__ __forceinline__ T *opaque(T *p) {
  asm volatile("" : "+s"(p));
  return p;
}
// The same for per-thread values: the thread id as a value the optimiser cannot trace (every use site gets its own copy, so
// nothing derived from it -- row ids, LDS addresses, predicates -- is a loop invariant worth keeping).
__device__ __forceinline__ int mytid() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

// lane `lane` (a compile-time constant) of v, as a wave-uniform value: two v_readlane into scalar registers.  A vector of up
// to 64 doubles that every lane of a wavefront needs (a pivot row, a right-hand side) is read from LDS ONCE -- lane l takes
// element l -- and handed round this way: no vector registers, no further LDS traffic.
__device__ __forceinline__ double lane_bcast(double v, int lane) {
  union { double d; int i[2]; } a;
  a.d = v;
  a.i[0] = __builtin_amdgcn_readlane(a.i[0], lane);
  a.i[1] = __builtin_amdgcn_readlane(a.i[1], lane);
  return a.d;
}

// v of the lane whose id differs in bit 0 (kXor = 1) or bit 1 (kXor = 2): a DPP quad permutation on the two halves -- a
// plain VALU move, where __shfl_xor goes through the LDS crossbar (ds_bpermute) and its queue
template <int kXor>
__device__ __forceinline__ double quad_xor(double v) {
  constexpr int ctrl = kXor == 1 ? 0xB1 : 0x4E;  // quad_perm [1,0,3,2] / [2,3,0,1]
  union { double d; int i[2]; } a;
  a.d = v;
  a.i[0] = __builtin_amdgcn_mov_dpp(a.i[0], ctrl, 0xF, 0xF, true);
  a.i[1] = __builtin_amdgcn_mov_dpp(a.i[1], ctrl, 0xF, 0xF, true);
  return a.d;
}

// a wave-uniform double the optimiser cannot see through: what is derived from it (1 - alpha ...) is recomputed where it is
// used instead of being kept in -- or spilled from -- a register across the ADMM loop
__device__ __forceinline__ double opaque_s(double v) {
  asm volatile("" : "+s"(v));
  return v;
}

// the nrm[] block both kernels keep in LDS: the 14 norms (Slot order of the large-problem path), then these.  N_RECORD: the
// four-wavefront kernel only (the 512-thread kernel uses 18 .. 23 as scratch), and so are N_XPX, N_QX (the two sums of the
// objective, kept for the gap test)
enum { N_PRI = 14, N_DUA = 15, N_OBJ = 16, N_STATUS = 17, N_RECORD = 18, N_XPX = 19, N_QX = 20, N_COUNT = 24 };
extern __shared__ __attribute__((aligned(16))) double lds_raw[];

// ---------------------------------------------------------------------------------------------------------
// Resident mode (osqp_amd_batch_setup ... _resolve): the state of an instance that outlives a launch, one contiguous row
// of doubles per instance in HBM (an even number of them: every row starts on a 16-byte boundary):
//   [ c | rho | flag | - | D[n] | x[n] | E[m] | z[m] | y[m] ]       x, z, y: the SCALED iterate; caller's numbering
// flag: 1 the factors are valid, 3 a solve has left its iterate.  The handle keeps the caller's RAW data; a solve applies
// D, E, c in one pass of its prologue.  res_mode is a kernel argument, uniform over the grid: 0 = the one-shot entry
// points (nothing of this is touched), otherwise bits:
//   RES_SCALE_ONLY  run the Ruiz passes on the raw data, write D, E, c to the record, return (setup, matrix updates);
//   RES_SOLVE       load D, E, c, rho and apply them instead of the Ruiz passes; leave x, z, y (zeros when the instance has
//                   no solution, as the oracle cold-starts it) and rho behind at the end;
//   RES_WARM        (with RES_SOLVE) start from the record's x, z, y instead of zero;
//   RES_CERT        (with RES_SOLVE; osqp_amd_batch_resolve only) an instance that ends primal infeasible leaves the scaled,
//                   projected delta_y in the y slot of its record instead of zeros, one that ends dual infeasible the scaled
//                   delta_x in the x slot: k_batch_cert (batch_cert.hpp), launched next on the same stream, turns them into
//                   the certificates and puts the zeros back.  No kernel argument and nothing before or inside the ADMM loop
//                   of k_batch_quad / k_batch_quad2: their epilogue tests the bit of res_mode itself, which the compiler
//                   loads again from the kernel arguments there, so a launch without the bit runs the code it ran before up
//                   to the store.  In k_batch_solve, whose certificate store is a call that takes everything from LDS, the
//                   bit travels in bit 0 of the parked record pointer (records are 16-byte aligned).
//   RES_GAP         (with RES_SOLVE; the resolves of a handle with osqp_amd_batch_duality_gap_check on) the duality gap is a
//                   third termination test, evaluated where both residual tests hold: cold code of the
//                   residual evaluation, nothing in the ADMM loop proper.  It travels as RES_CERT does: k_batch_quad /
//                   k_batch_quad2 test the bit of res_mode itself on that branch and in the epilogue, k_batch_solve finds it in
//                   bit 1 of the parked record pointer.  The epilogue leaves the number of checks the gap alone refused in
//                   header slot REC_GAPREF of the record (the `-` above); without the bit the slot keeps its zero
//                   (k_batch_solve does not write it, the four-wavefront kernels write the zero they counted).
// ---------------------------------------------------------------------------------------------------------
enum { RES_SOLVE = 1, RES_WARM = 2, RES_SCALE_ONLY = 4, RES_CERT = 8, RES_GAP = 16 };
enum { REC_C = 0, REC_RHO = 1, REC_FLAG = 2, REC_GAPREF = 3, REC_HDR = 4 };
__host__ __device__ constexpr int rec_D(int, int) { return REC_HDR; }
__host__ __device__ constexpr int rec_x(int n, int) { return REC_HDR + n; }
__host__ __device__ constexpr int rec_E(int n, int) { return REC_HDR + 2 * n; }
__host__ __device__ constexpr int rec_z(int n, int m) { return REC_HDR + 2 * n + m; }
__host__ __device__ constexpr int rec_y(int n, int m) { return REC_HDR + 2 * n + 2 * m; }
__host__ __device__ constexpr int rec_doubles(int n, int m) { return (REC_HDR + 2 * n + 3 * m + 1) & ~1; }
// a pointer parked in LDS by the prologue, back as a wave-uniform value; k_batch_solve parks RES_CERT in bit 0 and RES_GAP
// in bit 1 (park_rec)
typedef __attribute__((address_space(3))) unsigned long long lu64;
__device__ __forceinline__ unsigned long long park_rec(const double *rec, int res_mode) {
  return (res_mode & RES_SOLVE) ? ((unsigned long long)rec | ((res_mode & RES_CERT) ? 1ull : 0ull) | ((res_mode & RES_GAP) ? 2ull : 0ull)) : 0ull;
}
__device__ __forceinline__ double *parked_ptr(unsigned long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return (double *)(((unsigned long long)hi << 32) | (lo & ~7u));
}
__device__ __forceinline__ bool parked_cert(unsigned long long v) { return (__builtin_amdgcn_readfirstlane((int)(unsigned)v) & 1) != 0; }
__device__ __forceinline__ bool parked_gap(unsigned long long v) { return (__builtin_amdgcn_readfirstlane((int)(unsigned)v) & 2) != 0; }
__host__ __device__ inline bool status_prim_inf(int s) { return s == OSQP_PRIMAL_INFEASIBLE || s == OSQP_PRIMAL_INFEASIBLE_INACCURATE; }
__host__ __device__ inline bool status_dual_inf(int s) { return s == OSQP_DUAL_INFEASIBLE || s == OSQP_DUAL_INFEASIBLE_INACCURATE; }

// ---- the duality gap: THE statement of a row's support term and of the third termination test, shared
// by the reading kernel (batch_gap.hpp) and the stopping rule inside k_batch_quad / k_batch_solve -------------------------------
// u max(y, 0) + l min(y, 0) of one row, y projected onto the polar of the recession cone of [l, u]: a bound is infinite when
// the SCALED bound (l_s, u_s: the bound times the row's factor E) passes B_INF, and then adds 0.  l, u, y in one system of
// units, the caller's or the scaled one (there l_s = l, u_s = u).
__device__ __forceinline__ double support_term(double l, double u, double y, double l_s, double u_s) {
  const double up = u_s > B_INF ? 0.0 : u * fmax(y, 0.0);
  const double lo = l_s < -B_INF ? 0.0 : l * fmin(y, 0.0);
  return up + lo;
}
// |gap| < eps_abs + eps_rel max(|x'Px|, |q'x|, |SC|) on the scaled sums, k = 1 / c when the tests are in the caller's units
// (the scaled sums are c times the caller's), 1 otherwise; a NaN fails
__device__ __forceinline__ bool gap_test(double sxpx, double sqx, double ssc, double k, double ea, double er) {
  const double xpx = k * sxpx, qx = k * sqx, sc = k * ssc;
  const double gap = xpx + qx + sc;
  return fabs(gap) < ea + er * fmax(fabs(xpx), fmax(fabs(qx), fabs(sc)));
}

// the shape of the MPC family (BASELINE.json config 5; the generator is mpc_fill in batch.hip): both kernels have an
// instantiation with it compiled in
constexpr int NX = 6, NU = 4, TT = 10, NS = NX + NU, MPC_N = NS * TT, MPC_M = NX * TT + MPC_N + NU * TT;
__host__ __device__ constexpr int mpc_nnzA() {
  int c = 0;
  for (int t = 0; t < TT; t++) c += NX * (2 + (t + 1 < TT ? NX : 0)) + NU * (NX + 2 + (t + 1 < TT ? 1 : 0));
  return c;
}
constexpr int kMpcNnzA = mpc_nnzA();

// The argument block of a batched launch: the instances' data (nnzP / nnzA / n / m / m doubles per instance), where row i
// of x / y / info goes (x + i * x_stride etc.: packed layouts put all three in one row; info_cols 4 or 6), and for resident
// mode the state records.  sel (resident handles only): the workgroup at position p of the launch serves instance sel[p] --
// its data and its record -- and writes row p of x / y / info; nullptr: position = instance.  launch_batch takes it; its
// callers fill it by name.
struct BatchIO {
  const double *Px = nullptr, *Ax = nullptr, *q = nullptr, *l = nullptr, *u = nullptr;
  double *x = nullptr, *y = nullptr, *info = nullptr;
  int x_stride = 0, y_stride = 0, info_stride = 0, info_cols = 0;
  double *rec = nullptr;
  int rec_stride = 0, res_mode = 0;
  const int *sel = nullptr;
};

// ---- the instantiations of the four-wavefront kernel: stated HERE and nowhere else -----------------------------------------
// X(number, NH, KC, KE, CH, FIXED, KERNEL): quadrant size NH (n <= 2 NH), compile-time bounds KC / KE of the longest column /
// row of A, CH rows per assembly window; FIXED = 1: the shape of the MPC family is compiled in (every LDS offset an
// immediate; the others take the shape at run time); KERNEL: the occupancy wrapper -- k_batch_quad three QPs per compute
// unit, k_batch_quad2 two (batch_quad.hpp).  The NUMBER is public (osqp_amd_batch_last_kernel, OSQP_AMD_BATCH_QUAD_CFG,
// tests, committed profiles) and never changes; the ORDER of the rows is the order a pattern tries them in, it takes the
// first it fits: the MPC sizes with short columns / rows look at entry 10, whose LDS layout still holds THREE QPs per
// compute unit (bounds 12 / 12: 53 KB; 16 / 16 is 59 KB, two per unit), before entry 4.  The host table below, the
// schedule's loop over entries (batch_sched.hpp) and the launch dispatch (launch_batch) are generated from this list: an
// instantiation is added by adding a row.
#define OQ_QUAD_ENTRIES(X)              \
  X(0, 50, 9, 11, 16, 1, k_batch_quad)   \
  X(1, 16, 16, 16, 16, 0, k_batch_quad)  \
  X(2, 32, 16, 16, 16, 0, k_batch_quad)  \
  X(3, 48, 16, 16, 16, 0, k_batch_quad)  \
  X(10, 50, 12, 12, 16, 0, k_batch_quad) \
  X(4, 50, 16, 16, 16, 0, k_batch_quad)  \
  X(5, 64, 16, 16, 16, 0, k_batch_quad2) \
  X(6, 16, 32, 32, 16, 0, k_batch_quad)  \
  X(7, 32, 32, 32, 16, 0, k_batch_quad)  \
  X(8, 48, 32, 32, 16, 0, k_batch_quad2) \
  X(9, 64, 32, 32, 16, 0, k_batch_quad2)
struct QuadEntry { int number, NH, KC, KE, CH; bool fixed; };
#define OQ_QUAD_ROW(NUMBER, NH, KC, KE, CH, FIXED, KERNEL) {NUMBER, NH, KC, KE, CH, FIXED != 0},
constexpr QuadEntry kQuadEntries[] = {OQ_QUAD_ENTRIES(OQ_QUAD_ROW)};  // in try order
#undef OQ_QUAD_ROW
constexpr const QuadEntry *quad_entry(int number) {
  for (const QuadEntry &e : kQuadEntries) if (e.number == number) return &e;
  return nullptr;
}
// The half bandwidth of M that a FIXED entry compiles into the first phase of its sweeps (the MPC family: two stages): its
// steps skip the registers a pivot cannot reach, so the host leaves the phase out when a pattern's reach is larger.
constexpr int kQuadFixedBW = 19;

}  // namespace
}  // namespace oq
