// batch_sched.hpp -- host side of the batched small-QP path: the analysis of the shared sparsity pattern and the schedule of
// the four-wavefront kernel (batch_quad.hpp) for it.  Included by batch.hip; nothing here runs on the device.
#pragma once
#include <algorithm>
#include <vector>

#include "batch_quad.hpp"

namespace oq {
namespace {

// what the batched path derives on the host from the CSC patterns of P (upper triangle) and A
struct HostPattern {
  int n, m, nnzA, nnzP, nnzF;
  std::vector<int> Ap, Ai;          // A, CSC (the caller's)
  std::vector<int> rp, rc, rmap;    // A, CSR; rmap -> position in the CSC value array
  std::vector<int> fp, fc, fmap;    // full symmetric P, CSR, rows sorted by column; fmap -> position in the triu(P) value array
  std::vector<int> tp;              // term lists of A' diag(rho) A (Pattern::Tp .. Tb)
  std::vector<unsigned short> ti, tj, tr, ta, tb;
  int max_col = 0, max_row = 0;     // longest column / row of A
  bool mpc;                         // the MPC family of BASELINE.json config 5: both kernels have its shape compiled in
  // for the schedule of the four-wavefront kernel, whichever entry is tried: the pair of A' rho A / the entry of P at a
  // position of M (-1: none), and the rows by length, longest first (stable): lane L holds row order[L], so the long rows
  // share wavefronts
  std::vector<std::vector<int>> pair_of, pent0;
  std::vector<int> order;

  HostPattern(int n_, int m_, const std::vector<int> &Pp, const std::vector<int> &Pi, std::vector<int> Ap_, std::vector<int> Ai_)
      : n(n_), m(m_), nnzA(Ap_[n_]), nnzP(Pp[n_]), Ap(std::move(Ap_)), Ai(std::move(Ai_)), rp(m_ + 1, 0), rc(nnzA), rmap(nnzA), fp(n_ + 1, 0), tp(1, 0) {
    for (int k = 0; k < nnzA; k++) rp[Ai[k] + 1]++;
    for (int i = 0; i < m; i++) rp[i + 1] += rp[i];
    std::vector<int> f(rp.begin(), rp.end() - 1);
    for (int j = 0; j < n; j++)
      for (int k = Ap[j]; k < Ap[j + 1]; k++) { int q = f[Ai[k]]++; rc[q] = j; rmap[q] = k; }
    std::vector<std::vector<std::pair<int, int>>> rows(n);
    for (int j = 0; j < n; j++)
      for (int k = Pp[j]; k < Pp[j + 1]; k++) {
        int i = Pi[k];
        if (i > j) throw Error(1, "P is not upper triangular");
        rows[j].push_back({i, k});
        if (i != j) rows[i].push_back({j, k});
      }
    for (int r = 0; r < n; r++) {
      std::sort(rows[r].begin(), rows[r].end());
      for (auto &e : rows[r]) { fc.push_back(e.first); fmap.push_back(e.second); }
      fp[r + 1] = (int)fc.size();
    }
    nnzF = (int)fc.size();
    // term lists of A' rho A: rows of A give the products, grouped by (i >= j) pair in ascending row order
    // (the order of the sparse dot product of columns i and j, so the sums are the ones the merge would form)
    for (int i = 0; i < n; i++)
      for (int j = 0; j <= i; j++) {
        int a = Ap[i], ae = Ap[i + 1], b = Ap[j], be = Ap[j + 1], cnt = 0;
        while (a < ae && b < be) {
          if (Ai[a] == Ai[b]) { tr.push_back((unsigned short)Ai[a]); ta.push_back((unsigned short)a); tb.push_back((unsigned short)b); cnt++; a++; b++; }
          else if (Ai[a] < Ai[b]) a++; else b++;
        }
        if (cnt) { ti.push_back((unsigned short)i); tj.push_back((unsigned short)j); tp.push_back((int)tr.size()); }
      }
    for (int j = 0; j < n; j++) max_col = std::max(max_col, Ap[j + 1] - Ap[j]);
    for (int i = 0; i < m; i++) max_row = std::max(max_row, rp[i + 1] - rp[i]);
    mpc = n == MPC_N && m == MPC_M && nnzA == kMpcNnzA && nnzF == MPC_N;
    pair_of.assign(n, std::vector<int>(n, -1)); pent0 = pair_of;
    for (size_t t = 0; t < ti.size(); t++) { pair_of[ti[t]][tj[t]] = (int)t; pair_of[tj[t]][ti[t]] = (int)t; }
    for (int r = 0; r < n; r++) for (int q = fp[r]; q < fp[r + 1]; q++) pent0[r][fc[q]] = q;
    order.resize(m);
    for (int i = 0; i < m; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return rp[a + 1] - rp[a] > rp[b + 1] - rp[b]; });
  }
};

template <typename T>
void upload_vec(DevBuf<T> &d, const std::vector<T> &h, hipStream_t s) { d.alloc(h.size()); d.upload(h.data(), h.size(), s); }

// the shared pattern on the device
struct DevicePattern {
  Pattern P;
  bool mpc = false;                 // HostPattern::mpc
  bool large = false;               // n > 128, built while osqp_amd_batch_large was on: launch_batch runs k_batch_solve_large (set by build's caller)
  DevBuf<int> Ap, Ai, Rp, Rc, Rmap, Fp, Fc, Fmap, Tp;
  DevBuf<unsigned short> Ti, Tj, Tr, Ta, Tb;
  mutable DevBuf<double> scratch;  // [instances x n x n]: where a workgroup assembles its reduced KKT matrix (launch_batch sizes it)
  // schedule of the four-wavefront kernel (batch_quad.hpp) for the entry `quad` of kQuadEntries: the first whose compile-time
  // bounds the pattern fits (nullptr: none, the pattern runs the 512-thread kernel)
  const QuadEntry *quad = nullptr;
  quad::Sched QS;
  DevBuf<unsigned short> qs_colstart, qs_collist;
  DevBuf<unsigned> qs_roww, qs_meta;
  DevBuf<unsigned long long> qs_stream;
  DevBuf<int> qs_Fp, qs_Fc, qs_Fmap;   // the full symmetric P in the kernel's numbering of the variables
  DevBuf<unsigned short> qs_perm;
  void build(const HostPattern &h, hipStream_t s) {
    upload_vec(Ap, h.Ap, s); upload_vec(Ai, h.Ai, s); upload_vec(Rp, h.rp, s); upload_vec(Rc, h.rc, s); upload_vec(Rmap, h.rmap, s);
    upload_vec(Fp, h.fp, s); upload_vec(Fc, h.fc, s); upload_vec(Fmap, h.fmap, s);
    upload_vec(Tp, h.tp, s); upload_vec(Ti, h.ti, s); upload_vec(Tj, h.tj, s); upload_vec(Tr, h.tr, s); upload_vec(Ta, h.ta, s); upload_vec(Tb, h.tb, s);
    HIP_CHECK(hipStreamSynchronize(s));
    P = Pattern{h.n, h.m, h.nnzA, h.nnzP, h.nnzF, Ap.get(), Ai.get(), Rp.get(), Rc.get(), Rmap.get(), Fp.get(), Fc.get(), Fmap.get(),
                (int)h.ti.size(), Tp.get(), Ti.get(), Tj.get(), Tr.get(), Ta.get(), Tb.get(), h.max_col, h.max_row};
    mpc = h.mpc;
    // a pattern takes the first entry it fits, in the order of the table (round 5: up to round 4 entry 0 was the only one,
    // every other pattern ran the 512-thread kernel with its n x n global scratch)
    quad = nullptr;
    const int only = getenv("OSQP_AMD_BATCH_QUAD_CFG") ? atoi(getenv("OSQP_AMD_BATCH_QUAD_CFG")) : -1;  // experiments: one entry by number
    for (const QuadEntry &cfg : kQuadEntries) {
      if ((only >= 0 && cfg.number != only) || (cfg.fixed && !h.mpc)) continue;
      if (build_quad(h, cfg, s)) { quad = &cfg; break; }
    }
  }

  // the schedule for entry cfg; false: the pattern does not fit it (nothing of the schedule was touched)
  bool build_quad(const HostPattern &h, const QuadEntry &cfg, hipStream_t s) {
    using namespace quad;
    const int n = h.n, m = h.m, nnzA = h.nnzA, nnzF = h.nnzF;
    static const bool trace = getenv("OSQP_AMD_BATCH_TRACE") && atoi(getenv("OSQP_AMD_BATCH_TRACE")) == 1;
    auto refuse = [&](const char *why, int a, int b) {
      if (trace) fprintf(stderr, "[batch] quadrants of %d (columns <= %d, rows <= %d): not taken, %s (%d > %d)\n", cfg.NH, cfg.KC, cfg.KE, why, a, b);
      return false;
    };
    if (n > 2 * cfg.NH) return refuse("n", n, 2 * cfg.NH);
    if (m > QT || m == 0 || nnzA == 0) return refuse("rows", m, QT);
    if (h.max_col > cfg.KC) return refuse("longest column", h.max_col, cfg.KC);
    if (h.max_row > cfg.KE) return refuse("longest row", h.max_row, cfg.KE);
    const Layout L = make_layout(n, m, nnzA, nnzF, cfg.NH, cfg.KC, cfg.KE, cfg.CH);
    // the term words and row words carry 16-bit LDS offsets of values, row records and operands: everything up to the
    // pattern tables (colstart, collist, meta, row words -- addressed with 32-bit arithmetic) must lie below 64 KB
    if (L.colstart > 65535 || (size_t)(nnzA + 1) * 8 > 65535) return refuse("LDS bytes below the pattern tables (16-bit offsets)", L.colstart, 65535);
    if (L.total > 80 * 1024) return refuse("LDS bytes (two QPs per compute unit)", L.total, 80 * 1024);
    const int kch = L.kch, kep = L.kep;
    // ---- the pattern of M = P + sigma I + A' rho A and the kernel's numbering of the variables ---------------------------
    // perm[j]: the caller's index of the kernel's variable j.  Row half 1 is numbered in reverse when that lets the first
    // phase of the sweeps (batch_quad.hpp: two-ended) take pivots from both ends of a banded pattern: the kernel's pivots
    // 0, 1, ... of half 0 stay inside the quadrant (0, 0), its pivots cfg.NH, cfg.NH + 1, ... of half 1 -- the caller's n - 1,
    // n - 2, ... -- inside (1, 1).  Counted by symbolic elimination: a pivot reaches at most what the pivots before it reached.
    auto mnz = [&](int i, int j) { return i == j || h.pair_of[i][j] >= 0 || h.pent0[i][j] >= 0; };
    std::vector<int> perm(n), inv(n);
    int p1_top = 0, p1_bot = 0, bw = 0;
    {
      for (int i = 0; i < n; i++) perm[i] = i < cfg.NH ? i : n - 1 - (i - cfg.NH);
      auto count = [&](int first, int last, int &reach_over) {  // pivots first, first + 1, ... whose reach stays in [.., last]
        int reach = -1, cnt = 0;
        for (int a = first; a <= last; a++) {
          for (int j = last + 1; j < n; j++) if (mnz(perm[a], perm[j])) return cnt;      // (half 0 only: a column of half 1)
          for (int j = 0; j < first; j++) if (mnz(perm[a], perm[j])) return cnt;         // (half 1 only: a column of half 0)
          for (int j = a; j <= last; j++) if (mnz(perm[a], perm[j])) { reach = std::max(reach, j); reach_over = std::max(reach_over, j - a); }
          cnt = a - first + 1;
        }
        return cnt;
      };
      int over = 0;
      p1_top = count(0, std::min(n, cfg.NH) - 1, over);
      if (n > cfg.NH) p1_bot = count(cfg.NH, n - 1, over);
      bw = over;  // the furthest a first-phase pivot reaches beyond itself
      const int nb = (cfg.NH + 15) / 16, cap = nb > 1 ? (nb - 1) * 16 : cfg.NH;  // the kernel compiles the phase for its first nb - 1 pivot blocks
      p1_top = std::min(p1_top, cap); p1_bot = std::min(p1_bot, cap);
      static const bool off = getenv("OSQP_AMD_BATCH_TWO_ENDED") && atoi(getenv("OSQP_AMD_BATCH_TWO_ENDED")) == 0;  // A/B runs
      if (off || p1_top + p1_bot < 8 || (cfg.fixed && bw > kQuadFixedBW)) {  // (a fixed entry compiles the reach in)
        p1_top = p1_bot = 0;
        for (int i = 0; i < n; i++) perm[i] = i;
      }
      for (int i = 0; i < n; i++) inv[perm[i]] = i;
      if (trace) fprintf(stderr, "[batch] pattern of M: first-phase pivots %d + %d of %d (reach %d)\n", p1_top, p1_bot, n, bw);
    }
    // the full symmetric P in the kernel's numbering (entries of a row in the caller's order)
    std::vector<int> fp2(n + 1, 0), fc2(nnzF), fmap2(nnzF);
    std::vector<std::vector<int>> pent(n, std::vector<int>(n, -1));
    for (int i = 0, k = 0; i < n; i++) {
      for (int q = h.fp[perm[i]]; q < h.fp[perm[i] + 1]; q++, k++) { fc2[k] = inv[h.fc[q]]; fmap2[k] = h.fmap[q]; pent[i][fc2[k]] = k; }
      fp2[i + 1] = k;
    }
    std::vector<unsigned short> colstart(QT), collist((size_t)QT * kch);
    for (int t = 0; t < QT; t++) {
      const int wv = t >> 6, cbk = wv & 1, hb = wv >> 1, cl = t & 63, jk = cbk * cfg.NH + cl;
      const bool col = cl < cfg.NH && jk < n;
      const int j = col ? perm[jk] : 0;
      colstart[t] = (unsigned short)(col ? h.Ap[j] : nnzA);
      for (int e = 0; e < kch; e++) {
        const bool real = col && h.Ap[j] + 2 * e + hb < h.Ap[j + 1];
        collist[(size_t)t * kch + e] = (unsigned short)((real ? h.Ai[h.Ap[j] + 2 * e + hb] : m) * RECB);
      }
      collist[(size_t)t * kch + kch - 1] = colstart[t];  // the first value of the column rides in the last slot
    }
    std::vector<unsigned> roww((size_t)QT * kep, (unsigned)(nnzA * 8) << 16), meta((size_t)QT, 0xFFFFFFFFu);
    int kew[4] = {0, 0, 0, 0};
    for (int k = 0; k < m; k++) {
      const int row = h.order[k];
      meta[k] = (unsigned)row * RECB;
      kew[k >> 6] = std::max(kew[k >> 6], h.rp[row + 1] - h.rp[row]);
      for (int q = h.rp[row], e = 0; q < h.rp[row + 1]; q++, e++) roww[(size_t)k * kep + e] = ((unsigned)(h.rmap[q] * 8) << 16) | (unsigned)(inv[h.rc[q]] * 16);  // operands: 16 bytes per column
    }
    // terms of M, grouped by position (i, j) of a window (rows k cfg.CH / 2 + r of either row half), the groups of a window
    // dealt to the threads (longest first)
    const int ch2 = cfg.CH / 2, nwin = (cfg.NH + ch2 - 1) / ch2;
    struct Term { unsigned short r, a, b; };
    std::vector<std::vector<std::vector<Term>>> groups(nwin);
    std::vector<std::vector<unsigned short>> targets(nwin);
    {
      for (int i = 0; i < n; i++) {
        const int wh = i / cfg.NH, il = i - wh * cfg.NH, cw = il / ch2, wrow = wh * ch2 + il % ch2;
        for (int j = 0; j < n; j++) {
          std::vector<Term> g;
          const int io = perm[i], jo = perm[j];
          if (h.pair_of[io][jo] >= 0) {
            const int t = h.pair_of[io][jo];
            for (int q = h.tp[t]; q < h.tp[t + 1]; q++)
              g.push_back(Term{(unsigned short)(L.rec + h.tr[q] * RECB + F_RHO), (unsigned short)(L.Av + 8 * h.ta[q]), (unsigned short)(L.Av + 8 * h.tb[q])});
          }
          if (pent[i][j] >= 0) g.push_back(Term{(unsigned short)L.cst, (unsigned short)L.cst, (unsigned short)(L.Pv + 8 * pent[i][j])});
          if (i == j) g.push_back(Term{(unsigned short)L.cst, (unsigned short)L.cst, (unsigned short)(L.cst + 8)});
          if (g.empty()) continue;
          groups[cw].push_back(g);
          targets[cw].push_back((unsigned short)(wrow * n + j));
        }
      }
    }
    std::vector<std::vector<std::vector<int>>> deal(nwin, std::vector<std::vector<int>>(QT));
    int ns = 0;
    for (int cw = 0; cw < nwin; cw++) {
      std::vector<int> idx(groups[cw].size());
      for (size_t g = 0; g < idx.size(); g++) idx[g] = (int)g;
      std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return groups[cw][a].size() > groups[cw][b].size(); });
      std::vector<int> load(QT, 0);
      for (int g : idx) {
        int best = 0;
        for (int t = 1; t < QT; t++) if (load[t] < load[best]) best = t;
        deal[cw][best].push_back(g);
        load[best] += (int)groups[cw][g].size();
      }
      for (int t = 0; t < QT; t++) ns = std::max(ns, load[t]);
    }
    ns = std::max(4, (ns + 3) & ~3);
    if (ns > 64) return refuse("assembly terms per thread and window", ns, 64);  // (the kernel prefetches 12 slots -- its NSM -- and reads further ones in place)
    if (trace) fprintf(stderr, "[batch] quadrants of %d (columns <= %d, rows <= %d): taken, %d bytes of LDS, %d term slots\n", cfg.NH, cfg.KC, cfg.KE, L.total, ns);
    const unsigned long long pad = (unsigned long long)(cfg.CH * n) | 0x8000ull | ((unsigned long long)(L.rec + m * RECB + F_RHO) << 16) |
                                   ((unsigned long long)L.cst << 32) | ((unsigned long long)L.cst << 48);  // 0 * 1 * 1 into the spare position
    std::vector<unsigned long long> stream((size_t)nwin * ns * QT, pad);
    for (int cw = 0; cw < nwin; cw++)
      for (int t = 0; t < QT; t++) {
        int slot = 0;
        for (int g : deal[cw][t]) {
          const auto &G = groups[cw][g];
          for (size_t k = 0; k < G.size(); k++, slot++) {
            unsigned long long w = (unsigned long long)targets[cw][g] | ((unsigned long long)G[k].r << 16) | ((unsigned long long)G[k].a << 32) |
                                   ((unsigned long long)G[k].b << 48);
            if (k + 1 == G.size()) w |= 0x8000ull;
            stream[((size_t)cw * ns + slot) * QT + t] = w;
          }
        }
      }
    const std::vector<unsigned short> perm16(perm.begin(), perm.end());
    upload_vec(qs_colstart, colstart, s); upload_vec(qs_collist, collist, s); upload_vec(qs_roww, roww, s); upload_vec(qs_meta, meta, s);
    upload_vec(qs_stream, stream, s); upload_vec(qs_perm, perm16, s);
    upload_vec(qs_Fp, fp2, s); upload_vec(qs_Fc, fc2, s); upload_vec(qs_Fmap, fmap2, s);
    HIP_CHECK(hipStreamSynchronize(s));
    QS = Sched{n, m, nnzA, h.nnzP, nnzF, {kew[0], kew[1], kew[2], kew[3]}, ns, p1_top, p1_bot, bw, getenv("OSQP_AMD_BATCH_ROT") ? atoi(getenv("OSQP_AMD_BATCH_ROT")) : 0, qs_perm.get(), qs_colstart.get(),
               qs_collist.get(), qs_roww.get(), qs_meta.get(), qs_stream.get(), qs_Fp.get(), qs_Fc.get(), qs_Fmap.get()};
    return true;
  }
};

}  // namespace
}  // namespace oq
