// direct_knobs.hpp -- every environment switch of the direct KKT back-end, one line each, read when a DirectKnobs is constructed:
// an LdlFactor and a Direct hold one as a const member, abi.hip's symbolic probe reads the same table.  Host only.  DESIGN.md section 9.
#pragma once
#include <algorithm>
#include "common.hpp"

namespace oq {

constexpr int kChainRows = 512;   // levels at most this wide are chained in one workgroup
constexpr int kDenseSparseMax = 1024, kDenseMin = 32;  // the dense top block (symbolic.hpp, choose_dense_top)
constexpr int kSnMax = 64, kSnThreads = 256;
constexpr int kSnWaveLevel = 16384;  // supernodes in a level from which each gets a wavefront instead of a workgroup (below: the device is not full either way and a workgroup finishes its supernode sooner)
constexpr int kMfMaxFront = 192;     // rows of the largest front that fits one workgroup's LDS (mfront.hpp)
constexpr int64_t kMfShareMin = 16384;  // doubles from which an update matrix is placed by its lifetime (place_update_matrices)

struct DirectKnobs {
  int first_ordering = env_int("OSQP_AMD_FIRST_ORDERING", -1);  // 1: nested dissection at once, 0: min-degree first; unset (-1): by the depth of the KKT graph
  int nd_depth = env_int("OSQP_AMD_ND_DEPTH", 100);             // breadth-first levels from which a large KKT graph counts as long
  int lean = env_int("OSQP_AMD_LEAN", -1);                      // 0 never, 1 whenever the row map is the identity (tests); unset (-1): where the dissection goes first
  bool device_maps = env_on("OSQP_AMD_DEVICE_MAPS");            // 0: the scatter maps of the whole KKT system built on the host
  bool nd = env_on("OSQP_AMD_ND");                              // 0: no second analysis with nested dissection on a deep level schedule
  bool md_fifo = env_on("OSQP_AMD_MD_FIFO");                    // 0: no third analysis with the tie-breaking variant of min-degree
  bool dense_top = env_on("OSQP_AMD_DENSE_TOP");                // 0: never
  int dense_max = env_int("OSQP_AMD_DENSE_MAX", 12288);         // largest block in pivots
  double dense_probe_tol = env_double("OSQP_AMD_DENSE_PROBE_TOL", 1e-6);  // residual of the probe of the inverse above which the factor is rebuilt without the block
  bool schur_dense = env_on("OSQP_AMD_SCHUR_DENSE");            // 0: the Schur complement of a blocked inverse entry by entry instead of by rank-64 updates
  bool dense_sym = env_on("OSQP_AMD_DENSE_SYM");                // 0: the product with a blocked inverse over the full array instead of its lower triangle
  double long_row_mean = env_double("OSQP_AMD_LONG_ROW_MEAN", 24.0);  // mean row length from which a level is factorised through work rows
  bool gj_pivot_lds = env_int("OSQP_AMD_GJ_PIVOT_LDS", 0) == 1; // 1: the round-5 pivot kernel (A/B, test)
  bool gj_fuse = env_on("OSQP_AMD_GJ_FUSE");                    // 0: the pivot block a launch of its own
  bool gj_sparse = env_on("OSQP_AMD_GJ_SPARSE");                // 0: full sweeps (A/B, test)
  int snode = env_int("OSQP_AMD_SNODE", 1);                     // 0 never, 2 always (tests), otherwise by the model
  int snode_max = std::max(1, std::min(kSnMax, env_int("OSQP_AMD_SNODE_MAX", kSnMax)));  // smaller supernodes (tests: many levels on small problems)
  bool snode_flat = env_on("OSQP_AMD_SNODE_FLAT");              // 0: the entries outside the blocks row by row instead of flat (k_sn_level_f / _wf)
  int snode_fold = env_int("OSQP_AMD_SNODE_FOLD", 1);           // 0: the blocks left as packed triangles; 2: folded in the wavefront-form levels only
  bool snode_single = env_on("OSQP_AMD_SNODE_SINGLE");          // 0: single pivots through the quarter-wavefront kernel
  int snode_wave_min = env_int("OSQP_AMD_SNODE_WAVE_MIN", kSnWaveLevel);  // (tests) supernodes in a level from which the wavefront / quarter-wavefront form is used
  bool snode_tree = env_on("OSQP_AMD_SNODE_TREE");              // 0: one launch per level instead of one per direction
  int snode_tree_per_cu = [] { int v = 0; return env_read("OSQP_AMD_SNODE_TREE_PER_CU", v) ? std::max(1, v) : 0; }();  // (experiments) resident workgroups per compute unit instead of the occupancy query; unset: 0
  int snode_tree_oversub = std::max(1, env_int("OSQP_AMD_SNODE_TREE_OVERSUB", 2));  // device-fuls the one-launch tree may hold where fronts go through global memory; 1: all resident
  int snode_tree_512 = [] { int v = 0; return env_read("OSQP_AMD_SNODE_TREE_512", v) ? (v != 0 ? 1 : 0) : -1; }(); // 0 / 1: never / always try 512 threads per supernode; unset: where no front goes through global memory
  long long snode_tree_cap = env_i64("OSQP_AMD_SNODE_TREE_CAP", (long long)(~0ULL >> 1));  // (experiments: a later start) upper bound of the 512-thread launch
  int snode_tree_persist = env_int("OSQP_AMD_SNODE_TREE_PERSIST", 0);  // persistent workgroups from this level on (0: never)
  int snode_top = env_int("OSQP_AMD_SNODE_TOP", -1);            // 0: rows gathered entry by entry everywhere (A/B runs); 1: front vectors under a dense top too (tests)
  bool snode_fault_test = env_int("OSQP_AMD_SNODE_FAULT_TEST", 0) == 1;  // (tests) the first health check of the factor reports a timed-out wait
  int mf = env_int("OSQP_AMD_MF", 1);                           // 0: the numeric factorisation level by level
  int mf_max_front = std::min(kMfMaxFront, std::max(1, env_int("OSQP_AMD_MF_MAX_FRONT", kMfMaxFront)));  // tests: smaller fronts through the global-memory kernels too
  bool mf_big = env_on("OSQP_AMD_MF_BIG");                      // 0: the round-5 behaviour (A/B runs)
  bool mf_big_ancestors = env_on("OSQP_AMD_MF_BIG_ANCESTORS");  // 0: the ancestors of a front beyond LDS stay in LDS
  bool mf_share_u = env_on("OSQP_AMD_MF_SHARE_U");              // 0: every update matrix a place of its own (A/B, tests)
  int64_t mf_share_min = std::max(1, env_int("OSQP_AMD_MF_SHARE_MIN", (int)kMfShareMin));  // (tests: small problems)
  int mf_wide = env_int("OSQP_AMD_MF_WIDE", 1);                 // 0: the round-5 rule of threads per front (A/B)
  bool mfb_split = env_on("OSQP_AMD_MFB_SPLIT");                // 0: one workgroup per big front (A/B, tests)
  int sn_dense = env_int("OSQP_AMD_SN_DENSE", 1);               // 0 never, 2 whenever a level fits (tests: small problems)
  int sn_dense_max = 4300;                                      // pivots of the dense top over the supernodes ...
  bool sn_dense_max_set = env_read("OSQP_AMD_SN_DENSE_MAX", sn_dense_max);  // ... asked for explicitly: no chain levels are added
  bool sn_dense_order = env_on("OSQP_AMD_SN_DENSE_ORDER");      // 0: its pivots in slot order instead of the postorder of their tree
  bool fuse_ends = env_on("OSQP_AMD_FUSE_ENDS");                // 0: the six-kernel iteration
  bool fuse2 = env_on("OSQP_AMD_FUSE2");                        // 0: no two-launch iteration on two-level factors
  bool leave_rhs = env_on("OSQP_AMD_DIRECT_LEAVE_RHS");         // 0: a right-hand-side launch of its own in every iteration of a chunk graph
  bool setup_trace = env_int("OSQP_AMD_SETUP_TRACE", 0) == 1;   // 1: the [supernodes] / [fronts] lines of a setup on stderr
};

}  // namespace oq
