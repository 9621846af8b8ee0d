// pair_roles.h — which role a block of the paired launch k_dfs_pure_seed (graph_kernel.h) plays.  Shared by the
// kernel and by a CPU test (tests/host/pair_roles.cpp), so: no HIP type, nothing but integers.
//
// The grid holds n_dfs walk blocks and n_pure pure-chain blocks of one batch and n_seed seed blocks of the next.  The
// walk blocks come first (the long walks start at once), then
//   seeds_first != 0 (the default): the seed blocks, then the pure-chain blocks.  The walk's first round leaves about
//     a quarter of the device's wave slots free; they go to whatever comes next in the grid, and the seed blocks — the
//     role that is bound by the memory system, which idles under the walk — make more of them than the pure-chain
//     blocks, which wait for their own few dependent loads.  The launch then ends in the short pure-chain blocks.
//   seeds_first == 0 (round 7's order): the pure-chain blocks, then the seed blocks.
// Every block index below n_dfs + n_pure + n_seed maps to exactly one (role, index); the ones beyond to NONE.
// (Seed blocks BETWEEN the walk blocks — 1, 2 or 3 behind each — delay walk blocks and lost: DESIGN.md section 5,
// round 8.)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KM_PAIR_HD __host__ __device__
#else
#define KM_PAIR_HD
#endif

enum PairRole : uint32_t { PAIR_WALK = 0, PAIR_PURE = 1, PAIR_SEED = 2, PAIR_NONE = 3 };
struct PairBlock { uint32_t role, index; };

// (the caller keeps n_dfs + n_pure + n_seed below 2^32: the launch's grid)
KM_PAIR_HD inline PairBlock pair_block(uint32_t j, uint32_t n_dfs, uint32_t n_pure, uint32_t n_seed, uint32_t seeds_first) {
  if (j < n_dfs) return PairBlock{PAIR_WALK, j};
  j -= n_dfs;
  const uint32_t n_a = seeds_first ? n_seed : n_pure, n_b = seeds_first ? n_pure : n_seed;
  const uint32_t role_a = seeds_first ? PAIR_SEED : PAIR_PURE, role_b = seeds_first ? PAIR_PURE : PAIR_SEED;
  if (j < n_a) return PairBlock{role_a, j};
  j -= n_a;
  if (j < n_b) return PairBlock{role_b, j};
  return PairBlock{PAIR_NONE, 0};
}
