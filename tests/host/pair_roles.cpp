// pair_roles.cpp — km_amd/csrc/pair_roles.h on the CPU (built with AddressSanitizer + UBSan by
// tests/test_pair_roles_cpu.py): the block -> (role, index) map of the paired launch k_dfs_pure_seed must be a
// bijection from [0, n_dfs + n_pure + n_seed) onto the three index ranges, in either order of the seed and the
// pure-chain blocks, and NONE beyond.
//   * every small (n_dfs, n_pure, n_seed): each block marks its (role, index); every mark is set exactly once, the
//     walk blocks come first and in order (dfs_body's block 0 hands over by index, not by blockIdx), and the other two
//     roles follow in the order asked for;
//   * large grids up to the launch's limit of 2^31 - 1 blocks and up to 2^32 - 1 (the arithmetic is 32-bit): the ends of
//     every region and a few thousand random blocks go through an inverse map written here, independently, and back.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../km_amd/csrc/pair_roles.h"

namespace {
void die(const char* what, uint64_t a, uint64_t b, uint64_t c, uint64_t d, uint64_t j) {
  fprintf(stderr, "pair_roles: %s (n_dfs %llu, n_pure %llu, n_seed %llu, seeds_first %llu, block %llu)\n", what,
          (unsigned long long)a, (unsigned long long)b, (unsigned long long)c, (unsigned long long)d, (unsigned long long)j);
  exit(2);
}

// The inverse, from the description alone: where does (role, index) sit in the grid?
uint64_t block_of(uint32_t role, uint64_t index, uint64_t n_dfs, uint64_t n_pure, uint64_t n_seed, bool seeds_first) {
  if (role == PAIR_WALK) return index;
  if (role == PAIR_SEED) return n_dfs + (seeds_first ? 0 : n_pure) + index;
  return n_dfs + (seeds_first ? n_seed : 0) + index;
}

uint64_t count_of(uint32_t role, uint64_t n_dfs, uint64_t n_pure, uint64_t n_seed) {
  return role == PAIR_WALK ? n_dfs : role == PAIR_PURE ? n_pure : n_seed;
}

void there_and_back(uint64_t j, uint32_t n_dfs, uint32_t n_pure, uint32_t n_seed, uint32_t first) {
  const uint64_t total = (uint64_t)n_dfs + n_pure + n_seed;
  const PairBlock r = pair_block((uint32_t)j, n_dfs, n_pure, n_seed, first);
  if (j >= total) {
    if (r.role != PAIR_NONE) die("a block beyond the grid has a role", n_dfs, n_pure, n_seed, first, j);
    return;
  }
  if (r.role > PAIR_SEED) die("no role", n_dfs, n_pure, n_seed, first, j);
  if (r.index >= count_of(r.role, n_dfs, n_pure, n_seed)) die("index out of range", n_dfs, n_pure, n_seed, first, j);
  if (block_of(r.role, r.index, n_dfs, n_pure, n_seed, first != 0) != j) die("not the inverse's block", n_dfs, n_pure, n_seed, first, j);
}

void back_and_there(uint32_t role, uint64_t index, uint32_t n_dfs, uint32_t n_pure, uint32_t n_seed, uint32_t first) {
  const uint64_t j = block_of(role, index, n_dfs, n_pure, n_seed, first != 0);
  if (j >= (uint64_t)n_dfs + n_pure + n_seed) die("the inverse leaves the grid", n_dfs, n_pure, n_seed, first, j);
  const PairBlock r = pair_block((uint32_t)j, n_dfs, n_pure, n_seed, first);
  if (r.role != role || r.index != index) die("an index nobody gets", n_dfs, n_pure, n_seed, first, j);
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
}  // namespace

int main() {
  // ---- every small grid, exhaustively
  uint64_t small = 0;
  for (uint32_t n_dfs = 0; n_dfs <= 9; ++n_dfs)
    for (uint32_t n_pure = 0; n_pure <= 9; ++n_pure)
      for (uint32_t n_seed = 0; n_seed <= 9; ++n_seed)
        for (uint32_t first : {0u, 1u, 7u}) {
          const uint32_t total = n_dfs + n_pure + n_seed;
          std::vector<int> walk(n_dfs, 0), pure(n_pure, 0), seed(n_seed, 0);
          uint32_t last_role = PAIR_WALK;
          for (uint32_t j = 0; j < total + 3; ++j) {
            const PairBlock r = pair_block(j, n_dfs, n_pure, n_seed, first);
            if (j >= total) {
              if (r.role != PAIR_NONE) die("a block beyond the grid has a role", n_dfs, n_pure, n_seed, first, j);
              continue;
            }
            std::vector<int>* marks = r.role == PAIR_WALK ? &walk : r.role == PAIR_PURE ? &pure : r.role == PAIR_SEED ? &seed : nullptr;
            if (!marks) die("no role", n_dfs, n_pure, n_seed, first, j);
            if (++marks->at(r.index) != 1) die("an index given twice", n_dfs, n_pure, n_seed, first, j);   // (.at: range-checked)
            if ((j < n_dfs) != (r.role == PAIR_WALK) || (j < n_dfs && r.index != j))
              die("the walk blocks are not the first ones, in order", n_dfs, n_pure, n_seed, first, j);
            // behind the walk blocks: one role, then the other, the seeds first when asked for
            if (r.role != last_role) {
              const bool ok = last_role == PAIR_WALK ? (r.role == (first ? PAIR_SEED : PAIR_PURE) || (first ? n_seed : n_pure) == 0)
                                                     : r.role == (first ? PAIR_PURE : PAIR_SEED);
              if (!ok) die("roles out of order", n_dfs, n_pure, n_seed, first, j);
              last_role = r.role;
            }
            there_and_back(j, n_dfs, n_pure, n_seed, first);
          }
          for (const auto* m : {&walk, &pure, &seed})
            for (int v : *m) if (v != 1) die("an index nobody gets", n_dfs, n_pure, n_seed, first, 0);
          ++small;
        }

  // ---- large grids: the launch's limit (2^31 - 1 blocks) and the arithmetic's (2^32 - 1)
  const uint32_t M31 = 0x7FFFFFFFu, M32 = 0xFFFFFFFFu;
  const uint32_t large[][3] = {
      {2949, 10000, 20000},          {64, 10000, 8},                     {10000, 10000, 80000},
      {M31 - 2, 1, 1},               {1, M31 - 2, 1},                    {1, 1, M31 - 2},
      {M31 / 2, 0, M31 - M31 / 2},   {M31 / 4, M31 / 4, M31 - 2 * (M31 / 4)},   {1000, M31 - 4000, 3000},
      {M32 / 2, 0, M32 - M32 / 2},   {M32 / 4, 3, M32 - M32 / 4 - 3},    {M32 - 2, 1, 1},
      {3, M32 - 10, 7},              {M32 / 5, M32 / 5, M32 - 2 * (M32 / 5)},   {0, 0, M32},   {0, M32, 0},
  };
  for (const auto& c : large)
    for (uint32_t first : {0u, 1u}) {
      const uint32_t n_dfs = c[0], n_pure = c[1], n_seed = c[2];
      const uint64_t total = (uint64_t)n_dfs + n_pure + n_seed;
      if (total > M32) die("a case of this program beyond 32 bits", n_dfs, n_pure, n_seed, first, 0);
      const uint64_t edges[] = {0, n_dfs, (uint64_t)n_dfs + (first ? n_seed : n_pure), total};
      for (const uint64_t e : edges)
        for (int d = -3; d <= 3; ++d) {
          const uint64_t j = e + (uint64_t)(int64_t)d;
          if (j <= M32) there_and_back(j, n_dfs, n_pure, n_seed, first);      // (e + d below 0 wraps beyond 2^32: skipped)
        }
      for (int i = 0; i < 4000; ++i) {
        there_and_back(rnd() % total, n_dfs, n_pure, n_seed, first);
        for (uint32_t role = PAIR_WALK; role <= PAIR_SEED; ++role) {
          const uint64_t n = count_of(role, n_dfs, n_pure, n_seed);
          if (!n) continue;
          back_and_there(role, i == 0 ? 0 : i == 1 ? n - 1 : rnd() % n, n_dfs, n_pure, n_seed, first);
        }
      }
    }
  printf("PAIR ROLES OK %llu small grids, %zu large\n", (unsigned long long)small, 2 * (sizeof large / sizeof large[0]));
  return 0;
}
