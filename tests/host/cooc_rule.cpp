// cooc_rule.cpp — km_amd/csrc/cooc_rule.h on the CPU (built with AddressSanitizer + UBSan by
// tests/test_compare_cpu.py): the arithmetic of `compare`, with exactly sized arrays, so an index past the pairs, the
// ballots or the bins is an error the sanitizer names.
//   the pair index <-> (i, j) mapping is a bijection onto 0 .. n (n + 1) / 2 - 1 for every n from 1 to 32, and the
//   lanes' pairs (lane + 64 t) cover every pair exactly once within lane_trips(n) <= 9 trips;
//   the trip model (ballots, pairs lane by lane, popcount bins) equals brute force slot by slot over 64 x 32 bit
//   matrices: all zero, all one, a single slot, a single input, random dense, random sparse, bits at or above n set;
//   fold gives the full symmetric matrix, the union, and joins the mask of the key without a slot to every number.
// Prints "COOC RULE OK <cases> cases" and exits 0, or names what failed and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../km_amd/csrc/cooc_rule.h"

namespace {
int failures = 0;
uint64_t cases = 0;
#define CHECK(cond, ...)                                      \
  do {                                                        \
    if (!(cond)) {                                            \
      std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                               \
      std::printf("\n");                                      \
      if (++failures > 20) std::exit(1);                      \
    }                                                         \
  } while (0)

uint64_t rng_state = 0x243F6A8885A308D3ull;
uint64_t next_u64() {                                  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

void check_mapping(uint32_t n) {
  const uint32_t np = kmcooc::n_pairs(n);
  CHECK(np == n * (n + 1) / 2 && np <= kmcooc::MAX_PAIRS, "n=%u", n);
  std::vector<int> seen(np, 0);
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t j = 0; j <= i; ++j) {
      const uint32_t p = kmcooc::pair_index(i, j);
      CHECK(p < np, "n=%u i=%u j=%u p=%u", n, i, j, p);
      if (p >= np) continue;
      ++seen[p];
      const uint32_t ri = kmcooc::pair_row(p);
      CHECK(ri == i && kmcooc::pair_col(p, ri) == j, "n=%u p=%u -> (%u, %u), want (%u, %u)", n, p, ri, kmcooc::pair_col(p, ri), i, j);
    }
  for (uint32_t p = 0; p < np; ++p) CHECK(seen[p] == 1, "n=%u p=%u named %d times", n, p, seen[p]);
  // the lanes' share
  const uint32_t trips = kmcooc::lane_trips(n);
  CHECK(trips <= kmcooc::PAIRS_PER_LANE && trips * kmcooc::WAVE >= np && (trips == 0 || (trips - 1) * kmcooc::WAVE < np), "n=%u", n);
  std::vector<int> dealt(np, 0);
  for (uint32_t lane = 0; lane < kmcooc::WAVE; ++lane)
    for (uint32_t t = 0; t < trips; ++t) {
      const uint32_t p = kmcooc::lane_pair(lane, t);
      if (p < np) ++dealt[p];
    }
  for (uint32_t p = 0; p < np; ++p) CHECK(dealt[p] == 1, "n=%u p=%u dealt %d times", n, p, dealt[p]);
  ++cases;
}

// 64 masks against brute force, accumulated over `rounds` trips into the same sums
void check_trips(uint32_t n, const std::vector<std::vector<uint32_t>>& trips, const char* what) {
  const uint32_t np = kmcooc::n_pairs(n);
  std::vector<uint64_t> pairs(np, 0), exact(n + 1, 0), priv(n, 0);
  std::vector<uint64_t> want_pairs(np, 0), want_exact(n + 1, 0), want_priv(n, 0);
  for (const auto& masks : trips) {
    kmcooc::trip_model(masks.data(), n, pairs.data(), exact.data(), priv.data());
    for (uint32_t s = 0; s < kmcooc::WAVE; ++s) {
      uint32_t held = 0, last = 0;
      for (uint32_t i = 0; i < n; ++i)
        if ((masks[s] >> i) & 1u) {
          ++held;
          last = i;
          for (uint32_t j = 0; j <= i; ++j)
            if ((masks[s] >> j) & 1u) ++want_pairs[i * (i + 1) / 2 + j];
        }
      if (held) ++want_exact[held];
      if (held == 1) ++want_priv[last];
    }
  }
  for (uint32_t p = 0; p < np; ++p) CHECK(pairs[p] == want_pairs[p], "%s n=%u pair %u: %llu, want %llu", what, n, p,
                                          (unsigned long long)pairs[p], (unsigned long long)want_pairs[p]);
  for (uint32_t m = 0; m <= n; ++m) CHECK(exact[m] == want_exact[m], "%s n=%u in_exactly[%u]: %llu, want %llu", what, n, m,
                                          (unsigned long long)exact[m], (unsigned long long)want_exact[m]);
  for (uint32_t i = 0; i < n; ++i) CHECK(priv[i] == want_priv[i], "%s n=%u private[%u]: %llu, want %llu", what, n, i,
                                         (unsigned long long)priv[i], (unsigned long long)want_priv[i]);

  // fold: the cells as the device leaves them, without and with a key that has no slot
  std::vector<uint64_t> cells(kmcooc::CELLS, 0);
  for (uint32_t p = 0; p < np; ++p) cells[p] = pairs[p];
  for (uint32_t m = 0; m <= n; ++m) cells[kmcooc::CELL_EXACT + m] = exact[m];
  for (uint32_t i = 0; i < n; ++i) cells[kmcooc::CELL_PRIVATE + i] = priv[i];
  const uint32_t extras[3] = {0u, 1u << (n - 1), (uint32_t)next_u64()};
  for (uint32_t extra : extras) {
    kmcooc::Result r;
    kmcooc::fold(cells.data(), n, extra, &r);
    const uint32_t e = kmcooc::input_bits(extra, n);
    uint64_t un = e ? 1 : 0;
    for (uint32_t m = 1; m <= n; ++m) un += want_exact[m];
    CHECK(r.n_union == un, "%s n=%u extra=%x union %llu, want %llu", what, n, e, (unsigned long long)r.n_union, (unsigned long long)un);
    for (uint32_t i = 0; i < kmcooc::MAX_INPUTS; ++i)
      for (uint32_t j = 0; j < kmcooc::MAX_INPUTS; ++j) {
        uint64_t want = 0;
        if (i < n && j < n) want = want_pairs[i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i] + (((e >> i) & (e >> j) & 1u) ? 1 : 0);
        CHECK(r.shared[i * kmcooc::MAX_INPUTS + j] == want, "%s n=%u extra=%x shared[%u][%u]", what, n, e, i, j);
      }
    for (uint32_t m = 1; m <= n; ++m)
      CHECK(r.in_exactly[m] == want_exact[m] + (e && kmcooc::popc32(e) == m ? 1 : 0), "%s n=%u extra=%x in_exactly[%u]", what, n, e, m);
    for (uint32_t i = 0; i < n; ++i)
      CHECK(r.priv[i] == want_priv[i] + (e == (1u << i) ? 1 : 0), "%s n=%u extra=%x private[%u]", what, n, e, i);
  }
  ++cases;
}

std::vector<uint32_t> filled(uint32_t v) { return std::vector<uint32_t>(kmcooc::WAVE, v); }
uint32_t bits_of(uint32_t n) { return n >= 32 ? 0xFFFFFFFFu : (1u << n) - 1u; }
}  // namespace

int main() {
  for (uint32_t n = 1; n <= kmcooc::MAX_INPUTS; ++n) check_mapping(n);
  for (uint32_t n = 1; n <= kmcooc::MAX_INPUTS; ++n) {
    check_trips(n, {filled(0u)}, "all zero");
    check_trips(n, {filled(bits_of(n))}, "all one");
    for (uint32_t s : {0u, 1u, 31u, 32u, 63u}) {
      std::vector<uint32_t> one = filled(0u);
      one[s] = bits_of(n);
      check_trips(n, {one}, "a single slot");
    }
    for (uint32_t i : {0u, n / 2, n - 1}) check_trips(n, {filled(1u << i)}, "a single input");
    for (int round = 0; round < 8; ++round) {
      std::vector<std::vector<uint32_t>> dense(3, filled(0u)), sparse(3, filled(0u)), beyond(1, filled(0u));
      for (auto& t : dense)
        for (auto& m : t) m = (uint32_t)next_u64() & bits_of(n);
      for (auto& t : sparse)
        for (auto& m : t) m = (next_u64() & 3u) ? 0u : ((uint32_t)next_u64() & (uint32_t)next_u64() & bits_of(n));
      for (auto& m : beyond[0]) m = (uint32_t)next_u64();            // bits at or above n are ignored
      check_trips(n, dense, "random dense");
      check_trips(n, sparse, "random sparse");
      // (brute force must not see the ignored bits either)
      std::vector<std::vector<uint32_t>> cut = beyond;
      for (auto& m : cut[0]) m &= bits_of(n);
      std::vector<uint64_t> a(kmcooc::n_pairs(n), 0), ea(n + 1, 0), pa(n, 0), b(kmcooc::n_pairs(n), 0), eb(n + 1, 0), pb(n, 0);
      kmcooc::trip_model(beyond[0].data(), n, a.data(), ea.data(), pa.data());
      kmcooc::trip_model(cut[0].data(), n, b.data(), eb.data(), pb.data());
      CHECK(a == b && ea == eb && pa == pb, "n=%u: bits at or above n changed the sums", n);
      check_trips(n, cut, "random cut");
    }
  }
  if (failures) return 1;
  std::printf("COOC RULE OK %llu cases\n", (unsigned long long)cases);
  return 0;
}
