// tier_geometry.h — what the LDS-resident ("fast") tier of the walk and graph kernels can hold: its constants and
// the one predicate km_batch's geometry (batch_host.h: fast_geometry) bisects over.  Plain host arithmetic on the
// kernels' own size functions, kept apart from km_batch so that a host program can ask it too
// (tests/host/lds_tier_limit.hip, tests/host/walk_geometry.hip).
#pragma once
#include <algorithm>
#include "graph_kernel.h"
#include "walk_kernel.h"

namespace {

constexpr uint32_t FAST_EXTRA = 160;          // walk-discovered nodes a fast-tier target may add
constexpr uint32_t FAST_LDS_LIMIT = 64 * 1024;
constexpr uint32_t FAST_BCAP_MAX = 512;       // branch frames the fast tier keeps in LDS

static uint32_t round_up(uint32_t v, uint32_t m) { return (v + m - 1) / m * m; }
static uint32_t words_cap_for(uint32_t len) { return round_up((len + 31) / 32 + 1, 2); }
// slots of the graph kernels' node hash: load <= 2/3
static uint32_t graph_hcap(uint32_t ncap) { return round_up(ncap + ncap / 2 + 1, 64); }

// slots of k_dfs's node set in the fast tier.  It holds the walk's nodes, the stack, and the target k-mers that lost
// their slot of the position table (a fifth of them with the table at load 1/2): room for a quarter of the target's
// k-mers + every allowed extra node + 64 frames, at load <= 3/4 (what does not fit goes to the large tier)
static uint32_t walk_hs_cap(uint32_t nref) { return round_up((uint32_t)(((uint64_t)(nref / 4 + FAST_EXTRA + 64) * 4 + 2) / 3), 64); }
// slots of its position table: the power of two >= four times the target's k-mers (load <= 1/4: a tenth of the k-mers lose their slot)
static uint32_t walk_pcap(uint32_t nref) { uint32_t p = 64; while (p < 4 * nref) p <<= 1; return p; }

// a target of `nref` k-mers (k = `k`) with `bcap` branch frames
static bool fast_tier_fits(int k, uint32_t nref, uint32_t bcap) {
  const uint32_t len = nref + (uint32_t)k - 1;
  const uint32_t wc = words_cap_for(len);
  const uint32_t hs = walk_hs_cap(nref);
  const uint32_t ncap = nref + FAST_EXTRA + 2, hcap = graph_hcap(ncap);
  return kmd::walk_lds_bytes(hs, wc, bcap, walk_pcap(nref), 2) <= FAST_LDS_LIMIT &&
         kmd::graph_ws_bytes<uint16_t>(ncap, hcap, wc) <= FAST_LDS_LIMIT && ncap < 0xFFFF &&
         (uint64_t)hcap * 4 + (uint64_t)wc * 8 <= FAST_LDS_LIMIT;   // (k_graph_pure hands over what its own table cannot hold)
}

constexpr uint32_t FAST_FCAP_MAX = 4096;      // stack frames per target in the fast tier's scratch

// the sizes of the fast tier for a batch whose longest target has `max_nref` k-mers: what km_batch launches k_dfs and
// k_graph with (batch_host.h: fast_geometry) and what tests/host/walk_geometry.hip prints
struct FastGeometry { uint32_t nref, hs_cap, pcap, words_cap, fcap, bcap, ncap, hcap; };
static FastGeometry fast_tier_geometry(int k, uint32_t max_nref, uint32_t max_stack, uint32_t max_break) {
  FastGeometry g;
  g.bcap = std::min<uint32_t>(max_break, FAST_BCAP_MAX - 1) + 1;
  g.fcap = round_up(std::min<uint32_t>(max_stack, FAST_FCAP_MAX - 2) + 2, 2);
  uint32_t nref = max_nref;
  if (!fast_tier_fits(k, nref, g.bcap)) {
    uint32_t lo = 1, hi = max_nref;          // fits(lo) holds: a 1-k-mer target always fits
    while (lo + 1 < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (fast_tier_fits(k, mid, g.bcap)) lo = mid; else hi = mid;
    }
    nref = lo;
  }
  g.nref = nref;
  g.hs_cap = walk_hs_cap(nref);
  g.pcap = walk_pcap(nref);
  g.words_cap = words_cap_for(nref + (uint32_t)k - 1);
  g.ncap = nref + FAST_EXTRA + 2;
  g.hcap = graph_hcap(g.ncap);
  return g;
}

}  // namespace
