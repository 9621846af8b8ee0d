// merge_pieces.h — cutting n fixed-size records into the pieces a staging buffer holds, packing host arrays into file
// records, reading a piece out of a file (host only; merge_host.h, histo_host.h, db_host.h, tests/host/merge_pieces.cpp).
//
// A staging buffer of `stage` bytes takes whole records only, so a piece is stage / rec records — the staging size
// rounded DOWN to a multiple of the record size (16 MiB is not a multiple of 12) — and the last piece is what is
// left.  Piece i starts at record i * per, which is byte i * per * rec of the record area: a multiple of rec, so
// no record is ever split and every piece starts at the buffer's first byte.
#pragma once
#include <errno.h>
#include <stdint.h>
#include <string.h>
#include <unistd.h>

namespace kmpiece {

constexpr uint64_t PACKED_KEY_BYTES = 8, PACKED_COUNT_BYTES = 4;
constexpr uint64_t PACKED_RECORD = PACKED_KEY_BYTES + PACKED_COUNT_BYTES;     // what add_records stages

struct Piece {
  uint64_t first;      // index of its first record
  uint64_t records;    // 1 .. per
  uint64_t bytes;      // records * rec <= stage
};

// records per piece; 0 only for a staging buffer smaller than one record (the caller refuses that)
inline uint64_t per_piece(uint64_t stage, uint64_t rec) { return rec ? stage / rec : 0; }

inline uint64_t n_pieces(uint64_t n, uint64_t per) { return per ? (n + per - 1) / per : 0; }

// piece i of n records (i < n_pieces)
inline Piece piece(uint64_t n, uint64_t per, uint64_t rec, uint64_t i) {
  Piece p;
  p.first = i * per;
  p.records = n - p.first < per ? n - p.first : per;
  p.bytes = p.records * rec;
  return p;
}

// keys / counts [first, first + m) as m records of 8 little-endian key bytes and 4 count bytes at out[12 m]
// (the host is little-endian, as every reader and writer of this project assumes)
inline void pack(const uint64_t* keys, const uint32_t* counts, uint64_t first, uint64_t m, unsigned char* out) {
  for (uint64_t i = 0; i < m; ++i) {
    memcpy(out + i * PACKED_RECORD, keys + first + i, PACKED_KEY_BYTES);
    memcpy(out + i * PACKED_RECORD + PACKED_KEY_BYTES, counts + first + i, PACKED_COUNT_BYTES);
  }
}

// n bytes of fd from `offset` on into dst, in as many reads as that takes.  0: all n are there; an errno: a read
// failed; ENDED_EARLY: the file has fewer (what it had is in dst, and nothing was written behind that).
constexpr int ENDED_EARLY = -1;
inline int read_exact(int fd, unsigned char* dst, uint64_t n, uint64_t offset) {
  for (uint64_t got = 0; got < n;) {
    const ssize_t r = pread(fd, dst + got, n - got, (off_t)(offset + got));
    if (r < 0 && errno == EINTR) continue;
    if (r <= 0) return r < 0 ? errno : ENDED_EARLY;
    got += (uint64_t)r;
  }
  return 0;
}

}  // namespace kmpiece
