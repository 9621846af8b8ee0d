// CPU-only driver for km_amd/csrc/merge_pieces.h (the piece arithmetic of km_counter_add_records /
// km_counter_add_jf), built with -fsanitize=address,undefined by tests/test_merge.py:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o merge_pieces \
//       tests/host/merge_pieces.cpp && ./merge_pieces
// For every record size 3..12 and the staging sizes 256, 4 096 and 16 MiB it walks a record area the way
// merge_enqueue does — each piece copied into a heap buffer of EXACTLY the staging size, so a piece that is a byte
// too long is a heap overflow the sanitizer reports — and checks that the pieces are whole records, in order,
// without gap or overlap, that only the last one is short, and that what arrives is what was sent.  Then the same
// for host arrays packed into 12-byte records, and read_exact (the one loop over pread, under RecordFile::read) over
// a temporary file, into heap buffers of exactly the length asked for.  Prints "PIECES OK".
#include <fcntl.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../km_amd/csrc/merge_pieces.h"

#define REQUIRE(cond)                                                                  \
  do {                                                                                 \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

static uint64_t mix(uint64_t x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// the record counts worth walking for `per` records per piece: none, one, around one piece, and two pieces with a
// last one of a single record
static std::vector<uint64_t> counts_for(uint64_t per) { return {0, 1, per - 1, per, per + 1, 2 * per, 2 * per + 1}; }

static int walk_area(uint64_t stage, uint64_t rec) {
  const uint64_t per = kmpiece::per_piece(stage, rec);
  REQUIRE(per >= 1 && per * rec <= stage && stage - per * rec < rec);       // rounded DOWN to whole records
  for (uint64_t n : counts_for(per)) {
    std::vector<unsigned char> area(n * rec), back(n * rec);
    for (uint64_t i = 0; i < area.size(); i += 8) {                          // (a word at a time: 16 MiB pieces)
      const uint64_t v = mix(i + rec);
      memcpy(area.data() + i, &v, area.size() - i < 8 ? area.size() - i : 8);
    }
    const uint64_t pieces = kmpiece::n_pieces(n, per);
    REQUIRE(pieces == (n + per - 1) / per);
    uint64_t next = 0;
    std::vector<unsigned char> staged(stage);                                // one pinned buffer
    for (uint64_t i = 0; i < pieces; ++i) {
      const kmpiece::Piece p = kmpiece::piece(n, per, rec, i);
      REQUIRE(p.first == next && p.records >= 1 && p.records <= per && p.bytes == p.records * rec);
      REQUIRE(p.records == per || i + 1 == pieces);                          // only the last piece is short
      memcpy(staged.data(), area.data() + p.first * rec, p.bytes);
      memcpy(back.data() + p.first * rec, staged.data(), p.bytes);
      next += p.records;
    }
    REQUIRE(next == n && back == area);
  }
  return 0;
}

static int walk_arrays(uint64_t stage) {
  const uint64_t rec = kmpiece::PACKED_RECORD, per = kmpiece::per_piece(stage, rec);
  REQUIRE(rec == 12);
  for (uint64_t n : counts_for(per)) {
    std::vector<uint64_t> keys(n);                                           // exactly n: a read past the end is reported
    std::vector<uint32_t> counts(n);
    for (uint64_t i = 0; i < n; ++i) { keys[i] = mix(i + 1); counts[i] = (uint32_t)mix(~i); }
    if (n) { keys[0] = ~0ull; counts[0] = 0xFFFFFFFFu; }
    uint64_t seen = 0;
    std::vector<unsigned char> staged(stage);
    for (uint64_t i = 0; i < kmpiece::n_pieces(n, per); ++i) {
      const kmpiece::Piece p = kmpiece::piece(n, per, rec, i);
      kmpiece::pack(keys.data(), counts.data(), p.first, p.records, staged.data());
      for (uint64_t j = 0; j < p.records; ++j, ++seen) {                     // as the kernel and the readers decode
        uint64_t key = 0;
        uint32_t cnt = 0;
        for (int b = 0; b < 8; ++b) key |= (uint64_t)staged[j * 12 + b] << (8 * b);
        for (int b = 0; b < 4; ++b) cnt |= (uint32_t)staged[j * 12 + 8 + b] << (8 * b);
        REQUIRE(key == keys[seen] && cnt == counts[seen]);
      }
    }
    REQUIRE(seen == n);
  }
  return 0;
}

// read_exact over a file of a 9 + 5 byte header and 96 bytes of records (12 records of 8 bytes)
static int read_area() {
  char path[] = "/tmp/merge_pieces_XXXXXX";
  const int fd = mkstemp(path);
  REQUIRE(fd >= 0);
  const uint64_t header = 9 + 5, body = 96;
  std::vector<unsigned char> file(header + body);
  for (uint64_t i = 0; i < file.size(); ++i) file[i] = (unsigned char)mix(i);
  const bool written = write(fd, file.data(), file.size()) == (ssize_t)file.size();
  const int wr = open(path, O_WRONLY);
  unlink(path);
  REQUIRE(written && wr >= 0);
  {                                                                          // ends exactly at the end of the file
    std::vector<unsigned char> dst(body);
    REQUIRE(kmpiece::read_exact(fd, dst.data(), body, header) == 0);
    REQUIRE(memcmp(dst.data(), file.data() + header, body) == 0);
  }
  {                                                                          // the second of three pieces of 32 bytes
    std::vector<unsigned char> dst(32);
    REQUIRE(kmpiece::read_exact(fd, dst.data(), 32, header + 32) == 0);
    REQUIRE(memcmp(dst.data(), file.data() + header + 32, 32) == 0);
  }
  {                                                                          // nothing asked for: nothing touched
    std::vector<unsigned char> dst(1, 0xA5);
    REQUIRE(kmpiece::read_exact(fd, dst.data(), 0, header) == 0 && dst[0] == 0xA5);
    REQUIRE(kmpiece::read_exact(fd, nullptr, 0, file.size() + 7) == 0);
  }
  {                                                                          // the file is one byte short
    std::vector<unsigned char> dst(body, 0xA5);
    REQUIRE(kmpiece::read_exact(fd, dst.data(), body, header + 1) == kmpiece::ENDED_EARLY);
    REQUIRE(memcmp(dst.data(), file.data() + header + 1, body - 1) == 0 && dst[body - 1] == 0xA5);
    REQUIRE(kmpiece::read_exact(fd, dst.data(), 1, file.size()) == kmpiece::ENDED_EARLY);
  }
  {                                                                          // a read that fails: its errno
    std::vector<unsigned char> dst(body, 0xA5);
    REQUIRE(kmpiece::read_exact(wr, dst.data(), body, header) == EBADF);
    REQUIRE(dst[0] == 0xA5 && dst[body - 1] == 0xA5);
  }
  close(wr);
  close(fd);
  return 0;
}

int main() {
  if (read_area()) return 1;
  const uint64_t stages[] = {256, 4096, 16ull << 20};
  for (uint64_t stage : stages) {
    for (uint64_t rec = 3; rec <= 12; ++rec)
      if (walk_area(stage, rec)) return 1;
    if (walk_arrays(stage)) return 1;
  }
  REQUIRE(kmpiece::per_piece(256, 12) == 21 && kmpiece::per_piece(256, 10) == 25 && kmpiece::per_piece(4096, 12) == 341);
  REQUIRE(kmpiece::per_piece(16ull << 20, 12) == 1398101 && (16ull << 20) - 1398101ull * 12 == 4);
  printf("PIECES OK\n");
  return 0;
}
