// fastx_strip.h — FASTA / 4-line FASTQ text -> the byte stream the counting kernel reads (host only).
//
// Only sequence bytes leave the stripper, followed by one break byte where a read ends: the lines of a FASTA
// record are joined, of a FASTQ record only line 2 is taken (quality lines are made of letters that include
// A C G T).  The stripper works on whole lines: a call that ends inside a line leaves that line to the caller
// (*consumed), who passes it again in front of the next block; the last call (final) takes an unterminated
// last line as it is.  "\r\n" is accepted.  Every output byte stands for an input byte of its own (a break for
// the line's newline or for a header), plus one break at the very end: n input bytes give at most n + 1.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/kmgpu.h"

namespace kmstrip {

constexpr uint8_t BREAK = '\n';
enum { FMT_UNKNOWN = 0, FMT_FASTA = 1, FMT_FASTQ = 2 };
enum { ERR_NONE = 0, ERR_FIRST_BYTE = 1, ERR_NO_AT = 2, ERR_NO_PLUS = 3 };

struct Result {
  uint64_t consumed = 0;
  int error = ERR_NONE;
  uint64_t error_offset = 0;     // within the stream (all calls since the last final one)
};

// Sink: void bytes(const uint8_t*, uint64_t); void brk();
template <class Sink>
Result strip(km_text_state_t* st, const char* text, uint64_t n, int final, Sink& sink) {
  Result r;
  uint64_t pos = 0;
  while (pos < n) {
    const char* nl = (const char*)memchr(text + pos, '\n', n - pos);
    if (!nl && !final) break;                                   // an unfinished line: the caller's to keep
    const uint64_t end = nl ? (uint64_t)(nl - text) : n;        // one past the line's last byte
    uint64_t len = end - pos;
    if (len && text[pos + len - 1] == '\r') --len;
    const char* line = text + pos;
    const uint64_t line_off = st->offset + pos;
    const uint64_t next = nl ? end + 1 : n;
    if (st->format == FMT_UNKNOWN) {
      if (len == 0) { pos = next; continue; }                   // blank lines in front of the first record
      if (line[0] == '>') st->format = FMT_FASTA;
      else if (line[0] == '@') st->format = FMT_FASTQ;
      else { r.error = ERR_FIRST_BYTE; r.error_offset = line_off; r.consumed = pos; return r; }
      st->line = 0;
    }
    if (st->format == FMT_FASTA) {
      if (len && line[0] == '>') {
        if (st->open) { sink.brk(); st->open = 0; }
      } else if (len) {
        sink.bytes((const uint8_t*)line, len);
        st->open = 1;
      }
    } else {
      switch (st->line) {
        case 0:
          if (len == 0) { pos = next; continue; }               // blank line between records
          if (line[0] != '@') { r.error = ERR_NO_AT; r.error_offset = line_off; r.consumed = pos; return r; }
          st->line = 1;
          break;
        case 1:
          if (len) sink.bytes((const uint8_t*)line, len);
          sink.brk();
          st->line = 2;
          break;
        case 2:
          if (len == 0 || line[0] != '+') { r.error = ERR_NO_PLUS; r.error_offset = line_off; r.consumed = pos; return r; }
          st->line = 3;
          break;
        default:
          st->line = 0;                                         // the quality line: never looked at
          break;
      }
    }
    pos = next;
  }
  r.consumed = pos;
  if (final) {
    if (st->format == FMT_FASTQ && st->line == 2) {             // a sequence and then nothing
      r.error = ERR_NO_PLUS;
      r.error_offset = st->offset + n;
      return r;
    }
    if (st->open) sink.brk();
    memset(st, 0, sizeof *st);                                  // the next stream may be of the other format
  } else {
    st->offset += pos;
  }
  return r;
}

inline const char* error_text(int e) {
  switch (e) {
    case ERR_FIRST_BYTE: return "neither FASTA ('>') nor FASTQ ('@')";
    case ERR_NO_AT: return "FASTQ record does not start with '@'";
    case ERR_NO_PLUS: return "FASTQ record lacks its '+' line";
  }
  return "";
}

}  // namespace kmstrip
