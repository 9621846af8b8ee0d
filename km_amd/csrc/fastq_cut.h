// fastq_cut.h — where the last complete record of a block of 4-line FASTQ text ends (host only).
//
// km_counter_add_fastq hands raw text to the device in pieces of whole records, so the host has to find a record
// end near the end of a block without parsing the block.  The lines that start with '@' are headers and, at
// times, quality lines; what tells them apart is the line two below: below a header it is the '+' line, below a
// quality line it is the next record's sequence, which cannot start with '+'.  So a line that starts with '@'
// and has a line starting with '+' two below it is a header.  The last such line is looked for among the last
// CUT_LINES line starts, found by walking back from the end; the block itself is not passed over.
#pragma once
#include <stdint.h>
#include <string.h>

namespace kmcut {

constexpr int CUT_LINES = 8;     // a header with its '+' line in sight lies at most seven line starts from the end

// The largest offset <= n at which a record ends: behind the newline of the quality line of the last record
// whose four lines are all there, newlines included, or 0 if there is none.
inline uint64_t cut(const char* text, uint64_t n) {
  uint64_t start[CUT_LINES + 1];   // line starts, descending; start[i] == n: a line of which nothing is there yet
  int m = 0;
  uint64_t end = n;
  while (m < CUT_LINES && end > 0) {
    const char* nl = (const char*)memrchr(text, '\n', end);
    if (!nl) break;
    end = (uint64_t)(nl - text);
    start[m++] = end + 1;
  }
  if (m < CUT_LINES) start[m++] = 0;
  // ascending order: line i begins at at(i)
  auto at = [&](int i) { return start[m - 1 - i]; };
  for (int i = m - 1; i >= 0; --i) {
    if (at(i) >= n || text[at(i)] != '@') continue;
    if (i + 2 >= m || at(i + 2) >= n || text[at(i + 2)] != '+') continue;
    return i + 4 < m ? at(i + 4) : at(i);       // the header's own record if its quality line has its newline
  }
  return 0;
}

// ---- the pieces of a call: what every consumer of raw FASTQ text (counter, selector, pair selector, kmjf_fastq_hits)
// sends to the device, one staging buffer at a time
// The end of what a call may take of text[0 .. n): all of it when the stream ends with the call, else its whole records.
inline uint64_t call_end(const char* text, uint64_t n, bool final) { return final ? n : cut(text, n); }

// The next piece of text[pos .. end), pos < end, for staging buffers of `stage` bytes: all that is left if that fits,
// else the whole records within the next `stage` bytes; 0: no record ends within them.
inline uint64_t next_piece(const char* text, uint64_t pos, uint64_t end, uint64_t stage) {
  return end - pos <= stage ? end - pos : cut(text + pos, stage);
}

}  // namespace kmcut
