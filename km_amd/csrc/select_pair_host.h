// select_pair_host.h — km_select_pair_* (host part of kmgpu.hip; device side: select_pair_kernel.h behind
// select_host.h's SelDev per mate; the rule: select_pair_rule.h)
// ------------------------------------------------------------------ select, pairs: the mates of a run kept together
// Two FASTQ streams whose records correspond one to one.  A piece is one staging buffer's worth of whole records from
// EACH stream (fastq_take); the two hold different numbers of records wherever the mates differ in bytes per record.
// The device pairs the first R = min(records 1, records 2) of them and hands back, with the totals, the offset at which
// record R begins in either piece; the host advances each stream by that, and the surplus records of the longer side go
// to the device again at the head of the next piece.  The host never passes over the text to count lines: memcpy and
// kmcut::cut are its only contact with the bytes.  Output: a TextDrain per mate, written a piece later as in
// select_host.h.
struct km_select_pair : SelCore {
  uint32_t rule = 0;
  int check_names = 1;
  Staging in[2], out[2];
  SelDev dev[2];
  DevBuf<unsigned long long> pmeta;       // [0] the name cell, [1..4] the PAIR_* cells
  Pinned back;                            // 40 bytes of pmeta per output buffer
  DevBuf<uint8_t> d_out[2][2];            // [mate][buffer]
  TextDrain drain[2];                     // (their turns pass together)
  uint64_t offset[2] = {0, 0};            // bytes consumed by the earlier calls of this pair of streams
  uint64_t pair_base = 0;                 // ... and pairs
  km_select_pair_stats_t stats;
  StreamDrain sync;
  km_select_pair() { memset(&stats, 0, sizeof stats); }
  uint32_t* cells() const { return reinterpret_cast<uint32_t*>(pmeta.p + 1); }
  PairSide side(int m, uint64_t n) const {
    const SelDev& d = dev[m];
    return PairSide{d.d_text.p, d.fq.line_start.p, d.hits.p, d.cells(), d.len.p, (uint32_t)n,
                    (uint32_t)(SelDev::len_chunks(n) * SCAN_CHUNK)};
  }
  int names_failed(unsigned long long r, const uint64_t base[2]) {
    uint32_t header[2] = {0, 0};
    for (int m = 0; m < 2; ++m)
      HIPCHK(hipMemcpy(&header[m], dev[m].fq.line_start.p + 4ull * r, 4, hipMemcpyDeviceToHost));
    return fail(KM_E_FORMAT, "mate names differ at pair %llu: the header of mate 1 at byte offset %llu, of mate 2 at byte offset %llu",
                (unsigned long long)(pair_base + r), (unsigned long long)(base[0] + header[0]),
                (unsigned long long)(base[1] + header[1]));
  }
  // One piece of whole records from either stream, text[m][0 .. n[m]) at stream offset base[m]; ends[m]: stream m ends
  // with these bytes.  used[m]: the bytes of the pairs it made.
  int piece(const char* const text[2], const uint64_t n[2], const uint64_t base[2], const bool ends[2], uint64_t used[2]) {
    const int buf = drain[0].begin();
    drain[1].begin();
    const TableView tv = view_of(h);
    for (int m = 0; m < 2; ++m) {
      KMCHK(in[m].claim());
      memcpy(in[m].mine, text[m], n[m]);
      KMCHK(in[m].ship(dev[m].d_text, n[m], st));
      KMCHK(dev[m].front_hits(tv, n[m], base[m], min_qual, st));
    }
    const PairSide a = side(0, n[0]), b = side(1, n[1]);
    const uint32_t pad = std::max(a.n_pad, b.n_pad);
    KMCHK(dev[0].spans[2].open(st));
    hipLaunchKernelGGL(k_pair_clear, dim3(1), dim3(64), 0, st, pmeta.p, cells());
    hipLaunchKernelGGL(k_pair_sizes, dim3(pad / kmsel::THREADS), dim3(kmsel::THREADS), 0, st, a, b, min_hits,
                       invert ? 1u : 0u, rule, cells());
    if (check_names) {
      const uint32_t most = std::min(kmsel::max_records(n[0]), kmsel::max_records(n[1]));
      hipLaunchKernelGGL(k_pair_names, dim3(grid_for(most, kmsel::THREADS)), dim3(kmsel::THREADS), 0, st, a, b, pmeta.p);
    }
    for (int m = 0; m < 2; ++m) scan_in_place(dev[m].len.p, dev[m].sums.p, (m ? b.n_pad : a.n_pad) / SCAN_CHUNK, st);
    HIPCHK(hipGetLastError());
    KMCHK(dev[0].spans[2].close(st));
    KMCHK(dev[0].spans[3].open(st));
    const uint64_t words = (std::max(n[0], n[1]) + kmsel::WORD - 1) / kmsel::WORD;
    hipLaunchKernelGGL(k_pair_gather, dim3((uint32_t)((words + kmsel::THREADS - 1) / kmsel::THREADS), 2), dim3(kmsel::THREADS),
                       0, st, PairOut{a.text, a.line_start, a.len, d_out[0][buf].p},
                       PairOut{b.text, b.line_start, b.len, d_out[1][buf].p}, cells());
    HIPCHK(hipGetLastError());
    KMCHK(dev[0].spans[3].close(st));
    KMCHK(dev[0].read_back(buf, st));
    KMCHK(dev[1].read_back(buf, st));
    HIPCHK(hipMemcpyAsync(back.h + 64 * buf, pmeta.p, 8 + 4 * PAIR_CELLS, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(done[buf], st));
    KMCHK(drain[0].put_before(buf));      // while this one is scanned
    KMCHK(drain[1].put_before(buf));
    HIPCHK(hipEventSynchronize(done[buf]));
    for (int i = 0; i < 4; ++i) {
      float t[2] = {0.f, 0.f};
      for (int m = 0; m < 2; ++m) KMCHK(dev[m].spans[i].drain(&t[m]));
      g_select_ms[i] = t[0] + t[1];
    }
    for (int m = 0; m < 2; ++m)
      if (dev[m].error_of(buf) != FQ_NO_ERROR) {
        const unsigned long long error = dev[m].error_of(buf);
        return fail(KM_E_FORMAT, "mate %d: %s at byte offset %llu", m + 1, fastq_error_text((unsigned)(error & 0xFF)),
                    (unsigned long long)(error >> 8));
      }
    const unsigned long long differ = *reinterpret_cast<const volatile unsigned long long*>(back.h + 64 * buf);
    if (differ != PAIR_NAMES_AGREE) return names_failed(differ, base);
    const volatile uint32_t* c = reinterpret_cast<const volatile uint32_t*>(back.h + 64 * buf + 8);
    used[0] = c[PAIR_USED1];
    used[1] = c[PAIR_USED2];
    if (c[PAIR_R] == 0 || used[0] == 0 || used[1] == 0 || used[0] > n[0] || used[1] > n[1])
      return fail(KM_E_FORMAT, "a piece of whole records gave no pair at byte offsets %llu and %llu",
                  (unsigned long long)base[0], (unsigned long long)base[1]);
    stats.pairs_in += c[PAIR_R];
    stats.pairs_out += c[PAIR_KEPT];
    ++stats.pieces;
    pair_base += c[PAIR_R];
    for (int m = 0; m < 2; ++m) {
      const uint32_t bytes = c[m ? PAIR_BYTES2 : PAIR_BYTES1];
      stats.bytes_in[m] += used[m];
      stats.resent_bytes[m] += n[m] - used[m];
      stats.bytes_out[m] += bytes;
      drain[m].close_line[buf] = ends[m] && used[m] == n[m] && text[m][n[m] - 1] != '\n';
      KMCHK(drain[m].fetch(buf, d_out[m][buf].p, bytes));
    }
    return KM_OK;
  }
  int flush() {
    const int rc = drain[0].flush(&stats.bytes_out[0]);       // either mate's, whatever the other's did
    const int rc2 = drain[1].flush(&stats.bytes_out[1]);
    return rc != KM_OK ? rc : rc2;
  }
};

extern "C" int km_select_pair_create(kmjf_t* h, uint32_t min_hits, int invert, int min_qual_char, int rule, int check_names,
                                     int out_fd1, int out_fd2, void* stream, km_select_pair_t** out) {
  const int fds[2] = {out_fd1, out_fd2};
  KMCHK(select_check_create(h, out, min_hits, min_qual_char, rule, fds, 2));
  std::unique_ptr<km_select_pair> s(new (std::nothrow) km_select_pair);
  if (!s) return fail(KM_E_NOMEM, "host allocation failed");
  KMCHK(s->open(h, min_hits, invert, min_qual_char, stream, &s->sync));
  s->rule = (uint32_t)rule;
  s->check_names = check_names ? 1 : 0;
  KMCHK(s->pmeta.alloc(1 + PAIR_CELLS / 2));
  KMCHK(pinned_alloc(&s->back, 128, "pinned totals"));
  for (int m = 0; m < 2; ++m) {
    KMCHK(s->in[m].alloc(0));
    KMCHK(s->out[m].alloc(1));                          // (room for the newline behind an open last line)
    KMCHK(s->dev[m].alloc(s->in[m].bytes, true, s->st));
    for (int i = 0; i < 2; ++i) KMCHK(s->d_out[m][i].alloc(s->in[m].bytes + kmsel::OUT_PAD));
    s->drain[m].out = &s->out[m];
    s->drain[m].cs = s->cs;
    s->drain[m].fd = fds[m];
  }
  HIPCHK(hipStreamSynchronize(s->st));
  for (float& v : g_select_ms) v = 0.f;
  *out = s.release();
  return KM_OK;
}

extern "C" int km_select_pair_add_fastq(km_select_pair_t* s, const char* text1, uint64_t n1, const char* text2, uint64_t n2,
                                        int final, uint64_t* consumed1, uint64_t* consumed2) {
  if (!s || !consumed1 || !consumed2 || (n1 && !text1) || (n2 && !text2)) return fail(KM_E_ARG, "null argument");
  KMCHK(s->alive());
  *consumed1 = *consumed2 = 0;
  const char* const text[2] = {text1, text2};
  const uint64_t n[2] = {n1, n2};
  uint64_t end[2], pos[2] = {0, 0};
  for (int m = 0; m < 2; ++m) end[m] = kmcut::call_end(text[m], n[m], final);
  if (end[0] && end[1]) HIPCHK(hipSetDevice(s->h->device));
  int rc = KM_OK;
  while (pos[0] < end[0] && pos[1] < end[1] && rc == KM_OK) {
    uint64_t take[2] = {0, 0}, base[2], used[2] = {0, 0};
    const char* at[2];
    bool ends[2];
    for (int m = 0; m < 2 && rc == KM_OK; ++m) {
      rc = fastq_take(text[m], pos[m], end[m], s->in[m].bytes, s->offset[m], &take[m]);
      at[m] = text[m] + pos[m];
      base[m] = s->offset[m] + pos[m];
      ends[m] = final && pos[m] + take[m] == end[m];
    }
    if (rc == KM_OK) rc = s->piece(at, take, base, ends, used);
    if (rc == KM_OK) {
      pos[0] += used[0];
      pos[1] += used[1];
      *consumed1 = pos[0];
      *consumed2 = pos[1];
    }
  }
  std::string msg = rc != KM_OK ? g_last_error : std::string();
  const int rc_flush = s->flush();
  if (rc == KM_OK && rc_flush == KM_OK && final && (pos[0] < end[0]) != (pos[1] < end[1])) {
    rc = fail(KM_E_FORMAT, "mate files differ in their number of records: mate %d has more, the first pair without a partner is pair %llu",
              pos[0] < end[0] ? 1 : 2, (unsigned long long)s->pair_base);
    msg = g_last_error;
  }
  KMCHK(s->end_call(rc, msg, rc_flush));
  for (int m = 0; m < 2; ++m) s->offset[m] = final ? 0 : s->offset[m] + pos[m];
  if (final) s->pair_base = 0;
  return KM_OK;
}

extern "C" int km_select_pair_stats(km_select_pair_t* s, km_select_pair_stats_t* stats) {
  if (!s || !stats) return fail(KM_E_ARG, "null argument");
  *stats = s->stats;
  return KM_OK;
}

extern "C" int km_select_pair_destroy(km_select_pair_t* s) {
  delete s;
  return KM_OK;
}
