// select_pair_host.h — km_select_pair_* (host part of kmgpu.hip; device side: select_pair_kernel.h behind
// select_host.h's SelDev per mate; the rule: select_pair_rule.h)
// ------------------------------------------------------------------ select, pairs: the mates of a run kept together
// Two FASTQ streams whose records correspond one to one.  A piece is one staging buffer's worth of whole records from
// EACH stream (select_take); the two hold different numbers of records wherever the mates differ in bytes per record.
// The device pairs the first R = min(records 1, records 2) of them and hands back, with the totals, the offset at which
// record R begins in either piece; the host advances each stream by that, and the surplus records of the longer side go
// to the device again at the head of the next piece.  The host never passes over the text to count lines: memcpy and
// kmcut::cut are its only contact with the bytes.  Output: a TextDrain per mate, written a piece later as in
// select_host.h.
struct km_select_pair {
  kmjf_t* h = nullptr;
  uint32_t min_hits = 1, min_qual = 0, rule = 0;
  int invert = 0, check_names = 1;
  CallStream st, cs;                      // (declared before what runs on them: released after it)
  Staging in[2], out[2];
  SelDev dev[2];
  DevBuf<unsigned long long> pmeta;       // [0] the name cell, [1..4] the PAIR_* cells
  Pinned back;                            // 40 bytes of pmeta per output buffer
  DevBuf<uint8_t> d_out[2][2];            // [mate][buffer]
  Event done[2];                          // the piece gathered into d_out[.][i] is done, its totals are there
  TextDrain drain[2];
  int turn = 0;
  uint64_t offset[2] = {0, 0};            // bytes consumed by the earlier calls of this pair of streams
  uint64_t pair_base = 0;                 // ... and pairs
  int dead = KM_OK;                       // the code a call failed with: every further call fails the same way
  std::string dead_msg;
  km_select_pair_stats_t stats;
  km_select_pair() { memset(&stats, 0, sizeof stats); }
  // never leaves a copy into a freed buffer, or a kernel on a freed one, in flight
  ~km_select_pair() {
    if (h) (void)hipSetDevice(h->device);
    if (st.st) (void)hipStreamSynchronize(st);
    if (cs.st) (void)hipStreamSynchronize(cs);
  }
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
    const int buf = turn;
    turn ^= 1;
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
    for (int m = 0; m < 2; ++m) {
      const uint32_t chunks = (m ? b.n_pad : a.n_pad) / SCAN_CHUNK;
      hipLaunchKernelGGL(k_scan_reduce, dim3(chunks), dim3(SCAN_THREADS), 0, st, dev[m].len.p, dev[m].sums.p);
      hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(SCAN_THREADS), 0, st, dev[m].sums.p, chunks);
      hipLaunchKernelGGL(k_scan_apply, dim3(chunks), dim3(SCAN_THREADS), 0, st, dev[m].len.p, dev[m].sums.p);
    }
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
    KMCHK(drain[0].put(buf ^ 1));         // the piece before, while this one is scanned
    KMCHK(drain[1].put(buf ^ 1));
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
    int rc = KM_OK;
    for (int m = 0; m < 2; ++m) {         // (the older of the two first; either mate's, whatever the other's did)
      int r = drain[m].put(turn);
      if (r == KM_OK) r = drain[m].put(turn ^ 1);
      if (rc == KM_OK) rc = r;
      stats.bytes_out[m] += drain[m].closed;
      drain[m].closed = 0;
    }
    return rc;
  }
};

extern "C" int km_select_pair_create(kmjf_t* h, uint32_t min_hits, int invert, int min_qual_char, int rule, int check_names,
                                     int out_fd1, int out_fd2, void* stream, km_select_pair_t** out) {
  if (!h || !out) return fail(KM_E_ARG, "null argument");
  if (min_hits == 0) return fail(KM_E_ARG, "min_hits must be at least 1");
  KMCHK(select_check_qual(min_qual_char));
  if (rule < 0 || rule >= (int)kmpair::RULE_COUNT) return fail(KM_E_ARG, "pair rule %d is none of any (0), both (1), sum (2)", rule);
  if (out_fd1 == out_fd2) return fail(KM_E_ARG, "the two mates need two descriptors, both are %d", out_fd1);
  if (!h->d_slots) return fail(KM_E_STATE, "table not uploaded");
  KMCHK(dump_check_fd(out_fd1));
  KMCHK(dump_check_fd(out_fd2));
  std::unique_ptr<km_select_pair> s(new (std::nothrow) km_select_pair);
  if (!s) return fail(KM_E_NOMEM, "host allocation failed");
  s->h = h;
  s->min_hits = min_hits;
  s->invert = invert ? 1 : 0;
  s->min_qual = (uint32_t)min_qual_char;
  s->rule = (uint32_t)rule;
  s->check_names = check_names ? 1 : 0;
  KMCHK(s->st.get(h->device, stream));
  KMCHK(s->cs.get(h->device, nullptr));
  KMCHK(s->pmeta.alloc(1 + PAIR_CELLS / 2));
  KMCHK(pinned_alloc(&s->back, 128, "pinned totals"));
  for (int m = 0; m < 2; ++m) {
    KMCHK(s->in[m].alloc(0));
    KMCHK(s->out[m].alloc(1));                          // (room for the newline behind an open last line)
    KMCHK(s->dev[m].alloc(s->in[m].bytes, true, s->st));
    for (int i = 0; i < 2; ++i) KMCHK(s->d_out[m][i].alloc(s->in[m].bytes + kmsel::OUT_PAD));
    s->drain[m].out = &s->out[m];
    s->drain[m].cs = s->cs;
    s->drain[m].fd = m ? out_fd2 : out_fd1;
  }
  for (int i = 0; i < 2; ++i) HIPCHK(hipEventCreateWithFlags(&s->done[i].h, hipEventDisableTiming));
  HIPCHK(hipStreamSynchronize(s->st));
  for (float& v : g_select_ms) v = 0.f;
  *out = s.release();
  return KM_OK;
}

extern "C" int km_select_pair_add_fastq(km_select_pair_t* s, const char* text1, uint64_t n1, const char* text2, uint64_t n2,
                                        int final, uint64_t* consumed1, uint64_t* consumed2) {
  if (!s || !consumed1 || !consumed2 || (n1 && !text1) || (n2 && !text2)) return fail(KM_E_ARG, "null argument");
  if (s->dead != KM_OK) return fail(s->dead, "%s", s->dead_msg.c_str());
  *consumed1 = *consumed2 = 0;
  const char* const text[2] = {text1, text2};
  const uint64_t n[2] = {n1, n2};
  uint64_t end[2], pos[2] = {0, 0};
  for (int m = 0; m < 2; ++m) end[m] = final || n[m] == 0 ? n[m] : kmcut::cut(text[m], n[m]);
  if (end[0] && end[1]) HIPCHK(hipSetDevice(s->h->device));
  int rc = KM_OK;
  while (pos[0] < end[0] && pos[1] < end[1] && rc == KM_OK) {
    uint64_t take[2] = {0, 0}, base[2], used[2] = {0, 0};
    const char* at[2];
    bool ends[2];
    for (int m = 0; m < 2 && rc == KM_OK; ++m) {
      rc = select_take(text[m], pos[m], end[m], s->in[m].bytes, s->offset[m], &take[m]);
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
  const int rc_flush = s->flush();                      // what the pieces before a failure kept is written
  if (rc == KM_OK && rc_flush != KM_OK) {
    rc = rc_flush;
    msg = g_last_error;
  }
  if (rc == KM_OK && final && (pos[0] < end[0]) != (pos[1] < end[1])) {
    rc = fail(KM_E_FORMAT, "mate files differ in their number of records: mate %d has more, the first pair without a partner is pair %llu",
              pos[0] < end[0] ? 1 : 2, (unsigned long long)s->pair_base);
    msg = g_last_error;
  }
  if (rc != KM_OK) {                                    // whatever failed: nothing stays in flight, and the selector
    (void)hipStreamSynchronize(s->st);                  // fails from now on
    (void)hipStreamSynchronize(s->cs);
    s->dead = rc;
    s->dead_msg = msg;
    return fail(rc, "%s", msg.c_str());
  }
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
