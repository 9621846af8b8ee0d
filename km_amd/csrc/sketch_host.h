// sketch_host.h — km_sketch_words, km_sketch_slot, km_counter_set_sketch, km_counter_sketch_done,
// km_counter_sketch_stats (host part of kmgpu.hip; device side: sketch_kernel.h; the rule: sketch_rule.h; where a counter
// with a sketch differs on its way through count_host.h: its CountMode in launch_insert, counter_table_fixed,
// counter_sketch_settled)
// ------------------------------------------------------------------ solid k-mers in two passes
// A counter with a sketch is fed twice.  In the first pass (COUNT_SKETCH_NOTE) the text takes its usual way through the
// staging, and through the line table and mask of a FASTQ piece, but the kernel at the end of it notes every window's
// key in the sketch and the table is neither touched nor grown.  km_counter_sketch_done ends that pass and makes the
// counter's stream state that of a counter that has not been fed; from then on (COUNT_SKETCH_COUNT) the kernel is the plain
// insert kernel with one more condition, and counter_reserve grows the table on its exact occupancy as always, which
// now is that of the admitted keys.
// The set bits of the two planes into their meta cells (the caller reads the meta block next).
static int sketch_fill(km_counter* c) {
  HIPCHK(hipMemsetAsync(c->meta.p + CM_BITS_1, 0, 16, c->st));       // CM_BITS_1 and CM_BITS_2 are neighbours
  hipLaunchKernelGGL(k_sketch_fill, dim3(grid_for(c->sketch_words, SKETCH_THREADS)), dim3(SKETCH_THREADS), 0, c->st,
                     c->sketch.p, c->sketch_words, c->meta.p);
  HIPCHK(hipGetLastError());
  return KM_OK;
}
static_assert(CM_BITS_2 == CM_BITS_1 + 1, "sketch_fill clears the two cells in one call");

extern "C" int km_sketch_words(uint64_t expected_distinct, uint64_t* words) {
  if (!words) return fail(KM_E_ARG, "null argument");
  if (expected_distinct > 2 * kmsketch::MAX_WORDS)
    return fail(KM_E_ARG, "%llu expected k-mers: a sketch has at most 2^40 words", (unsigned long long)expected_distinct);
  *words = kmsketch::sketch_words_for(expected_distinct);
  return KM_OK;
}

extern "C" int km_sketch_slot(uint64_t key, uint64_t words, uint64_t* word, uint32_t* mask) {
  if (!word || !mask) return fail(KM_E_ARG, "null argument");
  if (!kmsketch::words_valid(words))
    return fail(KM_E_ARG, "a sketch of %llu words: a power of two from 64 to 2^40 is needed", (unsigned long long)words);
  const kmsketch::Slot s = kmsketch::slot_of(key, 64u - kmsketch::log2_words(words));
  *word = s.word;
  *mask = s.mask;
  return KM_OK;
}

extern "C" int km_counter_set_sketch(km_counter_t* c, uint64_t words) {
  if (!c) return fail(KM_E_ARG, "null argument");
  if (!kmsketch::words_valid(words))
    return fail(KM_E_ARG, "a sketch of %llu words: a power of two from 64 to 2^40 is needed", (unsigned long long)words);
  KMCHK(counter_usable(c));
  if (counter_has_sketch(c)) return fail(KM_E_STATE, "counter already has a sketch");
  if (counter_has_filter(c)) return fail(KM_E_STATE, "counter has a filter: it takes no sketch");
  if (c->feed != FEED_NONE) return fail(KM_E_STATE, "counter has been fed: the sketch comes before the first add_* or set_* call");
  HIPCHK(hipSetDevice(c->device));
  DevBuf<uint64_t> sketch;
  uint32_t blocks = 0;
  KMCHK(sketch.alloc(words));
  KMCHK(filter_grid_cap(c->device, COUNT_SKETCH_NOTE, &blocks));   // (filter_host.h: eight blocks of four waves per CU)
  HIPCHK(hipMemsetAsync(sketch.p, 0, words * 8, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  c->sketch = std::move(sketch);
  c->sketch_words = words;
  c->grid_cap = blocks;
  c->mode = COUNT_SKETCH_NOTE;
  return KM_OK;
}

extern "C" int km_counter_sketch_done(km_counter_t* c) {
  if (!c) return fail(KM_E_ARG, "null argument");
  KMCHK(counter_usable(c));
  if (!counter_has_sketch(c)) return fail(KM_E_STATE, "counter has no sketch");
  if (c->mode == COUNT_SKETCH_COUNT) return fail(KM_E_STATE, "the sketch's first pass has ended already");
  HIPCHK(hipSetDevice(c->device));
  KMCHK(counter_flush(c));
  KMCHK(sketch_fill(c));                                // (nothing writes the sketch from here on: the bits are final)
  unsigned long long m[CM_WORDS];
  KMCHK(counter_read_meta(c, m));                       // (waits; a malformed FASTQ record of this pass is reported here)
  KMCHK(c->insert_spans.drain(&c->sketch_note_ms));
  c->insert_spans.ms = 0.f;
  // the second pass is a stream of its own, from its first byte
  c->text = km_text_state_t{0, 0, 0, 0, 0};
  c->fill = 0;
  c->own_from = 0;
  c->fq_offset = 0;
  c->mode = COUNT_SKETCH_COUNT;
  return KM_OK;
}

extern "C" int km_counter_sketch_stats(km_counter_t* c, uint64_t* words, uint64_t* bits_1, uint64_t* bits_2,
                                       uint64_t* kmers_noted, uint64_t* kmers_admitted, float* kernel_ms) {
  if (!c) return fail(KM_E_ARG, "null argument");
  if (c->fq_error != FQ_NO_ERROR) return counter_format_failed(c);
  HIPCHK(hipSetDevice(c->device));
  if (!c->finished) KMCHK(counter_flush(c));
  if (c->mode == COUNT_SKETCH_NOTE) KMCHK(sketch_fill(c));
  unsigned long long m[CM_WORDS];
  KMCHK(counter_read_meta(c, m));
  float ms = 0.f;
  KMCHK(c->insert_spans.drain(&ms));
  if (words) *words = c->sketch_words;
  if (bits_1) *bits_1 = m[CM_BITS_1];
  if (bits_2) *bits_2 = m[CM_BITS_2];
  if (kmers_noted) *kmers_noted = m[CM_NOTED];
  if (kmers_admitted) *kmers_admitted = m[CM_ADMITTED];
  if (kernel_ms) {
    kernel_ms[0] = c->mode == COUNT_SKETCH_NOTE ? ms : c->sketch_note_ms;
    kernel_ms[1] = c->mode == COUNT_SKETCH_COUNT ? ms : 0.f;
  }
  return KM_OK;
}
