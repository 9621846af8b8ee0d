// kmin_host.h — km_linear_kmin (host part of kmgpu.hip; device side: kmin_kernel.h)
// ------------------------------------------------------------------ linear_kmin
// km/tools/linear_kmin.py:7-46 for a whole catalog: one launch per staging chunk (kmin_kernel.h), then the
// closed form of DESIGN.md §9 on the host (kmin_rule.h).
#include "kmin_rule.h"

namespace {
constexpr uint64_t KMIN_STAGE_BYTES = 256ull << 20;   // staged text per launch (a longer target goes alone)
}  // namespace

extern "C" int km_linear_kmin(int device, const uint8_t* bases, const uint64_t* base_off, uint32_t n_targets,
                              int32_t start, int32_t* kmin, int32_t* longest_repeat, uint8_t* nonexempt,
                              void* stream) {
  if (!base_off || !kmin) return fail(KM_E_ARG, "null argument");
  for (uint32_t t = 0; t < n_targets; ++t) {
    if (base_off[t + 1] < base_off[t]) return fail(KM_E_ARG, "offsets must be non-decreasing (target %u)", t);
    if (base_off[t + 1] - base_off[t] > 0x7FFFFFFFull) return fail(KM_E_ARG, "target %u longer than 2^31 - 1", t);
  }
  if (n_targets && base_off[n_targets] > base_off[0] && !bases) return fail(KM_E_ARG, "null argument");
  if (n_targets == 0) return KM_OK;

  // chunks of targets whose 16-byte aligned text fits the staging size (at least one target each);
  // KM_KMIN_STAGE_BYTES lowers it so that tests reach the multi-chunk path with a small catalog
  uint64_t stage_bytes = KMIN_STAGE_BYTES;
  if (const char* e = getenv("KM_KMIN_STAGE_BYTES")) stage_bytes = std::max<uint64_t>(16, strtoull(e, nullptr, 10));
  std::vector<uint32_t> chunk_first{0};
  uint64_t bytes = 0, max_bytes = 0;
  uint32_t max_targets = 0;
  for (uint32_t t = 0; t < n_targets; ++t) {
    const uint64_t b = (base_off[t + 1] - base_off[t] + 15) & ~15ull;
    if (bytes && bytes + b > stage_bytes) {
      max_targets = std::max(max_targets, t - chunk_first.back());
      chunk_first.push_back(t);
      bytes = 0;
    }
    bytes += b;
    max_bytes = std::max(max_bytes, bytes);
  }
  max_targets = std::max(max_targets, n_targets - chunk_first.back());
  chunk_first.push_back(n_targets);

  CallStream st;
  KMCHK(st.get(device, stream));

  struct {
    DevBuf<uint8_t> text;
    DevBuf<uint64_t> stage_off;
    DevBuf<uint32_t> len, unit_off;
    DevBuf<unsigned long long> keys;
  } dev;
  int rc = dev.text.alloc(max_bytes + KMIN_PAD);
  if (rc == KM_OK) rc = dev.stage_off.alloc(max_targets);
  if (rc == KM_OK) rc = dev.len.alloc(max_targets);
  if (rc == KM_OK) rc = dev.unit_off.alloc(max_targets + 1);
  if (rc == KM_OK) rc = dev.keys.alloc(max_targets);
  if (rc != KM_OK) return rc;
  std::vector<uint8_t> h_text;
  std::vector<uint64_t> h_off, h_keys;
  std::vector<uint32_t> h_len, h_units;
  for (size_t c = 0; c + 1 < chunk_first.size(); ++c) {
    const uint32_t t0 = chunk_first[c], nt = chunk_first[c + 1] - t0;
    h_off.resize(nt);
    h_len.resize(nt);
    h_units.resize(nt + 1);
    uint64_t pos = 0;
    uint32_t units = 0;
    for (uint32_t i = 0; i < nt; ++i) {
      const uint64_t n = base_off[t0 + i + 1] - base_off[t0 + i];
      h_off[i] = pos;
      h_len[i] = (uint32_t)n;
      h_units[i] = units;
      units += n >= 2 ? (uint32_t)((n - 1 + KMIN_LANES - 1) / KMIN_LANES) : 0;
      pos += (n + 15) & ~15ull;
    }
    h_units[nt] = units;
    h_text.assign(pos + KMIN_PAD, 0);
    for (uint32_t i = 0; i < nt; ++i)
      if (h_len[i]) memcpy(h_text.data() + h_off[i], bases + base_off[t0 + i], h_len[i]);
    HIPCHK(hipMemcpyAsync(dev.text, h_text.data(), h_text.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dev.stage_off, h_off.data(), 8ull * nt, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dev.len, h_len.data(), 4ull * nt, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dev.unit_off, h_units.data(), 4ull * (nt + 1), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(dev.keys, 0, 8ull * nt, st));
    if (units) {
      const uint32_t blocks = (units + KMIN_WAVES_PER_BLOCK - 1) / KMIN_WAVES_PER_BLOCK;
      hipLaunchKernelGGL(k_linear_kmin, dim3(blocks), dim3(KMIN_LANES * KMIN_WAVES_PER_BLOCK), 0, st,
                         dev.text, dev.stage_off, dev.len, dev.unit_off, nt, units, dev.keys);
      HIPCHK(hipGetLastError());
    }
    h_keys.resize(nt);
    HIPCHK(hipMemcpyAsync(h_keys.data(), dev.keys, 8ull * nt, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (uint32_t i = 0; i < nt; ++i) {
      const uint64_t R = h_keys[i] >> 1;
      uint8_t flag = (uint8_t)(h_keys[i] & 1);
      kmin[t0 + i] = kmlin::kmin_closed_form(h_len[i], start, R, &flag);
      if (longest_repeat) longest_repeat[t0 + i] = (int32_t)R;
      if (nonexempt) nonexempt[t0 + i] = flag;
    }
  }
  return KM_OK;
}
