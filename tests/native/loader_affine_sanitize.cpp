// Sanitizer driver for the affine entry point of the native shard loader
// (csrc/host/loader.cpp:dcpl_submit_affine), built by tests/test_native_affine_sanitizers_cpu.py
// with -fsanitize=address,undefined and with -fsanitize=thread: every batch in flight on an
// 8-thread pool through the rotate / pad-crop / stretch specs (and the 8-field plain ones), each
// with a heap-allocated matrix buffer of exactly B*8 floats that is freed after the wait; then
// every record, box, angle and matrix checked.  Exit status 0 = all checks passed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ddp_classification_pytorch_amd/csrc/host/loader.cpp"

namespace {
struct HeaderView {
  char magic[8];
  uint32_t version, channels;
  uint64_t count, index_off, data_off, max_bytes;
};
struct EntryView {
  uint64_t offset;
  uint32_t h, w;
  int64_t label;
};
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<uint8_t> file;
  uint8_t buf[1 << 16];
  size_t k;
  while ((k = fread(buf, 1, sizeof(buf), f)) > 0) file.insert(file.end(), buf, buf + k);
  fclose(f);
  HeaderView h;
  memcpy(&h, file.data(), sizeof(h));
  auto entry = [&](int64_t i) {
    EntryView e;
    memcpy(&e, file.data() + h.index_off + i * sizeof(EntryView), sizeof(e));
    return e;
  };

  char err[256];
  void* shard = dcpl_open(argv[1], err, sizeof(err));
  if (!shard) {
    fprintf(stderr, "open: %s\n", err);
    return 4;
  }
  void* pool = dcpl_pool_create(8);
  const int B = 16, NB = 30, OUT_H = 8, OUT_W = 6;  // records are >= 8 px: the pad-crop always fits
  const AugSpec specs[5] = {
      {0, 0, 0, 0.08f, 1.f, 0.75f, 1.333f, 0.5f, 15.f, 0, 12, 10},  // RRC -> rotate -> flip -> centre crop
      {3, 0, 0, 1.f, 1.f, 1.f, 1.f, 0.5f, 0.f, 4, 0, 0},            // RandomCrop(padding=4) -> flip
      {4, 0, 0, 1.f, 1.f, 1.f, 1.f, 0.5f, 0.f, 0, 9, 9},            // stretch -> flip -> centre crop
      {1, 40, 32, 0.08f, 1.f, 0.75f, 1.333f, 0.5f},                 // 8-field: no rotation, no padding
      {2, 0, 0, 1.f, 1.f, 1.f, 1.f, 0.5f}};
  std::vector<std::vector<uint8_t>> outs(NB, std::vector<uint8_t>(B * h.max_bytes));
  std::vector<std::vector<int64_t>> metas(NB, std::vector<int64_t>(B * 8)), labels(NB, std::vector<int64_t>(B));
  std::vector<std::vector<int64_t>> order(NB, std::vector<int64_t>(B));
  std::vector<float*> xfs(NB);
  std::vector<int64_t> tickets(NB);
  for (int b = 0; b < NB; ++b) {
    for (int i = 0; i < B; ++i) order[b][i] = (b * 7 + i * 3) % (int64_t)h.count;
    xfs[b] = static_cast<float*>(malloc(sizeof(float) * B * 8));
    tickets[b] = dcpl_submit_affine(pool, shard, order[b].data(), B, outs[b].data(), (int64_t)outs[b].size(),
                                    metas[b].data(), xfs[b], labels[b].data(), &specs[b % 5], 1234, (uint64_t)b,
                                    OUT_H, OUT_W);
    if (tickets[b] < 0) return 6;
  }
  AugSpec bad = specs[0];
  bad.pad = -1;
  if (dcpl_submit_affine(pool, shard, order[0].data(), B, outs[0].data(), 1, metas[0].data(), xfs[0], labels[0].data(),
                         &specs[0], 1, 0, OUT_H, OUT_W) != -2)
    return 7;  // capacity
  if (dcpl_submit_affine(pool, shard, order[0].data(), 0, outs[0].data(), 0, nullptr, nullptr, nullptr, &bad, 1, 0,
                         OUT_H, OUT_W) != -4)
    return 7;  // spec
  int mism = 0;
  for (int b = NB - 1; b >= 0; --b)
    if (dcpl_wait(pool, tickets[b]) != 0) return 8;
  for (int b = 0; b < NB; ++b) {
    const AugSpec& a = specs[b % 5];
    for (int i = 0; i < B; ++i) {
      const EntryView e = entry(order[b][i]);
      const int64_t* m = metas[b].data() + i * 8;
      const float* t = xfs[b] + i * 8;
      const size_t nb = (size_t)e.h * e.w * 3;
      if (m[1] != e.h || m[2] != e.w || labels[b][i] != e.label) ++mism;
      if (memcmp(outs[b].data() + m[0], file.data() + h.data_off + e.offset, nb) != 0) ++mism;
      if (m[3] < 0 || m[4] < 0 || m[5] < 1 || m[6] < 1 || m[3] + m[5] > m[1] || m[4] + m[6] > m[2]) ++mism;
      for (int j = 0; j < 8; ++j)
        if (!std::isfinite(t[j])) ++mism;
      if (std::fabs(t[6]) > a.rot_deg || t[7] != 0.f) ++mism;
      if (a.rot_deg == 0.f && (t[1] != 0.f || t[3] != 0.f)) ++mism;
      if (a.mode == 3) {  // scale 1: integer offsets within [-pad, H + pad - out]
        const float dx = m[7] ? t[2] - (OUT_W - 1) : t[2], dy = t[5];
        if (dx != std::floor(dx) || dx < -a.pad || dx > (float)m[2] + a.pad - OUT_W) ++mism;
        if (dy != std::floor(dy) || dy < -a.pad || dy > (float)m[1] + a.pad - OUT_H) ++mism;
      }
    }
    free(xfs[b]);
  }
  dcpl_pool_destroy(pool);
  dcpl_close(shard);
  if (mism) fprintf(stderr, "%d mismatches\n", mism);
  printf("loader_affine_sanitize ok=%d\n", mism == 0);
  return mism ? 9 : 0;
}
