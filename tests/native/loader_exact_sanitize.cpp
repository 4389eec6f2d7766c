// Sanitizer driver for the exact entry point of the native shard loader
// (csrc/host/loader.cpp:dcpl_submit_exact), built by tests/test_native_exact_sanitizers_cpu.py with
// -fsanitize=address,undefined and with -fsanitize=thread: every batch in flight on an 8-thread
// pool through the rotate / stretch / Resize+CenterCrop / plain specs, each with a heap-allocated
// geometry buffer of exactly B*12 int32 that is freed after the wait; then every record, box,
// canvas, window offset and rotation integer checked, and the refusals.  Exit status 0 = all passed.
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
  const int B = 16, NB = 30, OUT_H = 8, OUT_W = 8;  // records are 8..59 px: every canvas is within 8x
  const AugSpec specs[5] = {
      {0, 0, 0, 0.08f, 1.f, 0.75f, 1.333f, 0.5f, 15.f, 0, 12, 10, 0},  // RRC -> rotate -> flip -> centre crop
      {4, 0, 0, 1.f, 1.f, 1.f, 1.f, 0.5f, 0.f, 0, 9, 9, 1},            // bicubic stretch -> flip -> centre crop
      {1, 12, 8, 0.f, 0.f, 1.f, 1.f, 0.f},                             // Resize(12) + CenterCrop
      {0, 0, 0, 0.08f, 1.f, 0.75f, 1.333f, 0.5f},                      // RRC + flip, canvas = output
      {2, 0, 0, 1.f, 1.f, 1.f, 1.f, 0.5f}};
  std::vector<std::vector<uint8_t>> outs(NB, std::vector<uint8_t>(B * h.max_bytes));
  std::vector<std::vector<int64_t>> metas(NB, std::vector<int64_t>(B * 8)), labels(NB, std::vector<int64_t>(B));
  std::vector<std::vector<int64_t>> order(NB, std::vector<int64_t>(B));
  std::vector<int32_t*> geos(NB);
  std::vector<int64_t> tickets(NB);
  for (int b = 0; b < NB; ++b) {
    for (int i = 0; i < B; ++i) order[b][i] = (b * 7 + i * 3) % (int64_t)h.count;
    geos[b] = static_cast<int32_t*>(malloc(sizeof(int32_t) * B * 12));
    tickets[b] = dcpl_submit_exact(pool, shard, order[b].data(), B, outs[b].data(), (int64_t)outs[b].size(),
                                   metas[b].data(), geos[b], labels[b].data(), &specs[b % 5], 1234, (uint64_t)b,
                                   OUT_H, OUT_W);
    if (tickets[b] < 0) return 6;
  }
  // refusals by code: capacity, index, the pad-crop mode, an empty output
  AugSpec bad = specs[0];
  bad.mode = 3;
  int64_t past = (int64_t)h.count;
  if (dcpl_submit_exact(pool, shard, order[0].data(), B, outs[0].data(), 1, metas[0].data(), geos[0],
                        labels[0].data(), &specs[0], 1, 0, OUT_H, OUT_W) != -2)
    return 7;
  if (dcpl_submit_exact(pool, shard, &past, 1, outs[0].data(), (int64_t)outs[0].size(), nullptr, nullptr, nullptr,
                        &specs[0], 1, 0, OUT_H, OUT_W) != -3)
    return 7;
  if (dcpl_submit_exact(pool, shard, order[0].data(), 0, outs[0].data(), 0, nullptr, nullptr, nullptr, &bad, 1, 0,
                        OUT_H, OUT_W) != -4)
    return 7;
  if (dcpl_submit_exact(pool, shard, order[0].data(), 0, outs[0].data(), 0, nullptr, nullptr, nullptr, &specs[0], 1,
                        0, 0, OUT_W) != -4)
    return 7;
  int mism = 0;
  for (int b = NB - 1; b >= 0; --b)
    if (dcpl_wait(pool, tickets[b]) != 0) return 8;
  for (int b = 0; b < NB; ++b) {
    const AugSpec& a = specs[b % 5];
    for (int i = 0; i < B; ++i) {
      const EntryView e = entry(order[b][i]);
      const int64_t* m = metas[b].data() + i * 8;
      const int32_t* g = geos[b] + i * 12;
      const size_t nb = (size_t)e.h * e.w * 3;
      if (m[1] != e.h || m[2] != e.w || labels[b][i] != e.label) ++mism;
      if (memcmp(outs[b].data() + m[0], file.data() + h.data_off + e.offset, nb) != 0) ++mism;
      if (m[3] < 0 || m[4] < 0 || m[5] < 1 || m[6] < 1 || m[3] + m[5] > m[1] || m[4] + m[6] > m[2]) ++mism;
      float theta;
      memcpy(&theta, g + 11, sizeof(theta));
      if (!(std::fabs(theta) <= a.rot_deg) || g[10] != (a.rot_deg > 0.f)) ++mism;
      if (a.mode == 1) {  // the whole record, short side 12
        if (m[3] != 0 || m[4] != 0 || m[5] != e.h || m[6] != e.w || std::min(g[0], g[1]) != 12) ++mism;
      } else if (g[0] != (a.canvas_h ? a.canvas_h : OUT_H) || g[1] != (a.canvas_w ? a.canvas_w : OUT_W)) {
        ++mism;
      }
      if (g[2] != (int)std::nearbyint((g[0] - OUT_H) / 2.0)) ++mism;
      if (g[3] != (int)std::nearbyint((g[1] - OUT_W) / 2.0)) ++mism;
      // the map is [c s; -s c] in 16.16, the identity at angle 0
      if (g[4] != g[8] || std::abs(g[5] + g[7]) > 1 || std::abs(g[4]) > 65536 || std::abs(g[5]) > 65536) ++mism;
      if (theta == 0.f && (g[4] != 65536 || g[5] != 0 || g[6] != 32768 || g[9] != 32768)) ++mism;
    }
    free(geos[b]);
  }
  // a box more than 8x its canvas fails the ticket (code 6), it is not resampled with a cut filter
  {
    const AugSpec tiny = {4, 0, 0, 1.f, 1.f, 1.f, 1.f, 0.f, 0.f, 0, 1, 1, 0};
    std::vector<int32_t> g(B * 12);
    int64_t t = dcpl_submit_exact(pool, shard, order[0].data(), B, outs[0].data(), (int64_t)outs[0].size(),
                                  metas[0].data(), g.data(), labels[0].data(), &tiny, 1, 0, 1, 1);
    if (t < 0 || dcpl_wait(pool, t) != 6) ++mism;
  }
  dcpl_pool_destroy(pool);
  dcpl_close(shard);
  if (mism) fprintf(stderr, "%d mismatches\n", mism);
  printf("loader_exact_sanitize ok=%d\n", mism == 0);
  return mism ? 9 : 0;
}
