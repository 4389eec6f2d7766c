// Native batch loader for pre-decoded image shards (host C++, no device code).
//
// Reference behaviour being replaced: the torch DataLoader of BASELINE/main.py:127-131 (4 worker
// processes, each PIL-decoding a JPEG, running RandomResizedCrop(256, scale=(0.8, 1)) /
// Resize(256)+CenterCrop(224) (BASELINE/main.py:58-76) and ToTensor/Normalize on the CPU, then a
// pin-memory thread and `inputs.cuda(non_blocking=True)` (:273-274)).  A handful of host cores
// cannot decode and augment JPEGs at the ~14k img/s one MI355X trains ResNet-50 at, so the work
// is split differently here:
//
//   * images are decoded ONCE, offline, into a shard file of raw uint8 HWC records
//     (`data/shards.py:write_shard`); the loader memory-maps it;
//   * a pool of std::threads gathers the records of one batch (in the order the distributed
//     sampler produced) into a caller-owned pinned buffer and samples each image's augmentation
//     (RandomResizedCrop box with torchvision's 10-attempt algorithm, horizontal flip, or the
//     Resize+CenterCrop box of the eval transform) from a counter-based RNG keyed by
//     (seed, epoch, dataset index), so results do not depend on thread scheduling;
//   * the crop/resize/flip itself runs on the GPU (`dcp::crop_resize_kernel`) after one
//     H2D copy of the raw records, feeding the existing normalise/NHWC input kernel;
//   * presets that rotate or pad (CDR/main.py:112-130, NESTED/train.py:40-45 on CIFAR,
//     PLC/FolderDataset.py) go through dcpl_submit_affine: the same gather and box, plus one
//     inverse-affine matrix per image that composes resize-to-canvas, rotation about the canvas
//     centre, flip and the crop offset, resampled on the GPU by `dcp::warp_crop_kernel`;
//   * the opt-in `pil` resampling mode goes through dcpl_submit_exact: the same gather and draws, plus
//     the integers of the PIL chain itself per image (canvas size, window offset, the 16.16 map of
//     Image.rotate), for `dcp::resample_crop_kernel` / `dcp::rotate_nearest_crop_kernel`, which
//     reproduce Pillow's resize and rotate bit for bit.
//
// C ABI (ctypes, see data/shards.py): dcpl_open / dcpl_close / dcpl_count / dcpl_pool_create /
// dcpl_pool_destroy / dcpl_submit / dcpl_submit_affine / dcpl_submit_exact / dcpl_wait.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fcntl.h>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <sys/mman.h>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include <vector>

namespace {

constexpr char kMagic[8] = {'D', 'C', 'P', 'S', 'H', 'R', 'D', '1'};

#pragma pack(push, 1)
struct Header {        // 48 bytes at offset 0
  char magic[8];
  uint32_t version;    // 1
  uint32_t channels;   // 3
  uint64_t count;
  uint64_t index_off;  // byte offset of `count` IndexEntry records
  uint64_t data_off;   // byte offset of the image records
  uint64_t max_bytes;  // largest record (h*w*c)
};
struct IndexEntry {    // 24 bytes per image
  uint64_t offset;     // relative to data_off
  uint32_t h, w;
  int64_t label;
};
#pragma pack(pop)
static_assert(sizeof(Header) == 48, "header layout");
static_assert(sizeof(IndexEntry) == 24, "index layout");

struct Shard {
  int fd = -1;
  size_t size = 0;
  const uint8_t* base = nullptr;
  const Header* hdr = nullptr;
  const IndexEntry* index = nullptr;
  const uint8_t* data = nullptr;
  ~Shard() {
    if (base) munmap(const_cast<uint8_t*>(base), size);
    if (fd >= 0) close(fd);
  }
};

// Augmentation spec shared with Python (ctypes.Structure in data/shards.py).
// The fields after flip_p are read by dcpl_submit_affine and dcpl_submit_exact only; an 8-field
// initialiser leaves them zero: no rotation, no padding, canvas = output, bilinear.
struct AugSpec {
  int32_t mode;         // 0 = RandomResizedCrop (+flip), 1 = Resize(resize)+CenterCrop(crop), 2 = whole image,
                        // 3 = RandomCrop(out, padding=pad) of the image itself, 4 = whole image stretched to the canvas
  int32_t resize;       // mode 1: shorter side after resize
  int32_t crop;         // mode 1: centre crop edge (in resized pixels)
  float scale_lo, scale_hi;  // mode 0: area fraction range
  float ratio_lo, ratio_hi;  // mode 0: aspect ratio range
  float flip_p;         // horizontal flip probability (every mode but 1)
  float rot_deg;        // RandomRotation(rot_deg) about the canvas centre; 0 = none
  int32_t pad;          // mode 3: zero padding on every side
  int32_t canvas_h, canvas_w;  // the box is resized to this canvas, the output is its centre crop; 0 = output size
  int32_t filter;       // `pil` resampling mode, read by the device side only: 0 = bilinear, 1 = bicubic
};

// splitmix64 / counter-based stream: one independent stream per (seed, epoch, dataset index)
struct Rng {
  uint64_t s;
  explicit Rng(uint64_t key) : s(key) {}
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double uniform() { return (next() >> 11) * (1.0 / 9007199254740992.0); }  // [0, 1)
  int64_t randint(int64_t lo, int64_t hi) {                                 // [lo, hi)
    return lo + static_cast<int64_t>(uniform() * static_cast<double>(hi - lo));
  }
};

inline uint64_t mix_key(uint64_t seed, uint64_t epoch, uint64_t idx) {
  Rng r(seed * 0x100000001B3ull ^ (epoch + 0x51ED27ull) * 0x2545F4914F6CDD1Dull);
  uint64_t a = r.next();
  Rng r2(a ^ (idx * 0xD1B54A32D192ED03ull));
  return r2.next();
}

// torchvision.transforms.RandomResizedCrop.get_params (10 attempts, then the centre fallback).
void rrc_box(Rng& rng, int H, int W, const AugSpec& a, int out[4]) {
  const double area = static_cast<double>(H) * W;
  const double lr0 = std::log(a.ratio_lo), lr1 = std::log(a.ratio_hi);
  for (int t = 0; t < 10; ++t) {
    double target = area * (a.scale_lo + rng.uniform() * (a.scale_hi - a.scale_lo));
    double ar = std::exp(lr0 + rng.uniform() * (lr1 - lr0));
    int w = static_cast<int>(std::lround(std::sqrt(target * ar)));
    int h = static_cast<int>(std::lround(std::sqrt(target / ar)));
    if (w > 0 && h > 0 && w <= W && h <= H) {
      int i = static_cast<int>(rng.randint(0, H - h + 1));
      int j = static_cast<int>(rng.randint(0, W - w + 1));
      out[0] = i, out[1] = j, out[2] = h, out[3] = w;
      return;
    }
  }
  double in_ratio = static_cast<double>(W) / H;
  int w, h;
  if (in_ratio < a.ratio_lo) {
    w = W, h = static_cast<int>(std::lround(w / a.ratio_lo));
  } else if (in_ratio > a.ratio_hi) {
    h = H, w = static_cast<int>(std::lround(h * a.ratio_hi));
  } else {
    w = W, h = H;
  }
  out[0] = (H - h) / 2, out[1] = (W - w) / 2, out[2] = h, out[3] = w;
}

// Resize(shorter side -> resize) + CenterCrop(crop), expressed as a box in source pixels.
void center_box(int H, int W, const AugSpec& a, int out[4]) {
  double s = static_cast<double>(a.resize) / std::min(H, W);  // source -> resized scale
  int ch = std::min(H, static_cast<int>(std::lround(a.crop / s)));
  int cw = std::min(W, static_cast<int>(std::lround(a.crop / s)));
  out[0] = (H - ch) / 2, out[1] = (W - cw) / 2, out[2] = ch, out[3] = cw;
}

// The inverse map of "resize the h x w box to an Sh x Sw canvas, rotate by theta degrees about the
// canvas centre (PIL Image.rotate: counter-clockwise, cos/sin rounded to 15 digits), flip, crop
// out_w columns at offset (dx, dy)": output pixel (ox, oy) -> box-relative source position
// (sx, sy) = (m[0]*ox + m[1]*oy + m[2], m[3]*ox + m[4]*oy + m[5]), box pixel k centred at k.
void affine_matrix(int h, int w, int Sh, int Sw, int out_w, double dx, double dy, double theta, int flip,
                   float m[6]) {
  const double a = -theta * 3.14159265358979323846 / 180.0;
  const double ca = std::round(std::cos(a) * 1e15) / 1e15, sa = std::round(std::sin(a) * 1e15) / 1e15;
  const double cx = Sw / 2.0, cy = Sh / 2.0, kx = static_cast<double>(w) / Sw, ky = static_cast<double>(h) / Sh;
  const double fs = flip ? -1.0 : 1.0, f0 = flip ? out_w - 1.0 : 0.0;
  const double px0 = f0 + 0.5 + dx - cx, py0 = 0.5 + dy - cy;  // (px - cx, py - cy) at ox = oy = 0
  m[0] = static_cast<float>(ca * fs * kx);
  m[1] = static_cast<float>(sa * kx);
  m[2] = static_cast<float>((cx + ca * px0 + sa * py0) * kx - 0.5);
  m[3] = static_cast<float>(-sa * fs * ky);
  m[4] = static_cast<float>(ca * ky);
  m[5] = static_cast<float>((cy - sa * px0 + ca * py0) * ky - 0.5);
}

// Python's round(v, 15): both it and printf/strtod round the exact binary value correctly, which
// round(v * 1e15) / 1e15 does not always.
double round15(double v) {
  char buf[64];
  snprintf(buf, sizeof(buf), "%.15f", v);
  return std::strtod(buf, nullptr);
}

// The six 16.16 integers of PIL's Image.rotate(theta, NEAREST) on an Sh x Sw canvas, as Image.py and
// Geometry.c compute them: output (x, y) reads canvas ((a2 + a1*y + a0*x) >> 16, (a5 + a4*y + a3*x) >> 16).
// Every line is one double operation per operator (the library is built with -ffp-contract=off).
void rotate_fix16(double theta, int Sh, int Sw, int32_t a[6]) {
  double deg = std::fmod(theta, 360.0);  // Python's theta % 360.0
  if (deg < 0.0) deg += 360.0;
  const double ang = -(deg * (3.14159265358979323846 / 180.0));
  const double c = round15(std::cos(ang)), s = round15(std::sin(ang));
  const double cx = Sw / 2.0, cy = Sh / 2.0;
  const double m2 = c * (-cx) + s * (-cy) + 0.0 + cx;
  const double m5 = (-s) * (-cx) + c * (-cy) + 0.0 + cy;
  auto fix = [](double v) { return static_cast<int32_t>(std::floor(v * 65536.0 + 0.5)); };
  a[0] = fix(c), a[1] = fix(s), a[2] = fix(m2 + c * 0.5 + s * 0.5);
  a[3] = fix(-s), a[4] = fix(c), a[5] = fix(m5 + (-s) * 0.5 + c * 0.5);
}

class Pool {
 public:
  explicit Pool(int n) {
    for (int i = 0; i < std::max(1, n); ++i) threads_.emplace_back([this] { run(); });
  }
  ~Pool() {
    {
      std::lock_guard<std::mutex> g(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : threads_) t.join();
  }
  // Enqueue `n` jobs fn(0..n-1) as one ticket.
  int64_t submit(int n, std::function<int(int)> fn) {
    auto tk = std::make_shared<Ticket>();
    tk->left = n;
    tk->fn = std::move(fn);
    int64_t id;
    {
      std::lock_guard<std::mutex> g(mu_);
      id = next_id_++;
      tickets_[id] = tk;
      for (int i = 0; i < n; ++i) q_.push_back({tk, i});
    }
    cv_.notify_all();
    if (n == 0) {
      std::lock_guard<std::mutex> g(tk->mu);
      tk->done = true;
    }
    return id;
  }
  int wait(int64_t id) {
    std::shared_ptr<Ticket> tk;
    {
      std::lock_guard<std::mutex> g(mu_);
      auto it = tickets_.find(id);
      if (it == tickets_.end()) return -1;
      tk = it->second;
      tickets_.erase(it);
    }
    std::unique_lock<std::mutex> l(tk->mu);
    tk->cv.wait(l, [&] { return tk->done; });
    return tk->err.load();
  }

 private:
  struct Ticket {
    std::mutex mu;
    std::condition_variable cv;
    int left = 0;
    bool done = false;
    std::atomic<int> err{0};
    std::function<int(int)> fn;
  };
  struct Job {
    std::shared_ptr<Ticket> tk;
    int i;
  };
  void run() {
    for (;;) {
      Job j;
      {
        std::unique_lock<std::mutex> l(mu_);
        cv_.wait(l, [&] { return stop_ || !q_.empty(); });
        if (stop_ && q_.empty()) return;
        j = q_.front();
        q_.pop_front();
      }
      int rc = j.tk->fn(j.i);
      if (rc != 0) j.tk->err.store(rc);
      std::lock_guard<std::mutex> g(j.tk->mu);
      if (--j.tk->left == 0) {
        j.tk->done = true;
        j.tk->cv.notify_all();
      }
    }
  }
  std::vector<std::thread> threads_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<Job> q_;
  std::map<int64_t, std::shared_ptr<Ticket>> tickets_;
  int64_t next_id_ = 1;
  bool stop_ = false;
};

}  // namespace

extern "C" {

void* dcpl_open(const char* path, char* err, int errlen) {
  auto fail = [&](const std::string& m) -> void* {
    if (err && errlen > 0) snprintf(err, errlen, "%s: %s", path, m.c_str());
    return nullptr;
  };
  auto s = std::make_unique<Shard>();
  s->fd = open(path, O_RDONLY);
  if (s->fd < 0) return fail("cannot open");
  struct stat st;
  if (fstat(s->fd, &st) != 0) return fail("cannot stat");
  s->size = static_cast<size_t>(st.st_size);
  if (s->size < sizeof(Header)) return fail("truncated header");
  void* p = mmap(nullptr, s->size, PROT_READ, MAP_SHARED, s->fd, 0);
  if (p == MAP_FAILED) return fail("mmap failed");
  s->base = static_cast<const uint8_t*>(p);
  s->hdr = reinterpret_cast<const Header*>(s->base);
  const Header& h = *s->hdr;
  if (std::memcmp(h.magic, kMagic, 8) != 0 || h.version != 1 || h.channels != 3) return fail("bad magic/version");
  if (h.index_off + h.count * sizeof(IndexEntry) > s->size || h.data_off > s->size) return fail("truncated index");
  s->index = reinterpret_cast<const IndexEntry*>(s->base + h.index_off);
  s->data = s->base + h.data_off;
  for (uint64_t i = 0; i < h.count; ++i) {
    const IndexEntry& e = s->index[i];
    uint64_t nb = uint64_t(e.h) * e.w * 3;
    if (e.h == 0 || e.w == 0 || nb > h.max_bytes || h.data_off + e.offset + nb > s->size)
      return fail("record " + std::to_string(i) + " out of bounds");
  }
  madvise(p, s->size, MADV_RANDOM);
  return s.release();
}

void dcpl_close(void* shard) { delete static_cast<Shard*>(shard); }

int64_t dcpl_count(void* shard) { return static_cast<int64_t>(static_cast<Shard*>(shard)->hdr->count); }

void* dcpl_pool_create(int nthreads) { return new Pool(nthreads); }

void dcpl_pool_destroy(void* pool) { delete static_cast<Pool*>(pool); }

// Gather the records `indices[0..B)` into `out` (capacity `out_cap` bytes; record b starts at
// b * max_bytes) and write per-image metadata meta[b*8 .. b*8+8) =
// {byte offset in out, H, W, crop y0, crop x0, crop h, crop w, flip}; labels[b] = label.
// Returns a ticket for dcpl_wait (negative on argument errors).
int64_t dcpl_submit(void* pool, void* shard, const int64_t* indices, int B, uint8_t* out, int64_t out_cap,
                    int64_t* meta, int64_t* labels, const AugSpec* aug, uint64_t seed, uint64_t epoch) {
  auto* s = static_cast<Shard*>(shard);
  const uint64_t stride = s->hdr->max_bytes;
  if (B < 0 || static_cast<uint64_t>(B) * stride > static_cast<uint64_t>(out_cap)) return -2;
  for (int b = 0; b < B; ++b)
    if (indices[b] < 0 || static_cast<uint64_t>(indices[b]) >= s->hdr->count) return -3;
  std::vector<int64_t> idx(indices, indices + B);
  AugSpec a = *aug;
  return static_cast<Pool*>(pool)->submit(B, [=](int b) -> int {
    const IndexEntry& e = s->index[idx[b]];
    const int H = static_cast<int>(e.h), W = static_cast<int>(e.w);
    std::memcpy(out + b * stride, s->data + e.offset, size_t(H) * W * 3);
    Rng rng(mix_key(seed, epoch, static_cast<uint64_t>(idx[b])));
    int box[4];
    int flip = 0;
    if (a.mode == 0) {
      rrc_box(rng, H, W, a, box);
      flip = rng.uniform() < a.flip_p;
    } else if (a.mode == 1) {
      center_box(H, W, a, box);
    } else {
      box[0] = 0, box[1] = 0, box[2] = H, box[3] = W;
      flip = rng.uniform() < a.flip_p;
    }
    int64_t* m = meta + b * 8;
    m[0] = static_cast<int64_t>(b * stride);
    m[1] = H, m[2] = W, m[3] = box[0], m[4] = box[1], m[5] = box[2], m[6] = box[3], m[7] = flip;
    labels[b] = e.label;
    return 0;
  });
}

// dcpl_submit for the presets that rotate, pad or resize to a canvas other than the output: the
// same gather, meta and labels, plus xf[b*8 .. b*8+8) = {m00, m01, m02, m10, m11, m12, angle_deg, 0}
// (affine_matrix above) for an out_h x out_w output.  Draws per image, from the same
// (seed, epoch, index) stream: the mode's own, then the angle (only if rot_deg > 0), then the flip --
// so a spec without rotation and padding writes the meta dcpl_submit writes.
int64_t dcpl_submit_affine(void* pool, void* shard, const int64_t* indices, int B, uint8_t* out, int64_t out_cap,
                           int64_t* meta, float* xf, int64_t* labels, const AugSpec* aug, uint64_t seed,
                           uint64_t epoch, int out_h, int out_w) {
  auto* s = static_cast<Shard*>(shard);
  const uint64_t stride = s->hdr->max_bytes;
  if (B < 0 || static_cast<uint64_t>(B) * stride > static_cast<uint64_t>(out_cap)) return -2;
  for (int b = 0; b < B; ++b)
    if (indices[b] < 0 || static_cast<uint64_t>(indices[b]) >= s->hdr->count) return -3;
  AugSpec a = *aug;
  if (out_h <= 0 || out_w <= 0 || a.mode < 0 || a.mode > 4 || a.pad < 0 || a.canvas_h < 0 || a.canvas_w < 0 ||
      !(a.rot_deg >= 0.f))
    return -4;
  std::vector<int64_t> idx(indices, indices + B);
  return static_cast<Pool*>(pool)->submit(B, [=](int b) -> int {
    const IndexEntry& e = s->index[idx[b]];
    const int H = static_cast<int>(e.h), W = static_cast<int>(e.w);
    std::memcpy(out + b * stride, s->data + e.offset, size_t(H) * W * 3);
    Rng rng(mix_key(seed, epoch, static_cast<uint64_t>(idx[b])));
    int box[4] = {0, 0, H, W};
    int Sh = a.canvas_h > 0 ? a.canvas_h : out_h, Sw = a.canvas_w > 0 ? a.canvas_w : out_w;
    int rc = 0;
    if (a.mode == 0) rrc_box(rng, H, W, a, box);
    if (a.mode == 1) center_box(H, W, a, box);
    // CenterCrop's offset, int(round((S - out) / 2.0)): nearbyint rounds halves to even as Python does
    double dy = std::nearbyint((Sh - out_h) / 2.0), dx = std::nearbyint((Sw - out_w) / 2.0);
    if (a.mode == 3) {
      Sh = H, Sw = W;
      const int ri = H + 2 * a.pad - out_h, rj = W + 2 * a.pad - out_w;
      if (ri < 0 || rj < 0) rc = 4;  // RandomCrop of an image smaller than the output, padding included
      dy = static_cast<double>(rng.randint(0, std::max(ri, 0) + 1) - a.pad);
      dx = static_cast<double>(rng.randint(0, std::max(rj, 0) + 1) - a.pad);
    }
    // rounded to the float that xf records, so the matrix can be recomputed from meta and xf[6]
    const float theta = a.rot_deg > 0.f ? static_cast<float>((2.0 * rng.uniform() - 1.0) * a.rot_deg) : 0.f;
    const int flip = a.mode != 1 ? rng.uniform() < a.flip_p : 0;
    int64_t* m = meta + b * 8;
    m[0] = static_cast<int64_t>(b * stride);
    m[1] = H, m[2] = W, m[3] = box[0], m[4] = box[1], m[5] = box[2], m[6] = box[3], m[7] = flip;
    float* t = xf + b * 8;
    affine_matrix(box[2], box[3], Sh, Sw, out_w, dx, dy, theta, flip, t);
    t[6] = theta, t[7] = 0.f;
    labels[b] = e.label;
    return rc;
  });
}

// dcpl_submit_affine's draws for the `pil` resampling mode: the same gather, meta, labels and the
// same draws in the same order (so a `pil` run sees the geometry a `fast` run sees), but instead of a
// composed matrix each image gets the integers of the PIL chain itself,
//   geo[b*12 .. b*12+12) = {Sh, Sw, dy, dx, a0, a1, a2, a3, a4, a5, rotate, angle float32 bits}:
// resize the box to the Sh x Sw canvas (Image.resize), rotate it with the 16.16 map a0..a5 when
// `rotate` is set (rotate_fix16), mirror, cut the out_h x out_w window at (dy, dx).  MODE_CENTER is
// Resize(resize) + CenterCrop as data/transforms.py computes them: the box is the whole record, the
// canvas' short side is `resize`, its long side int(round(resize * long / short)).  The pad-crop
// (mode 3) mirrors after its crop and needs no resampling: it stays on dcpl_submit_affine (-4 here).
// The window is centred, so it always meets its canvas.  A job fails the ticket with 6 when the box is
// more than 8x the canvas on an axis (the filter of dcp::resample_crop_kernel stops there).
int64_t dcpl_submit_exact(void* pool, void* shard, const int64_t* indices, int B, uint8_t* out, int64_t out_cap,
                          int64_t* meta, int32_t* geo, int64_t* labels, const AugSpec* aug, uint64_t seed,
                          uint64_t epoch, int out_h, int out_w) {
  auto* s = static_cast<Shard*>(shard);
  const uint64_t stride = s->hdr->max_bytes;
  if (B < 0 || static_cast<uint64_t>(B) * stride > static_cast<uint64_t>(out_cap)) return -2;
  for (int b = 0; b < B; ++b)
    if (indices[b] < 0 || static_cast<uint64_t>(indices[b]) >= s->hdr->count) return -3;
  AugSpec a = *aug;
  if (out_h <= 0 || out_w <= 0 || out_h > 8192 || out_w > 8192 || a.mode < 0 || a.mode > 4 || a.mode == 3 ||
      a.canvas_h < 0 || a.canvas_w < 0 || a.canvas_h > 4096 || a.canvas_w > 4096 || !(a.rot_deg >= 0.f) ||
      (a.mode == 1 && (a.resize <= 0 || a.resize > 4096)))
    return -4;
  std::vector<int64_t> idx(indices, indices + B);
  return static_cast<Pool*>(pool)->submit(B, [=](int b) -> int {
    const IndexEntry& e = s->index[idx[b]];
    const int H = static_cast<int>(e.h), W = static_cast<int>(e.w);
    std::memcpy(out + b * stride, s->data + e.offset, size_t(H) * W * 3);
    Rng rng(mix_key(seed, epoch, static_cast<uint64_t>(idx[b])));
    int box[4] = {0, 0, H, W};
    int64_t Sh = a.canvas_h > 0 ? a.canvas_h : out_h, Sw = a.canvas_w > 0 ? a.canvas_w : out_w;
    if (a.mode == 0) rrc_box(rng, H, W, a, box);
    if (a.mode == 1) {  // transforms.Resize(int): nearbyint rounds halves to even as Python's round does
      const double r = a.resize;
      if (W <= H) Sw = a.resize, Sh = static_cast<int64_t>(std::nearbyint(r * H / W));
      else Sh = a.resize, Sw = static_cast<int64_t>(std::nearbyint(r * W / H));
    }
    const int64_t dy = static_cast<int64_t>(std::nearbyint((Sh - out_h) / 2.0));
    const int64_t dx = static_cast<int64_t>(std::nearbyint((Sw - out_w) / 2.0));
    const float theta = a.rot_deg > 0.f ? static_cast<float>((2.0 * rng.uniform() - 1.0) * a.rot_deg) : 0.f;
    const int flip = a.mode != 1 ? rng.uniform() < a.flip_p : 0;
    int64_t* m = meta + b * 8;
    m[0] = static_cast<int64_t>(b * stride);
    m[1] = H, m[2] = W, m[3] = box[0], m[4] = box[1], m[5] = box[2], m[6] = box[3], m[7] = flip;
    labels[b] = e.label;
    int32_t* g = geo + b * 12;
    std::memset(g, 0, 12 * sizeof(int32_t));
    if (Sh < 1 || Sw < 1 || Sh > 4096 || Sw > 4096) return 6;  // a record thinner than 1 / 4096 of its length
    g[0] = static_cast<int32_t>(Sh), g[1] = static_cast<int32_t>(Sw);
    g[2] = static_cast<int32_t>(dy), g[3] = static_cast<int32_t>(dx);
    rotate_fix16(theta, static_cast<int>(Sh), static_cast<int>(Sw), g + 4);
    g[10] = a.rot_deg > 0.f;
    std::memcpy(g + 11, &theta, sizeof(float));
    if (box[2] > 8 * Sh || box[3] > 8 * Sw) return 6;
    return 0;
  });
}

int dcpl_wait(void* pool, int64_t ticket) { return static_cast<Pool*>(pool)->wait(ticket); }

}  // extern "C"
