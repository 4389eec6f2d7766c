// Per-problem autotuning (g_tune[kAutotune] = 1), shared by the forward / data-gradient tap GEMM
// (conv_igemm.hip) and the weight gradient (bindings.cpp): the choice cache, the timing loop, the
// scoped g_tune override that runs a candidate, and the cache's text form.  Each user keeps its own
// candidate table, key builder and bypass conditions.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <mutex>
#include <string>
#include <unordered_map>

#include "tune.h"

namespace dcp {

// g_tune[slots[i]] = values[i] for the guard's lifetime (slots: a static list of at most kMax slots)
class TuneGuard {
 public:
  static constexpr int kMax = 8;
  TuneGuard(std::initializer_list<int> slots, std::initializer_list<int> values) : n_((int)slots.size()) {
    for (int i = 0; i < n_; ++i) {
      slot_[i] = slots.begin()[i];
      saved_[i] = g_tune[slot_[i]];
      g_tune[slot_[i]] = values.begin()[i];
    }
  }
  ~TuneGuard() {
    for (int i = 0; i < n_; ++i) g_tune[slot_[i]] = saved_[i];
  }
  TuneGuard(const TuneGuard&) = delete;
  TuneGuard& operator=(const TuneGuard&) = delete;

 private:
  int n_, slot_[kMax], saved_[kMax];
};

// The choices of one candidate table: problem key -> candidate index.
class Autotuner {
 public:
  // what: the name in the DCP_AUTOTUNE_LOG line; tag: the first field of the cache's text lines
  Autotuner(const char* what, const char* tag, int n_candidates) : what_(what), tag_(tag), n_(n_candidates) {}

  int size() {
    std::lock_guard<std::mutex> lk(mu_);
    return (int)choice_.size();
  }

  // The candidate to run for `key`: the recorded one, or, on the first call of a problem, the fastest
  // of one warm-up run and the best of 3 timed runs per candidate not skipped (every candidate
  // overwrites the same outputs with the same values).  Candidate 0 is the heuristic and is never
  // skipped; another one replaces it only below 0.98 x its time.  Returns -1, recording nothing, when
  // the problem is new and `stream` is capturing: no timing inside a capture, the caller runs the
  // heuristic (problems are tuned on the eager warm-up steps).
  template <class Skip, class RunWith>
  int pick(const std::string& key, hipStream_t stream, Skip skip, RunWith run_with) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      auto it = choice_.find(key);
      if (it != choice_.end()) return it->second;
    }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return -1;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    float best = 1e30f, t_heur = 1e30f;
    int choice = 0;
    for (int c = 0; c < n_; ++c) {
      if (c != 0 && skip(c)) continue;
      run_with(c);  // warm
      float t = 1e30f;
      for (int r = 0; r < 3; ++r) {
        (void)hipEventRecord(e0, stream);
        run_with(c);
        (void)hipEventRecord(e1, stream);
        (void)hipEventSynchronize(e1);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        t = std::min(t, ms);
      }
      if (c == 0) {
        t_heur = best = t;
      } else if (t < best && t < 0.98f * t_heur) {  // must beat the heuristic by 2 % to replace it
        best = t;
        choice = c;
      }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    {
      std::lock_guard<std::mutex> lk(mu_);
      choice_[key] = choice;
    }
    if (getenv("DCP_AUTOTUNE_LOG"))
      fprintf(stderr, "[dcp-autotune] %s %s -> cfg %d (%.1f us)\n", what_, key.c_str(), choice, best * 1e3f);
    return choice;
  }

  // The decisions as text, "<tag>\t<key>\t<choice>\n" per problem, and back: a tuning cache that makes a later
  // process run exactly the kernels an earlier one measured (DCP_TUNE_CACHE, _ext.py).  Keys never contain tabs
  // or newlines.  The import takes the lines of this tag, skips those without a key or with a choice out of
  // this build's candidate range, and returns the number accepted.
  std::string export_text() {
    std::lock_guard<std::mutex> lk(mu_);
    std::string out;
    for (const auto& kv : choice_) out += tag_ + "\t" + kv.first + "\t" + std::to_string(kv.second) + "\n";
    return out;
  }

  int import_text(const std::string& text) {
    const std::string head = tag_ + "\t";
    std::lock_guard<std::mutex> lk(mu_);
    int n = 0;
    size_t pos = 0;
    while (pos < text.size()) {
      size_t nl = text.find('\n', pos);
      if (nl == std::string::npos) nl = text.size();
      const std::string line = text.substr(pos, nl - pos);
      pos = nl + 1;
      if (line.compare(0, head.size(), head) != 0) continue;
      const size_t tab = line.rfind('\t');
      if (tab <= head.size()) continue;  // no choice field, or an empty key
      const int c = atoi(line.c_str() + tab + 1);
      if (c < 0 || c >= n_) continue;
      choice_[line.substr(head.size(), tab - head.size())] = c;
      ++n;
    }
    return n;
  }

 private:
  const char* what_;
  const std::string tag_;
  const int n_;
  std::mutex mu_;
  std::unordered_map<std::string, int> choice_;
};

}  // namespace dcp
