// dev_scratch.h -- scope-bound owners of what a door allocates per call: device scratch, the host arrays bound for the caller, and
// the HIP events of the optional kernel timing.  Every early return of a door releases what it took, by construction.
// Textually included by sqmc_gpu.hip behind <hip/hip_runtime.h>.  It names no HIP header itself: tests/scratch_host_check.cpp
// includes it behind counting stand-ins of the few HIP calls used here.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <atomic>
#include <vector>

// process-wide: what the owners hold now, the most they ever held, takes so far, and the injected-failure countdown
// (sqmc_gpu_debug_scratch_stats, sqmc_gpu_debug_scratch_stats_fail_at)
struct ScratchStats { std::atomic<int64_t> live_allocs{0}, live_bytes{0}, peak_bytes{0}, n_takes{0}, fail_at{0}; };
static ScratchStats g_scratch_stats;

struct ScratchNoCopy { ScratchNoCopy() {} ScratchNoCopy(const ScratchNoCopy &) = delete; ScratchNoCopy &operator=(const ScratchNoCopy &) = delete; };

// Device buffers owned until dropped, handed to another owner, or the scope ends.  The destructor synchronises the stream before it
// frees: after an early return, kernels that read these buffers may still be queued.
class DevScratch : ScratchNoCopy {
 public:
  hipStream_t stream;
  explicit DevScratch(hipStream_t st = nullptr) : stream(st) {}
  ~DevScratch() { clear(); }
  // count items of T; null on failure, and every later take fails too, so that a run of takes needs one check (ok / err).
  // A zero count still yields a valid pointer.
  template <class T> T *take(size_t count) {
    if (err_ != hipSuccess) return nullptr;
    size_t bytes = count * sizeof(T); if (!bytes) bytes = 8;
    void *p = nullptr; g_scratch_stats.n_takes++;
    if (g_scratch_stats.fail_at.load() > 0 && g_scratch_stats.fail_at.fetch_sub(1) == 1) err_ = hipErrorOutOfMemory;      // injected: no hipMalloc
    else if ((err_ = hipMalloc(&p, bytes)) != hipSuccess) (void)hipGetLastError();
    if (err_ != hipSuccess) return nullptr;
    mem_.push_back({p, bytes});
    g_scratch_stats.live_allocs++;
    const int64_t now = g_scratch_stats.live_bytes += (int64_t)bytes;
    for (int64_t pk = g_scratch_stats.peak_bytes.load(); pk < now && !g_scratch_stats.peak_bytes.compare_exchange_weak(pk, now);) {}
    return (T *)p;
  }
  bool ok() const { return err_ == hipSuccess; } hipError_t err() const { return err_; }
  // free one buffer now; hand one buffer to another owner (null: nothing to do)
  void drop(void *p) { const int k = find(p); if (k >= 0) { release(mem_[k]); mem_.erase(mem_.begin() + k); } }
  void keep(void *p, DevScratch &to) { const int k = find(p); if (k >= 0) { to.mem_.push_back(mem_[k]); mem_.erase(mem_.begin() + k); } }
  void clear() {
    if (!mem_.empty()) (void)hipStreamSynchronize(stream);
    for (const Buf &b : mem_) release(b);
    mem_.clear(); err_ = hipSuccess;
  }
 private:
  struct Buf { void *p; size_t bytes; };
  std::vector<Buf> mem_;
  hipError_t err_ = hipSuccess;
  int find(void *p) const { if (p) for (int k = (int)mem_.size() - 1; k >= 0; k--) if (mem_[k].p == p) return k; return -1; }
  static void release(const Buf &b) { (void)hipFree(b.p); g_scratch_stats.live_allocs--; g_scratch_stats.live_bytes -= (int64_t)b.bytes; }
};

// The malloc'ed arrays a door hands to its caller: freed at scope exit unless committed, so that the caller's pointers are written
// only when the whole call has succeeded.
class HostOut : ScratchNoCopy {
 public:
  ~HostOut() { for (void *q : mem_) free(q); }
  template <class T> T *take(size_t count) { void *p = malloc(count * sizeof(T) + 8); if (p) mem_.push_back(p); return (T *)p; }
  // the caller's pointer takes the array; a null destination leaves it to be freed
  template <class T, class U> void commit(T *p, U **out) {
    if (!out) return;
    for (size_t k = 0; k < mem_.size(); k++) if (mem_[k] == (void *)p) { mem_.erase(mem_.begin() + k); *out = (U *)p; return; }
  }
 private:
  std::vector<void *> mem_;
};

// The optional timing of a kernel group: up to four events, created only when `on`, recorded in order by mark(); after the caller's
// synchronise add() adds the milliseconds between consecutive marks to ms[0], ms[1], ... and starts over.  Destroyed on every path.
class EventMarks : ScratchNoCopy {
 public:
  EventMarks(bool on, int n) : on_(on) { if (on) for (; n_ < n && n_ < 4; n_++) if ((err_ = hipEventCreate(&ev_[n_])) != hipSuccess) break; }
  ~EventMarks() { for (int k = 0; k < n_; k++) (void)hipEventDestroy(ev_[k]); }
  hipError_t mark(hipStream_t st) {
    if (!on_) return hipSuccess;
    if (err_ != hipSuccess) return err_;
    if (marked_ >= n_) return hipErrorInvalidValue;
    return hipEventRecord(ev_[marked_++], st);
  }
  void add(double *ms) {
    for (int k = 0; k + 1 < marked_; k++) { float t = 0.f; if (hipEventElapsedTime(&t, ev_[k], ev_[k + 1]) == hipSuccess) ms[k] += t; }
    marked_ = 0;
  }
 private:
  hipEvent_t ev_[4]; int n_ = 0, marked_ = 0; bool on_; hipError_t err_ = hipSuccess;
};
