// scratch_host_check.cpp -- the owners of sqmc_amd/csrc/dev_scratch.h on the host, against counting stand-ins of the HIP calls they
// use.  A stand-alone program: tests/test_scratch_host.py builds it with -fsanitize=address,undefined and runs it as a child process.
// Every check prints its name; the first failure ends the program with status 1.
#include <stdio.h>
#include <stdlib.h>
#include <set>
#include <string>
#include <vector>

// ---- stand-ins
typedef int hipError_t;
enum { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 };
typedef struct StreamTag *hipStream_t;
typedef struct EventTag *hipEvent_t;
struct Fake {
  std::set<void *> live;                 // device buffers not yet freed
  std::vector<std::string> log;          // "sync", "free" in call order
  long n_malloc = 0, n_free = 0, n_double_free = 0, n_sync = 0, fail_malloc_at = 0, n_last_error = 0;
  long ev_live = 0, ev_created = 0, ev_fail_create_at = 0, ev_recorded = 0;
  hipStream_t last_sync = nullptr;
} F;
static hipError_t hipMalloc(void **p, size_t bytes) {
  F.n_malloc++;
  if (F.fail_malloc_at && F.n_malloc == F.fail_malloc_at) { *p = nullptr; return hipErrorOutOfMemory; }
  *p = malloc(bytes); F.live.insert(*p);
  return hipSuccess;
}
static hipError_t hipFree(void *p) {
  F.n_free++; F.log.push_back("free");
  if (!F.live.erase(p)) { F.n_double_free++; return hipErrorInvalidValue; }
  free(p);
  return hipSuccess;
}
static hipError_t hipGetLastError() { F.n_last_error++; return hipSuccess; }
static hipError_t hipStreamSynchronize(hipStream_t st) { F.n_sync++; F.last_sync = st; F.log.push_back("sync"); return hipSuccess; }
static hipError_t hipEventCreate(hipEvent_t *e) {
  F.ev_created++;
  if (F.ev_fail_create_at && F.ev_created == F.ev_fail_create_at) return hipErrorOutOfMemory;
  *e = (hipEvent_t)malloc(1); F.ev_live++;
  return hipSuccess;
}
static hipError_t hipEventDestroy(hipEvent_t e) { free(e); F.ev_live--; return hipSuccess; }
static hipError_t hipEventRecord(hipEvent_t, hipStream_t) { F.ev_recorded++; return hipSuccess; }
static hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 1.5f; return hipSuccess; }

#include "../sqmc_amd/csrc/dev_scratch.h"

static int n_checks = 0;
#define CHECK(cond) do { n_checks++; if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)
static void reset() { F = Fake(); g_scratch_stats.fail_at = 0; }
static bool balanced() { return F.live.empty() && g_scratch_stats.live_allocs == 0 && g_scratch_stats.live_bytes == 0 && F.n_double_free == 0; }
static hipStream_t const ST = (hipStream_t)0x40;

// a door in miniature: n takes in two runs with a drop and a keep between them, and an early return after each run
static int mini_door(int n, DevScratch &caller, void **kept) {
  DevScratch s(ST);
  std::vector<double *> b;
  for (int k = 0; k < n / 2; k++) b.push_back(s.take<double>(10 + k));
  if (!s.ok()) return 1;
  s.drop(b[0]);
  for (int k = n / 2; k < n; k++) b.push_back(s.take<double>(10 + k));
  if (!s.ok()) return 2;
  s.keep(b[1], caller); *kept = b[1];
  return 0;
}

int main() {
  // everything taken is freed at scope exit, after one synchronise of the owner's stream that comes before the first free
  reset();
  {
    DevScratch s(ST);
    double *a = s.take<double>(100); int *b = s.take<int>(7); char *z = s.take<char>(0);
    CHECK(a && b && z && s.ok() && s.err() == hipSuccess);
    CHECK(F.live.size() == 3 && g_scratch_stats.live_allocs == 3 && g_scratch_stats.live_bytes == 800 + 28 + 8);      // a zero count is 8 bytes
    CHECK(F.n_sync == 0 && F.n_free == 0);
  }
  CHECK(balanced() && F.n_free == 3 && F.n_sync == 1 && F.last_sync == ST);
  CHECK(F.log.size() == 4 && F.log[0] == "sync");
  CHECK(g_scratch_stats.peak_bytes == 836);
  puts("ok scope exit frees everything behind one synchronise");

  // an owner that holds nothing neither synchronises nor frees
  reset();
  { DevScratch s(ST); }
  { DevScratch s(ST); double *a = s.take<double>(4); s.drop(a); CHECK(F.n_free == 1); }
  CHECK(balanced() && F.n_sync == 0 && F.n_free == 1);
  puts("ok an empty owner does not synchronise");

  // a dropped pointer is freed once, at the drop; null and foreign pointers are left alone
  reset();
  {
    DevScratch s(ST);
    double *a = s.take<double>(4), *b = s.take<double>(4); int other = 0;
    s.drop(a);
    CHECK(F.n_free == 1 && F.live.size() == 1 && g_scratch_stats.live_allocs == 1 && g_scratch_stats.live_bytes == 32);
    s.drop(a); s.drop(nullptr); s.drop(&other);
    CHECK(F.n_free == 1 && b);
  }
  CHECK(balanced() && F.n_free == 2);
  puts("ok drop frees once");

  // a kept pointer is not freed by the owner that gave it away, stays counted, and goes with the owner that took it
  reset();
  {
    DevScratch plan(ST);
    double *kept = nullptr;
    {
      DevScratch s(ST);
      kept = s.take<double>(16); double *tmp = s.take<double>(16);
      s.keep(kept, plan); s.keep(nullptr, plan);
      CHECK(tmp && g_scratch_stats.live_allocs == 2);
    }
    CHECK(F.n_free == 1 && F.live.count(kept) == 1 && g_scratch_stats.live_allocs == 1 && g_scratch_stats.live_bytes == 128);
    kept[15] = 1.0;      // still ours: the sanitizer would object otherwise
    plan.clear();
    CHECK(balanced() && F.n_free == 2);
    plan.clear();
    CHECK(F.n_free == 2);
  }
  CHECK(balanced());
  puts("ok keep hands a buffer over");

  // the k-th allocation fails, for every k: nothing is left behind, the failure is remembered, later takes do not reach hipMalloc
  for (int n = 2; n <= 9; n++)
    for (int k = 1; k <= n; k++) {
      reset();
      F.fail_malloc_at = k;
      DevScratch caller(ST); void *kept = nullptr;
      const int rc = mini_door(n, caller, &kept);
      CHECK(rc == (k <= n / 2 ? 1 : 2));
      CHECK(balanced() && F.n_malloc == k);
      CHECK(F.n_last_error == 1);
      // whenever the door still owned something at its exit, it synchronised once, and every free of the exit came behind that
      const long owned = k <= n / 2 ? k - 1 : k - 2;      // the takes that succeeded, less the one dropped between the runs
      size_t sync_at = F.log.size();
      for (size_t q = 0; q < F.log.size(); q++) if (F.log[q] == "sync") { sync_at = q; break; }
      CHECK(F.n_sync == (owned > 0 ? 1 : 0));
      if (owned > 0) CHECK(sync_at == (k <= n / 2 ? 0u : 1u) && F.log.size() == sync_at + 1 + (size_t)owned);
    }
  // and the same door without a failure
  reset();
  {
    DevScratch caller(ST); void *kept = nullptr;
    CHECK(mini_door(6, caller, &kept) == 0 && F.live.size() == 1 && F.live.count(kept) == 1 && g_scratch_stats.live_allocs == 1);
  }
  CHECK(balanced());
  puts("ok a failing k-th allocation leaves nothing behind, for every k");

  // the error is sticky until clear()
  reset();
  {
    DevScratch s(ST);
    F.fail_malloc_at = 2;
    double *a = s.take<double>(1), *b = s.take<double>(1), *c2 = s.take<double>(1);
    CHECK(a && !b && !c2 && !s.ok() && s.err() == hipErrorOutOfMemory && F.n_malloc == 2);
    s.clear();
    CHECK(s.ok() && balanced());
    CHECK(s.take<double>(1) != nullptr);
  }
  CHECK(balanced());
  puts("ok the failure is remembered until clear");

  // fail_at: the nth take from now fails without a call of hipMalloc, exactly once; 0 disarms
  reset();
  {
    DevScratch s(ST);
    const long takes0 = g_scratch_stats.n_takes;
    g_scratch_stats.fail_at = 3;
    CHECK(s.take<int>(1) && s.take<int>(1) && F.n_malloc == 2);
    CHECK(!s.take<int>(1) && F.n_malloc == 2 && s.err() == hipErrorOutOfMemory && g_scratch_stats.fail_at == 0);
    CHECK(g_scratch_stats.n_takes == takes0 + 3);
    s.clear();
    for (int k = 0; k < 5; k++) CHECK(s.take<int>(1) != nullptr);
    g_scratch_stats.fail_at = 2; g_scratch_stats.fail_at = 0;
    for (int k = 0; k < 5; k++) CHECK(s.take<int>(1) != nullptr);
    CHECK(F.n_malloc == 12);
  }
  CHECK(balanced());
  puts("ok fail_at fires exactly once");

  // the peak follows the live bytes and not the total
  reset();
  g_scratch_stats.peak_bytes = 0;
  {
    DevScratch s(ST);
    char *a = s.take<char>(1000); s.drop(a);
    char *b = s.take<char>(600), *c2 = s.take<char>(300);
    CHECK(b && c2 && g_scratch_stats.peak_bytes == 1000 && g_scratch_stats.live_bytes == 900);
    char *d = s.take<char>(200);
    CHECK(d && g_scratch_stats.peak_bytes == 1100);
  }
  CHECK(balanced() && g_scratch_stats.peak_bytes == 1100);
  puts("ok peak bytes");

  // host arrays bound for the caller: the uncommitted ones are freed, the committed ones are the caller's
  reset();
  {
    double *out_a = nullptr; long *out_c = nullptr; double **no_dest = nullptr;
    {
      HostOut h;
      double *a = h.take<double>(50), *b = h.take<double>(50); long *c2 = h.take<long>(0); double *d = h.take<double>(5);
      a[49] = 1.0; b[49] = 2.0; c2[0] = 3;
      h.commit(a, &out_a); h.commit(c2, &out_c); h.commit(d, no_dest); h.commit((double *)nullptr, &out_a);
      CHECK(out_a == a && out_c == c2);
    }
    CHECK(out_a[49] == 1.0 && out_c[0] == 3);      // b and d are gone (the leak check of the sanitizer sees them if not)
    free(out_a); free(out_c);
  }
  {
    double *out = nullptr;
    const int rc = [&]() -> int { HostOut h; double *a = h.take<double>(8); a[0] = 1.0; if (F.n_malloc == 0) return 1; h.commit(a, &out); return 0; }();
    CHECK(rc == 1 && out == nullptr);      // an early return wrote nothing and freed the array
  }
  puts("ok host arrays are released unless committed");

  // the events of the optional timing: none when off; recorded in order, summed per interval, destroyed on every path
  reset();
  {
    EventMarks off(false, 2); double ms = 0.0;
    CHECK(off.mark(ST) == hipSuccess && off.mark(ST) == hipSuccess);
    off.add(&ms);
    CHECK(F.ev_created == 0 && F.ev_recorded == 0 && ms == 0.0);
  }
  {
    double ms[3] = {0.0, 0.0, 0.0};
    {
      EventMarks ev(true, 4);
      CHECK(F.ev_live == 4);
      for (int rep = 0; rep < 2; rep++) {
        for (int k = 0; k < 4; k++) CHECK(ev.mark(ST) == hipSuccess);
        CHECK(ev.mark(ST) != hipSuccess);      // a fifth mark has no event
        ev.add(ms);
      }
    }
    CHECK(F.ev_live == 0 && F.ev_recorded == 8 && ms[0] == 3.0 && ms[1] == 3.0 && ms[2] == 3.0);
  }
  for (int path = 0; path < 2; path++) {      // the error path: an early return between the marks; a creation that fails
    reset();
    if (path == 1) F.ev_fail_create_at = 2;
    double ms = 0.0;
    [&]() -> int {
      EventMarks ev(true, 2);
      if (ev.mark(ST) != hipSuccess) return 1;
      DevScratch s(ST);
      F.fail_malloc_at = 1;
      if (!s.take<double>(8)) return 2;
      ev.add(&ms);
      return 0;
    }();
    CHECK(F.ev_live == 0 && ms == 0.0 && balanced());
    CHECK(path == 0 ? F.ev_recorded == 1 : F.ev_recorded == 0);
  }
  puts("ok event marks are destroyed on every path");

  printf("all ok: %d checks\n", n_checks);
  return 0;
}
