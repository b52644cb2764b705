// The part of the extern "C" surface of libgeobi_hip.so (include/geobi_hip.h) that has no other home: error reporting,
// the shared argument checks (sizes_ok, parts_check), per-kernel event timing for bench.py, the side stream and the host
// utilities (mailbox, read-back).  Every other entry point is defined in the unit that implements it.
#include "../../include/geobi_hip.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <mutex>
#include <vector>

#include "common.h"

namespace geobi {

static thread_local char g_err[512] = "";

int set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return 1;
}

// ------------------------------------------------------------------------- profiling
struct ProfRec {
  hipEvent_t a, b;
  double bytes;
  int tag;
  hipStream_t stream = nullptr;
  bool closed = false;
  bool bound = false;      // events bound to a kernel's dispatch by the extended launch (no hipEventRecord)
};
static std::atomic<int> g_prof_kernel{PROF_NONE};
static std::mutex g_prof_mu;             // the record list is shared by the host threads of a concurrent step
static std::vector<ProfRec> g_prof;
static std::vector<hipEvent_t> g_event_pool;

static hipEvent_t get_event() {
  if (!g_event_pool.empty()) {
    hipEvent_t e = g_event_pool.back();
    g_event_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

void prof_begin(int kernel, hipStream_t s, double alg_bytes, int tag) {
  if (kernel != g_prof_kernel.load(std::memory_order_relaxed)) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  ProfRec r;
  r.a = get_event();
  r.b = get_event();
  r.bytes = alg_bytes;
  r.tag = tag;
  if (!r.a || !r.b) return;
  r.stream = s;
  (void)hipEventRecord(r.a, s);
  g_prof.push_back(r);
}

static thread_local hipEvent_t g_launch_ev[2] = {nullptr, nullptr};      // handed from prof_begin_launch to the launch site

void prof_begin_launch(int kernel, hipStream_t s, double alg_bytes, int tag) {
  if (kernel != g_prof_kernel.load(std::memory_order_relaxed)) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  ProfRec r;
  r.a = get_event();
  r.b = get_event();
  r.bytes = alg_bytes;
  r.tag = tag;
  if (!r.a || !r.b) return;
  r.stream = s;
  g_launch_ev[0] = r.a;
  g_launch_ev[1] = r.b;
  r.bound = true;
  g_prof.push_back(r);
}

bool prof_take_launch_events(hipEvent_t* start, hipEvent_t* stop) {
  if (g_launch_ev[0] == nullptr) return false;
  *start = g_launch_ev[0];
  *stop = g_launch_ev[1];
  g_launch_ev[0] = g_launch_ev[1] = nullptr;
  return true;
}

void prof_end(int kernel, hipStream_t s) {
  if (kernel != g_prof_kernel.load(std::memory_order_relaxed)) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (g_launch_ev[0] != nullptr) {
    // prof_begin_launch's events were not taken (a launch path without the extended launch): bracket nothing, drop the record
    g_launch_ev[0] = g_launch_ev[1] = nullptr;
    for (size_t i = g_prof.size(); i-- > 0;)
      if (g_prof[i].stream == s && !g_prof[i].closed) { g_prof.erase(g_prof.begin() + (long)i); break; }
    return;
  }
  // the most recent open record of THIS stream (another thread's record may sit behind it)
  for (size_t i = g_prof.size(); i-- > 0;) {
    if (g_prof[i].stream == s && !g_prof[i].closed) {
      g_prof[i].closed = true;
      if (!g_prof[i].bound) (void)hipEventRecord(g_prof[i].b, s);
      return;
    }
  }
}

// ------------------------------------------------------------------------- side stream
// Context = host thread.  Everything below the overlap switch is per host thread: a thread drives one stream at a time
// (the caller's stream of a per-op call; the stream of ONE mesh group in geobi_net_train_groups), so every context has
// its own side streams and fork / join events and two groups in flight never meet on a shared event.
static Knob g_overlap{"GEOBI_OVERLAP", 1};      // process-wide (geobi_set_overlap)
static thread_local int g_overlap_here = -1;   // this context's override of g_overlap (-1: none); side_override()
static thread_local int g_defer = 0;     // 1: backward calls fork but do not join; the caller joins once (geobi_side_join)
// Two side streams: [0] at the default priority, [1] at the lowest.  On a big batch the weight-gradient products
// compete with the backward's own kernels for workgroup slots: at the lowest priority they fill what the main stream
// leaves free (4.37-4.43 against 4.48-4.57 ms per step on the bench batch).  On small batches -- the host-bound regime,
// the device has idle gaps anyway -- the low-priority queue is served late and the join at the end waits for it (n = 16:
// 2.85-2.90 against 2.77-2.79 ms).  side_select() picks per backward; per-op callers get the default one.
static thread_local hipStream_t g_sides[2] = {nullptr, nullptr};
static thread_local int g_side_sel = 0;
static thread_local hipStream_t g_side = nullptr;           // the stream the current / last fork used
static thread_local hipEvent_t g_fork_ev = nullptr, g_join_ev = nullptr;

void side_select(int low_priority) {
  static Knob allow{"GEOBI_SIDE_PRIORITY", 1};
  g_side_sel = (low_priority && allow.on()) ? 1 : 0;
}

void side_override(int mode) { g_overlap_here = mode; }
hipStream_t side_current() { return g_side; }

Fork fork_side_stream(hipStream_t main) {
  Fork f;
  if (g_overlap_here == 0 || (g_overlap_here < 0 && !g_overlap.on())) return f;
  if (g_sides[g_side_sel] == nullptr) {
    int lo = 0, hi = 0;
    if (g_side_sel == 0 || hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = 0;
    const hipError_t ce = hipStreamCreateWithPriority(&g_sides[g_side_sel], hipStreamNonBlocking, lo);
    if (ce != hipSuccess) {
      g_sides[g_side_sel] = nullptr;
      return f;
    }
    if (g_fork_ev == nullptr &&
        (hipEventCreateWithFlags(&g_fork_ev, hipEventDisableTiming) != hipSuccess ||
         hipEventCreateWithFlags(&g_join_ev, hipEventDisableTiming) != hipSuccess)) { g_overlap.set(0); return f; }
  }
  g_side = g_sides[g_side_sel];
  if (hipEventRecord(g_fork_ev, main) != hipSuccess) return f;
  if (hipStreamWaitEvent(g_side, g_fork_ev, 0) != hipSuccess) return f;
  f.side = g_side;
  f.join = g_join_ev;
  return f;
}

int side_wait_main(const Fork& f, hipStream_t main) {
  if (f.side == nullptr) return 0;
  GEOBI_HIP(hipEventRecord(g_fork_ev, main));
  GEOBI_HIP(hipStreamWaitEvent(f.side, g_fork_ev, 0));
  return 0;
}

int join_side_stream(const Fork& f, hipStream_t main) {
  if (f.side == nullptr || g_defer) return 0;
  GEOBI_HIP(hipEventRecord(f.join, f.side));
  GEOBI_HIP(hipStreamWaitEvent(main, f.join, 0));
  return 0;
}

}  // namespace geobi

using namespace geobi;

// the size limits every entry point checks (GEOBI_SIZES, common.h)
int geobi::sizes_ok(const char* fn, int64_t nodes, int64_t edges) {
  if (nodes < 0 || edges < 0) return set_error("%s: negative size (%lld nodes, %lld edges)", fn, (long long)nodes, (long long)edges);
  if (nodes > GEOBI_MAX_NODES)
    return set_error("%s: %lld nodes exceed GEOBI_MAX_NODES = %d per call (split the mesh into patches)", fn, (long long)nodes, GEOBI_MAX_NODES);
  if (edges > GEOBI_MAX_EDGES)
    return set_error("%s: %lld edges exceed GEOBI_MAX_EDGES = %d per call (split the mesh into patches)", fn, (long long)edges, GEOBI_MAX_EDGES);
  return 0;
}

// the host part pointers of a union batch (common.h): every entry point that takes them checks them here, once
int geobi::parts_check(const char* fn, const int64_t* qptr, const int64_t* tptr, int P) {
  GEOBI_REQUIRE(P >= 1, "%s: P = %d parts (at least one)", fn, P);
  GEOBI_REQUIRE(qptr != nullptr && tptr != nullptr, "%s: qptr / tptr is NULL", fn);
  GEOBI_REQUIRE(qptr[0] >= 0 && tptr[0] >= 0, "%s: qptr / tptr starts below 0", fn);
  for (int p = 0; p < P; ++p)
    for (const int64_t* ptr : {qptr, tptr})
      GEOBI_REQUIRE(ptr[p + 1] > ptr[p], "%s: part %d of %s is empty (%lld .. %lld): an empty part is an error, not a launch", fn,
                    p, ptr == qptr ? "qptr" : "tptr", (long long)ptr[p], (long long)ptr[p + 1]);
  return sizes_ok(fn, qptr[P] > tptr[P] ? qptr[P] : tptr[P], 0);
}

extern "C" {

int geobi_version(void) { return 100; }
const char* geobi_last_error(void) { return g_err; }

// Spin (without the caller's interpreter lock: ctypes releases it for the call) until a mailbox word is non-zero or `stream`
// has drained without writing it; returns the word (0: the stream ran dry).
int geobi_host_mailbox_wait(const int32_t* word, void* stream) {
  if (word == nullptr) return 0;
  long spins = 0;
  int v;
  while ((v = __atomic_load_n(word, __ATOMIC_ACQUIRE)) == 0) {
    if ((++spins & 0x3fff) == 0 && hipStreamQuery(as_stream(stream)) != hipErrorNotReady) return __atomic_load_n(word, __ATOMIC_ACQUIRE);
  }
  return v;
}

// Mapped host memory a kernel can hand small results over through (patch sizes): `n` int32 slots, zeroed, valid until the
// next call from the same host thread asks for more.
int geobi_host_mailbox(int n, int32_t** host_ptr) {
  GEOBI_NOTNULL(host_ptr);
  GEOBI_REQUIRE(n > 0 && n <= (1 << 20), "geobi_host_mailbox: 1 .. 2^20 slots");
  static thread_local int32_t* box = nullptr;
  static thread_local int cap = 0;
  if (n > cap) {
    if (box) (void)hipHostFree(box);
    box = nullptr; cap = 0;
    const int want = n < 1024 ? 1024 : n;
    GEOBI_HIP(hipHostMalloc((void**)&box, (size_t)want * sizeof(int32_t), hipHostMallocMapped | hipHostMallocPortable));
    cap = want;
  }
  for (int i = 0; i < n; ++i) box[i] = 0;
  *host_ptr = box;
  return 0;
}

int geobi_side_defer(int on) {
  g_defer = on ? 1 : 0;
  return 0;
}

int geobi_side_join(void* stream) {
  if (g_side == nullptr) return 0;          // nothing was ever forked
  GEOBI_HIP(hipEventRecord(g_join_ev, g_side));
  GEOBI_HIP(hipStreamWaitEvent(as_stream(stream), g_join_ev, 0));
  return 0;
}

// Device -> host read of a few int32 (sizes a pooling step computed) with a spinning wait: the copy lands in a
// pinned staging buffer and the calling thread polls the event instead of sleeping on an interrupt, which
// takes ~10 us off every size read-back on this platform.
int geobi_read_i32(const int32_t* dev, int n, int32_t* host, void* stream) {
  GEOBI_NOTNULL(dev); GEOBI_NOTNULL(host);
  GEOBI_REQUIRE(n > 0 && n <= 64, "geobi_read_i32: 1..64 values");
  static thread_local int32_t* pinned = nullptr;
  static thread_local hipEvent_t ev = nullptr;
  if (pinned == nullptr) {
    GEOBI_HIP(hipHostMalloc((void**)&pinned, 64 * sizeof(int32_t), hipHostMallocDefault));
    GEOBI_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  }
  GEOBI_HIP(hipMemcpyAsync(pinned, dev, n * sizeof(int32_t), hipMemcpyDeviceToHost, as_stream(stream)));
  GEOBI_HIP(hipEventRecord(ev, as_stream(stream)));
  hipError_t st;
  while ((st = hipEventQuery(ev)) == hipErrorNotReady) {
  }
  GEOBI_HIP(st);
  for (int i = 0; i < n; ++i) host[i] = pinned[i];
  return 0;
}

int geobi_set_overlap(int enable) {
  g_overlap.set(enable ? 1 : 0);
  return 0;
}

int geobi_prof_enable(int kernel) {
  // returns recorded events to the pool; callers collect before re-enabling
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (auto& r : g_prof) { g_event_pool.push_back(r.a); g_event_pool.push_back(r.b); }
  g_prof.clear();
  g_prof_kernel = kernel;
  return 0;
}

int geobi_prof_collect(int tag, int64_t* launches, double* total_ms, double* total_bytes) {
  GEOBI_NOTNULL(launches); GEOBI_NOTNULL(total_ms); GEOBI_NOTNULL(total_bytes);
  *launches = 0; *total_ms = 0.0; *total_bytes = 0.0;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (auto& r : g_prof) {
    if (!r.closed) continue;
    GEOBI_HIP(hipEventSynchronize(r.b));
    if (tag != 0 && r.tag != tag) continue;
    float ms = 0.f;
    GEOBI_HIP(hipEventElapsedTime(&ms, r.a, r.b));
    *launches += 1;
    *total_ms += (double)ms;
    *total_bytes += r.bytes;
  }
  return 0;
}

}  // extern "C"
