// The part of the extern "C" surface of libgeobi_hip.so (include/geobi_hip.h) that has no other home: error reporting,
// the shared argument checks, per-kernel event timing for bench.py, the side stream, host utilities, the geobi_set_*
// hooks, and the entry points of the launchers executor.hip shares.  The mesh tools define theirs in their own unit.
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

int geobi_expand_rowptr(const int32_t* rowptr, int64_t N, int32_t* row, void* stream) {
  GEOBI_SIZES(N, 0);
  return expand_rowptr(rowptr, N, row, as_stream(stream));
}
int geobi_concat32(const geobi_copy_seg_t* segs, int n_segs, int is_float, void* stream) {
  if (n_segs <= 0) return 0;
  GEOBI_NOTNULL(segs);
  static_assert(sizeof(geobi_copy_seg_t) == sizeof(CopySeg) && offsetof(geobi_copy_seg_t, value) == offsetof(CopySeg, value),
                "the internal and the public segment struct are one layout");
  return concat32(reinterpret_cast<const CopySeg*>(segs), n_segs, is_float, as_stream(stream));
}
int geobi_gather_f32(const float* src, const int32_t* idx, int64_t n, float* dst, void* stream) {
  GEOBI_SIZES(0, n);
  return gather_f32(src, idx, n, dst, as_stream(stream));
}

int geobi_debug_exp_le0(const float* x, float* y, int64_t n, void* stream) {
  GEOBI_NOTNULL(x); GEOBI_NOTNULL(y);
  return exp_le0_probe(x, y, n, as_stream(stream));
}

size_t geobi_feast_wpack_floats(int Cin, int Cout) { return feast_wpack_floats(Cin, Cout); }

int geobi_feast_ldz(int Cin) { return feast_ldz(Cin); }
size_t geobi_feast_fwd_ws_bytes(int64_t N, int Cin, int Cout) { return feast_fwd_ws_bytes(N, Cin, Cout); }

static int check_channels(const char* fn, int Cin, int Cout) {
  bool in_ok = Cin == 6 || Cin == 12 || Cin == 32 || Cin == 64 || Cin == 128;
  bool out_ok = Cout == 32 || Cout == 64 || Cout == 128;
  if (!in_ok || !out_ok) return set_error("%s: unsupported channels Cin=%d Cout=%d", fn, Cin, Cout);
  return 0;
}

int geobi_feast_fwd(const float* xa, const float* xb, int Ca, int Cb, int64_t N, int64_t E,
                    const int32_t* rowptr_in, const int32_t* col_in, const float* lin_w, const float* u_w,
                    const float* c, const float* bias, int Cout, float slope, float* out, float* p, float* z,
                    float* wf, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(N, E);
  GEOBI_NOTNULL(xa); GEOBI_NOTNULL(rowptr_in); GEOBI_NOTNULL(lin_w); GEOBI_NOTNULL(u_w); GEOBI_NOTNULL(c); GEOBI_NOTNULL(bias);
  GEOBI_NOTNULL(out); GEOBI_NOTNULL(p);
  if (Cb > 0) GEOBI_NOTNULL(xb);
  if (E > 0) GEOBI_NOTNULL(col_in);
  GEOBI_TRY(check_channels(__func__, Ca + Cb, Cout));
  return feast_fwd(xa, Cb > 0 ? xb : nullptr, Ca, Cb, N, E, rowptr_in, col_in, lin_w, u_w, c, bias, Cout, slope, out,
                   p, z, wf, ws, ws_bytes, as_stream(stream));
}

size_t geobi_feast_bwd_ws_bytes(int64_t N, int64_t E, int Cin, int Cout) { return feast_bwd_ws_bytes(N, E, Cin, Cout); }

int geobi_feast_bwd(const float* xa, const float* xb, int Ca, int Cb, int64_t N, int64_t E,
                    const int32_t* rowptr_in, const int32_t* col_in, const int32_t* rowptr_out,
                    const int32_t* col_out, const int32_t* pos_in, const float* lin_w, const float* u_w,
                    const float* c, int Cout, float slope, const float* out, const float* gout, const float* p,
                    const float* z, const float* wf, float* dxa, float* dxb, float* dlin_w, float* du_w, float* dc,
                    float* dbias, int accumulate, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(N, E);
  GEOBI_NOTNULL(xa); GEOBI_NOTNULL(rowptr_in); GEOBI_NOTNULL(rowptr_out); GEOBI_NOTNULL(lin_w); GEOBI_NOTNULL(u_w); GEOBI_NOTNULL(c);
  GEOBI_NOTNULL(gout); GEOBI_NOTNULL(p); GEOBI_NOTNULL(dlin_w); GEOBI_NOTNULL(du_w); GEOBI_NOTNULL(dc); GEOBI_NOTNULL(dbias);
  if (slope != 1.0f) GEOBI_NOTNULL(out);
  if (Cb > 0) { GEOBI_NOTNULL(xb); if (dxa) GEOBI_NOTNULL(dxb); }
  if (E > 0) { GEOBI_NOTNULL(col_in); GEOBI_NOTNULL(col_out); GEOBI_NOTNULL(pos_in); }
  GEOBI_TRY(check_channels(__func__, Ca + Cb, Cout));
  return feast_bwd(xa, Cb > 0 ? xb : nullptr, Ca, Cb, N, E, rowptr_in, col_in, rowptr_out, col_out, pos_in, lin_w,
                   u_w, c, Cout, slope, out, gout, p, z, wf, dxa, dxb, dlin_w, du_w, dc, dbias, accumulate, ws, ws_bytes,
                   as_stream(stream));
}

int geobi_edge_weight_t10(const float* x, int C, const int32_t* row, const int32_t* col, const float* w_in,
                          int64_t E, float* w_out, void* stream) {
  GEOBI_SIZES(0, E);
  if (E > 0) { GEOBI_NOTNULL(x); GEOBI_NOTNULL(row); GEOBI_NOTNULL(col); GEOBI_NOTNULL(w_out); }
  return edge_weight_t10(x, C, row, col, w_in, E, w_out, as_stream(stream));
}

int geobi_edge_weight_att(const float* x, int C, const float* att_l, const float* att_r, const int32_t* row,
                          const int32_t* col, const float* w_in, int64_t N, int64_t E, float* node_ws, float* w_out,
                          void* stream) {
  GEOBI_SIZES(N, E);
  if (E > 0 && N > 0) {
    GEOBI_NOTNULL(x); GEOBI_NOTNULL(att_l); GEOBI_NOTNULL(att_r); GEOBI_NOTNULL(row); GEOBI_NOTNULL(col);
    GEOBI_NOTNULL(node_ws); GEOBI_NOTNULL(w_out);
  }
  return edge_weight_att(x, C, att_l, att_r, row, col, w_in, N, E, node_ws, w_out, as_stream(stream));
}

size_t geobi_match_ws_bytes(int64_t N) { return match_ws_bytes(N); }
int geobi_match_heavy_edge(const int32_t* rowptr, const int32_t* col, const float* w, int64_t N, int rounds,
                           int init, int32_t* cluster, int32_t* cluster_final, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(N, 0);
  GEOBI_NOTNULL(rowptr); GEOBI_NOTNULL(cluster); GEOBI_NOTNULL(status);
  return match_heavy_edge(rowptr, col, w, N, rounds, init, cluster, cluster_final, status, ws, ws_bytes, as_stream(stream));
}

int geobi_set_match_round_cap(int cap) { set_match_round_cap(cap); return 0; }
int geobi_set_match_scanfree(int on) { set_match_scanfree(on); return 0; }
int geobi_set_scan_lookback(int on) { set_scan_lookback(on); return 0; }
int geobi_set_tile_rows(int rows) { return set_tile_rows(rows); }
int geobi_set_head_precision(int mode) { return set_head_precision(mode); }
int geobi_set_rowpass_form(int staged, int chunked64) { return set_rowpass_form(staged, chunked64); }
int geobi_set_column_parts(int parts) { return set_column_parts(parts); }

size_t geobi_match_coarsen_ws_bytes(int64_t N) { return match_coarsen_ws_bytes(N); }
int geobi_match_coarsen(const int32_t* rowptr, const int32_t* col, const float* w, int64_t N, int rounds, int init,
                        int32_t* state, int32_t* cluster_final, int32_t* cnew, int32_t* segptr, int32_t* members,
                        int32_t* counters, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(N, 0);
  GEOBI_NOTNULL(rowptr); GEOBI_NOTNULL(state); GEOBI_NOTNULL(cluster_final); GEOBI_NOTNULL(cnew);     // col: NULL when E = 0
  GEOBI_NOTNULL(segptr); GEOBI_NOTNULL(members); GEOBI_NOTNULL(counters); GEOBI_NOTNULL(ws);
  return match_coarsen(rowptr, col, w, N, rounds, init, state, cluster_final, cnew, segptr, members, counters, ws,
                       ws_bytes, as_stream(stream));
}

int geobi_debug_match_coarsen_rowinfo(const int32_t* rowptr, const int32_t* col, const float* w, int64_t N, int rounds,
                                      int init, int32_t* state, int32_t* cluster_final, int32_t* cnew, int32_t* segptr,
                                      int32_t* members, int32_t* counters, int32_t* rowinfo, int32_t* rowinfo_made,
                                      void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(N, 0);
  GEOBI_NOTNULL(rowptr); GEOBI_NOTNULL(state); GEOBI_NOTNULL(cluster_final); GEOBI_NOTNULL(cnew); GEOBI_NOTNULL(segptr);
  GEOBI_NOTNULL(members); GEOBI_NOTNULL(counters); GEOBI_NOTNULL(rowinfo); GEOBI_NOTNULL(rowinfo_made); GEOBI_NOTNULL(ws);
  bool made = false;
  GEOBI_TRY(match_coarsen(rowptr, col, w, N, rounds, init, state, cluster_final, cnew, segptr, members, counters, ws,
                          ws_bytes, as_stream(stream), rowinfo, &made));
  *rowinfo_made = made ? 1 : 0;
  return 0;
}

size_t geobi_debug_scan_ws_bytes(int64_t n) { return scan_ws_bytes(n); }
int geobi_debug_scan_exclusive_i32(const int32_t* in, int32_t* out, int64_t n, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(0, n);
  if (n <= 0) return 0;
  GEOBI_NOTNULL(in); GEOBI_NOTNULL(out); GEOBI_NOTNULL(ws);
  GEOBI_REQUIRE(ws_bytes >= scan_ws_bytes(n), "%s: workspace too small (%zu < %zu)", __func__, ws_bytes, scan_ws_bytes(n));
  return scan_exclusive_i32(ws, ws_bytes, in, out, n, as_stream(stream));
}
int geobi_debug_scan_exclusive_i32_pair(const int32_t* in_a, const int32_t* in_b, int32_t* out_a, int32_t* out_b, int64_t n,
                                        void* stream) {
  GEOBI_SIZES(0, n);
  if (n <= 0) return 0;
  GEOBI_NOTNULL(in_a); GEOBI_NOTNULL(in_b); GEOBI_NOTNULL(out_a); GEOBI_NOTNULL(out_b);
  GEOBI_REQUIRE(n <= kSmallScan, "%s: n = %lld, the pair scan takes at most 2^18 elements", __func__, (long long)n);
  return scan_exclusive_i32_pair(in_a, in_b, out_a, out_b, n, as_stream(stream));
}

size_t geobi_relabel_ws_bytes(int64_t N) { return relabel_ws_bytes(N); }
int geobi_relabel_compact(const int32_t* cluster, int64_t N, int rep_is_self, int32_t* cnew, int32_t* count,
                          void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(N, 0);
  GEOBI_NOTNULL(cluster); GEOBI_NOTNULL(cnew); GEOBI_NOTNULL(count);
  return relabel_compact(cluster, N, rep_is_self, cnew, count, ws, ws_bytes, as_stream(stream));
}

size_t geobi_segment_csr_ws_bytes(int64_t n) { return segment_csr_ws_bytes(n); }
int geobi_segment_csr(const int32_t* seg, int64_t n, int64_t nseg, int32_t* segptr, int32_t* members, void* ws,
                      size_t ws_bytes, void* stream) {
  GEOBI_SIZES(nseg, n);          // n counts list entries (3 F corners of a face table): an edge-like count
  GEOBI_NOTNULL(segptr);
  return segment_csr(seg, n, nseg, segptr, members, ws, ws_bytes, as_stream(stream));
}
size_t geobi_segment_pairs_ws_bytes(int64_t nseg) { return segment_pairs_ws_bytes(nseg); }
int geobi_segment_csr_pairs(const int32_t* cnew, const int32_t* raw, int64_t N, int64_t nseg, int32_t* segptr,
                            int32_t* members, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(N, 0);
  GEOBI_NOTNULL(cnew); GEOBI_NOTNULL(raw); GEOBI_NOTNULL(segptr); GEOBI_NOTNULL(members);
  return segment_csr_pairs(cnew, raw, N, nseg, segptr, members, ws, ws_bytes, as_stream(stream));
}
int geobi_segment_csr_compose(const int32_t* segptr1, const int32_t* members1, const int32_t* segptr2,
                              const int32_t* members2, int64_t nseg2, int64_t n_fine, int32_t* segptr12,
                              int32_t* members12, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(n_fine, 0);
  GEOBI_NOTNULL(segptr1); GEOBI_NOTNULL(members1); GEOBI_NOTNULL(segptr2); GEOBI_NOTNULL(members2);
  GEOBI_NOTNULL(segptr12); GEOBI_NOTNULL(members12);
  return segment_csr_compose(segptr1, members1, segptr2, members2, nseg2, n_fine, segptr12, members12, ws, ws_bytes,
                             as_stream(stream));
}
int geobi_segment_max_fwd(const float* x, int C, const int32_t* segptr, const int32_t* members, int64_t nseg,
                          float* out, int32_t* arg, void* stream) {
  GEOBI_SIZES(nseg, 0);
  return segment_max_fwd(x, C, segptr, members, nseg, out, arg, as_stream(stream));
}
int geobi_segment_max_bwd(const float* gout, const int32_t* arg, const int32_t* seg, int C, int64_t nseg,
                          int64_t n_fine, float* gx, void* stream) {
  GEOBI_SIZES(n_fine, 0);
  return segment_max_bwd(gout, arg, seg, C, nseg, n_fine, gx, as_stream(stream));
}
int geobi_debug_segment_max2_fwd(const float* x, int C, const int32_t* segptr1, const int32_t* members1,
                                 const int32_t* segptr2, const int32_t* members2, int64_t nseg2, float* out,
                                 int32_t* arg12, void* stream) {
  GEOBI_SIZES(nseg2, 0);
  GEOBI_REQUIRE(C > 0, "%s: C = %d", __func__, C);
  if (nseg2 > 0) {
    GEOBI_NOTNULL(x); GEOBI_NOTNULL(segptr1); GEOBI_NOTNULL(members1); GEOBI_NOTNULL(segptr2); GEOBI_NOTNULL(members2);
    GEOBI_NOTNULL(out); GEOBI_NOTNULL(arg12);
  }
  return segment_max2_fwd(x, C, segptr1, members1, segptr2, members2, nseg2, out, arg12, as_stream(stream));
}
int geobi_debug_segment_max2_bwd(const float* gout, const int32_t* arg12, const int32_t* seg12, int C, int64_t nseg2,
                                 int64_t n_fine, float* gx, int add, void* stream) {
  GEOBI_SIZES(n_fine, 0);
  GEOBI_SIZES(nseg2, 0);
  GEOBI_REQUIRE(C > 0, "%s: C = %d", __func__, C);
  if (n_fine > 0) { GEOBI_NOTNULL(gout); GEOBI_NOTNULL(arg12); GEOBI_NOTNULL(seg12); GEOBI_NOTNULL(gx); }
  return segment_max2_bwd(gout, arg12, seg12, C, nseg2, n_fine, gx, add, as_stream(stream));
}
int geobi_debug_segment_sum2(const float* x, int C, const int32_t* segptr1, const int32_t* members1,
                             const int32_t* segptr2, const int32_t* members2, int64_t nseg2, float* out, void* stream) {
  GEOBI_SIZES(nseg2, 0);
  GEOBI_REQUIRE(C > 0, "%s: C = %d", __func__, C);
  if (nseg2 > 0) {
    GEOBI_NOTNULL(x); GEOBI_NOTNULL(segptr1); GEOBI_NOTNULL(members1); GEOBI_NOTNULL(segptr2); GEOBI_NOTNULL(members2);
    GEOBI_NOTNULL(out);
  }
  return segment_sum2(x, C, segptr1, members1, segptr2, members2, nseg2, out, as_stream(stream));
}
int geobi_segment_sum(const float* x, int C, const int32_t* segptr, const int32_t* members, int64_t nseg, int mean,
                      float* out, void* stream) {
  GEOBI_SIZES(nseg, 0);
  return segment_sum(x, C, segptr, members, nseg, mean, out, as_stream(stream));
}
int geobi_segment_mean_bwd(const float* gout, const int32_t* seg, const int32_t* segptr, int C, int64_t n_fine,
                           float* gx, void* stream) {
  GEOBI_SIZES(n_fine, 0);
  return segment_mean_bwd(gout, seg, segptr, C, n_fine, gx, as_stream(stream));
}
int geobi_gather_rows(const float* x, const int32_t* idx, int C, int64_t n_out, float* out, void* stream) {
  GEOBI_SIZES(n_out, 0);
  return gather_rows(x, idx, C, n_out, out, as_stream(stream));
}
size_t geobi_pool_edge_rows_ws_bytes(int64_t nbound) { return pool_edge_rows_ws_bytes(nbound); }
int geobi_pool_edge_rows(const int32_t* cnew, const int32_t* segptr, const int32_t* members, const int32_t* rowptr,
                         const int32_t* col, const float* w, const int32_t* ncount, int64_t nbound,
                         int32_t* rowptr_c, int32_t* row_c, int32_t* col_c, float* w_c, int32_t* count,
                         int32_t* overflow, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(nbound, 0);
  GEOBI_NOTNULL(cnew); GEOBI_NOTNULL(segptr); GEOBI_NOTNULL(members); GEOBI_NOTNULL(rowptr); GEOBI_NOTNULL(ncount);
  GEOBI_NOTNULL(rowptr_c); GEOBI_NOTNULL(row_c); GEOBI_NOTNULL(col_c); GEOBI_NOTNULL(count); GEOBI_NOTNULL(overflow);
  return pool_edge_rows(cnew, segptr, members, rowptr, col, w, ncount, nbound, rowptr_c, row_c, col_c, w_c, count,
                        overflow, ws, ws_bytes, as_stream(stream));
}
size_t geobi_debug_pool_edge_rows_onepass_ws_bytes(int64_t nbound, int64_t E) {
  return pool_edge_rows_ws_bytes_onepass(nbound, E);
}
int geobi_debug_pool_edge_rows_onepass(const int32_t* cnew, const int32_t* segptr, const int32_t* members,
                                       const int32_t* rowptr, const int32_t* col, const float* w, const int32_t* ncount,
                                       int64_t nbound, int64_t E_fine, const int32_t* rowinfo_in, int32_t* rowptr_c,
                                       int32_t* row_c, int32_t* col_c, float* w_c, int32_t* count, int32_t* overflow,
                                       void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(nbound, E_fine);
  GEOBI_REQUIRE(E_fine > 0, "%s: the one-pass form needs the fine edge count (E_fine = %lld)", __func__, (long long)E_fine);
  GEOBI_NOTNULL(cnew); GEOBI_NOTNULL(segptr); GEOBI_NOTNULL(members); GEOBI_NOTNULL(rowptr); GEOBI_NOTNULL(col);
  GEOBI_NOTNULL(ncount); GEOBI_NOTNULL(rowptr_c); GEOBI_NOTNULL(row_c); GEOBI_NOTNULL(col_c); GEOBI_NOTNULL(count);
  GEOBI_NOTNULL(overflow); GEOBI_NOTNULL(ws);
  if (w != nullptr) GEOBI_NOTNULL(w_c);
  return pool_edge_rows(cnew, segptr, members, rowptr, col, w, ncount, nbound, rowptr_c, row_c, col_c, w_c, count,
                        overflow, ws, ws_bytes, as_stream(stream), E_fine, rowinfo_in);
}
size_t geobi_pool_edge_ws_bytes(int64_t E) { return pool_edge_ws_bytes(E); }
int geobi_pool_edge(const int32_t* cnew, const int32_t* row, const int32_t* col, const float* w, int64_t E,
                    int64_t nmax, int32_t* rowptr_c, int32_t* row_c, int32_t* col_c, float* w_c, int32_t* count,
                    void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(nmax, E);
  GEOBI_NOTNULL(cnew); GEOBI_NOTNULL(rowptr_c); GEOBI_NOTNULL(count);
  return pool_edge(cnew, row, col, w, E, nmax, rowptr_c, row_c, col_c, w_c, count, ws, ws_bytes, as_stream(stream));
}

int geobi_face_geom_fwd(const float* verts, const int32_t* fv, const float* xf, int ldxf, int64_t F, float* out,
                        void* stream) {
  GEOBI_SIZES(F, 0);
  return face_geom_fwd(verts, fv, xf, ldxf, F, out, as_stream(stream));
}
int geobi_face_geom_bwd(const float* verts, const int32_t* fv, const float* gout, int64_t F, float* corner_grad,
                        void* stream) {
  GEOBI_SIZES(F, 0);
  return face_geom_bwd(verts, fv, gout, F, corner_grad, as_stream(stream));
}

int geobi_head_fwd(const float* x, int Cin, int64_t N, const float* w1, const float* b1, int K, const float* w2,
                   const float* b2, int nout, float slope, int mode, const float* dd, const float* resid,
                   int ld_resid, float* h, float* raw, float* out, void* stream) {
  GEOBI_SIZES(N, 0);
  GEOBI_NOTNULL(x); GEOBI_NOTNULL(w1); GEOBI_NOTNULL(b1); GEOBI_NOTNULL(w2); GEOBI_NOTNULL(b2);
  GEOBI_NOTNULL(raw); GEOBI_NOTNULL(out);
  if (mode == 0) GEOBI_NOTNULL(resid);
  return head_fwd(x, Cin, N, w1, b1, K, w2, b2, nout, slope, mode, dd, resid, ld_resid, h, raw, out, as_stream(stream));
}
size_t geobi_head_bwd_ws_bytes(int64_t N, int Cin, int K) { return head_bwd_ws_bytes(N, Cin, K); }
int geobi_head_bwd(const float* x, int Cin, int64_t N, const float* w1, const float* b1, int K, const float* w2,
                   int nout, float slope, int mode, const float* dd, const float* h, const float* raw, const float* gout,
                   float* dx, float* dw1, float* db1, float* dw2, float* db2, int accumulate, void* ws,
                   size_t ws_bytes, void* stream) {
  GEOBI_SIZES(N, 0);
  GEOBI_NOTNULL(x); GEOBI_NOTNULL(w1); GEOBI_NOTNULL(w2); GEOBI_NOTNULL(raw); GEOBI_NOTNULL(gout);
  GEOBI_NOTNULL(dw1); GEOBI_NOTNULL(db1); GEOBI_NOTNULL(dw2); GEOBI_NOTNULL(db2);
  return head_bwd(x, Cin, N, w1, b1, K, w2, nout, slope, mode, dd, h, raw, gout, dx, dw1, db1, dw2, db2, accumulate, ws,
                  ws_bytes, as_stream(stream));
}

size_t geobi_row_loss_ws_bytes(int64_t n) { return row_loss_ws_bytes(n); }
int geobi_row_loss_fwd(const float* a, const float* b, const float* w, int64_t n, int kind, float scale, float* out,
                       void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(n, 0);
  GEOBI_NOTNULL(a); GEOBI_NOTNULL(b); GEOBI_NOTNULL(out);
  return row_loss_fwd(a, b, w, n, kind, scale, out, ws, ws_bytes, as_stream(stream));
}
int geobi_row_loss_bwd(const float* a, const float* b, const float* w, const float* gout, int64_t n, int kind,
                       float scale, float* ga, void* stream) {
  GEOBI_SIZES(n, 0);
  GEOBI_NOTNULL(a); GEOBI_NOTNULL(b); GEOBI_NOTNULL(gout); GEOBI_NOTNULL(ga);
  return row_loss_bwd(a, b, w, gout, n, kind, scale, ga, as_stream(stream));
}

int geobi_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                    float weight_decay, float bias_corr1, float bias_corr2, void* stream) {
  GEOBI_NOTNULL(p); GEOBI_NOTNULL(g); GEOBI_NOTNULL(m); GEOBI_NOTNULL(v);
  return adam_flat(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, as_stream(stream));
}

int geobi_rotate_parts(const int64_t* part_ptr, int P, const float* R, float* x, int ldx, int x_triples, float* y, float* dd,
                       int64_t n, void* stream) {
  GEOBI_SIZES(n, 0);
  if (P < 1) return set_error("%s: P = %d parts (at least one)", __func__, P);
  GEOBI_NOTNULL(part_ptr); GEOBI_NOTNULL(R);
  if (x_triples < 0 || ldx < 3 * x_triples)
    return set_error("%s: ldx = %d is shorter than the x_triples = %d column triples to turn", __func__, ldx, x_triples);
  if (part_ptr[0] != 0 || part_ptr[P] != n)
    return set_error("%s: part_ptr runs from %lld to %lld, not from 0 to n = %lld", __func__, (long long)part_ptr[0],
                     (long long)part_ptr[P], (long long)n);
  for (int p = 0; p < P; ++p)
    if (part_ptr[p + 1] < part_ptr[p]) return set_error("%s: part_ptr decreases at part %d", __func__, p);
  if (n == 0) return 0;
  GEOBI_NOTNULL(x);
  return rotate_parts(part_ptr, P, R, x, ldx, x_triples, y, dd, as_stream(stream));
}

size_t geobi_update_position_ws_bytes(int64_t V, int64_t F) { return update_position_ws_bytes(V, F); }
int geobi_update_position2(const float* points, const int32_t* fv, const int32_t* vf, int maxval,
                           const float* normals, const float* dd, int64_t V, int64_t F, int n_iter, float* out,
                           void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(V > F ? V : F, 0);
  GEOBI_NOTNULL(points); GEOBI_NOTNULL(fv); GEOBI_NOTNULL(vf); GEOBI_NOTNULL(normals); GEOBI_NOTNULL(out);
  return update_position2(points, fv, vf, maxval, normals, dd, V, F, n_iter, out, ws, ws_bytes, as_stream(stream));
}

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

int geobi_gemm_nn(const float* A, int lda, const float* B, int ldb, int transB, float* C, int ldc, int M, int N,
                  int K, const float* bias, float slope, void* stream) {
  GEOBI_NOTNULL(A); GEOBI_NOTNULL(B); GEOBI_NOTNULL(C);
  GemmEpilogue ep;
  ep.bias = bias;
  ep.slope = slope;
  return gemm_nn(A, lda, B, ldb, transB, C, ldc, M, N, K, ep, as_stream(stream));
}
size_t geobi_gemm_tn_ws_bytes(int I, int J, int64_t M) { return gemm_tn_ws_bytes(I, J, M); }
int geobi_gemm_tn(const float* A, int lda, const float* B, int ldb, int64_t M, int I, int J, float* C, int ldc,
                  void* ws, size_t ws_bytes, void* stream) {
  GEOBI_NOTNULL(A); GEOBI_NOTNULL(B); GEOBI_NOTNULL(C);
  TnOutput o;
  o.C = C;
  o.ldc = ldc;
  return gemm_tn(A, lda, B, ldb, M, I, J, -1, -1, o, ws, ws_bytes, as_stream(stream));
}

// The two products with every argument their launchers take, and what the launcher decided (include/geobi_hip.h)
int geobi_debug_gemm_nn(const float* A, int lda, const float* B, int ldb, int transB, float* C, int ldc, int M, int N,
                        int K, const float* bias, float slope, float* C1, int split, int ldc1, void* ws, size_t ws_bytes,
                        int fixed_slices, int cfg, int64_t* plan, void* stream) {
  GEOBI_NOTNULL(A); GEOBI_NOTNULL(B); GEOBI_NOTNULL(C); GEOBI_NOTNULL(plan);
  GEOBI_REQUIRE(cfg >= 0 && cfg <= 5, "%s: cfg = %d (0: the launcher's choice, 1..5: a GEOBI_NN_CFG shape)", __func__, cfg);
  GEOBI_REQUIRE(C1 == nullptr || (split >= 0 && split <= N && ldc1 >= N - split && ldc >= split),
                "%s: split = %d, ldc = %d, ldc1 = %d do not hold N = %d columns", __func__, split, ldc, ldc1, N);
  GemmEpilogue ep;
  ep.bias = bias; ep.slope = slope;
  ep.C1 = C1; ep.split = split; ep.ldc1 = ldc1;
  ep.ws = ws; ep.ws_bytes = ws_bytes; ep.fixed_slices = fixed_slices;
  NnPlan p;
  const int rc = gemm_nn(A, lda, B, ldb, transB, C, ldc, M, N, K, ep, as_stream(stream), cfg, &p);
  const int64_t v[8] = {p.fast, p.shape, p.wm * 1000 + p.wn * 100 + p.tm * 10 + p.tn, p.bk, p.slices, p.k_chunk, p.wide,
                        p.slices > 1};
  for (int i = 0; i < 8; ++i) plan[i] = v[i];
  return rc;
}
int geobi_debug_gemm_tn(const float* A, int lda, const float* B, int ldb, int64_t M, int I, int J, int ones_row,
                        int ones_col, int sum_row, int mode, float* C, int ldc, float* C2, float* C3, float* C4, int Cin,
                        int Cout, int col0, int extra_row, int extra_col, int accumulate, void* ws, size_t ws_bytes,
                        int64_t* plan, void* stream) {
  GEOBI_NOTNULL(A); GEOBI_NOTNULL(B); GEOBI_NOTNULL(C); GEOBI_NOTNULL(plan);
  GEOBI_REQUIRE(mode >= TN_PLAIN && mode <= TN_RPRIME, "%s: mode = %d (0 plain, 1 lin-unpack, 2 du/dc, 3 r')", __func__, mode);
  if (mode == TN_PLAIN && (extra_row || extra_col)) GEOBI_NOTNULL(C2);
  if (mode == TN_LIN_UNPACK) GEOBI_NOTNULL(C2);
  TnOutput o;
  o.mode = mode; o.C = C; o.ldc = ldc; o.C2 = C2; o.C3 = C3; o.C4 = C4;
  o.Cin = Cin; o.Cout = Cout; o.col0 = col0;
  o.extra_row = extra_row; o.extra_col = extra_col; o.accumulate = accumulate;
  TnPlan p;
  const int rc = gemm_tn(A, lda, B, ldb, M, I, J, ones_row, ones_col, o, ws, ws_bytes, as_stream(stream), sum_row, &p);
  const int64_t v[8] = {p.va, p.ti, p.tj, p.tiles_i, p.tiles_j, p.blocks_y, p.m_per_slice, p.bias_blocks};
  for (int i = 0; i < 8; ++i) plan[i] = v[i];
  return rc;
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
