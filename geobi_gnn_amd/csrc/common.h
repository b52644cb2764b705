// Internal host/device helpers shared by the HIP translation units of libgeobi_hip.so.
// gfx950 (MI355X) only: 64-lane wavefronts are assumed throughout.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <stdlib.h>

#include <atomic>
#include <type_traits>

#define GEOBI_H 9    // FeaSt heads on the hot path (network.py:258-268 always passes 9)
#define GEOBI_HP 12  // row stride (floats) of per-node / per-edge head vectors: 9 padded to 3 x float4

namespace geobi {

int set_error(const char* fmt, ...);

#define GEOBI_HIP(expr)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return ::geobi::set_error("%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
  } while (0)
#define GEOBI_LAUNCH_OK() GEOBI_HIP(hipGetLastError())
#define GEOBI_TRY(expr)        \
  do {                         \
    int r_ = (expr);           \
    if (r_ != 0) return r_;    \
  } while (0)
#define GEOBI_REQUIRE(cond, ...)                          \
  do {                                                    \
    if (!(cond)) return ::geobi::set_error(__VA_ARGS__);  \
  } while (0)

// ---- argument checks of the extern "C" entry points: an entry point is defined in the unit that implements
// it and runs these first.  Size limits of the header (GEOBI_MAX_NODES / GEOBI_MAX_EDGES): every entry point that takes a
// node or edge count rejects what is above them, so that no kernel ever forms a 32-bit element index beyond its range.
int sizes_ok(const char* fn, int64_t nodes, int64_t edges);      // capi.hip
#define GEOBI_NOTNULL(p)                                                          \
  do {                                                                            \
    if ((p) == nullptr) return ::geobi::set_error("%s: %s is NULL", __func__, #p); \
  } while (0)
#define GEOBI_SIZES(nodes, edges) GEOBI_TRY(::geobi::sizes_ok(__func__, (int64_t)(nodes), (int64_t)(edges)))
// the face and vertex counts of a mesh: the larger within the limit, the smaller not negative
#define GEOBI_MESH_SIZES(F, V)             \
  GEOBI_SIZES((F) > (V) ? (F) : (V), 0);   \
  GEOBI_SIZES((F) < (V) ? (F) : (V), 0)
static inline hipStream_t as_stream(void* stream) { return (hipStream_t)stream; }

static inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }
static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// ---- Knob: a switch the environment decides until a geobi_set_* hook sets it.  One relaxed atomic: it may be set while
// other host threads launch.  A knob is a file-local object next to the code it switches (name NULL: no variable).
struct Knob {
  static constexpr long long kUnread = INT64_MIN;
  const char* name;
  long long unset;                                  // the value when the variable is not set
  std::atomic<long long> v{kUnread};
  constexpr Knob(const char* name_, long long unset_) : name(name_), unset(unset_) {}
  long long env() const {
    const char* e = name ? getenv(name) : nullptr;
    return e ? atoll(e) : unset;
  }
  long long get() {
    long long x = v.load(std::memory_order_relaxed);
    if (x != kUnread) return x;
    const long long e = env();                      // first use; a set() that lands meanwhile wins
    return v.compare_exchange_strong(x, e, std::memory_order_relaxed) ? e : x;
  }
  bool on() { return get() != 0; }
  void set(long long x) { v.store(x, std::memory_order_relaxed); }
  void reset() { set(env()); }                      // back to what the environment says
};

// ---- a run-time int as a template argument: fn(std::integral_constant<int, V>) for the V of the list that equals v.
// kNoCase: v is not in the list (or fn pruned the case with `if constexpr`); the caller reports it in its own words.
constexpr int kNoCase = INT32_MIN;
template <int... Vs, typename Fn>
static inline int dispatch_int(int v, Fn&& fn) {
  int rc = kNoCase;
  (void)((v == Vs && (rc = fn(std::integral_constant<int, Vs>{}), true)) || ...);
  return rc;
}

// ---- more dynamic LDS than the default limit: the opt-in of one kernel, once per process
template <auto kKernel>
static inline int allow_dynamic_lds(size_t bytes) {
  static std::atomic<bool> done{false};   // several host threads may launch (one per mesh group)
  if (!done.load(std::memory_order_relaxed)) {
    GEOBI_HIP(hipFuncSetAttribute((const void*)kKernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    done.store(true, std::memory_order_relaxed);
  }
  return 0;
}

struct SubWs { void* p; size_t bytes; };   // a workspace inside a workspace
// bump allocator over a caller-provided workspace (no hipMalloc on the hot path)
struct Arena {
  char* base;
  size_t off, cap;
  bool dry;             // dry run: only measure
  bool failed = false;  // a nested size query failed
  Arena(void* p, size_t bytes) : base((char*)p), off(0), cap(bytes), dry(p == nullptr) {}
  template <typename T>
  T* take(size_t n) {
    size_t o = align_up(off);
    off = o + n * sizeof(T);
    if (dry) return nullptr;
    return (off <= cap) ? (T*)(base + o) : nullptr;
  }
  // a nested workspace, sized by its own *_ws_bytes or temp-size query (0: that query failed, and so does this carve)
  SubWs take_ws(size_t bytes) {
    if (bytes == 0) failed = true;
    return {take<char>(bytes), bytes};
  }
  bool ok() const { return !failed && (dry || off <= cap); }
};

// ---- the workspace rule: a launcher's takes live in ONE carve, a function that returns its buffers (a
// braced list: the takes run in the order written); its *_ws_bytes is carve_bytes of that carve (a dry run), the launcher
// runs the same carve over the caller's memory and checks it with GEOBI_WS_CHECK.
constexpr size_t kWsSlack = 256;       // beyond the last take: the one slack constant of every workspace size
template <typename Carve>
static inline size_t carve_bytes(Carve&& carve) {
  Arena a(nullptr, 0);
  carve(a);
  return a.ok() ? align_up(a.off) + kWsSlack : 0;
}
#define GEOBI_WS_CHECK(fn, a, ws, ws_bytes)                                                                        \
  GEOBI_REQUIRE((a).ok() && (ws) != nullptr, "%s: workspace too small (%zu bytes given, %zu needed)", fn, \
                (size_t)(ws_bytes), (a).off)
// the launcher's half of the rule: b = carve(arena over the caller's memory), checked under the launcher's name
template <typename Buffers, typename Carve>
static inline int carve_checked(const char* what, void* ws, size_t ws_bytes, Buffers& b, Carve&& carve) {
  Arena a(ws, ws_bytes);
  b = carve(a);
  GEOBI_WS_CHECK(what, a, ws, ws_bytes);
  return 0;
}

// ---- mesh repair and topology (clean.hip, topo.hip): the state of a face, and the 48-bit key a << 24 | b of a
// half-edge (clean.hip: directed a -> b; topo.hip: undirected, a < b) -- vertex indices stay below 2^24
enum FaceState { kUndecided = 0, kKept = 1, kDropped = 2, kDegenerate = 3, kSmallPart = 4 };
constexpr unsigned kEdgeKeyBits = 48;
constexpr uint64_t kNoEdge = (1ull << kEdgeKeyBits) - 1;   // key of an excluded face's slots: a == b never is an edge
__host__ __device__ __forceinline__ uint64_t edge_key(int a, int b) { return (uint64_t)a << 24 | (uint64_t)b; }
// one atomic per wave for a count of lanes (integer adds: the total does not depend on their order)
__device__ __forceinline__ void count_lanes(bool mine, int* __restrict__ counter) {
  const unsigned long long m = __ballot(mine);
  if (m != 0 && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(counter, __popcll(m));
}

// ---- part table of a disjoint-union batch, carried in the kernel arguments: no copy of the host arrays, nothing out
// of stream order.  A launch takes kMaxParts parts; begin[k] .. begin[k + 1] are the rows of its part k.
constexpr int kMaxParts = 32;
template <typename T>
struct PartTable {
  T begin[kMaxParts + 1];
  int n;
};
// the parts base .. base + n of a host part pointer with P parts; the unused tail repeats the end: nothing is left unset
template <typename T>
static inline void fill_parts(PartTable<T>* tab, const int64_t* ptr, int base, int P) {
  tab->n = P - base < kMaxParts ? P - base : kMaxParts;
  for (int k = 0; k <= kMaxParts; ++k) tab->begin[k] = (T)ptr[base + (k < tab->n ? k : tab->n)];
}
// the table into LDS, where a lane indexes it by ITS part (the caller places the barrier)
template <typename T>
__device__ __forceinline__ void stage_parts(T* s_begin, const PartTable<T>& tab) {
  for (int k = threadIdx.x; k <= tab.n; k += blockDim.x) s_begin[k] = tab.begin[k];
}
// last part that starts at or before row i: an empty part never wins
template <typename T>
__device__ __forceinline__ int find_part(const T* begin, int n, T i) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (begin[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---- fp64 sum in a fixed order: an LDS tree over the kN threads of a block (halve from kN / 2 down to 1, a barrier
// per level), then the blocks' sums in ascending order.  The tree shape and the block order ARE the bits.
// `beside(h)` runs in the lanes below h at every level, for a second quantity folded by the same barriers.
template <int kN, typename Beside>
__device__ __forceinline__ double block_sum_fp64(double v, Beside beside) {
  __shared__ double s[kN];
  s[threadIdx.x] = v;
  __syncthreads();
  for (int h = kN / 2; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) {
      s[threadIdx.x] += s[threadIdx.x + h];
      beside(h);
    }
    __syncthreads();
  }
  return s[0];
}
template <int kN>
__device__ __forceinline__ double block_sum_fp64(double v) {
  return block_sum_fp64<kN>(v, [](int) {});
}
__device__ __forceinline__ double fold_ascending(const double* __restrict__ partial, int n, int stride = 1) {
  double s = 0.0;
  for (int b = 0; b < n; ++b) s += partial[(size_t)b * stride];
  return s;
}

// ---- optional per-kernel timing for bench.py's roofline object (events on the launch stream)
enum ProfKernel { PROF_NONE = 0, PROF_AGG_FWD = 1, PROF_AGG_BWD = 2, PROF_ROWPASS = 3, PROF_GEMM = 4, PROF_POOL_FORM = 5 };
// tags of PROF_POOL_FORM (scan.hip, match.hip): which form of a scan / of match_coarsen's tail a call took
enum PoolForm {
  POOL_FORM_SCAN_ONE_BLOCK = 1, POOL_FORM_SCAN_LOOKBACK = 2, POOL_FORM_SCAN_ROCPRIM = 3,
  POOL_FORM_MATCH_SCANFREE = 4, POOL_FORM_MATCH_TWOPASS_DUAL = 5
};
void prof_begin(int kernel, hipStream_t s, double alg_bytes, int tag);
void prof_end(int kernel, hipStream_t s);
// The same bracket for ONE kernel launched through hipExtLaunchKernelGGL: the two events are bound to the kernel's own
// dispatch (their elapsed time is the kernel's execution time, as a tracer reports it -- a pair of hipEventRecord packets
// around a launch adds ~4.7 us of its own).  prof_begin_launch hands the events to the launch site of this host thread,
// which takes them with prof_take_launch_events (false: not profiling, launch as usual).
void prof_begin_launch(int kernel, hipStream_t s, double alg_bytes, int tag);
bool prof_take_launch_events(hipEvent_t* start, hipEvent_t* stop);

// ---- side stream for work that is off the critical path of a backward call (weight gradients)
struct Fork {
  hipStream_t side = nullptr;   // nullptr: overlap disabled, run on the caller's stream
  hipEvent_t join = nullptr;
};
void side_override(int mode);                  // this host thread: 0 = no side stream, 1 = side stream, -1 = the process-wide setting
hipStream_t side_current();                    // the side stream this thread's last fork used (nullptr: none yet)
void side_select(int low_priority);            // which side stream the next forks use (default / lowest priority)
Fork fork_side_stream(hipStream_t main);       // side stream waits for everything enqueued on `main` so far
int join_side_stream(const Fork& f, hipStream_t main);   // `main` waits for the side stream
int side_wait_main(const Fork& f, hipStream_t main);     // side stream waits for `main` as of now

// ---- launchers that ANOTHER translation unit calls, grouped by the unit that defines them (all enqueue on `s`, never
// sync).  A launcher only its own entry point reaches has no prototype here: it is the body of that entry point

// ---- graph.hip; called by executor.hip
int csr_reverse_index(const int32_t* rowptr, const int32_t* row, const int32_t* col, int64_t E, int32_t* pos_rev,
                      int32_t* flag, hipStream_t s);

// ---- gemm.hip; called by feast.hip and geom.hip
struct GemmEpilogue {
  const float* bias = nullptr;  // [N] added per column
  float slope = 1.0f;           // leaky-relu negative slope (1 = identity)
  float* C1 = nullptr;          // optional split output: columns >= split go to C1 (ld = ldc1)
  int split = 0, ldc1 = 0;
  void* ws = nullptr;           // optional scratch for split-K partial sums (small-M GEMMs)
  size_t ws_bytes = 0;
  int fixed_slices = 0;         // > 0: split K exactly this way whatever M is (forward pass: keeps a
                                // node's result independent of how many other nodes are batched with it)
};
// split-K only engages for grids of < 512 small tiles, i.e. M * N < ~2.1 M elements
static inline size_t gemm_nn_ws_bytes(int64_t M, int N) {
  return (M * N < (int64_t)2200000) ? align_up((size_t)8 * M * N * sizeof(float)) + 256 : 256;
}
// forward GEMM of a FeaSt layer: the split is a function of the layer shape only
static inline int feast_fwd_slices(int Kp, int Cout) { return Kp >= 1024 ? 4 : ((Kp >= 512 && Cout >= 64) ? 2 : 1); }
static inline size_t gemm_nn_fixed_ws_bytes(int64_t M, int N, int slices) {
  size_t b = (size_t)slices * M * N * sizeof(float);
  return (slices > 1 && b <= ((size_t)256 << 20)) ? align_up(b) + 256 : 256;
}
// What a gemm_nn call decided on the host (the launch follows it; geobi_debug_gemm_nn reports it).  shape: the tile shape
// by its GEOBI_NN_CFG number, 0 = nothing was launched; slices > 1: split-K through ep.ws and the reduce kernel.
struct NnPlan { int fast = 0, shape = 0, wm = 0, wn = 0, tm = 0, tn = 0, bk = 0, slices = 0, k_chunk = 0, wide = 0; };
// cfg != 0: this call's tile shape, as GEOBI_NN_CFG of that value forces it for the process; ran: the plan that ran
int gemm_nn(const float* A, int lda, const float* B, int ldb, int transB, float* C, int ldc, int M, int N, int K,
            const GemmEpilogue& ep, hipStream_t s, int cfg = 0, NnPlan* ran = nullptr);
size_t gemm_tn_ws_bytes(int I, int J, int64_t M);
size_t gemm_tn_ws_bytes_any_width(int I, int J, int64_t M);   // max over column widths 1..J
enum TnOut { TN_PLAIN = 0, TN_LIN_UNPACK = 1, TN_DU_DC = 2, TN_RPRIME = 3 };
struct TnOutput {
  int mode = TN_PLAIN;
  float* C = nullptr;   // primary output
  int ldc = 0;
  float* C2 = nullptr;  // secondary output (bias gradient / c gradient)
  int Cin = 0, Cout = 0;
  int extra_row = 0, extra_col = 0;  // TN_PLAIN: last row / column is the implicit-ones one -> C2
  int accumulate = 0;   // != 0: add to what C / C2 hold (gradient accumulation) instead of overwriting
  // TN_RPRIME ([x | 1]^T [r | dp | dcs]): C = dlin, C2 = dbias, C3 = du, C4 = dc; col0 = first input channel of
  // this A operand (split inputs issue one GEMM per half)
  float* C3 = nullptr;
  float* C4 = nullptr;
  int col0 = 0;
};
// I, J: logical output sizes INCLUDING an implicit ones row / column when ones_row / ones_col >= 0, or the column-sums
// row (sum_row == I - 1: the sums of B's columns over the M rows, formed on the VALU beside the MFMAs; TnOutput.extra_row
// routes it).
// What a gemm_tn call decided on the host: the kernel instance <ti, tj, u, va> (va: the vector-A kernel), its grid
// (tiles_i x tiles_j output tiles, blocks_y blocks of four node slices of m_per_slice rows each = blocks_y slabs) and the
// extra bias blocks of the reduce kernel.  All zero: nothing was launched.
struct TnPlan {
  int ti = 0, tj = 0, va = 0, u = 0, tiles_i = 0, tiles_j = 0, slices = 0, blocks_y = 0, bias_blocks = 0;
  int64_t m_per_slice = 0;
};
int gemm_tn(const float* A, int lda, const float* B, int ldb, int64_t M, int I, int J, int ones_row, int ones_col,
            const TnOutput& o, void* ws, size_t ws_bytes, hipStream_t s, int sum_row = -1, TnPlan* ran = nullptr);

// ---- feast_fused.hip: the fused (aggregate -> LDS tile -> MFMA) kernels and their packed weights; called by feast.hip,
// the pack sizes and feast_fused_pack_batch by executor.hip too
size_t feast_fused_fwd_pack_floats(int Cin, int Cout);
size_t feast_fused_dx_pack_floats(int Cin, int Cout);
int feast_fused_pack_fwd(const float* lin_w, const float* c, int Cin, int Cout, float* bp, hipStream_t s);
// one launch for the packed forms of several layers
constexpr int kMaxPackBatch = 8;
struct FusedPackItem {
  const float* lin_w;
  const float* u_w;
  const float* c;
  int Cin, Cout;
  float* wf;     // [Kp, Cout] plain form (NULL: forward form only)
  float* bf;     // fragment-ordered forward weights
  float* bdx;    // fragment-ordered dx weights (with wf)
};
int feast_fused_pack_batch(const FusedPackItem* items, int n, hipStream_t s);
int feast_fused_pack_dx(const float* lin_w, const float* u_w, const float* c, int Cin, int Cout, float* bp, hipStream_t s);
int feast_fused_pack_all(const float* lin_w, const float* u_w, const float* c, int Cin, int Cout, int Kp, float* wf,
                         float* bf, float* bdx, hipStream_t s);
double feast_fused_bytes(int64_t N, int64_t E, int C, int nout);
// launch records: host-side only, filled by field name, passed by const reference down to the one
// place that spells a kernel's argument list.
// the layer input as every FeaSt kernel sees it; a second one describes the transposed graph the dx side walks
struct FeastIn {
  const float *xa = nullptr, *xb = nullptr;   // the two parts of a row; xb is never NULL (= xa when the input is unsplit)
  int Ca = 0;                                 // width of the first part (= the whole row when unsplit)
  const float *p = nullptr, *cvec = nullptr;
  const int *rowptr = nullptr, *col = nullptr;
  int N = 0, LC = 0;                          // LC: per-edge logit channels (0 / 6 / 12)
  const float* ul = nullptr;
};
// what feast_fused_kernel takes beyond the input
struct FusedLaunch {
  const int* deg_rowptr = nullptr;
  const float *xl = nullptr, *dpd = nullptr, *dl = nullptr;
  const int* pos = nullptr;
  const float *dpn = nullptr, *Bp = nullptr;
  int NOUT = 0;
  const float* bias = nullptr;
  float slope = 1.0f;
  float* out = nullptr;
  int ldo = 0;
  float* out1 = nullptr;
  int split = 0, ldo1 = 0;
  float* tile_out = nullptr;
};
// the backward row pass, fused (gout .. g_out: dz stays in LDS) or standalone (dz, ldz: dz from the plain GEMM)
struct RowpassLaunch {
  const float *gout = nullptr, *out_act = nullptr;
  float slope = 1.0f;
  const float* Wf = nullptr;
  int Kp = 0;
  float* g_out = nullptr;
  const float* dz = nullptr;
  int ldz = 0;
  float *dl = nullptr, *dpn = nullptr, *dcs = nullptr;
  int ld_dcs = 0;
};
int feast_fused_fwd(const FeastIn& in, int Cin, const float* Bp, int Cout, const float* bias, float slope, float* out,
                    hipStream_t s);
// gin: the rows of g [N, Cout] over the transposed CSR
int feast_fused_dx(const FeastIn& gin, const int* rowptr_in, const int* pos, const float* dl, const float* dpn,
                   const float* xl, const float* dpd, const float* Bp, int Cin, float* dxa, int Ca, float* dxb, int Cb,
                   float* tile_out, hipStream_t s);
bool feast_rowpass_fused_supported(int Cin, int Cb, int Cout);
int feast_rowpass_fused(const FeastIn& in, int Cin, int Cout, const RowpassLaunch& r, hipStream_t s);

// ---- feast.hip; called by executor.hip (feast_ldz by feast_fused.hip)
// packed-weight buffer shared by forward and backward: [Wf | W' | Bf (fused forward) | Bdx (fused dx)], with
// Wf [ldz(Cin), Cout] for z Wf / g Wf^T and W' [ldr(Cout), Cin] = [lin.weight ; u.weight ; 0] for dx = r' W'
static inline size_t feast_wpack_plain_floats(int Cin, int Cout) {
  return (size_t)((GEOBI_H * Cin + 3) / 4 * 4) * Cout + (size_t)(GEOBI_H * Cout + 2 * GEOBI_HP) * Cin;
}
static inline size_t feast_wpack_floats(int Cin, int Cout) {
  return feast_wpack_plain_floats(Cin, Cout) + feast_fused_fwd_pack_floats(Cin, Cout) +
         feast_fused_dx_pack_floats(Cin, Cout);
}
int feast_ldz(int Cin);
size_t feast_fwd_ws_bytes(int64_t N, int Cin, int Cout);
int feast_fwd(const float* xa, const float* xb, int Ca, int Cb, int64_t N, int64_t E, const int32_t* rowptr_in,
              const int32_t* col_in, const float* lin_w, const float* u_w, const float* cvec, const float* bias,
              int Cout, float slope, float* out, float* p, float* z, float* wf_out, void* ws, size_t ws_bytes,
              hipStream_t s, const float* bf_packed = nullptr);
size_t feast_bwd_ws_bytes(int64_t N, int64_t E, int Cin, int Cout);
size_t feast_bwd_ws_bytes_for(int64_t N, int64_t E, int Cin, int Cb, int Cout, bool need_dx);
int feast_bwd(const float* xa, const float* xb, int Ca, int Cb, int64_t N, int64_t E, const int32_t* rowptr_in,
              const int32_t* col_in, const int32_t* rowptr_out, const int32_t* col_out, const int32_t* pos_in,
              const float* lin_w, const float* u_w, const float* cvec, int Cout, float slope, const float* out,
              const float* gout, const float* p, const float* z, const float* wf_saved, float* dxa, float* dxb,
              float* dlin_w, float* du_w, float* dc, float* dbias, int accumulate, void* ws, size_t ws_bytes,
              hipStream_t s);

// ---- match.hip; called by executor.hip
int edge_weight_t10(const float* x, int C, const int32_t* row, const int32_t* col, const float* w_in, int64_t E,
                    float* w_out, hipStream_t s, int32_t* zero8 = nullptr);
size_t match_coarsen_ws_bytes(int64_t N);
int match_coarsen(const int32_t* rowptr, const int32_t* col, const float* w, int64_t N, int rounds, int init,
                  int32_t* state, int32_t* cluster_final, int32_t* cnew, int32_t* segptr, int32_t* members,
                  int32_t* counters, void* ws, size_t ws_bytes, hipStream_t s, void* rowinfo_out = nullptr,
                  bool* rowinfo_made = nullptr);

// ---- segment.hip; called by executor.hip
int segment_sum2(const float* x, int C, const int32_t* segptr1, const int32_t* members1, const int32_t* segptr2,
                 const int32_t* members2, int64_t nseg2, float* out, hipStream_t s);
int segment_max2_fwd(const float* x, int C, const int32_t* segptr1, const int32_t* members1, const int32_t* segptr2,
                     const int32_t* members2, int64_t nseg2, float* out, int32_t* arg12, hipStream_t s);
int segment_max2_bwd(const float* gout, const int32_t* arg12, const int32_t* seg12, int C, int64_t nseg2, int64_t n_fine,
                     float* gx, int add, hipStream_t s);
int segment_sum(const float* x, int C, const int32_t* segptr, const int32_t* members, int64_t nseg, int mean,
                float* out, hipStream_t s);
int segment_mean_bwd(const float* gout, const int32_t* seg, const int32_t* segptr, int C, int64_t n_fine, float* gx,
                     hipStream_t s);
int gather_rows(const float* x, const int32_t* idx, int C, int64_t n_out, float* out, hipStream_t s);

// ---- pool.hip; called by executor.hip
size_t pool_edge_rows_ws_bytes_onepass(int64_t nbound, int64_t E);
int pool_edge_rows(const int32_t* cnew, const int32_t* segptr, const int32_t* members, const int32_t* rowptr,
                   const int32_t* col, const float* w, const int32_t* ncount, int64_t nbound, int32_t* rowptr_c,
                   int32_t* row_c, int32_t* col_c, float* w_c, int32_t* count, int32_t* overflow, void* ws,
                   size_t ws_bytes, hipStream_t s, int64_t E_fine = 0, const void* rowinfo_in = nullptr,
                   const int32_t* publish_src = nullptr, int32_t* publish_host = nullptr, int publish_seq = 0);
size_t pool_edge_ws_bytes(int64_t E);
int pool_edge(const int32_t* cnew, const int32_t* row, const int32_t* col, const float* w, int64_t E, int64_t nmax,
              int32_t* rowptr_c, int32_t* row_c, int32_t* col_c, float* w_c, int32_t* count, void* ws,
              size_t ws_bytes, hipStream_t s);

// ---- scan.hip: the library's exclusive int scan (its own kernels, one launch and a 16-byte temporary, up to kSmallScan
// elements; rocPRIM above) and two scans of n <= kSmallScan elements in one launch.  The first two are what IntScan of
// device_steps.h runs, in every unit that carves one; the pair scan is called by match.hip
constexpr int64_t kSmallScan = 1 << 18;
size_t scan_ws_bytes(int64_t n);
int scan_exclusive_i32(void* temp, size_t temp_bytes, const int* in, int* out, int64_t n, hipStream_t s);
int scan_exclusive_i32_pair(const int* in_a, const int* in_b, int* out_a, int* out_b, int64_t n, hipStream_t s);

// ---- capi.hip: the one check of host part pointers (P >= 1, not NULL, start >= 0, no empty part, GEOBI_MAX_NODES rows);
// the entry points that take a union batch (dist.hip, chamfer.hip, icp.hip, sample.hip) run it first and rely on it
int parts_check(const char* fn, const int64_t* qptr, const int64_t* tptr, int P);

// ---- filter.hip; called by guided.hip
int bnf_spatial_factors(const float* rec_c, const int32_t* rowptr, const int32_t* col, int64_t F, int64_t E,
                        const float* inv2ss, float* wsp, hipStream_t s);

// ---- geom.hip; called by executor.hip
int face_geom_fwd(const float* verts, const int32_t* fv, const float* xf, int ldxf, int64_t F, float* out,
                  hipStream_t s);
int face_geom_bwd(const float* verts, const int32_t* fv, const float* g, int64_t F, float* corner_grad,
                  hipStream_t s);
int head_fwd(const float* x, int Cin, int64_t N, const float* w1, const float* b1, int K, const float* w2,
             const float* b2, int nout, float slope, int mode, const float* dd, const float* resid, int ld_resid,
             float* h, float* raw, float* out, hipStream_t s);
size_t head_bwd_ws_bytes(int64_t N, int Cin, int K);
int head_bwd(const float* x, int Cin, int64_t N, const float* w1, const float* b1, int K, const float* w2, int nout,
             float slope, int mode, const float* dd, const float* h, const float* raw, const float* gout, float* dx, float* dw1,
             float* db1, float* dw2, float* db2, int accumulate, void* ws, size_t ws_bytes, hipStream_t s);
size_t row_loss_ws_bytes(int64_t n);
int row_loss_fwd(const float* a, const float* b, const float* w, int64_t n, int kind, float scale, float* out,
                 void* ws, size_t ws_bytes, hipStream_t s);
int row_loss_bwd(const float* a, const float* b, const float* w, const float* gout, int64_t n, int kind,
                 float scale, float* ga, hipStream_t s);

// ---- head_fused.hip; called by geom.hip
bool head_fused_supported(int Cin, int K, int nout);
int head_fwd_fused(const float* x, int64_t N, const float* w1, const float* b1, const float* w2, const float* b2,
                   int nout, float slope, int mode, const float* dd, const float* resid, int ld_resid, float* raw,
                   float* out, hipStream_t s);
size_t head_bwd_fused_ws_bytes(int64_t N);
int head_bwd_fused(const float* x, int64_t N, const float* w1, const float* b1, const float* w2, int nout,
                   float slope, const float* graw, float* dx, float* dw1, float* db1, float* dw2, float* db2,
                   int accumulate, void* ws, size_t ws_bytes, hipStream_t s);

}  // namespace geobi
