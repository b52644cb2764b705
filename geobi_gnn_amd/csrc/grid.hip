// A uniform grid in front of the nearest-point and point-to-surface searches.
//
//   plan      the box of the FINITE targets (two-stage min / max, no float atomics), one read-back; the host picks the
//             per-axis resolution from the target count and the box alone (grid_resolution) and hands the caller a
//             16-word descriptor.  Triangles: a face is filed in every cell its bounding box meets, so the plan also
//             counts the entries and halves the resolution until they fit kEntryCap * F (one read-back per round, at
//             most kMaxRounds of them: one cell per axis gives at most F entries).
//   build     points: a cell id per target, ONE stable radix sort of (cell, index) -- indices ascend inside a cell --
//             and cell_start by a lower bound per cell.  Triangles: count, exclusive scan, emit (cell, face) in ascending
//             face order, the same sort; the 16-float records of dist_pairs.h written once, in face order.
//   search    one lane per query, the queries sorted by cell so that the lanes of a wave walk the same cells.  Chebyshev
//             shells r = 0, 1, 2, ... around the query's (clamped) cell; every entry of every visited cell goes through
//             pair_d2 / tri_d2 of dist_pairs.h, the TEXT the all-pairs walk of dist.hip compiles, and the minimum is kept
//             under the order (d2, index).  The walk stops after shell r when the distance from the query to everything
//             outside the visited block, minus the margin derived in 4u, is strictly greater than sqrt(best).  A query
//             that exhausts its shell budget is flagged; the flagged ids are compacted by a scan (ascending ids, no
//             atomic append) with their coordinates gathered, the caller finishes them with geobi_nearest_point /
//             geobi_nearest_triangle and geobi_grid_scatter puts the answers back.  Either way the answer is the all-pairs
//             answer bit for bit.
//
// Every loop of the search has a bound known at launch (shells <= max_rings, rows and cells <= the grid's dimensions,
// entries <= cell_start[cells]); nothing waits on another workgroup.  Every index is bounded: a cell id is clamped into
// the grid before cell_start is read, an entry index is below cell_start[cells] <= the rows of `order`, and what `order`
// holds is clamped into [0, T) before a target row is read.
#include "common.h"
#include "dist_pairs.h"
#include "device_steps.h"
#include "../../include/geobi_hip.h"

#include <math.h>
#include <string.h>

#include <algorithm>

namespace geobi {

namespace {

constexpr int kThreads = 256;
constexpr int kStatBlocks = 256;          // blocks of the two-stage reductions of the plan
// ---- the constants of the grid (DESIGN.md 4u says where each comes from)
constexpr int kMaxAxis = 256;             // cells per axis at most: the cell count stays <= 2^24 and a key in kKeyBits
constexpr unsigned kKeyBits = 25;         // sort key bits: cell ids 0 .. 2^24 (2^24 = the key of a target that is left out)
constexpr double kPerCell = 16.0;         // targets per cell of the longest axis' square: n_long = ceil(sqrt(N / kPerCell))
constexpr float kMinCellFrac = 1.0f / 16384.0f;   // cell edge >= 2^-14 of the largest coordinate magnitude
constexpr int kEntryCap = 8;              // triangles: (cell, face) entries <= kEntryCap * F
constexpr int kMaxRounds = 9;             // 256 -> 1 in eight halvings: nine counts at most
constexpr float kMarginUlps = 32.0f;      // margin = kMarginUlps * 2^-24 * (M + D + dq)
constexpr float kEps = 5.9604644775390625e-8f;    // 2^-24
constexpr int kDefaultRings = 8;          // shells r = 0 .. 7: a block of 15^3 cells before the all-pairs fallback

// the descriptor a plan hands out (HOST int32 [16]; floats by their bits) and every later call takes back
enum Desc { D_NX = 0, D_LO = 3, D_HI = 6, D_CELL = 9, D_MAG = 12, D_ENTRIES = 13, D_ROUNDS = 14, D_FINITE = 15, D_WORDS = 16 };

struct Grid {
  int n[3];
  float lo[3], hi[3], h[3], inv[3];
  float scale;                            // M + D: largest target coordinate magnitude + box diagonal
  int cells;
};

float bits_f(int32_t b) { float f; memcpy(&f, &b, 4); return f; }
int32_t f_bits(float f) { int32_t b; memcpy(&b, &f, 4); return b; }

// descriptor -> Grid; false: not a descriptor a plan made
bool grid_of(const int32_t* d, Grid* g) {
  double diag2 = 0.0;
  int64_t cells = 1;
  for (int a = 0; a < 3; ++a) {
    g->n[a] = d[D_NX + a];
    g->lo[a] = bits_f(d[D_LO + a]); g->hi[a] = bits_f(d[D_HI + a]); g->h[a] = bits_f(d[D_CELL + a]);
    if (g->n[a] < 1 || g->n[a] > kMaxAxis || !(g->h[a] > 0.f) || !(g->lo[a] <= g->hi[a])) return false;
    g->inv[a] = 1.0f / g->h[a];
    const double e = (double)g->hi[a] - (double)g->lo[a];
    diag2 += e * e;
    cells *= g->n[a];
  }
  g->scale = bits_f(d[D_MAG]) + (float)sqrt(diag2);
  g->cells = (int)cells;
  return d[D_ENTRIES] >= 0 && d[D_FINITE] >= 0;
}

// the resolution rule: from the count of finite targets and their box alone.  force > 0: that many cells on every axis
// with extent.  An axis without (finite) extent gets one cell; an edge below kMinCellFrac * mag takes fewer cells.
void grid_resolution(int64_t count, const float* lo, const float* hi, float mag, int force, int* n, float* h) {
  double e[3], emax = 0.0;
  for (int a = 0; a < 3; ++a) {
    e[a] = (double)hi[a] - (double)lo[a];
    if (!(e[a] > 0.0) || !std::isfinite((float)e[a])) e[a] = 0.0;
    emax = std::max(emax, e[a]);
  }
  int n_long = (int)ceil(sqrt((double)std::max<int64_t>(count, 1) / kPerCell));
  n_long = std::min(std::max(force > 0 ? force : n_long, 1), kMaxAxis);
  const double min_edge = (double)kMinCellFrac * (double)mag;
  for (int a = 0; a < 3; ++a) {
    n[a] = 1;
    if (e[a] > 0.0) {
      n[a] = force > 0 ? n_long : (int)ceil(e[a] / (emax / n_long));
      if (e[a] / n[a] < min_edge) n[a] = (int)floor(e[a] / min_edge);
      n[a] = std::min(std::max(n[a], 1), kMaxAxis);
    }
    h[a] = e[a] > 0.0 ? (float)(e[a] / n[a]) : 1.0f;
    if (!(h[a] > 0.f) || !std::isfinite(h[a])) { n[a] = 1; h[a] = 1.0f; }
  }
}
void set_cells(int32_t* d, const int* n, const float* lo, const float* hi) {
  for (int a = 0; a < 3; ++a) {
    const double e = (double)hi[a] - (double)lo[a];
    float h = n[a] > 1 ? (float)(e / n[a]) : (e > 0.0 && std::isfinite((float)e) ? (float)e : 1.0f);
    d[D_NX + a] = n[a];
    d[D_CELL + a] = f_bits(h);
  }
}

// ---------------------------------------------------------------- cells
// the cell of a coordinate on one axis: monotone in x (a difference, a product with a positive number, a floor, a clamp)
__device__ __forceinline__ int axis_cell(const Grid& g, int a, float x) {
#pragma clang fp contract(off)
  if (g.n[a] == 1) return 0;
  const float f = floorf((x - g.lo[a]) * g.inv[a]);
  return (int)fminf(fmaxf(f, 0.f), (float)(g.n[a] - 1));      // a NaN goes to cell 0
}
// the plane between the cells k - 1 and k of an axis
__device__ __forceinline__ float axis_plane(const Grid& g, int a, int k) {
#pragma clang fp contract(off)
  return g.lo[a] + (float)k * g.h[a];
}
__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }
__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// the corners of face f, its ids clamped as triangle_record clamps them -> finite?
__device__ __forceinline__ bool face_box(const float* __restrict__ verts, const int* __restrict__ fv, int V, int f, float* mn,
                                         float* mx) {
  bool fin = true;
  for (int a = 0; a < 3; ++a) { mn[a] = INFINITY; mx[a] = -INFINITY; }
  for (int k = 0; k < 3; ++k) {
    const size_t o = 3 * (size_t)clampi(fv[3 * (size_t)f + k], V);
    for (int a = 0; a < 3; ++a) {
      const float x = verts[o + a];
      fin = fin && isfinite(x);
      mn[a] = fminf(mn[a], x); mx[a] = fmaxf(mx[a], x);
    }
  }
  return fin;
}

// ---------------------------------------------------------------- plan: the box of the finite targets
// what a block knows of its targets: the box, the largest coordinate magnitude and the count of the finite ones; min, max
// and an integer sum do not depend on the order they are joined in
struct Stat { float mn[3], mx[3], mag; int count; };

__device__ __forceinline__ void stat_join(Stat& s, const Stat& o) {
  for (int a = 0; a < 3; ++a) { s.mn[a] = fminf(s.mn[a], o.mn[a]); s.mx[a] = fmaxf(s.mx[a], o.mx[a]); }
  s.mag = fmaxf(s.mag, o.mag);
  s.count += o.count;
}
__device__ __forceinline__ Stat stat_empty() { return {{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}, 0.f, 0}; }

__device__ __forceinline__ Stat stat_block(Stat s) {
  __shared__ Stat sh[kThreads];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int h = kThreads / 2; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) stat_join(sh[threadIdx.x], sh[threadIdx.x + h]);
    __syncthreads();
  }
  return sh[0];
}

template <bool kTri>
__global__ __launch_bounds__(kThreads) void grid_stat_kernel(const float* __restrict__ verts, const int* __restrict__ fv, int V,
                                                            int N, Stat* __restrict__ partial) {
  Stat s = stat_empty();
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < N; i += gridDim.x * kThreads) {
    float mn[3], mx[3];
    bool fin;
    if constexpr (kTri) {
      fin = face_box(verts, fv, V, i, mn, mx);
    } else {
      for (int a = 0; a < 3; ++a) mn[a] = mx[a] = verts[3 * (size_t)i + a];
      fin = finite3(mn[0], mn[1], mn[2]);
    }
    if (fin) {
      Stat o;
      for (int a = 0; a < 3; ++a) { o.mn[a] = mn[a]; o.mx[a] = mx[a]; }
      o.mag = fmaxf(fmaxf(fmaxf(fabsf(mn[0]), fabsf(mx[0])), fmaxf(fabsf(mn[1]), fabsf(mx[1]))), fmaxf(fabsf(mn[2]), fabsf(mx[2])));
      o.count = 1;
      stat_join(s, o);
    }
  }
  s = stat_block(s);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// out [8] int32: min xyz, max xyz, magnitude (float bits), finite count
__global__ __launch_bounds__(kThreads) void grid_stat_final_kernel(const Stat* __restrict__ partial, int blocks, int* __restrict__ out) {
  Stat s = (int)threadIdx.x < blocks ? partial[threadIdx.x] : stat_empty();
  s = stat_block(s);
  if (threadIdx.x == 0) {
    for (int a = 0; a < 3; ++a) { out[a] = __float_as_int(s.mn[a]); out[3 + a] = __float_as_int(s.mx[a]); }
    out[6] = __float_as_int(s.mag);
    out[7] = s.count;
  }
}

// ---------------------------------------------------------------- build
// key of a target: its cell, or g.cells for a target that is left out (sorted behind every cell)
__global__ __launch_bounds__(kThreads) void point_keys_kernel(Grid g, const float* __restrict__ t, int T, int* __restrict__ key,
                                                             int* __restrict__ val, bool leave_out) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= T) return;
  const float x = t[3 * (size_t)i], y = t[3 * (size_t)i + 1], z = t[3 * (size_t)i + 2];
  const bool fin = finite3(x, y, z);
  key[i] = fin ? (axis_cell(g, 2, z) * g.n[1] + axis_cell(g, 1, y)) * g.n[0] + axis_cell(g, 0, x) : (leave_out ? g.cells : 0);
  val[i] = i;
}

// cell_start[c] = the first sorted entry whose key is >= c, c = 0 .. cells: cell_start[cells] = the entries filed
__global__ __launch_bounds__(kThreads) void cell_start_kernel(const int* __restrict__ key, int n, int cells,
                                                             int* __restrict__ cell_start) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c > cells) return;
  int lo = 0, hi = n;                      // at most 32 halvings
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (key[mid] < c) lo = mid + 1; else hi = mid;
  }
  cell_start[c] = lo;
}

struct CellBox { int c0[3], c1[3]; };
__device__ __forceinline__ bool face_cells(const Grid& g, const float* __restrict__ verts, const int* __restrict__ fv, int V, int f,
                                           CellBox* b) {
  float mn[3], mx[3];
  if (!face_box(verts, fv, V, f, mn, mx)) return false;
  for (int a = 0; a < 3; ++a) { b->c0[a] = axis_cell(g, a, mn[a]); b->c1[a] = axis_cell(g, a, mx[a]); }
  return true;
}

// cnt[f] = the cells the box of face f meets (0: a corner that is not finite), cnt[F] = 0
__global__ __launch_bounds__(kThreads) void face_count_kernel(Grid g, const float* __restrict__ verts, const int* __restrict__ fv,
                                                             int V, int F, int* __restrict__ cnt) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  if (f > F) return;
  CellBox b;
  int c = 0;
  if (f < F && face_cells(g, verts, fv, V, f, &b)) c = (b.c1[0] - b.c0[0] + 1) * (b.c1[1] - b.c0[1] + 1) * (b.c1[2] - b.c0[2] + 1);
  cnt[f] = c;                             // <= 2^24
}

// the total of cnt [n] in int64, two stages; out[0] = min(total, INT32_MAX)
__global__ __launch_bounds__(kThreads) void count_sum_kernel(const int* __restrict__ cnt, int n, long long* __restrict__ partial) {
  __shared__ long long sh[kThreads];
  long long s = 0;
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) s += cnt[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int h = kThreads / 2; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}
__global__ void count_sum_final_kernel(const long long* __restrict__ partial, int blocks, int* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  long long s = 0;
  for (int b = 0; b < blocks; ++b) s += partial[b];
  out[0] = (int)(s > (long long)INT32_MAX ? (long long)INT32_MAX : s);
}

// (cell, face) for every cell of the face's box, x fastest: ascending cell id; the faces in ascending order by `off`
__global__ __launch_bounds__(kThreads) void face_emit_kernel(Grid g, const float* __restrict__ verts, const int* __restrict__ fv,
                                                            int V, int F, const int* __restrict__ off, int E,
                                                            int* __restrict__ key, int* __restrict__ val) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= F) return;
  CellBox b;
  if (!face_cells(g, verts, fv, V, f, &b)) return;
  int o = off[f];
  for (int z = b.c0[2]; z <= b.c1[2]; ++z)
    for (int y = b.c0[1]; y <= b.c1[1]; ++y)
      for (int x = b.c0[0]; x <= b.c1[0]; ++x) {
        if (o >= 0 && o < E) { key[o] = (z * g.n[1] + y) * g.n[0] + x; val[o] = f; }
        ++o;
      }
}

__global__ __launch_bounds__(kThreads) void face_records_kernel(const float* __restrict__ verts, const int* __restrict__ fv, int V,
                                                               int F, float4* __restrict__ rec) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= F) return;
  float4 r0, r1, r2, r3;
  triangle_record(verts, fv, V, f, &r0, &r1, &r2, &r3);
  rec[4 * (size_t)f] = r0; rec[4 * (size_t)f + 1] = r1; rec[4 * (size_t)f + 2] = r2; rec[4 * (size_t)f + 3] = r3;
}

// ---------------------------------------------------------------- search
struct PointEntries {
  const float* __restrict__ t;
  __device__ __forceinline__ float d2(float qx, float qy, float qz, int j) const {
    const float* p = t + 3 * (size_t)j;
    return pair_d2(qx, qy, qz, make_float4(p[0], p[1], p[2], 0.f));
  }
};
struct TriangleEntries {
  const float4* __restrict__ rec;
  __device__ __forceinline__ float d2(float qx, float qy, float qz, int j) const {
    const float4* r = rec + 4 * (size_t)j;
    return tri_d2(qx, qy, qz, r[0], r[1], r[2], r[3]);
  }
};

// qorder: the query ids sorted by cell.  T: the rows `order` may name.  flag[i] = 1: query i ran out of shells.
template <class Entries>
__global__ __launch_bounds__(kThreads) void grid_search_kernel(Grid g, Entries en, const float* __restrict__ q,
                                                              const int* __restrict__ qorder, int Q, int T,
                                                              const int* __restrict__ cell_start, const int* __restrict__ order,
                                                              int max_rings, float* __restrict__ dist, int* __restrict__ idx,
                                                              int* __restrict__ flag) {
#pragma clang fp contract(off)
  const int lane = blockIdx.x * kThreads + threadIdx.x;
  if (lane >= Q) return;
  const int i = clampi(qorder[lane], Q);
  if (max_rings <= 0) { flag[i] = 1; return; }
  const float qv[3] = {q[3 * (size_t)i], q[3 * (size_t)i + 1], q[3 * (size_t)i + 2]};
  float best = INFINITY;
  int bidx = 0;
  bool done = true;
  if (finite3(qv[0], qv[1], qv[2])) {
    int c[3], rmax = 0;
    float dq2 = 0.f;
    for (int a = 0; a < 3; ++a) {
      c[a] = axis_cell(g, a, qv[a]);
      rmax = max(rmax, max(c[a], g.n[a] - 1 - c[a]));
      const float d = fmaxf(fmaxf(g.lo[a] - qv[a], qv[a] - g.hi[a]), 0.f);
      dq2 += d * d;
    }
    const float margin = kMarginUlps * kEps * (g.scale + sqrtf(dq2));
    const int entries = cell_start[g.cells];
    const int shells = min(rmax + 1, max_rings);
    done = false;
    for (int r = 0; r < shells && !done; ++r) {
      const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.n[2] - 1), y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.n[1] - 1),
                x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g.n[0] - 1);
      for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y) {
          const int row = (z * g.n[1] + y) * g.n[0];
          const bool whole = abs(z - c[2]) == r || abs(y - c[1]) == r;     // the row lies on the shell from x0 to x1
          // otherwise its two end cells do, where they are inside the grid (r >= 1 here)
          for (int part = 0; part < (whole ? 1 : 2); ++part) {
            int xa = x0, xb = x1;
            if (!whole) {
              xa = xb = part == 0 ? c[0] - r : c[0] + r;
              if (xa < 0 || xa >= g.n[0]) continue;
            }
            const int e0 = max(cell_start[row + xa], 0), e1 = min(cell_start[row + xb + 1], entries);
            for (int e = e0; e < e1; ++e) {
              const int j = clampi(order[e], T);
              const float d2 = en.d2(qv[0], qv[1], qv[2], j);
              const bool lt = d2 < best || (d2 == best && j < bidx);
              best = lt ? d2 : best;
              bidx = lt ? j : bidx;
            }
          }
        }
      // the distance to everything outside the visited block; a side outside the grid bounds nothing
      float b = INFINITY;
      for (int a = 0; a < 3; ++a) {
        if (c[a] - r - 1 >= 0) b = fminf(b, qv[a] - axis_plane(g, a, c[a] - r));
        if (c[a] + r + 1 <= g.n[a] - 1) b = fminf(b, axis_plane(g, a, c[a] + r + 1) - qv[a]);
      }
      done = b == INFINITY || b - margin > sqrtf(best);
    }
  }
  flag[i] = done ? 0 : 1;
  if (done) {
    dist[i] = sqrtf(best);
    if (idx) idx[i] = bidx;
  }
}

// left[rank[i]] = i and left_q[rank[i]] = q[i] for the flagged queries, ascending; count[0] = how many
__global__ __launch_bounds__(kThreads) void compact_left_kernel(const int* __restrict__ flag, const int* __restrict__ rank,
                                                               const float* __restrict__ q, int Q, int* __restrict__ left,
                                                               float* __restrict__ left_q, int* __restrict__ count) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i == 0) count[0] = rank[Q];
  if (i >= Q || flag[i] == 0) return;
  const int k = rank[i];
  if (k < 0 || k >= Q) return;
  left[k] = i;
  for (int a = 0; a < 3; ++a) left_q[3 * (size_t)k + a] = q[3 * (size_t)i + a];
}

__global__ __launch_bounds__(kThreads) void scatter_left_kernel(const int* __restrict__ left, int n, int Q,
                                                               const float* __restrict__ dist_in, const int* __restrict__ idx_in,
                                                               float* __restrict__ dist, int* __restrict__ idx) {
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= n) return;
  const int i = left[k];
  if (i < 0 || i >= Q) return;
  dist[i] = dist_in[k];
  if (idx && idx_in) idx[i] = idx_in[k];
}

// ---------------------------------------------------------------- carves
struct PlanBufs { Stat* partial; long long* sums; int* out; int* cnt; };
PlanBufs carve_plan(Arena& a, int64_t F) {
  return {a.take<Stat>(kStatBlocks), a.take<long long>(kStatBlocks), a.take<int>(16), a.take<int>((size_t)F + 1)};
}
struct SortBufs { int *key_in, *val_in, *key_out; PairSort<int, int> sort; };
SortBufs carve_sort(Arena& a, int64_t n) {
  return {a.take<int>((size_t)n), a.take<int>((size_t)n), a.take<int>((size_t)n),
          PairSort<int, int>::take(a, n, kKeyBits)};
}
struct TriBufs { int *cnt, *off; IntScan scan; SortBufs sort; };
TriBufs carve_tri(Arena& a, int64_t F) {
  return {a.take<int>((size_t)F + 1), a.take<int>((size_t)F + 1), IntScan::take(a, F + 1), carve_sort(a, kEntryCap * F)};
}
struct SearchBufs { SortBufs sort; int *qorder, *flag, *rank; IntScan scan; };
SearchBufs carve_search(Arena& a, int64_t Q) {
  return {carve_sort(a, Q), a.take<int>((size_t)Q), a.take<int>((size_t)Q + 1), a.take<int>((size_t)Q + 1),
          IntScan::take(a, Q + 1)};
}

// one stable sort of n (cell, index) pairs: indices that ascend going in ascend inside every cell coming out
int sort_cells(const SortBufs& b, int64_t n, int* val_out, hipStream_t s) {
  size_t need = 0;
  GEOBI_TRY(b.sort.need(n, &need));
  GEOBI_REQUIRE(need <= b.sort.temp.bytes, "grid: the sort of %lld entries wants %zu bytes of temporary storage, %zu reserved",
                (long long)n, need, b.sort.temp.bytes);
  return b.sort.run(b.key_in, b.key_out, b.val_in, val_out, n, kKeyBits, s);
}

// the box of the finite targets -> the first words of a descriptor, the resolution rule applied; one read-back
template <bool kTri>
int plan_box(const float* verts, const int32_t* fv, int64_t V, int64_t N, int cells, const PlanBufs& b, int32_t* desc,
             hipStream_t s) {
  const int blocks = std::min(kStatBlocks, cdiv(N, kThreads));
  grid_stat_kernel<kTri><<<blocks, kThreads, 0, s>>>(verts, fv, (int)V, (int)N, b.partial);
  grid_stat_final_kernel<<<1, kThreads, 0, s>>>(b.partial, blocks, b.out);
  GEOBI_LAUNCH_OK();
  int32_t host[8];
  GEOBI_TRY(geobi_read_i32(b.out, 8, host, (void*)s));
  for (int k = 0; k < D_WORDS; ++k) desc[k] = 0;
  float lo[3], hi[3], h[3], mag = bits_f(host[6]);
  int n[3];
  const int count = host[7];
  for (int a = 0; a < 3; ++a) { lo[a] = count > 0 ? bits_f(host[a]) : 0.f; hi[a] = count > 0 ? bits_f(host[3 + a]) : 0.f; }
  if (count == 0) mag = 0.f;
  grid_resolution(count, lo, hi, mag, cells, n, h);
  for (int a = 0; a < 3; ++a) {
    desc[D_NX + a] = n[a]; desc[D_LO + a] = f_bits(lo[a]); desc[D_HI + a] = f_bits(hi[a]); desc[D_CELL + a] = f_bits(h[a]);
  }
  desc[D_MAG] = f_bits(mag);
  desc[D_ENTRIES] = count;
  desc[D_ROUNDS] = 0;
  desc[D_FINITE] = count;
  return 0;
}

int check_cells(const char* fn, int cells) {
  GEOBI_REQUIRE(cells >= 0 && cells <= kMaxAxis, "%s: cells = %d (0: the library's rule; 1 .. %d cells per axis)", fn, cells, kMaxAxis);
  return 0;
}

template <class Entries>
int search(const char* fn, const Entries& en, const float* q, int64_t Q, int64_t T, const int32_t* desc, const int32_t* cell_start,
           const int32_t* order, int max_rings, float* dist, int32_t* idx, int32_t* left, float* left_q, int32_t* count, void* ws,
           size_t ws_bytes, hipStream_t s) {
  Grid g;
  GEOBI_REQUIRE(grid_of(desc, &g), "%s: desc is not the descriptor of a grid plan", fn);
  GEOBI_REQUIRE(max_rings >= -1, "%s: max_rings = %d (-1: the default of %d shells; 0: every query is left over)", fn, max_rings,
                kDefaultRings);
  SearchBufs b;
  GEOBI_TRY(carve_checked(fn, ws, ws_bytes, b, [&](Arena& a) { return carve_search(a, Q); }));
  const int blocks = cdiv(Q, kThreads);
  // the queries by cell (one that is not finite: cell 0), so that the lanes of a wave walk the same cells
  point_keys_kernel<<<blocks, kThreads, 0, s>>>(g, q, (int)Q, b.sort.key_in, b.sort.val_in, false);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(sort_cells(b.sort, Q, b.qorder, s));
  GEOBI_HIP(hipMemsetAsync(b.flag, 0, ((size_t)Q + 1) * sizeof(int), s));
  grid_search_kernel<Entries><<<blocks, kThreads, 0, s>>>(g, en, q, b.qorder, (int)Q, (int)T, cell_start, order,
                                                          max_rings < 0 ? kDefaultRings : max_rings, dist, idx, b.flag);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(b.scan.run(b.flag, b.rank, s));
  compact_left_kernel<<<blocks, kThreads, 0, s>>>(b.flag, b.rank, q, (int)Q, left, left_q, count);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // namespace

}  // namespace geobi

using namespace geobi;

extern "C" {

int geobi_grid_default_rings(void) { return kDefaultRings; }
int geobi_grid_max_cells(void) { return kMaxAxis; }
int geobi_grid_entry_cap(void) { return kEntryCap; }

size_t geobi_grid_plan_ws_bytes(int64_t F) {
  return carve_bytes([&](Arena& a) { carve_plan(a, F < 0 ? 0 : F); });
}

int geobi_grid_points_plan(const float* t, int64_t T, int cells, int32_t* desc, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(T, 0);
  GEOBI_NOTNULL(t); GEOBI_NOTNULL(desc); GEOBI_NOTNULL(ws);
  GEOBI_REQUIRE(T > 0, "grid_points_plan: empty query or target set (Q = %lld, T = %lld)", 0LL, (long long)T);
  GEOBI_TRY(check_cells(__func__, cells));
  PlanBufs b;
  GEOBI_TRY(carve_checked("grid_points_plan", ws, ws_bytes, b, [&](Arena& a) { return carve_plan(a, 0); }));
  return plan_box<false>(t, nullptr, 0, T, cells, b, desc, as_stream(stream));
}

size_t geobi_grid_points_build_ws_bytes(int64_t T) {
  if (T <= 0) return 0;
  return carve_bytes([&](Arena& a) { carve_sort(a, T); });
}

int geobi_grid_points_build(const float* t, int64_t T, const int32_t* desc, int32_t* cell_start, int32_t* order, void* ws,
                            size_t ws_bytes, void* stream) {
  GEOBI_SIZES(T, 0);
  GEOBI_NOTNULL(t); GEOBI_NOTNULL(desc); GEOBI_NOTNULL(cell_start); GEOBI_NOTNULL(order); GEOBI_NOTNULL(ws);
  GEOBI_REQUIRE(T > 0, "grid_points_build: empty query or target set (Q = %lld, T = %lld)", 0LL, (long long)T);
  Grid g;
  GEOBI_REQUIRE(grid_of(desc, &g), "%s: desc is not the descriptor of a grid plan", __func__);
  hipStream_t s = as_stream(stream);
  SortBufs b;
  GEOBI_TRY(carve_checked("grid_points_build", ws, ws_bytes, b, [&](Arena& a) { return carve_sort(a, T); }));
  point_keys_kernel<<<cdiv(T, kThreads), kThreads, 0, s>>>(g, t, (int)T, b.key_in, b.val_in, true);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(sort_cells(b, T, order, s));
  cell_start_kernel<<<cdiv(g.cells + 1, kThreads), kThreads, 0, s>>>(b.key_out, (int)T, g.cells, cell_start);
  GEOBI_LAUNCH_OK();
  return 0;
}

int geobi_grid_triangles_plan(const float* verts, const int32_t* fv, int64_t V, int64_t F, int cells, int32_t* desc, void* ws,
                              size_t ws_bytes, void* stream) {
  GEOBI_MESH_SIZES(F, V);
  GEOBI_NOTNULL(verts); GEOBI_NOTNULL(fv); GEOBI_NOTNULL(desc); GEOBI_NOTNULL(ws);
  GEOBI_REQUIRE(V > 0 && F > 0, "grid_triangles_plan: empty query set or mesh (Q = %lld, V = %lld, F = %lld)", 0LL, (long long)V,
                (long long)F);
  GEOBI_TRY(check_cells(__func__, cells));
  hipStream_t s = as_stream(stream);
  PlanBufs b;
  GEOBI_TRY(carve_checked("grid_triangles_plan", ws, ws_bytes, b, [&](Arena& a) { return carve_plan(a, F); }));
  GEOBI_TRY(plan_box<true>(verts, fv, V, F, cells, b, desc, s));
  float lo[3], hi[3];
  int n[3];
  for (int a = 0; a < 3; ++a) { lo[a] = bits_f(desc[D_LO + a]); hi[a] = bits_f(desc[D_HI + a]); n[a] = desc[D_NX + a]; }
  const int blocks = std::min(kStatBlocks, cdiv(F + 1, kThreads));
  for (int round = 1; round <= kMaxRounds; ++round) {
    Grid g;
    GEOBI_REQUIRE(grid_of(desc, &g), "%s: the plan made no grid", __func__);
    face_count_kernel<<<cdiv(F + 1, kThreads), kThreads, 0, s>>>(g, verts, fv, (int)V, (int)F, b.cnt);
    count_sum_kernel<<<blocks, kThreads, 0, s>>>(b.cnt, (int)F + 1, b.sums);
    count_sum_final_kernel<<<1, 64, 0, s>>>(b.sums, blocks, b.out);
    GEOBI_LAUNCH_OK();
    int32_t total;
    GEOBI_TRY(geobi_read_i32(b.out, 1, &total, (void*)s));
    desc[D_ENTRIES] = total;
    desc[D_ROUNDS] = round;
    if ((int64_t)total <= (int64_t)kEntryCap * F) return 0;
    GEOBI_REQUIRE(n[0] > 1 || n[1] > 1 || n[2] > 1, "%s: %d entries in one cell for %lld faces", __func__, total, (long long)F);
    for (int a = 0; a < 3; ++a) n[a] = std::max(1, n[a] / 2);
    set_cells(desc, n, lo, hi);
  }
  return set_error("%s: the entries still exceed %d * F after %d rounds", __func__, kEntryCap, kMaxRounds);
}

size_t geobi_grid_triangles_build_ws_bytes(int64_t F) {
  if (F <= 0) return 0;
  return carve_bytes([&](Arena& a) { carve_tri(a, F); });
}

int geobi_grid_triangles_build(const float* verts, const int32_t* fv, int64_t V, int64_t F, const int32_t* desc,
                               int32_t* cell_start, int32_t* order, float* records, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_MESH_SIZES(F, V);
  GEOBI_NOTNULL(verts); GEOBI_NOTNULL(fv); GEOBI_NOTNULL(desc); GEOBI_NOTNULL(cell_start); GEOBI_NOTNULL(order);
  GEOBI_NOTNULL(records); GEOBI_NOTNULL(ws);
  GEOBI_REQUIRE(V > 0 && F > 0, "grid_triangles_build: empty query set or mesh (Q = %lld, V = %lld, F = %lld)", 0LL, (long long)V,
                (long long)F);
  Grid g;
  GEOBI_REQUIRE(grid_of(desc, &g), "%s: desc is not the descriptor of a grid plan", __func__);
  const int64_t E = desc[D_ENTRIES];
  GEOBI_REQUIRE(E <= (int64_t)kEntryCap * F, "%s: desc holds %lld entries for %lld faces (at most %d * F)", __func__, (long long)E,
                (long long)F, kEntryCap);
  hipStream_t s = as_stream(stream);
  TriBufs b;
  GEOBI_TRY(carve_checked("grid_triangles_build", ws, ws_bytes, b, [&](Arena& a) { return carve_tri(a, F); }));
  face_records_kernel<<<cdiv(F, kThreads), kThreads, 0, s>>>(verts, fv, (int)V, (int)F, (float4*)records);
  face_count_kernel<<<cdiv(F + 1, kThreads), kThreads, 0, s>>>(g, verts, fv, (int)V, (int)F, b.cnt);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(b.scan.run(b.cnt, b.off, s));
  if (E > 0) {
    face_emit_kernel<<<cdiv(F, kThreads), kThreads, 0, s>>>(g, verts, fv, (int)V, (int)F, b.off, (int)E, b.sort.key_in, b.sort.val_in);
    GEOBI_LAUNCH_OK();
    GEOBI_TRY(sort_cells(b.sort, E, order, s));
  }
  cell_start_kernel<<<cdiv(g.cells + 1, kThreads), kThreads, 0, s>>>(b.sort.key_out, (int)E, g.cells, cell_start);
  GEOBI_LAUNCH_OK();
  return 0;
}

size_t geobi_grid_nearest_ws_bytes(int64_t Q) {
  if (Q <= 0) return 0;
  return carve_bytes([&](Arena& a) { carve_search(a, Q); });
}

int geobi_grid_nearest_point(const float* q, const float* t, int64_t Q, int64_t T, const int32_t* desc, const int32_t* cell_start,
                             const int32_t* order, int max_rings, float* dist, int32_t* idx, int32_t* left, float* left_q,
                             int32_t* count, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(Q > T ? Q : T, 0);
  GEOBI_NOTNULL(q); GEOBI_NOTNULL(t); GEOBI_NOTNULL(desc); GEOBI_NOTNULL(cell_start); GEOBI_NOTNULL(order); GEOBI_NOTNULL(dist);
  GEOBI_NOTNULL(left); GEOBI_NOTNULL(left_q); GEOBI_NOTNULL(count); GEOBI_NOTNULL(ws);
  GEOBI_REQUIRE(Q > 0 && T > 0, "grid_nearest_point: empty query or target set (Q = %lld, T = %lld)", (long long)Q, (long long)T);
  return search("grid_nearest_point", PointEntries{t}, q, Q, T, desc, cell_start, order, max_rings, dist, idx, left, left_q, count,
                ws, ws_bytes, as_stream(stream));
}

int geobi_grid_nearest_triangle(const float* q, const float* records, int64_t Q, int64_t F, const int32_t* desc,
                                const int32_t* cell_start, const int32_t* order, int max_rings, float* dist, int32_t* face,
                                int32_t* left, float* left_q, int32_t* count, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(Q > F ? Q : F, 0);
  GEOBI_NOTNULL(q); GEOBI_NOTNULL(records); GEOBI_NOTNULL(desc); GEOBI_NOTNULL(cell_start); GEOBI_NOTNULL(order);
  GEOBI_NOTNULL(dist); GEOBI_NOTNULL(left); GEOBI_NOTNULL(left_q); GEOBI_NOTNULL(count); GEOBI_NOTNULL(ws);
  GEOBI_REQUIRE(Q > 0 && F > 0, "grid_nearest_triangle: empty query set or mesh (Q = %lld, V = %lld, F = %lld)", (long long)Q, 1LL,
                (long long)F);
  return search("grid_nearest_triangle", TriangleEntries{(const float4*)records}, q, Q, F, desc, cell_start, order, max_rings, dist,
                face, left, left_q, count, ws, ws_bytes, as_stream(stream));
}

int geobi_grid_scatter(const int32_t* left, int64_t n, int64_t Q, const float* dist_in, const int32_t* idx_in, float* dist,
                       int32_t* idx, void* stream) {
  GEOBI_SIZES(Q, 0);
  GEOBI_NOTNULL(left); GEOBI_NOTNULL(dist_in); GEOBI_NOTNULL(dist);
  GEOBI_REQUIRE(n >= 1 && n <= Q, "%s: n = %lld left-over queries of Q = %lld", __func__, (long long)n, (long long)Q);
  scatter_left_kernel<<<cdiv(n, kThreads), kThreads, 0, as_stream(stream)>>>(left, (int)n, (int)Q, dist_in, idx_in, dist, idx);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // extern "C"
