// Self-intersections of one mesh: every pair of faces whose triangles meet anywhere other than
// where their shared vertex ids force them to.  The reference has no counterpart (it never asks); the rules are stated in
// include/geobi_hip.h (geobi_self_intersections) and restated in tests/selfx_model.py, once in numpy in the same order
// of operations (every output is compared exactly) and once as the point-set definition in exact arithmetic.
//
// The all-pairs walk of dist.hip: a lane owns kQpl query faces in registers (float32 box, ids, corners); the workgroup
// stages a tile of target records in LDS (five float4 per face, the corners gathered once per tile); every lane reads the
// SAME record (LDS broadcast).  The inner loop is the closed box test on two float4; only a pair whose boxes overlap reads
// the rest of the record, counts the shared ids and runs the fp64 test (pair_hit, inline: candidates are rare, and a
// compacted list would need a buffer whose size F and V do not give; DESIGN.md 4t has the register report).  Targets are
// cut into slices by THE slicing rule (pair_slices.h).  The predicates are __host__ __device__ so that a host program can
// run them under a sanitizer.
//
// Determinism: a pair is evaluated as (lower face, higher face) whichever of the two is the query, so hits is symmetric
// by construction.  The pair list needs no sort: the counting walk writes per (face, slice) the number of partners
// b > a, one exclusive scan over (face-major, slice-minor) gives the first row of each, and a second, identical walk
// writes the partners, which it meets in ascending order.  The totals are integer atomics on buffers no kernel reads in
// the same launch (hits, counts); integer sums do not depend on their order.  No float atomics.
//
// Bounds: a face row is read only for f < F; its ids are tested against [0, V) in selfx_prep_kernel before any vertex
// is read (a face that fails is not included and its corners are never gathered); a tile index j stays below the staged
// n <= kTile; a pair row is written only below max_pairs; cnt / offs are indexed f * S + slice with f < F, slice < S.
#include "common.h"
#include "pair_slices.h"
#include "device_steps.h"
#include "../../include/geobi_hip.h"

#include <math.h>

#pragma clang fp contract(off)

namespace geobi {

namespace {

constexpr int kThreads = kWalkThreads;
constexpr int kQpl = 2, kTile = 256;                // 20 KB of LDS: five float4 per face
static_assert(kTile == kThreads, "one thread stages one face of the tile");
enum Count { kPairs = 0, kPairsK0 = 1, kPairsK1 = 2, kPairsK2 = 3, kFacesHit = 4, kDegenerateFaces = 5, kIncluded = 6,
             kBoxCandidates = 7, kCounts = 8 };

struct D3 { double x, y, z; };
struct D2 { double u, v; };
struct Face { int id0, id1, id2; float c[9]; };     // the ids and the corners a, b, c of one face

__host__ __device__ __forceinline__ D3 sub(const D3& u, const D3& w) {
#pragma clang fp contract(off)
  return {u.x - w.x, u.y - w.y, u.z - w.z};
}
__host__ __device__ __forceinline__ D3 cross(const D3& u, const D3& w) {
#pragma clang fp contract(off)
  return {u.y * w.z - u.z * w.y, u.z * w.x - u.x * w.z, u.x * w.y - u.y * w.x};
}
__host__ __device__ __forceinline__ double dot(const D3& u, const D3& w) {
#pragma clang fp contract(off)
  return (u.x * w.x + u.y * w.y) + u.z * w.z;
}
__host__ __device__ __forceinline__ D3 corner(const float* c, int k) { return {(double)c[3 * k], (double)c[3 * k + 1], (double)c[3 * k + 2]}; }
// corner i of (c0, c1, c2) without indexing registers by a run-time value
__host__ __device__ __forceinline__ D3 pick(const D3& c0, const D3& c1, const D3& c2, int i) { return i == 0 ? c0 : (i == 1 ? c1 : c2); }
__host__ __device__ __forceinline__ bool same_side(double a, double b) { return (a > 0.0 && b > 0.0) || (a < 0.0 && b < 0.0); }
__host__ __device__ __forceinline__ bool one_side(double a, double b, double c) {
  return (a > 0.0 && b > 0.0 && c > 0.0) || (a < 0.0 && b < 0.0 && c < 0.0);
}
__host__ __device__ __forceinline__ bool no_sign_change(double a, double b, double c) {
  return (a >= 0.0 && b >= 0.0 && c >= 0.0) || (a <= 0.0 && b <= 0.0 && c <= 0.0);
}

__host__ __device__ __forceinline__ int axis_of(const D3& n) {
  int ax = 0;
  double m = fabs(n.x);
  if (fabs(n.y) > m) { ax = 1; m = fabs(n.y); }
  if (fabs(n.z) > m) ax = 2;
  return ax;
}
__host__ __device__ __forceinline__ D2 flat(const D3& p, int ax) {
  return {ax == 0 ? p.y : p.x, ax == 2 ? p.y : p.z};
}
__host__ __device__ __forceinline__ double o2(const D2& a, const D2& b, const D2& c) {
#pragma clang fp contract(off)
  return (b.u - a.u) * (c.v - a.v) - (b.v - a.v) * (c.u - a.u);
}

// closed segments pq and cd of one plane
__host__ __device__ __forceinline__ bool seg_seg(const D2& p, const D2& q, const D2& c, const D2& d) {
  const double o1 = o2(p, q, c), o2b = o2(p, q, d), o3 = o2(c, d, p), o4 = o2(c, d, q);
  if (o1 == 0.0 && o2b == 0.0 && o3 == 0.0 && o4 == 0.0)
    return fmax(fmin(p.u, q.u), fmin(c.u, d.u)) <= fmin(fmax(p.u, q.u), fmax(c.u, d.u)) &&
           fmax(fmin(p.v, q.v), fmin(c.v, d.v)) <= fmin(fmax(p.v, q.v), fmax(c.v, d.v));
  return !same_side(o1, o2b) && !same_side(o3, o4);
}

// the closed segment pq meets the closed triangle (t0, t1, t2) with the normal n; dp, dq: side of p and of q
__host__ __device__ __forceinline__ bool seg_tri(const D3& p, const D3& q, const D3& t0, const D3& t1, const D3& t2, const D3& n, double dp,
                                        double dq) {
#pragma clang fp contract(off)
  if (same_side(dp, dq)) return false;
  if (dp == 0.0 && dq == 0.0) {
    const int ax = axis_of(n);
    const D2 p2 = flat(p, ax), q2 = flat(q, ax), a = flat(t0, ax), b = flat(t1, ax), c = flat(t2, ax);
    if (no_sign_change(o2(a, b, p2), o2(b, c, p2), o2(c, a, p2))) return true;
    return seg_seg(p2, q2, a, b) || seg_seg(p2, q2, b, c) || seg_seg(p2, q2, c, a);
  }
  const D3 d = sub(q, p), u0 = sub(t0, p), u1 = sub(t1, p), u2 = sub(t2, p);
  return no_sign_change(dot(d, cross(u0, u1)), dot(d, cross(u1, u2)), dot(d, cross(u2, u0)));
}

// The pair (A, B), A the LOWER face.  -> k (0 .. 3), *hit: the rule of the header for that k.  The edge tests of k = 0
// and k = 1 are ONE loop over (half, edge) around one copy of seg_tri -- an `or` of pure tests, whose order decides
// nothing -- so that the walk carries the code and the registers of one segment test, not of eight.
__host__ __device__ __forceinline__ int pair_hit(const Face& A, const Face& B, bool* hit) {
#pragma clang fp contract(off)
  *hit = false;
  const bool m00 = A.id0 == B.id0, m01 = A.id0 == B.id1, m02 = A.id0 == B.id2;
  const bool m10 = A.id1 == B.id0, m11 = A.id1 == B.id1, m12 = A.id1 == B.id2;
  const bool m20 = A.id2 == B.id0, m21 = A.id2 == B.id1, m22 = A.id2 == B.id2;
  const bool sa0 = m00 || m01 || m02, sa1 = m10 || m11 || m12, sa2 = m20 || m21 || m22;      // A's corner is shared
  const bool sb0 = m00 || m10 || m20, sb1 = m01 || m11 || m21;                               // B's corner is shared
  const int k = (int)sa0 + (int)sa1 + (int)sa2;
  if (k == 3) return 3;
  const D3 a0 = corner(A.c, 0), a1 = corner(A.c, 1), a2 = corner(A.c, 2);
  const D3 b0 = corner(B.c, 0), b1 = corner(B.c, 1), b2 = corner(B.c, 2);
  const D3 nA = cross(sub(a1, a0), sub(a2, a0));
  if (k == 2) {
    const int ia = sa0 ? (sa1 ? 2 : 1) : 0, ib = sb0 ? (sb1 ? 2 : 1) : 0;                     // the corners off the edge
    const D3 pa = pick(a0, a1, a2, ia), u = pick(a1, a2, a0, ia), v = pick(a2, a0, a1, ia), pb = pick(b0, b1, b2, ib);
    if (dot(nA, sub(pb, a0)) != 0.0) return 2;
    const int ax = axis_of(nA);
    const D2 u2 = flat(u, ax), v2 = flat(v, ax);
    *hit = same_side(o2(u2, v2, flat(pa, ax)), o2(u2, v2, flat(pb, ax)));
    return 2;
  }
  const D3 nB = cross(sub(b1, b0), sub(b2, b0));
  const double db0 = dot(nA, sub(b0, a0)), db1 = dot(nA, sub(b1, a0)), db2 = dot(nA, sub(b2, a0));
  const double da0 = dot(nB, sub(a0, b0)), da1 = dot(nB, sub(a1, b0)), da2 = dot(nB, sub(a2, b0));
  if (k == 0 && (one_side(db0, db1, db2) || one_side(da0, da1, da2))) return 0;
  // k == 1: only the edge opposite the shared corner, which starts at the corner after it
  const int only_a = sa0 ? 1 : (sa1 ? 2 : 0), only_b = sb0 ? 1 : (sb1 ? 2 : 0);
  bool any = false;
#pragma nounroll
  for (int half = 0; half < 2 && !any; ++half) {         // 0: the edges of B against A; 1: the edges of A against B
    const bool h = half == 0;
    const D3 x0 = h ? b0 : a0, x1 = h ? b1 : a1, x2 = h ? b2 : a2, t0 = h ? a0 : b0, t1 = h ? a1 : b1, t2 = h ? a2 : b2;
    const D3 n = h ? nA : nB;
    const double d0 = h ? db0 : da0, d1 = h ? db1 : da1, d2 = h ? db2 : da2;
    const int only = h ? only_b : only_a;
#pragma nounroll
    for (int e = 0; e < 3 && !any; ++e) {                // the edge from corner e to corner e + 1
      if (k == 1 && e != only) continue;
      any = seg_tri(pick(x0, x1, x2, e), pick(x1, x2, x0, e), t0, t1, t2, n, e == 0 ? d0 : (e == 1 ? d1 : d2),
                    e == 0 ? d1 : (e == 1 ? d2 : d0));
    }
  }
  *hit = any;
  return k;
}

// one atomic per wave for a per-lane count; every lane of the wave calls it
__device__ __forceinline__ void add_lanes(int mine, unsigned long long* __restrict__ counter) {
  for (int o = 32; o >= 1; o >>= 1) mine += __shfl_xor(mine, o);
  if ((threadIdx.x & 63) == 0 && mine != 0) atomicAdd(counter, (unsigned long long)mine);
}

// incl[f] = 1 for an included face; counts the degenerate and the included ones
__global__ __launch_bounds__(kThreads) void selfx_prep_kernel(const float* __restrict__ verts, const int* __restrict__ fv,
                                                              const int* __restrict__ state, int V, int F,
                                                              int* __restrict__ incl, unsigned long long* __restrict__ counts) {
#pragma clang fp contract(off)
  const int f = blockIdx.x * kThreads + threadIdx.x;
  int in = 0, deg = 0;
  if (f < F && (state == nullptr || state[f] == 1)) {
    const int ia = fv[3 * (size_t)f], ib = fv[3 * (size_t)f + 1], ic = fv[3 * (size_t)f + 2];
    bool ok = (unsigned)ia < (unsigned)V && (unsigned)ib < (unsigned)V && (unsigned)ic < (unsigned)V && ia != ib && ib != ic &&
              ic != ia;
    if (ok) {
      const D3 a = corner(verts + 3 * (size_t)ia, 0), b = corner(verts + 3 * (size_t)ib, 0), c = corner(verts + 3 * (size_t)ic, 0);
      const D3 n = cross(sub(b, a), sub(c, a));
      ok = !(n.x == 0.0 && n.y == 0.0 && n.z == 0.0);
    }
    in = ok ? 1 : 0;
    deg = 1 - in;
  }
  if (f < F) incl[f] = in;
  add_lanes(deg, counts + kDegenerateFaces);
  add_lanes(in, counts + kIncluded);
}

// The record of face f: box (lo, hi), ids, corners.  A face that is not included (or f >= F) gets the EMPTY box
// lo = +inf, hi = -inf, which overlaps nothing, and its vertices are not read.
__device__ __forceinline__ void load_face(const float* __restrict__ verts, const int* __restrict__ fv,
                                          const int* __restrict__ incl, int F, int f, float* lo, float* hi, Face* face) {
  face->id0 = -1; face->id1 = -2; face->id2 = -3;
#pragma unroll
  for (int k = 0; k < 9; ++k) face->c[k] = 0.f;
  lo[0] = lo[1] = lo[2] = INFINITY;
  hi[0] = hi[1] = hi[2] = -INFINITY;
  if (f >= F || !incl[f]) return;
  face->id0 = fv[3 * (size_t)f]; face->id1 = fv[3 * (size_t)f + 1]; face->id2 = fv[3 * (size_t)f + 2];   // in [0, V): prep
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    face->c[k] = verts[3 * (size_t)face->id0 + k];
    face->c[3 + k] = verts[3 * (size_t)face->id1 + k];
    face->c[6 + k] = verts[3 * (size_t)face->id2 + k];
    lo[k] = fminf(face->c[k], fminf(face->c[3 + k], face->c[6 + k]));
    hi[k] = fmaxf(face->c[k], fmaxf(face->c[3 + k], face->c[6 + k]));
  }
}

struct Tile { float4 r[5][kTile]; };   // r0 = (lo, hi.x)  r1 = (hi.y, hi.z, id0, id1)  r2 = (id2, a)  r3 = (b, c.x)  r4 = (c.y, c.z, -, -)

// kWrite == false: the counting walk (hits, cnt, the class counts); true: the same walk writes the partners b > a of
// every query a from row offs[a * S + slice] on, below max_pairs.
template <bool kWrite>
__global__ __launch_bounds__(kThreads) void selfx_walk_kernel(const float* __restrict__ verts, const int* __restrict__ fv,
                                                              const int* __restrict__ incl, int F, int tiles_per_slice,
                                                              int* __restrict__ hits, long long* __restrict__ cnt,
                                                              const long long* __restrict__ offs, int* __restrict__ pairs,
                                                              long long max_pairs, unsigned long long* __restrict__ counts) {
  __shared__ Tile tile;
  const int tid = threadIdx.x, slice = blockIdx.y, S = gridDim.y;
  const int q0 = blockIdx.x * (kThreads * kQpl);
  const int t_begin = slice * tiles_per_slice * kTile;                   // < F: no slice is empty
  const int t_end = min(F, t_begin + tiles_per_slice * kTile);
  float qlo[kQpl][3], qhi[kQpl][3];
  Face qf[kQpl];
  int nhit[kQpl], ngt[kQpl];
  int nk0 = 0, nk1 = 0, nk2 = 0, ncand = 0;
#pragma unroll
  for (int k = 0; k < kQpl; ++k) {
    load_face(verts, fv, incl, F, q0 + k * kThreads + tid, qlo[k], qhi[k], &qf[k]);
    nhit[k] = ngt[k] = 0;
  }
  for (int t0 = t_begin; t0 < t_end; t0 += kTile) {
    const int n = min(kTile, t_end - t0);
    __syncthreads();
    if (tid < n) {
      float lo[3], hi[3];
      Face tf;
      load_face(verts, fv, incl, F, t0 + tid, lo, hi, &tf);
      tile.r[0][tid] = make_float4(lo[0], lo[1], lo[2], hi[0]);
      tile.r[1][tid] = make_float4(hi[1], hi[2], __int_as_float(tf.id0), __int_as_float(tf.id1));
      tile.r[2][tid] = make_float4(__int_as_float(tf.id2), tf.c[0], tf.c[1], tf.c[2]);
      tile.r[3][tid] = make_float4(tf.c[3], tf.c[4], tf.c[5], tf.c[6]);
      tile.r[4][tid] = make_float4(tf.c[7], tf.c[8], 0.f, 0.f);
    }
    __syncthreads();
    for (int j = 0; j < n; ++j) {
      const float4 b0 = tile.r[0][j], b1 = tile.r[1][j];
#pragma unroll
      for (int k = 0; k < kQpl; ++k) {
        const bool overlap = qlo[k][0] <= b0.w && b0.x <= qhi[k][0] && qlo[k][1] <= b1.x && b0.y <= qhi[k][1] &&
                             qlo[k][2] <= b1.y && b0.z <= qhi[k][2];
        if (!overlap) continue;
        const float4 r2 = tile.r[2][j], r3 = tile.r[3][j], r4 = tile.r[4][j];
        const Face tf = {__float_as_int(b1.z), __float_as_int(b1.w), __float_as_int(r2.x),
                         {r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w, r4.x, r4.y}};
        const int q = q0 + k * kThreads + tid, t = t0 + j;
        const bool up = t > q;                                            // the target is the higher face
        bool hit;
        const int shared = pair_hit(up ? qf[k] : tf, up ? tf : qf[k], &hit);
        if (shared == 3) continue;                                        // the face itself, or a duplicate of it
        if (kWrite) {
          if (up && hit) {
            const long long row = offs[(size_t)q * S + slice] + ngt[k];
            if (row < max_pairs) { pairs[2 * row] = q; pairs[2 * row + 1] = t; }
            ++ngt[k];
          }
        } else {
          nhit[k] += hit;
          if (up) {
            ++ncand;
            ngt[k] += hit;
            nk0 += hit && shared == 0; nk1 += hit && shared == 1; nk2 += hit && shared == 2;
          }
        }
      }
    }
  }
  if (kWrite) return;
#pragma unroll
  for (int k = 0; k < kQpl; ++k) {
    const int q = q0 + k * kThreads + tid;
    if (q < F) {
      cnt[(size_t)q * S + slice] = ngt[k];
      if (nhit[k] != 0) atomicAdd(hits + q, nhit[k]);
    }
  }
  add_lanes(nk0, counts + kPairsK0);
  add_lanes(nk1, counts + kPairsK1);
  add_lanes(nk2, counts + kPairsK2);
  add_lanes(ncand, counts + kBoxCandidates);
}

// faces with hits > 0, and the total: the end of the scanned (face, slice) counts
__global__ __launch_bounds__(kThreads) void selfx_totals_kernel(const int* __restrict__ hits, int F, const long long* __restrict__ cnt,
                                                                const long long* __restrict__ offs, long long n,
                                                                unsigned long long* __restrict__ counts) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  add_lanes(f < F && hits[f] > 0 ? 1 : 0, counts + kFacesHit);
  if (f == 0) counts[kPairs] = (unsigned long long)(offs[n - 1] + cnt[n - 1]);
}

struct SelfxBuffers {
  int* incl;
  long long *cnt, *offs;        // [F * S], face-major and slice-minor
  ExclusiveScan<long long> scan;
};
SelfxBuffers carve_selfx(Arena& a, int64_t F, int slices) {
  const size_t n = (size_t)F * slices;
  return {a.take<int>(F), a.take<long long>(n), a.take<long long>(n), ExclusiveScan<long long>::take(a, n)};
}

Slicing selfx_slices(int64_t F) { return choose_slices(F, F, kQpl, kTile); }

}  // namespace

}  // namespace geobi

using namespace geobi;

extern "C" {

int geobi_self_intersections_slices(int64_t F) { return F <= 0 || F > GEOBI_MAX_NODES ? 0 : selfx_slices(F).slices; }

size_t geobi_self_intersections_ws_bytes(int64_t F, int64_t V) {
  if (F < 0 || V < 0 || F > GEOBI_MAX_NODES || V > GEOBI_MAX_NODES) return 0;
  if (F == 0) return kWsSlack;
  return carve_bytes([&](Arena& a) { carve_selfx(a, F, selfx_slices(F).slices); });
}

// The counterpart of nothing in the reference: it denoises and scores meshes and never asks whether a surface passes
// through itself.
int geobi_self_intersections(const float* verts, const int32_t* faces, const int32_t* state, int64_t V, int64_t F,
                             int32_t* hits, int32_t* pairs, int64_t max_pairs, void* counts, void* ws, size_t ws_bytes,
                             void* stream) {
  GEOBI_MESH_SIZES(F, V);
  GEOBI_NOTNULL(counts);
  GEOBI_REQUIRE(max_pairs >= 0 && max_pairs <= INT32_MAX, "%s: max_pairs = %lld (0 .. 2^31 - 1 rows)", __func__, (long long)max_pairs);
  GEOBI_REQUIRE(max_pairs == 0 || pairs != nullptr, "%s: pairs is NULL with max_pairs = %lld", __func__, (long long)max_pairs);
  hipStream_t s = as_stream(stream);
  unsigned long long* c = (unsigned long long*)counts;
  GEOBI_HIP(hipMemsetAsync(c, 0, sizeof(unsigned long long) * kCounts, s));
  if (F == 0) return 0;
  GEOBI_NOTNULL(verts); GEOBI_NOTNULL(faces); GEOBI_NOTNULL(hits);
  const Slicing sl = selfx_slices(F);
  SelfxBuffers b;
  GEOBI_TRY(carve_checked("self_intersections", ws, ws_bytes, b, [&](Arena& a) { return carve_selfx(a, F, sl.slices); }));
  const int n = (int)F, blocks = cdiv(F, kThreads);
  const long long cells = (long long)F * sl.slices;
  const dim3 grid(sl.qblocks, sl.slices);
  GEOBI_HIP(hipMemsetAsync(hits, 0, sizeof(int32_t) * (size_t)F, s));
  selfx_prep_kernel<<<blocks, kThreads, 0, s>>>(verts, faces, state, (int)V, n, b.incl, c);
  GEOBI_LAUNCH_OK();
  selfx_walk_kernel<false><<<grid, kThreads, 0, s>>>(verts, faces, b.incl, n, sl.tiles_per_slice, hits, b.cnt, nullptr, nullptr, 0, c);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(b.scan.run(b.cnt, b.offs, s));
  if (max_pairs > 0) {
    selfx_walk_kernel<true><<<grid, kThreads, 0, s>>>(verts, faces, b.incl, n, sl.tiles_per_slice, nullptr, nullptr, b.offs, pairs,
                                                      (long long)max_pairs, nullptr);
    GEOBI_LAUNCH_OK();
  }
  selfx_totals_kernel<<<blocks, kThreads, 0, s>>>(hits, n, b.cnt, b.offs, cells, c);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // extern "C"
