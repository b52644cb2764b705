// Generalised winding numbers of query points against one mesh (Jacobson et al. 2013), and the two
// helpers that turn them into an outward orientation: per-component signed volume and closedness (geobi_part_solids) and
// the flip of marked components (geobi_flip_faces).  The reference has no counterpart; the rules are stated in
// include/geobi_hip.h and restated in numpy fp64 in tests/wind_model.py.
//
// The term of one (query, face) pair, in ONE order, contraction off: a, b, c = the fp64 differences of the float32 corners
// and the float32 query (exact);
//   det   = (ax*(by*cz - bz*cy) + ay*(bz*cx - bx*cz)) + az*(bx*cy - by*cx)
//   (u.w) = (ux*wx + uy*wy) + uz*wz,   la = sqrt(a.a), lb = sqrt(b.b), lc = sqrt(c.c)
//   den   = (la*(lb*lc) + (b.c)*la) + ((a.b)*lc + (c.a)*lb)       (symmetric in b and c: reversing a face negates det
//           and leaves den its bits, so it negates the term exactly)
//   theta = 2*atan2(det, den);  det == 0: the term is 0 (the principal value for a query in the face's plane, on the
//           face included: the sign of a zero never decides between 0 and +-2 pi)
// Finite float32 inputs cannot overflow: |difference| < 2^129, a product of three < 2^387.
//
// The sum is an INTEGER sum.  Quantum: 2^-40 of a full turn.  A term is llrint(theta / (4 pi) * 2^40), |term| <= 2^39
// (|theta| <= 2 pi); the terms of a query are added as int64 -- per (query, slice) in the walk, the slices in the reduce
// -- and w = sum * 2^-40.  Integer addition is associative, so w does not depend on how choose_slices cut the faces
// (a function of Q): the same query gets the same bits alone and in a batch.  Bound: F <= 2^23 faces keep |sum| <= 2^62;
// more are refused by name (GEOBI_MAX_NODES = 2^24 - 1 would allow 2^63).  The int64 -> fp64 conversion is exact for
// |sum| < 2^53, that is |w| < 2^13.  No float atomics, no integer ones either: a partial has one writer.
//
// The all-pairs walk of dist.hip / selfx.hip: a lane owns ONE query in registers; the workgroup stages a tile of 256 faces
// in LDS (three float4 per face: the corners, gathered once per tile, a mark for a face that takes part and its part id;
// see Tile); every lane reads the SAME record (LDS broadcast).  A face takes part when its state is 1
// (no state: all), its ids are distinct and lie in [0, V).  With both part arrays a pair whose parts are equal is skipped.
// One query per lane and no unroll of the record loop: one inlined copy of the term (three fp64 sqrt, one fp64 atan2, one
// fp64 division), no scratch -- DESIGN.md 4v has the register report.
//
// Bounds: a face row is read for f < F only and its ids are tested against [0, V) before a vertex is read; a query row
// for q < Q only; a tile index j stays below the staged n <= kTile; part[q * S + slice] has q < Q, slice < S; label values
// used as indices are tested against [0, F) first; sorted positions stay below the n of their table.
#include "common.h"
#include "pair_slices.h"
#include "edge_table.h"
#include "../../include/geobi_hip.h"

#include <math.h>

#pragma clang fp contract(off)

namespace geobi {

namespace {

constexpr int kThreads = kWalkThreads;
constexpr int kQpl = 1, kTile = 256;                    // 12 KB of LDS: three float4 per face
static_assert(kTile == kThreads, "one thread stages one face of the tile");
constexpr int64_t kMaxWindingFaces = (int64_t)1 << 23;  // |term| <= 2^39: the int64 sum stays within 2^62
constexpr double kQuantaPerTurn = 1099511627776.0;      // 2^40
constexpr double kFourPi = 12.566370614359172;          // fp64 nearest to 4 pi = 0x402921FB54442D18

struct D3 { double x, y, z; };
__device__ __forceinline__ double dot(const D3& u, const D3& w) {
#pragma clang fp contract(off)
  return (u.x * w.x + u.y * w.y) + u.z * w.z;
}
__device__ __forceinline__ double det3(const D3& a, const D3& b, const D3& c) {
#pragma clang fp contract(off)
  return (a.x * (b.y * c.z - b.z * c.y) + a.y * (b.z * c.x - b.x * c.z)) + a.z * (b.x * c.y - b.y * c.x);
}

// the quantised signed solid angle of the triangle whose corners, seen from the query, are a, b, c
__device__ __forceinline__ long long winding_term(const D3& a, const D3& b, const D3& c) {
#pragma clang fp contract(off)
  const double det = det3(a, b, c);
  if (det == 0.0) return 0;
  const double la = sqrt(dot(a, a)), lb = sqrt(dot(b, b)), lc = sqrt(dot(c, c));
  const double den = (la * (lb * lc) + dot(b, c) * la) + (dot(a, b) * lc + dot(c, a) * lb);
  const double theta = 2.0 * atan2(det, den);
  return llrint(theta / kFourPi * kQuantaPerTurn);
}

// r0 = (a, b.x)  r1 = (b.y, b.z, c.x, c.y)  r2 = (c.z, takes part ? 1 : 0, part id as bits, -)
struct Tile { float4 r[3][kTile]; };

__global__ __launch_bounds__(kThreads) void winding_walk_kernel(const float* __restrict__ q, const float* __restrict__ verts,
                                                                const int* __restrict__ fv, const int* __restrict__ state,
                                                                const int* __restrict__ face_part,
                                                                const int* __restrict__ query_part, int Q, int V, int F,
                                                                int tiles_per_slice, long long* __restrict__ part) {
  __shared__ Tile tile;
  const int tid = threadIdx.x, slice = blockIdx.y, S = gridDim.y;
  const int qi = blockIdx.x * (kThreads * kQpl) + tid;
  const int t_begin = slice * tiles_per_slice * kTile;                   // < F: no slice is empty
  const int t_end = min(F, t_begin + tiles_per_slice * kTile);
  const bool parts = face_part != nullptr && query_part != nullptr;
  D3 p = {0.0, 0.0, 0.0};
  int my_part = 0;
  if (qi < Q) {
    p = {(double)q[3 * (size_t)qi], (double)q[3 * (size_t)qi + 1], (double)q[3 * (size_t)qi + 2]};
    if (parts) my_part = query_part[qi];
  }
  long long sum = 0;
  for (int t0 = t_begin; t0 < t_end; t0 += kTile) {
    const int n = min(kTile, t_end - t0);
    __syncthreads();
    if (tid < n) {
      const int f = t0 + tid;                                            // < t_end <= F
      const int ia = fv[3 * (size_t)f], ib = fv[3 * (size_t)f + 1], ic = fv[3 * (size_t)f + 2];
      const bool in = (state == nullptr || state[f] == 1) && (unsigned)ia < (unsigned)V && (unsigned)ib < (unsigned)V &&
                      (unsigned)ic < (unsigned)V && ia != ib && ib != ic && ic != ia;
      float c[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (in) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          c[k] = verts[3 * (size_t)ia + k];
          c[3 + k] = verts[3 * (size_t)ib + k];
          c[6 + k] = verts[3 * (size_t)ic + k];
        }
      }
      tile.r[0][tid] = make_float4(c[0], c[1], c[2], c[3]);
      tile.r[1][tid] = make_float4(c[4], c[5], c[6], c[7]);
      tile.r[2][tid] = make_float4(c[8], in ? 1.f : 0.f, __int_as_float(parts ? face_part[f] : 0), 0.f);
    }
    __syncthreads();
#pragma nounroll
    for (int j = 0; j < n; ++j) {
      const float4 r2 = tile.r[2][j];
      if (r2.y == 0.f) continue;                                         // uniform: every lane reads the same record
      if (parts && __float_as_int(r2.z) == my_part) continue;
      const float4 r0 = tile.r[0][j], r1 = tile.r[1][j];
      const D3 a = {(double)r0.x - p.x, (double)r0.y - p.y, (double)r0.z - p.z};
      const D3 b = {(double)r0.w - p.x, (double)r1.x - p.y, (double)r1.y - p.z};
      const D3 c = {(double)r1.z - p.x, (double)r1.w - p.y, (double)r2.x - p.z};
      sum += winding_term(a, b, c);
    }
  }
  if (qi < Q) part[(size_t)qi * S + slice] = sum;
}

// w[q] = (the int64 sum of q's S partials) * 2^-40
__global__ __launch_bounds__(kThreads) void winding_reduce_kernel(const long long* __restrict__ part, int Q, int S,
                                                                  double* __restrict__ w) {
  const int qi = blockIdx.x * kThreads + threadIdx.x;
  if (qi >= Q) return;
  long long sum = 0;
  for (int s = 0; s < S; ++s) sum += part[(size_t)qi * S + s];
  w[qi] = (double)sum * (1.0 / kQuantaPerTurn);                          // a power of two: the product is exact
}

struct WindingBuffers { long long* part; };                              // [Q * S], query-major and slice-minor
WindingBuffers carve_winding(Arena& a, int64_t Q, int slices) { return {a.take<long long>((size_t)Q * slices)}; }
Slicing winding_slices(int64_t Q, int64_t F) { return choose_slices(Q, F, kQpl, kTile); }

// ---------------------------------------------------------------------------------------------- part_solids
constexpr int kT = 256;
constexpr unsigned kLabelBits = 25;                                      // labels < 2^24, and 2^24 for a face outside

// whether face f belongs to a component: included as edge_table.h says, with a label in [0, F)
__device__ __forceinline__ bool solid_face(const int* __restrict__ fv, const int* __restrict__ state,
                                           const int* __restrict__ label, int f, int V, int F, int& a, int& b, int& c) {
  return face_included(fv, state, f, V, a, b, c) && (unsigned)label[f] < (unsigned)F;
}

// sort keys: the label, or 2^24 for a face that belongs to none; closed / consistent start as 1 at the roots
__global__ void solids_init_kernel(const int* __restrict__ fv, const int* __restrict__ state, const int* __restrict__ label,
                                   int F, int V, uint32_t* __restrict__ keys, int* __restrict__ vals,
                                   int* __restrict__ closed, int* __restrict__ consistent, int* __restrict__ start,
                                   int* __restrict__ end, double* __restrict__ volume6) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  int a, b, c;
  const bool in = solid_face(fv, state, label, f, V, F, a, b, c);
  const int root = in && label[f] == f ? 1 : 0;
  keys[f] = in ? (uint32_t)label[f] : (1u << 24);
  vals[f] = f;
  closed[f] = root;
  consistent[f] = root;
  start[f] = 0;
  end[f] = 0;
  volume6[f] = 0.0;
}

// per sorted edge slot: a run that is not of exactly two opens the component of its face; a run of two whose claimants
// walk the edge the same way makes it inconsistent (plain stores of one value)
__global__ void solids_edges_kernel(const uint64_t* __restrict__ keys, const int* __restrict__ vals,
                                    const int* __restrict__ label, int n, int F, int* __restrict__ closed,
                                    int* __restrict__ consistent) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = keys[i];
  if (key == kNoEdge) return;
  const int f = (vals[i] >> 1) / 3;
  if ((unsigned)f >= (unsigned)F) return;                               // never: a value is slot << 1 | bit, slot < 3 F
  const int lab = label[f];
  if ((unsigned)lab >= (unsigned)F) return;
  const bool has_prev = i > 0 && keys[i - 1] == key, has_next = i + 1 < n && keys[i + 1] == key;
  bool two = has_prev != has_next;
  if (two) {
    const int j = has_prev ? i - 1 : i + 1, far = has_prev ? i - 2 : i + 2;
    if (far >= 0 && far < n && keys[far] == key) two = false;
    else if (((vals[i] ^ vals[j]) & 1) == 0) consistent[lab] = 0;
  }
  if (!two) closed[lab] = 0;
}

// the run of every label in the table sorted by label: [start, end)
__global__ void solids_runs_kernel(const uint32_t* __restrict__ keys, int F, int* __restrict__ start, int* __restrict__ end) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= F) return;
  const uint32_t key = keys[i];
  if (key >= (uint32_t)F) return;
  if (i == 0 || keys[i - 1] != key) start[key] = i;
  if (i + 1 == F || keys[i + 1] != key) end[key] = i + 1;
}

// one 64-lane wave per face x; the wave of a root sums its component: lane l adds the ranks r == l (mod 64) of the run in
// ascending r, then every lane adds the 64 partial sums in ascending lane order from 0.0 (fill.hip's shape)
__global__ __launch_bounds__(kT) void solids_volume_kernel(const float* __restrict__ verts, const int* __restrict__ fv,
                                                           const int* __restrict__ state, const int* __restrict__ label,
                                                           const int* __restrict__ sorted_face, const int* __restrict__ start,
                                                           const int* __restrict__ end, int F, int V,
                                                           double* __restrict__ volume6) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int x = blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
  if (x >= F) return;                                                    // uniform over the wave
  int a, b, c;
  if (!solid_face(fv, state, label, x, V, F, a, b, c) || label[x] != x) return;
  const int r0 = start[x], r1 = end[x];
  if (r0 < 0 || r1 > F || r0 >= r1) return;                              // never: a root is in its own run
  const D3 o = {(double)verts[3 * (size_t)a], (double)verts[3 * (size_t)a + 1], (double)verts[3 * (size_t)a + 2]};
  double partial = 0.0;
  for (int r = r0 + lane; r < r1; r += 64) {
    const int f = sorted_face[r];
    if ((unsigned)f >= (unsigned)F) continue;                            // never
    int i0, i1, i2;
    if (!solid_face(fv, state, label, f, V, F, i0, i1, i2)) continue;    // never: the run holds faces of the label
    const D3 u = {(double)verts[3 * (size_t)i0] - o.x, (double)verts[3 * (size_t)i0 + 1] - o.y, (double)verts[3 * (size_t)i0 + 2] - o.z};
    const D3 v = {(double)verts[3 * (size_t)i1] - o.x, (double)verts[3 * (size_t)i1 + 1] - o.y, (double)verts[3 * (size_t)i1 + 2] - o.z};
    const D3 w = {(double)verts[3 * (size_t)i2] - o.x, (double)verts[3 * (size_t)i2 + 1] - o.y, (double)verts[3 * (size_t)i2 + 2] - o.z};
    partial += det3(u, v, w);
  }
  double total = 0.0;
  for (int src = 0; src < 64; ++src) total += __shfl(partial, src);
  if (lane == 0) volume6[x] = total;
}

struct SolidsBuffers {
  MeshTables t;                                                          // the edge table alone
  uint32_t *k_in, *k_out;                                                // [F] labels before and after the sort
  int *v_in, *v_out, *start, *end;                                       // [F] faces before and after it; the runs
  PairSort<uint32_t, int> label_sort;
};
SolidsBuffers carve_solids(Arena& a, int64_t F) {
  return {carve_tables<false, false>(a, F), a.take<uint32_t>(F), a.take<uint32_t>(F), a.take<int>(F), a.take<int>(F),
          a.take<int>(F), a.take<int>(F), PairSort<uint32_t, int>::take(a, F, kLabelBits)};
}

// faces_out may be fv itself (no __restrict__ on the two): a lane reads its row before it writes it
__global__ void flip_faces_kernel(const int* fv, const int* __restrict__ label, const int* __restrict__ flip_of_label, int F,
                                  int* faces_out, int* __restrict__ flip_io) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  const int lab = label[f];
  const bool turn = (unsigned)lab < (unsigned)F && flip_of_label[lab] != 0;
  const int a = fv[3 * (size_t)f], b = fv[3 * (size_t)f + 1], c = fv[3 * (size_t)f + 2];   // read before the row is written
  faces_out[3 * (size_t)f] = a;
  faces_out[3 * (size_t)f + 1] = turn ? c : b;
  faces_out[3 * (size_t)f + 2] = turn ? b : c;
  if (turn) flip_io[f] ^= 1;
}

}  // namespace

}  // namespace geobi

using namespace geobi;

extern "C" {

int geobi_winding_number_slices(int64_t Q, int64_t F) {
  return Q <= 0 || F <= 0 || Q > GEOBI_MAX_NODES || F > kMaxWindingFaces ? 0 : winding_slices(Q, F).slices;
}

size_t geobi_winding_number_ws_bytes(int64_t Q, int64_t F) {
  if (Q < 0 || F < 0 || Q > GEOBI_MAX_NODES || F > kMaxWindingFaces) return 0;
  if (Q == 0 || F == 0) return kWsSlack;
  return carve_bytes([&](Arena& a) { carve_winding(a, Q, winding_slices(Q, F).slices); });
}

// The counterpart of nothing in the reference.
int geobi_winding_number(const float* q, const float* verts, const int32_t* faces, const int32_t* state,
                         const int32_t* face_part, const int32_t* query_part, int64_t Q, int64_t V, int64_t F, void* w_out,
                         void* ws, size_t ws_bytes, void* stream) {
  GEOBI_MESH_SIZES(F, V);
  GEOBI_SIZES(Q, 0);
  GEOBI_REQUIRE(F <= kMaxWindingFaces, "%s: F = %lld faces (at most 2^23 = %lld: the int64 sum of terms of up to 2^39 each)",
                __func__, (long long)F, (long long)kMaxWindingFaces);
  hipStream_t s = as_stream(stream);
  if (Q == 0) return 0;
  GEOBI_NOTNULL(w_out);
  double* w = (double*)w_out;
  if (F == 0) {
    GEOBI_HIP(hipMemsetAsync(w, 0, sizeof(double) * (size_t)Q, s));
    return 0;
  }
  GEOBI_NOTNULL(q); GEOBI_NOTNULL(verts); GEOBI_NOTNULL(faces);
  const Slicing sl = winding_slices(Q, F);
  WindingBuffers b;
  GEOBI_TRY(carve_checked("winding_number", ws, ws_bytes, b, [&](Arena& a) { return carve_winding(a, Q, sl.slices); }));
  winding_walk_kernel<<<dim3(sl.qblocks, sl.slices), kThreads, 0, s>>>(q, verts, faces, state, face_part, query_part, (int)Q,
                                                                      (int)V, (int)F, sl.tiles_per_slice, b.part);
  GEOBI_LAUNCH_OK();
  winding_reduce_kernel<<<cdiv(Q, kThreads), kThreads, 0, s>>>(b.part, (int)Q, sl.slices, w);
  GEOBI_LAUNCH_OK();
  return 0;
}

size_t geobi_part_solids_ws_bytes(int64_t F) {
  if (F < 0 || F > GEOBI_MAX_NODES) return 0;
  if (F == 0) return kWsSlack;
  return carve_bytes([&](Arena& a) { carve_solids(a, F); });
}

int geobi_part_solids(const float* verts, const int32_t* faces, const int32_t* state, const int32_t* label, int64_t V,
                      int64_t F, void* volume6_out, int32_t* closed, int32_t* consistent, void* ws, size_t ws_bytes,
                      void* stream) {
  GEOBI_MESH_SIZES(F, V);
  hipStream_t s = as_stream(stream);
  if (F == 0) return 0;
  GEOBI_NOTNULL(verts); GEOBI_NOTNULL(faces); GEOBI_NOTNULL(label); GEOBI_NOTNULL(volume6_out); GEOBI_NOTNULL(closed);
  GEOBI_NOTNULL(consistent);
  double* volume6 = (double*)volume6_out;
  SolidsBuffers b;
  GEOBI_TRY(carve_checked("part_solids", ws, ws_bytes, b, [&](Arena& a) { return carve_solids(a, F); }));
  const int n = (int)F, blocks = cdiv(F, kT);
  solids_init_kernel<<<blocks, kT, 0, s>>>(faces, state, label, n, (int)V, b.k_in, b.v_in, closed, consistent, b.start, b.end,
                                          volume6);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(build_edge_table(b.t, faces, state, F, V, s));
  solids_edges_kernel<<<cdiv(3 * F, kT), kT, 0, s>>>(b.t.k_out, b.t.v_out, label, 3 * n, n, closed, consistent);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(b.label_sort.run(b.k_in, b.k_out, b.v_in, b.v_out, s));
  solids_runs_kernel<<<blocks, kT, 0, s>>>(b.k_out, n, b.start, b.end);
  GEOBI_LAUNCH_OK();
  solids_volume_kernel<<<cdiv(F, kT / 64), kT, 0, s>>>(verts, faces, state, label, b.v_out, b.start, b.end, n, (int)V, volume6);
  GEOBI_LAUNCH_OK();
  return 0;
}

int geobi_flip_faces(const int32_t* faces, const int32_t* label, const int32_t* flip_of_label, int64_t F,
                     int32_t* faces_out, int32_t* flip_io, void* stream) {
  GEOBI_SIZES(F, 0);
  if (F == 0) return 0;
  GEOBI_NOTNULL(faces); GEOBI_NOTNULL(label); GEOBI_NOTNULL(flip_of_label); GEOBI_NOTNULL(faces_out); GEOBI_NOTNULL(flip_io);
  flip_faces_kernel<<<cdiv(F, kT), kT, 0, as_stream(stream)>>>(faces, label, flip_of_label, (int)F, faces_out, flip_io);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // extern "C"
