// Mesh repair on the device: weld vertices with equal keys, drop degenerate faces, apply
// openmesh's "complex edge" rule (a directed half-edge has one owner: the first kept face that lists it), compact.
// The reference gets the same effect from om.read_trimesh, which refuses such faces while it reads the file
// (code/test_dual.py:30, code/dataset.py:197); this project's reader keeps every face, so the rule lives here.
//
// Everything is integer-exact and independent of launch geometry:
//   weld     keys per vertex (three 32-bit words), three stable 32-bit LSD radix passes z, y, x over (key, index) pairs
//            (rocPRIM), run heads flagged, group numbers by a scan of the flags, every member takes its run's head --
//            the LOWEST index of the run, because the sort is stable
//   faces    corners through canon, degenerate faces marked, the 3F half-edges (a << 24 | b) sorted stably with their
//            slot 3f + k as value (the buffers and the sort of edge_table.h; the slots are filled here, DIRECTED): a run
//            lists the claimants of one half-edge in ascending face order.  Kept / dropped is
//            resolved in JACOBI rounds over ping-pong state: an undecided face walks the EARLIER claimants of its three
//            runs in the previous round's state -- one kept: dropped; all dropped: kept; else still undecided.  The lowest
//            undecided face is decided in every round, so the loop ends; the states a round reads are the previous
//            round's only, so the result and the number of rounds are functions of the input alone
//   compact  used flags by plain stores of one value, two exclusive scans, gathers
// The only floating-point operation is the division of the grid key.
#include "common.h"
#include "edge_table.h"
#include "../../include/geobi_hip.h"

namespace geobi {

namespace {

constexpr int kT = 256;
constexpr int kFirstBatch = 4;       // rounds enqueued before the first read of the undecided counts
constexpr int kBatch = 32;           // and per read after that (geobi_read_i32 takes 64 words)

// mode 1: the bit pattern with -0.0 folded into +0.0 (what x + 0.0f gives, without an fp operation);
// mode 2: floorf(x / tol) as int32, plain correctly rounded division; a quotient outside int32 sets bad[0]
__global__ void weld_keys_kernel(const float* __restrict__ pts, int V, int mode, float tol, uint32_t* __restrict__ kx,
                                 uint32_t* __restrict__ ky, uint32_t* __restrict__ kz, int* __restrict__ idx,
                                 int* __restrict__ bad) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  uint32_t k[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float x = pts[3 * (size_t)v + c];
    if (mode == 1) {
      const uint32_t b = __float_as_uint(x);
      k[c] = b == 0x80000000u ? 0u : b;
    } else {
      const float q = floorf(__fdiv_rn(x, tol));
      if (q >= -2147483648.0f && q < 2147483648.0f) {
        k[c] = (uint32_t)(int32_t)q;
      } else {
        k[c] = 0u;
        bad[0] = 1;
      }
    }
  }
  kx[v] = k[0]; ky[v] = k[1]; kz[v] = k[2];
  idx[v] = v;
}

__global__ void gather_u32_kernel(const uint32_t* __restrict__ src, const int* __restrict__ order, int n,
                                  uint32_t* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[order[i]];
}

// flag[i] = 1 where sorted position i starts a run of equal keys; flag[V] = 0 (scan tail)
__global__ void weld_heads_kernel(const uint32_t* __restrict__ kx, const uint32_t* __restrict__ ky,
                                  const uint32_t* __restrict__ kz, const int* __restrict__ order, int V,
                                  int* __restrict__ flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > V) return;
  if (i == V) { flag[V] = 0; return; }
  int head = 1;
  if (i > 0) {
    const int p = order[i], q = order[i - 1];
    head = (kx[p] != kx[q]) | (ky[p] != ky[q]) | (kz[p] != kz[q]);
  }
  flag[i] = head;
}

__global__ void weld_head_index_kernel(const int* __restrict__ order, const int* __restrict__ flag,
                                       const int* __restrict__ rank, int V, int* __restrict__ head_of_group) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < V && flag[i]) head_of_group[rank[i]] = order[i];
}

__global__ void weld_canon_kernel(const int* __restrict__ order, const int* __restrict__ flag, const int* __restrict__ rank,
                                  const int* __restrict__ head_of_group, int V, const int* __restrict__ bad,
                                  int* __restrict__ canon, int* __restrict__ counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) { counts[0] = rank[V]; counts[1] = bad[0]; }
  if (i < V) canon[order[i]] = head_of_group[rank[i] + flag[i] - 1];
}

__global__ void weld_identity_kernel(int V, int* __restrict__ canon, int* __restrict__ counts) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v == 0) { counts[0] = V; counts[1] = 0; }
  if (v < V) canon[v] = v;
}

// corners through canon, the start state, the three half-edge slots.  A corner outside [0, V) (the caller range-checks;
// this only keeps the gather inside the array) makes the face degenerate.
__global__ void face_remap_kernel(const int* __restrict__ fv, const int* __restrict__ canon, int F, int V, int manifold,
                                  int* __restrict__ fc, int* __restrict__ state, uint64_t* __restrict__ keys,
                                  int* __restrict__ slots, int* __restrict__ n_degenerate) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  bool deg = false;
  if (f < F) {
    int a = fv[3 * (size_t)f], b = fv[3 * (size_t)f + 1], c = fv[3 * (size_t)f + 2];
    const bool ok = (unsigned)a < (unsigned)V && (unsigned)b < (unsigned)V && (unsigned)c < (unsigned)V;
    if (ok) { a = canon[a]; b = canon[b]; c = canon[c]; } else { a = b = c = 0; }
    deg = a == b || b == c || c == a;
    fc[3 * (size_t)f] = a; fc[3 * (size_t)f + 1] = b; fc[3 * (size_t)f + 2] = c;
    state[f] = deg ? kDegenerate : (manifold ? kUndecided : kKept);
    if (manifold) {
      keys[3 * (size_t)f] = deg ? kNoEdge : edge_key(a, b);
      keys[3 * (size_t)f + 1] = deg ? kNoEdge : edge_key(b, c);
      keys[3 * (size_t)f + 2] = deg ? kNoEdge : edge_key(c, a);
      slots[3 * f] = 3 * f; slots[3 * f + 1] = 3 * f + 1; slots[3 * f + 2] = 3 * f + 2;
    }
  }
  count_lanes(deg, n_degenerate);
}

__global__ void slot_position_kernel(const int* __restrict__ sorted_slots, int n, int* __restrict__ pos) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) pos[sorted_slots[i]] = i;
}

// one Jacobi round: reads s_in only, writes every face of s_out; undecided[0] += faces still undecided after it
__global__ void face_round_kernel(const uint64_t* __restrict__ keys, const int* __restrict__ sorted_slots,
                                  const int* __restrict__ pos, const int* __restrict__ s_in, int* __restrict__ s_out, int F,
                                  int* __restrict__ undecided) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  int st = kKept;
  if (f < F) {
    st = s_in[f];
    if (st == kUndecided) {
      bool hit = false, pending = false;
      for (int k = 0; k < 3 && !hit; ++k) {
        const int p = pos[3 * f + k];
        const uint64_t key = keys[p];
        for (int j = p - 1; j >= 0 && keys[j] == key; --j) {      // earlier claimants: lower faces, the sort is stable
          const int sg = s_in[sorted_slots[j] / 3];
          if (sg == kKept) { hit = true; break; }
          if (sg == kUndecided) pending = true;
        }
      }
      st = hit ? kDropped : (pending ? kUndecided : kKept);
    }
    s_out[f] = st;
  }
  count_lanes(st == kUndecided, undecided);
}

__global__ void compact_mark_kernel(const int* __restrict__ fc, const int* __restrict__ state, int F, int V,
                                    int* __restrict__ keep, int* __restrict__ used, int* __restrict__ counts) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  int st = -1;
  if (f == F) keep[F] = 0;            // scan tail
  if (f < F) {
    st = state[f];
    keep[f] = st == kKept;
    if (st == kKept) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int a = fc[3 * (size_t)f + k];
        if ((unsigned)a < (unsigned)V) used[a] = 1;
      }
    }
  }
  count_lanes(st == kDegenerate, counts + 2);
  count_lanes(st == kDropped, counts + 3);
}

__global__ void compact_vertices_kernel(const float* __restrict__ pts, const int* __restrict__ canon,
                                        const int* __restrict__ used, const int* __restrict__ vrank, int V,
                                        float* __restrict__ pts_out, int* __restrict__ vertex_map,
                                        int* __restrict__ vertex_src, int* __restrict__ counts) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  bool loose = false;
  if (v < V) {
    int c = canon[v];
    if ((unsigned)c >= (unsigned)V) c = v;
    const int m = used[c] ? vrank[c] : -1;
    vertex_map[v] = m;
    loose = m < 0;
    if (used[v]) {                    // only canonical vertices are ever marked
      const int r = vrank[v];
      pts_out[3 * (size_t)r] = pts[3 * (size_t)v];
      pts_out[3 * (size_t)r + 1] = pts[3 * (size_t)v + 1];
      pts_out[3 * (size_t)r + 2] = pts[3 * (size_t)v + 2];
      vertex_src[r] = v;
    }
  }
  count_lanes(loose, counts + 4);
}

__global__ void compact_faces_kernel(const int* __restrict__ fc, const int* __restrict__ keep, const int* __restrict__ frank,
                                     const int* __restrict__ vrank, int F, int V, int* __restrict__ faces_out,
                                     int* __restrict__ face_map, int* __restrict__ counts) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f == 0) { counts[0] = vrank[V]; counts[1] = frank[F]; }
  if (f >= F || !keep[f]) return;
  const int r = frank[f];
  face_map[r] = f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = fc[3 * (size_t)f + k];
    faces_out[3 * (size_t)r + k] = (unsigned)a < (unsigned)V ? vrank[a] : 0;
  }
}

struct WeldBuffers {
  uint32_t *kx, *ky, *kz, *ka, *kb;
  int *idx, *va, *vb, *flag, *rank, *head, *bad;
  PairSort<uint32_t, int> sort; IntScan scan;      // sort: one temporary, the three passes of the LSD sort
};
WeldBuffers carve_weld(Arena& a, int64_t V) {
  return {a.take<uint32_t>(V), a.take<uint32_t>(V), a.take<uint32_t>(V), a.take<uint32_t>(V), a.take<uint32_t>(V),
          a.take<int>(V), a.take<int>(V), a.take<int>(V), a.take<int>(V + 1), a.take<int>(V + 1), a.take<int>(V),
          a.take<int>(1), PairSort<uint32_t, int>::take(a, V), IntScan::take(a, V + 1)};
}

struct FaceBuffers {
  MeshTables t;                      // the edge table alone, here over DIRECTED half-edges: face_remap_kernel fills it
  int *pos, *state_b, *counters;
};
FaceBuffers carve_faces(Arena& a, int64_t F) {
  return {carve_tables<false, false>(a, F), a.take<int>(3 * F), a.take<int>(F), a.take<int>(1 + kBatch)};
}

struct CompactBuffers {
  int *used, *vrank, *keep, *frank;
  IntScan scan_v, scan_f;
};
CompactBuffers carve_compact(Arena& a, int64_t V, int64_t F) {
  return {a.take<int>(V + 1), a.take<int>(V + 1), a.take<int>(F + 1), a.take<int>(F + 1),
          IntScan::take(a, V + 1), IntScan::take(a, F + 1)};
}

}  // namespace

}  // namespace geobi

using namespace geobi;

extern "C" {

size_t geobi_clean_weld_ws_bytes(int64_t V) {
  return V < 0 || V > GEOBI_MAX_NODES ? 0 : carve_bytes([&](Arena& a) { carve_weld(a, V); });
}

int geobi_clean_weld(const float* points, int64_t V, int mode, float weld_tol, int32_t* canon, int32_t* counts, void* ws,
                     size_t ws_bytes, void* stream) {
  GEOBI_SIZES(V, 0);
  GEOBI_NOTNULL(points); GEOBI_NOTNULL(canon); GEOBI_NOTNULL(counts);
  GEOBI_REQUIRE(mode >= 0 && mode <= 2, "clean_weld: mode %d (0 none, 1 exact, 2 grid)", mode);
  GEOBI_REQUIRE(mode != 2 || (weld_tol > 0.0f && weld_tol <= 3.0e38f), "clean_weld: grid mode needs a finite weld_tol > 0");
  hipStream_t s = as_stream(stream);
  const int n = (int)V, blocks = cdiv(V > 0 ? V : 1, kT);
  if (mode == 0 || V == 0) {
    weld_identity_kernel<<<blocks, kT, 0, s>>>(n, canon, counts);
    GEOBI_LAUNCH_OK();
    return 0;
  }
  WeldBuffers w;
  GEOBI_TRY(carve_checked("clean_weld", ws, ws_bytes, w, [&](Arena& a) { return carve_weld(a, V); }));
  GEOBI_HIP(hipMemsetAsync(w.bad, 0, sizeof(int), s));
  weld_keys_kernel<<<blocks, kT, 0, s>>>(points, n, mode, weld_tol, w.kx, w.ky, w.kz, w.idx, w.bad);
  GEOBI_LAUNCH_OK();
  // LSD: least significant word first; each pass is stable, so the order of the earlier passes survives among equal keys
  GEOBI_TRY(w.sort.run(w.kz, w.kb, w.idx, w.vb, s));
  gather_u32_kernel<<<blocks, kT, 0, s>>>(w.ky, w.vb, n, w.ka);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(w.sort.run(w.ka, w.kb, w.vb, w.va, s));
  gather_u32_kernel<<<blocks, kT, 0, s>>>(w.kx, w.va, n, w.ka);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(w.sort.run(w.ka, w.kb, w.va, w.vb, s));
  weld_heads_kernel<<<cdiv(V + 1, kT), kT, 0, s>>>(w.kx, w.ky, w.kz, w.vb, n, w.flag);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(w.scan.run(w.flag, w.rank, s));
  weld_head_index_kernel<<<blocks, kT, 0, s>>>(w.vb, w.flag, w.rank, n, w.head);
  GEOBI_LAUNCH_OK();
  weld_canon_kernel<<<blocks, kT, 0, s>>>(w.vb, w.flag, w.rank, w.head, n, w.bad, canon, counts);
  GEOBI_LAUNCH_OK();
  return 0;
}

size_t geobi_clean_faces_ws_bytes(int64_t F) {
  return F < 0 || F > GEOBI_MAX_NODES ? 0 : carve_bytes([&](Arena& a) { carve_faces(a, F); });
}

int geobi_clean_faces(const int32_t* faces, const int32_t* canon, int64_t F, int64_t V, int manifold, int max_rounds,
                      int32_t* faces_canon, int32_t* state, int32_t* rounds, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(F > V ? F : V, 0);
  GEOBI_NOTNULL(faces); GEOBI_NOTNULL(canon); GEOBI_NOTNULL(faces_canon); GEOBI_NOTNULL(state); GEOBI_NOTNULL(rounds);
  GEOBI_REQUIRE(max_rounds >= 1, "clean_faces: max_rounds = %d (at least 1)", max_rounds);
  hipStream_t s = as_stream(stream);
  *rounds = 0;
  if (F == 0) return 0;
  FaceBuffers b;
  GEOBI_TRY(carve_checked("clean_faces", ws, ws_bytes, b, [&](Arena& a) { return carve_faces(a, F); }));
  const int n = (int)F, blocks = cdiv(F, kT);
  GEOBI_HIP(hipMemsetAsync(b.counters, 0, sizeof(int), s));
  face_remap_kernel<<<blocks, kT, 0, s>>>(faces, canon, n, (int)V, manifold, faces_canon, state, b.t.k_in, b.t.v_in, b.counters);
  GEOBI_LAUNCH_OK();
  if (!manifold) return 0;
  GEOBI_TRY(sort_edge_table(b.t, F, s));
  slot_position_kernel<<<cdiv(3 * F, kT), kT, 0, s>>>(b.t.v_out, 3 * n, b.pos);
  GEOBI_LAUNCH_OK();
  int* cur = state;
  int* other = b.state_b;
  int done = 0;
  while (true) {
    const int left = max_rounds - done;
    const int want = done == 0 ? kFirstBatch : kBatch;
    const int batch = left < want ? left : want;
    GEOBI_HIP(hipMemsetAsync(b.counters + 1, 0, sizeof(int) * batch, s));
    for (int r = 0; r < batch; ++r) {
      face_round_kernel<<<blocks, kT, 0, s>>>(b.t.k_out, b.t.v_out, b.pos, cur, other, n, b.counters + 1 + r);
      GEOBI_LAUNCH_OK();
      int* t = cur; cur = other; other = t;
    }
    int32_t host[1 + kBatch];
    GEOBI_TRY(geobi_read_i32(b.counters, 1 + batch, host, (void*)s));      // one wait per batch
    if (host[0] == n) break;                                               // nothing but degenerate faces: 0 rounds
    int r = 0;
    while (r < batch && host[1 + r] != 0) ++r;
    if (r < batch) { *rounds = done + r + 1; break; }                      // the rounds after it only copied the state
    done += batch;
    if (done >= max_rounds)
      return set_error("clean_faces: %d faces still undecided after max_rounds = %d rounds (a chain of faces that "
                       "each share a directed edge with the next)", (int)host[batch], max_rounds);
  }
  if (cur != state) GEOBI_HIP(hipMemcpyAsync(state, cur, sizeof(int) * (size_t)F, hipMemcpyDeviceToDevice, s));
  return 0;
}

size_t geobi_clean_compact_ws_bytes(int64_t V, int64_t F) {
  if (V < 0 || F < 0 || V > GEOBI_MAX_NODES || F > GEOBI_MAX_NODES) return 0;
  return carve_bytes([&](Arena& a) { carve_compact(a, V, F); });
}

int geobi_clean_compact(const float* points, const int32_t* faces_canon, const int32_t* state, const int32_t* canon,
                        int64_t V, int64_t F, float* points_out, int32_t* faces_out, int32_t* vertex_map,
                        int32_t* vertex_src, int32_t* face_map, int32_t* counts, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(F > V ? F : V, 0);
  GEOBI_NOTNULL(points); GEOBI_NOTNULL(faces_canon); GEOBI_NOTNULL(state); GEOBI_NOTNULL(canon);
  GEOBI_NOTNULL(points_out); GEOBI_NOTNULL(faces_out);
  GEOBI_NOTNULL(vertex_map); GEOBI_NOTNULL(vertex_src); GEOBI_NOTNULL(face_map); GEOBI_NOTNULL(counts);
  hipStream_t s = as_stream(stream);
  CompactBuffers c;
  GEOBI_TRY(carve_checked("clean_compact", ws, ws_bytes, c, [&](Arena& a) { return carve_compact(a, V, F); }));
  GEOBI_HIP(hipMemsetAsync(counts, 0, sizeof(int) * 5, s));
  GEOBI_HIP(hipMemsetAsync(c.used, 0, sizeof(int) * (size_t)(V + 1), s));
  compact_mark_kernel<<<cdiv(F + 1, kT), kT, 0, s>>>(faces_canon, state, (int)F, (int)V, c.keep, c.used, counts);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(c.scan_v.run(c.used, c.vrank, s));
  GEOBI_TRY(c.scan_f.run(c.keep, c.frank, s));
  if (V > 0) {
    compact_vertices_kernel<<<cdiv(V, kT), kT, 0, s>>>(points, canon, c.used, c.vrank, (int)V, points_out, vertex_map,
                                                       vertex_src, counts);
    GEOBI_LAUNCH_OK();
  }
  compact_faces_kernel<<<cdiv(F > 0 ? F : 1, kT), kT, 0, s>>>(faces_canon, c.keep, c.frank, c.vrank, (int)F, (int)V,
                                                              faces_out, face_map, counts);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // extern "C"
