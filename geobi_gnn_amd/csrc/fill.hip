// Hole filling on the device: boundary slots -> ordered closed loops by pointer doubling -> one fan
// per selected loop around a new vertex.  The rules are stated in include/geobi_hip.h (geobi_fill_*); tests/fill_model.py
// restates them in plain Python and every output is compared bit for bit.
//
// The topology is integer-exact and independent of launch geometry; a centre is summed in one stated fp64 order by one wave,
// no float atomics:
//   table    the edge table of edge_table.h (build_edge_table)
//   flags    per sorted position: a run of one claimant flags its SLOT; a scan over the 3F slots compacts the boundary slots
//            into B ENTRIES in ascending slot order (entry e <-> slot ent_slot[e], bpos[slot] = e); in / out counts of the
//            vertices with integer atomicAdd; out_ent[v] = the entry that leaves v, a PLAIN STORE (it is read for simple
//            vertices only, where exactly one entry writes); successors
//   labels   pointer doubling on the entries, ping-pong: (lab, jump) <- (min(lab, lab[jump]), jump[jump]).  "dead" is
//            carried as lab = -1, below every slot, so the one min is both updates of the header's (lab, dead, jump);
//            an entry without successor starts dead with jump = itself
//   ranks    a second doubling towards the leader (lab == own slot: d = 0, jump = itself; the others d = 1, jump = next):
//            (d, jump) <- (d + d[jump], jump[jump]); len = d[next(leader)] + 1, rank = (len - d) mod len
//   rounds   ceil(log2(max(3F, 2))) for either doubling: B <= 3F, and B itself is known on the device only.  The grids
//            are sized for 3F entries; the lanes at and beyond B leave at once
//   tables   leader flags -> loop numbers (scan over the entries = ascending leader), selection -> new vertex ids and face
//            offsets (two scans over F >= L rows), per-slot loop / rank, and the rim vertices from(s) scattered to off + rank
//            so that a wave reads its loop contiguously (done here, not in the emit: a replay needs it before any emit)
//   emit     one lane per old row (copies), one lane per slot (the face of a selected boundary slot), one 64-lane wave per
//            selected loop (the centre)
// Every index is bounded: corners of included faces are below V (face_included), entries below B <= 3F, loops below L <= F,
// new rows below the V' and F' the caller read from the plan's counts.  No index comes out of a 48-bit key here: from / to
// are read from the face table (edge_table.h: index_from_key is for indices taken out of keys).
#include "common.h"
#include "edge_table.h"
#include "stage_timer.h"
#include "../../include/geobi_hip.h"

namespace geobi {

namespace {

constexpr int kT = 256;
enum Count { kB = 0, kBlocked = 1, kChain = 2, kLoops = 3, kLongest = 4, kFilled = 5, kSkipped = 6, kNewFaces = 7,
             kVOut = 8, kFOut = 9, kCounts = 16 };

// bflag[slot] = 1 for the one claimant of a run of one, 0 for every other slot (every slot is some position's value)
__global__ void fill_flags_kernel(const uint64_t* __restrict__ keys, const int* __restrict__ vals, int n,
                                  int* __restrict__ bflag, int* __restrict__ counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool boundary = false;
  if (i < n) {
    const Run r = run_at(keys, n, i);
    boundary = r.head && !r.two;
    const int slot = vals[i] >> 1;
    if ((unsigned)slot < (unsigned)n) bflag[slot] = boundary ? 1 : 0;
  }
  count_lanes(boundary, counts + kB);
}

// the walk of the hole along slot s = 3f + k: from corner k + 1 to corner k
__device__ __forceinline__ void slot_ends(const int* __restrict__ fv, int slot, int& from, int& to) {
  const int f = slot / 3, k = slot - 3 * f;
  to = fv[3 * (size_t)f + k];
  from = fv[3 * (size_t)f + (k + 1) % 3];
}

// one lane per slot: a boundary slot becomes entry bpos[slot], counts its two ends and names itself at its `from`
__global__ void fill_entries_kernel(const int* __restrict__ fv, int n, int V, const int* __restrict__ bflag,
                                    const int* __restrict__ bpos, int* __restrict__ ent_slot, int* __restrict__ out_cnt,
                                    int* __restrict__ in_cnt, int* __restrict__ out_ent) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n || bflag[s] == 0) return;
  const int e = bpos[s];
  int from, to;
  slot_ends(fv, s, from, to);
  if ((unsigned)e >= (unsigned)n || (unsigned)from >= (unsigned)V || (unsigned)to >= (unsigned)V) return;   // never
  ent_slot[e] = s;
  atomicAdd(out_cnt + from, 1);
  atomicAdd(in_cnt + to, 1);
  out_ent[from] = e;
}

__global__ void fill_blocked_kernel(const int* __restrict__ out_cnt, const int* __restrict__ in_cnt, int V,
                                    int* __restrict__ counts) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  bool blocked = false;
  if (v < V) blocked = out_cnt[v] + in_cnt[v] > 0 && !(out_cnt[v] == 1 && in_cnt[v] == 1);
  count_lanes(blocked, counts + kBlocked);
}

// next[e] (-1: none) and the start of the label doubling
__global__ void fill_successor_kernel(const int* __restrict__ fv, const int* __restrict__ ent_slot,
                                      const int* __restrict__ out_cnt, const int* __restrict__ in_cnt,
                                      const int* __restrict__ out_ent, const int* __restrict__ counts, int n, int V,
                                      int* __restrict__ next, int2* __restrict__ state) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x, B = counts[kB];
  if (e >= B) return;
  const int slot = ent_slot[e];
  int from = 0, to = -1;
  if ((unsigned)slot < (unsigned)n) slot_ends(fv, slot, from, to);     // always: every entry below B was written
  int nx = -1;
  if ((unsigned)to < (unsigned)V && out_cnt[to] == 1 && in_cnt[to] == 1) {
    nx = out_ent[to];
    if ((unsigned)nx >= (unsigned)B) nx = -1;                         // never: the one writer of a simple vertex is an entry
  }
  next[e] = nx;
  state[e] = nx >= 0 ? make_int2(slot, nx) : make_int2(-1, e);
}

__global__ void fill_label_round_kernel(const int2* __restrict__ in, const int* __restrict__ counts, int2* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= counts[kB]) return;
  const int2 x = in[e], y = in[x.y];
  out[e] = make_int2(x.x < y.x ? x.x : y.x, y.y);
}

// keeps the labels, counts chain entries and leaders, flags the leaders (0 at and beyond B: the scan runs over 3F) and
// starts the rank doubling
__global__ void fill_rank_start_kernel(const int2* __restrict__ labels, const int* __restrict__ ent_slot,
                                       const int* __restrict__ next, int n, int* __restrict__ lab, int* __restrict__ lead,
                                       int2* __restrict__ state, int* __restrict__ counts) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  bool chain = false, leader = false;
  if (e < n) {
    if (e < counts[kB]) {
      const int l = labels[e].x;
      chain = l < 0;
      leader = !chain && l == ent_slot[e];
      lab[e] = l;
      state[e] = chain || leader ? make_int2(0, e) : make_int2(1, next[e]);
    }
    lead[e] = leader ? 1 : 0;
  }
  count_lanes(chain, counts + kChain);
  count_lanes(leader, counts + kLoops);
}

__global__ void fill_rank_round_kernel(const int2* __restrict__ in, const int* __restrict__ counts, int2* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= counts[kB]) return;
  const int2 x = in[e], y = in[x.y];
  out[e] = make_int2(x.x + y.x, y.y);
}

// one lane per entry, the leaders write the row of their loop
__global__ void fill_loops_kernel(const int2* __restrict__ ranks, const int* __restrict__ lead,
                                  const int* __restrict__ loop_no, const int* __restrict__ ent_slot,
                                  const int* __restrict__ next, int F, int* __restrict__ loop_leader,
                                  int* __restrict__ loop_len, int* __restrict__ counts) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x, B = counts[kB];
  if (e >= B || lead[e] == 0) return;
  const int l = loop_no[e], nx = next[e];
  if ((unsigned)l >= (unsigned)F || (unsigned)nx >= (unsigned)B) return;   // never: L <= B / 3 <= F, a leader has a successor
  const int len = ranks[nx].x + 1;
  loop_leader[l] = ent_slot[e];
  loop_len[l] = len;
  atomicMax(counts + kLongest, len);
}

// one lane per row of the loop tables: the selection and the lengths it contributes (0 at and beyond L)
__global__ void fill_select_kernel(const int* __restrict__ loop_len, int F, int max_hole_edges,
                                   const int* __restrict__ counts, int* __restrict__ sel, int* __restrict__ sel_len) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= F) return;
  const bool take = l < counts[kLoops] && (max_hole_edges == 0 || loop_len[l] <= max_hole_edges);
  sel[l] = take ? 1 : 0;
  sel_len[l] = take ? loop_len[l] : 0;
}

// the loop of every new vertex, and the totals
__global__ void fill_totals_kernel(const int* __restrict__ sel, const int* __restrict__ sel_len,
                                   const int* __restrict__ sel_id, const int* __restrict__ sel_off, int F, int V,
                                   int* __restrict__ sel_loop, int* __restrict__ counts) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= F) return;
  if (sel[l] != 0 && (unsigned)sel_id[l] < (unsigned)F) sel_loop[sel_id[l]] = l;
  if (l == F - 1) {
    const int filled = sel_id[l] + sel[l], new_faces = sel_off[l] + sel_len[l];
    counts[kFilled] = filled;
    counts[kSkipped] = counts[kLoops] - filled;
    counts[kNewFaces] = new_faces;
    counts[kVOut] = V + filled;
    counts[kFOut] = F + new_faces;
  }
}

// one lane per slot: its loop and rank, and the rim vertex of a selected slot at off + rank of the ring
__global__ void fill_slots_kernel(const int* __restrict__ fv, int n, int F, const int* __restrict__ bflag,
                                  const int* __restrict__ bpos, const int* __restrict__ lab, const int2* __restrict__ ranks,
                                  const int* __restrict__ loop_no, const int* __restrict__ loop_len,
                                  const int* __restrict__ sel, const int* __restrict__ sel_off, const int* __restrict__ counts,
                                  int* __restrict__ slot_loop, int* __restrict__ slot_rank, int* __restrict__ ring) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  int loop = -1, rank = -1;
  if (bflag[s] != 0) {
    const int e = bpos[s], B = counts[kB];
    loop = -2;
    if ((unsigned)e < (unsigned)B && lab[e] >= 0) {
      const int2 r = ranks[e];                                        // (distance to the leader, the leader's entry)
      const int l = (unsigned)r.y < (unsigned)B ? loop_no[r.y] : -1;
      if ((unsigned)l < (unsigned)F) {
        const int len = loop_len[l];
        loop = l;
        rank = r.x == 0 ? 0 : len - r.x;
        if (sel[l] != 0 && rank >= 0 && rank < len && sel_off[l] + rank < n) {
          int from, to;
          slot_ends(fv, s, from, to);
          ring[sel_off[l] + rank] = from;
        }
      }
    }
  }
  slot_loop[s] = loop;
  slot_rank[s] = rank;
}

__global__ void fill_no_faces_kernel(int V, int* __restrict__ counts) { counts[kVOut] = V; }

// ---- emit
// one lane per old row of either table
__global__ void fill_copy_kernel(const int* __restrict__ fv, const float* __restrict__ points, int F, int V,
                                 int* __restrict__ faces_out, float* __restrict__ points_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < F && faces_out != nullptr)
    for (int k = 0; k < 3; ++k) faces_out[3 * (size_t)i + k] = fv[3 * (size_t)i + k];
  if (i < V)
    for (int k = 0; k < 3; ++k) points_out[3 * (size_t)i + k] = points[3 * (size_t)i + k];
}

// one lane per slot: the face of a selected boundary slot, (from, to, V + j) in row F + off + rank
__global__ void fill_faces_kernel(const int* __restrict__ fv, int n, int F, int V, int Vn, int Fn,
                                  const int* __restrict__ slot_loop, const int* __restrict__ slot_rank,
                                  const int* __restrict__ sel, const int* __restrict__ sel_id,
                                  const int* __restrict__ sel_off, int* __restrict__ faces_out,
                                  int* __restrict__ new_face_loop) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const int l = slot_loop[s];
  if ((unsigned)l >= (unsigned)F || sel[l] == 0) return;
  const int centre = V + sel_id[l], row = F + sel_off[l] + slot_rank[s];
  if (centre < V || centre >= Vn || row < F || row >= Fn) return;
  int from, to;
  slot_ends(fv, s, from, to);
  faces_out[3 * (size_t)row] = from;
  faces_out[3 * (size_t)row + 1] = to;
  faces_out[3 * (size_t)row + 2] = centre;
  new_face_loop[row - F] = l;
}

// one 64-lane wave per selected loop: lane l adds the ranks r == l (mod 64) in ascending r, then every lane adds the 64
// partial sums in ascending lane order (the same sequence in every lane); one division, one rounding
__global__ void fill_centres_kernel(const float* __restrict__ points, int V, int Vn, int F, int n,
                                    const int* __restrict__ sel_loop, const int* __restrict__ loop_len,
                                    const int* __restrict__ sel_off, const int* __restrict__ ring,
                                    const int* __restrict__ counts, float* __restrict__ points_out,
                                    int* __restrict__ new_vertex_loop) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
  if (j >= counts[kFilled] || j >= Vn - V) return;                    // uniform over the wave
  const int l = sel_loop[j];
  if ((unsigned)l >= (unsigned)F) return;
  const int len = loop_len[l], off = sel_off[l];
  if (len < 1 || off < 0 || off + len > n) return;                    // never
  double partial[3] = {0.0, 0.0, 0.0};
  for (int r = lane; r < len; r += 64) {
    const int v = ring[off + r];
    if ((unsigned)v >= (unsigned)V) continue;                         // never: the ring holds corners of included faces
    for (int k = 0; k < 3; ++k) partial[k] += (double)points[3 * (size_t)v + k];
  }
  double total[3] = {0.0, 0.0, 0.0};
  for (int src = 0; src < 64; ++src)
    for (int k = 0; k < 3; ++k) total[k] += __shfl(partial[k], src);
  if (lane < 3) {
    const double t = lane == 0 ? total[0] : (lane == 1 ? total[1] : total[2]);
    points_out[3 * (size_t)(V + j) + lane] = (float)(t / (double)len);
  }
  if (lane == 0 && new_vertex_loop != nullptr) new_vertex_loop[j] = l;
}

struct FillBuffers {
  // the state of a plan, read by emit and points
  int *slot_loop, *slot_rank, *ring, *loop_leader, *loop_len, *sel, *sel_id, *sel_off, *sel_loop, *counts;
  // scratch of the plan
  MeshTables t;
  int *bflag, *bpos, *ent_slot, *next, *lab, *lead, *loop_no, *out_cnt, *in_cnt, *out_ent, *sel_len;
  int2 *ping, *pong;
  ExclusiveScan<int> slot_scan, loop_scan;     // each serves two runs
};
FillBuffers carve_fill(Arena& a, int64_t F, int64_t V) {
  const int64_t n = 3 * F;
  return {a.take<int>(n), a.take<int>(n), a.take<int>(n), a.take<int>(F), a.take<int>(F), a.take<int>(F), a.take<int>(F),
          a.take<int>(F), a.take<int>(F), a.take<int>(kCounts),
          carve_tables<false, false>(a, F),
          a.take<int>(n), a.take<int>(n), a.take<int>(n), a.take<int>(n), a.take<int>(n), a.take<int>(n), a.take<int>(n),
          a.take<int>(V), a.take<int>(V), a.take<int>(V), a.take<int>(F),
          a.take<int2>(n), a.take<int2>(n),
          ExclusiveScan<int>::take(a, n), ExclusiveScan<int>::take(a, F)};
}

int fill_buffers(const char* what, int64_t F, int64_t V, void* ws, size_t ws_bytes, FillBuffers& b) {
  return carve_checked(what, ws, ws_bytes, b, [&](Arena& a) { return carve_fill(a, F, V); });
}

// the rounds of either doubling: 2^rounds >= 3F >= B
int doubling_rounds(int64_t n) {
  int r = 1;
  while (((int64_t)1 << r) < n) ++r;
  return r;
}

// the rows V .. Vn - 1 of points_out over the plan in b
int launch_centres(const float* points, int64_t F, int64_t V, int64_t Vn, const FillBuffers& b, float* points_out,
                   int32_t* new_vertex_loop, hipStream_t s) {
  if (Vn == V) return 0;
  fill_centres_kernel<<<cdiv(Vn - V, kT / 64), kT, 0, s>>>(points, (int)V, (int)Vn, (int)F, (int)(3 * F), b.sel_loop, b.loop_len,
                                                          b.sel_off, b.ring, b.counts, points_out, new_vertex_loop);
  GEOBI_LAUNCH_OK();
  return 0;
}

// what a plan of V, F can give: at most F loops (L <= B / 3), at most 3F new faces
int sizes_of_a_plan(const char* fn, int64_t F, int64_t V, int64_t Vn, int64_t Fn) {
  GEOBI_REQUIRE(Vn >= V && Vn - V <= F && Fn >= F && Fn - F <= 3 * F,
                "%s: V' = %lld, F' = %lld are not what a plan of V = %lld, F = %lld can give", fn, (long long)Vn,
                (long long)Fn, (long long)V, (long long)F);
  return 0;
}

}  // namespace

}  // namespace geobi

using namespace geobi;

extern "C" {

size_t geobi_fill_ws_bytes(int64_t F, int64_t V) {
  if (sizes_ok("geobi_fill_ws_bytes", F > V ? F : V, 0) != 0 || sizes_ok("geobi_fill_ws_bytes", F < V ? F : V, 0) != 0) return 0;
  return carve_bytes([&](Arena& a) { carve_fill(a, F, V); });
}

int geobi_fill_plan(const int32_t* faces, int64_t F, int64_t V, int max_hole_edges, int32_t* slot_loop,
                    int32_t* slot_rank, int32_t* loop_leader, int32_t* loop_len, int32_t* counts, float* stage_ms,
                    void* ws, size_t ws_bytes, void* stream) {
  GEOBI_MESH_SIZES(F, V);
  GEOBI_REQUIRE(max_hole_edges >= 0, "fill_plan: max_hole_edges = %d (0: every loop, else the longest loop to fill)",
                max_hole_edges);
  if (F > 0) GEOBI_NOTNULL(faces);
  GEOBI_NOTNULL(counts);
  hipStream_t s = as_stream(stream);
  if (F == 0) {                                   // nothing to fill: V' = V, F' = 0
    GEOBI_HIP(hipMemsetAsync(counts, 0, sizeof(int) * kCounts, s));
    fill_no_faces_kernel<<<1, 1, 0, s>>>((int)V, counts);
    GEOBI_LAUNCH_OK();
    return 0;
  }
  FillBuffers b;
  GEOBI_TRY(fill_buffers("fill_plan", F, V, ws, ws_bytes, b));
  const int n = (int)(3 * F), grid_n = cdiv(n, kT), grid_f = cdiv(F, kT);
  const int rounds = doubling_rounds(n);
  StageTimer timer(stage_ms, s);
  GEOBI_TRY(timer.mark());
  GEOBI_TRY(build_edge_table(b.t, faces, nullptr, F, V, s));
  GEOBI_TRY(timer.mark());
  // flags, entries, counts of the ends, successors
  GEOBI_HIP(hipMemsetAsync(b.counts, 0, sizeof(int) * kCounts, s));
  if (V > 0) {
    GEOBI_HIP(hipMemsetAsync(b.out_cnt, 0, sizeof(int) * (size_t)V, s));
    GEOBI_HIP(hipMemsetAsync(b.in_cnt, 0, sizeof(int) * (size_t)V, s));
  }
  fill_flags_kernel<<<grid_n, kT, 0, s>>>(b.t.k_out, b.t.v_out, n, b.bflag, b.counts);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(b.slot_scan.run(b.bflag, b.bpos, s));
  fill_entries_kernel<<<grid_n, kT, 0, s>>>(faces, n, (int)V, b.bflag, b.bpos, b.ent_slot, b.out_cnt, b.in_cnt, b.out_ent);
  GEOBI_LAUNCH_OK();
  if (V > 0) {
    fill_blocked_kernel<<<cdiv(V, kT), kT, 0, s>>>(b.out_cnt, b.in_cnt, (int)V, b.counts);
    GEOBI_LAUNCH_OK();
  }
  int2 *cur = b.ping, *other = b.pong;
  fill_successor_kernel<<<grid_n, kT, 0, s>>>(faces, b.ent_slot, b.out_cnt, b.in_cnt, b.out_ent, b.counts, n, (int)V,
                                             b.next, cur);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(timer.mark());
  // labels, then ranks
  for (int r = 0; r < rounds; ++r) {
    fill_label_round_kernel<<<grid_n, kT, 0, s>>>(cur, b.counts, other);
    GEOBI_LAUNCH_OK();
    int2* t = cur; cur = other; other = t;
  }
  fill_rank_start_kernel<<<grid_n, kT, 0, s>>>(cur, b.ent_slot, b.next, n, b.lab, b.lead, other, b.counts);
  GEOBI_LAUNCH_OK();
  { int2* t = cur; cur = other; other = t; }
  for (int r = 0; r < rounds; ++r) {
    fill_rank_round_kernel<<<grid_n, kT, 0, s>>>(cur, b.counts, other);
    GEOBI_LAUNCH_OK();
    int2* t = cur; cur = other; other = t;
  }
  GEOBI_TRY(timer.mark());
  // loop tables, selection, per-slot results
  GEOBI_TRY(b.slot_scan.run(b.lead, b.loop_no, s));
  fill_loops_kernel<<<grid_n, kT, 0, s>>>(cur, b.lead, b.loop_no, b.ent_slot, b.next, (int)F, b.loop_leader, b.loop_len, b.counts);
  GEOBI_LAUNCH_OK();
  fill_select_kernel<<<grid_f, kT, 0, s>>>(b.loop_len, (int)F, max_hole_edges, b.counts, b.sel, b.sel_len);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(b.loop_scan.run(b.sel, b.sel_id, s));
  GEOBI_TRY(b.loop_scan.run(b.sel_len, b.sel_off, s));
  fill_totals_kernel<<<grid_f, kT, 0, s>>>(b.sel, b.sel_len, b.sel_id, b.sel_off, (int)F, (int)V, b.sel_loop, b.counts);
  GEOBI_LAUNCH_OK();
  fill_slots_kernel<<<grid_n, kT, 0, s>>>(faces, n, (int)F, b.bflag, b.bpos, b.lab, cur, b.loop_no, b.loop_len, b.sel, b.sel_off,
                                         b.counts, b.slot_loop, b.slot_rank, b.ring);
  GEOBI_LAUNCH_OK();
  if (slot_loop != nullptr) GEOBI_HIP(hipMemcpyAsync(slot_loop, b.slot_loop, sizeof(int) * (size_t)n, hipMemcpyDeviceToDevice, s));
  if (slot_rank != nullptr) GEOBI_HIP(hipMemcpyAsync(slot_rank, b.slot_rank, sizeof(int) * (size_t)n, hipMemcpyDeviceToDevice, s));
  if (loop_leader != nullptr)
    GEOBI_HIP(hipMemcpyAsync(loop_leader, b.loop_leader, sizeof(int) * (size_t)F, hipMemcpyDeviceToDevice, s));
  if (loop_len != nullptr) GEOBI_HIP(hipMemcpyAsync(loop_len, b.loop_len, sizeof(int) * (size_t)F, hipMemcpyDeviceToDevice, s));
  GEOBI_HIP(hipMemcpyAsync(counts, b.counts, sizeof(int) * kCounts, hipMemcpyDeviceToDevice, s));
  GEOBI_TRY(timer.mark());
  return timer.finish();
}

int geobi_fill_emit(const int32_t* faces, const float* points, int64_t F, int64_t V, int64_t Vn, int64_t Fn,
                    int32_t* faces_out, float* points_out, int32_t* new_vertex_loop, int32_t* new_face_loop,
                    const void* ws, size_t ws_bytes, void* stream) {
  GEOBI_MESH_SIZES(F, V);
  GEOBI_SIZES(Vn > Fn ? Vn : Fn, 0);
  GEOBI_TRY(sizes_of_a_plan("fill_emit", F, V, Vn, Fn));
  if (F > 0) { GEOBI_NOTNULL(faces); GEOBI_NOTNULL(faces_out); }      // an empty array may have no address
  if (V > 0) { GEOBI_NOTNULL(points); GEOBI_NOTNULL(points_out); }
  if (Vn > V) { GEOBI_NOTNULL(points_out); GEOBI_NOTNULL(new_vertex_loop); }
  if (Fn > F) GEOBI_NOTNULL(new_face_loop);
  hipStream_t s = as_stream(stream);
  if ((F > V ? F : V) > 0) {
    fill_copy_kernel<<<cdiv(F > V ? F : V, kT), kT, 0, s>>>(faces, points, (int)F, (int)V, faces_out, points_out);
    GEOBI_LAUNCH_OK();
  }
  if (F == 0) return 0;
  FillBuffers b;
  GEOBI_TRY(fill_buffers("fill_emit", F, V, const_cast<void*>(ws), ws_bytes, b));
  if (Fn > F) {
    fill_faces_kernel<<<cdiv(3 * F, kT), kT, 0, s>>>(faces, (int)(3 * F), (int)F, (int)V, (int)Vn, (int)Fn, b.slot_loop,
                                                    b.slot_rank, b.sel, b.sel_id, b.sel_off, faces_out, new_face_loop);
    GEOBI_LAUNCH_OK();
  }
  return launch_centres(points, F, V, Vn, b, points_out, new_vertex_loop, s);
}

int geobi_fill_points(const float* points, int64_t F, int64_t V, int64_t Vn, float* points_out, const void* ws,
                      size_t ws_bytes, void* stream) {
  GEOBI_MESH_SIZES(F, V);
  GEOBI_SIZES(Vn, 0);
  GEOBI_TRY(sizes_of_a_plan("fill_points", F, V, Vn, F));
  if (Vn > 0) { GEOBI_NOTNULL(points); GEOBI_NOTNULL(points_out); }
  hipStream_t s = as_stream(stream);
  if (V > 0) {
    fill_copy_kernel<<<cdiv(V, kT), kT, 0, s>>>(nullptr, points, 0, (int)V, nullptr, points_out);
    GEOBI_LAUNCH_OK();
  }
  if (F == 0) return 0;
  FillBuffers b;
  GEOBI_TRY(fill_buffers("fill_points", F, V, const_cast<void*>(ws), ws_bytes, b));
  return launch_centres(points, F, V, Vn, b, points_out, nullptr, s);
}

}  // extern "C"
