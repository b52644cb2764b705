// Mesh topology on the device: consistent winding, connected components, the edge report -- the
// stage between "weld / drop bad faces" (clean.hip) and "build graphs".
//
// Everything is integer-exact and independent of launch geometry; there is no floating point in this file:
//   table    the edge table of edge_table.h, which subdiv.hip, decim.hip and remesh.hip build through the same code: every
//            included face (state 1, three different corners) lists its three UNDIRECTED edges lo << 24 | hi in the
//            slots 3f + k, sorted stably (48 bits, rocPRIM) with slot << 1 | direction bit as value: a run lists the
//            claimants of one edge in ascending slot order.  One pass over the sorted table writes, per slot, the
//            orientation link (runs of exactly two with different opposite corners; odd when the direction bits are equal)
//            and the component links (the previous and the next claimant of every run of two or more)
//   rounds   connected components with parity by synchronous hooking: key[x] = 2 * label + parity, a round reads `key`
//            only and lowers `next` (a copy of key) with integer atomicMin -- hook the parent, hook the face, shortcut.
//            No thread reads `next` during the round and min commutes, so `next`, the result and the number of changed
//            rounds are functions of the input alone.  A min is only issued where it is below the key it targets (next
//            starts as key: the others change nothing), and any such min marks the round as changed
//   finish   label = key >> 1, parity = key & 1; bad[label] = 1 by a plain store where a link contradicts the parities;
//            component sizes by integer adds, the lanes of a wave that share a label first summed in the wave
// Every value used as an index is a face index below F: keys only ever hold 2 * face + bit, links hold slot / 3.
#include "common.h"
#include "edge_table.h"
#include "stage_timer.h"
#include "../../include/geobi_hip.h"

namespace geobi {

namespace {

constexpr int kT = 256;
constexpr int kBatch = 8;            // rounds enqueued per read of the changed flags

// per sorted position: the links of its slot.  olink[s] = (face << 1 | odd) or -1; clink[2s], clink[2s + 1] = the previous
// and the next claimant (face << 1) or -1
__global__ void topo_links_kernel(const uint64_t* __restrict__ keys, const int* __restrict__ vals,
                                  const int* __restrict__ fv, int n, int* __restrict__ olink, int* __restrict__ clink) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = keys[i];
  const int s = vals[i] >> 1, d = vals[i] & 1;
  int o = -1, cp = -1, cn = -1;
  if (key != kNoEdge) {
    const bool has_prev = i > 0 && keys[i - 1] == key, has_next = i + 1 < n && keys[i + 1] == key;
    if (has_prev) cp = ((vals[i - 1] >> 1) / 3) << 1;
    if (has_next) cn = ((vals[i + 1] >> 1) / 3) << 1;
    if (has_prev != has_next) {
      const int j = has_prev ? i - 1 : i + 1, far = has_prev ? i - 2 : i + 2;
      const bool longer = far >= 0 && far < n && keys[far] == key;
      if (!longer) {                                  // a run of exactly two
        const int t = vals[j] >> 1, dj = vals[j] & 1;
        const int g = t / 3, f = s / 3;
        const int opp_other = fv[3 * (size_t)g + (t % 3 + 2) % 3], opp_mine = fv[3 * (size_t)f + (s % 3 + 2) % 3];
        if (opp_other != opp_mine) o = g << 1 | (d == dj ? 1 : 0);
      }
    }
  }
  olink[s] = o;
  clink[2 * (size_t)s] = cp;
  clink[2 * (size_t)s + 1] = cn;
}

// run heads: edges, boundary edges (run of 1), complex edges (3 and more), inconsistent edges (2 with equal direction bits)
__global__ void topo_edge_report_kernel(const uint64_t* __restrict__ keys, const int* __restrict__ vals, int n,
                                        int* __restrict__ counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool head = false, boundary = false, complex_edge = false, inconsistent = false;
  if (i < n) {
    const uint64_t key = keys[i];
    head = key != kNoEdge && (i == 0 || keys[i - 1] != key);
    if (head) {
      const bool two = i + 1 < n && keys[i + 1] == key, three = two && i + 2 < n && keys[i + 2] == key;
      boundary = !two;
      complex_edge = three;
      inconsistent = two && !three && ((vals[i] ^ vals[i + 1]) & 1) == 0;
    }
  }
  count_lanes(head, counts);
  count_lanes(boundary, counts + 1);
  count_lanes(complex_edge, counts + 2);
  count_lanes(inconsistent, counts + 3);
}

__global__ void topo_mark_used_kernel(const int* __restrict__ fv, const int* __restrict__ state, int F, int V,
                                      int* __restrict__ used, int* __restrict__ counts) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  bool inc = false;
  if (f < F) {
    int a, b, c;
    inc = face_included(fv, state, f, V, a, b, c);
    if (inc) { used[a] = 1; used[b] = 1; used[c] = 1; }             // plain stores of one value
  }
  count_lanes(inc, counts + 5);
  count_lanes(f < F && !inc, counts + 6);
}

__global__ void topo_count_used_kernel(const int* __restrict__ used, int V, int* __restrict__ counts) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  count_lanes(v < V && used[v] != 0, counts + 4);
}

__global__ void topo_init_keys_kernel(int F, uint32_t* __restrict__ key, uint32_t* __restrict__ next) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x < F) { key[x] = 2u * (uint32_t)x; next[x] = 2u * (uint32_t)x; }
}

// One synchronous round.  links holds L entries per face (face << 1 | odd, or -1).  Reads key only; lowers next, which
// holds a copy of key, with atomicMin; changed[0] = 1 (a plain store of one value) iff some min is below the key it targets,
// which is exactly next != key after the round.
__global__ void topo_round_kernel(const int* __restrict__ links, int L, int F, const uint32_t* __restrict__ key,
                                  uint32_t* __restrict__ next, int* __restrict__ changed) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= F) return;
  const uint32_t kx = key[x];
  const uint32_t f = kx >> 1, p = kx & 1u;
  const uint32_t g = key[f];
  uint32_t best = (g & ~1u) | (p ^ (g & 1u));                      // shortcut: 2 * gf + pg
  bool any = false;
  for (int k = 0; k < L; ++k) {
    const int e = links[(size_t)L * x + k];
    if (e < 0) continue;
    const uint32_t w = (uint32_t)e >> 1, odd = (uint32_t)e & 1u;
    const uint32_t kw = key[w];
    const uint32_t gw = key[kw >> 1];
    const uint32_t to_w = odd ^ (kw & 1u) ^ (gw & 1u);             // parity of x against w's grandparent
    const uint32_t hook_parent = (gw & ~1u) | (p ^ to_w);
    if (hook_parent < g) { atomicMin(next + f, hook_parent); any = true; }
    const uint32_t hook_face = (gw & ~1u) | to_w;
    best = hook_face < best ? hook_face : best;
  }
  if (best < kx) { atomicMin(next + x, best); any = true; }
  if (any) changed[0] = 1;
}

// bad[label[u]] = 1 where a link contradicts the parities (a plain store of one value)
__global__ void topo_check_kernel(const int* __restrict__ olink, int F, const uint32_t* __restrict__ key,
                                  int* __restrict__ bad) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= F) return;
  const uint32_t kx = key[x];
  for (int k = 0; k < 3; ++k) {
    const int e = olink[3 * (size_t)x + k];
    if (e < 0) continue;
    const uint32_t kw = key[(uint32_t)e >> 1];
    if (((kx ^ kw) & 1u) != ((uint32_t)e & 1u)) bad[kx >> 1] = 1;
  }
}

// label, flip, the oriented face table (any of the three may be NULL) and the counts: [0] components, [1] non-orientable
// components, [2] flipped faces
__global__ void topo_orient_out_kernel(const int* __restrict__ fv, const int* __restrict__ state, int F, int V,
                                       const uint32_t* __restrict__ key, const int* __restrict__ bad,
                                       int* __restrict__ faces_out, int* __restrict__ flip, int* __restrict__ label,
                                       int* __restrict__ counts) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  bool root = false, bad_root = false, flipped = false;
  if (x < F) {
    int a, b, c;
    const bool inc = face_included(fv, state, x, V, a, b, c);
    const uint32_t kx = key[x];
    const int lab = (int)(kx >> 1);
    root = inc && lab == x;
    bad_root = root && bad[x] != 0;
    flipped = inc && (kx & 1u) != 0 && bad[lab] == 0;
    if (label != nullptr) label[x] = inc ? lab : -1;
    if (flip != nullptr) flip[x] = flipped ? 1 : 0;
    if (faces_out != nullptr) {
      faces_out[3 * (size_t)x] = a;
      faces_out[3 * (size_t)x + 1] = flipped ? c : b;
      faces_out[3 * (size_t)x + 2] = flipped ? b : c;
    }
  }
  count_lanes(root, counts);
  count_lanes(bad_root, counts + 1);
  count_lanes(flipped, counts + 2);
}

// size[label] += 1 per included face: the lanes of a wave that share a label are summed first (a one-component mesh
// sends every face to one address), then one integer add per distinct label and wave
__global__ void topo_sizes_kernel(const int* __restrict__ fv, const int* __restrict__ state, int F, int V,
                                  const uint32_t* __restrict__ key, int* __restrict__ size) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  bool pending = false;
  int lab = -1;
  if (x < F) {
    int a, b, c;
    pending = face_included(fv, state, x, V, a, b, c);
    lab = (int)(key[x] >> 1);
  }
  const int lane = threadIdx.x & 63;
  unsigned long long left = __ballot(pending);
  while (left != 0) {
    const int leader = __ffsll((long long)left) - 1;
    const int leader_label = __shfl(lab, leader);
    const unsigned long long same = __ballot(pending && lab == leader_label);
    if (lane == leader) atomicAdd(size + leader_label, __popcll(same));
    if (pending && lab == leader_label) pending = false;
    left &= ~same;
  }
}

// comp, state_out (either may be NULL) and the counts: [0] components, [1] components below min_component, [2] their faces;
// size == NULL: no sizes were taken, no part is small
__global__ void topo_components_out_kernel(const int* __restrict__ fv, const int* __restrict__ state, int F, int V,
                                           const uint32_t* __restrict__ key, const int* __restrict__ size,
                                           int min_component, int* __restrict__ comp, int* __restrict__ state_out,
                                           int* __restrict__ counts) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  bool root = false, small_root = false, small = false;
  if (x < F) {
    int a, b, c;
    const bool inc = face_included(fv, state, x, V, a, b, c);
    const int lab = (int)(key[x] >> 1);
    root = inc && lab == x;
    small = inc && size != nullptr && size[lab] < min_component;
    small_root = root && small;
    if (comp != nullptr) comp[x] = inc ? lab : -1;
    if (state_out != nullptr) {
      const int st = state == nullptr ? kKept : state[x];
      state_out[x] = small ? kSmallPart : (st == kKept && !inc ? kDegenerate : st);
    }
  }
  count_lanes(root, counts);
  count_lanes(small_root, counts + 1);
  count_lanes(small, counts + 2);
}

struct TopoBuffers {
  MeshTables t;                                                    // the edge table alone
  int *olink, *clink, *per_label, *used, *flags;                   // per_label: bad marks, then component sizes
  uint32_t *key, *next;
};
TopoBuffers carve_topo(Arena& a, int64_t F, int64_t V) {
  return {carve_tables<false, false>(a, F), a.take<int>(3 * F), a.take<int>(6 * F), a.take<int>(F), a.take<int>(V),
          a.take<int>(kBatch), a.take<uint32_t>(F), a.take<uint32_t>(F)};
}

int build_table(const int32_t* faces, const int32_t* state, int64_t F, int64_t V, const TopoBuffers& b, hipStream_t s) {
  GEOBI_TRY(build_edge_table(b.t, faces, state, F, V, s));
  topo_links_kernel<<<cdiv(3 * F, kT), kT, 0, s>>>(b.t.k_out, b.t.v_out, faces, (int)(3 * F), b.olink, b.clink);
  GEOBI_LAUNCH_OK();
  return 0;
}

// the rounds over one set of links, until a round changes nothing; the keys are left in b.key.  At most max_rounds + 1
// rounds are enqueued: the last of them only shows that round max_rounds was the last one that changed something.
int run_rounds(const char* what, const int* links, int L, int64_t F, int max_rounds, const TopoBuffers& b, int32_t* rounds,
               hipStream_t s) {
  const int n = (int)F, blocks = cdiv(F, kT);
  topo_init_keys_kernel<<<blocks, kT, 0, s>>>(n, b.key, b.next);
  GEOBI_LAUNCH_OK();
  const int64_t limit = (int64_t)max_rounds + 1;
  int64_t done = 0;
  while (true) {
    const int batch = (int)(limit - done < kBatch ? limit - done : kBatch);
    GEOBI_HIP(hipMemsetAsync(b.flags, 0, sizeof(int) * batch, s));
    for (int r = 0; r < batch; ++r) {
      topo_round_kernel<<<blocks, kT, 0, s>>>(links, L, n, b.key, b.next, b.flags + r);
      GEOBI_LAUNCH_OK();
      GEOBI_HIP(hipMemcpyAsync(b.key, b.next, sizeof(uint32_t) * (size_t)F, hipMemcpyDeviceToDevice, s));
    }
    int32_t host[kBatch];
    GEOBI_TRY(geobi_read_i32(b.flags, batch, host, (void*)s));             // one wait per batch
    int r = 0;
    while (r < batch && host[r] != 0) ++r;
    if (r < batch) { *rounds = (int32_t)(done + r); return 0; }            // the rounds after it changed nothing either
    done += batch;
    if (done >= limit)
      return set_error("%s: the labels still change after max_rounds = %d rounds (a long chain of faces whose order in "
                       "the file works against the hooking)", what, max_rounds);
  }
}

int topo_buffers(const char* what, int64_t F, int64_t V, void* ws, size_t ws_bytes, TopoBuffers& b) {
  return carve_checked(what, ws, ws_bytes, b, [&](Arena& a) { return carve_topo(a, F, V); });
}

}  // namespace

}  // namespace geobi

using namespace geobi;

extern "C" {

size_t geobi_topo_ws_bytes(int64_t F, int64_t V) {
  if (V < 0 || F < 0 || V > GEOBI_MAX_NODES || F > GEOBI_MAX_NODES) return 0;
  return carve_bytes([&](Arena& a) { carve_topo(a, F, V); });
}

int geobi_topo_orient(const int32_t* faces, const int32_t* state, int64_t F, int64_t V, int max_rounds,
                      int32_t* faces_out, int32_t* flip, int32_t* label, int32_t* counts, int32_t* rounds,
                      float* stage_ms, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(F > V ? F : V, 0);
  GEOBI_NOTNULL(faces); GEOBI_NOTNULL(faces_out); GEOBI_NOTNULL(flip); GEOBI_NOTNULL(label); GEOBI_NOTNULL(counts);
  GEOBI_NOTNULL(rounds);
  GEOBI_REQUIRE(max_rounds >= 1, "topo_orient: max_rounds = %d (at least 1)", max_rounds);
  hipStream_t s = as_stream(stream);
  *rounds = 0;
  GEOBI_HIP(hipMemsetAsync(counts, 0, sizeof(int) * 3, s));
  if (F == 0) return 0;
  TopoBuffers b;
  GEOBI_TRY(topo_buffers("topo_orient", F, 0, ws, ws_bytes, b));
  StageTimer timer(stage_ms, s);
  GEOBI_TRY(timer.mark());
  GEOBI_TRY(build_table(faces, state, F, V, b, s));
  GEOBI_TRY(timer.mark());
  GEOBI_TRY(run_rounds("topo_orient", b.olink, 3, F, max_rounds, b, rounds, s));
  GEOBI_TRY(timer.mark());
  GEOBI_HIP(hipMemsetAsync(b.per_label, 0, sizeof(int) * (size_t)F, s));
  topo_check_kernel<<<cdiv(F, kT), kT, 0, s>>>(b.olink, (int)F, b.key, b.per_label);
  GEOBI_LAUNCH_OK();
  topo_orient_out_kernel<<<cdiv(F, kT), kT, 0, s>>>(faces, state, (int)F, (int)V, b.key, b.per_label, faces_out, flip,
                                                    label, counts);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(timer.mark());
  return timer.finish();
}

int geobi_topo_components(const int32_t* faces, const int32_t* state, int64_t F, int64_t V, int min_component,
                          int max_rounds, int32_t* comp, int32_t* state_out, int32_t* counts, int32_t* rounds,
                          float* stage_ms, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(F > V ? F : V, 0);
  GEOBI_NOTNULL(faces); GEOBI_NOTNULL(comp); GEOBI_NOTNULL(state_out); GEOBI_NOTNULL(counts); GEOBI_NOTNULL(rounds);
  GEOBI_REQUIRE(max_rounds >= 1, "topo_components: max_rounds = %d (at least 1)", max_rounds);
  GEOBI_REQUIRE(min_component >= 0, "topo_components: min_component = %d (0 or more)", min_component);
  hipStream_t s = as_stream(stream);
  *rounds = 0;
  GEOBI_HIP(hipMemsetAsync(counts, 0, sizeof(int) * 3, s));
  if (F == 0) return 0;
  TopoBuffers b;
  GEOBI_TRY(topo_buffers("topo_components", F, 0, ws, ws_bytes, b));
  StageTimer timer(stage_ms, s);
  GEOBI_TRY(timer.mark());
  GEOBI_TRY(build_table(faces, state, F, V, b, s));
  GEOBI_TRY(timer.mark());
  GEOBI_TRY(run_rounds("topo_components", b.clink, 6, F, max_rounds, b, rounds, s));
  GEOBI_TRY(timer.mark());
  GEOBI_HIP(hipMemsetAsync(b.per_label, 0, sizeof(int) * (size_t)F, s));
  topo_sizes_kernel<<<cdiv(F, kT), kT, 0, s>>>(faces, state, (int)F, (int)V, b.key, b.per_label);
  GEOBI_LAUNCH_OK();
  topo_components_out_kernel<<<cdiv(F, kT), kT, 0, s>>>(faces, state, (int)F, (int)V, b.key, b.per_label, min_component,
                                                        comp, state_out, counts);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(timer.mark());
  return timer.finish();
}

int geobi_topo_report(const int32_t* faces, const int32_t* state, int64_t F, int64_t V, int max_rounds, int32_t* counts,
                      int32_t* rounds, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(F > V ? F : V, 0);
  GEOBI_NOTNULL(faces); GEOBI_NOTNULL(counts); GEOBI_NOTNULL(rounds);
  GEOBI_REQUIRE(max_rounds >= 1, "topo_report: max_rounds = %d (at least 1)", max_rounds);
  hipStream_t s = as_stream(stream);
  rounds[0] = rounds[1] = 0;
  GEOBI_HIP(hipMemsetAsync(counts, 0, sizeof(int) * 16, s));
  if (F == 0) return 0;
  TopoBuffers b;
  GEOBI_TRY(topo_buffers("topo_report", F, V, ws, ws_bytes, b));
  const int blocks = cdiv(F, kT);
  GEOBI_TRY(build_table(faces, state, F, V, b, s));
  topo_edge_report_kernel<<<cdiv(3 * F, kT), kT, 0, s>>>(b.t.k_out, b.t.v_out, 3 * (int)F, counts);
  GEOBI_LAUNCH_OK();
  if (V > 0) GEOBI_HIP(hipMemsetAsync(b.used, 0, sizeof(int) * (size_t)V, s));
  topo_mark_used_kernel<<<blocks, kT, 0, s>>>(faces, state, (int)F, (int)V, b.used, counts);
  GEOBI_LAUNCH_OK();
  if (V > 0) {
    topo_count_used_kernel<<<cdiv(V, kT), kT, 0, s>>>(b.used, (int)V, counts);
    GEOBI_LAUNCH_OK();
  }
  GEOBI_TRY(run_rounds("topo_report", b.olink, 3, F, max_rounds, b, rounds, s));
  GEOBI_HIP(hipMemsetAsync(b.per_label, 0, sizeof(int) * (size_t)F, s));
  topo_check_kernel<<<blocks, kT, 0, s>>>(b.olink, (int)F, b.key, b.per_label);
  GEOBI_LAUNCH_OK();
  topo_orient_out_kernel<<<blocks, kT, 0, s>>>(faces, state, (int)F, (int)V, b.key, b.per_label, nullptr, nullptr, nullptr,
                                               counts + 8);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(run_rounds("topo_report", b.clink, 6, F, max_rounds, b, rounds + 1, s));
  // without sizes only counts[7] (the components) is added to
  topo_components_out_kernel<<<blocks, kT, 0, s>>>(faces, state, (int)F, (int)V, b.key, nullptr, 0, nullptr, nullptr,
                                                   counts + 7);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // extern "C"
