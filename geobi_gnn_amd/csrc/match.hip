// Which nodes merge: the front half of a pooling step (PoolingLayer of the hot path, the reference's net_util.py:56-245),
// with its entry points.  segment.hip reduces over the clusters found here, pool.hip coarsens the edges.
//
//   edge_weight_t10   w_e += exp(-|x_i - x_j|^2 / 2)                       (net_util.py:226-230)
//   edge_weight_att   learned weights, edge_weight_type 3 / 4 / 5          (net_util.py:182-206)
//   match_*           heavy-edge matching, cluster id = min(u, v)          (graclus, net_util.py:127)
//   relabel           dense ids by rank of the representative              (consecutive_cluster, :128)
//   match_coarsen     rounds, commit, relabel and the matching's inverse lists in one call
//
// Matching specification (deterministic, unlike torch_cluster's randomised orders): an edge is
// taken iff it is the best remaining edge at BOTH endpoints under the total order
// (weight desc, min(u,v) asc, max(u,v) asc) -- i.e. greedy matching in globally descending edge
// order, computed by rounds of mutual proposals.  oracle/oracle_c.c:oracle_greedy_sorted is the
// sequential statement of the same rule.
//
// The count-to-offset scans are IntScan records (device_steps.h) and scan_exclusive_i32_pair; their kernels live in
// scan.hip.  Only the scan-free matching pair scans in place, with block_scan.h.  Nothing here sorts.
#include "../../include/geobi_hip.h"

#include "block_scan.h"
#include "common.h"
#include "device_steps.h"

namespace geobi {

namespace {

// A/B knob with a test hook: the environment decides (unset or non-zero = on) until geobi_set_match_scanfree forces a form
Knob g_match_scanfree{"GEOBI_MATCH_SCANFREE", 1};

// ------------------------------------------------------------------------ edge weights
// 8 lanes per edge, float4 per lane per pass.
__global__ __launch_bounds__(256) void edge_weight_t10_kernel(const float* __restrict__ x, int C,
                                                              const int* __restrict__ row,
                                                              const int* __restrict__ col,
                                                              const float* __restrict__ w_in, int64_t E,
                                                              float* __restrict__ w_out, int* __restrict__ zero8) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (zero8 != nullptr && t < 8) zero8[t] = 0;     // the pooling layer's counters, cleared on the way (one fill launch less)
  int64_t e = t >> 3;
  int l = (int)(t & 7);
  bool ok = e < E;
  int i = ok ? row[e] : 0, j = ok ? col[e] : 0;
  float d = 0.f;
  if (ok) {
    const float* xi = x + (size_t)i * C;
    const float* xj = x + (size_t)j * C;
    if ((C & 3) == 0) {
      for (int c = l * 4; c < C; c += 32) {
        float4 a = *reinterpret_cast<const float4*>(xi + c);
        float4 b = *reinterpret_cast<const float4*>(xj + c);
        float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z, dw = a.w - b.w;
        d = fmaf(dx, dx, d); d = fmaf(dy, dy, d); d = fmaf(dz, dz, d); d = fmaf(dw, dw, d);
      }
    } else {
      for (int c = l; c < C; c += 8) {
        float dd = xi[c] - xj[c];
        d = fmaf(dd, dd, d);
      }
    }
  }
  d += __shfl_xor(d, 1, 64);
  d += __shfl_xor(d, 2, 64);
  d += __shfl_xor(d, 4, 64);
  if (ok && l == 0) w_out[e] = (w_in ? w_in[e] : 0.f) + expf(d * -0.5f);
}

// Learned edge weights, PoolingLayer edge_weight_type 3 / 4 / 5 (/root/reference/code/net_util.py:182-206, GAT-style):
// per node al = x . att_l, ar = x . att_r (8 lanes per node, float4 per lane and pass), per edge
// sigmoid((al[r] + ar[c]) + (al[c] + ar[r])) in the reference's order of additions; type 5 averages with the given weight.
__global__ __launch_bounds__(256) void node_att_kernel(const float* __restrict__ x, int C, const float* __restrict__ att_l,
                                                       const float* __restrict__ att_r, int64_t N,
                                                       float2* __restrict__ alr) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i = t >> 3;
  const int l = (int)(t & 7);
  const bool ok = i < N;
  float a = 0.f, b = 0.f;
  if (ok) {
    const float* xi = x + (size_t)i * C;
    if ((C & 3) == 0) {
      for (int c = l * 4; c < C; c += 32) {
        const float4 v = *reinterpret_cast<const float4*>(xi + c);
        const float4 p = *reinterpret_cast<const float4*>(att_l + c);
        const float4 q = *reinterpret_cast<const float4*>(att_r + c);
        a = fmaf(v.x, p.x, a); a = fmaf(v.y, p.y, a); a = fmaf(v.z, p.z, a); a = fmaf(v.w, p.w, a);
        b = fmaf(v.x, q.x, b); b = fmaf(v.y, q.y, b); b = fmaf(v.z, q.z, b); b = fmaf(v.w, q.w, b);
      }
    } else {
      for (int c = l; c < C; c += 8) {
        a = fmaf(xi[c], att_l[c], a);
        b = fmaf(xi[c], att_r[c], b);
      }
    }
  }
#pragma unroll
  for (int m = 1; m < 8; m <<= 1) {
    a += __shfl_xor(a, m, 64);
    b += __shfl_xor(b, m, 64);
  }
  if (ok && l == 0) alr[i] = make_float2(a, b);
}

__global__ __launch_bounds__(256) void edge_weight_att_kernel(const float2* __restrict__ alr, const int* __restrict__ row,
                                                              const int* __restrict__ col, const float* __restrict__ w_in,
                                                              int64_t E, float* __restrict__ w_out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const float2 r = alr[row[e]], c = alr[col[e]];
  const float alpha = (r.x + c.y) + (c.x + r.y);
  const float sg = 1.0f / (1.0f + expf(-alpha));
  w_out[e] = w_in != nullptr ? (sg + w_in[e]) * 0.5f : sg;
}

// ---------------------------------------------------------------------------- matching
__device__ __forceinline__ bool edge_better(float w1, int a1, int b1, float w2, int a2, int b2) {
  // (a, b) = (min, max) endpoint ids
  if (w1 != w2) return w1 > w2;
  if (a1 != a2) return a1 < a2;
  return b1 < b2;
}

// One kernel per round: node u first commits the outcome of the PREVIOUS round from the proposal
// array alone (a pair is matched iff the proposals are mutual), then, if still free, proposes to its
// best free neighbour.  Whether a neighbour w is free is derived the same way (cluster[w] may or may
// not have been committed yet by w's own thread -- both views agree), so no second "resolve" launch
// and no grid-wide barrier is needed between the two halves of a round.
//   prop == -2 : no proposal information (before round 0)      prop == -1 : no free neighbour
// FIRST != 0: round 0 of a call -- every proposal is "no information" (-2) and, when the call starts from
// scratch (FIRST == 1), every node is undecided: nothing is read for it, and the round initialises the state
// itself (no separate init launch).
// A round is a chain of dependent loads per node, not bandwidth (9-11 us for 12 k nodes as for 82 k): the loads are
// therefore issued in four steps, each step's loads independent of one another --
//   A: own state, own proposal, row range      B: partner's proposal, up to MB neighbour ids + weights
//   C: the neighbours' states and proposals    D: the proposals of the neighbours' targets
// -- speculatively (a node that turns out to be decided has loaded a few words too many), instead of walking the
// neighbours one by one with four dependent loads each.
template <int FIRST>
__global__ __launch_bounds__(256) void match_round_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                   const float* __restrict__ w, const int* __restrict__ prop_prev, int N,
                                   int* __restrict__ cluster, int* __restrict__ prop_next, int* __restrict__ status) {
  constexpr int MB = 4;                  // neighbours per batch (8 and 4 measure alike, 16 is slower)
  int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (FIRST != 0 && u == 0) *status = 0;
  if (u >= N) return;
  // ---- step A
  const int rs = rowptr[u], re = rowptr[u + 1];
  int cu = -1, pv = -2;
  if (FIRST != 1) cu = cluster[u];
  if (FIRST == 0) pv = prop_prev[u];
  // ---- step B (speculative: issued before the node's own outcome is known)
  int ppv = -2;
  if (FIRST == 0) ppv = prop_prev[pv >= 0 ? pv : u];
  int vb[MB];
  float wb[MB];
#pragma unroll
  for (int i = 0; i < MB; ++i) {
    const int e = rs + i < re ? rs + i : (re > rs ? re - 1 : 0);
    vb[i] = re > rs ? col[e] : u;
    wb[i] = (w && re > rs) ? w[e] : 1.0f;
  }
  if (FIRST == 1) {
    cluster[u] = -1;
  } else {
    if (cu >= 0) { prop_next[u] = -1; return; }
    if (FIRST == 0) {
      if (pv == -1) { cluster[u] = u; prop_next[u] = -1; return; }
      if (pv >= 0 && ppv == u) { cluster[u] = pv; prop_next[u] = -1; return; }    // state = partner
    }
  }
  int best = -1, ba = 0, bb = 0;
  float bw = 0.f;
  for (int e0 = rs; e0 < re; e0 += MB) {
    if (e0 > rs) {                        // rows longer than one batch: the next MB ids and weights
#pragma unroll
      for (int i = 0; i < MB; ++i) {
        const int e = e0 + i < re ? e0 + i : re - 1;
        vb[i] = col[e];
        wb[i] = w ? w[e] : 1.0f;
      }
    }
    // ---- step C
    int cv[MB], pw[MB];
#pragma unroll
    for (int i = 0; i < MB; ++i) {
      cv[i] = FIRST == 1 ? -1 : cluster[vb[i]];
      pw[i] = FIRST == 0 ? prop_prev[vb[i]] : -2;
    }
    // ---- step D
    int ppw[MB];
#pragma unroll
    for (int i = 0; i < MB; ++i) ppw[i] = (FIRST == 0 && pw[i] >= 0) ? prop_prev[pw[i]] : -2;
#pragma unroll
    for (int i = 0; i < MB; ++i) {
      if (e0 + i >= re) break;
      const int v = vb[i];
      if (v == u) continue;
      // free = undecided and neither closed as a singleton nor mutually matched by the previous round (derived the
      // same way whether or not v's own thread has committed it yet -- both views agree)
      bool free_v = true;
      if (FIRST != 1) {
        if (cv[i] >= 0) free_v = false;
        else if (FIRST == 0) {
          if (pw[i] == -1) free_v = false;
          else if (pw[i] >= 0 && ppw[i] == v) free_v = false;
        }
      }
      if (!free_v) continue;
      const float we = wb[i];
      const int a = u < v ? u : v, b = u < v ? v : u;
      if (best < 0 || edge_better(we, a, b, bw, ba, bb)) { best = v; bw = we; ba = a; bb = b; }
    }
  }
  prop_next[u] = best;
}

// State of a node between calls (`cluster` of the launchers): -1 undecided, u closed as a singleton,
// v != u matched with partner v.  The cluster id graclus reports is min(u, state).
//
// commit of the last round + count of nodes that are still undecided; `final` (optional) receives the
// clustering with the undecided nodes closed as singletons; flag / sz (optional, both or neither):
// flag[u] = u is the representative (smaller member) of its cluster, sz[u] = its cluster size (0 for non-reps)
__global__ void match_commit_kernel(const int* __restrict__ prop, int N, int* __restrict__ cluster,
                                    int* __restrict__ remaining, int* __restrict__ final, int* __restrict__ flag,
                                    int* __restrict__ sz) {
  int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u == 0 && flag) { flag[N] = 0; sz[N] = 0; }      // scan tails
  if (u >= N) return;
  int st = cluster[u];
  if (st < 0) {
    int v = prop[u];
    if (v == -1) st = u;
    else if (v >= 0 && prop[v] == u) st = v;
    else atomicAdd(remaining, 1);
    if (st >= 0) cluster[u] = st;
  }
  const int fin = st < 0 ? u : (u < st ? u : st);
  if (final) final[u] = fin;
  if (flag) {
    const bool rep = fin == u;
    flag[u] = rep ? 1 : 0;
    sz[u] = rep ? ((st >= 0 && st != u) ? 2 : 1) : 0;
  }
}

// dense ids + inverse lists of the matching from the two scans (rank of a representative, offset of its
// members): cnew[u] = rank[rep(u)]; segment c = [rep, partner]; segptr[nc] = N closes the list
__global__ void match_lists_kernel(const int* __restrict__ state, const int* __restrict__ final,
                                   const int* __restrict__ rank, const int* __restrict__ offs, int N,
                                   int* __restrict__ cnew, int* __restrict__ count, int* __restrict__ segptr,
                                   int* __restrict__ members) {
  int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= N) return;
  const int rep = final[u];
  cnew[u] = rank[rep];
  if (rep == u) {
    const int o = offs[u];
    segptr[rank[u]] = o;
    members[o] = u;
    const int st = state[u];
    if (st >= 0 && st != u) members[o + 1] = st;
  }
  if (u == N - 1) {
    const int nc = rank[N];                            // exclusive scan over N + 1 entries: total at [N]
    *count = nc;
    segptr[nc] = N;
  }
}

// Scan-free variant of (match_commit, exclusive scans, match_lists) for up to 256 * kMaxScanBlocks nodes: the commit
// kernel scans its own 256 (flag, size) pairs in LDS and writes block-local prefixes plus one total per block; the
// list kernel turns the <= kMaxScanBlocks totals into global prefixes in LDS at its start.  Two launches instead of
// three, and no single-workgroup walk over the whole array.
constexpr int kMaxScanBlocks = 4096;

__global__ __launch_bounds__(256) void match_commit_scan_kernel(const int* __restrict__ prop, int N,
                                                                int* __restrict__ cluster, int* __restrict__ remaining,
                                                                int* __restrict__ final, int* __restrict__ lrank,
                                                                int* __restrict__ loffs, int* __restrict__ bt_rank,
                                                                int* __restrict__ bt_offs) {
  __shared__ int s_wave[4];
  const int u = blockIdx.x * 256 + threadIdx.x;
  int rep = 0, size = 0;
  if (u < N) {
    int st = cluster[u];
    if (st < 0) {
      int v = prop[u];
      if (v == -1) st = u;
      else if (v >= 0 && prop[v] == u) st = v;
      else atomicAdd(remaining, 1);
      if (st >= 0) cluster[u] = st;
    }
    const int fin = st < 0 ? u : (u < st ? u : st);
    final[u] = fin;
    rep = fin == u ? 1 : 0;
    size = rep ? ((st >= 0 && st != u) ? 2 : 1) : 0;
  }
  int tr, to;
  const int pr = block_exclusive_scan<4>(rep, s_wave, tr);
  const int po = block_exclusive_scan<4>(size, s_wave, to);
  if (u < N) { lrank[u] = pr; loffs[u] = po; }
  if (threadIdx.x == 0) { bt_rank[blockIdx.x] = tr; bt_offs[blockIdx.x] = to; }
}

__global__ __launch_bounds__(256) void match_lists_scan_kernel(const int* __restrict__ state, const int* __restrict__ final,
                                                               const int* __restrict__ lrank, const int* __restrict__ loffs,
                                                               const int* __restrict__ bt_rank, const int* __restrict__ bt_offs,
                                                               int nblocks, int N, int* __restrict__ cnew,
                                                               int* __restrict__ count, int* __restrict__ segptr,
                                                               int* __restrict__ members, const int* __restrict__ rowptr,
                                                               int4* __restrict__ rowinfo) {
  // exclusive prefixes of the block totals (every block recomputes them: <= 4096 ints, L2-resident)
  __shared__ int s_rank[kMaxScanBlocks], s_offs[kMaxScanBlocks];
  __shared__ int s_wave[4];
  __shared__ int s_total[2];
  int carry_r = 0, carry_o = 0;
  for (int base = 0; base < nblocks; base += 256) {
    const int i = base + threadIdx.x;
    const int vr = i < nblocks ? bt_rank[i] : 0, vo = i < nblocks ? bt_offs[i] : 0;
    int tr, to;
    const int pr = block_exclusive_scan<4>(vr, s_wave, tr);
    const int po = block_exclusive_scan<4>(vo, s_wave, to);
    if (i < nblocks) { s_rank[i] = carry_r + pr; s_offs[i] = carry_o + po; }
    carry_r += tr; carry_o += to;
  }
  if (threadIdx.x == 0) { s_total[0] = carry_r; s_total[1] = carry_o; }
  __syncthreads();
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= N) return;
  const int rep = final[u];
  cnew[u] = s_rank[rep >> 8] + lrank[rep];
  if (rep == u) {
    const int o = s_offs[u >> 8] + loffs[u];
    const int cid = s_rank[u >> 8] + lrank[u];
    segptr[cid] = o;
    members[o] = u;
    const int st = state[u];
    const bool pair = st >= 0 && st != u;
    if (pair) members[o + 1] = st;
    if (rowinfo != nullptr) {
      // the members' rows of the matched graph, for the edge coarsening behind this call (it would otherwise walk
      // segptr -> members -> rowptr, three dependent loads per coarse node)
      const int r0 = rowptr[u], d0 = rowptr[u + 1] - r0;
      const int r1 = pair ? rowptr[st] : 0, d1 = pair ? rowptr[st + 1] - r1 : 0;
      rowinfo[cid] = make_int4(r0, d0, r1, d1);
    }
  }
  if (u == N - 1) {
    const int nc = s_total[0];
    *count = nc;
    segptr[nc] = N;
  }
}

__global__ void match_finish_kernel(int N, const int* __restrict__ state, int* __restrict__ cluster) {
  int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u < N) { int c = state[u]; cluster[u] = c < 0 ? u : (u < c ? u : c); }
}

// ----------------------------------------------------------------------------- relabel
// clusterings whose ids are member indices with cluster[id] == id (graclus: id = min member): no scatter
__global__ void rep_self_flag_kernel(const int* __restrict__ cluster, int N, int* __restrict__ flag) {
  int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u < N) flag[u] = cluster[u] == u ? 1 : 0;
}

__global__ void rep_flag_kernel(const int* __restrict__ cluster, int N, int* __restrict__ flag) {
  // flag every id that occurs (benign race: all writers store 1); ids must lie in [0, N)
  int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u < N) flag[cluster[u]] = 1;
}

__global__ void relabel_apply_kernel(const int* __restrict__ cluster, const int* __restrict__ flag,
                                     const int* __restrict__ rank, int N, int* __restrict__ cnew,
                                     int* __restrict__ count) {
  int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= N) return;
  cnew[u] = rank[cluster[u]];
  if (u == N - 1) *count = rank[u] + flag[u];
}

}  // namespace

int edge_weight_t10(const float* x, int C, const int32_t* row, const int32_t* col, const float* w_in, int64_t E,
                    float* w_out, hipStream_t s, int32_t* zero8) {
  if (E <= 0) return 0;
  edge_weight_t10_kernel<<<cdiv(E * 8, 256), 256, 0, s>>>(x, C, row, col, w_in, E, w_out, zero8);
  GEOBI_LAUNCH_OK();
  return 0;
}

// `rounds` proposal rounds; the first one initialises the state (init != 0) and the undecided counter.
// On return pp holds the proposals of the last round.
// Test hook (geobi_set_match_round_cap): at most cap x (rounds / 8) rounds per call.  The callers ask for 8 rounds and
// double the number on every resume of their repair loops; a cap of 1 makes those 1, 2, 4, ... -- every pooling step then
// comes back with undecided nodes and is resumed, which an uncapped mesh graph almost never needs.
static Knob g_round_cap{nullptr, 0};

static void launch_match_rounds(const int32_t* rowptr, const int32_t* col, const float* w, int N, int rounds, int init,
                                int32_t* cluster, int32_t* status, int*& pp, int*& pn, hipStream_t s) {
  const int blocks = cdiv(N, 256);
  if (const int64_t cap = g_round_cap.get(); cap > 0) {
    const int64_t capped = cap * (rounds > 8 ? rounds / 8 : 1);
    if (capped < rounds) rounds = (int)capped;
  }
  for (int r = 0; r < rounds; ++r) {
    if (r > 0)
      match_round_kernel<0><<<blocks, 256, 0, s>>>(rowptr, col, w, pp, N, cluster, pn, status);
    else if (init)
      match_round_kernel<1><<<blocks, 256, 0, s>>>(rowptr, col, w, pp, N, cluster, pn, status);
    else
      match_round_kernel<2><<<blocks, 256, 0, s>>>(rowptr, col, w, pp, N, cluster, pn, status);
    int* t = pp; pp = pn; pn = t;
  }
}

namespace {
struct MatchBuffers { int *prop0, *prop1; };            // the proposals, ping-pong
struct CoarsenBuffers { MatchBuffers m; int *flag, *sz, *rank, *offs; IntScan scan_a, scan_b; };
MatchBuffers carve_match(Arena& a, int64_t N) { return {a.take<int>(N), a.take<int>(N)}; }
CoarsenBuffers carve_match_coarsen(Arena& a, int64_t N) {
  return {carve_match(a, N), a.take<int>(N + 1), a.take<int>(N + 1), a.take<int>(N + 1), a.take<int>(N + 1),
          IntScan::take(a, N + 1), IntScan::take(a, N + 1)};
}
struct RelabelBuffers { CountScan flag; int* rank; };
RelabelBuffers carve_relabel(Arena& a, int64_t N) { return {carve_count_scan(a, N), a.take<int>(N)}; }
}  // namespace

size_t match_coarsen_ws_bytes(int64_t N) { return carve_bytes([&](Arena& a) { carve_match_coarsen(a, N); }); }

// One pooling step's integer front end in one call: matching rounds, commit, dense relabel and the inverse
// lists of the matching (what geobi_match_heavy_edge + geobi_relabel_compact + geobi_segment_csr_pairs
// produce, 6 launches fewer).  counters[0] = undecided nodes, counters[1] = coarse node count.
int match_coarsen(const int32_t* rowptr, const int32_t* col, const float* w, int64_t N, int rounds, int init,
                  int32_t* state, int32_t* cluster_final, int32_t* cnew, int32_t* segptr, int32_t* members,
                  int32_t* counters, void* ws, size_t ws_bytes, hipStream_t s, void* rowinfo_out, bool* rowinfo_made) {
  GEOBI_REQUIRE(N > 0 && rounds > 0, "match_coarsen: empty graph or no rounds");
  Arena a(ws, ws_bytes);
  const CoarsenBuffers b = carve_match_coarsen(a, N);
  GEOBI_WS_CHECK("match_coarsen", a, ws, ws_bytes);
  int *flag = b.flag, *sz = b.sz, *rank = b.rank, *offs = b.offs;
  const int blocks = cdiv(N, 256);
  int* pp = b.m.prop0;
  int* pn = b.m.prop1;
  launch_match_rounds(rowptr, col, w, (int)N, rounds, init, state, counters, pp, pn, s);
  const bool scan_free = g_match_scanfree.on();
  if (scan_free && blocks <= kMaxScanBlocks) {
    // scan-free pair: block-local prefixes in the commit kernel, block totals folded by the list kernel
    int* bt_rank = rank;                 // rank / offs are free in this variant: reuse them for the block totals
    int* bt_offs = offs;
    prof_begin(PROF_POOL_FORM, s, 0.0, POOL_FORM_MATCH_SCANFREE);
    match_commit_scan_kernel<<<blocks, 256, 0, s>>>(pp, (int)N, state, counters, cluster_final, flag, sz, bt_rank, bt_offs);
    GEOBI_LAUNCH_OK();
    match_lists_scan_kernel<<<blocks, 256, 0, s>>>(state, cluster_final, flag, sz, bt_rank, bt_offs, blocks, (int)N, cnew,
                                                   counters + 1, segptr, members, rowptr, (int4*)rowinfo_out);
    prof_end(PROF_POOL_FORM, s);
    GEOBI_LAUNCH_OK();
    if (rowinfo_made) *rowinfo_made = rowinfo_out != nullptr;
    return 0;
  }
  if (rowinfo_made) *rowinfo_made = false;
  match_commit_kernel<<<blocks, 256, 0, s>>>(pp, (int)N, state, counters, cluster_final, flag, sz);
  GEOBI_LAUNCH_OK();
  if (N + 1 <= kSmallScan) {
    prof_begin(PROF_POOL_FORM, s, 0.0, POOL_FORM_MATCH_TWOPASS_DUAL);
    const int rc = scan_exclusive_i32_pair(flag, sz, rank, offs, N + 1, s);
    prof_end(PROF_POOL_FORM, s);
    GEOBI_TRY(rc);
  } else {
    GEOBI_TRY(b.scan_a.run(flag, rank, s));
    GEOBI_TRY(b.scan_b.run(sz, offs, s));
  }
  match_lists_kernel<<<blocks, 256, 0, s>>>(state, cluster_final, rank, offs, (int)N, cnew, counters + 1, segptr,
                                            members);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // namespace geobi

using namespace geobi;

extern "C" {

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
  hipStream_t s = as_stream(stream);
  if (E <= 0 || N <= 0) return 0;
  if (C <= 0) return set_error("edge_weight_att: C = %d", C);
  node_att_kernel<<<cdiv(N * 8, 256), 256, 0, s>>>(x, C, att_l, att_r, N, reinterpret_cast<float2*>(node_ws));
  GEOBI_LAUNCH_OK();
  edge_weight_att_kernel<<<cdiv(E, 256), 256, 0, s>>>(reinterpret_cast<const float2*>(node_ws), row, col, w_in, E, w_out);
  GEOBI_LAUNCH_OK();
  return 0;
}

size_t geobi_match_ws_bytes(int64_t N) { return carve_bytes([&](Arena& a) { carve_match(a, N); }); }

// Runs `rounds` proposal rounds.  init != 0 starts from scratch, init == 0 continues from the state
// in `cluster` (entries < 0 = undecided).  `status[0]` receives the number of nodes still undecided
// after the last round (0 = converged).  `cluster` keeps the resumable state; `cluster_final`
// (optional) receives a copy with undecided nodes closed as singletons, i.e. always a valid clustering.
int geobi_match_heavy_edge(const int32_t* rowptr, const int32_t* col, const float* w, int64_t N, int rounds,
                           int init, int32_t* cluster, int32_t* cluster_final, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(N, 0);
  GEOBI_NOTNULL(rowptr); GEOBI_NOTNULL(cluster); GEOBI_NOTNULL(status);
  hipStream_t s = as_stream(stream);
  GEOBI_REQUIRE(N > 0 && rounds > 0, "match: empty graph or no rounds");
  Arena a(ws, ws_bytes);
  const MatchBuffers m = carve_match(a, N);
  GEOBI_WS_CHECK("match_heavy_edge", a, ws, ws_bytes);
  int blocks = cdiv(N, 256);
  int* pp = m.prop0;
  int* pn = m.prop1;
  launch_match_rounds(rowptr, col, w, (int)N, rounds, init, cluster, status, pp, pn, s);
  match_commit_kernel<<<blocks, 256, 0, s>>>(pp, (int)N, cluster, status, cluster_final, nullptr, nullptr);
  GEOBI_LAUNCH_OK();
  return 0;
}

int geobi_set_match_round_cap(int cap) { g_round_cap.set(cap > 0 ? cap : 0); return 0; }

// Test hook: 1 / 0 force the form, a negative value goes back to what the environment says.  Without a call nothing changes.
int geobi_set_match_scanfree(int on) {
  if (on < 0) g_match_scanfree.reset(); else g_match_scanfree.set(on != 0);
  return 0;
}

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

size_t geobi_relabel_ws_bytes(int64_t N) { return carve_bytes([&](Arena& a) { carve_relabel(a, N); }); }

int geobi_relabel_compact(const int32_t* cluster, int64_t N, int rep_is_self, int32_t* cnew, int32_t* count,
                          void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(N, 0);
  GEOBI_NOTNULL(cluster); GEOBI_NOTNULL(cnew); GEOBI_NOTNULL(count);
  hipStream_t s = as_stream(stream);
  GEOBI_REQUIRE(N > 0, "relabel: empty");
  Arena a(ws, ws_bytes);
  const RelabelBuffers b = carve_relabel(a, N);
  GEOBI_WS_CHECK("relabel_compact", a, ws, ws_bytes);
  int *flag = b.flag.cnt, *rank = b.rank;
  int blocks = cdiv(N, 256);
  if (rep_is_self) {
    rep_self_flag_kernel<<<blocks, 256, 0, s>>>(cluster, (int)N, flag);
  } else {
    GEOBI_HIP(hipMemsetAsync(flag, 0, sizeof(int) * N, s));
    rep_flag_kernel<<<blocks, 256, 0, s>>>(cluster, (int)N, flag);
  }
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(b.flag.scan.run(flag, rank, s));
  relabel_apply_kernel<<<blocks, 256, 0, s>>>(cluster, flag, rank, (int)N, cnew, count);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // extern "C"
