// Graph pooling / unpooling kernels (PoolingLayer of the hot path,
// /root/reference/code/net_util.py:56-245, and pool_edge :289-295).
//
//   edge_weight_t10   w_e += exp(-|x_i - x_j|^2 / 2)                       (net_util.py:226-230)
//   match_*           heavy-edge matching, cluster id = min(u, v)          (graclus, net_util.py:127)
//   relabel           dense ids by rank of the representative              (consecutive_cluster, :128)
//   segment_csr       inverse lists  cluster -> members  (sorted, deterministic)
//   segment_max/mean  feature pooling with arg-max for the backward        (scatter, :131-134)
//   segment_sum       unpool backward (gather forward = `x[unpooling_indices]`, :242-245)
//   pool_edge         relabel endpoints, drop loops, sort, merge duplicates by mean  (:289-295)
//
// Matching specification (deterministic, unlike torch_cluster's randomised orders): an edge is
// taken iff it is the best remaining edge at BOTH endpoints under the total order
// (weight desc, min(u,v) asc, max(u,v) asc) -- i.e. greedy matching in globally descending edge
// order, computed by rounds of mutual proposals.  oracle/oracle_c.c:oracle_greedy_sorted is the
// sequential statement of the same rule.
//
// The count-to-offset scans of these steps are IntScan records (device_steps.h) and scan_exclusive_i32_pair; their
// kernels live in scan.hip.  Only the scan-free matching pair scans in place, with block_scan.h.
#include "block_scan.h"
#include "common.h"
#include "device_steps.h"

#include <atomic>
#include <cstdlib>
#include <cstring>

namespace geobi {

namespace {

constexpr uint64_t kSentinel = ~0ull;

// A/B knob with a test hook: the environment decides (unset or non-zero = on) until geobi_set_match_scanfree forces a form
Knob g_match_scanfree{"GEOBI_MATCH_SCANFREE", 1};

static inline int key_bits(int64_t N) {   // (1 << bits) > N: see graph.hip
  int b = 1;
  while ((1ll << b) <= N) ++b;
  return b;
}

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

// ------------------------------------------------------------------------ inverse lists
__global__ void seg_keys_kernel(const int* __restrict__ seg, int64_t n, int bits, uint64_t* __restrict__ keys) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) keys[i] = ((uint64_t)(uint32_t)seg[i] << bits) | (uint64_t)(uint32_t)i;
}

__global__ void seg_unpack_kernel(const uint64_t* __restrict__ keys, int64_t n, int bits,
                                  int* __restrict__ members) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) members[i] = (int)(uint32_t)(keys[i] & ((1ull << bits) - 1));
}

__global__ void seg_ptr_kernel(const uint64_t* __restrict__ keys, int64_t n, int nseg, int bits,
                               int* __restrict__ segptr) {
  int sidx = blockIdx.x * blockDim.x + threadIdx.x;
  if (sidx > nseg) return;
  uint64_t target = (uint64_t)sidx << bits;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < target) lo = mid + 1; else hi = mid;
  }
  segptr[sidx] = (int)lo;
}

// Inverse lists of a MATCHING (clusters of <= 2 nodes, raw id = smaller member, cnew = dense id):
// no sort needed -- the representative takes slot 0, its partner slot 1 (members stay ascending).
__global__ void pair_count_kernel(const int* __restrict__ cnew, const int* __restrict__ raw, int N, int nseg,
                                  int* __restrict__ cnt) {
  int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u < nseg) cnt[u] = 1;              // pass 1 of 2 (see launcher): every cluster has its representative
  (void)cnew; (void)raw; (void)N;
}

__global__ void pair_mark_kernel(const int* __restrict__ cnew, const int* __restrict__ raw, int N,
                                 int* __restrict__ cnt) {
  int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u < N && raw[u] != u) cnt[cnew[u]] = 2;       // exactly one writer per matched cluster
}

__global__ void pair_fill_kernel(const int* __restrict__ cnew, const int* __restrict__ raw, int N, int nseg,
                                 int* __restrict__ segptr, int* __restrict__ members) {
  int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u == 0) segptr[nseg] = N;
  if (u < N) members[segptr[cnew[u]] + (raw[u] == u ? 0 : 1)] = u;
}

// Inverse lists of a composition  fine --(idx1)--> mid --(idx2)--> coarse :
// members12(C) = concat over m in members2(C) of members1(m)   (fixed order -> deterministic sums)
__global__ void compose_count_kernel(const int* __restrict__ segptr1, const int* __restrict__ segptr2,
                                     const int* __restrict__ members2, int nseg2, int* __restrict__ cnt) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nseg2) return;
  int n = 0;
  for (int e = segptr2[c]; e < segptr2[c + 1]; ++e) { int m = members2[e]; n += segptr1[m + 1] - segptr1[m]; }
  cnt[c] = n;
}

__global__ void compose_fill_kernel(const int* __restrict__ segptr1, const int* __restrict__ members1,
                                    const int* __restrict__ segptr2, const int* __restrict__ members2, int nseg2,
                                    int n_fine, int* __restrict__ segptr12, int* __restrict__ members12) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0) segptr12[nseg2] = n_fine;
  if (c >= nseg2) return;
  int o = segptr12[c];
  for (int e = segptr2[c]; e < segptr2[c + 1]; ++e) {
    int m = members2[e];
    for (int f = segptr1[m]; f < segptr1[m + 1]; ++f) members12[o++] = members1[f];
  }
}

// ----------------------------------------------------------------------- segment reduce
__global__ void segment_max_fwd_kernel(const float* __restrict__ x, int C, const int* __restrict__ segptr,
                                       const int* __restrict__ members, int nseg, float* __restrict__ out,
                                       int* __restrict__ arg) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nseg * C) return;
  int sidx = (int)(t / C), c = (int)(t % C);
  int rs = segptr[sidx], re = segptr[sidx + 1];
  float best = 0.f;          // empty segment -> 0 (torch_scatter fills untouched rows with 0)
  int bi = -1;
  for (int e = rs; e < re; ++e) {
    int m = members[e];      // members ascend, strict '>' keeps the first maximum
    float v = x[(size_t)m * C + c];
    if (bi < 0 || v > best) { best = v; bi = m; }
  }
  out[t] = best;
  arg[t] = bi;
}

// Max over the composition of two clusterings (a pooling layer's two matching steps) in ONE pass: segment c of the
// second step = concatenation, in order, of the first-step segments of its members.  The running maximum keeps the
// first maximum in that order -- the element the two-step form (max of the step-one maxima, first maximum at each
// step) routes to -- so out and the backward's routing are identical to two segment_max passes; the step-one
// maxima are never materialised.  arg12 holds the FINE row of the maximum.
__global__ void segment_max2_fwd_kernel(const float* __restrict__ x, int C, const int* __restrict__ segptr1,
                                        const int* __restrict__ members1, const int* __restrict__ segptr2,
                                        const int* __restrict__ members2, int nseg2, float* __restrict__ out,
                                        int* __restrict__ arg12) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nseg2 * C) return;
  const int sidx = (int)(t / C), c = (int)(t % C);
  float best = 0.f;
  int bi = -1;
  for (int e2 = segptr2[sidx]; e2 < segptr2[sidx + 1]; ++e2) {
    const int m = members2[e2];
    float mb = 0.f;                               // the step-one maximum of segment m and its first position
    int mi = -1;
    for (int e1 = segptr1[m]; e1 < segptr1[m + 1]; ++e1) {
      const int f = members1[e1];
      const float v = x[(size_t)f * C + c];
      if (mi < 0 || v > mb) { mb = v; mi = f; }
    }
    if (mi >= 0 && (bi < 0 || mb > best)) { best = mb; bi = mi; }
  }
  out[t] = best;
  arg12[t] = bi;
}

// gather form of its backward: fine row n receives the gradient of its composed segment where it was the arg-max
__global__ void segment_max2_bwd_kernel(const float* __restrict__ gout, const int* __restrict__ arg12,
                                        const int* __restrict__ seg12, int C, int64_t total, int nseg2,
                                        float* __restrict__ gx, int add) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int n = (int)(t / C), c = (int)(t % C);
  const int sg = seg12[n];
  float v = 0.f;
  if (sg >= 0 && sg < nseg2) {
    const size_t o = (size_t)sg * C + c;
    if (arg12[o] == n) v = gout[o];
  }
  gx[t] = add ? gx[t] + v : v;                  // add: on top of what gx holds (a skip connection's gradient)
}

// gather form: fine row n receives the gradient of its segment where it was the arg-max (every
// element of gx is written exactly once -> no zero-fill pass)
__global__ void segment_max_bwd_kernel(const float* __restrict__ gout, const int* __restrict__ arg,
                                       const int* __restrict__ seg, int C, int64_t total, int nseg,
                                       float* __restrict__ gx) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  int n = (int)(t / C), c = (int)(t % C);
  int sg = seg[n];
  float v = 0.f;
  if (sg >= 0 && sg < nseg) {
    size_t o = (size_t)sg * C + c;
    if (arg[o] == n) v = gout[o];
  }
  gx[t] = v;
}

__global__ void segment_sum_kernel(const float* __restrict__ x, int C, const int* __restrict__ segptr,
                                   const int* __restrict__ members, int nseg, int mean, float* __restrict__ out) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nseg * C) return;
  int sidx = (int)(t / C), c = (int)(t % C);
  int rs = segptr[sidx], re = segptr[sidx + 1];
  float s = 0.f;
  for (int e = rs; e < re; ++e) s += x[(size_t)members[e] * C + c];
  if (mean) s = s / (float)max(re - rs, 1);
  out[t] = s;
}

// Sum over the composition of two clusterings, the members walked in the order the composed list (compose_fill_kernel)
// would hold them -- same sums bit for bit, without building that list.
__global__ void segment_sum2_kernel(const float* __restrict__ x, int C, const int* __restrict__ segptr1,
                                    const int* __restrict__ members1, const int* __restrict__ segptr2,
                                    const int* __restrict__ members2, int nseg2, float* __restrict__ out) {
  // four channels per thread (16-B loads; C is 64 or 128 on the path), same summation order per channel as before
  const int Q = C >> 2;
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nseg2 * Q) return;
  const int sidx = (int)(t / Q), c = (int)(t % Q) * 4;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int e2 = segptr2[sidx]; e2 < segptr2[sidx + 1]; ++e2) {
    const int m = members2[e2];
    for (int e1 = segptr1[m]; e1 < segptr1[m + 1]; ++e1) {
      const float4 v = *reinterpret_cast<const float4*>(x + (size_t)members1[e1] * C + c);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  *reinterpret_cast<float4*>(out + (size_t)sidx * C + c) = s;
}

__global__ void segment_mean_bwd_kernel(const float* __restrict__ gout, const int* __restrict__ seg,
                                        const int* __restrict__ segptr, int C, int64_t total,
                                        float* __restrict__ gx) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  int n = (int)(t / C), c = (int)(t % C);
  int sidx = seg[n];
  gx[t] = gout[(size_t)sidx * C + c] / (float)max(segptr[sidx + 1] - segptr[sidx], 1);
}

__global__ void gather_rows_kernel(const float* __restrict__ x, const int* __restrict__ idx, int C, int64_t total,
                                   float* __restrict__ out) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  int n = (int)(t / C), c = (int)(t % C);
  out[t] = x[(size_t)idx[n] * C + c];
}

// ---------------------------------------------------------------------------- pool_edge
__global__ void pool_edge_keys_kernel(const int* __restrict__ cnew, const int* __restrict__ row,
                                      const int* __restrict__ col, int64_t E, int bits,
                                      uint64_t* __restrict__ keys, int* __restrict__ vals) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  int a = cnew[row[e]], b = cnew[col[e]];
  keys[e] = (a == b) ? kSentinel : (((uint64_t)(uint32_t)a << bits) | (uint64_t)(uint32_t)b);
  vals[e] = (int)e;
}

__global__ void pool_edge_heads_kernel(const uint64_t* __restrict__ keys, int64_t E, int* __restrict__ head) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  uint64_t k = keys[e];
  head[e] = (k != kSentinel && (e == 0 || keys[e - 1] != k)) ? 1 : 0;
}

__global__ void pool_edge_emit_kernel(const uint64_t* __restrict__ keys, const int* __restrict__ vals,
                                      const int* __restrict__ head, const int* __restrict__ rank,
                                      const float* __restrict__ w, int64_t E, int* __restrict__ row_c,
                                      int* __restrict__ col_c, float* __restrict__ w_c, uint64_t* __restrict__ ukeys,
                                      int* __restrict__ count, int bits) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  if (e == E - 1) *count = rank[e] + head[e];
  if (!head[e]) return;
  uint64_t k = keys[e];
  int o = rank[e];
  row_c[o] = (int)(uint32_t)(k >> bits);
  col_c[o] = (int)(uint32_t)(k & ((1ull << bits) - 1));
  ukeys[o] = k;
  if (w) {
    // mean of the merged duplicates; fp64 accumulation makes the result independent of the
    // order of the run, so w(a,b) == w(b,a) bit for bit and the matching stays symmetric
    double s = 0.0;
    int n = 0;
    for (int64_t f = e; f < E && keys[f] == k; ++f) { s += (double)w[vals[f]]; ++n; }
    w_c[o] = (float)(s / (double)n);
  }
}

// ---------------------------------------------------------- pool_edge, sort-free (matchings)
// For a matching every coarse node has 1-2 members, so its coarse row is the union of at most two
// fine rows: one wave per coarse node gathers those (<= 64) entries, relabels them, sorts them with a
// 64-lane bitonic network, drops the self entry and merges duplicates -- no global radix sort.
// PASS 0 counts the unique neighbours (-> exclusive scan -> rowptr), PASS 1 repeats and writes.
// Rows with more than 64 gathered entries set `overflow` (the caller falls back to the sorted path).
template <int PASS>
__global__ __launch_bounds__(256) void pool_edge_rows_kernel(
    const int* __restrict__ cnew, const int* __restrict__ segptr, const int* __restrict__ members,
    const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ w,
    const int* __restrict__ ncount, int nbound, int* __restrict__ cnt, const int* __restrict__ rowptr_c,
    int* __restrict__ row_c, int* __restrict__ col_c, float* __restrict__ w_c, int* __restrict__ overflow,
    int* __restrict__ total, int4* __restrict__ rowinfo, const int4* __restrict__ rowinfo_in) {
  const int lane = threadIdx.x & 63;
  const int A = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (PASS != 1 && blockIdx.x == 0 && threadIdx.x == 0) cnt[nbound] = 0;     // scan tail: rowptr_c[nbound] = total
  if (PASS == 1 && blockIdx.x == 0 && threadIdx.x == 0) *total = rowptr_c[nbound];
  if (A >= nbound) return;
  // requested before the coarse count is known (entries past it are never read back): one dependent load less
  int4 ri_in = make_int4(0, 0, 0, 0);
  if (PASS == 2 && rowinfo_in != nullptr) ri_in = rowinfo_in[A];
  const int nc = *ncount;
  if (A >= nc) { if (PASS != 1) cnt[A] = 0; return; }
  // the members' fine rows: PASS 0 walks segptr -> members -> rowptr (three dependent loads) and leaves the result
  // for PASS 1, whose chain then starts at the row entries
  int r0, d0, r1, d1;
  if (PASS == 2 && rowinfo_in != nullptr) {
    const int4 ri = ri_in;
    r0 = ri.x; d0 = ri.y; r1 = ri.z; d1 = ri.w;
    if (lane == 0) {
      rowinfo[A] = ri;
      if (d0 + d1 > 64) atomicOr(overflow, 1);
    }
  } else if (PASS != 1) {
    const int ms = segptr[A], me = segptr[A + 1];
    const int m0 = members[ms];
    const int m1 = (me - ms > 1) ? members[ms + 1] : -1;
    r0 = rowptr[m0]; d0 = rowptr[m0 + 1] - r0;
    r1 = m1 >= 0 ? rowptr[m1] : 0; d1 = m1 >= 0 ? rowptr[m1 + 1] - r1 : 0;
    if (lane == 0) {
      rowinfo[A] = make_int4(r0, d0, r1, d1);
      if (d0 + d1 > 64 || me - ms > 2) atomicOr(overflow, 1);
    }
  } else {
    const int4 ri = rowinfo[A];
    r0 = ri.x; d0 = ri.y; r1 = ri.z; d1 = ri.w;
  }
  int key = 0x7fffffff;
  float val = 0.f;
  if (lane < d0 + d1) {
    const int e = lane < d0 ? r0 + lane : r1 + (lane - d0);
    int k = cnew[col[e]];
    if (k != A) { key = k; val = w ? w[e] : 0.f; }
  }
  // bitonic sort, ascending by key; rows of up to 32 entries (the usual case: two mesh rows) skip the 64-wide merge.
  // Partner exchange at distance 1, 2, 4, 8 by DPP lane permutes (quad_perm, row_shl/shr:4, row_ror:8) -- 14 of the 15
  // stages of the 32-wide sort; a wave is a chain of ~20 dependent exchanges, and an LDS-crossbar permute costs ~10x
  // a DPP move in latency.  Every lane of the wave is active here (waves past the coarse count left as a whole).
  auto xchg = [&](int v, int j) -> int {
    switch (j) {
      case 1: return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true);          // quad_perm [1,0,3,2]
      case 2: return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true);          // quad_perm [2,3,0,1]
      case 4: {
        const int up = __builtin_amdgcn_update_dpp(0, v, 0x104, 0xf, 0xf, true);       // row_shl:4  lane i <- i + 4
        const int dn = __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);       // row_shr:4  lane i <- i - 4
        return (lane & 4) ? dn : up;
      }
      case 8: return __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, true);          // row_ror:8 = xor 8 in a row
      default: return __shfl_xor(v, j, 64);
    }
  };
  auto stage = [&](int k, int j) {
    const int pk = xchg(key, j);
    const float pv = __int_as_float(xchg(__float_as_int(val), j));
    const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
    const bool take = keep_min ? (pk < key) : (pk > key);
    if (take) { key = pk; val = pv; }
  };
#pragma unroll
  for (int k = 2; k <= 32; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) stage(k, j);
  }
  if (d0 + d1 > 32) {                            // wave-uniform
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) stage(64, j);
  }
  const int prev = __shfl_up(key, 1, 64);
  const bool head = key != 0x7fffffff && (lane == 0 || prev != key);
  const unsigned long long hm = __ballot(head);
  if (PASS == 0) {
    if (lane == 0) cnt[A] = __popcll(hm);
    return;
  }
  if (PASS == 2 && lane == 0) cnt[A] = __popcll(hm);
  // run of duplicates starting at a head lane: up to the next head (or the first invalid lane)
  const unsigned long long vm = __ballot(key != 0x7fffffff);
  const int nvalid = __popcll(vm);
  const unsigned long long after = (lane >= 63) ? 0ull : (hm >> (lane + 1));
  const int next = after ? lane + 1 + (__ffsll((long long)after) - 1) : nvalid;
  const int len = head ? next - lane : 0;
  int maxlen = len;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) maxlen = max(maxlen, __shfl_xor(maxlen, m, 64));
  double sum = (double)val;
  for (int t = 1; t < maxlen; ++t) {
    float v = __shfl_down(val, t, 64);
    if (t < len) sum += (double)v;
  }
  if (head) {
    const int t = __popcll(hm & ((1ull << lane) - 1ull));
    if (PASS == 2) {
      // one-pass form: the t-th unique entry parks in the t-th slot of the members' own fine rows (there are at most
      // d0 + d1 of them); pool_edge_compact_kernel moves the rows to their final places once the offsets are known
      const int pos = t < d0 ? r0 + t : r1 + (t - d0);
      col_c[pos] = key;                          // (col_c / w_c are the scratch pair here)
      if (w) w_c[pos] = (float)(sum / (double)len);
    } else {
      const int pos = rowptr_c[A] + t;
      row_c[pos] = A;
      col_c[pos] = key;
      if (w) w_c[pos] = (float)(sum / (double)len);
    }
  }
}

// second half of the one-pass form: 16 lanes per coarse node copy its parked entries to rowptr_c[A] ...
__global__ __launch_bounds__(256) void pool_edge_compact_kernel(const int* __restrict__ ncount, int nbound,
                                                                const int* __restrict__ rowptr_c,
                                                                const int4* __restrict__ rowinfo,
                                                                const int* __restrict__ tcol, const float* __restrict__ tw,
                                                                int* __restrict__ row_c, int* __restrict__ col_c,
                                                                float* __restrict__ w_c, int* __restrict__ total,
                                                                const int* publish_src, int* publish_host, int publish_seq) {
  const int A = (blockIdx.x * 256 + threadIdx.x) >> 4, k = threadIdx.x & 15;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int tot = rowptr_c[nbound];
    *total = tot;
    if (publish_host != nullptr) {
      // The sizes the host is waiting for are all final once this kernel has started (its own total included):
      // thread 0 hands them over through mapped host memory right away -- the host learns them while the copy pass
      // below is still running, without a device-to-host copy launch and a stream drain in between.
      for (int i = 0; i < 8; ++i) {
        const int* src = publish_src + i;
        publish_host[i] = (src == total) ? tot : *src;
      }
      __threadfence_system();
      __hip_atomic_store(publish_host + 8, publish_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  if (A >= nbound || A >= *ncount) return;
  const int o = rowptr_c[A], c = rowptr_c[A + 1] - o;
  const int4 ri = rowinfo[A];
  for (int t = k; t < c; t += 16) {
    const int src = t < ri.y ? ri.x + t : ri.z + (t - ri.y);
    row_c[o + t] = A;
    col_c[o + t] = tcol[src];
    if (tw) w_c[o + t] = tw[src];
  }
}

__global__ void pool_edge_rowptr_kernel(const uint64_t* __restrict__ ukeys, const int* __restrict__ count, int nmax,
                                        int bits, int* __restrict__ rowptr) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n > nmax) return;
  uint64_t target = (uint64_t)n << bits;
  int lo = 0, hi = *count;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (ukeys[mid] < target) lo = mid + 1; else hi = mid;
  }
  rowptr[n] = lo;
}

__global__ void expand_rowptr_kernel(const int* __restrict__ rowptr, int N, int* __restrict__ row) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  for (int e = rowptr[n]; e < rowptr[n + 1]; ++e) row[e] = n;
}

__global__ void gather_f32_kernel(const float* __restrict__ src, const int* __restrict__ idx, int64_t n,
                                  float* __restrict__ dst) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { int k = idx[i]; dst[i] = k >= 0 ? src[k] : 0.f; }
}

}  // namespace

int edge_weight_t10(const float* x, int C, const int32_t* row, const int32_t* col, const float* w_in, int64_t E,
                    float* w_out, hipStream_t s, int32_t* zero8) {
  if (E <= 0) return 0;
  edge_weight_t10_kernel<<<cdiv(E * 8, 256), 256, 0, s>>>(x, C, row, col, w_in, E, w_out, zero8);
  GEOBI_LAUNCH_OK();
  return 0;
}

int edge_weight_att(const float* x, int C, const float* att_l, const float* att_r, const int32_t* row, const int32_t* col,
                    const float* w_in, int64_t N, int64_t E, float* node_ws, float* w_out, hipStream_t s) {
  if (E <= 0 || N <= 0) return 0;
  if (C <= 0) return set_error("edge_weight_att: C = %d", C);
  node_att_kernel<<<cdiv(N * 8, 256), 256, 0, s>>>(x, C, att_l, att_r, N, reinterpret_cast<float2*>(node_ws));
  GEOBI_LAUNCH_OK();
  edge_weight_att_kernel<<<cdiv(E, 256), 256, 0, s>>>(reinterpret_cast<const float2*>(node_ws), row, col, w_in, E, w_out);
  GEOBI_LAUNCH_OK();
  return 0;
}

int gather_f32(const float* src, const int32_t* idx, int64_t n, float* dst, hipStream_t s) {
  if (n <= 0) return 0;
  gather_f32_kernel<<<cdiv(n, 256), 256, 0, s>>>(src, idx, n, dst);
  GEOBI_LAUNCH_OK();
  return 0;
}

int expand_rowptr(const int32_t* rowptr, int64_t N, int32_t* row, hipStream_t s) {
  if (N <= 0) return 0;
  expand_rowptr_kernel<<<cdiv(N, 256), 256, 0, s>>>(rowptr, (int)N, row);
  GEOBI_LAUNCH_OK();
  return 0;
}

// `rounds` proposal rounds; the first one initialises the state (init != 0) and the undecided counter.
// On return pp holds the proposals of the last round.
// Test hook (geobi_set_match_round_cap): at most cap x (rounds / 8) rounds per call.  The callers ask for 8 rounds and
// double the number on every resume of their repair loops; a cap of 1 makes those 1, 2, 4, ... -- every pooling step then
// comes back with undecided nodes and is resumed, which an uncapped mesh graph almost never needs.
static Knob g_round_cap{nullptr, 0};
void set_match_round_cap(int cap) { g_round_cap.set(cap > 0 ? cap : 0); }

// Test hook (geobi_set_match_scanfree): 1 / 0 force the form, a negative value goes back to what the environment says.
// Without a call nothing changes.
void set_match_scanfree(int on) { if (on < 0) g_match_scanfree.reset(); else g_match_scanfree.set(on != 0); }

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
// n counts (or flags) and the scan over them
struct CountScan { int* cnt; IntScan scan; };
CountScan carve_count_scan(Arena& a, int64_t n) { return {a.take<int>(n), IntScan::take(a, n)}; }
}  // namespace

size_t match_ws_bytes(int64_t N) { return carve_bytes([&](Arena& a) { carve_match(a, N); }); }

// Runs `rounds` proposal rounds.  init != 0 starts from scratch, init == 0 continues from the state
// in `cluster` (entries < 0 = undecided).  `status[0]` receives the number of nodes still undecided
// after the last round (0 = converged).  `cluster` keeps the resumable state; `cluster_final`
// (optional) receives a copy with undecided nodes closed as singletons, i.e. always a valid clustering.
int match_heavy_edge(const int32_t* rowptr, const int32_t* col, const float* w, int64_t N, int rounds, int init,
                     int32_t* cluster, int32_t* cluster_final, int32_t* status, void* ws, size_t ws_bytes,
                     hipStream_t s) {
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

namespace {
struct RelabelBuffers { CountScan flag; int* rank; };
RelabelBuffers carve_relabel(Arena& a, int64_t N) { return {carve_count_scan(a, N), a.take<int>(N)}; }
}  // namespace

size_t relabel_ws_bytes(int64_t N) { return carve_bytes([&](Arena& a) { carve_relabel(a, N); }); }

int relabel_compact(const int32_t* cluster, int64_t N, int rep_is_self, int32_t* cnew, int32_t* count, void* ws,
                    size_t ws_bytes, hipStream_t s) {
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

namespace {
struct KeySortBuffers { uint64_t *k_in, *k_out; KeySort<uint64_t> sort; };
KeySortBuffers carve_key_sort(Arena& a, int64_t n) {
  return {a.take<uint64_t>(n), a.take<uint64_t>(n), KeySort<uint64_t>::take(a, n)};
}
}  // namespace

size_t segment_csr_ws_bytes(int64_t n) { return carve_bytes([&](Arena& a) { carve_key_sort(a, n); }); }

int segment_csr(const int32_t* seg, int64_t n, int64_t nseg, int32_t* segptr, int32_t* members, void* ws,
                size_t ws_bytes, hipStream_t s) {
  if (n <= 0) {
    GEOBI_HIP(hipMemsetAsync(segptr, 0, sizeof(int) * (nseg + 1), s));
    return 0;
  }
  Arena a(ws, ws_bytes);
  const KeySortBuffers b = carve_key_sort(a, n);
  GEOBI_WS_CHECK("segment_csr", a, ws, ws_bytes);
  uint64_t *k_in = b.k_in, *k_out = b.k_out;
  const int bits = key_bits(n);                 // member index < n
  const int sbits = key_bits(nseg);
  seg_keys_kernel<<<cdiv(n, 256), 256, 0, s>>>(seg, n, bits, k_in);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(b.sort.run(k_in, k_out, n, (unsigned)(bits + sbits), s));
  seg_unpack_kernel<<<cdiv(n, 256), 256, 0, s>>>(k_out, n, bits, members);
  seg_ptr_kernel<<<cdiv(nseg + 1, 256), 256, 0, s>>>(k_out, n, (int)nseg, bits, segptr);
  GEOBI_LAUNCH_OK();
  return 0;
}

size_t segment_pairs_ws_bytes(int64_t nseg) { return carve_bytes([&](Arena& a) { carve_count_scan(a, nseg); }); }

int segment_csr_pairs(const int32_t* cnew, const int32_t* raw, int64_t N, int64_t nseg, int32_t* segptr,
                      int32_t* members, void* ws, size_t ws_bytes, hipStream_t s) {
  GEOBI_REQUIRE(N > 0 && nseg > 0, "segment_csr_pairs: empty");
  Arena a(ws, ws_bytes);
  const CountScan c = carve_count_scan(a, nseg);
  GEOBI_WS_CHECK("segment_csr_pairs", a, ws, ws_bytes);
  int* cnt = c.cnt;
  pair_count_kernel<<<cdiv(nseg, 256), 256, 0, s>>>(cnew, raw, (int)N, (int)nseg, cnt);
  pair_mark_kernel<<<cdiv(N, 256), 256, 0, s>>>(cnew, raw, (int)N, cnt);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(c.scan.run(cnt, segptr, s));
  pair_fill_kernel<<<cdiv(N, 256), 256, 0, s>>>(cnew, raw, (int)N, (int)nseg, segptr, members);
  GEOBI_LAUNCH_OK();
  return 0;
}

int segment_csr_compose(const int32_t* segptr1, const int32_t* members1, const int32_t* segptr2,
                        const int32_t* members2, int64_t nseg2, int64_t n_fine, int32_t* segptr12,
                        int32_t* members12, void* ws, size_t ws_bytes, hipStream_t s) {
  GEOBI_REQUIRE(nseg2 > 0, "segment_csr_compose: empty");
  Arena a(ws, ws_bytes);
  const CountScan c = carve_count_scan(a, nseg2);
  GEOBI_WS_CHECK("segment_csr_compose", a, ws, ws_bytes);
  int* cnt = c.cnt;
  compose_count_kernel<<<cdiv(nseg2, 256), 256, 0, s>>>(segptr1, segptr2, members2, (int)nseg2, cnt);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(c.scan.run(cnt, segptr12, s));
  compose_fill_kernel<<<cdiv(nseg2, 256), 256, 0, s>>>(segptr1, members1, segptr2, members2, (int)nseg2,
                                                       (int)n_fine, segptr12, members12);
  GEOBI_LAUNCH_OK();
  return 0;
}

int segment_max_fwd(const float* x, int C, const int32_t* segptr, const int32_t* members, int64_t nseg, float* out,
                    int32_t* arg, hipStream_t s) {
  if (nseg <= 0) return 0;
  segment_max_fwd_kernel<<<cdiv(nseg * C, 256), 256, 0, s>>>(x, C, segptr, members, (int)nseg, out, arg);
  GEOBI_LAUNCH_OK();
  return 0;
}

int segment_max_bwd(const float* gout, const int32_t* arg, const int32_t* seg, int C, int64_t nseg, int64_t n_fine,
                    float* gx, hipStream_t s) {
  if (n_fine <= 0) return 0;
  segment_max_bwd_kernel<<<cdiv(n_fine * C, 256), 256, 0, s>>>(gout, arg, seg, C, n_fine * C, (int)nseg, gx);
  GEOBI_LAUNCH_OK();
  return 0;
}

int segment_max2_fwd(const float* x, int C, const int32_t* segptr1, const int32_t* members1, const int32_t* segptr2,
                     const int32_t* members2, int64_t nseg2, float* out, int32_t* arg12, hipStream_t s) {
  if (nseg2 <= 0) return 0;
  segment_max2_fwd_kernel<<<cdiv(nseg2 * C, 256), 256, 0, s>>>(x, C, segptr1, members1, segptr2, members2, (int)nseg2, out,
                                                              arg12);
  GEOBI_LAUNCH_OK();
  return 0;
}

int segment_max2_bwd(const float* gout, const int32_t* arg12, const int32_t* seg12, int C, int64_t nseg2, int64_t n_fine,
                     float* gx, int add, hipStream_t s) {
  if (n_fine <= 0) return 0;
  segment_max2_bwd_kernel<<<cdiv(n_fine * C, 256), 256, 0, s>>>(gout, arg12, seg12, C, n_fine * C, (int)nseg2, gx, add);
  GEOBI_LAUNCH_OK();
  return 0;
}

int segment_sum(const float* x, int C, const int32_t* segptr, const int32_t* members, int64_t nseg, int mean,
                float* out, hipStream_t s) {
  if (nseg <= 0) return 0;
  segment_sum_kernel<<<cdiv(nseg * C, 256), 256, 0, s>>>(x, C, segptr, members, (int)nseg, mean, out);
  GEOBI_LAUNCH_OK();
  return 0;
}

int segment_sum2(const float* x, int C, const int32_t* segptr1, const int32_t* members1, const int32_t* segptr2,
                 const int32_t* members2, int64_t nseg2, float* out, hipStream_t s) {
  if (nseg2 <= 0) return 0;
  GEOBI_REQUIRE((C & 3) == 0, "segment_sum2: channel count %d is not a multiple of 4", C);
  segment_sum2_kernel<<<cdiv(nseg2 * (C >> 2), 256), 256, 0, s>>>(x, C, segptr1, members1, segptr2, members2, (int)nseg2, out);
  GEOBI_LAUNCH_OK();
  return 0;
}

int segment_mean_bwd(const float* gout, const int32_t* seg, const int32_t* segptr, int C, int64_t n_fine, float* gx,
                     hipStream_t s) {
  if (n_fine <= 0) return 0;
  segment_mean_bwd_kernel<<<cdiv(n_fine * C, 256), 256, 0, s>>>(gout, seg, segptr, C, n_fine * C, gx);
  GEOBI_LAUNCH_OK();
  return 0;
}

int gather_rows(const float* x, const int32_t* idx, int C, int64_t n_out, float* out, hipStream_t s) {
  if (n_out <= 0) return 0;
  gather_rows_kernel<<<cdiv(n_out * C, 256), 256, 0, s>>>(x, idx, C, n_out * C, out);
  GEOBI_LAUNCH_OK();
  return 0;
}

namespace {
struct EdgeRowsBuffers { CountScan cnt; int4* rowinfo; int* tcol; float* tw; };
// with E_fine (the fine edge count) the workspace also holds the scratch pair tcol, tw of the one-pass form
EdgeRowsBuffers carve_edge_rows(Arena& a, int64_t nbound, int64_t E_fine) {
  return {carve_count_scan(a, nbound + 1), a.take<int4>(nbound), E_fine > 0 ? a.take<int>(E_fine) : nullptr,
          E_fine > 0 ? a.take<float>(E_fine) : nullptr};
}
}  // namespace

size_t pool_edge_rows_ws_bytes_onepass(int64_t nbound, int64_t E) {
  return carve_bytes([&](Arena& a) { carve_edge_rows(a, nbound, E); });
}
size_t pool_edge_rows_ws_bytes(int64_t nbound) { return pool_edge_rows_ws_bytes_onepass(nbound, 0); }

// cnew, (segptr, members) = pair lists built with the bound `nbound` (fine node count), ncount = device
// count of coarse nodes.  rowptr_c has nbound + 1 entries; count[0] = coarse edges; overflow[0] |= 1 if
// some row did not fit (outputs are then incomplete and the caller must use pool_edge).
int pool_edge_rows(const int32_t* cnew, const int32_t* segptr, const int32_t* members, const int32_t* rowptr,
                   const int32_t* col, const float* w, const int32_t* ncount, int64_t nbound, int32_t* rowptr_c,
                   int32_t* row_c, int32_t* col_c, float* w_c, int32_t* count, int32_t* overflow, void* ws,
                   size_t ws_bytes, hipStream_t s, int64_t E_fine, const void* rowinfo_in, const int32_t* publish_src,
                   int32_t* publish_host, int publish_seq) {
  GEOBI_REQUIRE(nbound > 0, "pool_edge_rows: empty");
  Arena a(ws, ws_bytes);
  const EdgeRowsBuffers b = carve_edge_rows(a, nbound, E_fine);
  GEOBI_WS_CHECK("pool_edge_rows", a, ws, ws_bytes);
  int* cnt = b.cnt.cnt;
  int4* rowinfo = b.rowinfo;
  int blocks = cdiv(nbound, 4);
  if (E_fine > 0) {
    // one-pass form (callers that sized the workspace with pool_edge_rows_ws_bytes_onepass): gather + relabel + sort +
    // merge ONCE, entries parked in scratch, then a short copy pass instead of a second merge
    int* tcol = b.tcol;
    float* tw = b.tw;
    pool_edge_rows_kernel<2><<<blocks, 256, 0, s>>>(cnew, segptr, members, rowptr, col, w, ncount, (int)nbound, cnt,
                                                     nullptr, nullptr, tcol, tw, overflow, nullptr, rowinfo,
                                                     (const int4*)rowinfo_in);
    GEOBI_LAUNCH_OK();
    GEOBI_TRY(b.cnt.scan.run(cnt, rowptr_c, s));
    pool_edge_compact_kernel<<<cdiv(nbound * 16, 256), 256, 0, s>>>(ncount, (int)nbound, rowptr_c, rowinfo, tcol,
                                                                    w ? tw : nullptr, row_c, col_c, w_c, count,
                                                                    publish_src, publish_host, publish_seq);
    GEOBI_LAUNCH_OK();
    return 0;
  }
  pool_edge_rows_kernel<0><<<blocks, 256, 0, s>>>(cnew, segptr, members, rowptr, col, w, ncount, (int)nbound, cnt,
                                                   nullptr, nullptr, nullptr, nullptr, overflow, nullptr, rowinfo, nullptr);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(b.cnt.scan.run(cnt, rowptr_c, s));
  pool_edge_rows_kernel<1><<<blocks, 256, 0, s>>>(cnew, segptr, members, rowptr, col, w, ncount, (int)nbound, cnt,
                                                   rowptr_c, row_c, col_c, w_c, overflow, count, rowinfo, nullptr);
  GEOBI_LAUNCH_OK();
  return 0;
}

namespace {
struct PoolEdgeBuffers { uint64_t *k_in, *k_out, *ukeys; int *v_in, *v_out, *rank; CountScan head; PairSort<uint64_t, int> sort; };
PoolEdgeBuffers carve_pool_edge(Arena& a, int64_t E) {
  return {a.take<uint64_t>(E), a.take<uint64_t>(E), a.take<uint64_t>(E), a.take<int>(E), a.take<int>(E), a.take<int>(E),
          carve_count_scan(a, E), PairSort<uint64_t, int>::take(a, E)};
}
}  // namespace

size_t pool_edge_ws_bytes(int64_t E) { return carve_bytes([&](Arena& a) { carve_pool_edge(a, E); }); }

// Outputs are sized for the worst case (E entries, nmax + 1 row pointers); the true edge count is
// written to count[0] on the device.
int pool_edge(const int32_t* cnew, const int32_t* row, const int32_t* col, const float* w, int64_t E, int64_t nmax,
              int32_t* rowptr_c, int32_t* row_c, int32_t* col_c, float* w_c, int32_t* count, void* ws,
              size_t ws_bytes, hipStream_t s) {
  if (E <= 0) {
    GEOBI_HIP(hipMemsetAsync(rowptr_c, 0, sizeof(int) * (nmax + 1), s));
    GEOBI_HIP(hipMemsetAsync(count, 0, sizeof(int), s));
    return 0;
  }
  Arena a(ws, ws_bytes);
  const PoolEdgeBuffers b = carve_pool_edge(a, E);
  GEOBI_WS_CHECK("pool_edge", a, ws, ws_bytes);
  uint64_t *k_in = b.k_in, *k_out = b.k_out, *ukeys = b.ukeys;
  int *v_in = b.v_in, *v_out = b.v_out, *head = b.head.cnt, *rank = b.rank;
  int blocks = cdiv(E, 256);
  const int bits = key_bits(nmax);
  pool_edge_keys_kernel<<<blocks, 256, 0, s>>>(cnew, row, col, E, bits, k_in, v_in);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(b.sort.run(k_in, k_out, v_in, v_out, E, (unsigned)(2 * bits), s));
  pool_edge_heads_kernel<<<blocks, 256, 0, s>>>(k_out, E, head);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(b.head.scan.run(head, rank, s));
  pool_edge_emit_kernel<<<blocks, 256, 0, s>>>(k_out, v_out, head, rank, w, E, row_c, col_c, w_c, ukeys, count,
                                               bits);
  GEOBI_LAUNCH_OK();
  pool_edge_rowptr_kernel<<<cdiv(nmax + 1, 256), 256, 0, s>>>(ukeys, count, (int)nmax, bits, rowptr_c);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // namespace geobi
