// Mesh regularisers on the loop-free symmetric vertex CSR of a sample (graph.py: rowptr_out / col_out): the reference's
// Laplacian term, laplacian_loss(vp, v, edge_idx_v, normal) (code/network.py:347-361), and an edge-length term beside it.
// N(i) = row i of the CSR, deg_i its length, m_i = max(deg_i, 1); vp the prediction, v the ground truth [V, 3].
//
//   lap(p)_i = (1 / m_i) sum_{j in N(i)} (p_i - p_j)            with a normal:  lap(p)_i <- n_i (n_i . lap(p)_i)
//   d_i      = lap(vp)_i - lap(v)_i
//   L_lap    = sum_i wl_i sum_c |d_ic|                          wl_i = 1 / V, or 1 / (B n_mesh) of a union batch
//   L_edge   = sum_i we_i sum_{j in N(i)} (|vp_i - vp_j| - |v_i - v_j|)^2      we_i = 1 / E, or 1 / (B E_mesh)
//
//   forward   one pass over the rows: both terms from ONE walk of the row (row_walk: a neighbour's vp_j and v_j are
//             gathered once, whatever the term mask), per-row terms times the row weight into fp64 block partials
//             (block_sum_fp64), the partials in ascending order (fold_ascending) by a second launch.  The same pass
//             writes the Laplacian's backward seed u_i = wl_i g_i / m_i, g_i = sign(d_i) or n_i (n_i . sign(d_i)).
//   backward  gvp_k = gout_lap (deg_k u_k - sum_{i in N(k)} u_i)
//                     + gout_edge sum_{j in N(k)} (we_k + we_j) 2 (|e_p| - |e_g|) e_p / |e_p|,   e_p = vp_k - vp_j
//             one gather over the same walk: k in N(i) <=> i in N(k) on a symmetric graph, so the rows that hold k ARE
//             row k.  An entry with |e_p| = 0 has no direction and adds nothing.
//
// Every sum is formed from coordinate differences p_i - p_j in ascending column order (after scaling the
// coordinates are 10-100 edge lengths from the origin; p_i - mean_j p_j would lose those digits).  No atomics, no order
// that depends on timing, no host synchronisation: the same input gives the same bits.  One thread per row: level-0
// degrees are 6-7, a hub is only slower.  What the kernels read is clamped to the arrays (row ends to [0, E], column ids
// to [0, V)): a foreign CSR gives wrong numbers, never a read outside.
#include "common.h"
#include "../../include/geobi_hip.h"

#include <math.h>

namespace geobi {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 512;        // forward grid: above kMaxBlocks * kThreads rows a thread walks several rows
constexpr int kTermLap = 1, kTermEdge = 2;

struct F3 { float x, y, z; };
__device__ __forceinline__ F3 load3(const float* __restrict__ p, int i) {
  return {p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]};
}
// written out, contraction off: lap(vp) and lap(v) go through the same instructions, so vp == v gives d == 0 exactly
__device__ __forceinline__ F3 diff(F3 a, F3 b) {
#pragma clang fp contract(off)
  return {a.x - b.x, a.y - b.y, a.z - b.z};
}
__device__ __forceinline__ float length(F3 e) {
#pragma clang fp contract(off)
  return sqrtf(e.x * e.x + e.y * e.y + e.z * e.z);
}
__device__ __forceinline__ F3 project(F3 n, F3 s) {
#pragma clang fp contract(off)
  const float d = n.x * s.x + n.y * s.y + n.z * s.z;
  return {n.x * d, n.y * d, n.z * d};
}
__device__ __forceinline__ float sign0(float d) { return d > 0.f ? 1.0f : (d < 0.f ? -1.0f : 0.f); }   // sign(0) = 0, as torch

// THE walk: row i of the CSR in ascending column order; visit(j, vp_i - vp_j, v_i - v_j) per neighbour.  kPoints = false:
// the neighbour ids alone (visit(j, {}, {})), nothing is gathered from vp / v.  -> deg_i
template <bool kPoints, class Visit>
__device__ __forceinline__ int row_walk(const int* __restrict__ rowptr, const int* __restrict__ col, int V, int E,
                                        const float* __restrict__ vp, const float* __restrict__ v, int i, Visit visit) {
  const int k0 = min(max(rowptr[i], 0), E), k1 = min(max(rowptr[i + 1], k0), E);
  F3 pi = {0.f, 0.f, 0.f}, gi = pi;
  if (kPoints) { pi = load3(vp, i); gi = load3(v, i); }
  for (int k = k0; k < k1; ++k) {
    const int j = min(max(col[k], 0), V - 1);
    if (kPoints) visit(j, diff(pi, load3(vp, j)), diff(gi, load3(v, j)));
    else visit(j, pi, gi);
  }
  return k1 - k0;
}

__global__ __launch_bounds__(kThreads) void reg_fwd_kernel(const float* __restrict__ vp, const float* __restrict__ v,
                                                           const float* __restrict__ normal, const int* __restrict__ rowptr,
                                                           const int* __restrict__ col, int V, int E,
                                                           const float* __restrict__ w_lap, const float* __restrict__ w_edge,
                                                           float wl_all, float we_all, int terms, float* __restrict__ u,
                                                           double* __restrict__ partial) {
  __shared__ double s_edge[kThreads];
  const bool do_lap = terms & kTermLap, do_edge = terms & kTermEdge;
  double acc_lap = 0.0, acc_edge = 0.0;
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < V; i += gridDim.x * kThreads) {
    F3 sp = {0.f, 0.f, 0.f}, sg = sp;
    double row_edge = 0.0;
    const int deg = row_walk<true>(rowptr, col, V, E, vp, v, i, [&](int, F3 ep, F3 eg) {
      sp.x += ep.x; sp.y += ep.y; sp.z += ep.z;
      sg.x += eg.x; sg.y += eg.y; sg.z += eg.z;
      if (do_edge) {
        const float dl = length(ep) - length(eg);
        row_edge += (double)dl * (double)dl;
      }
    });
    if (do_edge) acc_edge += (double)(w_edge ? w_edge[i] : we_all) * row_edge;
    if (do_lap) {
      const float inv = 1.0f / (float)max(deg, 1);
      F3 lp = {sp.x * inv, sp.y * inv, sp.z * inv}, lg = {sg.x * inv, sg.y * inv, sg.z * inv};
      F3 n = {0.f, 0.f, 0.f};
      if (normal) { n = load3(normal, i); lp = project(n, lp); lg = project(n, lg); }
      const F3 d = diff(lp, lg);
      const float wl = w_lap ? w_lap[i] : wl_all;
      acc_lap += (double)wl * (double)(fabsf(d.x) + fabsf(d.y) + fabsf(d.z));
      F3 g = {sign0(d.x), sign0(d.y), sign0(d.z)};
      if (normal) g = project(n, g);
      const float c = wl * inv;
      u[3 * (size_t)i] = c * g.x; u[3 * (size_t)i + 1] = c * g.y; u[3 * (size_t)i + 2] = c * g.z;
    }
  }
  s_edge[threadIdx.x] = acc_edge;
  const double sum_lap = block_sum_fp64<kThreads>(acc_lap, [&](int h) { s_edge[threadIdx.x] += s_edge[threadIdx.x + h]; });
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = sum_lap;
    partial[2 * blockIdx.x + 1] = s_edge[0];
  }
}

__global__ void reg_final_kernel(const double* __restrict__ partial, int n, float* __restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x < 2) out[threadIdx.x] = (float)fold_ascending(partial + threadIdx.x, n, 2);
}

template <bool kLap, bool kEdge>
__global__ __launch_bounds__(kThreads) void reg_bwd_kernel(const float* __restrict__ vp, const float* __restrict__ v,
                                                           const int* __restrict__ rowptr, const int* __restrict__ col,
                                                           int V, int E, const float* __restrict__ u,
                                                           const float* __restrict__ w_edge, float we_all,
                                                           const float* __restrict__ gout, float* __restrict__ gvp) {
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= V) return;
  F3 su = {0.f, 0.f, 0.f}, se = su;
  const float wk = kEdge ? (w_edge ? w_edge[k] : we_all) : 0.f;
  const int deg = row_walk<kEdge>(rowptr, col, V, E, vp, v, k, [&](int j, F3 ep, F3 eg) {
    if (kLap) {
      const F3 uj = load3(u, j);
      su.x += uj.x; su.y += uj.y; su.z += uj.z;
    }
    if (kEdge) {
      const float lp = length(ep);
      const float c = lp > 0.f ? (wk + (w_edge ? w_edge[j] : we_all)) * 2.0f * (lp - length(eg)) / lp : 0.f;
      se.x += c * ep.x; se.y += c * ep.y; se.z += c * ep.z;
    }
  });
  F3 g = {0.f, 0.f, 0.f};
  if (kLap) {
    const F3 uk = load3(u, k);
    const float gl = gout[0], fd = (float)deg;
    g.x = gl * (fd * uk.x - su.x); g.y = gl * (fd * uk.y - su.y); g.z = gl * (fd * uk.z - su.z);
  }
  if (kEdge) {
    const float ge = gout[1];
    g.x += ge * se.x; g.y += ge * se.y; g.z += ge * se.z;
  }
  gvp[3 * (size_t)k] = g.x; gvp[3 * (size_t)k + 1] = g.y; gvp[3 * (size_t)k + 2] = g.z;
}

int fwd_blocks(int64_t V) {
  const int64_t b = (V + kThreads - 1) / kThreads;
  return (int)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

// the block sums of the forward: (Laplacian, edge) per block
double* carve_partials(Arena& a, int64_t V) { return a.take<double>((size_t)2 * fwd_blocks(V)); }

// the weight of an entry / a row when no per-row weights are given: the plain mean (0 for a mesh without edges)
float uniform_weight(int64_t n) { return n > 0 ? (float)(1.0 / (double)n) : 0.f; }

}  // namespace

}  // namespace geobi

using namespace geobi;

extern "C" {

size_t geobi_mesh_reg_ws_bytes(int64_t V) {
  return V < 0 || V > GEOBI_MAX_NODES ? 0 : carve_bytes([&](Arena& a) { carve_partials(a, V); });
}

int geobi_mesh_reg_fwd(const float* vp, const float* v, const float* normal, const int32_t* rowptr, const int32_t* col,
                       int64_t V, int64_t E, const float* w_lap, const float* w_edge, int terms, float* out, float* u,
                       void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(V, E);
  GEOBI_REQUIRE(V >= 1, "%s: V = %lld vertices (at least one)", __func__, (long long)V);
  GEOBI_REQUIRE(terms >= 1 && terms <= 3, "%s: terms %d (bit 0 Laplacian, bit 1 edge length, at least one)", __func__, terms);
  GEOBI_NOTNULL(vp); GEOBI_NOTNULL(v); GEOBI_NOTNULL(rowptr); GEOBI_NOTNULL(out); GEOBI_NOTNULL(ws);
  if (E > 0) GEOBI_NOTNULL(col);
  if (terms & 1) GEOBI_NOTNULL(u);
  hipStream_t s = as_stream(stream);
  Arena ar(ws, ws_bytes);
  double* partial = carve_partials(ar, V);
  GEOBI_WS_CHECK("mesh_reg_fwd", ar, ws, ws_bytes);
  const int blocks = fwd_blocks(V);
  reg_fwd_kernel<<<blocks, kThreads, 0, s>>>(vp, v, normal, rowptr, col, (int)V, (int)E, w_lap, w_edge, uniform_weight(V),
                                             uniform_weight(E), terms, u, partial);
  reg_final_kernel<<<1, 64, 0, s>>>(partial, blocks, out);
  GEOBI_LAUNCH_OK();
  return 0;
}

int geobi_mesh_reg_bwd(const float* vp, const float* v, const int32_t* rowptr, const int32_t* col, int64_t V, int64_t E,
                       const float* u, const float* w_edge, const float* gout, int terms, float* gvp, void* stream) {
  GEOBI_SIZES(V, E);
  GEOBI_REQUIRE(V >= 1, "%s: V = %lld vertices (at least one)", __func__, (long long)V);
  GEOBI_REQUIRE(terms >= 1 && terms <= 3, "%s: terms %d (bit 0 Laplacian, bit 1 edge length, at least one)", __func__, terms);
  GEOBI_NOTNULL(vp); GEOBI_NOTNULL(v); GEOBI_NOTNULL(rowptr); GEOBI_NOTNULL(gout); GEOBI_NOTNULL(gvp);
  if (E > 0) GEOBI_NOTNULL(col);
  if (terms & 1) GEOBI_NOTNULL(u);
  hipStream_t s = as_stream(stream);
  const int blocks = cdiv(V, kThreads);
  const float we_all = uniform_weight(E);
  if ((terms & kTermLap) && (terms & kTermEdge))
    reg_bwd_kernel<true, true><<<blocks, kThreads, 0, s>>>(vp, v, rowptr, col, (int)V, (int)E, u, w_edge, we_all, gout, gvp);
  else if (terms & kTermLap)
    reg_bwd_kernel<true, false><<<blocks, kThreads, 0, s>>>(vp, v, rowptr, col, (int)V, (int)E, u, w_edge, we_all, gout, gvp);
  else
    reg_bwd_kernel<false, true><<<blocks, kThreads, 0, s>>>(vp, v, rowptr, col, (int)V, (int)E, u, w_edge, we_all, gout, gvp);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // extern "C"
