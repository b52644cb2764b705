// FeaSt graph convolution (the 16 message-passing layers of the hot path), node-level form.
//
// Reference semantics (torch_geometric FeaStConv, called at /root/reference/code/network.py:271-299):
//   q_ij = softmax_h(u (x_j - x_i) + c),  out_i = mean_{j in N(i) + self} sum_h q_ijh W_h x_j + bias.
// The reference evaluates `lin(x_j)` per EDGE ([E, 9*Cout] temporaries).  Here
//   p = x u^T                       per node   [N, 9]
//   z_i[h,:] = 1/deg_i sum_j q_ijh x_j         (aggregation: the "scatter-add" of the path, done
//                                               as a sorted-segment gather over the CSR -- no atomics)
//   out = z W_packed + bias         per node   MFMA fp32 GEMM  [N, 9*Cin] x [9*Cin, Cout]
// which needs Cin floats per edge instead of 9*Cout and keeps every sum in a fixed order.
//
// Backward (transposed aggregation instead of atomics):
//   dz = g W_packed^T;  row pass over targets: s_ijh = dz_i[h,:].x_j, softmax backward -> dl_ij;
//   column pass over sources j: r_j[h,:] = sum_i q_ijh/deg_i g_i  (same gather kernel, transposed CSR);
//   dx = [r | dp] [lin.weight ; u.weight];  dW = z^T g;  du = dp^T x;  dc, dbias column sums.
#include "../../include/geobi_hip.h"

#include <algorithm>
#include <cstdlib>

#include "common.h"
#include "feast_dev.h"

namespace geobi {

namespace {

using namespace feast_dev;

// ----------------------------------------------------------------------------- logits
template <int C>
__global__ __launch_bounds__(256) void feast_logits_kernel(const float* __restrict__ xa, const float* __restrict__ xb,
                                                           int Ca, const float* __restrict__ u, int N,
                                                           float* __restrict__ p) {
  __shared__ float su[H * C];
  for (int i = threadIdx.x; i < H * C; i += 256) su[i] = u[i];
  __syncthreads();
  int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float acc[H];
#pragma unroll
  for (int h = 0; h < H; ++h) acc[h] = 0.f;
  const int Cb = C - Ca;
  // 16-B pieces only when neither input part cuts one (a 12-channel row split 6 | 6 used to be read as three float4 from
  // the first part: found by tools/fuzz_kernels.py, no layer of the network has that shape)
  if ((C & 3) == 0 && (Ca & 3) == 0) {
    for (int k = 0; k < C; k += 4) {
      const float* src = (k < Ca) ? xa + (size_t)n * Ca + k : xb + (size_t)n * Cb + (k - Ca);
      float4 t = *reinterpret_cast<const float4*>(src);
      float xv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int h = 0; h < H; ++h) acc[h] = fmaf(xv[i], su[h * C + k + i], acc[h]);
    }
  } else {
    for (int k = 0; k < C; ++k) {
      float xv = (k < Ca) ? xa[(size_t)n * Ca + k] : xb[(size_t)n * Cb + (k - Ca)];
#pragma unroll
      for (int h = 0; h < H; ++h) acc[h] = fmaf(xv, su[h * C + k], acc[h]);
    }
  }
  float4* dst = reinterpret_cast<float4*>(p + (size_t)n * HP);
  dst[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
  dst[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
  dst[2] = make_float4(acc[8], 0.f, 0.f, 0.f);
}

// Same product with 16 lanes per node (C >= 32): one thread per node walks its row piece by piece, every load waited
// for in turn -- 13 us per launch whatever N (6 + 6 launches per step, 10 % of a single-mesh inference).  Here a
// node's row is ONE coalesced read of its 16-lane group (C / 16 channels per lane), the nine partial dot products are
// reduced over the group with DPP steps, four nodes per wave.
template <int C>
__global__ __launch_bounds__(256) void feast_logits_group_kernel(const float* __restrict__ xa, const float* __restrict__ xb,
                                                                 int Ca, const float* __restrict__ u, int N,
                                                                 float* __restrict__ p) {
  constexpr int VEC = C / 16;
  static_assert(VEC == 2 || VEC == 4 || VEC == 8, "32, 64 or 128 channels");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, k = lane & 15;
  const int node = (blockIdx.x * 4 + wave) * 4 + g;
  const int ns = node < N ? node : N - 1;          // every lane takes part in the reductions
  const int c0 = k * VEC;
  const float* src = c0 < Ca ? xa + (size_t)ns * Ca + c0 : xb + (size_t)ns * (C - Ca) + (c0 - Ca);
  float xv[VEC];
  if constexpr (VEC == 2) {
    const float2 t = *reinterpret_cast<const float2*>(src);
    xv[0] = t.x; xv[1] = t.y;
  } else {
#pragma unroll
    for (int q = 0; q < VEC / 4; ++q) {
      const float4 t = reinterpret_cast<const float4*>(src)[q];
      xv[4 * q] = t.x; xv[4 * q + 1] = t.y; xv[4 * q + 2] = t.z; xv[4 * q + 3] = t.w;
    }
  }
  float acc[H];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    const float* ur = u + h * C + c0;              // 9 C floats in all: L1 / L2 resident
    float a = 0.f;
    if constexpr (VEC == 2) {
      const float2 t = *reinterpret_cast<const float2*>(ur);
      a = fmaf(xv[0], t.x, xv[1] * t.y);
    } else {
#pragma unroll
      for (int q = 0; q < VEC / 4; ++q) {
        const float4 t = reinterpret_cast<const float4*>(ur)[q];
        a = fmaf(xv[4 * q], t.x, a); a = fmaf(xv[4 * q + 1], t.y, a);
        a = fmaf(xv[4 * q + 2], t.z, a); a = fmaf(xv[4 * q + 3], t.w, a);
      }
    }
    acc[h] = group_allreduce<16>(a);
  }
  if (node < N && k == 0) {
    float4* dst = reinterpret_cast<float4*>(p + (size_t)node * HP);
    dst[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    dst[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    dst[2] = make_float4(acc[8], 0.f, 0.f, 0.f);
  }
}

// ------------------------------------------------------------------------- aggregation
// G = C / VEC lanes own one centre node (VEC consecutive channels each); a wave owns 64 / G
// consecutive nodes.  Per group and per chunk of G edges:
//   phase 1 (lane = edge)   : gather p of the neighbour, 9-way softmax, park q and the neighbour
//                             id in the wave's LDS slots -> every exp is computed exactly once;
//   phase 2 (lane = channel): for each parked edge read q (LDS broadcast), gather the neighbour's
//                             feature slice (VEC*4 B per lane, a row is one contiguous G*VEC*4 B
//                             read) and fma into the 9 x VEC register accumulators.
// MODE 0: forward  z_i[h,:] = 1/deg_i (q_self x_i + sum_j q_ij x_j),  logits p_j - p_i + c
// MODE 1: backward transposed   r_j[h,:] = sum_i q_ij / deg_i g_i  (+ self), logits p_ctr - p_nbr + c,
//         walking the CSR of the OTHER direction; deg comes from `deg_rowptr`.
// LC > 0: logits from the raw rows `xl` [N, LC] and `ul` [H, LC] per edge (see edge_logits) instead of `p`.
template <int C, int VEC, int MODE, int LC>
__global__ __launch_bounds__(256) void feast_aggregate_kernel(
    const float* __restrict__ xa, const float* __restrict__ xb, int Ca, const float* __restrict__ p,
    const float* __restrict__ cvec, const int* __restrict__ rowptr, const int* __restrict__ col,
    const int* __restrict__ deg_rowptr, int N, float* __restrict__ out, int ldo, const float* __restrict__ xl,
    const float* __restrict__ ul) {
  constexpr int G = C / VEC;
  constexpr int NPW = 64 / G;
  static_assert(G * VEC == C && G >= 2 && (64 % G) == 0, "group shape");
  __shared__ __attribute__((aligned(16))) float s_slot[4][64][HP];
  __shared__ __attribute__((aligned(16))) float s_u[LC > 0 ? LC * HP : 4];
  if constexpr (LC > 0) stage_u<LC>(ul, s_u);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / G, k = lane % G;
  float(*slot)[HP] = s_slot[wave];
  const int node0 = (xcd_block(blockIdx.x, gridDim.x) * 4 + wave) * NPW;
  if (node0 >= N) return;
  const int node = node0 + g;
  const bool valid = node < N;
  const int ns = valid ? node : N - 1;
  const int rs = rowptr[ns];
  const int re = valid ? rowptr[ns + 1] : rs;

  const int c0 = k * VEC;
  const float* fbase;
  int fstride;
  if (c0 < Ca) { fbase = xa + c0; fstride = Ca; } else { fbase = xb + (c0 - Ca); fstride = C - Ca; }

  float pc[H], cc[H], qs[H];
  float xc[LC > 0 ? LC : 1];
  if constexpr (LC > 0) load_row<LC>(xl + (size_t)ns * LC, xc);
  else load_hp(p + (size_t)ns * HP, pc);
#pragma unroll
  for (int h = 0; h < H; ++h) { cc[h] = cvec[h]; qs[h] = cc[h]; }
  softmax9(qs);   // the self edge: u(x_i - x_i) + c = c exactly

  float acc[H][VEC];
  {
    float xs[VEC];
    load_vec<VEC>(fbase + (size_t)ns * fstride, xs);
    float sscale = 1.0f;
    if constexpr (MODE == 1) sscale = 1.0f / (float)(deg_rowptr[ns + 1] - deg_rowptr[ns] + 1);
#pragma unroll
    for (int h = 0; h < H; ++h)
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[h][v] = qs[h] * sscale * xs[v];
  }

  for (int base = rs; base < re; base += G) {
    // ---- phase 1: lane k of the group handles edge base + k
    {
      const int e = base + k;
      float q[H];
      int j = ns;
      if (e < re) {
        j = col[e];
        if constexpr (LC > 0) {
          float d[LC];
          load_row<LC>(xl + (size_t)j * LC, d);
#pragma unroll
          for (int i = 0; i < LC; ++i) d[i] = (MODE == 0) ? (d[i] - xc[i]) : (xc[i] - d[i]);
          edge_logits<LC>(d, s_u, cc, q);
        } else {
          float pn[H];
          load_hp(p + (size_t)j * HP, pn);
#pragma unroll
          for (int h = 0; h < H; ++h) q[h] = (MODE == 0) ? (pn[h] - pc[h] + cc[h]) : (pc[h] - pn[h] + cc[h]);
        }
        softmax9(q);
        if constexpr (MODE == 1) {
          float w = 1.0f / (float)(deg_rowptr[j + 1] - deg_rowptr[j] + 1);
#pragma unroll
          for (int h = 0; h < H; ++h) q[h] *= w;
        }
      } else {
#pragma unroll
        for (int h = 0; h < H; ++h) q[h] = 0.f;
      }
      float4* dst = reinterpret_cast<float4*>(slot[lane]);
      dst[0] = make_float4(q[0], q[1], q[2], q[3]);
      dst[1] = make_float4(q[4], q[5], q[6], q[7]);
      dst[2] = make_float4(q[8], __int_as_float(j), 0.f, 0.f);
    }
    wave_lds_sync();
    // ---- phase 2: all G lanes of the group walk the parked edges, two at a time
    const int cnt = min(G, re - base);
    for (int t = 0; t < cnt; t += 2) {
      const float4* s0 = reinterpret_cast<const float4*>(slot[g * G + t]);
      const float4* s1 = reinterpret_cast<const float4*>(slot[g * G + t + 1]);
      float4 a0 = s0[0], b0 = s0[1], d0 = s0[2];
      float4 a1 = s1[0], b1 = s1[1], d1 = s1[2];
      float x0[VEC], x1[VEC];
      load_vec<VEC>(fbase + (size_t)__float_as_int(d0.y) * fstride, x0);
      load_vec<VEC>(fbase + (size_t)__float_as_int(d1.y) * fstride, x1);
      const float q0[H] = {a0.x, a0.y, a0.z, a0.w, b0.x, b0.y, b0.z, b0.w, d0.x};
      const float q1[H] = {a1.x, a1.y, a1.z, a1.w, b1.x, b1.y, b1.z, b1.w, d1.x};
#pragma unroll
      for (int h = 0; h < H; ++h)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[h][v] = fmaf(q0[h], x0[v], acc[h][v]);
#pragma unroll
      for (int h = 0; h < H; ++h)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[h][v] = fmaf(q1[h], x1[v], acc[h][v]);
    }
    wave_lds_sync();
  }

  if (!valid) return;
  float scale = 1.0f;
  if constexpr (MODE == 0) scale = 1.0f / (float)(re - rs + 1);
  float* orow = out + (size_t)node * ldo;
#pragma unroll
  for (int h = 0; h < H; ++h) {
    float v[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = acc[h][i] * scale;
    if constexpr (MODE == 0 && VEC == 4) {
      typedef float f4 __attribute__((ext_vector_type(4)));
      f4 t = {v[0], v[1], v[2], v[3]};
      __builtin_nontemporal_store(t, reinterpret_cast<f4*>(orow + h * C + c0));   // z is written once, streamed
    } else {
      store_vec<VEC>(orow + h * C + c0, v);
    }
  }
  if constexpr (MODE == 0) {
    // zero the row padding [H*C, ldo) so the packed GEMM can run over the padded K
    for (int i = H * C + k; i < ldo; i += G) orow[i] = 0.f;
  }
}

// --------------------------------------------------------------------- backward row pass
// For every target i (group of G lanes holding dz_i): per in-edge recompute q, form
// s_h = dz_i[h,:].x_j, softmax backward dl_h = q_h (s_h - sum q s) / deg_i, write dl per edge
// and the per-node sums:  dpn_i = sum_j dl_ij  (what flows to -p_i),  dcs_i = dpn_i + dl_self.
template <int C, int VEC, int LC>
__global__ __launch_bounds__(256) void feast_rowpass_kernel(
    const float* __restrict__ xa, const float* __restrict__ xb, int Ca, const float* __restrict__ p,
    const float* __restrict__ cvec, const int* __restrict__ rowptr, const int* __restrict__ col,
    const float* __restrict__ dz, int ldz, int N, float* __restrict__ dl, float* __restrict__ dpn,
    float* __restrict__ dcs, int ld_dcs, const float* __restrict__ ul) {
  constexpr int G = C / VEC;
  constexpr int NPW = 64 / G;
  static_assert(LC == 0 || LC == C, "per-edge logits read the layer's own (unsplit) input rows");
  __shared__ __attribute__((aligned(16))) float s_slot[4][64][HP];
  __shared__ __attribute__((aligned(16))) float s_u[LC > 0 ? LC * HP : 4];
  if constexpr (LC > 0) stage_u<LC>(ul, s_u);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / G, k = lane % G;
  float(*slot)[HP] = s_slot[wave];
  const int node0 = (xcd_block(blockIdx.x, gridDim.x) * 4 + wave) * NPW;
  if (node0 >= N) return;
  const int node = node0 + g;
  const bool valid = node < N;
  const int ns = valid ? node : N - 1;
  const int rs = rowptr[ns];
  const int re = valid ? rowptr[ns + 1] : rs;

  const int c0 = k * VEC;
  const float* fbase;
  int fstride;
  if (c0 < Ca) { fbase = xa + c0; fstride = Ca; } else { fbase = xb + (c0 - Ca); fstride = C - Ca; }

  float pc[H], cc[H], qs[H];
  float xc[LC > 0 ? LC : 1];
  if constexpr (LC > 0) load_row<LC>(xa + (size_t)ns * LC, xc);
  else load_hp(p + (size_t)ns * HP, pc);
#pragma unroll
  for (int h = 0; h < H; ++h) { cc[h] = cvec[h]; qs[h] = cc[h]; }
  softmax9(qs);

  float dzr[H][VEC];
#pragma unroll
  for (int h = 0; h < H; ++h) load_vec<VEC>(dz + (size_t)ns * ldz + h * C + c0, dzr[h]);
  const float invd = 1.0f / (float)(re - rs + 1);

  float dsum[H];   // sum over real edges of dl
  float dself[H];
  {
    float xs[VEC];
    load_vec<VEC>(fbase + (size_t)ns * fstride, xs);
    float s[H];
    float tq = 0.f;
#pragma unroll
    for (int h = 0; h < H; ++h) {
      float a = 0.f;
#pragma unroll
      for (int v = 0; v < VEC; ++v) a = fmaf(dzr[h][v], xs[v], a);
      s[h] = group_allreduce<G>(a);
      tq = fmaf(qs[h], s[h], tq);
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {
      dself[h] = qs[h] * (s[h] - tq) * invd;
      dsum[h] = 0.f;
    }
  }

  for (int base = rs; base < re; base += G) {
    {
      const int e = base + k;
      float q[H];
      int j = ns;
      if (e < re) {
        j = col[e];
        if constexpr (LC > 0) {
          float d[LC];
          load_row<LC>(xa + (size_t)j * LC, d);
#pragma unroll
          for (int i = 0; i < LC; ++i) d[i] -= xc[i];
          edge_logits<LC>(d, s_u, cc, q);
        } else {
          float pn[H];
          load_hp(p + (size_t)j * HP, pn);
#pragma unroll
          for (int h = 0; h < H; ++h) q[h] = pn[h] - pc[h] + cc[h];
        }
        softmax9(q);
      } else {
#pragma unroll
        for (int h = 0; h < H; ++h) q[h] = 0.f;
      }
      float4* dst = reinterpret_cast<float4*>(slot[lane]);
      dst[0] = make_float4(q[0], q[1], q[2], q[3]);
      dst[1] = make_float4(q[4], q[5], q[6], q[7]);
      dst[2] = make_float4(q[8], __int_as_float(j), 0.f, 0.f);
    }
    wave_lds_sync();
    const int cnt = min(G, re - base);
    for (int t = 0; t < cnt; ++t) {
      const float4* s0 = reinterpret_cast<const float4*>(slot[g * G + t]);
      float4 a0 = s0[0], b0 = s0[1], d0 = s0[2];
      float xj[VEC];
      load_vec<VEC>(fbase + (size_t)__float_as_int(d0.y) * fstride, xj);
      const float q[H] = {a0.x, a0.y, a0.z, a0.w, b0.x, b0.y, b0.z, b0.w, d0.x};
      float s[H];
      float tq = 0.f;
#pragma unroll
      for (int h = 0; h < H; ++h) {
        float a = 0.f;
#pragma unroll
        for (int v = 0; v < VEC; ++v) a = fmaf(dzr[h][v], xj[v], a);
        s[h] = group_allreduce<G>(a);
        tq = fmaf(q[h], s[h], tq);
      }
      float d[HP];
#pragma unroll
      for (int h = 0; h < H; ++h) {
        d[h] = q[h] * (s[h] - tq) * invd;
        dsum[h] += d[h];
      }
      d[9] = d[10] = d[11] = 0.f;
      float4* drow = reinterpret_cast<float4*>(dl + (size_t)(base + t) * HP);
#pragma unroll
      for (int c4 = 0; c4 < 3; ++c4)
        if (k == (c4 % G)) drow[c4] = make_float4(d[4 * c4], d[4 * c4 + 1], d[4 * c4 + 2], d[4 * c4 + 3]);
    }
    wave_lds_sync();
  }
  if (!valid) return;
  if (k == 0) {
    float4* a = reinterpret_cast<float4*>(dpn + (size_t)node * HP);
    a[0] = make_float4(dsum[0], dsum[1], dsum[2], dsum[3]);
    a[1] = make_float4(dsum[4], dsum[5], dsum[6], dsum[7]);
    a[2] = make_float4(dsum[8], 0.f, 0.f, 0.f);
    float4* b = reinterpret_cast<float4*>(dcs + (size_t)node * ld_dcs);
    b[0] = make_float4(dsum[0] + dself[0], dsum[1] + dself[1], dsum[2] + dself[2], dsum[3] + dself[3]);
    b[1] = make_float4(dsum[4] + dself[4], dsum[5] + dself[5], dsum[6] + dself[6], dsum[7] + dself[7]);
    b[2] = make_float4(dsum[8] + dself[8], 0.f, 0.f, 0.f);
  }
}

// dp_j = sum over out-edges (j -> i) of dl_ij  -  dpn_j, written into the tail columns of r'
__global__ void feast_dp_gather_kernel(const int* __restrict__ rowptr_out, const int* __restrict__ pos_in,
                                       const float* __restrict__ dl, const float* __restrict__ dpn, int N,
                                       float* __restrict__ rp, int ldr, int col0) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  int n = t / 3, q = t % 3;   // three float4 chunks per node
  if (n >= N) return;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  int rs = rowptr_out[n], re = rowptr_out[n + 1];
#pragma unroll 4
  for (int e = rs; e < re; ++e) {
    float4 v = reinterpret_cast<const float4*>(dl + (size_t)pos_in[e] * HP)[q];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  float4 m = reinterpret_cast<const float4*>(dpn + (size_t)n * HP)[q];
  s.x -= m.x; s.y -= m.y; s.z -= m.z; s.w -= m.w;
  reinterpret_cast<float4*>(rp + (size_t)n * ldr + col0)[q] = s;
}

// Level-0 layers (per-edge logits): the attention-weight gradient is formed per edge as well,
//   du[h,k] = sum over in-edges (j -> i) of dl_e,h (x_j[k] - x_i[k]),      dc[h] = sum_i dcs_i,h,
// the reference's own summation (autograd of u(x_j - x_i)); the node-level form du = dp^T x multiplies by
// coordinates of magnitude ~n and cancels afterwards.  One thread per target node, fixed-order block and
// grid reductions (deterministic).
template <int LC>
__global__ __launch_bounds__(256) void feast_du_edge_kernel(const float* __restrict__ x, const int* __restrict__ rowptr,
                                                            const int* __restrict__ col, const float* __restrict__ dl,
                                                            const float* __restrict__ dcs, int ld_dcs, int N,
                                                            float* __restrict__ partial) {
  // LP = LC / 3 lanes per node, 3 input channels (27 accumulators) each; 256 / LP nodes per block
  constexpr int LP = LC / 3;
  constexpr int NV = H * LC + H;
  __shared__ float red[4][NV];
  const int i = blockIdx.x * (256 / LP) + threadIdx.x / LP;
  const int part = threadIdx.x % LP;
  float acc[H][3], dca[H];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    dca[h] = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[h][k] = 0.f;
  }
  if (i < N) {
    const float* xi = x + (size_t)i * LC + 3 * part;
    const float xc[3] = {xi[0], xi[1], xi[2]};
    if (part == 0) load_hp(dcs + (size_t)i * ld_dcs, dca);
    const int rs = rowptr[i], re = rowptr[i + 1];
    for (int e = rs; e < re; ++e) {
      const float* xj = x + (size_t)col[e] * LC + 3 * part;
      float g[H];
      load_hp(dl + (size_t)e * HP, g);
      const float d[3] = {xj[0] - xc[0], xj[1] - xc[1], xj[2] - xc[2]};
#pragma unroll
      for (int h = 0; h < H; ++h)
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[h][k] = fmaf(g[h], d[k], acc[h][k]);
    }
  }
  // lanes with the same `part` hold the same channels: butterfly over the node bits of the lane id only
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int h = 0; h < H; ++h) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float v = acc[h][k];
#pragma unroll
      for (int o = 32; o >= LP; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane < LP) red[wave][h * LC + 3 * lane + k] = v;
    }
    float v = dca[h];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[wave][H * LC + h] = v;
  }
  __syncthreads();
  if (threadIdx.x < NV)
    partial[(size_t)blockIdx.x * NV + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__global__ void feast_du_final_kernel(const float* __restrict__ partial, int blocks, int LCn, int accumulate,
                                      float* __restrict__ du, float* __restrict__ dc) {
  // one wave per output value: lane l adds the partials of blocks l, l + 64, ... in order, then a fixed butterfly
  const int NV = H * LCn + H;
  const int t = blockIdx.x, lane = threadIdx.x;
  float s = 0.f;
  for (int b = lane; b < blocks; b += 64) s += partial[(size_t)b * NV + t];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane != 0) return;
  float* dst = t < H * LCn ? du + t : dc + (t - H * LCn);
  *dst = accumulate ? *dst + s : s;
}

// diagnostic: the softmax's exp alone (tests/test_gpu_kernels.py checks it against fp64)
__global__ void exp_le0_probe_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = exp_le0(x[i]);
}

// ------------------------------------------------------------------------- small helpers
__global__ void pack_wf_kernel(const float* __restrict__ lin_w, int Cin, int Cout, int Kp, float* __restrict__ wf) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= Kp * Cout) return;
  int kk = idx / Cout, o = idx % Cout;
  int h = kk / Cin, k = kk % Cin;
  wf[idx] = (h < H) ? lin_w[((size_t)h * Cout + o) * Cin + k] : 0.f;
}

__global__ void pack_wprime_kernel(const float* __restrict__ lin_w, const float* __restrict__ u_w, int Cin, int Cout,
                                   int ldr, float* __restrict__ wp) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= ldr * Cin) return;
  int r = idx / Cin, k = idx % Cin;
  float v = 0.f;
  if (r < H * Cout) v = lin_w[(size_t)r * Cin + k];
  else if (r < H * Cout + H) v = u_w[(size_t)(r - H * Cout) * Cin + k];
  wp[idx] = v;
}

// forward: both packed forms in one launch (the backward's W' costs a second launch otherwise)
__global__ void pack_weights_kernel(const float* __restrict__ lin_w, const float* __restrict__ u_w, int Cin, int Cout,
                                    int Kp, int ldr, float* __restrict__ wf, float* __restrict__ wp) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int nwf = Kp * Cout;
  if (idx < nwf) {
    int kk = idx / Cout, o = idx % Cout;
    int h = kk / Cin, k = kk % Cin;
    wf[idx] = (h < H) ? lin_w[((size_t)h * Cout + o) * Cin + k] : 0.f;
    return;
  }
  idx -= nwf;
  if (idx >= ldr * Cin) return;
  int r = idx / Cin, k = idx % Cin;
  float v = 0.f;
  if (r < H * Cout) v = lin_w[(size_t)r * Cin + k];
  else if (r < H * Cout + H) v = u_w[(size_t)(r - H * Cout) * Cin + k];
  wp[idx] = v;
}

__global__ void lrelu_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ out, float slope, int64_t n,
                                 float* __restrict__ g) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  g[i] = out[i] > 0.f ? gout[i] : gout[i] * slope;
}

// per-edge logits apply when the logit-source rows are an unsplit 6- or 12-channel input
__host__ inline int edge_logit_channels(int Cin, int Cb) { return (Cb == 0 && (Cin == 6 || Cin == 12)) ? Cin : 0; }

template <int MODE>
int launch_aggregate(int C, const FeastIn& in, const int* deg_rowptr, float* out, int ldo, const float* xl, hipStream_t s) {
  const int LC = in.LC;
  if (LC != 0 && LC != 6 && LC != 12) return set_error("feast: per-edge logits take 6 or 12 channels, got %d", LC);
  if (MODE == 0 && LC != 0 && LC != C) return set_error("feast: forward per-edge logits read the layer input");
  // every (C, LC) pair is built for both modes, as it always was: the forward ones with LC != C are behind the check above
  const int rc = dispatch_int<6, 12, 32, 64, 128>(C, [&](auto c) {
    return dispatch_int<0, 6, 12>(LC, [&](auto lc) {
      constexpr int kC = decltype(c)::value, kLC = decltype(lc)::value, kV = kC < 32 ? 3 : 4, kNPW = 64 / (kC / kV);
      feast_aggregate_kernel<kC, kV, MODE, kLC><<<xcd_grid(cdiv(in.N, 4 * kNPW)), 256, 0, s>>>(
          in.xa, in.xb, in.Ca, in.p, in.cvec, in.rowptr, in.col, deg_rowptr, in.N, out, ldo, xl, in.ul);
      return 0;
    });
  });
  if (rc == kNoCase) return set_error("feast: unsupported channel count %d (supported: 6, 12, 32, 64, 128)", C);
  GEOBI_LAUNCH_OK();
  return 0;
}

// The row pass with lane = edge (feast_dev.h rowpass_edge_node), dz rows read from HBM: the standalone form of what
// the fused backward kernel runs on its LDS tile; used where dz was formed by the plain GEMM (128-channel layers,
// split inputs the fused kernel does not take, GEOBI_FUSED=0).  Four waves x four nodes per block.
template <int C, int LC>
__global__ __launch_bounds__(256, 4) void feast_rowpass_edge_kernel(
    const float* __restrict__ xa, const float* __restrict__ xb, int Ca, const float* __restrict__ p,
    const float* __restrict__ cvec, const int* __restrict__ rowptr, const int* __restrict__ col,
    const float* __restrict__ dz, int ldz, int N, float* __restrict__ dl, float* __restrict__ dpn,
    float* __restrict__ dcs, int ld_dcs, const float* __restrict__ ul) {
  __shared__ __attribute__((aligned(16))) float s_u[LC > 0 ? LC * HP : 4];
  if constexpr (LC > 0) stage_u<LC>(ul, s_u);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int node0 = (xcd_block(blockIdx.x, gridDim.x) * 4 + wave) * 4;
  if (node0 >= N) return;
  const int node = node0 + lane / 16;
  const int zn = node < N ? node : N - 1;
  rowpass_edge_node<C, LC>(dz + (size_t)zn * ldz, xa, xb, Ca, p, cvec, s_u, rowptr, col, N, node,
                                             lane % 16, dl, dpn, dcs, ld_dcs);
}

static Knob g_rowpass_edge{"GEOBI_ROWPASS_EDGE", 1};   // A/B knob

int launch_rowpass(int C, const FeastIn& in, const RowpassLaunch& r, hipStream_t s) {
  // lane = edge form unless the first input part of a split row ends off a 16-channel batch boundary; the per-edge
  // logit layers (LC > 0: level 0, normally inside the fused kernel) keep the older form here
  const bool edge = g_rowpass_edge.on() && in.LC == 0 && (in.Ca >= C || (C >= 32 && in.Ca % 16 == 0));
  const int rc = dispatch_int<6, 12, 32, 64, 128>(C, [&](auto c) {
    constexpr int kC = decltype(c)::value, kV = kC < 32 ? 3 : 4, kNPW = 64 / (kC / kV);
    auto with_args = [&](auto&& go) {
      go(in.xa, in.xb, in.Ca, in.p, in.cvec, in.rowptr, in.col, r.dz, r.ldz, in.N, r.dl, r.dpn, r.dcs, r.ld_dcs, in.ul);
    };
    const int blocks = xcd_grid(cdiv(in.N, 4 * kNPW));
    if (edge) {
      with_args([&](auto... a) { feast_rowpass_edge_kernel<kC, 0><<<xcd_grid(cdiv(in.N, 16)), 256, 0, s>>>(a...); });
      return 0;
    }
    if constexpr (kC <= 12) {      // per-edge logits: from the layer's own 6 / 12-channel input
      if (in.LC) {
        with_args([&](auto... a) { feast_rowpass_kernel<kC, kV, kC><<<blocks, 256, 0, s>>>(a...); });
        return 0;
      }
    }
    with_args([&](auto... a) { feast_rowpass_kernel<kC, kV, 0><<<blocks, 256, 0, s>>>(a...); });
    return 0;
  });
  if (rc == kNoCase) return set_error("feast: unsupported channel count %d", C);
  GEOBI_LAUNCH_OK();
  return 0;
}

// p = the node-level logits of the layer input
int launch_logits(int C, const FeastIn& in, float* p, hipStream_t s) {
  int rc;
  if (C >= 32 && in.Ca % (C / 16) == 0) {            // a lane's channels never straddle the two input parts
    rc = dispatch_int<32, 64, 128>(C, [&](auto c) {
      feast_logits_group_kernel<decltype(c)::value><<<cdiv(in.N, 16), 256, 0, s>>>(in.xa, in.xb, in.Ca, in.ul, in.N, p);
      return 0;
    });
  } else {
    rc = dispatch_int<6, 12, 32, 64, 128>(C, [&](auto c) {
      feast_logits_kernel<decltype(c)::value><<<cdiv(in.N, 256), 256, 0, s>>>(in.xa, in.xb, in.Ca, in.ul, in.N, p);
      return 0;
    });
  }
  if (rc == kNoCase) return set_error("feast: unsupported channel count %d", C);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // namespace

int feast_ldz(int Cin) { return (H * Cin + 3) / 4 * 4; }
int feast_ldr(int Cout) { return H * Cout + 2 * HP; }   // [r | dp(12) | dcs(12)]

// algorithmic bytes of one aggregation launch (B_agg with z written out)
double feast_agg_bytes(int64_t N, int64_t E, int C, int ld_out) {
  return (double)E * (4.0 + 4.0 * C + 4.0 * H) + 4.0 * (double)N * H + 4.0 * (double)(N + 1) +
         4.0 * (double)N * ld_out;
}

namespace {
// fused (z never reaches HBM): the fragment-ordered forward weights.  Unfused: the packed weights Wf and the split-K
// slices of the node GEMM.  own_weights: the caller supplied no buffer for the weights, they live here
struct FwdBuffers { float *bf, *wf; SubWs gemm; };
FwdBuffers carve_fwd(Arena& a, int64_t N, int Cin, int Cout, bool fused, bool own_weights) {
  const int Kp = feast_ldz(Cin);
  if (fused) return {own_weights ? a.take<float>(feast_fused_fwd_pack_floats(Cin, Cout)) : nullptr, nullptr, {nullptr, 0}};
  return {nullptr, own_weights ? a.take<float>((size_t)Kp * Cout) : nullptr,
          a.take_ws(gemm_nn_fixed_ws_bytes(N, Cout, feast_fwd_slices(Kp, Cout)))};
}
}  // namespace

// either path, with the weights in the workspace (the caller does not say which)
size_t feast_fwd_ws_bytes(int64_t N, int Cin, int Cout) {
  return std::max(carve_bytes([&](Arena& a) { carve_fwd(a, N, Cin, Cout, false, true); }),
                  carve_bytes([&](Arena& a) { carve_fwd(a, N, Cin, Cout, true, true); }));
}

int feast_fwd(const float* xa, const float* xb, int Ca, int Cb, int64_t N, int64_t Ecap, const int32_t* rowptr_in,
              const int32_t* col_in, const float* lin_w, const float* u_w, const float* cvec, const float* bias,
              int Cout, float slope, float* out, float* p, float* z, float* wf_out, void* ws, size_t ws_bytes,
              hipStream_t s, const float* bf_packed) {
  // bf_packed (fused path): the layer's fragment-ordered forward weights, packed by the caller (feast_fused_pack_batch,
  // one launch for a branch's eight layers); with wf_out also given, wf_out holds every form already.
  const int Cin = Ca + Cb;
  GEOBI_REQUIRE(N > 0 && N < (1ll << 31), "feast_fwd: bad node count");
  GEOBI_REQUIRE(Cb == 0 || Ca == Cb, "feast_fwd: a split input must have two equal halves");
  const int Kp = feast_ldz(Cin);
  const bool fused = z == nullptr;
  const bool own_weights = wf_out == nullptr && !(fused && bf_packed != nullptr);
  Arena a(ws, ws_bytes);
  const FwdBuffers fb = carve_fwd(a, N, Cin, Cout, fused, own_weights);
  FeastIn in;
  in.xa = xa;
  in.xb = xb ? xb : xa;
  in.Ca = Cb ? Ca : Cin;
  in.p = p;
  in.cvec = cvec;
  in.rowptr = rowptr_in;
  in.col = col_in;
  in.N = (int)N;
  in.LC = edge_logit_channels(Cin, Cb);      // level-0 layers: logits per edge from the raw rows, no p
  in.ul = u_w;
  if (!fused || own_weights) GEOBI_WS_CHECK("feast_fwd", a, ws, ws_bytes);      // else nothing is taken
  if (fused) {
    // Fused path: aggregation + node transform in one kernel, z never reaches HBM (feast_fused.hip).
    const size_t plain = feast_wpack_plain_floats(Cin, Cout);
    const float* bf = bf_packed;
    if (bf == nullptr) bf = wf_out ? wf_out + plain : fb.bf;
    if (bf_packed != nullptr) {
      // packed by the caller
    } else if (wf_out != nullptr) {      // + the backward's packed forms (Wf for dz, the fused dx weights), one launch
      float* bfw = wf_out + plain;
      GEOBI_TRY(feast_fused_pack_all(lin_w, u_w, cvec, Cin, Cout, Kp, wf_out, bfw,
                                     bfw + feast_fused_fwd_pack_floats(Cin, Cout), s));
    } else {
      GEOBI_TRY(feast_fused_pack_fwd(lin_w, cvec, Cin, Cout, const_cast<float*>(bf), s));
    }
    if (in.LC == 0) GEOBI_TRY(launch_logits(Cin, in, p, s));
    prof_begin_launch(PROF_AGG_FWD, s, feast_fused_bytes(N, Ecap, Cin, Cout), Cin * 1000 + Cout);   // ONE launch: feast_fused_kernel
    int rcf = feast_fused_fwd(in, Cin, bf, Cout, bias, slope, out, s);
    prof_end(PROF_AGG_FWD, s);
    return rcf;
  }
  float* wf = wf_out ? wf_out : fb.wf;   // packed weights, kept for the backward
  if (wf_out != nullptr) {     // kept for the backward: Wf and W' side by side
    const int ldr_ = feast_ldr(Cout);
    pack_weights_kernel<<<cdiv((int64_t)Kp * Cout + (int64_t)ldr_ * Cin, 256), 256, 0, s>>>(
        lin_w, u_w, Cin, Cout, Kp, ldr_, wf, wf + (size_t)Kp * Cout);
  } else {
    pack_wf_kernel<<<cdiv((int64_t)Kp * Cout, 256), 256, 0, s>>>(lin_w, Cin, Cout, Kp, wf);
  }
  GEOBI_LAUNCH_OK();
  if (in.LC == 0) GEOBI_TRY(launch_logits(Cin, in, p, s));
  prof_begin(PROF_AGG_FWD, s, feast_agg_bytes(N, Ecap, Cin, Kp), Cin);
  int rc = launch_aggregate<0>(Cin, in, nullptr, z, Kp, xa, s);
  prof_end(PROF_AGG_FWD, s);
  GEOBI_TRY(rc);
  GemmEpilogue ep;
  ep.bias = bias;
  ep.slope = slope;
  ep.ws = fb.gemm.p;
  ep.ws_bytes = fb.gemm.bytes;
  ep.fixed_slices = feast_fwd_slices(Kp, Cout);      // shape-only split: batching-invariant forward results
  GEOBI_TRY(gemm_nn(z, Kp, wf, Cout, 0, out, Cout, (int)N, Cout, Kp, ep, s));
  return 0;
}

struct BwdPlan {
  float *g, *wf, *dz, *dl, *dpn, *rp, *wp, *z, *bdx, *dpd;
  void *tn_ws, *tn_ws2, *tn_ws3, *gemm_ws;
  size_t tn_bytes, tn_bytes2, tn_bytes3, gemm_bytes;
};

// need_dz: dz [N, 9 Cin] goes through HBM (no fused row pass for this shape);  need_z: z is recomputed here (fused
// forward, no input gradient wanted).  The two [N, 9 Cin] arrays are most of a big layer's workspace (2 x 189 MB at
// 82 k nodes and 64 channels): callers that know the path ask for what it needs (feast_bwd_ws_bytes_for).
static void plan_bwd(Arena& a, int64_t N, int64_t Ecap, int Cin, int Cout, bool need_dz, bool need_z, BwdPlan& b) {
  const int Kp = feast_ldz(Cin), ldr = feast_ldr(Cout);
  b.g = a.take<float>((size_t)N * Cout);
  b.wf = a.take<float>((size_t)Kp * Cout);
  b.dz = a.take<float>(need_dz ? (size_t)N * Kp : 4);
  b.dl = a.take<float>((size_t)(Ecap > 0 ? Ecap : 1) * HP);
  b.dpn = a.take<float>((size_t)N * HP);
  b.rp = a.take<float>((size_t)N * ldr);
  b.wp = a.take<float>((size_t)ldr * Cin);
  b.z = a.take<float>(need_z ? (size_t)N * Kp : 4);          // fused forward, no dx wanted: z is recomputed here
  b.dpd = a.take<float>((size_t)N * 2 * HP);                 // fused: compact [dp | dcs]
  b.tn_bytes3 = 0;                                           // fused: x^T r' (per half for split inputs: fewer
  for (int rows : {Cin + 1, Cin, Cin / 2 + 1, Cin / 2}) {    // output tiles get more slabs)
    if (rows < 1) continue;
    const size_t t = gemm_tn_ws_bytes(rows, ldr, N);
    if (t > b.tn_bytes3) b.tn_bytes3 = t;
  }
  b.tn_ws3 = a.take_ws(b.tn_bytes3).p;
  b.bdx = a.take<float>(feast_fused_dx_pack_floats(Cin, Cout));
  b.tn_bytes = gemm_tn_ws_bytes(Kp + 1, Cout, N);           // [z | 1]^T g   (side stream)
  b.tn_ws = a.take_ws(b.tn_bytes).p;
  b.tn_bytes2 = gemm_tn_ws_bytes_any_width(2 * HP, Cin + 1, N);   // [dp | dcs]^T [x | 1], per input half
  if (b.tn_bytes2 < (size_t)2048 * (128 + H) * sizeof(float) + 256) b.tn_bytes2 = (size_t)2048 * (128 + H) * sizeof(float) + 256;
  {                                                               // or the per-edge du / dc partials (level 0)
    const size_t du_bytes = align_up((size_t)cdiv(N, 64) * (H * Cin + H) * sizeof(float)) + 256;
    if ((Cin == 6 || Cin == 12) && du_bytes > b.tn_bytes2) b.tn_bytes2 = du_bytes;
  }
  b.tn_ws2 = a.take_ws(b.tn_bytes2).p;
  size_t g1 = need_dz ? gemm_nn_ws_bytes(N, Kp) : 0, g2 = gemm_nn_ws_bytes(N, Cin);
  b.gemm_bytes = g1 > g2 ? g1 : g2;
  b.gemm_ws = a.take_ws(b.gemm_bytes).p;
}

static Knob g_rowpass_fused{"GEOBI_ROWPASS_FUSED", 1};

// what feast_bwd will take from its workspace, from the same facts it decides its path with
static void bwd_needs(int Cin, int Cb, int Cout, bool fused, bool need_dx, bool& need_dz, bool& need_z) {
  need_dz = !(fused && g_rowpass_fused.on() && feast_rowpass_fused_supported(Cin, Cb, Cout));
  need_z = fused && !need_dx;
}

// any path (the C ABI's query: the caller does not say which)
size_t feast_bwd_ws_bytes(int64_t N, int64_t Ecap, int Cin, int Cout) {
  return carve_bytes([&](Arena& a) { BwdPlan b; plan_bwd(a, N, Ecap, Cin, Cout, true, true, b); });
}

// the fused path with this input split and this need for an input gradient (the executor's query)
size_t feast_bwd_ws_bytes_for(int64_t N, int64_t Ecap, int Cin, int Cb, int Cout, bool need_dx) {
  bool need_dz, need_z;
  bwd_needs(Cin, Cb, Cout, true, need_dx, need_dz, need_z);
  return carve_bytes([&](Arena& a) { BwdPlan b; plan_bwd(a, N, Ecap, Cin, Cout, need_dz, need_z, b); });
}

int feast_bwd(const float* xa, const float* xb, int Ca, int Cb, int64_t N, int64_t Ecap, const int32_t* rowptr_in,
              const int32_t* col_in, const int32_t* rowptr_out, const int32_t* col_out, const int32_t* pos_in,
              const float* lin_w, const float* u_w, const float* cvec, int Cout, float slope, const float* out,
              const float* gout, const float* p, const float* z, const float* wf_saved, float* dxa, float* dxb,
              float* dlin_w, float* du_w, float* dc, float* dbias, int accumulate, void* ws, size_t ws_bytes,
              hipStream_t s) {
  const int Cin = Ca + Cb;
  const int Kp = feast_ldz(Cin), ldr = feast_ldr(Cout);
  GEOBI_REQUIRE(N > 0 && N < (1ll << 31), "feast_bwd: bad node count");
  Arena a(ws, ws_bytes);
  BwdPlan b;
  bool need_dz, need_z;
  bwd_needs(Cin, Cb, Cout, z == nullptr, dxa != nullptr, need_dz, need_z);
  plan_bwd(a, N, Ecap, Cin, Cout, need_dz, need_z, b);
  GEOBI_WS_CHECK("feast_bwd", a, ws, ws_bytes);
  const int LC = edge_logit_channels(Cin, Cb);
  FeastIn in;                    // the layer input over the in-CSR
  in.xa = xa;
  in.xb = xb ? xb : xa;
  in.Ca = Cb ? Ca : Cin;
  in.p = p;
  in.cvec = cvec;
  in.rowptr = rowptr_in;
  in.col = col_in;
  in.N = (int)N;
  in.LC = LC;
  in.ul = u_w;
  const int Ca_ = in.Ca;
  // Fused forward (z == NULL): the aggregated rows were never written
  const bool fused = z == nullptr;
  // [dp | dcs]: the tail columns of r' (unfused dx GEMM) or a compact [N, 24] array (fused dx kernel)
  float* dpd = fused ? b.dpd : b.rp + H * Cout;
  const int ld_dpd = fused ? 2 * HP : ldr;
  // packed Wf [Kp, Cout] for dz = g Wf^T
  const float* wf = wf_saved;
  if (wf == nullptr) {     // not kept from the forward: repack
    pack_wf_kernel<<<cdiv((int64_t)Kp * Cout, 256), 256, 0, s>>>(lin_w, Cin, Cout, Kp, b.wf);
    GEOBI_LAUNCH_OK();
    wf = b.wf;
  }
  // One kernel for the first half of the backward when the layer reads <= 64 channels (GEOBI_ROWPASS_FUSED=0: A/B):
  // g, dz (LDS only), row pass.  Otherwise three: leaky-relu backward, dz GEMM (dz [N, 9 Cin] through HBM), row pass.
  const bool rp_fused = !need_dz;
  const float* g = gout;
  if (slope != 1.0f) g = b.g;
  RowpassLaunch row;
  row.gout = gout;
  row.out_act = slope != 1.0f ? out : nullptr;
  row.slope = slope;
  row.Wf = wf;
  row.Kp = Kp;
  row.g_out = b.g;
  row.dz = b.dz;
  row.ldz = Kp;
  row.dl = b.dl;
  row.dpn = b.dpn;
  row.dcs = dpd + HP;
  row.ld_dcs = ld_dpd;
  if (rp_fused) {
    prof_begin(PROF_ROWPASS, s, 0.0, Cin);
    int rcf = feast_rowpass_fused(in, Cin, Cout, row, s);
    prof_end(PROF_ROWPASS, s);
    GEOBI_TRY(rcf);
  } else if (slope != 1.0f) {
    // 1. gradient through the fused leaky-relu
    lrelu_bwd_kernel<<<cdiv(N * Cout, 256), 256, 0, s>>>(gout, out, slope, N * Cout, b.g);
    GEOBI_LAUNCH_OK();
  }
  // Fused + input gradient wanted: every weight gradient comes from ONE product x^T r' on the rows r' the dx
  // kernel forms anyway (dW[h,k,o] = sum_j x_j[k] r_j[h,o]): no z needed.  Without dx (first layer of the vertex
  // branch) z is recomputed by the aggregation kernel for dW = z^T g.
  const bool rform = fused && dxa != nullptr;
  FeastIn gin = in;              // what the dx side walks: the unsplit rows of g [N, Cout] over the transposed graph
  gin.xa = gin.xb = g;
  gin.Ca = Cout;
  gin.rowptr = rowptr_out;
  gin.col = col_out;
  if (fused && !rform) {
    GEOBI_TRY(launch_aggregate<0>(Cin, in, nullptr, b.z, Kp, xa, s));
    z = b.z;
  }
  // 2'. weight + bias gradient [z | 1]^T g: needs only z and g, nothing downstream needs it -> side stream
  Fork fk = fork_side_stream(s);
  if (!rform) {
    TnOutput ow;
    ow.mode = TN_LIN_UNPACK; ow.C = dlin_w; ow.C2 = dbias; ow.Cin = Cin; ow.Cout = Cout; ow.accumulate = accumulate;
    GEOBI_TRY(gemm_tn(z, Kp, g, Cout, N, Kp + 1, Cout, Kp, -1, ow, b.tn_ws, b.tn_bytes, fk.side ? fk.side : s));
  }
  int rc = 0;
  if (!rp_fused) {
    // 2. dz = g Wf^T   ([N, Cout] x [Cout, Kp]; Wf is [Kp, Cout] row-major = B transposed)
    GemmEpilogue ep0;
    ep0.ws = b.gemm_ws;
    ep0.ws_bytes = b.gemm_bytes;
    GEOBI_TRY(gemm_nn(g, Cout, wf, Cout, 1, b.dz, Kp, (int)N, Kp, Cout, ep0, s));
    // 3. row pass: per-edge softmax backward
    prof_begin(PROF_ROWPASS, s, 0.0, Cin);
    rc = launch_rowpass(Cin, in, row, s);
    prof_end(PROF_ROWPASS, s);
    GEOBI_TRY(rc);
  }
  // 6. dp (tail columns of r'), and -- when the input needs a gradient -- r and dx.  The fused dx kernel sums dp
  //    itself over the out-edges it walks anyway; a layer with per-edge logits and no input gradient (the first of each
  //    branch) has no reader of dp at all (du / dc come from dl and dcs)
  if (!rform && (dxa != nullptr || LC == 0)) {
    feast_dp_gather_kernel<<<cdiv(N * 3, 256), 256, 0, s>>>(rowptr_out, pos_in, b.dl, b.dpn, (int)N, dpd, ld_dpd, 0);
    GEOBI_LAUNCH_OK();
  }
  // 7. du = dp^T x and dc = dcs^T 1 in one pass: A = r' tail [dp | dcs], B = [x | 1]; needs the row
  //    pass and dp_gather only -> also off the critical path (side stream, after an event on main)
  if (LC > 0) {
    // per-edge du / dc (see feast_du_edge_kernel); needs dl and dcs only -> side stream as well
    GEOBI_TRY(side_wait_main(fk, s));
    hipStream_t ss = fk.side ? fk.side : s;
    const int blocks = cdiv(N, 256 / (LC / 3));
    float* partial = (float*)b.tn_ws2;
    GEOBI_REQUIRE((size_t)blocks * (H * LC + H) * sizeof(float) <= b.tn_bytes2, "feast_bwd: du workspace too small");
    if (LC == 6)
      feast_du_edge_kernel<6><<<blocks, 256, 0, ss>>>(xa, rowptr_in, col_in, b.dl, dpd + HP, ld_dpd, (int)N, partial);
    else
      feast_du_edge_kernel<12><<<blocks, 256, 0, ss>>>(xa, rowptr_in, col_in, b.dl, dpd + HP, ld_dpd, (int)N, partial);
    GEOBI_LAUNCH_OK();
    feast_du_final_kernel<<<H * LC + H, 64, 0, ss>>>(partial, blocks, LC, accumulate, du_w, dc);
    GEOBI_LAUNCH_OK();
  } else if (!rform) {
    GEOBI_TRY(side_wait_main(fk, s));
    hipStream_t ss = fk.side ? fk.side : s;
    TnOutput ou;
    ou.mode = TN_DU_DC; ou.C = du_w; ou.ldc = Cin; ou.C2 = dc; ou.accumulate = accumulate;
    GEOBI_TRY(gemm_tn(dpd, ld_dpd, xa, Ca_, N, 2 * HP, Ca_ + 1, -1, Ca_, ou, b.tn_ws2, b.tn_bytes2, ss));
    if (Cb) {
      ou.C = du_w + Ca; ou.C2 = nullptr;
      GEOBI_TRY(gemm_tn(dpd, ld_dpd, xb, Cb, N, 2 * HP, Cb + 1, -1, Cb, ou, b.tn_ws2, b.tn_bytes2, ss));
    }
  }
  if (dxa != nullptr && fused) {
    // dx = [r | dp | dcs] W' in one kernel: the transposed aggregation feeds the MFMA tile through LDS
    const float* bdx = b.bdx;
    if (wf_saved != nullptr) {
      bdx = wf_saved + feast_wpack_plain_floats(Cin, Cout) + feast_fused_fwd_pack_floats(Cin, Cout);
    } else {
      GEOBI_TRY(feast_fused_pack_dx(lin_w, u_w, cvec, Cin, Cout, b.bdx, s));
    }
    prof_begin(PROF_AGG_BWD, s, feast_fused_bytes(N, Ecap, Cout, Cin), Cout);
    rc = feast_fused_dx(gin, rowptr_in, pos_in, b.dl, b.dpn, xa, dpd, bdx, Cin, dxa, Ca_, dxb, Cb, b.rp, s);
    prof_end(PROF_AGG_BWD, s);
    GEOBI_TRY(rc);
    // every weight gradient of the layer: [x | 1]^T r' (side stream; du / dc of the per-edge-logit layers come from
    // feast_du_edge_kernel above instead)
    GEOBI_TRY(side_wait_main(fk, s));
    hipStream_t ss = fk.side ? fk.side : s;
    // bias.grad and (node-level layers) c.grad ride along as the column sums of r' (one more logical row of the
    // product, formed on the VALU inside the GEMM: no column-sum kernels, no ones row on the matrix cores)
    TnOutput o;
    o.mode = TN_RPRIME; o.C = dlin_w; o.C3 = LC ? nullptr : du_w;
    o.C2 = dbias; o.C4 = LC ? nullptr : dc; o.extra_row = 1;
    o.Cin = Cin; o.Cout = Cout; o.col0 = 0; o.accumulate = accumulate;
    GEOBI_TRY(gemm_tn(xa, Ca_, b.rp, ldr, N, Ca_ + 1, ldr, -1, -1, o, b.tn_ws3, b.tn_bytes3, ss, Ca_));
    if (Cb) {
      o.col0 = Ca; o.extra_row = 0; o.C2 = nullptr; o.C4 = nullptr;
      GEOBI_TRY(gemm_tn(xb, Cb, b.rp, ldr, N, Cb, ldr, -1, -1, o, b.tn_ws3, b.tn_bytes3, ss));
    }
  } else if (dxa != nullptr) {
    prof_begin(PROF_AGG_BWD, s, feast_agg_bytes(N, Ecap, Cout, H * Cout), Cout);
    rc = launch_aggregate<1>(Cout, gin, rowptr_in, b.rp, ldr, xa, s);
    prof_end(PROF_AGG_BWD, s);
    GEOBI_TRY(rc);
    const float* wp = wf_saved ? wf_saved + (size_t)Kp * Cout : b.wp;
    if (wf_saved == nullptr) {
      pack_wprime_kernel<<<cdiv((int64_t)ldr * Cin, 256), 256, 0, s>>>(lin_w, u_w, Cin, Cout, ldr, b.wp);
      GEOBI_LAUNCH_OK();
    }
    GemmEpilogue ep1;
    ep1.ws = b.gemm_ws;
    ep1.ws_bytes = b.gemm_bytes;
    if (Cb) { ep1.C1 = dxb; ep1.split = Ca; ep1.ldc1 = Cb; }
    GEOBI_TRY(gemm_nn(b.rp, ldr, wp, Cin, 0, dxa, Cb ? Ca : Cin, (int)N, Cin, ldr, ep1, s));
  }
  // the side stream's results (and its scratch) are handed back before the call returns
  GEOBI_TRY(join_side_stream(fk, s));
  return 0;
}

}  // namespace geobi

using namespace geobi;

static int check_channels(const char* fn, int Cin, int Cout) {
  bool in_ok = Cin == 6 || Cin == 12 || Cin == 32 || Cin == 64 || Cin == 128;
  bool out_ok = Cout == 32 || Cout == 64 || Cout == 128;
  if (!in_ok || !out_ok) return set_error("%s: unsupported channels Cin=%d Cout=%d", fn, Cin, Cout);
  return 0;
}

extern "C" {

int geobi_debug_exp_le0(const float* x, float* y, int64_t n, void* stream) {
  GEOBI_NOTNULL(x); GEOBI_NOTNULL(y);
  hipStream_t s = as_stream(stream);
  if (n <= 0) return 0;
  exp_le0_probe_kernel<<<cdiv(n, 256), 256, 0, s>>>(x, y, n);
  GEOBI_LAUNCH_OK();
  return 0;
}

size_t geobi_feast_wpack_floats(int Cin, int Cout) { return feast_wpack_floats(Cin, Cout); }

int geobi_feast_ldz(int Cin) { return feast_ldz(Cin); }
size_t geobi_feast_fwd_ws_bytes(int64_t N, int Cin, int Cout) { return feast_fwd_ws_bytes(N, Cin, Cout); }

int geobi_feast_fwd(const float* xa, const float* xb, int Ca, int Cb, int64_t N, int64_t E,
                    const int32_t* rowptr_in, const int32_t* col_in, const float* lin_w, const float* u_w,
                    const float* c, const float* bias, int Cout, float slope, float* out, float* p, float* z,
                    float* wf, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(N, E);
  GEOBI_NOTNULL(xa); GEOBI_NOTNULL(rowptr_in); GEOBI_NOTNULL(lin_w); GEOBI_NOTNULL(u_w); GEOBI_NOTNULL(c); GEOBI_NOTNULL(bias);
  GEOBI_NOTNULL(out); GEOBI_NOTNULL(p);
  if (Cb > 0) GEOBI_NOTNULL(xb);
  if (E > 0) GEOBI_NOTNULL(col_in);
  GEOBI_TRY(check_channels(__func__, Ca + Cb, Cout));
  return feast_fwd(xa, Cb > 0 ? xb : nullptr, Ca, Cb, N, E, rowptr_in, col_in, lin_w, u_w, c, bias, Cout, slope, out,
                   p, z, wf, ws, ws_bytes, as_stream(stream));
}

size_t geobi_feast_bwd_ws_bytes(int64_t N, int64_t E, int Cin, int Cout) { return feast_bwd_ws_bytes(N, E, Cin, Cout); }

int geobi_feast_bwd(const float* xa, const float* xb, int Ca, int Cb, int64_t N, int64_t E,
                    const int32_t* rowptr_in, const int32_t* col_in, const int32_t* rowptr_out,
                    const int32_t* col_out, const int32_t* pos_in, const float* lin_w, const float* u_w,
                    const float* c, int Cout, float slope, const float* out, const float* gout, const float* p,
                    const float* z, const float* wf, float* dxa, float* dxb, float* dlin_w, float* du_w, float* dc,
                    float* dbias, int accumulate, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(N, E);
  GEOBI_NOTNULL(xa); GEOBI_NOTNULL(rowptr_in); GEOBI_NOTNULL(rowptr_out); GEOBI_NOTNULL(lin_w); GEOBI_NOTNULL(u_w); GEOBI_NOTNULL(c);
  GEOBI_NOTNULL(gout); GEOBI_NOTNULL(p); GEOBI_NOTNULL(dlin_w); GEOBI_NOTNULL(du_w); GEOBI_NOTNULL(dc); GEOBI_NOTNULL(dbias);
  if (slope != 1.0f) GEOBI_NOTNULL(out);
  if (Cb > 0) { GEOBI_NOTNULL(xb); if (dxa) GEOBI_NOTNULL(dxb); }
  if (E > 0) { GEOBI_NOTNULL(col_in); GEOBI_NOTNULL(col_out); GEOBI_NOTNULL(pos_in); }
  GEOBI_TRY(check_channels(__func__, Ca + Cb, Cout));
  return feast_bwd(xa, Cb > 0 ? xb : nullptr, Ca, Cb, N, E, rowptr_in, col_in, rowptr_out, col_out, pos_in, lin_w,
                   u_w, c, Cout, slope, out, gout, p, z, wf, dxa, dxb, dlin_w, du_w, dc, dbias, accumulate, ws, ws_bytes,
                   as_stream(stream));
}

}  // extern "C"
