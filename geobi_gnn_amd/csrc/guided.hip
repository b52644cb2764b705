// Guided mesh normal filter (Zhang, Deng, Zhang, Bouaziz, Liu: "Guided Mesh Normal Filtering", Pacific Graphics 2015)
// over the facet graph: the second model-free method of the `denoise` command.  The bilateral filter of filter.hip
// measures its range weight on the noisy normals; this one measures it on a guidance normal g_i, the area-weighted mean
// normal of the most consistent patch that contains face i.
//
// The reference has no call site for this: its scratch code only lists result folders of classical filters beside
// its own (code/data_util.py:732-745).
//
//   records          cr_i, A_i, c_i, n_i^0, the loop-free facet graph (columns ascending) and a = 1 / (2 sigma_s^2) are
//                    filter.hip's; b = 1 / (2 sigma_r^2)
//   patch            P_k = N(k) u {k}: row k of the facet graph plus k (the faces sharing a vertex with k)
//   edge pair        {j, m}, j != m, whose sets of DISTINCT vertex ids have at least 2 ids in common (non-manifold edges,
//                    duplicate faces and faces with a repeated vertex included); one flag per CSR entry, once per call
//   patch measures   Phi_k = max_{j, m in P_k} |n_j - n_m|;  over the edge pairs with both faces in P_k:
//                    R_k = max |n_j - n_m| / (1e-9 + sum |n_j - n_m|) (0 without such a pair);  H_k = Phi_k R_k
//   selection        sel_i = argmin_{k in N(i) u {i}} H_k, ties to the lowest face index
//   guidance         s = sum_{j in P_sel_i} A_j n_j;  g_i = s / |s| if |s| > 1e-6 sum A_j, else n_i
//   sweep (Jacobi)   w_ij = A_j exp(-a |c_i - c_j|^2 - b |g_i - g_j|^2),  s_i = sum_{N(i) u {i}} w_ij n_j,  W_i = sum w_ij,
//                    n_i' = s_i / |s_i| if |s_i| > 1e-6 W_i, else n_i;  H, sel and g are made again in every sweep
//
// Shape of the kernels (three launches per sweep)
//   lanes      the lane groups of filter.hip: 16 lanes per face, 16 faces per 256-thread block, xor butterflies of a fixed
//              shape inside a group, no atomics -- the same input gives the same bits
//   measure    gnf_measure_kernel, the patch search: O(|P_k|^2) normal comparisons per patch.  A group stages its patch
//              (normal | area as one 16-byte row, and the face id) in LDS while |P_k| <= kStage = 64 entries (20 KiB per
//              block); a longer row (a fan's hub patch) takes the same walk with every entry read through the CSR from
//              global memory.  Phi: entry t is compared with the |P_k| / 2 entries that follow it cyclically, which covers
//              every unordered pair once (twice at the opposite entry of an even row; a maximum does not mind).  Edge
//              pairs: a lane walks row j of the CSR for its entry j, takes the flagged entries m > j (each unordered pair
//              once) and looks m up in the ascending row k by bisection -- no dense mark.  The sum of the edge differences
//              is kept in fp64, where a sum of equal fp32 terms is exact in any order: patches that are congruent (a clean
//              CAD shape) get the same bits, so their tie is a tie and goes to the lowest index.  The kernel also writes
//              the patch's guidance candidate (mean normal | valid) as a 16-byte row: every face that selects the patch
//              reads it instead of walking the patch again
//   select     gnf_select_kernel: lexicographic minimum of (H_k, k) over the row (order-independent), one 16-byte gather
//   sweep      gnf_sweep_kernel: filter.hip's sweep with the range term on g; the per-edge spatial factor is the one
//              bnf_spatial_factors writes once per call
#include "common.h"
#include "../../include/geobi_hip.h"
#include "feast_dev.h"

namespace geobi {

namespace {

constexpr int kLanes = 16;                          // lanes per face
constexpr int kThreads = 256;
constexpr int kFacesPerBlock = kThreads / kLanes;
constexpr int kStage = 64;                          // patch entries a group keeps in LDS

__device__ __forceinline__ float dist2(const float4& p, const float4& q) {
  const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
  return (dx * dx + dy * dy) + dz * dz;
}

// flag[e] = 1 when the faces of CSR entry e = (i, j) share at least 2 distinct vertex ids
__global__ __launch_bounds__(kThreads) void gnf_edge_flags_kernel(const int* __restrict__ fv, const int* __restrict__ rowptr,
                                                                   const int* __restrict__ col, int F,
                                                                   uint8_t* __restrict__ flag) {
  const int face = blockIdx.x * kFacesPerBlock + (threadIdx.x / kLanes);
  if (face >= F) return;
  const int sub = threadIdx.x & (kLanes - 1);
  const int r0 = rowptr[face], deg = rowptr[face + 1] - r0;
  const int a0 = fv[3 * face], a1 = fv[3 * face + 1], a2 = fv[3 * face + 2];
  const bool d1 = a1 != a0, d2 = a2 != a0 && a2 != a1;          // a1, a2 count only where they are new ids
  for (int t = sub; t < deg; t += kLanes) {
    const int j = col[r0 + t];
    const int b0 = fv[3 * j], b1 = fv[3 * j + 1], b2 = fv[3 * j + 2];
    const int common = (int)(a0 == b0 || a0 == b1 || a0 == b2) + (int)(d1 && (a1 == b0 || a1 == b1 || a1 == b2)) +
                       (int)(d2 && (a2 == b0 || a2 == b1 || a2 == b2));
    flag[r0 + t] = common >= 2 ? 1 : 0;
  }
}

// Entry t of patch P_k: t < deg is entry t of row k, t == deg is k itself.  Staged: read from the group's LDS rows.
template <bool Staged>
struct Patch {
  const float4* st_n;          // [kStage] normal | area
  const int* st_id;            // [kStage]
  const float4* rec_c;
  const float4* nsrc;
  const int* rowk;             // col + rowptr[k]
  int k, deg;
  __device__ __forceinline__ int id(int t) const {
    if (Staged) return st_id[t];
    return t == deg ? k : rowk[t];
  }
  __device__ __forceinline__ float4 normal_area(int t) const {
    if (Staged) return st_n[t];
    const int j = id(t);
    float4 v = nsrc[j];
    v.w = rec_c[j].w;
    return v;
  }
  // position of face m in the patch, -1 when it is not a member: bisection of the ascending row
  __device__ __forceinline__ int find(int m) const {
    if (m == k) return deg;
    int lo = 0, hi = deg;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (id(mid) < m) lo = mid + 1; else hi = mid;
    }
    return (lo < deg && id(lo) == m) ? lo : -1;
  }
};

struct Partial {
  float mx = 0.f, emax = 0.f, sx = 0.f, sy = 0.f, sz = 0.f, sa = 0.f;
  double esum = 0.0;
};

template <bool Staged>
__device__ __forceinline__ void measure_row(const Patch<Staged>& P, int sub, const int* __restrict__ rowptr,
                                            const int* __restrict__ col, const uint8_t* __restrict__ flag, Partial& r) {
  const int p = P.deg + 1, half = p >> 1;
  for (int t = sub; t < p; t += kLanes) {
    const float4 nj = P.normal_area(t);
    r.sx += nj.w * nj.x;
    r.sy += nj.w * nj.y;
    r.sz += nj.w * nj.z;
    r.sa += nj.w;
    int u = t;
    for (int q = 0; q < half; ++q) {                // the `half` entries after t, cyclically
      u = u + 1 == p ? 0 : u + 1;
      r.mx = fmaxf(r.mx, dist2(nj, P.normal_area(u)));
    }
    const int j = P.id(t);
    const int rj = rowptr[j], dj = rowptr[j + 1] - rj;
    for (int e = 0; e < dj; ++e) {                  // edge pairs {j, m}, m > j, m in P_k
      const int m = col[rj + e];
      if (m <= j || !flag[rj + e]) continue;
      const int pos = P.find(m);
      if (pos < 0) continue;
      const float d = sqrtf(dist2(nj, P.normal_area(pos)));
      r.emax = fmaxf(r.emax, d);
      r.esum += (double)d;
    }
  }
}

__global__ __launch_bounds__(kThreads) void gnf_measure_kernel(const float4* __restrict__ rec_c,
                                                                const float4* __restrict__ nsrc,
                                                                const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                const uint8_t* __restrict__ flag, int F,
                                                                float* __restrict__ H, float4* __restrict__ pmean) {
  __shared__ float4 st_n[kFacesPerBlock][kStage];
  __shared__ int st_id[kFacesPerBlock][kStage];
  const int grp = threadIdx.x / kLanes, sub = threadIdx.x & (kLanes - 1);
  const int face = blockIdx.x * kFacesPerBlock + grp;
  const bool live = face < F;                       // the tail block's spare groups walk the last face and store nothing
  const int k = live ? face : F - 1;
  const int r0 = rowptr[k], deg = rowptr[k + 1] - r0;
  const bool staged = deg + 1 <= kStage;
  if (staged) {
    for (int t = sub; t <= deg; t += kLanes) {
      const int j = t == deg ? k : col[r0 + t];
      float4 v = nsrc[j];
      v.w = rec_c[j].w;
      st_n[grp][t] = v;
      st_id[grp][t] = j;
    }
  }
  __syncthreads();
  Partial r;
  if (staged) {
    const Patch<true> P{st_n[grp], st_id[grp], rec_c, nsrc, col + r0, k, deg};
    measure_row(P, sub, rowptr, col, flag, r);
  } else {
    const Patch<false> P{nullptr, nullptr, rec_c, nsrc, col + r0, k, deg};
    measure_row(P, sub, rowptr, col, flag, r);
  }
#pragma unroll
  for (int o = kLanes / 2; o > 0; o >>= 1) {        // fixed-shape butterfly inside the face's 16 lanes
    r.mx = fmaxf(r.mx, __shfl_xor(r.mx, o, kLanes));
    r.emax = fmaxf(r.emax, __shfl_xor(r.emax, o, kLanes));
    r.esum += __shfl_xor(r.esum, o, kLanes);
    r.sx += __shfl_xor(r.sx, o, kLanes);
    r.sy += __shfl_xor(r.sy, o, kLanes);
    r.sz += __shfl_xor(r.sz, o, kLanes);
    r.sa += __shfl_xor(r.sa, o, kLanes);
  }
  if (!live || sub != 0) return;
  const double phi = (double)sqrtf(r.mx);           // sqrt is monotone: the root of the largest square
  H[k] = (float)(phi * (double)r.emax / (1e-9 + r.esum));
  if (pmean != nullptr) {
    const float len = sqrtf((r.sx * r.sx + r.sy * r.sy) + r.sz * r.sz);
    pmean[k] = len > 1e-6f * r.sa ? make_float4(r.sx / len, r.sy / len, r.sz / len, 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

__device__ __forceinline__ void take_lower(float& bh, int& bk, float h, int k) {
  if (h < bh || (h == bh && k < bk)) {
    bh = h;
    bk = k;
  }
}

__global__ __launch_bounds__(kThreads) void gnf_select_kernel(const float4* __restrict__ nsrc, const int* __restrict__ rowptr,
                                                               const int* __restrict__ col, int F,
                                                               const float* __restrict__ H, const float4* __restrict__ pmean,
                                                               int* __restrict__ sel, float4* __restrict__ g) {
  const int face = blockIdx.x * kFacesPerBlock + (threadIdx.x / kLanes);
  const bool live = face < F;
  const int f = live ? face : F - 1;
  const int sub = threadIdx.x & (kLanes - 1);
  const int r0 = rowptr[f], deg = rowptr[f + 1] - r0;
  float bh = INFINITY;
  int bk = INT_MAX;
  for (int t = sub; t <= deg; t += kLanes) {        // entry `deg` is the face itself
    const int k = t == deg ? f : col[r0 + t];
    take_lower(bh, bk, H[k], k);
  }
#pragma unroll
  for (int o = kLanes / 2; o > 0; o >>= 1) {        // lexicographic minimum of (H, index): the order does not matter
    const float oh = __shfl_xor(bh, o, kLanes);
    const int ok = __shfl_xor(bk, o, kLanes);
    take_lower(bh, bk, oh, ok);
  }
  if (!live || sub != 0) return;
  if (bk == INT_MAX) bk = f;                        // nothing compared (every H a NaN): the face's own patch
  const float4 pm = pmean[bk];
  const float4 ni = nsrc[f];
  g[f] = pm.w != 0.f ? make_float4(pm.x, pm.y, pm.z, 0.f) : make_float4(ni.x, ni.y, ni.z, 0.f);
  if (sel != nullptr) sel[f] = bk;
}

__global__ __launch_bounds__(kThreads) void gnf_sweep_kernel(const float4* __restrict__ rec_c,
                                                              const float4* __restrict__ nsrc, const float4* __restrict__ g,
                                                              const int* __restrict__ rowptr, const int* __restrict__ col,
                                                              int F, float b, const float* __restrict__ wsp,
                                                              float4* __restrict__ ndst) {
  const int face = blockIdx.x * kFacesPerBlock + (threadIdx.x / kLanes);
  const bool live = face < F;
  const int f = live ? face : F - 1;
  const int sub = threadIdx.x & (kLanes - 1);
  const int r0 = rowptr[f], deg = rowptr[f + 1] - r0;
  const float area = rec_c[f].w;
  const float4 gi = g[f];
  float sx = 0.f, sy = 0.f, sz = 0.f, sw = 0.f;
  for (int t = sub; t <= deg; t += kLanes) {        // entry `deg` is the face itself
    const bool self = t == deg;
    const int j = self ? f : col[r0 + t];
    const float4 nj = nsrc[j];
    const float4 gj = g[j];
    const float spatial = self ? area : wsp[r0 + t];
    const float w = spatial * feast_dev::exp_le0(-(b * dist2(gi, gj)));
    sx += w * nj.x;
    sy += w * nj.y;
    sz += w * nj.z;
    sw += w;
  }
#pragma unroll
  for (int o = kLanes / 2; o > 0; o >>= 1) {
    sx += __shfl_xor(sx, o, kLanes);
    sy += __shfl_xor(sy, o, kLanes);
    sz += __shfl_xor(sz, o, kLanes);
    sw += __shfl_xor(sw, o, kLanes);
  }
  if (!live || sub != 0) return;
  const float len = sqrtf((sx * sx + sy * sy) + sz * sz);
  const float4 ni = nsrc[f];
  ndst[f] = len > 1e-6f * sw ? make_float4(sx / len, sy / len, sz / len, 0.f) : make_float4(ni.x, ni.y, ni.z, 0.f);
}

// the two launchers gnf_filter shares with their own entry points
int gnf_edge_flags(const int32_t* fv, const int32_t* rowptr, const int32_t* col, int64_t F, int64_t E, uint8_t* flags,
                   hipStream_t s) {
  if (F == 0 || E == 0) return 0;
  gnf_edge_flags_kernel<<<cdiv(F, kFacesPerBlock), kThreads, 0, s>>>(fv, rowptr, col, (int)F, flags);
  GEOBI_LAUNCH_OK();
  return 0;
}

int gnf_patch_measure(const float* rec_c, const float* normals, const int32_t* rowptr, const int32_t* col,
                      const uint8_t* flags, int64_t F, float* H, float* pmean, hipStream_t s) {
  if (F == 0) return 0;
  gnf_measure_kernel<<<cdiv(F, kFacesPerBlock), kThreads, 0, s>>>((const float4*)rec_c, (const float4*)normals, rowptr, col,
                                                                  flags, (int)F, H, (float4*)pmean);
  GEOBI_LAUNCH_OK();
  return 0;
}

// one buffer of normals (the sweeps alternate between it and `out`), the per-edge spatial factors and edge-pair flags,
// and per face H, the patch means and the guidance normals
struct GnfBuffers { float4 *tmp, *pmean, *g; float *H, *wsp; uint8_t* flags; };
GnfBuffers carve_gnf(Arena& a, int64_t F, int64_t E) {
  return {a.take<float4>(F), a.take<float4>(F), a.take<float4>(F), a.take<float>(F), a.take<float>(E), a.take<uint8_t>(E)};
}

}  // namespace

}  // namespace geobi

using namespace geobi;

extern "C" {

int geobi_gnf_edge_flags(const int32_t* fv, const int32_t* rowptr, const int32_t* col, int64_t F, int64_t E, uint8_t* flags,
                         void* stream) {
  GEOBI_SIZES(F, E);
  if (F == 0 || E == 0) return 0;
  GEOBI_NOTNULL(fv); GEOBI_NOTNULL(rowptr); GEOBI_NOTNULL(col); GEOBI_NOTNULL(flags);
  return gnf_edge_flags(fv, rowptr, col, F, E, flags, as_stream(stream));
}

int geobi_gnf_patch_measure(const float* rec_c, const float* normals, const int32_t* rowptr, const int32_t* col,
                            const uint8_t* flags, int64_t F, int64_t E, float* H, void* stream) {
  GEOBI_SIZES(F, E);
  if (F == 0) return 0;
  GEOBI_NOTNULL(rec_c); GEOBI_NOTNULL(normals); GEOBI_NOTNULL(rowptr); GEOBI_NOTNULL(H);
  if (E > 0) { GEOBI_NOTNULL(col); GEOBI_NOTNULL(flags); }
  if ((const float*)H == rec_c || (const float*)H == normals) return set_error("%s: H aliases an input", __func__);
  return gnf_patch_measure(rec_c, normals, rowptr, col, flags, F, H, nullptr, as_stream(stream));
}

size_t geobi_gnf_filter_ws_bytes(int64_t F, int64_t E) { return carve_bytes([&](Arena& a) { carve_gnf(a, F, E); }); }

int geobi_gnf_filter(const float* rec_c, const float* rec_n, const int32_t* fv, const int32_t* rowptr, const int32_t* col,
                     int64_t F, int64_t E, const float* inv2ss, float inv2sr, int n_sweeps, float* out, int32_t* sel_out,
                     void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(F, E);
  if (F == 0) return 0;
  GEOBI_NOTNULL(rec_c); GEOBI_NOTNULL(rec_n); GEOBI_NOTNULL(fv); GEOBI_NOTNULL(rowptr); GEOBI_NOTNULL(inv2ss);
  GEOBI_NOTNULL(out); GEOBI_NOTNULL(ws);
  if (E > 0) GEOBI_NOTNULL(col);
  GEOBI_REQUIRE(n_sweeps >= 0, "gnf_filter: n_sweeps = %d (not negative)", n_sweeps);
  GEOBI_REQUIRE(inv2sr >= 0.f && inv2sr <= 3.0e38f, "gnf_filter: inv2sr = %g (finite and not negative)", (double)inv2sr);
  GEOBI_REQUIRE(out != rec_n && out != rec_c, "gnf_filter: out aliases a record array");
  hipStream_t s = as_stream(stream);
  if (F == 0) return 0;
  if (n_sweeps == 0) {
    GEOBI_HIP(hipMemcpyAsync(out, rec_n, (size_t)F * sizeof(float4), hipMemcpyDeviceToDevice, s));
    return 0;
  }
  Arena a(ws, ws_bytes);
  const GnfBuffers b = carve_gnf(a, F, E);
  GEOBI_WS_CHECK("gnf_filter", a, ws, ws_bytes);
  const int blocks = cdiv(F, kFacesPerBlock);
  GEOBI_TRY(bnf_spatial_factors(rec_c, rowptr, col, F, E, inv2ss, b.wsp, s));
  GEOBI_TRY(gnf_edge_flags(fv, rowptr, col, F, E, b.flags, s));
  const float4* src = (const float4*)rec_n;
  for (int k = 1; k <= n_sweeps; ++k) {
    float4* dst = ((n_sweeps - k) & 1) ? b.tmp : (float4*)out;     // the last sweep lands in `out`
    GEOBI_TRY(gnf_patch_measure(rec_c, (const float*)src, rowptr, col, b.flags, F, b.H, (float*)b.pmean, s));
    gnf_select_kernel<<<blocks, kThreads, 0, s>>>(src, rowptr, col, (int)F, b.H, b.pmean,
                                                  sel_out ? sel_out + (size_t)(k - 1) * F : nullptr, b.g);
    GEOBI_LAUNCH_OK();
    gnf_sweep_kernel<<<blocks, kThreads, 0, s>>>((const float4*)rec_c, src, b.g, rowptr, col, (int)F, inv2sr, b.wsp, dst);
    GEOBI_LAUNCH_OK();
    src = dst;
  }
  return 0;
}

}  // extern "C"
