// Bilateral normal filter (Zheng, Fu, Au, Tai: "Bilateral normal filtering for mesh denoising", TVCG 2011, the local
// iterative scheme) over the facet graph: the model-free baseline of the `denoise` command.
//
// The reference has no call site for this: its scratch code only lists result folders of classical filters beside
// its own (code/data_util.py:732-745).
//
//   per face i      cr = (b - a) x (c - a),  A_i = |cr| / 2,  c_i = centroid,  n_i^0 = cr / max(|cr|, 1e-12)
//   N(i)            row i of the loop-free facet graph (faces sharing a vertex, columns ascending) plus i itself
//   one sweep       w_ij = A_j exp(-a |c_i - c_j|^2 - b |n_i - n_j|^2)        a = 1 / (2 sigma_s^2), b = 1 / (2 sigma_r^2)
//                   s_i = sum_j w_ij n_j,  W_i = sum_j w_ij
//                   n_i' = s_i / |s_i| if |s_i| > 1e-6 W_i, else n_i (exact cancellation, all-degenerate neighbourhood)
//   sweeps are Jacobi: every face reads the previous sweep's normals (two buffers, one launch per sweep).
//
// Shape of the sweep kernel
//   lanes      a fixed group of 16 lanes per face (4 faces per wave, 16 per 256-thread block): the group's lanes take the
//              entries t = lane, lane + 16, ... of the row, the face itself being entry `deg`.  Facet degrees are 12-13 on
//              the spheres (one pass of the group), 8-40 on scans (1-3 passes), 199 on a fan's hub (13 passes) -- one lane
//              per face would serialise those and diverge inside the wave.  The four partial sums are folded by an xor
//              butterfly over the 16 lanes (8, 4, 2, 1): a fixed shape, so the bits do not depend on timing, and every lane
//              of the group ends with the same sums.  No atomics, no LDS.
//   spatial    A_j exp(-a d^2) does not change between sweeps: bnf_spatial_kernel writes it once per call into a per-edge
//              array of the workspace, and a sweep reads 4 bytes per entry coalesced (the lanes of a group walk
//              consecutive edges).  Recomputing it in every sweep from a second 16-byte gather of the neighbour's
//              (cx, cy, cz, A) row was measured beside it: the same time at F = 20 480, 8 % more at F = 151 380
//              (profiles/filter_bnf.txt), so that form is not kept.
//   gathers    the neighbour's normal is a 16-byte row (nx, ny, nz, .): one gather per entry and sweep
//   exp        one per entry and sweep: feast_dev::exp_le0 (v_exp_f32 on fl(x log2 e) plus a first-order correction of
//              the product's rounding: <= 2 ulp against exp for finite x <= 0, results below 2^-126 flush to 0).  The
//              arguments -a d^2 and -b |dn|^2 are never positive and formed from DIFFERENCES (translation-invariant).
//   a          read from device memory (sigma_s comes from the mesh's mean centroid distance and never visits the host)
#include "common.h"
#include "../../include/geobi_hip.h"
#include "feast_dev.h"

namespace geobi {

namespace {

constexpr int kLanes = 16;                          // lanes per face
constexpr int kThreads = 256;
constexpr int kFacesPerBlock = kThreads / kLanes;

__global__ __launch_bounds__(kThreads) void bnf_prepare_kernel(const float* __restrict__ pts, const int* __restrict__ fv,
                                                                int F, float4* __restrict__ rec_c,
                                                                float4* __restrict__ rec_n) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= F) return;
  const int ia = fv[3 * f], ib = fv[3 * f + 1], ic = fv[3 * f + 2];
  double pa[3], e1[3], e2[3], cen[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    pa[k] = pts[3 * (size_t)ia + k];
    const double pb = pts[3 * (size_t)ib + k], pc = pts[3 * (size_t)ic + k];
    e1[k] = pb - pa[k];
    e2[k] = pc - pa[k];
    cen[k] = ((pa[k] + pb) + pc) / 3.0;
  }
  const double cx = e1[1] * e2[2] - e1[2] * e2[1];
  const double cy = e1[2] * e2[0] - e1[0] * e2[2];
  const double cz = e1[0] * e2[1] - e1[1] * e2[0];
  const double len = sqrt(cx * cx + cy * cy + cz * cz);
  const double den = len > 1e-12 ? len : 1e-12;     // a face of exactly zero area starts with the zero vector
  rec_c[f] = make_float4((float)cen[0], (float)cen[1], (float)cen[2], (float)(0.5 * len));
  rec_n[f] = make_float4((float)(cx / den), (float)(cy / den), (float)(cz / den), 0.f);
}

__device__ __forceinline__ float dist2(const float4& p, const float4& q) {
  const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
  return (dx * dx + dy * dy) + dz * dz;
}

// wsp[e] = A_j exp(-a |c_i - c_j|^2) for every edge e = (i, j) of the CSR: the factor that no sweep changes
__global__ __launch_bounds__(kThreads) void bnf_spatial_kernel(const float4* __restrict__ rec_c,
                                                                const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                int F, const float* __restrict__ inv2ss,
                                                                float* __restrict__ wsp) {
  const int face = blockIdx.x * kFacesPerBlock + (threadIdx.x / kLanes);
  if (face >= F) return;
  const int sub = threadIdx.x & (kLanes - 1);
  const float a = inv2ss[0];
  const int r0 = rowptr[face], deg = rowptr[face + 1] - r0;
  const float4 ci = rec_c[face];
  for (int t = sub; t < deg; t += kLanes) {
    const float4 cj = rec_c[col[r0 + t]];
    wsp[r0 + t] = cj.w * feast_dev::exp_le0(-(a * dist2(ci, cj)));
  }
}

__global__ __launch_bounds__(kThreads) void bnf_sweep_kernel(const float4* __restrict__ rec_c,
                                                              const float4* __restrict__ nsrc,
                                                              const int* __restrict__ rowptr, const int* __restrict__ col,
                                                              int F, float b, const float* __restrict__ wsp,
                                                              float4* __restrict__ ndst) {
  const int face = blockIdx.x * kFacesPerBlock + (threadIdx.x / kLanes);
  const bool live = face < F;                       // the tail block's spare groups walk the last face and store nothing
  const int f = live ? face : F - 1;
  const int sub = threadIdx.x & (kLanes - 1);
  const int r0 = rowptr[f], deg = rowptr[f + 1] - r0;
  const float area = rec_c[f].w;
  const float4 ni = nsrc[f];
  float sx = 0.f, sy = 0.f, sz = 0.f, sw = 0.f;
  for (int t = sub; t <= deg; t += kLanes) {        // entry `deg` is the face itself
    const bool self = t == deg;
    const int j = self ? f : col[r0 + t];
    const float4 nj = nsrc[j];
    const float spatial = self ? area : wsp[r0 + t];
    const float w = spatial * feast_dev::exp_le0(-(b * dist2(ni, nj)));
    sx += w * nj.x;
    sy += w * nj.y;
    sz += w * nj.z;
    sw += w;
  }
#pragma unroll
  for (int o = kLanes / 2; o > 0; o >>= 1) {        // fixed-shape butterfly inside the face's 16 lanes
    sx += __shfl_xor(sx, o, kLanes);
    sy += __shfl_xor(sy, o, kLanes);
    sz += __shfl_xor(sz, o, kLanes);
    sw += __shfl_xor(sw, o, kLanes);
  }
  if (!live || sub != 0) return;
  const float len = sqrtf((sx * sx + sy * sy) + sz * sz);
  // kept on exact cancellation and when every weight is 0 (and, the comparison being false, on a NaN)
  ndst[f] = len > 1e-6f * sw ? make_float4(sx / len, sy / len, sz / len, 0.f) : make_float4(ni.x, ni.y, ni.z, 0.f);
}

// one buffer of normals (the sweeps alternate between it and `out`) and the per-edge spatial factors
struct BnfBuffers { float4* tmp; float* wsp; };
BnfBuffers carve_bnf(Arena& a, int64_t F, int64_t E) { return {a.take<float4>(F), a.take<float>(E)}; }

}  // namespace

// wsp [E]: the per-edge spatial factors, once per call (guided.hip's sweep reads the same array)
int bnf_spatial_factors(const float* rec_c, const int32_t* rowptr, const int32_t* col, int64_t F, int64_t E,
                        const float* inv2ss, float* wsp, hipStream_t s) {
  if (F == 0 || E == 0) return 0;
  bnf_spatial_kernel<<<cdiv(F, kFacesPerBlock), kThreads, 0, s>>>((const float4*)rec_c, rowptr, col, (int)F, inv2ss, wsp);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // namespace geobi

using namespace geobi;

extern "C" {

int geobi_bnf_prepare(const float* points, const int32_t* fv, int64_t F, int64_t V, float* rec_c, float* rec_n,
                      void* stream) {
  GEOBI_SIZES(F > V ? F : V, 0);
  if (F == 0) return 0;
  GEOBI_NOTNULL(points); GEOBI_NOTNULL(fv); GEOBI_NOTNULL(rec_c); GEOBI_NOTNULL(rec_n);
  hipStream_t s = as_stream(stream);
  if (F == 0) return 0;
  bnf_prepare_kernel<<<cdiv(F, kThreads), kThreads, 0, s>>>(points, fv, (int)F, (float4*)rec_c, (float4*)rec_n);
  GEOBI_LAUNCH_OK();
  return 0;
}

size_t geobi_bnf_filter_ws_bytes(int64_t F, int64_t E) { return carve_bytes([&](Arena& a) { carve_bnf(a, F, E); }); }

int geobi_bnf_filter(const float* rec_c, const float* rec_n, const int32_t* rowptr, const int32_t* col, int64_t F,
                     int64_t E, const float* inv2ss, float inv2sr, int n_sweeps, float* out, void* ws, size_t ws_bytes,
                     void* stream) {
  GEOBI_SIZES(F, E);
  if (F == 0) return 0;
  GEOBI_NOTNULL(rec_c); GEOBI_NOTNULL(rec_n); GEOBI_NOTNULL(rowptr); GEOBI_NOTNULL(inv2ss); GEOBI_NOTNULL(out);
  GEOBI_NOTNULL(ws);
  if (E > 0) GEOBI_NOTNULL(col);
  GEOBI_REQUIRE(n_sweeps >= 0, "bnf_filter: n_sweeps = %d (not negative)", n_sweeps);
  GEOBI_REQUIRE(inv2sr >= 0.f && inv2sr <= 3.0e38f, "bnf_filter: inv2sr = %g (finite and not negative)", (double)inv2sr);
  GEOBI_REQUIRE(out != rec_n && out != rec_c, "bnf_filter: out aliases a record array");
  hipStream_t s = as_stream(stream);
  if (F == 0) return 0;
  if (n_sweeps == 0) {
    GEOBI_HIP(hipMemcpyAsync(out, rec_n, (size_t)F * sizeof(float4), hipMemcpyDeviceToDevice, s));
    return 0;
  }
  Arena a(ws, ws_bytes);
  const BnfBuffers b = carve_bnf(a, F, E);
  GEOBI_WS_CHECK("bnf_filter", a, ws, ws_bytes);
  const int blocks = cdiv(F, kFacesPerBlock);
  GEOBI_TRY(bnf_spatial_factors(rec_c, rowptr, col, F, E, inv2ss, b.wsp, s));
  const float4* src = (const float4*)rec_n;
  for (int k = 1; k <= n_sweeps; ++k) {
    float4* dst = ((n_sweeps - k) & 1) ? b.tmp : (float4*)out;     // the last sweep lands in `out`
    bnf_sweep_kernel<<<blocks, kThreads, 0, s>>>((const float4*)rec_c, src, rowptr, col, (int)F, inv2sr, b.wsp, dst);
    GEOBI_LAUNCH_OK();
    src = dst;
  }
  return 0;
}

}  // extern "C"
