// Rigid point-to-point ICP of a disjoint-union batch: the step that brings a result into its ground truth's frame
// (loss_v(..., apply_icp=True) of the reference calls pytorch3d's iterative_closest_point, code/network.py:15,364-367).
// The search is geobi_nearest_parts (dist.hip), unchanged; this file is what follows it in one iteration, per part that
// has not converged:
//
//   moments   sixteen fp64 sums of dx = x - px, dy = y[idx] - py about the part's pivots (its first x row, its first
//             gathered y row): coordinates far from the origin do not cancel
//   solve     Umeyama's closed form from the moments, 3x3 SVD by one-sided Jacobi (icp_solve.h), one thread per part
//   apply     xt = float32(s x R + T) in fp64, rounded once, and the fp64 partials of |s x R + T - y[idx]|^2
//   finish    rmse, the relative change against the step before, the iteration count and the converged flag
//
// No atomics and no order that depends on timing: a part owns blocks (blockIdx.y = the part, blockIdx.x < icp_blocks(rows)),
// each walks the part's rows with a stride of icp_blocks(rows) blocks, block_sum_fp64 folds a block and one thread adds the
// block sums in ascending order (common.h).  The block count and the walk are functions of the part's OWN row count, so a
// part gives the same bits alone and inside a union.  A converged part is frozen: its blocks leave after reading slot 16,
// its state and its xt rows are not written again.  The part tables ride in the kernel arguments (PartTable), kMaxParts
// parts per launch; the part pointers were checked once, by the entry point (parts_check).
#include "common.h"
#include "../../include/geobi_hip.h"
#include "icp_solve.h"

namespace geobi {

namespace {

constexpr int kThreads = 256;          // 16 fp64 accumulators are 32 VGPRs: far from the 128 that four waves per SIMD leave
constexpr int kMaxBlocks = 64;         // blocks of one part
constexpr int kRowsPerBlock = 4 * kThreads;

struct IcpJob {
  PartTable<int> x, y;
  int base;                            // first part of this launch: where its state and its partial sums are
};

__host__ __device__ inline int icp_blocks(int rows) {
  const int b = (rows + kRowsPerBlock - 1) / kRowsPerBlock;
  return b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b);
}

__device__ __forceinline__ int clamp_idx(int j, int lo, int hi) { return min(max(j, lo), hi - 1); }

// coordinate b of s v R + T, the one expression both the step and geobi_icp_apply round to float32.  No contraction into
// fused multiply-adds: the compiler would choose them per kernel, and the two kernels must give the same bits
__device__ __forceinline__ double icp_coord(const double* v, const double* st, int b) {
#pragma clang fp contract(off)
  return st[12] * (v[0] * st[b] + v[1] * st[3 + b] + v[2] * st[6 + b]) + st[9 + b];
}

__global__ void icp_init_kernel(double* __restrict__ state, int P, const double* __restrict__ init) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  double* st = state + (size_t)p * kIcpState;
  for (int k = 0; k < kIcpState; ++k) st[k] = 0.0;
  if (init) {
    for (int k = 0; k < 13; ++k) st[k] = init[(size_t)p * 13 + k];
  } else {
    st[0] = st[4] = st[8] = 1.0;
    st[12] = 1.0;
  }
}

// mode 0: out = s x R + T; mode 1: out = s x R^T (the gradient of mode 0 to x for a constant transform)
__global__ __launch_bounds__(kThreads) void icp_transform_kernel(PartTable<int> tab, int base, const float* __restrict__ x,
                                                                 const double* __restrict__ state, int mode,
                                                                 float* __restrict__ out) {
  __shared__ int s_x[kMaxParts + 1];
  stage_parts(s_x, tab);
  __syncthreads();
  const int n = tab.n;
  const int i = s_x[0] + blockIdx.x * kThreads + threadIdx.x;
  if (i >= s_x[n]) return;
  const double* st = state + (size_t)(base + find_part(s_x, n, i)) * kIcpState;
  const double s = st[12];
  const double v[3] = {(double)x[3 * (size_t)i], (double)x[3 * (size_t)i + 1], (double)x[3 * (size_t)i + 2]};
  for (int b = 0; b < 3; ++b) {
    double r;
    if (mode == 0) r = icp_coord(v, st, b);
    else r = s * (v[0] * st[3 * b] + v[1] * st[3 * b + 1] + v[2] * st[3 * b + 2]);
    out[3 * (size_t)i + b] = (float)r;
  }
}

__global__ __launch_bounds__(kThreads) void icp_moments_kernel(IcpJob job, const float* __restrict__ x,
                                                               const float* __restrict__ y, const int* __restrict__ idx,
                                                               const double* __restrict__ state,
                                                               double* __restrict__ partial) {
  const int k = blockIdx.y, part = job.base + k;
  if (state[(size_t)part * kIcpState + 16] != 0.0) return;             // frozen (the same answer in every lane)
  const int x_lo = job.x.begin[k], rows = job.x.begin[k + 1] - x_lo;
  const int nb = icp_blocks(rows);
  if ((int)blockIdx.x >= nb) return;
  const int y_lo = job.y.begin[k], y_hi = job.y.begin[k + 1];
  const int j0 = clamp_idx(idx[x_lo], y_lo, y_hi);
  const float px[3] = {x[3 * (size_t)x_lo], x[3 * (size_t)x_lo + 1], x[3 * (size_t)x_lo + 2]};
  const float py[3] = {y[3 * (size_t)j0], y[3 * (size_t)j0 + 1], y[3 * (size_t)j0 + 2]};
  double acc[kIcpMoments];
  for (int a = 0; a < kIcpMoments; ++a) acc[a] = 0.0;
  for (int r = blockIdx.x * kThreads + threadIdx.x; r < rows; r += nb * kThreads) {
    const size_t i = (size_t)(x_lo + r);
    // an index the search wrote lies inside the part; the clamp keeps a foreign array from reading outside y
    const size_t j = (size_t)clamp_idx(idx[i], y_lo, y_hi);
    double dx[3], dy[3];
    for (int a = 0; a < 3; ++a) {
      dx[a] = (double)x[3 * i + a] - (double)px[a];
      dy[a] = (double)y[3 * j + a] - (double)py[a];
    }
    for (int a = 0; a < 3; ++a) {
      acc[a] += dx[a];
      acc[3 + a] += dy[a];
      for (int b = 0; b < 3; ++b) acc[6 + 3 * a + b] += dx[a] * dy[b];
      acc[15] += dx[a] * dx[a];
    }
  }
  double* out = partial + ((size_t)part * kMaxBlocks + blockIdx.x) * kIcpMoments;
  for (int a = 0; a < kIcpMoments; ++a) {
    const double sum = block_sum_fp64<kThreads>(acc[a]);
    if (threadIdx.x == 0) out[a] = sum;
    __syncthreads();                                                   // the tree's LDS is reused by the next sum
  }
}

__global__ void icp_solve_kernel(IcpJob job, const float* __restrict__ x, const float* __restrict__ y,
                                 const int* __restrict__ idx, int flags, double* __restrict__ state,
                                 const double* __restrict__ partial) {
  const int k = threadIdx.x;
  if (k >= job.x.n) return;
  const int part = job.base + k;
  double* st = state + (size_t)part * kIcpState;
  if (st[16] != 0.0) return;
  const int x_lo = job.x.begin[k], rows = job.x.begin[k + 1] - x_lo;
  const int nb = icp_blocks(rows);
  const int j0 = clamp_idx(idx[x_lo], job.y.begin[k], job.y.begin[k + 1]);
  double m[kIcpMoments], px[3], py[3];
  for (int a = 0; a < kIcpMoments; ++a) m[a] = fold_ascending(partial + (size_t)part * kMaxBlocks * kIcpMoments + a, nb, kIcpMoments);
  for (int a = 0; a < 3; ++a) { px[a] = (double)x[3 * (size_t)x_lo + a]; py[a] = (double)y[3 * (size_t)j0 + a]; }
  icp_solve_part(m, px, py, (double)rows, flags, st);
}

__global__ __launch_bounds__(kThreads) void icp_apply_kernel(IcpJob job, const float* __restrict__ x,
                                                             const float* __restrict__ y, const int* __restrict__ idx,
                                                             const double* __restrict__ state, float* __restrict__ xt,
                                                             double* __restrict__ residual) {
  const int k = blockIdx.y, part = job.base + k;
  const double* st = state + (size_t)part * kIcpState;
  if (st[16] != 0.0) return;
  const int x_lo = job.x.begin[k], rows = job.x.begin[k + 1] - x_lo;
  const int nb = icp_blocks(rows);
  if ((int)blockIdx.x >= nb) return;
  const int y_lo = job.y.begin[k], y_hi = job.y.begin[k + 1];
  double tr[13];                                                       // R, T, s: read once
  for (int a = 0; a < 13; ++a) tr[a] = st[a];
  double acc = 0.0;
  for (int r = blockIdx.x * kThreads + threadIdx.x; r < rows; r += nb * kThreads) {
    const size_t i = (size_t)(x_lo + r);
    const size_t j = (size_t)clamp_idx(idx[i], y_lo, y_hi);
    const double v[3] = {(double)x[3 * i], (double)x[3 * i + 1], (double)x[3 * i + 2]};
    for (int b = 0; b < 3; ++b) {
      const double t = icp_coord(v, tr, b);
      const double d = t - (double)y[3 * j + b];
      acc += d * d;
      xt[3 * i + b] = (float)t;
    }
  }
  const double sum = block_sum_fp64<kThreads>(acc);
  if (threadIdx.x == 0) residual[(size_t)part * kMaxBlocks + blockIdx.x] = sum;
}

__global__ void icp_finish_kernel(IcpJob job, double thr, double* __restrict__ state, const double* __restrict__ residual) {
  const int k = threadIdx.x;
  if (k >= job.x.n) return;
  const int part = job.base + k;
  double* st = state + (size_t)part * kIcpState;
  if (st[16] != 0.0) return;
  const int rows = job.x.begin[k + 1] - job.x.begin[k];
  const double rmse = sqrt(fold_ascending(residual + (size_t)part * kMaxBlocks, icp_blocks(rows)) / (double)rows);
  const double prev = st[13], iter = st[15] + 1.0;
  const bool compare = iter >= 2.0 && prev > 0.0;
  const double rel = compare ? (prev - rmse) / prev : 0.0;
  st[13] = rmse;
  st[14] = rel;
  st[15] = iter;
  st[16] = ((compare && rel <= thr) || rmse == 0.0) ? 1.0 : 0.0;
}

// per part and block: the moment sums of the solve, the squared residual of the apply
struct IcpBuffers { double *partial, *residual; };
IcpBuffers carve_icp(Arena& a, int P) {
  const size_t parts = P < 1 ? 0 : P;
  return {a.take<double>(parts * kMaxBlocks * kIcpMoments), a.take<double>(parts * kMaxBlocks)};
}

}  // namespace

}  // namespace geobi

using namespace geobi;

extern "C" {

size_t geobi_icp_ws_bytes(const int64_t* xptr, int P) {
  (void)xptr;
  return carve_bytes([&](Arena& a) { carve_icp(a, P); });
}

int geobi_icp_init(void* state, int P, const double* init, void* stream) {
  GEOBI_REQUIRE(P >= 1, "%s: P = %d parts (at least one)", __func__, P);
  GEOBI_NOTNULL(state);
  hipStream_t s = as_stream(stream);
  icp_init_kernel<<<cdiv(P, 64), 64, 0, s>>>((double*)state, P, init);
  GEOBI_LAUNCH_OK();
  return 0;
}

int geobi_icp_apply(const float* x, const int64_t* xptr, int P, const void* state, int mode, float* out, void* stream) {
  GEOBI_TRY(parts_check(__func__, xptr, xptr, P));
  GEOBI_REQUIRE(mode == 0 || mode == 1, "%s: mode %d (0: s x R + T, 1: s x R^T)", __func__, mode);
  GEOBI_NOTNULL(x); GEOBI_NOTNULL(state); GEOBI_NOTNULL(out);
  hipStream_t s = as_stream(stream);
  for (int base = 0; base < P; base += kMaxParts) {
    PartTable<int> tab;
    fill_parts(&tab, xptr, base, P);
    const int rows = tab.begin[tab.n] - tab.begin[0];
    icp_transform_kernel<<<cdiv(rows, kThreads), kThreads, 0, s>>>(tab, base, x, (const double*)state, mode, out);
  }
  GEOBI_LAUNCH_OK();
  return 0;
}

int geobi_icp_step(const float* x, const float* y, const int32_t* idx, const int64_t* xptr, const int64_t* yptr, int P,
                   int flags, double relative_rmse_thr, void* state, float* xt, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_TRY(parts_check(__func__, xptr, yptr, P));
  GEOBI_REQUIRE((flags & ~3) == 0, "%s: flags %d (bit 0 estimate_scale, bit 1 allow_reflection)", __func__, flags);
  GEOBI_REQUIRE(relative_rmse_thr >= 0.0, "%s: relative_rmse_thr %g is negative", __func__, relative_rmse_thr);
  GEOBI_NOTNULL(x); GEOBI_NOTNULL(y); GEOBI_NOTNULL(idx); GEOBI_NOTNULL(state); GEOBI_NOTNULL(xt); GEOBI_NOTNULL(ws);
  hipStream_t s = as_stream(stream);
  Arena ar(ws, ws_bytes);
  const IcpBuffers b = carve_icp(ar, P);
  GEOBI_WS_CHECK("icp_step", ar, ws, ws_bytes);
  double *st = (double*)state, *partial = b.partial, *residual = b.residual;
  for (int base = 0; base < P; base += kMaxParts) {
    IcpJob job;
    fill_parts(&job.x, xptr, base, P);
    fill_parts(&job.y, yptr, base, P);
    job.base = base;
    int blocks = 1;
    for (int k = 0; k < job.x.n; ++k) {
      const int b = icp_blocks(job.x.begin[k + 1] - job.x.begin[k]);
      if (b > blocks) blocks = b;
    }
    const dim3 grid(blocks, job.x.n);
    icp_moments_kernel<<<grid, kThreads, 0, s>>>(job, x, y, idx, st, partial);
    icp_solve_kernel<<<1, 64, 0, s>>>(job, x, y, idx, flags, st, partial);
    icp_apply_kernel<<<grid, kThreads, 0, s>>>(job, x, y, idx, st, xt, residual);
    icp_finish_kernel<<<1, 64, 0, s>>>(job, relative_rmse_thr, st, residual);
  }
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // extern "C"
