// Chamfer distance between predicted and ground-truth vertices of a disjoint-union batch: the value and the gradient
// of loss_v(vp, v, dis='CD') (code/network.py:369-370, kaolin's chamfer_distance with squared distances), on top of the
// two searches of nearest_parts (dist.hip).
//
//   forward   out = sum_p (1/B) [ (1/Q_p) sum_{i in p} d2a_i + (1/M_p) sum_{j in p} d2b_j ]      B = P parts
//   backward  gp_i = gout (2 / (B Q_p)) (p_i - t_a(i)) + gout (2 / (B M_p)) sum_{j : b(j) = i} (p_i - t_j)
//
// Both are free of atomics and of any order that depends on timing.  The sum is fp64 in a fixed order: a grid of a size
// that depends on the row counts only walks the rows with a grid stride, block_sum_fp64 folds a block, one thread adds
// the block sums in ascending order (fold_ascending; both in common.h).  The backward writes every row of gp exactly once: the targets that chose row i
// come from the inverse lists of b (geobi_segment_csr: members ascending), gathered and summed by the row's own lane.
// The part tables ride in the kernel arguments (PartTable, common.h), kMaxParts parts per launch, with the weights.
// The part pointers were checked once, by the entry point (parts_check).
#include "common.h"
#include "../../include/geobi_hip.h"

namespace geobi {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256;

struct ChamferJob {
  PartTable<int> q, t;            // prediction / target rows of part k
  float wq[kMaxParts];            // 1 / (B Q_p), rounded once from fp64
  float wt[kMaxParts];            // 1 / (B M_p)
};

__global__ __launch_bounds__(kThreads) void chamfer_partial_kernel(ChamferJob job, const float* __restrict__ d2a,
                                                                   const float* __restrict__ d2b,
                                                                   double* __restrict__ partial) {
  __shared__ int s_q[kMaxParts + 1], s_t[kMaxParts + 1];
  __shared__ float s_wq[kMaxParts], s_wt[kMaxParts];
  const int n = job.q.n;
  stage_parts(s_q, job.q);
  stage_parts(s_t, job.t);
  for (int k = threadIdx.x; k < n; k += kThreads) { s_wq[k] = job.wq[k]; s_wt[k] = job.wt[k]; }
  __syncthreads();
  const int nq = s_q[n] - s_q[0], nt = s_t[n] - s_t[0];
  double acc = 0.0;
  for (int r = blockIdx.x * kThreads + threadIdx.x; r < nq + nt; r += gridDim.x * kThreads) {
    if (r < nq) {
      const int i = s_q[0] + r;
      acc += (double)s_wq[find_part(s_q, n, i)] * (double)d2a[i];
    } else {
      const int j = s_t[0] + (r - nq);
      acc += (double)s_wt[find_part(s_t, n, j)] * (double)d2b[j];
    }
  }
  const double sum = block_sum_fp64<kThreads>(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

__global__ void chamfer_final_kernel(const double* __restrict__ partial, int n, float* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = (float)fold_ascending(partial, n);
}

__global__ __launch_bounds__(kThreads) void chamfer_bwd_kernel(ChamferJob job, const float* __restrict__ p,
                                                               const float* __restrict__ t, const int* __restrict__ idx_a,
                                                               const int* __restrict__ segptr, const int* __restrict__ members,
                                                               int n_members, const float* __restrict__ gout,
                                                               float* __restrict__ gp) {
  __shared__ int s_q[kMaxParts + 1];
  __shared__ float s_wq[kMaxParts], s_wt[kMaxParts];
  const int n = job.q.n;
  stage_parts(s_q, job.q);
  for (int k = threadIdx.x; k < n; k += kThreads) { s_wq[k] = job.wq[k]; s_wt[k] = job.wt[k]; }
  __syncthreads();
  const int i = s_q[0] + blockIdx.x * kThreads + threadIdx.x;
  if (i >= s_q[n]) return;
  const int part = find_part(s_q, n, i);
  const int t_lo = job.t.begin[0], t_hi = job.t.begin[n];            // uniform: rows this launch may gather
  const float g = gout[0];
  const float px = p[3 * (size_t)i], py = p[3 * (size_t)i + 1], pz = p[3 * (size_t)i + 2];
  // direction a: the row's own nearest target (an index the search wrote: inside the part; the clamp keeps a foreign
  // array from reading outside t)
  const int a = min(max(idx_a[i], t_lo), t_hi - 1);
  const float ca = 2.0f * s_wq[part];
  float gx = ca * (px - t[3 * (size_t)a]), gy = ca * (py - t[3 * (size_t)a + 1]), gz = ca * (pz - t[3 * (size_t)a + 2]);
  // direction b: every target whose nearest prediction is this row, ascending target index
  float sx = 0.f, sy = 0.f, sz = 0.f;
  const int k_end = min(segptr[i + 1], n_members);
  for (int k = max(segptr[i], 0); k < k_end; ++k) {
    const int j = min(max(members[k], t_lo), t_hi - 1);
    sx += px - t[3 * (size_t)j]; sy += py - t[3 * (size_t)j + 1]; sz += pz - t[3 * (size_t)j + 2];
  }
  const float cb = 2.0f * s_wt[part];
  gp[3 * (size_t)i] = g * (gx + cb * sx);
  gp[3 * (size_t)i + 1] = g * (gy + cb * sy);
  gp[3 * (size_t)i + 2] = g * (gz + cb * sz);
}

int partial_blocks(int64_t rows) {
  const int64_t b = (rows + 4 * kThreads - 1) / (4 * kThreads);
  return (int)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

void fill_job(ChamferJob* job, const int64_t* qptr, const int64_t* tptr, int base, int P) {
  fill_parts(&job->q, qptr, base, P);
  fill_parts(&job->t, tptr, base, P);
  for (int k = 0; k < kMaxParts; ++k) {              // the unused tail weighs nothing
    const bool used = k < job->q.n;
    job->wq[k] = used ? (float)(1.0 / ((double)P * (double)(job->q.begin[k + 1] - job->q.begin[k]))) : 0.f;
    job->wt[k] = used ? (float)(1.0 / ((double)P * (double)(job->t.begin[k + 1] - job->t.begin[k]))) : 0.f;
  }
}

// the block sums of every launch (kMaxParts parts each)
double* carve_partials(Arena& a, int P) {
  const int launches = P < 1 ? 0 : (P + kMaxParts - 1) / kMaxParts;
  return a.take<double>((size_t)launches * kMaxBlocks);
}

}  // namespace

}  // namespace geobi

using namespace geobi;

extern "C" {

size_t geobi_chamfer_ws_bytes(int P) { return carve_bytes([&](Arena& a) { carve_partials(a, P); }); }

int geobi_chamfer_fwd(const float* d2a, const float* d2b, const int64_t* qptr, const int64_t* tptr, int P, float* out,
                      void* ws, size_t ws_bytes, void* stream) {
  GEOBI_TRY(parts_check(__func__, qptr, tptr, P));
  GEOBI_NOTNULL(d2a); GEOBI_NOTNULL(d2b); GEOBI_NOTNULL(out); GEOBI_NOTNULL(ws);
  hipStream_t s = as_stream(stream);
  Arena ar(ws, ws_bytes);
  double* partial = carve_partials(ar, P);
  GEOBI_WS_CHECK("chamfer_fwd", ar, ws, ws_bytes);
  int used = 0;
  for (int base = 0; base < P; base += kMaxParts) {
    ChamferJob job;
    fill_job(&job, qptr, tptr, base, P);
    const int64_t rows = (int64_t)(job.q.begin[job.q.n] - job.q.begin[0]) + (job.t.begin[job.t.n] - job.t.begin[0]);
    const int blocks = partial_blocks(rows);
    chamfer_partial_kernel<<<blocks, kThreads, 0, s>>>(job, d2a, d2b, partial + used);
    used += blocks;
  }
  chamfer_final_kernel<<<1, 64, 0, s>>>(partial, used, out);
  GEOBI_LAUNCH_OK();
  return 0;
}

int geobi_chamfer_bwd(const float* p, const float* t, const int32_t* idx_a, const int32_t* segptr, const int32_t* members,
                      const int64_t* qptr, const int64_t* tptr, int P, const float* gout, float* gp, void* stream) {
  GEOBI_TRY(parts_check(__func__, qptr, tptr, P));
  GEOBI_NOTNULL(p); GEOBI_NOTNULL(t); GEOBI_NOTNULL(idx_a); GEOBI_NOTNULL(segptr); GEOBI_NOTNULL(members);
  GEOBI_NOTNULL(gout); GEOBI_NOTNULL(gp);
  GEOBI_REQUIRE(qptr[0] == 0 && tptr[0] == 0, "chamfer_bwd: qptr / tptr start at %lld / %lld (the inverse lists are indexed by "
                "the rows themselves: both 0)", (long long)qptr[0], (long long)tptr[0]);
  hipStream_t s = as_stream(stream);
  for (int base = 0; base < P; base += kMaxParts) {
    ChamferJob job;
    fill_job(&job, qptr, tptr, base, P);
    const int rows = job.q.begin[job.q.n] - job.q.begin[0];
    chamfer_bwd_kernel<<<cdiv(rows, kThreads), kThreads, 0, s>>>(job, p, t, idx_a, segptr, members, (int)tptr[P], gout, gp);
  }
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // extern "C"
