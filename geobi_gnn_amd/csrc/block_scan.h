// Block-wide exclusive int scan in pieces (device only): the wave ladder, the fold of the wave sums through LDS, and the
// load / store of a thread's chunk of consecutive ints.  scan.hip builds the library's scan kernels from them and match.hip
// the scan-free matching pair.  patch.hip's grow_wave_scan is the same ladder, so it calls wave_inclusive_scan; what it
// adds (the total by a lane-63 broadcast, the exclusive value) stays there.  Blocks are 64 * WAVES threads wide, one
// dimension; s_wave arrays have WAVES entries per list and are indexed by threadIdx.x >> 6.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace geobi {

// inclusive prefix of v over the lanes 0 .. lane of the wave: six __shfl_up steps
__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}

// LISTS independent scans over the block with ONE barrier between them all: ex[l] = sum of v[l] over the threads before
// this one, total[l] = over the whole block.  s_wave is read after the barrier and not fenced again: the caller passes
// another buffer to the next call (the walking kernels alternate two), or has a barrier of its own in between.
template <int WAVES, int LISTS>
__device__ __forceinline__ void block_exclusive_scan_lists(const int (&v)[LISTS], int (*s_wave)[WAVES], int (&ex)[LISTS],
                                                           int (&total)[LISTS]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc[LISTS];
#pragma unroll
  for (int l = 0; l < LISTS; ++l) inc[l] = wave_inclusive_scan(v[l], lane);
  if (lane == 63) {
#pragma unroll
    for (int l = 0; l < LISTS; ++l) s_wave[l][wave] = inc[l];
  }
  __syncthreads();
#pragma unroll
  for (int l = 0; l < LISTS; ++l) {
    int off = 0, tot = 0;                 // a running total over the waves, caught where it reaches this one
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      if (w == wave) off = tot;
      tot += s_wave[l][w];
    }
    ex[l] = off + inc[l] - v[l];
    total[l] = tot;
  }
}

// One list: returns the exclusive prefix of v inside the block and the block total.  REUSE: a second barrier behind the
// fold, so that s_wave (WAVES ints) may be written again at once -- the matching pair scans twice through one array.
// Without it the rule of block_exclusive_scan_lists holds.
template <int WAVES, bool REUSE = true>
__device__ __forceinline__ int block_exclusive_scan(int v, int* s_wave, int& total) {
  const int vv[1] = {v};
  int ex[1], tot[1];
  block_exclusive_scan_lists<WAVES, 1>(vv, reinterpret_cast<int(*)[WAVES]>(s_wave), ex, tot);
  if (REUSE) __syncthreads();
  total = tot[0];
  return ex[0];
}

// A thread's EPT consecutive ints in[i0 .. i0 + EPT), EPT a multiple of 4: int4 loads when `vec` (every pointer of the
// kernel 16-byte aligned, i0 a multiple of 4) and the chunk lies inside n, one guarded load per int otherwise (0 behind n).
template <int EPT>
__device__ __forceinline__ void load_chunk(const int* __restrict__ in, int64_t i0, int64_t n, bool vec, int (&v)[EPT]) {
  if (vec && i0 + EPT <= n) {
#pragma unroll
    for (int q = 0; q < EPT / 4; ++q) {
      const int4 t = *reinterpret_cast<const int4*>(in + i0 + 4 * q);
      v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int q = 0; q < EPT; ++q) v[q] = (i0 + q < n) ? in[i0 + q] : 0;
  }
}

template <int EPT>
__device__ __forceinline__ int chunk_sum(const int (&v)[EPT]) {
  int s = 0;
#pragma unroll
  for (int q = 0; q < EPT; ++q) s += v[q];
  return s;
}

// out[i0 + q] = ex + v[0] + ... + v[q - 1] for the q with i0 + q < n: the same rule as load_chunk, nothing written behind n
template <int EPT>
__device__ __forceinline__ void store_chunk(int* __restrict__ out, int64_t i0, int64_t n, bool vec, const int (&v)[EPT],
                                            int ex) {
  if (vec && i0 + EPT <= n) {
#pragma unroll
    for (int q = 0; q < EPT / 4; ++q) {
      int4 t;
      t.x = ex; ex += v[4 * q];
      t.y = ex; ex += v[4 * q + 1];
      t.z = ex; ex += v[4 * q + 2];
      t.w = ex; ex += v[4 * q + 3];
      *reinterpret_cast<int4*>(out + i0 + 4 * q) = t;
    }
  } else {
#pragma unroll
    for (int q = 0; q < EPT; ++q) {
      if (i0 + q < n) out[i0 + q] = ex;
      ex += v[q];
    }
  }
}

}  // namespace geobi
