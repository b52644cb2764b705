// Synthetic mesh noise drawn on the device: out[v] = points[v] + displacement(v).
//
// The reference has no call site for this: its training data is an external download (README.md:7) and its noise
// generator is not in its tree.  This kernel is what lets `train` run from clean meshes alone, with fresh noise per
// epoch and no host round trip.
//
// Random numbers: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123
// constants), one counter per vertex:
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (v, stream_id, draw, block)
// so a vertex's numbers depend on (seed, stream_id, draw, v) only -- never on the grid shape, the launch order or the
// number of calls.  v is the row index of THIS call.
//
//   word -> uniform   u = ((w >> 9) + 0.5) * 2^-23: exact in fp32, never 0 or 1, so -2 ln u <= 33.3
//   block 0           four standard normals by two Box-Muller pairs, r(u) = sqrt(-2 ln u):
//                     g0 = r(u0) cos(2 pi u1), g1 = r(u0) sin(2 pi u1), g2 = r(u2) cos(2 pi u3), g3 = r(u2) sin(2 pi u3)
//                     with the precise logf / sincosf / sqrtf (no fast intrinsics)
//   block 1, word 0   the impulsive kind's coin: the vertex moves only if u < fraction
//
//   direction 0 (normal)   sigma * g0 * vnormal[v]
//   direction 1 (random)   sigma * g0 * normalize(g1, g2, g3); (0, 0, 1) if that vector has no length
//
// Shape: one thread per vertex, grid-stride; the Philox products through __umulhi; plain vector stores, no atomics, no
// LDS.  ALU-bound (ten rounds, two logs, two sincos) at 12-24 bytes in and 12 bytes out per vertex.  `out` may alias
// `points`: a thread reads its own row before it writes it and touches no other.
#include "common.h"
#include "../../include/geobi_hip.h"
#include "philox.h"

#include <math.h>

namespace geobi {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;                    // 256 CUs x 8 workgroups; the rest by grid stride

__global__ __launch_bounds__(kThreads) void mesh_noise_kernel(const float* points, const float* vnormal, int V, float sigma,
                                                              int kind, int direction, float fraction, uint32_t k0,
                                                              uint32_t k1, uint32_t stream_id, uint32_t draw, float* out) {
#pragma clang fp contract(off)
  for (int v = blockIdx.x * kThreads + threadIdx.x; v < V; v += gridDim.x * kThreads) {
    const size_t o = 3 * (size_t)v;
    const float px = points[o], py = points[o + 1], pz = points[o + 2];
    const U4 w = philox4x32_10((uint32_t)v, stream_id, draw, 0u, k0, k1);
    float s0, c0;
    sincosf(6.283185307179586f * word_uniform(w.y), &s0, &c0);
    const float r0 = sqrtf(-2.0f * logf(word_uniform(w.x)));
    const float a = sigma * (r0 * c0);              // sigma * g0
    float dx, dy, dz;
    if (direction == 0) {
      dx = a * vnormal[o];
      dy = a * vnormal[o + 1];
      dz = a * vnormal[o + 2];
    } else {
      float s1, c1;
      sincosf(6.283185307179586f * word_uniform(w.w), &s1, &c1);
      const float r1 = sqrtf(-2.0f * logf(word_uniform(w.z)));
      const float g1 = r0 * s0, g2 = r1 * c1, g3 = r1 * s1;
      const float len = sqrtf(g1 * g1 + g2 * g2 + g3 * g3);
      const bool flat = !(len > 0.f);
      const float q = flat ? a : a / len;
      dx = flat ? 0.f : q * g1;
      dy = flat ? 0.f : q * g2;
      dz = flat ? q : q * g3;
    }
    bool move = sigma > 0.f;                        // level 0 leaves every bit alone (-0.0 + 0.0 would not)
    if (kind == 1) move = move && word_uniform(philox4x32_10((uint32_t)v, stream_id, draw, 1u, k0, k1).x) < fraction;
    out[o] = move ? px + dx : px;
    out[o + 1] = move ? py + dy : py;
    out[o + 2] = move ? pz + dz : pz;
  }
}

}  // namespace

}  // namespace geobi

using namespace geobi;

extern "C" {

int geobi_mesh_noise(const float* points, const float* vnormal, int64_t V, float sigma, int kind, int direction,
                     float fraction, uint64_t seed, uint32_t stream_id, uint32_t draw, float* out, void* stream) {
  GEOBI_SIZES(V, 0);
  if (V == 0) return 0;
  GEOBI_NOTNULL(points); GEOBI_NOTNULL(out);
  GEOBI_REQUIRE(kind == 0 || kind == 1, "mesh_noise: kind = %d (0 gaussian, 1 impulsive)", kind);
  GEOBI_REQUIRE(direction == 0 || direction == 1, "mesh_noise: direction = %d (0 normal, 1 random)", direction);
  GEOBI_REQUIRE(direction == 1 || vnormal != nullptr, "mesh_noise: vnormal is NULL (direction 0 moves along the vertex normal)");
  GEOBI_REQUIRE(sigma >= 0.f && sigma <= 3.0e38f, "mesh_noise: sigma = %g (finite and not negative)", (double)sigma);
  GEOBI_REQUIRE(fraction >= 0.f && fraction <= 1.f, "mesh_noise: fraction = %g outside [0, 1]", (double)fraction);
  hipStream_t s = as_stream(stream);
  if (V == 0) return 0;
  int blocks = cdiv(V, kThreads);
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  mesh_noise_kernel<<<blocks, kThreads, 0, s>>>(points, vnormal, (int)V, sigma, kind, direction, fraction,
                                                (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), stream_id, draw,
                                                out);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // extern "C"
