// THE slicing rule of the all-pairs walks (dist.hip: nearest point / triangle; selfx.hip: self-intersections): a walk's
// workgroups are (query block, slice of the targets); the target set is cut into slices of whole tiles so that a small
// query set still fills the chip.  Host code only; every number is a function of the sizes alone.
#pragma once
#include "common.h"

namespace geobi {

constexpr int kWalkThreads = 256;                   // lanes of a walk's workgroup: a query block is kWalkThreads * qpl queries
constexpr int kTargetBlocks = 1024;                 // workgroups wanted per launch (256 CUs x 4)
constexpr int kMaxSlices = 1024;

struct Slicing { int qblocks, slices, tiles_per_slice; };

// slices a launch with `qblocks` query blocks in all would like: its workgroups together should fill the chip
static inline int want_slices(int64_t qblocks) {
  const int64_t want = (kTargetBlocks + qblocks - 1) / qblocks;
  return (int)(want > kMaxSlices ? kMaxSlices : (want < 1 ? 1 : want));
}

// THE slicing rule: T targets in whole tiles, at most `want` slices, no empty slice
static inline Slicing slice_targets(int64_t Q, int64_t T, int qpl, int tile, int want) {
  Slicing c;
  c.qblocks = cdiv(Q, (int64_t)kWalkThreads * qpl);
  const int ntiles = cdiv(T, tile);
  if (want > ntiles) want = ntiles;
  c.tiles_per_slice = cdiv(ntiles, want);
  c.slices = cdiv(ntiles, c.tiles_per_slice);
  return c;
}

static inline Slicing choose_slices(int64_t Q, int64_t T, int qpl, int tile) {
  return slice_targets(Q, T, qpl, tile, want_slices(cdiv(Q, (int64_t)kWalkThreads * qpl)));
}

}  // namespace geobi
