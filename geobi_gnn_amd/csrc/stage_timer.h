// Device events at the stage borders of one call, for the measurement tools (tools/bench_topo.py, tools/bench_subdiv.py,
// tools/bench_decim.py, tools/bench_remesh.py, tools/bench_fill.py).
#pragma once
#include "common.h"

namespace geobi {

// device events at the stage borders of one call, read after a wait for the last
struct StageTimer {
  float* out;
  hipStream_t s;
  static constexpr int kMaxMarks = 5;          // four stages at the most (fill.hip)
  hipEvent_t ev[kMaxMarks] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int n = 0;
  StageTimer(float* out_ms, hipStream_t stream) : out(out_ms), s(stream) {}
  ~StageTimer() {
    for (hipEvent_t e : ev)
      if (e != nullptr) (void)hipEventDestroy(e);
  }
  int mark() {
    if (out == nullptr || n >= kMaxMarks) return 0;
    GEOBI_HIP(hipEventCreate(&ev[n]));
    GEOBI_HIP(hipEventRecord(ev[n], s));
    ++n;
    return 0;
  }
  int finish() {
    if (out == nullptr) return 0;
    GEOBI_HIP(hipEventSynchronize(ev[n - 1]));
    for (int k = 0; k + 1 < n; ++k) GEOBI_HIP(hipEventElapsedTime(out + k, ev[k], ev[k + 1]));
    return 0;
  }
};

}  // namespace geobi
