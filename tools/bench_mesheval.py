"""Times of the nearest-distance kernels (csrc/dist.hip) on the MI355X, the record behind profiles/mesheval_kernels.txt.

  python tools/bench_mesheval.py                 # kernel call times + nearest_point against torch.cdist(...).min(1), alternating
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_mesheval.py --mode trace      # a run of its own

Sizes: a 20 k-face mesh (icosphere n = 32: V = 10 242, F = 20 480) and a 150 k-face scan (n = 87: V = 75 692,
F = 151 380); queries = the noisy vertices, targets = the clean vertices / the clean surface.
Pair tests per second = Q x T / time.  Arithmetic per pair (counted from the source, selects and compares not counted):
point 8 flop (3 sub, 1 mul, 2 fma), triangle 67 flop; the share of peak is that rate over the 157.3 TFLOP/s fp32 vector peak.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geobi_gnn_amd import mesheval, meshgen      # noqa: E402

PEAK_FP32 = 157.3e12
FLOP_POINT, FLOP_TRI = 8, 67


def cdist_min(q, t, rows=2048):
    """The plumbing form: all distances of a query chunk stored, then read back for the minimum."""
    d = torch.empty(q.shape[0], dtype=torch.float32, device=q.device)
    i = torch.empty(q.shape[0], dtype=torch.int64, device=q.device)
    for a in range(0, q.shape[0], rows):
        m = torch.cdist(q[a:a + rows], t).min(1)
        d[a:a + rows], i[a:a + rows] = m.values, m.indices
    return d, i


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def line(name, ms, pairs, flop):
    med = statistics.median(ms)
    rate = pairs / (med * 1e-3)
    return '%-44s median %9.3f ms  (min %9.3f, max %9.3f, n = %d)  %8.3f G pairs/s  %5.1f %% of fp32 vector peak' % (
        name, med, min(ms), max(ms), len(ms), rate / 1e9, 100.0 * rate * flop / PEAK_FP32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=['time', 'trace'], default='time')
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--freqs', type=int, nargs='+', default=[32, 87])
    opt = ap.parse_args()
    dev = torch.device('cuda:0')
    for n in opt.freqs:
        noisy, clean, faces = meshgen.noisy_icosphere(n, 0.2, seed=1)
        q = torch.as_tensor(noisy, device=dev)
        t = torch.as_tensor(clean, device=dev)
        fv = torch.as_tensor(faces, dtype=torch.int32, device=dev)
        V, F = t.shape[0], fv.shape[0]
        if opt.mode == 'trace':
            t2 = torch.cat([t, t])[:F].contiguous()          # F target points: the same pair count for both kernels
            for _ in range(5):
                mesheval.nearest_point(q, t2)
                mesheval.point_to_mesh(q, t, fv)
            torch.cuda.synchronize()
            continue
        # the kernel's answer is the plumbing form's (up to cdist's own rounding: it expands |q|^2 + |t|^2 - 2 q.t)
        d, _ = mesheval.nearest_point(q, t)
        dc, _ = cdist_min(q, t)
        print('n = %d: V = %d, F = %d; max |nearest_point - cdist.min| = %.3e' % (n, V, F, float((d - dc).abs().max())))
        for _ in range(3):                       # warm-up of every shape that is timed
            mesheval.nearest_point(q, t)
            mesheval.point_to_mesh(q, t, fv)
            cdist_min(q, t)
        a, b = [], []
        for _ in range(opt.reps):                # alternating, so that both see the same neighbours on the box
            a += timed(lambda: mesheval.nearest_point(q, t), 1)
            b += timed(lambda: cdist_min(q, t), 1)
        print(line('nearest_point  %d x %d' % (V, V), a, V * V, FLOP_POINT))
        print(line('cdist.min(1)   %d x %d (chunks of 2048)' % (V, V), b, V * V, FLOP_POINT))
        print('   ratio cdist / kernel (medians): %.2f' % (statistics.median(b) / statistics.median(a)))
        # the sizes of the kernel record: queries x a target set of F points / F triangles
        t2 = torch.cat([t, t])[:F].contiguous()
        mesheval.nearest_point(q, t2)
        print(line('nearest_point  %d x %d' % (V, F), timed(lambda: mesheval.nearest_point(q, t2), opt.reps), V * F, FLOP_POINT))
        print(line('point_to_mesh  %d x %d' % (V, F), timed(lambda: mesheval.point_to_mesh(q, t, fv), opt.reps), V * F, FLOP_TRI))
        sys.stdout.flush()


if __name__ == '__main__':
    main()
