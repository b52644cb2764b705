"""Cost of the surface sampler on the MI355X: the record behind the numbers of DESIGN.md 4l.

  python tools/bench_sample.py                   # device events, alternating cases

In ONE process, after a warm-up of every shape, per mesh (default: icospheres of frequency 8 and 87, F = 1 280 -- all of
cum in the LDS table -- and F = 151 380) and per sample count the script alternates

  weights      geobi_sample_weights: three kernels and the 64-bit scan
  draw         geobi_sample_surface alone, through the C ABI (no host read)
  python       meshsample.sample_surface with weights handed in: the draw plus its one host read of cum[-1]

timed with device events around `--inner` calls, and prints medians, minima and maxima in microseconds per call.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geobi_gnn_amd import _lib as L, meshgen, meshsample      # noqa: E402


def events_us(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return 1000.0 * a.elapsed_time(b) / inner


def cases(dev, freq, n):
    points, faces = meshgen.icosphere(freq)
    p = torch.as_tensor(points).to(device=dev, dtype=torch.float32).contiguous()
    fv = torch.as_tensor(faces).to(device=dev, dtype=torch.int32).contiguous()
    weights = meshsample.surface_weights(p, fv)
    out = meshsample.sample_surface(p, fv, n, seed=1, weights=weights)
    cum, F, V = weights[1], fv.shape[0], p.shape[0]

    def draw():
        L.call('geobi_sample_surface', L.ptr(p), L.ptr(fv), L.ptr(cum), F, V, n, 0, 1, 0, 0, L.ptr(out.points),
               L.ptr(out.face), L.ptr(out.bary), L.stream())
    return F, [('weights', lambda: meshsample._weights(p, fv)), ('draw', draw),
               ('python', lambda: meshsample.sample_surface(p, fv, n, seed=1, weights=weights, check=False))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[8, 87], help='icosphere frequencies')
    ap.add_argument('--samples', type=int, nargs='+', default=[2000, 1000000])
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--inner', type=int, default=20, help='calls between two device events')
    opt = ap.parse_args()
    dev = torch.device('cuda:0')
    for freq in opt.sizes:
        for n in opt.samples:
            F, cs = cases(dev, freq, n)
            for _, fn in cs:                         # warm-up of every shape that is timed
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            us = [[] for _ in cs]
            for _ in range(opt.rounds):              # alternating: every case sees the same neighbours on the box
                for k, (_, fn) in enumerate(cs):
                    us[k].append(events_us(fn, opt.inner))
            for (name, _), m in zip(cs, us):
                print('F = %6d  n = %7d  %-8s median %9.2f us  (min %9.2f, max %9.2f, rounds = %d)'
                      % (F, n, name, statistics.median(m), min(m), max(m), len(m)))
            sys.stdout.flush()


if __name__ == '__main__':
    main()
