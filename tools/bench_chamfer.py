"""Cost of the correspondence-free losses on the MI355X, the record behind profiles/chamfer_loss.txt.

  python tools/bench_chamfer.py                  # searches and training steps, alternating, device events
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_chamfer.py --mode trace      # a run of its own

In ONE process, after a warm-up of every shape, the script alternates

  search   geobi_nearest_point (the kernel the segmented search was derived from) -- twice per round, so that its own
           run-to-run spread is measured by the same loop -- and geobi_nearest_parts with P = 1 and with P = 4 parts of that
           size, at 10 242 x 10 242 (the vertices of a 20 k-face mesh) and 20 480 x 20 480 (its face centroids)
  step     the training step of BASELINE.json configs[2] (4 meshes x 20 480 faces as one union graph: forward, losses,
           backward, Adam) with L1 / L1 and with CD / sided

and prints medians, minima, maxima and the differences.  Searches are timed with device events around `--inner` calls
(one call is shorter than the event resolution is good for), steps with events around one step.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geobi_gnn_amd import mesheval, meshgen, network, ops      # noqa: E402


def events_ms(fn, inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def stats(name, ms):
    return '%-46s median %8.4f ms  (min %8.4f, max %8.4f, n = %d)' % (name, statistics.median(ms), min(ms), max(ms), len(ms))


def search_cases(dev, n, parts=4):
    g = torch.Generator().manual_seed(n)
    q = torch.randn((parts * n, 3), generator=g).to(dev)
    t = (q + 0.01 * torch.randn((parts * n, 3), generator=g).to(dev)).contiguous()
    ptr = [k * n for k in range(parts + 1)]
    q1, t1 = q[:n].contiguous(), t[:n].contiguous()
    return [
        ('nearest_point  %d x %d' % (n, n), lambda: mesheval.nearest_point(q1, t1)),
        ('nearest_point  %d x %d (again)' % (n, n), lambda: mesheval.nearest_point(q1, t1)),
        ('nearest_parts  P = 1, %d x %d' % (n, n), lambda: ops.nearest_parts(q1, t1)),
        ('nearest_parts  P = %d, %d x %d each' % (parts, n, n), lambda: ops.nearest_parts(q, t, ptr, ptr)),
    ]


def make_step(dev, losses):
    from geobi_gnn_amd.data import union_batch
    from geobi_gnn_amd.parallel import FlatParameters, batched_losses
    from geobi_gnn_amd.train_util import FlatAdam
    pairs = [meshgen.synthetic_dual_data(32, (0.1, 0.2, 0.3)[i % 3], seed=200 + i) for i in range(4)]
    dv0, df0 = union_batch(pairs)
    dv0, df0 = dv0.to(dev), df0.to(dev)
    torch.manual_seed(0)
    net = network.DualGNN().to(dev)
    flat = FlatParameters(net)
    opt = FlatAdam(flat.parameters(), lr=1e-3)

    def step():
        flat.bucket.zero()
        vp, npred, _ = net((dv0.shallow_copy(), df0.shallow_copy()))
        lv, ln = batched_losses(vp, npred, dv0, df0, losses[0], losses[1])
        network.dual_loss(lv, ln).backward()
        opt.step()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=['time', 'trace'], default='time')
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--inner', type=int, default=20, help='search calls between two device events')
    ap.add_argument('--sizes', type=int, nargs='+', default=[10242, 20480])
    opt = ap.parse_args()
    dev = torch.device('cuda:0')
    steps = [('step L1 / L1', make_step(dev, ('L1', 'L1'))), ('step CD / sided', make_step(dev, ('CD', 'sided')))]
    if opt.mode == 'trace':
        for n in opt.sizes:                      # kernel times free of the host's share of a call
            for _, fn in search_cases(dev, n)[1:]:
                for _ in range(10):
                    fn()
        for _, fn in steps:
            for _ in range(8):
                fn()
        torch.cuda.synchronize()
        return
    for n in opt.sizes:
        cases = search_cases(dev, n)
        for _, fn in cases:                      # warm-up of every shape that is timed
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = [[] for _ in cases]
        for _ in range(opt.rounds):              # alternating: every case sees the same neighbours on the box
            for k, (_, fn) in enumerate(cases):
                ms[k].append(events_ms(fn, opt.inner))
        for (name, _), v in zip(cases, ms):
            print(stats(name, v))
        base, again, p1, p4 = [statistics.median(v) for v in ms]
        print('   spread of the parent kernel (|again - first| of the medians): %.4f ms; P = 1 minus parent: %+.4f ms; '
              'P = 4 over 4 x P = 1: %.3f' % (abs(again - base), p1 - 0.5 * (base + again), p4 / (4 * p1)))
        sys.stdout.flush()
    for _, fn in steps:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in steps]
    for _ in range(opt.rounds):
        for k, (_, fn) in enumerate(steps):
            ms[k].append(events_ms(fn))
    for (name, _), v in zip(steps, ms):
        print(stats(name, v))
    print('   CD / sided minus L1 / L1 (medians): %+.4f ms per 4-mesh step' % (statistics.median(ms[1]) - statistics.median(ms[0])))


if __name__ == '__main__':
    main()
