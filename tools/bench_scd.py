"""Cost of the sampled surface Chamfer loss on the MI355X, the record behind profiles/scd_loss.txt.

  python tools/bench_scd.py

In ONE process, after a warm-up of every shape, the script alternates, on the union of 4 icospheres of 20 480 faces

  weights  surface_weights_parts on the union  |  surface_weights on each of the four meshes
  draw     sample_surface_parts, N = 10 000 per mesh, weights given  |  sample_surface on each of the four (both forms
           read their totals back once per call, as the training step does)
  points   bary_points forward  |  its backward (keys, inverse lists, the list walk) under a fixed incoming gradient
  step     the 4-mesh training step of tools/bench_chamfer.py with L1 / L1, CD / sided and SCD / sided

and prints medians, minima and maxima.  The small calls are timed with device events around `--inner` calls, the steps
with events around one step.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geobi_gnn_amd import meshgen, meshsample, network, ops      # noqa: E402

from bench_chamfer import events_ms, stats                       # noqa: E402


def union(dev, parts=4, freq=32):
    """`parts` icospheres of frequency `freq` (20 480 faces at 32), each scaled on its own -> points, faces (global ids),
    fptr, and the meshes one by one"""
    import numpy as np
    pts, faces = meshgen.icosphere(freq)
    meshes = [(torch.as_tensor(pts * (1.0 + 0.1 * k), dtype=torch.float32).to(dev),
               torch.as_tensor(np.ascontiguousarray(faces), dtype=torch.int32).to(dev)) for k in range(parts)]
    V, F = pts.shape[0], faces.shape[0]
    p = torch.cat([m[0] for m in meshes]).contiguous()
    f = torch.cat([m[1] + k * V for k, m in enumerate(meshes)]).contiguous()
    return p, f, [k * F for k in range(parts + 1)], meshes


def sampler_cases(dev, n):
    p, f, fptr, meshes = union(dev)
    P = len(meshes)
    wp = meshsample.surface_weights_parts(p, f, fptr, check=False)
    w1 = [meshsample.surface_weights(a, b, check=False) for a, b in meshes]
    s = meshsample.sample_surface_parts(p, f, fptr, n, seed=1, stream_ids=list(range(P)), weights=wp, check=False)
    gx = torch.randn((P * n, 3), generator=torch.Generator().manual_seed(1)).to(dev)
    leaf = p.clone().requires_grad_()

    def backward():
        x = ops.bary_points(leaf, f, s.face, s.bary)
        leaf.grad = None
        x.backward(gx)

    def forward():                                      # (forward + backward) minus this = the backward's share
        with torch.no_grad():
            ops.bary_points(p, f, s.face, s.bary)
    return [
        ('weights  parts, P = %d x F = %d' % (P, fptr[1]), lambda: meshsample.surface_weights_parts(p, f, fptr, check=False)),
        ('weights  %d single-mesh calls' % P, lambda: [meshsample._weights(a, b) for a, b in meshes]),
        ('draw     parts, N = %d each' % n,
         lambda: meshsample.sample_surface_parts(p, f, fptr, n, seed=1, stream_ids=list(range(P)), weights=wp, check=False)),
        ('draw     %d single-mesh calls' % P,
         lambda: [meshsample.sample_surface(a, b, n, seed=1, stream_id=k, weights=w, check=False)
                  for k, ((a, b), w) in enumerate(zip(meshes, w1))]),
        ('points   bary_points forward, n = %d' % (P * n), forward),
        ('points   forward + backward (keys, lists, walk)', backward),
    ]


def make_step(dev, losses, n):
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
    sampling = dict(n=n, seed=1, draw=1, stream_ids=[0, 1, 2, 3]) if losses[0] == 'SCD' else None

    def step():
        flat.bucket.zero()
        vp, npred, _ = net((dv0.shallow_copy(), df0.shallow_copy()))
        lv, ln = batched_losses(vp, npred, dv0, df0, losses[0], losses[1], sampling=sampling)
        network.dual_loss(lv, ln).backward()
        opt.step()
    return step


def alternate(cases, rounds, inner, warm):
    for _, fn in cases:                          # warm-up of every shape that is timed
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in cases]
    for _ in range(rounds):                      # alternating: every case sees the same neighbours on the box
        for k, (_, fn) in enumerate(cases):
            ms[k].append(events_ms(fn, inner))
    for (name, _), v in zip(cases, ms):
        print(stats(name, v))
    sys.stdout.flush()
    return [statistics.median(v) for v in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--inner', type=int, default=20, help='sampler calls between two device events')
    ap.add_argument('--samples', type=int, default=10000, help='N per mesh')
    opt = ap.parse_args()
    dev = torch.device('cuda:0')
    wp, w4, dp, d4, fwd, both = alternate(sampler_cases(dev, opt.samples), opt.rounds, opt.inner, 3)
    print('   weights: parts over 4 calls %.3f; draw: parts over 4 calls %.3f; backward alone (difference) %.4f ms'
          % (wp / w4, dp / d4, both - fwd))
    steps = [('step L1 / L1', make_step(dev, ('L1', 'L1'), opt.samples)),
             ('step CD / sided', make_step(dev, ('CD', 'sided'), opt.samples)),
             ('step SCD / sided, N = %d' % opt.samples, make_step(dev, ('SCD', 'sided'), opt.samples))]
    l1, cd, scd = alternate(steps, opt.rounds, 1, 5)
    print('   CD / sided minus L1 / L1: %+.4f ms; SCD / sided minus CD / sided: %+.4f ms per 4-mesh step' % (cd - l1, scd - cd))


if __name__ == '__main__':
    main()
