"""Cost of the mesh regularisers on the MI355X: the record behind the table of DESIGN.md 4k.

  python tools/bench_reg.py                      # device events, alternating cases

In ONE process, after a warm-up of every shape, per size (default: icospheres of frequency 32 and 87, V = 10 242 and
75 692) the script alternates forward + backward of

  torch ops    network.laplacian_loss_torch on device tensors (gathers, index_add_ = float atomics, and their autograd
               backward): what laplacian_loss was before the kernel
  lap          ops.mesh_reg with the Laplacian term alone
  lap + edge   ops.mesh_reg with both terms (the fused call a training step makes)

timed with device events around `--inner` calls, and prints medians, minima and maxima in ms per call.  The graph (CSR)
and the loop-free COO are built before the clock starts: both paths find their adjacency ready.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geobi_gnn_amd import meshgen, network, ops      # noqa: E402
from geobi_gnn_amd.graph import graph_of             # noqa: E402


def events_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def cases(dev, n):
    noisy, clean, faces = meshgen.noisy_icosphere(n, 0.3, seed=5)
    V = noisy.shape[0]
    ei = torch.from_numpy(meshgen.vertex_graph_index(faces, V)).to(dev)
    g = graph_of(ei, V)
    coo = g.coo64()                                  # loop-free, sorted: the torch path drops no loop per call
    vp = torch.from_numpy(noisy).to(dev).requires_grad_(True)
    v = torch.from_numpy(clean).to(dev)

    def run(loss):
        vp.grad = None
        loss().backward()

    both = ops.TERM_LAP | ops.TERM_EDGE
    return V, [
        ('torch ops  laplacian, fwd + bwd', lambda: run(lambda: network.laplacian_loss_torch(vp, v, coo))),
        ('mesh_reg   laplacian, fwd + bwd', lambda: run(lambda: ops.mesh_reg(vp, v, g, terms=ops.TERM_LAP)[0])),
        ('mesh_reg   laplacian + edge, fwd + bwd', lambda: run(lambda: sum(ops.mesh_reg(vp, v, g, terms=both)))),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[32, 87], help='icosphere frequencies')
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--inner', type=int, default=20, help='calls between two device events')
    opt = ap.parse_args()
    dev = torch.device('cuda:0')
    for n in opt.sizes:
        V, cs = cases(dev, n)
        for _, fn in cs:                             # warm-up of every shape that is timed
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        ms = [[] for _ in cs]
        for _ in range(opt.rounds):                  # alternating: every case sees the same neighbours on the box
            for k, (_, fn) in enumerate(cs):
                ms[k].append(events_ms(fn, opt.inner))
        for (name, _), m in zip(cs, ms):
            print('n = %3d  V = %6d  %-40s median %8.4f ms  (min %8.4f, max %8.4f, rounds = %d)'
                  % (n, V, name, statistics.median(m), min(m), max(m), len(m)))
        sys.stdout.flush()


if __name__ == '__main__':
    main()
