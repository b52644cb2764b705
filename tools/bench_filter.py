"""Cost of the bilateral normal filter on the MI355X, the record behind profiles/filter_bnf.txt.

  python tools/bench_filter.py [--out profiles/filter_bnf.txt]

In ONE process, after a warm-up of every shape, with device events around `--inner` calls, alternating round by round:

  kernel               geobi_bnf_filter, 20 sweeps (the launch that fills the per-edge spatial factors is inside the call)
  torch device ops     the same 20 sweeps written with index_add_ over the COO (rows, columns and self loops), on the same
                       inputs and the same device

at F = 20 480 and F = 151 380 (icospheres n = 32 and n = 87, noise 0.2).  Per sweep it reports the time and the bytes the
kernel must move by its own account (every array element it touches, once):

  per face   8 B row pointers + 16 B own (c, A) + 16 B own normal + 16 B result
  per edge   4 B column + 16 B neighbour normal + 4 B spatial factor

and the kernel's result is compared with the torch result (largest component difference).
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geobi_gnn_amd import filters, meshgen, meshprep         # noqa: E402

SWEEPS = 20
SIGMA_R = 0.35


def events_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def sweep_bytes(F, E):
    return F * (8 + 16 + 16 + 16) + E * (4 + 16 + 4)


def torch_filter(rec_c, rec_n, row, col, a, b, sweeps):
    """The filter in torch device ops: COO with the self loops appended, index_add_ for the two sums."""
    cen, area = rec_c[:, :3], rec_c[:, 3]
    w_s = area[col] * torch.exp(-a * (cen[row] - cen[col]).pow(2).sum(1))
    n = rec_n[:, :3]
    for _ in range(sweeps):
        nj = n[col]
        w = w_s * torch.exp(-b * (n[row] - nj).pow(2).sum(1))
        s = torch.zeros_like(n).index_add_(0, row, w[:, None] * nj)
        W = torch.zeros_like(area).index_add_(0, row, w)
        ln = s.norm(dim=1)
        n = torch.where((ln > 1e-6 * W)[:, None], s / ln.clamp(min=1e-38)[:, None], n)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--inner', type=int, default=10, help='calls between two device events')
    ap.add_argument('--freqs', type=int, nargs='+', default=[32, 87])
    ap.add_argument('--out', type=str, default='')
    opt = ap.parse_args()
    dev = torch.device('cuda:0')
    lines = ['Bilateral normal filter (csrc/filter.hip): cost record of tools/bench_filter.py',
             '%s, torch %s; %d sweeps per call, sigma_r %.2f, sigma_s 1; device events around %d calls, %d rounds, the two '
             'cases alternating in one process after a warm-up'
             % (torch.cuda.get_device_name(0), torch.__version__, SWEEPS, SIGMA_R, opt.inner, opt.rounds)]
    for freq in opt.freqs:
        noisy, _, faces = meshgen.noisy_icosphere(freq, 0.2, seed=freq)
        pts = torch.from_numpy(noisy).to(dev)
        fv = torch.from_numpy(np.asarray(faces, dtype=np.int32)).to(dev)
        rowptr, lst = meshprep.vertex_faces(fv, pts.shape[0])
        graph = meshprep.ring_graph(1, fv, rowptr, lst, fv.shape[0])
        rec_c, rec_n = filters.face_records(pts, fv)
        inv2ss = filters.spatial_scale(pts, fv, graph, 1.0)
        F, E = fv.shape[0], graph.E
        loops = torch.arange(F, device=dev)
        row = torch.cat([graph.ensure_rows().long(), loops])
        col = torch.cat([graph.col_out.long(), loops])
        b = 0.5 / (SIGMA_R * SIGMA_R)

        cases = [('kernel (geobi_bnf_filter)', lambda: filters.filter_records(rec_c, rec_n, graph, inv2ss, SIGMA_R, SWEEPS),
                  sweep_bytes(F, E)),
                 ('torch device ops (index_add_ over the COO)', lambda: torch_filter(rec_c, rec_n, row, col, inv2ss, b, SWEEPS), None)]
        results = []
        for _, fn, _ in cases:                   # warm-up of every shape that is timed
            for _ in range(3):
                results.append(fn())
        torch.cuda.synchronize()
        want = results[-1]
        diff = float((results[0][:, :3] - want).abs().max())
        ms = [[] for _ in cases]
        for _ in range(opt.rounds):              # alternating: every case sees the same neighbours on the box
            for k, (_, fn, _) in enumerate(cases):
                ms[k].append(events_ms(fn, opt.inner))
        lines.append('')
        lines.append('F = %d faces, E = %d facet-graph edges (mean degree %.2f)' % (F, E, E / F))
        for (name, _, nbytes), v in zip(cases, ms):
            med = statistics.median(v)
            text = '  %-46s %8.4f ms per call (min %8.4f, max %8.4f), %7.2f us per sweep' % (name, med, min(v), max(v), 1e3 * med / SWEEPS)
            if nbytes is not None:
                text += ', %6.2f MB per sweep = %6.1f GB/s' % (nbytes / 1e6, nbytes / (med / SWEEPS * 1e-3) / 1e9)
            lines.append(text)
        med = [statistics.median(v) for v in ms]
        lines.append('  torch / kernel: %.1f x;  largest |kernel - torch| component: %.2e' % (med[1] / med[0], diff))
        print('\n'.join(lines[-5:]), flush=True)
    text = '\n'.join(lines) + '\n'
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, 'w') as fh:
            fh.write(text)
    else:
        print(text)


if __name__ == '__main__':
    main()
