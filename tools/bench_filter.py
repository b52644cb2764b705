"""Cost of the bilateral and the guided normal filter on the MI355X, the records behind profiles/filter_bnf.txt and
profiles/filter_gnf.txt.

  python tools/bench_filter.py [--out profiles/filter_bnf.txt]
  python tools/bench_filter.py --case gnf [--out profiles/filter_gnf.txt]

In ONE process, after a warm-up of every shape, with device events around `--inner` calls, alternating round by round:

  kernel               geobi_bnf_filter, 20 sweeps (the launch that fills the per-edge spatial factors is inside the call)
  torch device ops     the same 20 sweeps written with index_add_ over the COO (rows, columns and self loops), on the same
                       inputs and the same device

at F = 20 480 and F = 151 380 (icospheres n = 32 and n = 87, noise 0.2).  Per sweep it reports the time and the bytes the
kernel must move by its own account (every array element it touches, once):

  per face   8 B row pointers + 16 B own (c, A) + 16 B own normal + 16 B result
  per edge   4 B column + 16 B neighbour normal + 4 B spatial factor

and the kernel's result is compared with the torch result (largest component difference).

--case gnf, same protocol, the cases alternating: geobi_gnf_filter (20 sweeps: patch measure, selection + guidance, guided
sweep, three launches each), the same three stages in torch device ops over patches padded to the longest row (the table of
edge pairs inside every patch is built before the clock starts), geobi_bnf_filter on the same inputs, and
geobi_gnf_patch_measure alone (x 20), which gives the share of the patch search and its rate in normal comparisons
(sum_k |P_k|^2) per second.  That rate is measured once more on the shape that is slowest per comparison, a closed fan of
valence 2048 whose every patch is the whole fan (unstaged rows, 16 lanes per row): filters.GNF_COST_BUDGET is set from it.
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


def padded_patches(graph, F, dev):
    """[F, pmax] face ids of every patch (row + the face itself), -1 padded, and the validity mask."""
    deg = (graph.rowptr_out[1:F + 1] - graph.rowptr_out[:F]).long()
    pmax = int(deg.max()) + 1
    P = torch.full((F, pmax), -1, dtype=torch.long, device=dev)
    rows = graph.ensure_rows().long()
    slot = torch.arange(graph.E, device=dev) - graph.rowptr_out[:F].long()[rows]
    P[rows, slot] = graph.col_out.long()
    P[torch.arange(F, device=dev), deg] = torch.arange(F, device=dev)
    return P, P >= 0


def torch_guided(rec_c, rec_n, row, col, a, b, sweeps, P, ok, edge):
    """The guided filter in torch device ops: padded patches, cdist for the comparisons, index_add_ for the sweep."""
    cen, area = rec_c[:, :3], rec_c[:, 3]
    w_s = area[col] * torch.exp(-a * (cen[row] - cen[col]).pow(2).sum(1))
    Ps = P.clamp(min=0)
    both = ok[:, :, None] & ok[:, None, :]
    n = rec_n[:, :3]
    for _ in range(sweeps):
        N = n[Ps]
        D = torch.cdist(N, N)
        phi = (D * both).flatten(1).amax(1)
        De = (D * edge).flatten(1)
        H = phi * De.amax(1) / (1e-9 + De.sum(1))
        sel = Ps.gather(1, torch.where(ok, H[Ps], torch.full_like(H[Ps], float('inf'))).argmin(1, keepdim=True))[:, 0]
        wa = area[Ps[sel]] * ok[sel]
        s = (wa[:, :, None] * n[Ps[sel]]).sum(1)
        ln = s.norm(dim=1)
        g = torch.where((ln > 1e-6 * wa.sum(1))[:, None], s / ln.clamp(min=1e-38)[:, None], n)
        nj = n[col]
        w = w_s * torch.exp(-b * (g[row] - g[col]).pow(2).sum(1))
        s = torch.zeros_like(n).index_add_(0, row, w[:, None] * nj)
        W = torch.zeros_like(area).index_add_(0, row, w)
        ln = s.norm(dim=1)
        n = torch.where((ln > 1e-6 * W)[:, None], s / ln.clamp(min=1e-38)[:, None], n)
    return n


def edge_table(P, ok, graph, flags, F):
    """[F, pmax, pmax] bool: entries (s, t) of a patch that are an edge pair, each unordered pair once."""
    rows = graph.ensure_rows().long()
    on = flags.bool()
    keys = torch.sort(rows[on] * F + graph.col_out.long()[on]).values
    Ps = P.clamp(min=0)
    q = Ps[:, :, None] * F + Ps[:, None, :]
    at = torch.searchsorted(keys, q.flatten()).clamp(max=max(keys.numel() - 1, 0)).view_as(q)
    hit = (keys[at] == q) if keys.numel() else torch.zeros_like(q, dtype=torch.bool)
    return hit & ok[:, :, None] & ok[:, None, :] & (Ps[:, :, None] < Ps[:, None, :])


def fan_mesh(valence):
    k = np.arange(valence)
    ang = 2 * np.pi * k / valence
    rng = np.random.default_rng(valence)
    rim = np.stack([np.cos(ang), np.sin(ang), 0.2 * rng.uniform(-1, 1, valence)], 1)
    pts = np.concatenate([[[0.0, 0.0, 0.5]], rim], 0).astype(np.float32)
    return pts, np.stack([np.zeros(valence, dtype=np.int64), 1 + k, 1 + (k + 1) % valence], 1).astype(np.int32)


def main_gnf(opt, dev):
    lines = ['Guided normal filter (csrc/guided.hip): cost record of tools/bench_filter.py --case gnf',
             '%s, torch %s; %d sweeps per call, sigma_r %.2f, sigma_s 1; device events around %d calls, %d rounds, the '
             'cases alternating in one process after a warm-up'
             % (torch.cuda.get_device_name(0), torch.__version__, SWEEPS, SIGMA_R, opt.inner, opt.rounds)]
    b = 0.5 / (SIGMA_R * SIGMA_R)
    for freq in opt.freqs:
        noisy, _, faces = meshgen.noisy_icosphere(freq, 0.2, seed=freq)
        pts = torch.from_numpy(noisy).to(dev)
        fv = torch.from_numpy(np.asarray(faces, dtype=np.int32)).to(dev)
        rowptr, lst = meshprep.vertex_faces(fv, pts.shape[0])
        graph = meshprep.ring_graph(1, fv, rowptr, lst, fv.shape[0])
        rec_c, rec_n = filters.face_records(pts, fv)
        inv2ss = filters.spatial_scale(pts, fv, graph, 1.0)
        flags = filters.edge_flags(fv, graph)
        F, E = fv.shape[0], graph.E
        cost = filters.patch_cost(graph, F)
        loops = torch.arange(F, device=dev)
        row = torch.cat([graph.ensure_rows().long(), loops])
        col = torch.cat([graph.col_out.long(), loops])
        P, ok = padded_patches(graph, F, dev)
        edge = edge_table(P, ok, graph, flags, F)

        def measure_only():
            for _ in range(SWEEPS):
                H = filters.patch_measure(rec_c, rec_n, graph, flags)
            return H

        cases = [('kernel (geobi_gnf_filter)', lambda: filters.guided_records(rec_c, rec_n, fv, graph, inv2ss, SIGMA_R, SWEEPS)),
                 ('torch device ops (cdist over padded patches)',
                  lambda: torch_guided(rec_c, rec_n, row, col, inv2ss, b, SWEEPS, P, ok, edge)),
                 ('kernel (geobi_bnf_filter)', lambda: filters.filter_records(rec_c, rec_n, graph, inv2ss, SIGMA_R, SWEEPS)),
                 ('geobi_gnf_patch_measure alone x %d' % SWEEPS, measure_only)]
        results = []
        for _, fn in cases:
            for _ in range(3):
                results.append(fn())
        torch.cuda.synchronize()
        diff = float((results[2][:, :3] - results[5]).abs().max())
        rounds = [opt.rounds, max(2, opt.rounds // 5), opt.rounds, opt.rounds]      # the torch form is slow: fewer rounds
        ms = [[] for _ in cases]
        for r in range(opt.rounds):
            for k, (_, fn) in enumerate(cases):
                if r < rounds[k]:
                    ms[k].append(events_ms(fn, opt.inner if k != 1 else 1))
        lines.append('')
        lines.append('F = %d faces, E = %d facet-graph edges (mean degree %.2f), sum |P_k|^2 = %d comparisons per sweep'
                     % (F, E, E / F, cost))
        med = [statistics.median(v) for v in ms]
        for (name, _), v, m in zip(cases, ms, med):
            lines.append('  %-46s %8.4f ms per call (min %8.4f, max %8.4f), %7.2f us per sweep' % (name, m, min(v), max(v), 1e3 * m / SWEEPS))
        lines.append('  torch / kernel: %.1f x;  guided / bilateral kernel: %.1f x;  patch measure: %.0f %% of the guided call, '
                     '%.3g comparisons per second;  largest |kernel - torch| component: %.2e'
                     % (med[1] / med[0], med[0] / med[2], 100 * med[3] / med[0], cost * SWEEPS / (med[3] * 1e-3), diff))
        print('\n'.join(lines[-6:]), flush=True)
        del edge, P, ok
    # the shape that is slowest per comparison: one hub, every patch the whole fan
    pts, fv = (torch.from_numpy(x).to(dev) for x in fan_mesh(opt.fan))
    rowptr, lst = meshprep.vertex_faces(fv, pts.shape[0])
    graph = meshprep.ring_graph(1, fv, rowptr, lst, fv.shape[0])
    rec_c, rec_n = filters.face_records(pts, fv)
    flags = filters.edge_flags(fv, graph)
    cost = filters.patch_cost(graph, fv.shape[0])
    for _ in range(2):
        filters.patch_measure(rec_c, rec_n, graph, flags)
    torch.cuda.synchronize()
    v = [events_ms(lambda: filters.patch_measure(rec_c, rec_n, graph, flags), 2) for _ in range(5)]
    m = statistics.median(v)
    lines.append('')
    lines.append('closed fan of valence %d (every patch the whole fan, rows read through the CSR): sum |P_k|^2 = %d' % (opt.fan, cost))
    lines.append('  geobi_gnf_patch_measure %8.3f ms per launch (min %8.3f, max %8.3f): %.3g comparisons per second'
                 % (m, min(v), max(v), cost / (m * 1e-3)))
    print('\n'.join(lines[-2:]), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', type=str, default='bnf', choices=['bnf', 'gnf'])
    ap.add_argument('--fan', type=int, default=2048, help='gnf: valence of the fan the comparison rate is measured on')
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--inner', type=int, default=10, help='calls between two device events')
    ap.add_argument('--freqs', type=int, nargs='+', default=[32, 87])
    ap.add_argument('--out', type=str, default='')
    opt = ap.parse_args()
    dev = torch.device('cuda:0')
    if opt.case == 'gnf':
        return finish(main_gnf(opt, dev), opt)
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
    finish(lines, opt)


def finish(lines, opt):
    text = '\n'.join(lines) + '\n'
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, 'w') as fh:
            fh.write(text)
    else:
        print(text)


if __name__ == '__main__':
    main()
