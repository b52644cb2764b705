"""Cost of mesh simplification (csrc/decim.hip, geobi_gnn_amd/meshdecim.py) on the MI355X, the record behind DESIGN.md 4o.

  python tools/bench_decim.py [--out profiles/meshdecim.txt]

Input: the two sizes of tools/bench_subdiv.py, the icospheres of 20 480 faces (n = 32) and 151 380 faces (n = 87), to
ratio 0.5.  In ONE process, after a warm-up of every shape, median of --rounds (20) measurements of

  the first round          geobi_decim_plan with its stage_ms argument (device events at the stage borders inside the call:
                           the tables -- slots, corner keys, directed pairs and their three 48-bit sorts; the values --
                           quadrics, candidates with their tests, the hash sort and the cost sort; the selection -- the
                           sweeps, the budget, the roles and the scans), then geobi_decim_emit between two device events
  the whole call           host clock around the synchronous meshdecim.decimate(ratio=0.5), and its number of rounds

and beside each stage the bytes it must move at least: every array it reads or writes counted once per kernel that
touches it, a sort as one read and one write of its keys (and values) per 8-bit digit pass, the neighbour and corner lists
of a vertex once per vertex (the walks of the candidate tests re-read them from cache).
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geobi_gnn_amd import meshdecim, meshgen                   # noqa: E402

SWEEPS = 3                                                     # GEOBI_DECIM_SWEEPS


def stage_bytes(F, V, Vn, Fn):
    n = 3 * F
    tables = ((12 * F + 12 * n) + (12 * F + 8 * n + 4 * F) + 6 * 2 * 12 * n + 6 * 2 * 8 * n + (8 * n + 8 * 2 * n)
              + 6 * 2 * 8 * 2 * n)
    quadrics = 8 * n + 12 * F + 12 * V + 80 * V
    candidates = 8 * n + 80 * V + 12 * V + 12 * F + 8 * n + 8 * 2 * n + (8 + 4 + 4 + 4) * n
    rank = 4 * 2 * 8 * n + (4 + 8 + 8) * n + 8 * 2 * 12 * n + (8 + 4 + 4 + 4) * n
    sweep = 4 * V + (4 + 4 + 8) * n + (8 * V + 8 * 2 * n) + (4 + 4 + 8) * n + 4 * V + (4 + 8) * n
    budget = (4 + 4 + 4) * n + 2 * 4 * n + (4 + 4 + 4 + 8) * n + 8 * V + 8 * V + 8 * F
    emit = 12 * V + 4 * V + 9 * Vn + 12 * F + 8 * F + 16 * Fn + 12 * V + 12 * Vn
    return tables, quadrics + candidates + rank, SWEEPS * sweep + budget, emit


def one_round(fv, pts, target):
    """-> (ms of tables, values, selection, emit; counts)"""
    stage = (ctypes.c_float * 3)()
    ws, c = meshdecim._plan(fv, pts, None, target, stage)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    meshdecim._emit(fv, pts, c['V'], c['F'], ws)
    b.record()
    b.synchronize()
    return list(stage) + [a.elapsed_time(b)], c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--out', type=str, default='')
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_decim.py measures on the MI355X'
    dev = torch.device('cuda:0')
    lines = ['Mesh simplification (csrc/decim.hip): cost record of tools/bench_decim.py',
             '%s, torch %s; median of %d in one process after a warm-up; device events at the stage borders, host clock for '
             'the whole call; GEOBI_DECIM_SWEEPS = %d' % (torch.cuda.get_device_name(0), torch.__version__, opt.rounds, SWEEPS)]
    for freq in (32, 87):
        points, faces = meshgen.icosphere(freq)
        points, faces = points.astype(np.float32), faces.astype(np.int32)
        pts, fv = torch.from_numpy(points).to(dev), torch.from_numpy(faces).to(dev)
        V, F = points.shape[0], faces.shape[0]
        target = F // 2
        for _ in range(3):                       # warm-up of every shape that is timed
            one_round(fv, pts, target)
            whole = meshdecim.decimate(pts, fv, ratio=0.5, device=dev)
        torch.cuda.synchronize()
        ms, wall = [], []
        for _ in range(opt.rounds):
            t, c = one_round(fv, pts, target)
            ms.append(t)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            meshdecim.decimate(pts, fv, ratio=0.5, device=dev)
            wall.append(1e3 * (time.perf_counter() - t0))
        med = [statistics.median(x[k] for x in ms) for k in range(4)]
        total = sum(med)
        lines.append('')
        lines.append('icosphere n = %d: V = %d, F = %d, to ratio 0.5' % (freq, V, F))
        lines.append('  the first round: E = %d, valid candidates = %d, collapses = %d in %d sweeps, V -> %d, F -> %d; %.4f ms'
                     % (c['edges'], c['valid'], c['collapses'], c['sweeps_selected'], c['V'], c['F'], total))
        labels = ('tables (slots, corners, pairs, 3 sorts)', 'values (quadrics, tests, 2 sorts)',
                  'selection (%d sweeps, budget, scans)' % SWEEPS, 'emit')
        for label, t, nbytes in zip(labels, med, stage_bytes(F, V, c['V'], c['F'])):
            lines.append('    %-40s %9.4f ms  %5.1f %%   %8.2f MB at least   %7.1f GB/s'
                         % (label, t, 100.0 * t / total, nbytes / 1e6, nbytes / t / 1e6))
        per_round = [p.counts['collapses'] for p in whole.passes]
        lines.append('  meshdecim.decimate(ratio=0.5), host clock, synchronous: %d rounds (collapses %s), V -> %d, F -> %d, '
                     'reached %s; %.4f ms (min %.4f, max %.4f)'
                     % (whole.counts['rounds'], ' '.join(str(x) for x in per_round), whole.points.shape[0],
                        whole.faces.shape[0], whole.counts['reached'], statistics.median(wall), min(wall), max(wall)))
        print('\n'.join(lines[-8:]), flush=True)
    text = '\n'.join(lines) + '\n'
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, 'w') as fh:
            fh.write(text)
    else:
        print(text)


if __name__ == '__main__':
    main()
