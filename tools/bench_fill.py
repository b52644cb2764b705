"""Cost of hole filling (csrc/fill.hip, geobi_gnn_amd/meshfill.py) on the MI355X, the record behind DESIGN.md 4q.

  python tools/bench_fill.py [--out profiles/meshfill.txt]

Input: the icospheres of 20 480 faces (n = 32) and 151 380 faces (n = 87), each once without the fan of every 50th vertex
(many short loops) and once cut to the faces with z >= 0 (an open hemisphere: one long loop).  In ONE process, after a
warm-up of every shape, median of --rounds (20) measurements of

  the plan      geobi_fill_plan with its stage_ms argument (device events at the stage borders inside the call): the edge
                table (slots and the 48-bit sort of 3F pairs), the flags / counts / successors, the two pointer doublings
                over the B boundary entries, the loop tables
  the emit      geobi_fill_emit between two device events
  the whole     host clock around a synchronous meshfill.fill_holes call on device tensors

and beside each stage the bytes it must move at least (reads + writes of its arrays, the sort counted as one read and one
write of its pairs per 8-bit digit pass, a doubling round as one read, one gather and one write of 8 bytes per entry).
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
from geobi_gnn_amd import meshfill, meshgen                    # noqa: E402

LABELS = ('edge table (slots + sort)', 'flags, counts, successors', 'two doublings', 'loop tables', 'emit')


def doubling_rounds(F):
    r = 1
    while (1 << r) < 3 * F:
        r += 1
    return r


def stage_bytes(F, V, c):
    """the least bytes per stage.  table: faces in, 3F 12-byte pairs out, 6 digit passes over them (read + write).  flags:
    the sorted pairs in, the slot flags out, their scan, flags and positions in again, two memsets and one read of the two
    vertex counts, ~ 48 bytes per boundary entry (corners, entry slot, counts, successor, state).  doublings: 24 bytes per
    entry and round, 2 x rounds rounds.  tables: leader flags and their scan over 3F, flags / positions in and loop / rank
    out and copied per slot, ~ 64 bytes per row of the F-row loop tables.  emit: the old rows in and out, the slot loops in,
    16 bytes per new face, 16 per rim vertex read and 16 per new vertex"""
    B, filled, new_faces = c[0], c[5], c[7]
    table = 12 * F + 12 * 3 * F + 6 * 2 * 12 * 3 * F
    flags = 12 * 3 * F + 4 * 3 * F + 8 * 3 * F + 8 * 3 * F + 16 * V + 48 * B
    doublings = 2 * doubling_rounds(F) * 24 * B + 32 * B
    tables = 12 * 3 * F + 8 * 3 * F + 8 * 3 * F + 16 * 3 * F + 64 * F + 16 * B
    emit = 24 * F + 24 * V + 4 * 3 * F + 16 * new_faces + 16 * new_faces + 16 * filled
    return table, flags, doublings, tables, emit


def one_fill(fv, pts):
    """-> (ms of the four plan stages and the emit; counts)"""
    stage = (ctypes.c_float * 4)()
    ws, _, c = meshfill._plan(fv, pts.shape[0], 0, stage)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    meshfill._emit(fv, pts, c[8], c[9], ws)
    b.record()
    b.synchronize()
    return list(stage) + [a.elapsed_time(b)], c


def inputs(freq):
    points, faces = meshgen.icosphere(freq)
    points, faces = points.astype(np.float32), faces.astype(np.int32)
    gone = np.isin(faces, np.arange(0, points.shape[0], 50)).any(axis=1)
    yield 'without the fan of every 50th vertex', points, np.ascontiguousarray(faces[~gone])
    yield 'open hemisphere (z >= 0)', points, np.ascontiguousarray(faces[(points[faces][:, :, 2] >= 0).all(axis=1)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--out', type=str, default='')
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_fill.py measures on the MI355X'
    dev = torch.device('cuda:0')
    lines = ['Hole filling (csrc/fill.hip): cost record of tools/bench_fill.py',
             '%s, torch %s; median of %d in one process after a warm-up; device events at the stage borders, host clock for '
             'the whole fill_holes call' % (torch.cuda.get_device_name(0), torch.__version__, opt.rounds)]
    for freq in (32, 87):
        for name, points, faces in inputs(freq):
            pts, fv = torch.from_numpy(points).to(dev), torch.from_numpy(faces).to(dev)
            V, F = points.shape[0], faces.shape[0]
            for _ in range(3):
                one_fill(fv, pts)
                whole = meshfill.fill_holes(pts, fv, device=dev)
            torch.cuda.synchronize()
            ms, host = [], []
            for _ in range(opt.rounds):
                t, c = one_fill(fv, pts)
                ms.append(t)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                meshfill.fill_holes(pts, fv, device=dev)
                torch.cuda.synchronize()
                host.append(1e3 * (time.perf_counter() - t0))
            med = [statistics.median(x[k] for x in ms) for k in range(5)]
            total = sum(med)
            lines.append('')
            lines.append('icosphere n = %d %s: V = %d, F = %d' % (freq, name, V, F))
            lines.append('  B = %d, blocked = %d, chain = %d, loops = %d, longest = %d, filled = %d, new faces = %d, %d rounds per '
                         'doubling; V -> %d, F -> %d' % (c[0], c[1], c[2], c[3], c[4], c[5], c[7], doubling_rounds(F), c[8], c[9]))
            lines.append('  plan + emit %.4f ms: the sort stage %.1f %%, the doublings %.1f %% of it'
                         % (total, 100.0 * med[0] / total, 100.0 * med[2] / total))
            for label, t, nbytes in zip(LABELS, med, stage_bytes(F, V, c)):
                lines.append('    %-28s %9.4f ms   %8.2f MB at least   %7.1f GB/s' % (label, t, nbytes / 1e6, nbytes / t / 1e6))
            lines.append('  meshfill.fill_holes, host clock, synchronous: V -> %d, F -> %d; %.4f ms (min %.4f, max %.4f)'
                         % (whole.points.shape[0], whole.faces.shape[0], statistics.median(host), min(host), max(host)))
            print('\n'.join(lines[-11:]), flush=True)
    text = '\n'.join(lines) + '\n'
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, 'w') as fh:
            fh.write(text)
    else:
        print(text)


if __name__ == '__main__':
    main()
