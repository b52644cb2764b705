"""Cost of mesh refinement (csrc/subdiv.hip, geobi_gnn_amd/meshsubdiv.py) on the MI355X, the record behind DESIGN.md 4n.

  python tools/bench_subdiv.py [--out profiles/meshsubdiv.txt]

Input: the icospheres of 20 480 faces (n = 32) and 151 380 faces (n = 87, the scan-sized mesh of BASELINE.json
configs[3]).  In ONE process, after a warm-up of every shape, median of --rounds (20) measurements of

  one uniform pass         midpoint and Loop: geobi_subdiv_plan with its stage_ms argument (device events at the stage
                           borders inside the call: the slots, the 48-bit sort, the rest of the plan -- flags, scans, for
                           Loop the directed pairs and their sort), then geobi_subdiv_emit between two device events
  one max_edge run         max_edge = 0.6 of the longest edge (on these near-uniform spheres: one round that splits every edge
                           and the plan that ends the run): host clock around the whole synchronous call, and its first
                           round by stages as above

and beside each stage the bytes it must move at least (reads + writes of its arrays, the sort counted as one read and
one write of its pairs per 8-bit digit pass).
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
from geobi_gnn_amd import meshgen, meshsubdiv                  # noqa: E402


def stage_bytes(F, V, E, split, Fn, loop):
    """the least bytes per stage: slots (faces in, 3F keys and values out); sort (6 digit passes over 3F 12-byte pairs,
    read + write); rest (keys twice, flags, scans, slot ranks, child counts; Loop: 6F 8-byte pairs and 7 passes over them);
    emit (faces, ranks, keys and points in; faces, parents, points out)"""
    slots = 12 * F + 12 * 3 * F
    sort = 6 * 2 * 12 * 3 * F
    rest = 2 * 8 * 3 * F + 4 * 4 * 3 * F + 4 * 3 * F + 4 * 4 * F + (8 * 6 * F + 7 * 2 * 8 * 6 * F if loop else 0)
    Vn = V + split
    emit = 12 * F + 12 * F + 4 * F + (8 + 4 + 4) * 3 * F + 12 * V + 12 * Fn + 4 * Fn + 8 * Vn + 12 * Vn
    return slots, sort, rest, emit


def one_pass(fv, pts, loop, max_edge):
    """-> (ms of slots, sort, rest, emit; counts)"""
    stage = (ctypes.c_float * 3)()
    ws, c = meshsubdiv._plan(fv, pts, loop, max_edge, stage)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    meshsubdiv._emit(fv, pts, loop, c[4], c[5], ws)
    b.record()
    b.synchronize()
    return list(stage) + [a.elapsed_time(b)], c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--out', type=str, default='')
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_subdiv.py measures on the MI355X'
    dev = torch.device('cuda:0')
    lines = ['Mesh refinement (csrc/subdiv.hip): cost record of tools/bench_subdiv.py',
             '%s, torch %s; median of %d in one process after a warm-up; device events at the stage borders, host clock for '
             'the whole max_edge call' % (torch.cuda.get_device_name(0), torch.__version__, opt.rounds)]
    for freq in (32, 87):
        points, faces = meshgen.icosphere(freq)
        points, faces = points.astype(np.float32), faces.astype(np.int32)
        pts, fv = torch.from_numpy(points).to(dev), torch.from_numpy(faces).to(dev)
        V, F = points.shape[0], faces.shape[0]
        d = points[faces].astype(np.float64) - points[faces[:, [1, 2, 0]]].astype(np.float64)
        max_edge = float(np.float32(0.6 * np.sqrt((d * d).sum(axis=2).max())))
        modes = (('midpoint, one uniform pass', False, None), ('Loop, one uniform pass', True, None),
                 ('max_edge %.4g, first round' % max_edge, False, max_edge))
        for _ in range(3):                       # warm-up of every shape that is timed
            for _, loop, edge in modes:
                one_pass(fv, pts, loop, edge)
            whole = meshsubdiv.subdivide(pts, fv, max_edge=max_edge, device=dev)
        torch.cuda.synchronize()
        ms = {name: [] for name, _, _ in modes}
        ms['whole'] = []
        counts = {}
        for _ in range(opt.rounds):
            for name, loop, edge in modes:
                t, counts[name] = one_pass(fv, pts, loop, edge)
                ms[name].append(t)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            meshsubdiv.subdivide(pts, fv, max_edge=max_edge, device=dev)
            ms['whole'].append(1e3 * (time.perf_counter() - t0))
        lines.append('')
        lines.append('icosphere n = %d: V = %d, F = %d' % (freq, V, F))
        for name, loop, edge in modes:
            c = counts[name]
            med = [statistics.median(x[k] for x in ms[name]) for k in range(4)]
            total = sum(med)
            lines.append('  %s: E = %d, split = %d, V -> %d, F -> %d; %.4f ms, the sort %.1f %% of it'
                         % (name, c[0], c[1], c[4], c[5], total, 100.0 * med[1] / total))
            for label, t, nbytes in zip(('slots', 'sort (48 bits, 3F pairs)', 'rest of the plan', 'emit'), med,
                                        stage_bytes(F, V, c[0], c[1], c[5], loop)):
                lines.append('    %-28s %9.4f ms   %8.2f MB at least   %7.1f GB/s' % (label, t, nbytes / 1e6, nbytes / t / 1e6))
        w = ms['whole']
        lines.append('  meshsubdiv.subdivide(max_edge=%.4g), host clock, synchronous: %d passes, V -> %d, F -> %d; %.4f ms '
                     '(min %.4f, max %.4f)' % (max_edge, whole.counts['passes'], whole.points.shape[0], whole.faces.shape[0],
                                               statistics.median(w), min(w), max(w)))
        print('\n'.join(lines[-20:]), flush=True)
    text = '\n'.join(lines) + '\n'
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, 'w') as fh:
            fh.write(text)
    else:
        print(text)


if __name__ == '__main__':
    main()
