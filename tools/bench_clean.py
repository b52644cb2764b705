"""Cost of mesh cleaning (csrc/clean.hip, geobi_gnn_amd/meshclean.py) on the MI355X, the record behind
profiles/meshclean.txt.

  python tools/bench_clean.py [--out profiles/meshclean.txt]

Input: the scan-sized mesh of BASELINE.json configs[3] (icosphere n = 87: F = 151 380, V = 75 692) as it is and as a
triangle soup (every face with its own three vertices: V = 454 140).  In ONE process, after a warm-up of every shape,
median of --rounds (20) measurements, the stages alternating round by round:

  weld / faces / compact   device events around one call of the stage (geobi_clean_weld / _faces / _compact); `faces`
                           waits for the device once per batch of rounds, so its figure holds that wait as idle time
  clean_mesh               host clock around the whole call, which ends in a read of the counts (two reads and the waits
                           of `faces`: the call is synchronous by construction)
  host np.unique           np.unique(points, axis=0, return_inverse=True) of the same points: the weld a user would write on
                           the host (the copies to and from the device are not in it)

and the number of Jacobi rounds the half-edge rule took.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geobi_gnn_amd import meshclean, meshgen         # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--freq', type=int, default=87)
    ap.add_argument('--out', type=str, default='')
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_clean.py measures on the MI355X'
    dev = torch.device('cuda:0')
    lines = ['Mesh cleaning (csrc/clean.hip): cost record of tools/bench_clean.py',
             '%s, torch %s; median of %d, the stages alternating in one process after a warm-up; device events per stage, '
             'host clock for the whole call and for numpy' % (torch.cuda.get_device_name(0), torch.__version__, opt.rounds)]
    noisy, _, faces = meshgen.noisy_icosphere(opt.freq, 0.2, seed=opt.freq)
    noisy, faces = np.asarray(noisy, dtype=np.float32), np.asarray(faces, dtype=np.int32)
    soup = (np.ascontiguousarray(noisy[faces.reshape(-1)]), np.arange(3 * faces.shape[0], dtype=np.int32).reshape(-1, 3))
    for name, (points, fv_host) in (('as is', (noisy, faces)), ('triangle soup', soup)):
        pts = torch.from_numpy(points).to(dev)
        fv = torch.from_numpy(fv_host).to(dev)
        V, F = pts.shape[0], fv.shape[0]

        def whole():
            return meshclean.clean_mesh(pts, fv, device=dev)

        for _ in range(3):                       # warm-up of every shape that is timed
            result = whole()
        torch.cuda.synchronize()
        ms = {k: [] for k in ('weld', 'faces', 'compact', 'clean_mesh', 'numpy')}
        for _ in range(opt.rounds):
            t, (canon, _) = event_ms(lambda: meshclean.weld(pts, 0.0))
            ms['weld'].append(t)
            t, (fc, state, rounds) = event_ms(lambda: meshclean.resolve_faces(fv, canon, V))
            ms['faces'].append(t)
            t, _ = event_ms(lambda: meshclean.compact(pts, fc, state, canon, F))
            ms['compact'].append(t)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            whole()
            ms['clean_mesh'].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            uniq, inverse = np.unique(points, axis=0, return_inverse=True)
            ms['numpy'].append(1e3 * (time.perf_counter() - t0))
        assert rounds == result.counts['rounds'] and uniq.shape[0] == V - result.counts['welded']
        lines.append('')
        lines.append('%s: V = %d -> %d, F = %d -> %d, welded %d, rounds %d'
                     % (name, V, result.points.shape[0], F, result.faces.shape[0], result.counts['welded'], rounds))
        for key, label in (('weld', 'geobi_clean_weld (keys, 3 radix passes, heads, scan)'),
                           ('faces', 'geobi_clean_faces (remap, 48-bit sort, 4 rounds, their wait)'),
                           ('compact', 'geobi_clean_compact (flags, 2 scans, gathers)'),
                           ('clean_mesh', 'meshclean.clean_mesh, host clock, synchronous'),
                           ('numpy', 'host np.unique(points, axis=0, return_inverse=True)')):
            v = ms[key]
            lines.append('  %-58s %9.4f ms (min %9.4f, max %9.4f)' % (label, statistics.median(v), min(v), max(v)))
        stages = sum(statistics.median(ms[k]) for k in ('weld', 'faces', 'compact'))
        lines.append('  stages together %.4f ms; host unique / device weld: %.0f x'
                     % (stages, statistics.median(ms['numpy']) / statistics.median(ms['weld'])))
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
