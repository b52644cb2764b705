"""Cost of the projection onto the input surface (csrc/project.hip, geobi_move_to of csrc/remesh.hip,
geobi_gnn_amd/meshproject.py, meshremesh.remesh(project=True)) on the MI355X, the record behind DESIGN.md 4r.

  python tools/bench_project.py [--out profiles/meshproject.txt] [--parent_lib PATH]

Input: the two icospheres of tools/bench_remesh.py, 20 480 faces (n = 32) and 151 380 faces (n = 87), with the target edge
L at 1.5 times the mean edge.  The queries of the timed steps are the relaxed vertices of the first iteration of the call
itself (tools/bench_remesh.py: phases, then one relaxation), the surface is the input.  In ONE process, after a warm-up of
every shape, median of --rounds (20) measurements of

  closest alone    the all-pairs search (geobi_nearest_triangle: V' x F_in pair tests) and geobi_closest_on_faces behind it,
                   each between two device events
  move_to          geobi_move_to with its stage_ms argument (tables, the four launches)
  the whole call   host clock around the synchronous meshremesh.remesh(target_edge=L, iterations=5, max_rounds=256) without
                   and with project=True, alternating inside every round

--parent_lib: the library of the parent commit (the same C ABI without the new entry points).  One child process then
measures the default call alone through that library (GEOBI_LIB) before this process measures its own, and one after: the
default path makes the same launches in both libraries, so the medians are expected equal within the spread of the run.
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from geobi_gnn_amd import _lib as L                                       # noqa: E402
from geobi_gnn_amd import meshgen, mesheval, meshremesh                   # noqa: E402

SIZES = (32, 87)


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def inputs(freq, dev):
    points, faces = meshgen.icosphere(freq)
    pts = torch.from_numpy(points.astype(np.float32)).to(dev)
    fv = torch.from_numpy(faces.astype(np.int32)).to(dev)
    return pts, fv, 1.5 * meshremesh.mesh_stats(pts, fv, 0.0, 0.0, dev)['edge_mean']


def whole(pts, fv, L_edge, dev, project=None):
    """-> (milliseconds on the host clock, the result); project=None: the keyword is not passed (an older Python layer)"""
    kw = {} if project is None else {'project': project}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = meshremesh.remesh(pts, fv, target_edge=L_edge, iterations=5, max_rounds=256, device=dev, **kw)
    return 1e3 * (time.perf_counter() - t0), r


def spread(x):
    return '%.4f ms (min %.4f, max %.4f)' % (statistics.median(x), min(x), max(x))


def default_only(rounds):
    """the child of --parent_lib: the default call alone, one line per size"""
    dev = torch.device('cuda:0')
    for freq in SIZES:
        pts, fv, L_edge = inputs(freq, dev)
        with torch.cuda.device(dev):
            for _ in range(3):
                whole(pts, fv, L_edge, dev)
            wall = [whole(pts, fv, L_edge, dev)[0] for _ in range(rounds)]
        print('PARENT %d %s' % (freq, spread(wall)), flush=True)


def parent_run(parent_lib, rounds):
    """{frequency: 'median (min, max)'} of the default call through the parent's library, in a child process of its own"""
    env = dict(os.environ, GEOBI_LIB=os.path.abspath(parent_lib), GEOBI_LIB_OLDER='1')
    run = subprocess.run([sys.executable, os.path.abspath(__file__), '--default_only', '--rounds', str(rounds)], env=env,
                         capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr
    return {int(l.split()[1]): l.split(None, 2)[2] for l in run.stdout.splitlines() if l.startswith('PARENT ')}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--out', type=str, default='')
    ap.add_argument('--parent_lib', type=str, default='', help="the parent commit's libgeobi_hip.so: its default remesh is timed too")
    ap.add_argument('--default_only', action='store_true', help=argparse.SUPPRESS)
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_project.py measures on the MI355X'
    if opt.default_only:
        return default_only(opt.rounds)
    parent = [parent_run(opt.parent_lib, opt.rounds)] if opt.parent_lib else []
    import bench_remesh
    from geobi_gnn_amd import meshproject
    dev = torch.device('cuda:0')
    lines = ['Projection onto the input surface (csrc/project.hip, geobi_move_to): cost record of tools/bench_project.py',
             '%s, torch %s; median of %d in one process after a warm-up; device events around the two steps of closest, '
             'stage_ms for move_to, host clock for the whole calls; feature_angle 40, relax_lambda 0.5'
             % (torch.cuda.get_device_name(0), torch.__version__, opt.rounds)]
    for freq in SIZES:
        pts, fv, L_edge = inputs(freq, dev)
        V, F = pts.shape[0], fv.shape[0]
        low, high = meshremesh.band(L_edge)
        with torch.cuda.device(dev):
            fr, pr, lock = bench_remesh.phases(pts, fv, low, high)[2]
            relaxed = meshremesh._relax(fr, pr, lock, 0.5)[0]
            Q = relaxed.shape[0]

            def closest():
                t_search, (_, face) = events(lambda: mesheval.point_to_mesh(relaxed, pts, fv))
                t_on, out = events(lambda: meshproject.closest_on_faces(relaxed, pts, fv, face))
                return [t_search, t_on], out[1]

            def move_timed(target):
                stage = (ctypes.c_float * 2)()
                c = meshremesh._move_to(fr, relaxed, target, lock, stage)[1]
                return list(stage), c
            for _ in range(3):                   # warm-up of every shape that is timed
                target = closest()[1]
                move_timed(target)
                whole(pts, fv, L_edge, dev, False)
                projected = whole(pts, fv, L_edge, dev, True)[1]
            ms_closest, ms_move, wall, wall_p = [], [], [], []
            for _ in range(opt.rounds):
                t, target = closest()
                ms_closest.append(t)
                t, mc = move_timed(target)
                ms_move.append(t)
                wall.append(whole(pts, fv, L_edge, dev, False)[0])
                wall_p.append(whole(pts, fv, L_edge, dev, True)[0])
        med_c = [statistics.median(x[k] for x in ms_closest) for k in range(2)]
        med_m = [statistics.median(x[k] for x in ms_move) for k in range(2)]
        slices = L.lib().geobi_nearest_slices(Q, F, 1)
        lines.append('')
        lines.append('icosphere n = %d: V = %d, F = %d, L = 1.5 mean edges = %.6f; the relaxed mesh of iteration 1: V\' = %d, F\' = %d'
                     % (freq, V, F, L_edge, Q, fr.shape[0]))
        lines.append('  closest (V\' queries on the input); %.4f ms' % sum(med_c))
        lines.append('    %-44s %9.4f ms   %.3e pair tests, %d slices, %.1f G pairs/s'
                     % ('search (point_to_mesh: range check, all pairs)', med_c[0], float(Q) * F, slices, Q * F / med_c[0] / 1e6))
        lines.append('    %-44s %9.4f ms   %8.2f MB at least   %7.1f GB/s'
                     % ('geobi_closest_on_faces', med_c[1], 92 * Q / 1e6, 92 * Q / med_c[1] / 1e6))
        lines.append('  move_to: moved = %d, refused = %d, reverted = %d, turned = %d; %.4f ms'
                     % (mc['moved'], mc['refused'], mc['reverted'], mc['turned'], sum(med_m)))
        for label, t, b in zip(('tables (slots, corners, pairs, 3 sorts)', 'move, turned, revert, turned'), med_m,
                               bench_remesh.relax_bytes(fr.shape[0], Q)):
            lines.append('    %-44s %9.4f ms   %8.2f MB at least   %7.1f GB/s' % (label, t, b / 1e6, b / t / 1e6))
        lines.append('  meshremesh.remesh(target_edge=L, iterations=5, max_rounds=256), host clock, synchronous, alternating:')
        lines.append('    %-44s %s' % ('without project', spread(wall)))
        lines.append('    %-44s %s   V -> %d, F -> %d' % ('project=True', spread(wall_p), projected.points.shape[0],
                                                          projected.faces.shape[0]))
        for k, it in enumerate(projected.per_iteration):
            lines.append('      iteration %d: %d moved, %d refused, %d reverted; projected %d, refused %d, reverted %d, turned %d'
                         % (k + 1, it['moved'], it['refused'], it['reverted'], it['projected'], it['project_refused'],
                            it['project_reverted'], it['project_turned']))
        print('\n'.join(lines[-16:]), flush=True)
    if opt.parent_lib:
        parent.append(parent_run(opt.parent_lib, opt.rounds))
        lines.append('')
        lines.append("meshremesh.remesh without project through the parent commit's library, one child process before and one "
                     'after the measurements above:')
        for freq in SIZES:
            lines.append('  n = %-3d before %s   after %s' % (freq, parent[0][freq], parent[1][freq]))
        print('\n'.join(lines[-3:]), flush=True)
    text = '\n'.join(lines) + '\n'
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, 'w') as fh:
            fh.write(text)
    else:
        print(text)


if __name__ == '__main__':
    main()
