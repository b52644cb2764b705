"""The grid in front of the nearest searches (csrc/grid.hip, geobi_gnn_amd/meshgrid.py) against the all-pairs searches on the
same inputs on the MI355X: the record behind DESIGN.md 4u.

  python tools/bench_grid.py [--out profiles/meshgrid.txt] [--rounds 20] [--big 256]

In ONE process, after a warm-up of every shape, the median of --rounds measurements with min and max, host clock around
calls that end synchronised (a grid call waits for its read-backs, so device events alone would not see it whole):

  the two icospheres of DESIGN.md 4r (tools/bench_project.py: 20 480 and 151 380 faces; the queries are the relaxed vertices
  of the first iteration of the remeshing call, the surface is the input)
      build alone       meshgrid.TriangleGrid(points, faces) / meshgrid.PointGrid(points)
      search alone      grid.nearest(queries) against mesheval.point_to_mesh / nearest_point, alternating
      the whole call    meshremesh.remesh(target_edge=L, iterations=5, max_rounds=256, project=True) without and with
                        index='grid', alternating
  meshgen.icosphere(--big) (256: 1 310 720 faces) from the noisy vertices of the same sphere
      build, search and mesheval.point_to_mesh as above

and the share of the queries that the all-pairs search had to finish at the default max_rings.  Before anything is timed
the two answers are compared bit for bit; a difference ends the run.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from geobi_gnn_amd import meshgen, mesheval, meshgrid, meshremesh          # noqa: E402


def clock(fn):
    """-> (milliseconds on the host clock around fn between two synchronisations, its result)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def spread(x):
    return '%9.4f ms (min %.4f, max %.4f)' % (statistics.median(x), min(x), max(x))


def same_bits(got, want, what):
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1]), \
        '%s: the grid and the all-pairs search differ' % what


def searches(lines, q, pts, fv, rounds, points_too=True):
    """build and search of both grids against the all-pairs calls on (q, pts, fv) -> the TriangleGrid"""
    Q, F, V = q.shape[0], fv.shape[0], pts.shape[0]
    cases = [('triangles', lambda: meshgrid.TriangleGrid(pts, fv), lambda: mesheval.point_to_mesh(q, pts, fv), float(Q) * F)]
    if points_too:
        cases.append(('points', lambda: meshgrid.PointGrid(pts), lambda: mesheval.nearest_point(q, pts), float(Q) * V))
    kept = None
    for name, build, all_pairs, pairs in cases:
        g = build()
        same_bits(g.nearest(q), all_pairs(), name)                     # before anything is timed; also the warm-up
        left = g.left_over
        for _ in range(2):
            build(), g.nearest(q), all_pairs()
        t_build, t_grid, t_all = [], [], []
        for _ in range(rounds):
            t_build.append(clock(build)[0])
            t_grid.append(clock(lambda: g.nearest(q))[0])
            t_all.append(clock(all_pairs)[0])
        lines.append('  %s: Q = %d queries; grid %s = %d cells, %d entries (%.2f per target), %d counting rounds; left over at '
                     'max_rings = %d: %d of %d (%.3f %%)' % (name, Q, 'x'.join(str(d) for d in g.dims), g.cells, g.entries,
                                                             g.entries / max(g.finite, 1), g.rounds, meshgrid.default_rings(),
                                                             left, Q, 100.0 * left / Q))
        lines.append('    %-28s %s' % ('build alone', spread(t_build)))
        lines.append('    %-28s %s' % ('grid search alone', spread(t_grid)))
        lines.append('    %-28s %s   %.3e pair tests' % ('all-pairs search', spread(t_all), pairs))
        lines.append('    %-28s %9.2f x   (with the build: %.2f x)'
                     % ('all pairs / grid search', statistics.median(t_all) / statistics.median(t_grid),
                        statistics.median(t_all) / (statistics.median(t_grid) + statistics.median(t_build))))
        print('\n'.join(lines[-5:]), flush=True)
        kept = kept or g
    return kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--big', type=int, default=256, help='frequency of the large icosphere (0: leave it out)')
    ap.add_argument('--out', type=str, default='')
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_grid.py measures on the MI355X'
    import bench_project
    import bench_remesh
    dev = torch.device('cuda:0')
    lines = ['Grid in front of the nearest searches (csrc/grid.hip) against the all-pairs searches: record of tools/bench_grid.py',
             '%s, torch %s; median of %d in one process after a warm-up, host clock around synchronised calls; the answers '
             'compared bit for bit before any timing' % (torch.cuda.get_device_name(0), torch.__version__, opt.rounds)]
    with torch.cuda.device(dev):
        for freq in bench_project.SIZES:
            pts, fv, L_edge = bench_project.inputs(freq, dev)
            low, high = meshremesh.band(L_edge)
            fr, pr, lock = bench_remesh.phases(pts, fv, low, high)[2]
            relaxed = meshremesh._relax(fr, pr, lock, 0.5)[0]
            lines.append('')
            lines.append('icosphere n = %d: V = %d, F = %d; queries: the %d relaxed vertices of iteration 1 at L = 1.5 mean edges'
                         % (freq, pts.shape[0], fv.shape[0], relaxed.shape[0]))
            searches(lines, relaxed, pts, fv, opt.rounds)

            def whole(index):
                return clock(lambda: meshremesh.remesh(pts, fv, target_edge=L_edge, iterations=5, max_rounds=256, device=dev,
                                                       project=True, index=index))
            a, b = whole(None)[1], whole('grid')[1]
            for field in ('points', 'faces', 'source_face', 'source_bary'):
                assert torch.equal(getattr(a, field).view(torch.int32), getattr(b, field).view(torch.int32)), field
            for _ in range(2):
                whole(None), whole('grid')
            wall, wall_g = [], []
            for _ in range(opt.rounds):
                wall.append(whole(None)[0])
                wall_g.append(whole('grid')[0])
            lines.append('  meshremesh.remesh(target_edge=L, iterations=5, max_rounds=256, project=True), alternating; the same bits:')
            lines.append('    %-28s %s' % ('all pairs', spread(wall)))
            lines.append("    %-28s %s" % ("index='grid'", spread(wall_g)))
            print('\n'.join(lines[-3:]), flush=True)
        if opt.big:
            noisy, clean, faces = meshgen.noisy_icosphere(opt.big, sigma=0.2, seed=1)
            q = torch.from_numpy(noisy.astype(np.float32)).to(dev)
            pts = torch.from_numpy(clean.astype(np.float32)).to(dev)
            fv = torch.from_numpy(faces.astype(np.int32)).to(dev)
            lines.append('')
            lines.append('icosphere n = %d: V = %d, F = %d; queries: its %d vertices with noise of 0.2 mean edges along the normals'
                         % (opt.big, pts.shape[0], fv.shape[0], q.shape[0]))
            searches(lines, q, pts, fv, opt.rounds, points_too=False)
    text = '\n'.join(lines) + '\n'
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, 'w') as fh:
            fh.write(text)
    print(text)


if __name__ == '__main__':
    main()
