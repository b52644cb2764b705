"""Cost of the mesh topology stage (csrc/topo.hip, geobi_gnn_amd/meshtopo.py) on the MI355X, the record behind
profiles/meshtopo.txt.

  python tools/bench_topo.py [--out profiles/meshtopo.txt]

Input: the scan-sized mesh of BASELINE.json configs[3] (icosphere n = 87: F = 151 380, V = 75 692) as it is, with half
of its faces reversed, and with half reversed and the face order shuffled.  In ONE process, after a warm-up of every
shape, median of --rounds (20) measurements, the calls alternating round by round:

  orient / components      device events at the stage borders INSIDE one call of geobi_topo_orient / _components (their
                           stage_ms argument): the edge table (slots, 48-bit sort, links), the rounds with the waits of
                           their batches, and the rest (orient: parity check and outputs; components: sizes and outputs)
  clean_mesh               host clock around the whole synchronous call, without and with orient=True, min_component=2
  host scipy               scipy.sparse.csgraph.connected_components on the same face adjacency (built outside the clock
                           from the model's component links): the labelling a user would run on the host

and the round counts, which are functions of the input.
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from geobi_gnn_amd import meshclean, meshgen, meshtopo         # noqa: E402
import topo_model as T                                         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--freq', type=int, default=87)
    ap.add_argument('--out', type=str, default='')
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_topo.py measures on the MI355X'
    dev = torch.device('cuda:0')
    lines = ['Mesh topology (csrc/topo.hip): cost record of tools/bench_topo.py',
             '%s, torch %s; median of %d, the calls alternating in one process after a warm-up; device events at the stage '
             'borders inside a call, host clock for clean_mesh and for scipy' % (torch.cuda.get_device_name(0), torch.__version__,
                                                                                  opt.rounds)]
    points, faces = meshgen.icosphere(opt.freq)
    points, faces = points.astype(np.float32), faces.astype(np.int32)
    V = points.shape[0]
    inputs = (('as is', faces), ('half reversed', T.mess_up(faces, 1, shuffle=False)),
              ('half reversed, shuffled', T.mess_up(faces, 1, shuffle=True)))
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        connected_components = None
    for name, fv_host in inputs:
        pts, fv = torch.from_numpy(points).to(dev), torch.from_numpy(fv_host).to(dev)
        F = fv.shape[0]
        for _ in range(3):                       # warm-up of every shape that is timed
            plain = meshclean.clean_mesh(pts, fv, device=dev)
            both = meshclean.clean_mesh(pts, fv, orient=True, min_component=2, device=dev)
        torch.cuda.synchronize()
        graph = None
        if connected_components is not None:
            l = np.asarray(T.links(fv_host)[1], dtype=np.int64)
            graph = coo_matrix((np.ones(l.shape[0], dtype=np.int8), (l[:, 0], l[:, 1])), shape=(F, F)).tocsr()
        keys = ['o_table', 'o_rounds', 'o_rest', 'c_table', 'c_rounds', 'c_rest', 'clean_plain', 'clean_topo', 'scipy']
        ms = {k: [] for k in keys}
        for _ in range(opt.rounds):
            stage = (ctypes.c_float * 3)()
            _, _, _, _, orient_rounds = meshtopo.orient_device(fv, V, None, 256, stage)
            for k, v in zip(keys[0:3], stage):
                ms[k].append(v)
            stage = (ctypes.c_float * 3)()
            _, _, _, component_rounds = meshtopo.components_device(fv, V, None, 2, 256, stage)
            for k, v in zip(keys[3:6], stage):
                ms[k].append(v)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            meshclean.clean_mesh(pts, fv, device=dev)
            ms['clean_plain'].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            meshclean.clean_mesh(pts, fv, orient=True, min_component=2, device=dev)
            ms['clean_topo'].append(1e3 * (time.perf_counter() - t0))
            if graph is not None:
                t0 = time.perf_counter()
                n_parts, _ = connected_components(graph, directed=False)
                ms['scipy'].append(1e3 * (time.perf_counter() - t0))
                assert n_parts == both.topology['components']
        assert orient_rounds == both.topology['orient_rounds']
        lines.append('')
        lines.append('%s: V = %d, F = %d; clean_mesh alone keeps %d faces in %d rounds, with orient %d (flipped %d); orient '
                     'rounds %d, component rounds %d'
                     % (name, V, F, plain.faces.shape[0], plain.counts['rounds'], both.faces.shape[0], both.topology['flipped'],
                        orient_rounds, component_rounds))
        for key, label in (('o_table', 'geobi_topo_orient: edge table (slots, 48-bit sort, links)'),
                           ('o_rounds', 'geobi_topo_orient: rounds, their copies and waits'),
                           ('o_rest', 'geobi_topo_orient: parity check, outputs'),
                           ('c_table', 'geobi_topo_components: edge table'),
                           ('c_rounds', 'geobi_topo_components: rounds, their copies and waits'),
                           ('c_rest', 'geobi_topo_components: sizes, outputs'),
                           ('clean_plain', 'meshclean.clean_mesh, host clock, synchronous'),
                           ('clean_topo', 'meshclean.clean_mesh(orient=True, min_component=2), host clock'),
                           ('scipy', 'host scipy connected_components (labels only, graph prebuilt)')):
            v = ms[key]
            if not v:
                lines.append('  %-66s NOT MEASURED (scipy is not installed)' % label)
                continue
            lines.append('  %-66s %9.4f ms (min %9.4f, max %9.4f)' % (label, statistics.median(v), min(v), max(v)))
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
