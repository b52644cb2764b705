"""Per-sample rotation of a union batch: geobi_rotate_parts (data.rotate_union, one launch per graph) against the torch
form it replaces (RandomRotate.__call__'s slice-and-matmul, applied per mesh), alternated in one process, device events.

  python tools/bench_rotate.py [--freq 32] [--meshes 4] [--reps 200]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geobi_gnn_amd import meshgen, meshprep                                   # noqa: E402
from geobi_gnn_amd.data import RandomRotate, rotate_union, union_batch_graphs   # noqa: E402


def torch_form(dv, df, mats):
    """What a per-mesh rotation costs without the kernel: per graph and mesh a slice, a 3x3 matmul and a strided
    write-back for x[:, 0:3], x[:, 3:6] and y.  mats: device fp32 [B, 3, 3] (uploaded outside the timed region)."""
    for d in (dv, df):
        ptr = d.mesh_ptr.tolist()
        for k in range(len(ptr) - 1):
            a, b, r = ptr[k], ptr[k + 1], mats[k]
            d.x[a:b, 0:3] = d.x[a:b, 0:3] @ r
            d.x[a:b, 3:6] = d.x[a:b, 3:6] @ r
            d.y[a:b] = d.y[a:b] @ r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--freq', type=int, default=32)
    ap.add_argument('--meshes', type=int, default=4)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    opt = ap.parse_args()
    dev = torch.device('cuda:0')
    parts = []
    for i in range(opt.meshes):
        noisy, clean, faces = meshgen.noisy_icosphere(opt.freq, 0.2, seed=i)
        parts.append(meshprep.build_dual_data(noisy, faces, clean, device=dev))
    dv, df = union_batch_graphs(parts)
    mats = RandomRotate(z_rotated=False, rng=np.random.default_rng(0)).matrices(opt.meshes)
    mats_dev = torch.from_numpy(mats).to(device=dev, dtype=torch.float32)
    forms = {'geobi_rotate_parts': lambda: rotate_union(dv, df, mats), 'torch per mesh': lambda: torch_form(dv, df, mats_dev)}
    for _ in range(opt.warmup):
        for fn in forms.values():
            fn()
    times = {k: [] for k in forms}
    for _ in range(opt.reps):
        for name, fn in forms.items():            # alternated: both see the same clocks and the same cache state
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    out = {'freq': opt.freq, 'meshes': opt.meshes, 'reps': opt.reps, 'rows_v': int(dv.x.shape[0]), 'rows_f': int(df.x.shape[0]),
           'bytes_moved': int(2 * 4 * 9 * (dv.x.shape[0] + df.x.shape[0])),
           'launches_per_step': {'geobi_rotate_parts': 2, 'torch per mesh': 2 * opt.meshes * 6}}
    for name, t in times.items():
        t = np.sort(np.asarray(t))
        out[name] = {'median_us': round(float(np.median(t)), 2), 'p10_us': round(float(t[len(t) // 10]), 2),
                     'p90_us': round(float(t[(9 * len(t)) // 10]), 2)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
