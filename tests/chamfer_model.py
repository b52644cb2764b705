"""fp64 statements of the correspondence-free losses, written in numpy: the nearest-row search (with the gap to the
second-best row), the Chamfer distance and the sided normal loss of one mesh with their gradients, and the inputs they
are checked on.  Shared by tests/test_chamfer_host.py and tests/test_gpu_chamfer.py."""
import numpy as np


def _argmin64(q, t, chunk=256):
    """Per row of q: index of the nearest row of t (lowest among equals), its squared distance and the relative gap to
    the second-best squared distance, all in fp64."""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    idx, d2, gap = np.empty(len(q), np.int64), np.empty(len(q)), np.ones(len(q))
    for s in range(0, len(q), chunk):
        d = ((q[s:s + chunk, None, :] - t[None, :, :]) ** 2).sum(2)
        idx[s:s + chunk] = d.argmin(1)
        d2[s:s + chunk] = d.min(1)
        if t.shape[0] > 1:
            two = np.partition(d, 1, axis=1)[:, :2]
            gap[s:s + chunk] = (two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], 1e-300)
    return idx, d2, gap


def _cd64(p, t):
    """Chamfer distance of one mesh (squared distances, both directions, means) and its gradient to p."""
    p, t = np.asarray(p, np.float64), np.asarray(t, np.float64)
    a, d2a, _ = _argmin64(p, t)
    b, d2b, _ = _argmin64(t, p)
    grad = (2.0 / len(p)) * (p - t[a])
    np.add.at(grad, b, (2.0 / len(t)) * (p[b] - t))
    return d2a.mean() + d2b.mean(), grad


def _sided64(normals_p, normals, fc_p, fc):
    """mean_i sum_c |np_i - n[idx_i]|, idx_i = nearest ground-truth centroid; gradient to np."""
    normals_p, normals = np.asarray(normals_p, np.float64), np.asarray(normals, np.float64)
    idx, _, _ = _argmin64(fc_p, fc)
    d = normals_p - normals[idx]
    return np.abs(d).sum(1).mean(), np.sign(d) / len(d)


_CACHE = {}


def _input(n, s):
    """The frequency-n icosphere as target, a copy jittered by s mean edge lengths (default_rng(5)) as prediction."""
    if (n, s) not in _CACHE:
        from geobi_gnn_amd import meshgen
        pts, faces = meshgen.icosphere(n)
        ev = meshgen.mesh_edges(faces)
        mean_len = np.linalg.norm(pts[ev[:, 0]] - pts[ev[:, 1]], axis=1).mean()
        q = (pts + s * mean_len * np.random.default_rng(5).standard_normal(pts.shape)).astype(np.float32)
        _CACHE[(n, s)] = (q, pts.astype(np.float32), faces)
    return _CACHE[(n, s)]


def _union(parts):
    """[(q, t, faces)] -> q, t, faces of the disjoint union and the vertex / face pointers."""
    vptr = np.cumsum([0] + [len(q) for q, _, _ in parts]).tolist()
    fptr = np.cumsum([0] + [len(f) for _, _, f in parts]).tolist()
    q = np.concatenate([q for q, _, _ in parts])
    t = np.concatenate([t for _, t, _ in parts])
    faces = np.concatenate([f + o for (_, _, f), o in zip(parts, vptr)])
    return q, t, faces, vptr, fptr
