"""The sequential statement of mesh cleaning in plain numpy / Python: a dict of half-edge owners
and one loop over the faces.  Written from the statement of the semantics, not from the kernels; the device path
(geobi_gnn_amd/meshclean.py, csrc/clean.hip) is compared with it exactly.

    weld        canon[v] = lowest index among the vertices with v's key; key = float32 bit patterns of x + 0.0f
                (weld_tol 0), int32 floor(x / weld_tol) in float32 (weld_tol > 0), none (weld_tol None)
    degenerate  two equal corners after canon: dropped
    half-edge   ascending faces; kept iff none of a->b, b->c, c->a is owned by a kept earlier face; kept faces own theirs
    compaction  kept faces / used canonical vertices keep their order and their own coordinates

`rounds` is the depth of the dependency the round-parallel form resolves, stated on the sequential walk: a face without an
earlier claimant on any of its half-edges is decided in round 1; a dropped face one round after the EARLIEST-decided kept
earlier claimant; a kept face one round after the LATEST-decided earlier claimant (all of them dropped).
"""
import numpy as np


class Cleaned(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def weld_keys(points, weld_tol):
    """-> [V, 3] integer keys (uint32 bit patterns or int64 cell numbers); ValueError for a cell outside int32."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    if weld_tol == 0.0:
        return (p + np.float32(0.0)).view(np.uint32).astype(np.int64)
    q = np.floor(p / np.float32(weld_tol))                       # float32 division, correctly rounded
    if q.size and (q.min() < -2147483648.0 or q.max() >= 2147483648.0):
        raise ValueError('quotient outside the int32 range')
    return q.astype(np.int64)


def clean(points, faces, weld_tol=0.0, manifold=True):
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V, F = points.shape[0], faces.shape[0]
    canon = np.arange(V, dtype=np.int64)
    if weld_tol is not None:
        first = {}
        for v, key in enumerate(map(tuple, weld_keys(points, weld_tol).tolist())):
            canon[v] = first.setdefault(key, v)
    groups = len(set(canon.tolist()))
    owner = {}                 # half-edge -> the kept face that owns it
    claimants = {}             # half-edge -> every earlier non-degenerate face that lists it
    decided = {}               # face -> round in which the round-parallel form decides it
    kept, degenerate, nonmanifold = [], 0, 0
    for f in range(F):
        a, b, c = (int(canon[x]) for x in faces[f])
        if a == b or b == c or c == a:
            degenerate += 1
            continue
        edges = [(a, b), (b, c), (c, a)]
        if not manifold:
            kept.append(f)
            continue
        owners = [owner[e] for e in edges if e in owner]
        earlier = [g for e in edges for g in claimants.get(e, [])]
        if owners:
            nonmanifold += 1
            decided[f] = 1 + min(decided[g] for g in owners)
        else:
            kept.append(f)
            decided[f] = 1 + max([decided[g] for g in earlier] or [0])
            for e in edges:
                owner[e] = f
        for e in edges:
            claimants.setdefault(e, []).append(f)
    fc = canon[faces[kept]] if kept else np.zeros((0, 3), dtype=np.int64)
    used = np.zeros(V, dtype=bool)
    used[fc.reshape(-1)] = True
    new_index = np.cumsum(used) - 1
    vertex_map = np.where(used[canon], new_index[canon], -1).astype(np.int32) if V else np.zeros(0, np.int32)
    vertex_src = np.nonzero(used)[0].astype(np.int32)
    return Cleaned(points=points[used], faces=new_index[fc].astype(np.int32).reshape(-1, 3), vertex_map=vertex_map,
                   vertex_src=vertex_src, face_map=np.asarray(kept, dtype=np.int32), canon=canon.astype(np.int32),
                   counts={'welded': V - groups, 'degenerate': degenerate, 'nonmanifold': nonmanifold,
                           'unreferenced': int((vertex_map < 0).sum()), 'rounds': max(decided.values()) if decided else 0})


def soup(points, faces):
    """Every face with its own three vertices (what an STL-derived OBJ is): (points [3F, 3], faces [F, 3])."""
    points, faces = np.asarray(points), np.asarray(faces).reshape(-1, 3)
    return (np.ascontiguousarray(points[faces.reshape(-1)], dtype=np.float32),
            np.arange(3 * faces.shape[0], dtype=np.int32).reshape(-1, 3))
