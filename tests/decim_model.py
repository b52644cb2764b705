"""Sequential statement of the edge-collapse rules of include/geobi_hip.h (geobi_decim_*), written from that text and not
from the kernels: every step a Python loop over faces, edges or vertices, the float work in Python floats (IEEE fp64, no
contraction) from the float32 inputs, math.sqrt and / correctly rounded.  Also the comparison helper and the case builders
of tests/test_gpu_decim.py.  The mesh builders are those of subdiv_model.py."""
import math
import struct

import numpy as np

import subdiv_model as S

F32 = np.float32
SWEEPS = 3                                     # GEOBI_DECIM_SWEEPS
NONE = 0x7fffffff
COUNT_KEYS = ('edges', 'locked', 'valid', 'collapses', 'V', 'F', 'not_included', 'sweeps_selected')
FAULTS = ('no_link', 'no_valence', 'no_blocking', 'id_order')
HASH_MUL = 0x9E3779B97F4A7C15
PAIRS = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))


def orderable(x):
    """the bits of an fp64 as a uint64 that orders as the numbers do"""
    b = struct.unpack('<Q', struct.pack('<d', x))[0]
    return (~b & 0xffffffffffffffff) if b >> 63 else b | 1 << 63


def edge_hash(lo, hi):
    return ((lo << 24 | hi) * HASH_MUL & 0xffffffffffffffff) >> 32


def normal(pa, pb, pc):
    """n = (b - a) x (c - a), every component two products and one subtraction, and s = (nx nx + ny ny) + nz nz"""
    ux, uy, uz = pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]
    wx, wy, wz = pc[0] - pa[0], pc[1] - pa[1], pc[2] - pa[2]
    nx, ny, nz = uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx
    return nx, ny, nz, (nx * nx + ny * ny) + nz * nz


def face_quadric(pa, pb, pc):
    """the ten entries K_ij = (p_i p_j) / l of the face's plane, None when s == 0"""
    nx, ny, nz, s = normal(pa, pb, pc)
    if s == 0.0:
        return None
    l = math.sqrt(s)
    d = -((nx * pa[0] + ny * pa[1]) + nz * pa[2])
    p = (nx, ny, nz, d)
    return [(p[i] * p[j]) / l for i, j in PAIRS]


def cost_of(q, x, y, z):
    """x^T Q x, x = (x, y, z, 1), in the parenthesisation of the header"""
    diag = ((q[0] * x) * x + (q[4] * y) * y) + (q[7] * z) * z
    off = ((q[1] * x) * y + (q[2] * x) * z) + (q[5] * y) * z
    lin = (q[3] * x + q[6] * y) + q[8] * z
    return (diag + 2.0 * off) + (2.0 * lin + q[9])


def midpoint32(a, b):
    return S.HALF * F32(a) + S.HALF * F32(b)


class Round(object):
    """one round: the outputs of the header and, for the host tests, collapsed [(lo, hi)], candidates {(lo, hi): rank},
    nbrs (the sorted neighbour lists of the round's input)"""


def one_round(points, faces, max_cost=None, budget=None, sweeps=SWEEPS, faults=()):
    """budget: the face count to stop at (None: no limit); max_cost: a float32 or None"""
    assert all(f in FAULTS for f in faults)
    points = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    t = S.Table(faces)
    V, F, E = points.shape[0], t.faces.shape[0], t.E
    P = [tuple(float(x) for x in row) for row in points]
    fv = [tuple(int(x) for x in row) for row in t.faces]
    # 2 locked vertices; the neighbour lists
    locked = [False] * V
    nbrs = [[] for _ in range(V)]
    for e in range(E):
        lo, hi = int(t.lo[e]), int(t.hi[e])
        nbrs[lo].append(hi)
        nbrs[hi].append(lo)
        if t.n[e] != 2:
            locked[lo] = locked[hi] = True
    nbrs = [sorted(x) for x in nbrs]
    # 3 quadrics: the included faces at v in ascending face id
    faces_at = [[] for _ in range(V)]
    for f in range(F):
        if t.included[f]:
            for c in fv[f]:
                faces_at[c].append(f)
    Q = []
    for v in range(V):
        q = [0.0] * 10
        for f in faces_at[v]:
            k = face_quadric(P[fv[f][0]], P[fv[f][1]], P[fv[f][2]])
            if k is not None:
                q = [q[i] + k[i] for i in range(10)]
        Q.append(q)
    # 4, 5 candidates and their validity
    valid = {}                                                      # edge -> (cost key, hash, code)
    for e in range(E):
        lo, hi = int(t.lo[e]), int(t.hi[e])
        if t.n[e] != 2 or (locked[lo] and locked[hi]):
            continue
        q = [Q[lo][i] + Q[hi][i] for i in range(10)]
        mid = tuple(float(midpoint32(points[lo, k], points[hi, k])) for k in range(3))
        places = [(0, P[lo])] if locked[lo] else [(1, P[hi])] if locked[hi] else [(0, P[lo]), (1, P[hi]), (2, mid)]
        cost, code, at = None, None, None
        for c, x in places:
            value = cost_of(q, *x)
            if cost is None or value < cost:
                cost, code, at = value, c, x
        if not math.isfinite(cost) or (max_cost is not None and cost > float(F32(max_cost))):
            continue
        shared = sorted(set(nbrs[lo]) & set(nbrs[hi]))
        if 'no_link' not in faults and len(shared) != 2:
            continue
        if 'no_valence' not in faults and any(len(nbrs[w]) < 4 for w in shared):
            continue
        claimants = [s // 3 for s in t.claimants[e]]
        ok = True
        for v in (lo, hi):
            for f in faces_at[v]:
                if f in claimants:
                    continue
                corners = [P[c] for c in fv[f]]
                nx, ny, nz, s = normal(*corners)
                if s == 0.0:
                    continue
                moved = [at if c == v else P[c] for c in fv[f]]
                mx, my, mz, _ = normal(*moved)
                if not (nx * mx + ny * my) + nz * mz > 0.0:
                    ok = False
        if ok:
            valid[e] = (orderable(cost), e if 'id_order' in faults else edge_hash(lo, hi), code)
    # 6 rank
    order = sorted(valid, key=lambda e: (valid[e][0], valid[e][1], e))
    rank = {e: r for r, e in enumerate(order)}
    # 7 selection
    live, blocked, selected, sweeps_selected = set(order), [False] * V, [], 0
    for _ in range(sweeps):
        m1 = [NONE] * V
        for e in live:
            for v in (int(t.lo[e]), int(t.hi[e])):
                m1[v] = min(m1[v], rank[e])
        m2 = [min([m1[v]] + [m1[w] for w in nbrs[v]]) for v in range(V)]
        now = [e for e in sorted(live) if min(m2[int(t.lo[e])], m2[int(t.hi[e])]) == rank[e]]
        sweeps_selected += 1 if now else 0
        selected += now
        if 'no_blocking' not in faults:
            for e in now:
                for v in (int(t.lo[e]), int(t.hi[e])):
                    blocked[v] = True
                    for w in nbrs[v]:
                        blocked[w] = True
        live = set(e for e in live if e not in now and not blocked[int(t.lo[e])] and not blocked[int(t.hi[e])])
    # 8 budget
    selected.sort(key=lambda e: rank[e])
    n_included = int(t.included.sum())
    if budget is not None:
        selected = selected[:max(0, (n_included - int(budget) + 1) // 2)]
    # 9 emit
    role, partner = [-1] * V, list(range(V))
    gone = np.zeros(F, dtype=bool) | ~t.included
    for e in selected:
        lo, hi = int(t.lo[e]), int(t.hi[e])
        role[lo], partner[lo], role[hi], partner[hi] = valid[e][2], hi, 3, lo
        for s in t.claimants[e]:
            gone[s // 3] = True
    row, rows = [0] * V, 0
    for v in range(V):
        row[v] = rows
        rows += role[v] != 3
    vertex_map = np.array([row[partner[v]] if role[v] == 3 else row[v] for v in range(V)], dtype=np.int32).reshape(-1)
    out_points, parents, place = [], [], []
    for v in range(V):
        if role[v] == 3:
            continue
        parents.append((v, partner[v]))
        place.append(max(role[v], 0))
        out_points.append(points[v] if role[v] <= 0 else points[partner[v]] if role[v] == 1 else
                          midpoint32(points[v], points[partner[v]]))
    face_map = np.nonzero(~gone)[0].astype(np.int32)
    r = Round()
    r.points = np.asarray(out_points, dtype=F32).reshape(-1, 3)
    r.faces = vertex_map[t.faces[face_map]].astype(np.int32).reshape(-1, 3)
    r.face_map, r.vertex_map = face_map, vertex_map
    r.vertex_parents = np.asarray(parents, dtype=np.int32).reshape(-1, 2)
    r.place = np.asarray(place, dtype=np.int8)
    r.counts = dict(zip(COUNT_KEYS, (E, sum(locked), len(order), len(selected), rows, int(face_map.shape[0]),
                                     F - n_included, sweeps_selected)))
    r.collapsed = [(int(t.lo[e]), int(t.hi[e])) for e in selected]
    r.candidates = {(int(t.lo[e]), int(t.hi[e])): rank[e] for e in order}
    r.nbrs = nbrs
    return r


def replay(other, vertex_parents, place):
    """the placements of one round on another point array of the round's input size"""
    other = np.ascontiguousarray(other, dtype=F32).reshape(-1, 3)
    out = np.zeros((vertex_parents.shape[0], 3), dtype=F32)
    for r, ((a, b), code) in enumerate(zip(vertex_parents.tolist(), place.tolist())):
        out[r] = other[a] if code == 0 else other[b] if code == 1 else midpoint32(other[a], other[b])
    return out


class Decimated(object):
    pass


class TooManyRounds(RuntimeError):
    pass


def stop_target(F, target_faces=None, ratio=None):
    """the face count the rounds run to: target_faces, or floor(ratio * F) of the F rows of the input's face table"""
    return int(target_faces) if target_faces is not None else int(math.floor(float(ratio) * F)) if ratio is not None else None


def decimate(points, faces, target_faces=None, ratio=None, max_cost=None, max_rounds=256, sweeps=SWEEPS, faults=()):
    """the whole call, as meshdecim.decimate runs it"""
    points = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    V, F = points.shape[0], faces.shape[0]
    target = stop_target(F, target_faces, ratio)
    d = Decimated()
    d.face_map, d.vertex_map = np.arange(F, dtype=np.int32), np.arange(V, dtype=np.int32)
    d.rounds, d.per_round = [], []
    first, included = None, F
    while F > 0:
        r = one_round(points, faces, max_cost, target, sweeps, faults)
        first = first or r.counts
        included = F - r.counts['not_included']
        if r.counts['collapses'] == 0 and r.counts['not_included'] == 0:
            break
        if len(d.rounds) == max_rounds:
            raise TooManyRounds('%d rounds' % max_rounds)
        d.rounds.append(r)
        d.per_round.append(dict(r.counts))
        points, faces = r.points, r.faces
        d.face_map, d.vertex_map = d.face_map[r.face_map], r.vertex_map[d.vertex_map]
        F = included = r.counts['F']
        if r.counts['collapses'] == 0 or (target is not None and F <= target):
            break
    d.points, d.faces = points, faces
    d.counts = {'edges': first['edges'] if first else 0, 'locked': first['locked'] if first else 0,
                'not_included': first['not_included'] if first else 0,
                'collapses': sum(r.counts['collapses'] for r in d.rounds), 'rounds': len(d.rounds),
                'reached': bool(target is None or included <= target)}
    return d


def apply(decimated, other_points):
    pts = np.ascontiguousarray(other_points, dtype=F32).reshape(-1, 3)
    for r in decimated.rounds:
        pts = replay(pts, r.vertex_parents, r.place)
    return pts


# ---------------------------------------------------------------------------------------------- comparison
bits = S.bits


def assert_same(got, want, name=''):
    """everything exact: faces, face_map, vertex_map int32 and equal, the points equal as uint32 patterns, the counts and
    the counts of every round equal.  got, want: objects with points, faces, face_map, vertex_map (numpy), counts, per_round"""
    for field in ('faces', 'face_map', 'vertex_map'):
        g, w = np.asarray(getattr(got, field)), np.asarray(getattr(want, field))
        assert g.dtype == np.int32, '%s %s: dtype %s' % (name, field, g.dtype)
        assert g.shape == w.shape and np.array_equal(g, w), '%s: %s differ' % (name, field)
    g, w = np.asarray(got.points), np.asarray(want.points)
    assert g.dtype == F32 and g.shape == w.shape, '%s: points %s %s' % (name, g.dtype, g.shape)
    assert np.array_equal(bits(g), bits(w)), '%s: points differ in %d rows' % (name, int((bits(g) != bits(w)).any(axis=1).sum()))
    assert dict(got.counts) == dict(want.counts), '%s: counts %s != %s' % (name, got.counts, want.counts)
    assert list(got.per_round) == list(want.per_round), '%s: the counts of the rounds differ' % name


# ---------------------------------------------------------------------------------------------- mesh facts
def volume(points, faces):
    """the signed fp64 volume of a closed mesh"""
    p, f = np.asarray(points, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    return float((p[f[:, 0]] * np.cross(p[f[:, 1]], p[f[:, 2]])).sum() / 6.0)


def closed_ring(nbrs, v):
    return set(nbrs[v]) | {v}


# ---------------------------------------------------------------------------------------------- case builders
def bipyramid(rim, shuffled=False, seed=2):
    """a closed double cone: the apexes 0 and 1, a rim of `rim` vertices (2 rim faces, 3 rim edges); shuffled: the rim
    numbered in a random order, so that the sorted neighbour lists of the apexes are not the walk around them"""
    rng = np.random.RandomState(seed)
    ang = 2.0 * np.pi * np.arange(rim) / rim
    ring = np.stack([np.cos(ang), np.sin(ang), 0.05 * rng.rand(rim)], axis=1)
    pts = np.concatenate([[[0.0, 0.0, 0.75], [0.0, 0.0, -0.5]], ring]).astype(F32)
    ids = (rng.permutation(rim) if shuffled else np.arange(rim)) + 2
    pts[ids] = pts[2:].copy()
    faces = []
    for k in range(rim):
        a, b = int(ids[k]), int(ids[(k + 1) % rim])
        faces += [(0, a, b), (1, b, a)]
    return pts, np.asarray(faces, dtype=np.int32)


def neck():
    """a closed surface pinched to a triangle of three edges that is no face: the ring r0 r1 r2 between an upper and a
    lower cap of three vertices and one face each.  The ends of a ring edge share THREE neighbours of valence >= 4, so
    only the link test keeps it from collapsing into a surface that touches itself"""
    ang = 2.0 * np.pi * np.arange(3) / 3.0
    ring = np.stack([np.cos(ang), np.sin(ang), np.zeros(3)], axis=1)
    cap = np.stack([0.75 * np.cos(ang + np.pi / 3.0), 0.75 * np.sin(ang + np.pi / 3.0), np.ones(3)], axis=1)
    pts = np.concatenate([ring, cap, cap * [1.0, 1.0, -1.25]]).astype(F32)
    faces = []
    for k in range(3):
        r0, r1, u0, u1, d0, d1 = k, (k + 1) % 3, 3 + k, 3 + (k + 1) % 3, 6 + k, 6 + (k + 1) % 3
        faces += [(r0, r1, u0), (u0, r1, u1), (r1, r0, d0), (r1, d0, d1)]
    faces += [(3, 4, 5), (8, 7, 6)]
    return pts, np.asarray(faces, dtype=np.int32)


def octahedron():
    pts = np.array([[1, 0, 0], [-1, 0, 0.125], [0, 1, 0], [0, -1, 0.25], [0, 0, 1], [0, 0, -1.5]], dtype=F32)
    faces = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    return pts, np.asarray(faces, dtype=np.int32)


def icosphere(n):
    from geobi_gnn_amd import meshgen
    pts, faces = meshgen.icosphere(n)
    return np.ascontiguousarray(pts, dtype=F32), np.ascontiguousarray(faces, dtype=np.int32)


def flat_grid(n=16):
    """an open n x n grid in the plane z = 0 with whole-number coordinates: every cost is exactly 0"""
    return S.grid(n, n)


def dyadic_box():
    """the 1 x 2 x 3 box after three midpoint passes: 768 faces on axis-aligned planes, coordinates multiples of 1 / 8"""
    r = S.subdivide(*S.box(), levels=3)
    return r.points, r.faces


def hand_cases():
    cases = S.hand_cases()
    del cases['sharp_1_2_3']
    cases['octahedron'] = octahedron()
    cases['icosahedron'] = S.icosahedron()
    return cases
