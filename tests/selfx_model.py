"""Two independent statements of the self-intersection search (include/geobi_hip.h: geobi_self_intersections).

``exact_*``   the DEFINITION, in Python integers and ``fractions.Fraction``: two included faces a < b that share k vertex
              ids intersect iff the closed triangles share a point (k = 0), a point other than the shared vertex (k = 1), a
              point off the shared edge (k = 2); never for k = 3.  The shared points are computed as a set, not decided by
              predicates: a pair that is not coplanar cuts A with B's plane to a segment, a point or nothing and clips that by
              B's three in-plane half-spaces; a coplanar pair clips the polygon A by the same three half-spaces.  What is
              left is the convex hull of a short list of points, and the three questions are questions about that list.
              Integer coordinates only.
``search``    the kernel's DECISION PROCEDURE in numpy fp64, every operation in the order the header states, vectorised
              over the pairs whose float32 boxes overlap: hits, the ordered pair list and the eight counts.  For integer
              coordinates of magnitude <= 2^14 every intermediate is exact, so it must agree with ``exact_pairs``; for
              general floats it is what the kernel must reproduce exactly.  ``fault`` plants a mistake in it (the host
              test shows that the exact statement catches each).

Also the cases: ``hand_cases`` (a few faces each, integer coordinates, with the expected pairs written down by hand),
``soup`` (random integer triangle soups over few vertices in a small cube, so that shared vertices, shared edges, coplanar
and touching pairs are common) and ``pushed_sphere``."""
from fractions import Fraction

import numpy as np

COUNT_KEYS = ('pairs', 'pairs_k0', 'pairs_k1', 'pairs_k2', 'faces_hit', 'degenerate', 'included', 'box_candidates')
TILE, QUERY_BLOCK = 256, 512            # kTile and kThreads * kQpl of csrc/selfx.hip
SOUP_SEEDS = (2, 4, 7)          # chosen on the host: every class occurs both ways and every planted fault shows in each


# ------------------------------------------------------------------------------------------------ the exact statement
def _sub(u, w):
    return (u[0] - w[0], u[1] - w[1], u[2] - w[2])


def _cross(u, w):
    return (u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0])


def _dot(u, w):
    return u[0] * w[0] + u[1] * w[1] + u[2] * w[2]


def _lerp(p, q, t):
    return tuple(p[i] + t * (q[i] - p[i]) for i in range(3))


def _clip(points, g):
    """the convex set spanned by ``points`` (one point, the two ends of a segment, or the corners of a convex polygon in
    order) cut by the closed half-space g(x) >= 0, g affine -> the same kind of list (possibly empty)"""
    if len(points) <= 1:
        return [p for p in points if g(p) >= 0]
    out = []
    n = len(points)
    edges = [(0, 1)] if n == 2 else [(i, (i + 1) % n) for i in range(n)]
    for i, j in edges:
        p, q = points[i], points[j]
        gp, gq = g(p), g(q)
        if gp >= 0:
            out.append(p)
        if (gp > 0 and gq < 0) or (gp < 0 and gq > 0):
            out.append(_lerp(p, q, Fraction(gp) / Fraction(gp - gq)))
        if n == 2 and gq >= 0:
            out.append(q)
    uniq = []
    for p in out:
        if p not in uniq:
            uniq.append(p)
    return uniq


def exact_degenerate(tri, ids):
    return len(set(ids)) < 3 or _cross(_sub(tri[1], tri[0]), _sub(tri[2], tri[0])) == (0, 0, 0)


def exact_common(A, B):
    """the points that span A n B (closed triangles of integer corners): [] iff they are disjoint"""
    nB = _cross(_sub(B[1], B[0]), _sub(B[2], B[0]))
    d = [_dot(nB, _sub(a, B[0])) for a in A]
    if all(x == 0 for x in d):
        part = list(A)                                      # coplanar: the polygon A itself
    else:
        part = [A[i] for i in range(3) if d[i] == 0]        # A cut with B's plane: corners in it, edges through it
        for i, j in ((0, 1), (1, 2), (2, 0)):
            if (d[i] > 0 and d[j] < 0) or (d[i] < 0 and d[j] > 0):
                part.append(_lerp(A[i], A[j], Fraction(d[i]) / Fraction(d[i] - d[j])))
        assert len(part) <= 2
    for i, j, k in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):       # B's in-plane half-space of the edge ij: the side of corner k
        inward = _cross(nB, _sub(B[j], B[i]))
        sign = 1 if _dot(inward, _sub(B[k], B[i])) > 0 else -1
        part = _clip(part, lambda x, inward=inward, sign=sign, o=B[i]: sign * _dot(inward, _sub(x, o)))
    return part


def _on_segment(x, u, v):
    e, w = _sub(v, u), _sub(x, u)
    return _cross(w, e) == (0, 0, 0) and 0 <= _dot(w, e) <= _dot(e, e)


def exact_pair(verts, fa, fb):
    """-> (k, intersects) for two included faces given as id triples"""
    A, B = [tuple(int(c) for c in verts[i]) for i in fa], [tuple(int(c) for c in verts[i]) for i in fb]
    shared = [i for i in fa if i in fb]
    k = len(shared)
    if k == 3:
        return 3, False
    common = exact_common(A, B)
    if k == 0:
        return 0, len(common) > 0
    s = tuple(int(c) for c in verts[shared[0]])
    if k == 1:
        return 1, any(p != s for p in common)
    t = tuple(int(c) for c in verts[shared[1]])
    return 2, any(not _on_segment(p, s, t) for p in common)


def exact_pairs(verts, faces, state=None):
    """every intersecting pair (a, b, k), a < b, in ascending order: all pairs, no box test"""
    verts, faces = np.asarray(verts), np.asarray(faces)
    assert np.issubdtype(verts.dtype, np.integer) or np.array_equal(verts, np.round(verts))
    rows = [tuple(int(i) for i in f) for f in faces]
    tri = [[tuple(int(c) for c in verts[i]) for i in f] for f in rows]
    inc = [(state is None or int(state[f]) == 1) and not exact_degenerate(tri[f], rows[f]) for f in range(len(rows))]
    out = []
    for a in range(len(rows)):
        for b in range(a + 1, len(rows)):
            if inc[a] and inc[b]:
                k, hit = exact_pair(verts, rows[a], rows[b])
                if hit:
                    out.append((a, b, k))
    return out


def exact_classes(verts, faces):
    """{(k, intersects): count} over all pairs of included faces with k < 3"""
    verts, faces = np.asarray(verts), np.asarray(faces)
    rows = [tuple(int(i) for i in f) for f in faces]
    seen = {}
    for a in range(len(rows)):
        for b in range(a + 1, len(rows)):
            ta, tb = [tuple(int(c) for c in verts[i]) for i in rows[a]], [tuple(int(c) for c in verts[i]) for i in rows[b]]
            if exact_degenerate(ta, rows[a]) or exact_degenerate(tb, rows[b]):
                continue
            key = exact_pair(verts, rows[a], rows[b])
            if key[0] < 3:
                seen[key] = seen.get(key, 0) + 1
    return seen


# ------------------------------------------------------------------------------------------------ the order statement
def _vsub(u, w):
    return u - w


def _vcross(u, w):
    return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                     u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)


def _vdot(u, w):
    return (u[:, 0] * w[:, 0] + u[:, 1] * w[:, 1]) + u[:, 2] * w[:, 2]


def _same_side(a, b):
    return ((a > 0) & (b > 0)) | ((a < 0) & (b < 0))


def _one_side(a, b, c):
    return ((a > 0) & (b > 0) & (c > 0)) | ((a < 0) & (b < 0) & (c < 0))


def _no_sign_change(a, b, c, strict=False):
    if strict:
        return _one_side(a, b, c)
    return ((a >= 0) & (b >= 0) & (c >= 0)) | ((a <= 0) & (b <= 0) & (c <= 0))


def _axis(n):
    ax = np.zeros(n.shape[0], dtype=np.int64)
    m = np.abs(n[:, 0])
    up = np.abs(n[:, 1]) > m
    ax[up] = 1
    m = np.where(up, np.abs(n[:, 1]), m)
    ax[np.abs(n[:, 2]) > m] = 2
    return ax


def _flat(p, ax):
    return np.where(ax == 0, p[:, 1], p[:, 0]), np.where(ax == 2, p[:, 1], p[:, 2])


def _o2(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def _seg_seg(p, q, c, d):
    o1, o2, o3, o4 = _o2(p, q, c), _o2(p, q, d), _o2(c, d, p), _o2(c, d, q)
    line = (o1 == 0) & (o2 == 0) & (o3 == 0) & (o4 == 0)
    boxes = ((np.maximum(np.minimum(p[0], q[0]), np.minimum(c[0], d[0])) <= np.minimum(np.maximum(p[0], q[0]), np.maximum(c[0], d[0])))
             & (np.maximum(np.minimum(p[1], q[1]), np.minimum(c[1], d[1])) <= np.minimum(np.maximum(p[1], q[1]), np.maximum(c[1], d[1]))))
    return np.where(line, boxes, ~_same_side(o1, o2) & ~_same_side(o3, o4))


def _seg_tri(p, q, t0, t1, t2, n, dp, dq, fault):
    ax = _axis(n)
    p2, q2, a, b, c = _flat(p, ax), _flat(q, ax), _flat(t0, ax), _flat(t1, ax), _flat(t2, ax)
    flat_hit = (_no_sign_change(_o2(a, b, p2), _o2(b, c, p2), _o2(c, a, p2)) | _seg_seg(p2, q2, a, b) | _seg_seg(p2, q2, b, c)
                | _seg_seg(p2, q2, c, a))
    if fault == 'no_coplanar':
        flat_hit = np.zeros_like(flat_hit)
    d, u0, u1, u2 = _vsub(q, p), _vsub(t0, p), _vsub(t1, p), _vsub(t2, p)
    through = _no_sign_change(_vdot(d, _vcross(u0, u1)), _vdot(d, _vcross(u1, u2)), _vdot(d, _vcross(u2, u0)),
                              strict=fault == 'touching_apart')
    apart = _same_side(dp, dq)
    if fault == 'touching_apart':
        apart = apart | (dp == 0) | (dq == 0)
    return ~apart & np.where((dp == 0) & (dq == 0), flat_hit, through)


def _take(c, i):
    """corner i[n] of c [n, 3, 3]"""
    return c[np.arange(c.shape[0]), i]


def included(verts, faces, state=None):
    """-> (included [F] bool, degenerate: the faces that pass the state and fail an id or the area test)"""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok_state = np.ones(f.shape[0], dtype=bool) if state is None else np.asarray(state).reshape(-1) == 1
    in_range = ((f >= 0) & (f < v.shape[0])).all(1)
    g = np.where(in_range[:, None], f, 0)
    distinct = (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 2] != g[:, 0])
    if v.shape[0]:
        n = _vcross(v[g[:, 1]] - v[g[:, 0]], v[g[:, 2]] - v[g[:, 0]])
        area = ~((n[:, 0] == 0) & (n[:, 1] == 0) & (n[:, 2] == 0))
    else:
        area = np.zeros(f.shape[0], dtype=bool)
    inc = ok_state & in_range & distinct & area
    return inc, int((ok_state & ~inc).sum())


class Found(object):
    """hits [F] int32, pairs [P, 2] int32 ascending, ks [P] (the k of every pair), counts: dict over COUNT_KEYS"""

    def __init__(self, hits, pairs, ks, counts):
        self.hits, self.pairs, self.ks, self.counts = hits, pairs, ks, counts


def search(verts, faces, state=None, fault=None):
    """the kernel's procedure -> Found"""
    v32 = np.asarray(verts, dtype=np.float32)
    v = v32.astype(np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    F = f.shape[0]
    inc, degenerate = included(v32, f, state)
    g = np.where(inc[:, None], f, 0)
    corners32 = v32[g] if v32.shape[0] else np.zeros((F, 3, 3), dtype=np.float32)
    lo, hi = corners32.min(1), corners32.max(1)
    over = inc[:, None] & inc[None, :]
    for k in range(3):
        over &= (lo[:, None, k] <= hi[None, :, k]) & (lo[None, :, k] <= hi[:, None, k])
    cand = np.argwhere(np.triu(over, 1))                    # ascending (a, b)
    a, b = cand[:, 0], cand[:, 1]
    match = f[a][:, :, None] == f[b][:, None, :]            # [n, corner of A, corner of B]
    sa, sb = match.any(2), match.any(1)
    k = sa.sum(1)
    keep = k < 3
    a, b, sa, sb, k = a[keep], b[keep], sa[keep], sb[keep], k[keep]
    A, B = v[f[a]], v[f[b]]                                 # [n, 3, 3]
    a0, a1, a2, b0, b1, b2 = A[:, 0], A[:, 1], A[:, 2], B[:, 0], B[:, 1], B[:, 2]
    nA, nB = _vcross(_vsub(a1, a0), _vsub(a2, a0)), _vcross(_vsub(b1, b0), _vsub(b2, b0))
    db = [_vdot(nA, _vsub(x, a0)) for x in (b0, b1, b2)]
    da = [_vdot(nB, _vsub(x, b0)) for x in (a0, a1, a2)]
    # k = 0
    hit0 = np.zeros(a.shape[0], dtype=bool)
    for i, j in ((0, 1), (1, 2), (2, 0)):
        hit0 |= _seg_tri(B[:, i], B[:, j], a0, a1, a2, nA, db[i], db[j], fault)
        hit0 |= _seg_tri(A[:, i], A[:, j], b0, b1, b2, nB, da[i], da[j], fault)
    hit0 &= ~(_one_side(*db) | _one_side(*da))
    # k = 1: the edges opposite the shared corners i of A and j of B
    i, j = np.argmax(sa, 1), np.argmax(sb, 1)
    i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
    dA, dB = np.stack(da, 1), np.stack(db, 1)
    rows = np.arange(a.shape[0])
    hit1 = (_seg_tri(_take(A, i1), _take(A, i2), b0, b1, b2, nB, dA[rows, i1], dA[rows, i2], fault)
            | _seg_tri(_take(B, j1), _take(B, j2), a0, a1, a2, nA, dB[rows, j1], dB[rows, j2], fault))
    if fault == 'no_k1':
        hit1 = np.zeros_like(hit1)
    # k = 2: the corners off the shared edge
    ia, ib = np.argmin(sa, 1), np.argmin(sb, 1)
    pa, u, w, pb = _take(A, ia), _take(A, (ia + 1) % 3), _take(A, (ia + 2) % 3), _take(B, ib)
    ax = _axis(nA)
    u2, w2 = _flat(u, ax), _flat(w, ax)
    hit2 = (_vdot(nA, _vsub(pb, a0)) == 0) & _same_side(_o2(u2, w2, _flat(pa, ax)), _o2(u2, w2, _flat(pb, ax)))
    if fault == 'no_coplanar':
        hit2 = np.zeros_like(hit2)
    hit = np.where(k == 0, hit0, np.where(k == 1, hit1, hit2))
    pairs = np.stack([a[hit], b[hit]], 1).astype(np.int32)
    ks = k[hit]
    hits = (np.bincount(pairs[:, 0], minlength=F) + np.bincount(pairs[:, 1], minlength=F)).astype(np.int32)
    counts = {'pairs': int(hit.sum()), 'pairs_k0': int((ks == 0).sum()), 'pairs_k1': int((ks == 1).sum()),
              'pairs_k2': int((ks == 2).sum()), 'faces_hit': int((hits > 0).sum()), 'degenerate': degenerate,
              'included': int(inc.sum()), 'box_candidates': int(a.shape[0])}
    return Found(hits, pairs, ks, counts)


def pair_set(found):
    return [(int(a), int(b), int(k)) for (a, b), k in zip(found.pairs, found.ks)]


# ------------------------------------------------------------------------------------------------ cases
_A = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]           # the triangle every hand case starts from: vertices 0, 1, 2, face 0


def _case(extra_vertices, faces, pairs, state=None):
    return (np.array(_A + extra_vertices, dtype=np.int64), np.array(faces, dtype=np.int32),
            None if state is None else np.array(state, dtype=np.int32), pairs)


def hand_cases():
    """name -> (verts int64 [V, 3], faces int32 [F, 3], state or None, the intersecting pairs (a, b, k) written by hand)"""
    other = [[0, 1, 2], [3, 4, 5]]
    c = {}
    # k = 0
    c['k0_through_the_interior'] = _case([(1, 1, -2), (1, 1, 2), (2, 2, 3)], other, [(0, 1, 0)])
    c['k0_vertex_in_the_face'] = _case([(1, 1, 0), (1, 1, 3), (2, 1, 3)], other, [(0, 1, 0)])
    c['k0_vertex_on_an_edge'] = _case([(2, 0, 0), (2, 0, 3), (3, 0, 3)], other, [(0, 1, 0)])
    c['k0_vertex_on_a_vertex_of_another_index'] = _case([(4, 0, 0), (4, 0, 3), (5, 0, 3)], other, [(0, 1, 0)])
    c['k0_edges_cross_in_one_point'] = _case([(2, -1, -1), (2, 1, 1), (2, -1, 3)], other, [(0, 1, 0)])
    c['k0_coplanar_overlap'] = _case([(1, 1, 0), (5, 1, 0), (1, 5, 0)], other, [(0, 1, 0)])
    c['k0_one_inside_the_other'] = _case([(1, 1, 0), (2, 1, 0), (1, 2, 0)], other, [(0, 1, 0)])
    c['k0_coplanar_apart'] = _case([(3, 3, 0), (5, 3, 0), (3, 5, 0)], other, [])
    c['k0_parallel_planes'] = _case([(0, 0, 1), (4, 0, 1), (0, 4, 1)], other, [])
    c['k0_boxes_overlap_triangles_apart'] = _case([(3, 3, -1), (3, 3, 1), (4, 4, 0)], other, [])
    # k = 1: vertex 0 is shared
    c['k1_clean_fan'] = _case([(-1, -1, 3), (-3, 1, 3)], [[0, 1, 2], [0, 3, 4]], [])
    c['k1_opposite_edge_through_the_face'] = _case([(1, 1, -2), (1, 1, 2)], [[0, 1, 2], [3, 0, 4]], [(0, 1, 1)])
    c['k1_coplanar_wedges_overlap'] = _case([(3, 1, 0), (1, 3, 0)], [[0, 1, 2], [4, 3, 0]], [(0, 1, 1)])
    c['k1_coplanar_contact_in_the_vertex_alone'] = _case([(-4, 0, 0), (0, -4, 0)], [[0, 1, 2], [0, 3, 4]], [])
    # k = 2: the edge 0 1 is shared
    c['k2_dihedral'] = _case([(2, -1, 3)], [[0, 1, 2], [1, 0, 3]], [])
    c['k2_flat_unfolded'] = _case([(2, -4, 0)], [[0, 1, 2], [1, 0, 3]], [])
    c['k2_folded_flat'] = _case([(1, 2, 0)], [[0, 1, 2], [1, 0, 3]], [(0, 1, 2)])
    c['k2_folded_flat_same_winding'] = _case([(3, 1, 0)], [[2, 0, 1], [0, 1, 3]], [(0, 1, 2)])
    # never counted, never included (face 2 of each passes through what is left out, and through face 0)
    through = [(1, 1, -2), (1, 1, 2), (2, 2, 3)]
    c['k3_duplicates'] = _case(through, [[0, 1, 2], [1, 2, 0], [3, 4, 5], [2, 1, 0]], [(0, 2, 0), (1, 2, 0), (2, 3, 0)])
    c['repeated_index'] = _case(through, [[0, 1, 2], [3, 4, 4], [3, 4, 5]], [(0, 2, 0)])
    c['zero_area'] = _case(through + [(1, 1, 0), (2, 2, 0), (3, 3, 0)], [[0, 1, 2], [6, 7, 8], [3, 4, 5]], [(0, 2, 0)])
    c['excluded_by_state'] = _case(through, [[0, 1, 2], [3, 4, 5], [3, 4, 5]], [], state=[1, 0, 2])
    return c


def soup(seed, F=96, V=24, extent=6):
    """a random triangle soup: V integer vertices in [-extent, extent]^3, F id triples (some with a repeated id)"""
    rng = np.random.RandomState(seed)
    return rng.randint(-extent, extent + 1, (V, 3)).astype(np.int64), rng.randint(0, V, (F, 3)).astype(np.int32)


def scaled(verts):
    """the same soup on coordinates of magnitude up to 2^14: still exact"""
    out = verts * 1024 + np.array([3000, -2000, 1000], dtype=np.int64)
    assert np.abs(out).max() <= 1 << 14
    return out


def pushed_sphere(points, seed=7, pushed=(0, 5, 11, 17, 40), jitter=0.01):
    """a closed sphere mesh with a fixed handful of vertices pushed through the opposite side, then float jitter"""
    p = np.array(points, dtype=np.float64)
    p[list(pushed)] *= -1.3
    p += np.random.RandomState(seed).standard_normal(p.shape) * jitter
    return p.astype(np.float32)
