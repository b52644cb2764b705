"""Sequential numpy statement of the refinement rules of include/geobi_hip.h (geobi_subdiv_*), written from that text and
not from the kernels: faces in a Python loop, edges through np.unique of the 48-bit keys, the Loop sums an explicit
ascending loop in np.float64.  Also the case builders and the comparison helper of tests/test_gpu_subdiv.py."""
import numpy as np

MAX_NODES = (1 << 24) - 1
F32, F64 = np.float32, np.float64
HALF = F32(0.5)


class Table(object):
    """included [F] bool; slot_edge [3F] the edge id of every slot (-1: the face is not included); lo, hi, n [E]: the ends
    and the claimant count of every edge, in edge-id order (ascending (lo, hi)); claimants: per edge its slots, ascending"""

    def __init__(self, faces):
        faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
        F = faces.shape[0]
        self.faces = faces
        self.included = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 2] != faces[:, 0])
        a, b = faces.reshape(-1), faces[:, [1, 2, 0]].reshape(-1)                  # slot 3f + k joins c_k and c_k+1
        keys = np.minimum(a, b) << 24 | np.maximum(a, b)
        slots = np.nonzero(np.repeat(self.included, 3))[0]
        uniq, inverse, n = np.unique(keys[slots], return_inverse=True, return_counts=True)
        self.slot_edge = np.full(3 * F, -1, dtype=np.int64)
        self.slot_edge[slots] = inverse
        self.lo, self.hi, self.n = uniq >> 24, uniq & 0xffffff, n
        self.claimants = [[] for _ in range(uniq.shape[0])]
        for s in slots:                                                            # ascending slot order
            self.claimants[self.slot_edge[s]].append(int(s))

    @property
    def E(self):
        return self.lo.shape[0]


def len2(points, lo, hi):
    """(dx * dx + dy * dy) + dz * dz in fp64, d = hi - lo taken in fp64 from the float32 coordinates"""
    d = points[hi].astype(F64) - points[lo].astype(F64)
    return F64((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def midpoint(a, b):
    """0.5f * a + 0.5f * b in float32, per coordinate"""
    return HALF * a.astype(F32) + HALF * b.astype(F32)


class PassRecord(object):
    """what the positions of a pass need: the table, which edges are split, the scheme"""

    def __init__(self, table, split, loop, V):
        self.table, self.split, self.loop, self.V = table, split, loop, V
        self.rank = np.cumsum(split) - split                                       # position among the split edges


def positions(points, rec):
    """points [V, 3] float32 of the pass's input -> [V', 3] float32"""
    t, V = rec.table, rec.V
    points = np.ascontiguousarray(points, dtype=F32)
    out = np.zeros((V + int(rec.split.sum()), 3), dtype=F32)
    out[:V] = points
    with np.errstate(over='ignore', invalid='ignore'):
        if rec.loop:
            sharp = t.n != 2
            nbrs = [[] for _ in range(V)]                                          # (neighbour, sharp) per vertex
            for e in range(t.E):
                nbrs[t.lo[e]].append((int(t.hi[e]), bool(sharp[e])))
                nbrs[t.hi[e]].append((int(t.lo[e]), bool(sharp[e])))
            for v in range(V):
                ring = sorted(nbrs[v])                                             # ascending vertex id
                n, ends = len(ring), [w for w, s in ring if s]
                own = points[v].astype(F64)
                if len(ends) == 0 and n >= 1:
                    beta = 3.0 / 16.0 if n == 3 else 3.0 / (8.0 * n)
                    total = points[ring[0][0]].astype(F64)
                    for w, _ in ring[1:]:
                        total = total + points[w].astype(F64)
                    out[v] = (F64(1.0 - n * beta) * own + F64(beta) * total).astype(F32)
                elif len(ends) == 2:
                    pq = points[ends[0]].astype(F64) + points[ends[1]].astype(F64)
                    out[v] = (F64(0.75) * own + F64(0.125) * pq).astype(F32)
        for e in range(t.E):
            if not rec.split[e]:
                continue
            lo, hi = t.lo[e], t.hi[e]
            if rec.loop and t.n[e] == 2:
                s0, s1 = t.claimants[e]
                c = t.faces[s0 // 3, (s0 % 3 + 2) % 3]
                d = t.faces[s1 // 3, (s1 % 3 + 2) % 3]
                ends = points[lo].astype(F64) + points[hi].astype(F64)
                wings = points[c].astype(F64) + points[d].astype(F64)
                out[V + rec.rank[e]] = (F64(0.375) * ends + F64(0.125) * wings).astype(F32)
            else:
                out[V + rec.rank[e]] = midpoint(points[lo], points[hi])
    return out


def one_pass(points, faces, loop=False, max_edge=None):
    """-> (points', faces', face_parent, vertex_parents, counts, record); max_edge: a float32 length or None (uniform)"""
    points = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    t = Table(faces)
    V, F = points.shape[0], t.faces.shape[0]
    if max_edge is None:
        split = np.ones(t.E, dtype=np.int64)
        l2 = None
    else:
        limit = F64(F32(max_edge)) * F64(F32(max_edge))
        l2 = np.array([len2(points, t.lo[e], t.hi[e]) for e in range(t.E)], dtype=F64)
        split = (l2 > limit).astype(np.int64)
    rec = PassRecord(t, split, loop, V)
    counts = {'edges': t.E, 'split': int(split.sum()), 'boundary_edges': int((t.n == 1).sum()),
              'complex_edges': int((t.n >= 3).sum())}
    vertex_parents = [(v, v) for v in range(V)] + [(int(t.lo[e]), int(t.hi[e])) for e in range(t.E) if split[e]]
    out_faces, parent = [], []
    for f in range(F):
        c = [int(x) for x in t.faces[f]]
        e = [int(t.slot_edge[3 * f + k]) for k in range(3)]
        m = [V + int(rec.rank[e[k]]) if e[k] >= 0 and split[e[k]] else -1 for k in range(3)]
        which = [k for k in range(3) if m[k] >= 0]
        if len(which) == 0:
            kids = [(c[0], c[1], c[2])]
        elif len(which) == 3:
            kids = [(c[0], m[0], m[2]), (c[1], m[1], m[0]), (c[2], m[2], m[1]), (m[0], m[1], m[2])]
        elif len(which) == 1:
            k = which[0]
            a, b, cc = c[k], c[(k + 1) % 3], c[(k + 2) % 3]
            kids = [(a, m[k], cc), (m[k], b, cc)]
        else:
            u = [k for k in range(3) if m[k] < 0][0]
            a, b, cc = c[u], c[(u + 1) % 3], c[(u + 2) % 3]
            e1, e2 = e[(u + 1) % 3], e[(u + 2) % 3]
            p, q = m[(u + 1) % 3], m[(u + 2) % 3]
            first_longer = l2[e1] > l2[e2] or (l2[e1] == l2[e2] and e1 < e2)
            kids = [(p, cc, q)] + ([(a, b, p), (a, p, q)] if first_longer else [(a, b, q), (b, p, q)])
        out_faces.extend(kids)
        parent.extend([f] * len(kids))
    return (positions(points, rec), np.asarray(out_faces, dtype=np.int32).reshape(-1, 3), np.asarray(parent, dtype=np.int32),
            np.asarray(vertex_parents, dtype=np.int32).reshape(-1, 2), counts, rec)


class Refined(object):
    def __init__(self, points, faces, face_parent, vertex_parents, counts, records, per_pass):
        self.points, self.faces, self.face_parent, self.vertex_parents = points, faces, face_parent, vertex_parents
        self.counts, self.records, self.per_pass = counts, records, per_pass


class TooManyRounds(RuntimeError):
    pass


def subdivide(points, faces, levels=1, scheme='midpoint', max_edge=None, max_rounds=16):
    """the whole call: levels uniform passes, or rounds of max_edge until a round splits nothing"""
    points = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    V, F = points.shape[0], faces.shape[0]
    face_parent = np.arange(F, dtype=np.int32)
    vertex_parents = np.stack([np.arange(V, dtype=np.int32)] * 2, axis=1)
    counts = {'edges': 0, 'split': 0, 'boundary_edges': 0, 'complex_edges': 0, 'passes': 0}
    records, per_pass = [], []
    while F > 0 and (max_edge is not None or len(records) < levels):
        p, fv, parent, vp, c, rec = one_pass(points, faces, scheme == 'loop', max_edge)
        if not records:
            counts.update(c, split=0)
        if max_edge is not None and c['split'] == 0:
            break
        if max_edge is not None and len(records) == max_rounds:
            raise TooManyRounds('%d rounds' % max_rounds)
        assert p.shape[0] <= MAX_NODES and fv.shape[0] <= MAX_NODES
        records.append(rec)
        per_pass.append(dict(c, V=p.shape[0], F=fv.shape[0]))
        points, faces, vertex_parents = p, fv, vp
        face_parent = face_parent[parent]
        counts['split'] += c['split']
        F = faces.shape[0]
    counts['passes'] = len(records)
    return Refined(points, faces, face_parent, vertex_parents, counts, records, per_pass)


def apply(refined, other_points):
    pts = np.ascontiguousarray(other_points, dtype=F32).reshape(-1, 3)
    for rec in refined.records:
        pts = positions(pts, rec)
    return pts


# ---------------------------------------------------------------------------------------------- comparison
def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def assert_same(got, want, name=''):
    """everything exact: the integer arrays equal, the points equal as uint32 bit patterns, the counts equal.  got, want:
    objects with points, faces, face_parent, vertex_parents (numpy) and counts"""
    for field in ('faces', 'face_parent', 'vertex_parents'):
        g, w = np.asarray(getattr(got, field)), np.asarray(getattr(want, field))
        assert g.dtype == np.int32, '%s %s: dtype %s' % (name, field, g.dtype)
        assert g.shape == w.shape and np.array_equal(g, w), '%s: %s differ' % (name, field)
    g, w = np.asarray(got.points), np.asarray(want.points)
    assert g.dtype == F32 and g.shape == w.shape, '%s: points %s %s' % (name, g.dtype, g.shape)
    assert np.array_equal(bits(g), bits(w)), '%s: points differ in %d rows' % (name, int((bits(g) != bits(w)).any(axis=1).sum()))
    assert dict(got.counts) == dict(want.counts), '%s: counts %s != %s' % (name, got.counts, want.counts)


# ---------------------------------------------------------------------------------------------- mesh facts
def edge_facts(faces):
    """-> dict: E, boundary, complex, repeated (directed edges walked more than once) of the included faces"""
    t = Table(faces)
    inc = t.faces[t.included]
    directed = np.concatenate([inc[:, [0, 1]], inc[:, [1, 2]], inc[:, [2, 0]]]) if inc.shape[0] else np.zeros((0, 2), np.int64)
    _, n = np.unique(directed[:, 0] << 24 | directed[:, 1], return_counts=True)
    return {'E': t.E, 'boundary': int((t.n == 1).sum()), 'complex': int((t.n >= 3).sum()), 'repeated': int((n > 1).sum())}


def area(points, faces):
    p = np.asarray(points, dtype=F64)
    f = np.asarray(faces, dtype=np.int64)
    return float(0.5 * np.linalg.norm(np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]), axis=1).sum())


def longest_edge2(points, faces):
    t = Table(faces)
    return max(len2(np.asarray(points, dtype=F32), t.lo[e], t.hi[e]) for e in range(t.E))


# ---------------------------------------------------------------------------------------------- case builders
def box(sx=1.0, sy=2.0, sz=3.0):
    """the box of 12 triangles, outward winding, every side cut by the diagonal from its lowest corner"""
    pts = np.array([[x, y, z] for x in (0.0, sx) for y in (0.0, sy) for z in (0.0, sz)], dtype=F32)

    def vid(x, y, z):
        return 4 * x + 2 * y + z
    faces = []
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, 1):
            def corner(i, j):
                c = [0, 0, 0]
                c[axis], c[u], c[w] = side, i, j
                return vid(*c)
            quad = [corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)]       # counter-clockwise seen from +axis
            if side == 0:
                quad = [quad[0], quad[3], quad[2], quad[1]]
            faces += [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]    # quad[0] is the side's lowest corner
    return pts, np.asarray(faces, dtype=np.int32)


def icosahedron(snap=None):
    """snap: the coordinates rounded to multiples of 1 / snap (a power of two): midpoints of several levels are then exact
    in float32 and the area is kept to fp64 rounding"""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    pts = np.array([[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g],
                    [g, 0, -1], [g, 0, 1], [-g, 0, -1], [-g, 0, 1]], dtype=F64)
    pts = (np.round(pts * snap) / snap if snap else pts).astype(F32)
    faces = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2],
                      [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11],
                      [6, 2, 10], [8, 6, 7], [9, 8, 1]], dtype=np.int32)
    return pts, faces


def tetrahedron():
    pts = np.array([[0, 0, 0], [1, 0, 0.25], [0, 1, 0.5], [0.25, 0.5, 1.5]], dtype=F32)
    return pts, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], dtype=np.int32)


def grid(nx, ny, seed=None, regular=False):
    """an open (nx x ny)-cell grid, two triangles per cell, all cut the same way (interior valence 6); z from a seed"""
    xs, ys = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing='ij')
    pts = np.stack([xs.reshape(-1), ys.reshape(-1), np.zeros(xs.size)], axis=1).astype(F32)
    if regular:                                      # a plane that is not axis-aligned, coordinates exact in float32
        pts[:, 2] = 0.5 * pts[:, 0] - 0.25 * pts[:, 1]
    elif seed is not None:
        rng = np.random.RandomState(seed)
        pts += (0.3 * rng.rand(*pts.shape)).astype(F32)
    faces = []
    for i in range(nx):
        for j in range(ny):
            a, b, c, d = i * (ny + 1) + j, (i + 1) * (ny + 1) + j, (i + 1) * (ny + 1) + j + 1, i * (ny + 1) + j + 1
            faces += [(a, b, c), (a, c, d)]
    return pts, np.asarray(faces, dtype=np.int32)


def strip(n_faces, seed=0):
    """a triangle strip of n_faces faces over two rows of vertices"""
    n = n_faces + 2
    rng = np.random.RandomState(seed)
    pts = np.stack([0.5 * np.arange(n), (np.arange(n) % 2).astype(float), np.zeros(n)], axis=1)
    pts = (pts + 0.2 * rng.rand(n, 3)).astype(F32)
    faces = [(k, k + 1, k + 2) if k % 2 == 0 else (k + 1, k, k + 2) for k in range(n_faces)]
    return pts, np.asarray(faces, dtype=np.int32)


def hub(valence, closed=True, seed=3):
    """a fan around vertex 0: closed, the hub is interior (s_v = 0) and the rim vertices have s_v = 2"""
    rng = np.random.RandomState(seed)
    ang = 2.0 * np.pi * np.arange(valence) / valence
    rim = np.stack([np.cos(ang), np.sin(ang), 0.1 * rng.rand(valence)], axis=1)
    pts = np.concatenate([[[0.0, 0.0, 0.5]], rim]).astype(F32)
    order = rng.permutation(valence) + 1             # the rim in a shuffled numbering: the ascending sum is not the walk
    n_faces = valence if closed else valence - 1
    faces = [(0, order[k], order[(k + 1) % valence]) for k in range(n_faces)]
    return pts, np.asarray(faces, dtype=np.int32)


def hand_cases():
    """name -> (points, faces): the smallest inputs at which a kernel can go wrong"""
    rng = np.random.RandomState(11)

    def pts(n):
        return (rng.rand(n, 3) + np.arange(n)[:, None] * [0.7, 0.2, 0.1]).astype(F32)
    cases = {
        'one_triangle': (pts(3), [[0, 1, 2]]),
        'two_consistent': (pts(4), [[0, 1, 2], [2, 1, 3]]),
        'two_inconsistent': (pts(4), [[0, 1, 2], [1, 2, 3]]),
        'tetrahedron': tetrahedron(),
        'three_on_an_edge': (pts(5), [[0, 1, 2], [1, 0, 3], [0, 1, 4]]),
        'duplicated_face': (pts(4), [[0, 1, 2], [0, 1, 2], [2, 1, 3]]),
        'repeated_corner': (pts(5), [[0, 1, 2], [1, 1, 2], [2, 1, 3], [3, 3, 3], [1, 4, 1]]),
        'unreferenced_vertex': (pts(6), [[0, 1, 2], [2, 1, 4]]),
        'sharp_1_2_3': sharp_counts(),
    }
    return {k: (np.asarray(p, dtype=F32), np.asarray(f, dtype=np.int32).reshape(-1, 3)) for k, (p, f) in cases.items()}


def sharp_counts():
    """s_v = 1, 2 and 3 in one mesh: a tetrahedron on the vertices 0 .. 3, and on each of its edges 0-k another closed
    tetrahedron (0, k and two vertices of its own) -- the edge 0-k has four claimants, every other edge two: vertex 0 has three
    sharp edges, the vertices 1, 2, 3 one each; a lone triangle has three vertices with two"""
    rng = np.random.RandomState(5)
    faces = [(0, 2, 1), (0, 1, 3), (1, 2, 3), (2, 0, 3)]
    for k in (1, 2, 3):
        x, y = 2 + 2 * k, 3 + 2 * k
        faces += [(0, k, x), (0, y, k), (0, x, y), (k, y, x)]
    faces.append((10, 11, 12))
    return (rng.rand(13, 3) * 2.0).astype(F32), np.asarray(faces, dtype=np.int32)


def sharp_of(points, faces):
    """s_v of every vertex"""
    t = Table(faces)
    s = np.zeros(np.asarray(points).shape[0], dtype=np.int64)
    for e in range(t.E):
        if t.n[e] != 2:
            s[t.lo[e]] += 1
            s[t.hi[e]] += 1
    return s


def mixed_templates():
    """(points, faces, L): a patch whose edge lengths straddle L, so that faces with 0, 1, 2 and 3 split edges all occur"""
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [3, 0, 0], [3, 3, 0], [0, 3, 0], [1, 1, 0.5], [-1, 0, 0], [0, -1, 0],
                    [4.5, 0.5, 0], [1, -1, 0.25], [3.9, -0.3, 0]], dtype=F32)
    faces = np.array([[0, 1, 2], [1, 3, 4], [1, 4, 2], [2, 4, 5], [0, 7, 8], [0, 2, 7], [3, 9, 4], [0, 8, 1], [8, 10, 1],
                      [1, 10, 3], [3, 11, 9]], dtype=np.int32)
    return pts, faces, 1.5


def exact_length():
    """an edge of length exactly L = 5 (3-4-5, squares exact) beside a longer and a shorter one"""
    pts = np.array([[0, 0, 0], [3, 4, 0], [0, 4, 0], [3, 0, 0], [3, 4, 12]], dtype=F32)
    return pts, np.array([[0, 1, 2], [0, 3, 1], [1, 3, 4]], dtype=np.int32), 5.0


def isosceles(variant):
    """one triangle whose two split edges (the legs, longer than L) have exactly equal len2 and whose base stays; the four
    variants number the apex last or first and wind the face both ways, so that the tie falls on edge u + 1 and on edge u + 2"""
    base_first = np.array([[0, 0, 0], [1, 0, 0], [0.5, 4, 0]], dtype=F32)
    pts = base_first if variant < 2 else base_first[[2, 0, 1]]
    face = ([0, 1, 2], [1, 0, 2], [1, 2, 0], [2, 1, 0])[variant]
    return pts, np.asarray([face], dtype=np.int32), 2.0
