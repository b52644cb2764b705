"""The statement of hole filling (include/geobi_hip.h geobi_fill_*) in plain Python: a dict of
undirected edges, a walk along `next`, and sums in the stated order.  Written from the header text, not from the
kernels; the device path (geobi_gnn_amd/meshfill.py, csrc/fill.hip) is compared with it exactly.

    boundary slot   slot s = 3f + k of an included face (three different corners) whose edge {corner k, corner k + 1} has
                    exactly one claimant; the hole walks it against the face: from(s) = corner k + 1, to(s) = corner k
    simple vertex   out[v] == in[v] == 1 (the boundary slots with from = v / to = v); any other boundary vertex is blocked
    successor       next(s) = the one boundary slot with from == to(s) if to(s) is simple, else none
    loop            s is on a loop iff following next from s returns to s, else it is a chain slot; the leader is the
                    lowest slot, rank = the steps from the leader, loops numbered in ascending leader
    selection       loop i iff max_hole_edges == 0 or len_i <= max_hole_edges; the j-th selected loop gets vertex V + j, its
                    slot s the face row F + off_j + rank(s) = (from(s), to(s), V + j)
    position        partial[l], l = 0 .. 63, starts at +0.0 and adds in fp64 the coordinate of from(s) for the ranks
                    r == l (mod 64) in ascending r; total starts at +0.0 and adds partial[0 .. 63] in ascending l;
                    (float)(total / (double)len)
"""
import numpy as np

F32, F64 = np.float32, np.float64
COUNT_KEYS = ('boundary_edges', 'blocked_vertices', 'chain_edges', 'loops', 'longest_loop', 'filled_loops', 'skipped_loops',
              'new_faces')


class Loops(object):
    """loop [3F] (-1: no boundary slot, -2: chain slot), rank [3F] (-1 off the loops), length [L], leader [L], loop_ptr
    [L + 1], loop_vertices (from(s) in rank order), int32; counts: the first five COUNT_KEYS; and for the fill: from / to of
    every boundary slot"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class Filled(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def boundary_loops(faces, V):
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    F = faces.shape[0]
    claimants = {}
    for f in range(F):
        a, b, c = (int(x) for x in faces[f])
        if a == b or b == c or c == a:
            continue
        for k in range(3):
            p, q = int(faces[f, k]), int(faces[f, (k + 1) % 3])
            claimants.setdefault((min(p, q), max(p, q)), []).append(3 * f + k)
    boundary = sorted(run[0] for run in claimants.values() if len(run) == 1)
    frm = {s: int(faces[s // 3, (s % 3 + 1) % 3]) for s in boundary}
    to = {s: int(faces[s // 3, s % 3]) for s in boundary}
    out_n, in_n, leaves = {}, {}, {}
    for s in boundary:
        out_n[frm[s]] = out_n.get(frm[s], 0) + 1
        in_n[to[s]] = in_n.get(to[s], 0) + 1
        leaves.setdefault(frm[s], []).append(s)
    touched = set(out_n) | set(in_n)
    simple = set(v for v in touched if out_n.get(v, 0) == 1 and in_n.get(v, 0) == 1)
    nxt = {s: (leaves[to[s]][0] if to[s] in simple else None) for s in boundary}
    loop = np.full(3 * F, -1, dtype=np.int32)
    rank = np.full(3 * F, -1, dtype=np.int32)
    length, leader, vertices = [], [], []
    for s in boundary:                               # ascending: the first slot of a loop met is its leader
        if loop[s] != -1:
            continue
        walk, t = [s], nxt[s]
        while t is not None and t != s and len(walk) <= len(boundary):
            walk.append(t)
            t = nxt[t]
        if t != s:                                   # the walk ended or never came back: s is a chain slot
            loop[s] = -2
            continue
        for r, w in enumerate(walk):
            loop[w], rank[w] = len(length), r
        vertices += [frm[w] for w in walk]
        leader.append(s)
        length.append(len(walk))
    counts = {'boundary_edges': len(boundary), 'blocked_vertices': len(touched) - len(simple),
              'chain_edges': int((loop == -2).sum()), 'loops': len(length), 'longest_loop': max(length) if length else 0}
    ptr = np.concatenate([[0], np.cumsum(np.asarray(length, dtype=np.int64))]).astype(np.int32)
    return Loops(loop=loop, rank=rank, length=np.asarray(length, dtype=np.int32), leader=np.asarray(leader, dtype=np.int32),
                 loop_ptr=ptr, loop_vertices=np.asarray(vertices, dtype=np.int32), counts=counts, frm=frm, to=to)


def centre(rim):
    """rim [len, 3] float32, the coordinates of from(s) in rank order -> [3] float32"""
    rim = np.asarray(rim, dtype=F32).reshape(-1, 3)
    out = np.zeros(3, dtype=F32)
    for k in range(3):
        partial = [0.0] * 64
        for r in range(rim.shape[0]):
            partial[r % 64] = partial[r % 64] + float(rim[r, k])
        total = 0.0
        for l in range(64):
            total = total + partial[l]
        out[k] = F32(total / float(rim.shape[0]))
    return out


def centres(points, loops, selected):
    points = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    rows = [centre(points[loops.loop_vertices[loops.loop_ptr[i]:loops.loop_ptr[i + 1]]]) for i in selected]
    return np.asarray(rows, dtype=F32).reshape(-1, 3)


def fill_holes(points, faces, max_hole_edges=0):
    points = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    V, F = points.shape[0], faces.shape[0]
    loops = boundary_loops(faces, V)
    selected = [i for i in range(len(loops.length)) if max_hole_edges == 0 or loops.length[i] <= max_hole_edges]
    off = np.concatenate([[0], np.cumsum([int(loops.length[i]) for i in selected])]).astype(np.int64)
    new_faces = np.zeros((int(off[-1]), 3), dtype=np.int32)
    new_face_loop = np.zeros(int(off[-1]), dtype=np.int32)
    where = {i: j for j, i in enumerate(selected)}
    for s in sorted(loops.frm):
        i = int(loops.loop[s])
        if i in where:
            row = int(off[where[i]]) + int(loops.rank[s])
            new_faces[row] = (loops.frm[s], loops.to[s], V + where[i])
            new_face_loop[row] = i
    counts = dict(loops.counts, filled_loops=len(selected), skipped_loops=len(loops.length) - len(selected),
                  new_faces=int(off[-1]))
    return Filled(points=np.concatenate([points, centres(points, loops, selected)]),
                  faces=np.concatenate([faces, new_faces]), new_vertex_loop=np.asarray(selected, dtype=np.int32),
                  new_face_loop=new_face_loop, loops=loops, counts=counts, V=V)


def apply(filled, other_points):
    pts = np.ascontiguousarray(other_points, dtype=F32).reshape(-1, 3)
    assert pts.shape[0] == filled.V
    return np.concatenate([pts, centres(pts, filled.loops, filled.new_vertex_loop.tolist())])


# ---------------------------------------------------------------------------------------------- comparison
def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


LOOP_FIELDS = ('loop', 'rank', 'length', 'leader', 'loop_ptr', 'loop_vertices')


def assert_same_loops(got, want, name=''):
    for field in LOOP_FIELDS:
        g, w = np.asarray(getattr(got, field)), np.asarray(getattr(want, field))
        assert g.dtype == np.int32, '%s %s: dtype %s' % (name, field, g.dtype)
        assert g.shape == w.shape and np.array_equal(g, w), '%s: loops.%s differ' % (name, field)
    want_counts = {k: want.counts[k] for k in COUNT_KEYS[:5]}
    assert {k: got.counts[k] for k in COUNT_KEYS[:5]} == want_counts, '%s: counts %s != %s' % (name, got.counts, want_counts)


def assert_same(got, want, name=''):
    """everything exact: the integer arrays equal, the points equal as uint32 bit patterns, the counts equal.  got, want:
    objects with points, faces, new_vertex_loop, new_face_loop (numpy), loops and counts"""
    for field in ('faces', 'new_vertex_loop', 'new_face_loop'):
        g, w = np.asarray(getattr(got, field)), np.asarray(getattr(want, field))
        assert g.dtype == np.int32, '%s %s: dtype %s' % (name, field, g.dtype)
        assert g.shape == w.shape and np.array_equal(g, w), '%s: %s differ' % (name, field)
    g, w = np.asarray(got.points), np.asarray(want.points)
    assert g.dtype == F32 and g.shape == w.shape, '%s: points %s %s' % (name, g.dtype, g.shape)
    assert np.array_equal(bits(g), bits(w)), '%s: points differ in %d rows' % (name, int((bits(g) != bits(w)).any(axis=1).sum()))
    assert dict(got.counts) == dict(want.counts), '%s: counts %s != %s' % (name, got.counts, want.counts)
    assert_same_loops(got.loops, want.loops, name)


# ---------------------------------------------------------------------------------------------- case builders
def full_mantissa(shape, seed):
    """float32 coordinates [n, 3] with all 24 bits in use: magnitudes in [1/8, 16), and per coordinate a few pairs +a, -a of
    magnitude 2^40 at random rows.  A pair cancels, but while a partial sum holds one half the small terms lose their low
    bits to it: WHICH terms meet it depends on the order of the sum, and the difference is far above a float32 ulp of the
    result (all-small fp64 sums of float32 terms would be exact in any order)"""
    rng = np.random.RandomState(seed)
    raw = rng.randint(0, 1 << 23, size=shape).astype(np.uint32) | np.uint32(0x3f800000)
    pts = (raw.view(F32) * np.where(rng.rand(*shape) < 0.5, -1.0, 1.0) * (2.0 ** rng.randint(-3, 4, size=shape))).astype(F32)
    n = shape[0]
    for k in range(shape[1]):
        rows = rng.permutation(n)[:2 * max(1, min(4, n // 8))]
        for i, j in zip(rows[0::2], rows[1::2]):
            big = F32(F32(1.0 + rng.randint(0, 1 << 23) * 2.0 ** -23) * 2.0 ** 40)
            pts[i, k], pts[j, k] = big, -big
    return pts


def shuffled(points, faces, seed):
    """the same mesh with its vertices renumbered, its faces reordered and every face rotated, from one seed"""
    rng = np.random.RandomState(seed)
    points, faces = np.asarray(points, dtype=F32), np.asarray(faces, dtype=np.int32)
    new_id = rng.permutation(points.shape[0])
    out_points = np.zeros_like(points)
    out_points[new_id] = points
    out = new_id[faces][rng.permutation(faces.shape[0])]
    for f in range(out.shape[0]):
        out[f] = np.roll(out[f], rng.randint(3))
    return out_points, np.ascontiguousarray(out, dtype=np.int32)


def cup(n, shuffle=None, mantissa=None):
    """a hub (vertex 0) and a rim of n vertices 1 .. n, the faces (0, i, i + 1): one hole of n edges.  shuffle: a seed for
    `shuffled`; mantissa: a seed for coordinates with full 24-bit mantissas"""
    ang = 2.0 * np.pi * np.arange(n) / n
    pts = np.concatenate([[[0.0, 0.0, 1.0]], np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], axis=1)]).astype(F32)
    if mantissa is not None:
        pts = full_mantissa(pts.shape, mantissa)
    faces = np.asarray([(0, 1 + i, 1 + (i + 1) % n) for i in range(n)], dtype=np.int32)
    return shuffled(pts, faces, shuffle) if shuffle is not None else (pts, faces)


def cylinder(m, seed=4):
    """an open tube: two rings of m vertices (0 .. m - 1 below, m .. 2m - 1 above), 2m faces, wound outwards"""
    rng = np.random.RandomState(seed)
    ang = 2.0 * np.pi * np.arange(m) / m
    ring = np.stack([np.cos(ang), np.sin(ang), np.zeros(m)], axis=1)
    pts = (np.concatenate([ring, ring + [0.0, 0.0, 1.0]]) + 0.01 * rng.rand(2 * m, 3)).astype(F32)
    faces = []
    for i in range(m):
        j = (i + 1) % m
        faces += [(i, j, m + j), (i, m + j, m + i)]
    return pts, np.asarray(faces, dtype=np.int32)


def tetrahedron():
    pts = np.array([[0, 0, 0], [1, 0, 0.25], [0, 1, 0.5], [0.25, 0.5, 1.5]], dtype=F32)
    return pts, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], dtype=np.int32)


def _some_points(n, seed=11):
    return np.random.RandomState(seed).rand(n, 3).astype(F32)


def hand_cases():
    """name -> (points, faces, the counts written out by hand)"""
    def counts(*values):
        return dict(zip(COUNT_KEYS, values))
    cases = {}
    cases['cup7'] = cup(7) + (counts(7, 0, 0, 1, 7, 1, 0, 7),)
    cases['cylinder6'] = cylinder(6) + (counts(12, 0, 0, 2, 6, 2, 0, 12),)
    # two fans meet in vertex 2: out = in = 2 there, every path of boundary slots ends at it
    cases['bow_tie'] = (_some_points(5), np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int32), counts(6, 1, 6, 0, 0, 0, 0, 0))
    # a cup of 6 with face 2 reversed: its rim edge is walked the other way, one end has out = 2, the other in = 2
    p, f = cup(6)
    f = f.copy()
    f[2] = f[2, [0, 2, 1]]
    cases['wound_against'] = (p, f, counts(6, 2, 6, 0, 0, 0, 0, 0))
    # three faces on the edge {0, 1}: it is no boundary, its ends have out = 2 / in = 2 from the six other edges
    cases['next_to_a_complex_edge'] = (_some_points(5), np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int32),
                                       counts(6, 2, 6, 0, 0, 0, 0, 0))
    cases['isolated_triangle'] = (_some_points(3), np.array([[0, 1, 2]], dtype=np.int32), counts(3, 0, 0, 1, 3, 1, 0, 3))
    cases['closed'] = tetrahedron() + (counts(0, 0, 0, 0, 0, 0, 0, 0),)
    # a face with a repeated corner on the rim claims nothing (and is copied through), vertex 9 is referenced by nothing
    p, f = cup(8)
    cases['not_included_and_unreferenced'] = (np.concatenate([p, _some_points(1)]),
                                              np.concatenate([f[:3], [[1, 2, 2]], f[3:]]).astype(np.int32),
                                              counts(8, 0, 0, 1, 8, 1, 0, 8))
    return cases


def icosphere(n):
    from geobi_gnn_amd import meshgen
    pts, faces = meshgen.icosphere(n)
    return pts.astype(F32), faces.astype(np.int32)


def sphere_without_fans(n, k, stride=1):
    """an icosphere of frequency n without the fans of k vertices whose rims share no vertex (chosen greedily among every
    `stride`-th vertex) -> (points, faces, the removed vertices, their valences)"""
    pts, faces = icosphere(n)
    ring = [set() for _ in range(pts.shape[0])]
    for a, b, c in faces.tolist():
        ring[a] |= {b, c}
        ring[b] |= {a, c}
        ring[c] |= {a, b}
    taken, removed = set(), []
    for v in range(0, pts.shape[0], stride):
        if len(removed) < k and not (ring[v] | {v}) & taken:
            removed.append(v)
            taken |= ring[v] | {v}
    assert len(removed) == k, 'only %d fans with disjoint rims' % len(removed)
    gone = np.isin(faces, removed).any(axis=1)
    return pts, np.ascontiguousarray(faces[~gone]), removed, [len(ring[v]) for v in removed]


def sphere_without_faces(n, k):
    """an icosphere without k single faces that share no vertex: k triangular holes"""
    pts, faces = icosphere(n)
    taken, gone = set(), []
    for f, corners in enumerate(faces.tolist()):
        if len(gone) < k and not set(corners) & taken:
            gone.append(f)
            taken |= set(corners)
    assert len(gone) == k, 'only %d faces without a common vertex' % len(gone)
    return pts, np.ascontiguousarray(np.delete(faces, gone, axis=0))


def hemisphere(n):
    """the faces of an icosphere whose three corners have z >= 0"""
    pts, faces = icosphere(n)
    return pts, np.ascontiguousarray(faces[(pts[faces][:, :, 2] >= 0).all(axis=1)])


def grid_with_holes(nx, ny, blocks):
    """a flat (nx x ny)-cell grid on whole-number coordinates, two triangles per cell, without the cells of the blocks
    (x0, y0, x1, y1): [x0, x1) x [y0, y1)"""
    xs, ys = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing='ij')
    pts = np.stack([xs.reshape(-1), ys.reshape(-1), np.zeros(xs.size)], axis=1).astype(F32)
    faces = []
    for i in range(nx):
        for j in range(ny):
            if any(x0 <= i < x1 and y0 <= j < y1 for x0, y0, x1, y1 in blocks):
                continue
            a, b, c, d = i * (ny + 1) + j, (i + 1) * (ny + 1) + j, (i + 1) * (ny + 1) + j + 1, i * (ny + 1) + j + 1
            faces += [(a, b, c), (a, c, d)]
    return pts, np.asarray(faces, dtype=np.int32)


def rims_in_one_mesh(lengths):
    """one cup per length, side by side in one table"""
    points, faces, base = [], [], 0
    for k, n in enumerate(lengths):
        p, f = cup(n)
        points.append(p + F32([3.0 * k, 0.0, 0.0]))
        faces.append(f + base)
        base += p.shape[0]
    return np.concatenate(points).astype(F32), np.concatenate(faces).astype(np.int32)
