"""Plain-Python statement of the projection rules of include/geobi_hip.h (geobi_closest_on_faces, geobi_move_to), written
from that text and not from the kernels: one query at a time, the float work in Python floats (IEEE fp64, no contraction)
from the float32 inputs, the float32 fma of the position emulated exactly.  Also the remeshing loop with its fifth step as
meshremesh.remesh(project=True) runs it, the map back to the input surface, the comparison helper with its planted faults
and the case builders of tests/test_gpu_project.py.

WHICH face is nearest is the one thing no model can restate: the device search (geobi_nearest_triangle) is fp32 with a
hardware reciprocal, and between two faces that meet at the closest edge its choice is its own.  ``closest(face=None)`` and
``remesh(nearest_face=None)`` therefore search themselves -- the fp64 arg-min of ``distances``, the lowest id among equals
-- while with the device's face ids handed in every other bit is comparable."""
import math
import struct

import numpy as np

import remesh_model as R
import subdiv_model as S

F32 = np.float32
bits = S.bits
CLOSEST_FAULTS = ('priority', 'b0')
PROJECT_KEYS = ('projected', 'project_refused', 'project_reverted', 'project_turned')


def dot(u, w):
    return (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2]


def fma32(x, y, z):
    """fmaf(x, y, z) of three float32 values -> float32, ONE rounding: the product of two float32 is exact in fp64; the
    fp64 sum is taken round-to-odd (its exact error from the two-sum), which the rounding to float32 cannot tell from the
    exact sum (53 >= 2 * 24 + 2)"""
    p, z = float(x) * float(y), float(z)
    s = p + z
    if math.isfinite(s):
        t = s - p
        err = (p - (s - t)) + (z - t)
        if err != 0.0 and struct.unpack('<q', struct.pack('<d', s))[0] & 1 == 0:
            s = math.nextafter(s, math.inf if err > 0.0 else -math.inf)
    with np.errstate(over='ignore'):
        return F32(s)


def weight(num, den):
    """num / den; 0 for a zero denominator or a NaN"""
    if den == 0.0:
        return 0.0
    t = num / den
    return t if t == t else 0.0


def region_weights(p, a, b, c, faults=()):
    """Ericson's region test on tuples of Python floats -> (v, w, region), before the final clamp"""
    ab, ac = [b[k] - a[k] for k in range(3)], [c[k] - a[k] for k in range(3)]
    ap, bp, cp = [p[k] - a[k] for k in range(3)], [p[k] - b[k] for k in range(3)], [p[k] - c[k] for k in range(3)]
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    rules = [('a', lambda: d1 <= 0.0 and d2 <= 0.0, lambda: (0.0, 0.0)),
             ('b', lambda: d3 >= 0.0 and d4 <= d3, lambda: (1.0, 0.0)),
             ('ab', lambda: vc <= 0.0 and d1 >= 0.0 and d3 <= 0.0, lambda: (weight(d1, d1 - d3), 0.0)),
             ('c', lambda: d6 >= 0.0 and d5 <= d6, lambda: (0.0, 1.0)),
             ('ac', lambda: vb <= 0.0 and d2 >= 0.0 and d6 <= 0.0, lambda: (0.0, weight(d2, d2 - d6))),
             ('bc', lambda: va <= 0.0 and d4 - d3 >= 0.0 and d5 - d6 >= 0.0, None)]
    if 'priority' in faults:                       # the planted fault: the edges are asked before the corners
        rules = [rules[k] for k in (2, 4, 5, 0, 1, 3)]
    for name, holds, value in rules:
        if holds():
            if name == 'bc':
                t = weight(d4 - d3, (d4 - d3) + (d5 - d6))
                return 1.0 - t, t, name
            return value() + (name,)
    den = (va + vb) + vc
    return weight(vb, den), weight(vc, den), 'inside'


class Closest(object):
    """face [Q] int32, bary [Q, 3] float32, points [Q, 3] float32, dist [Q] float32; regions: the rule that decided"""

    def __init__(self, face, bary, points, dist, regions):
        self.face, self.bary, self.points, self.dist, self.regions = face, bary, points, dist, regions


def bary_points(verts, faces, face, bary):
    """geobi_bary_points: out = fmaf(b2, c, fmaf(b1, b, b0 * a)) per coordinate in float32; zeros for a face outside [0, F)"""
    verts = np.ascontiguousarray(verts, dtype=F32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    bary = np.ascontiguousarray(bary, dtype=F32).reshape(-1, 3)
    V, out = verts.shape[0], np.zeros((len(face), 3), dtype=F32)
    for i, f in enumerate(np.asarray(face).tolist()):
        if not 0 <= f < faces.shape[0]:
            continue
        a, b, c = (verts[min(max(int(x), 0), V - 1)] for x in faces[f])
        for k in range(3):
            with np.errstate(over='ignore', invalid='ignore'):
                out[i, k] = fma32(bary[i, 2], c[k], fma32(bary[i, 1], b[k], F32(float(bary[i, 0]) * float(a[k]))))
    return out


def distances(p, verts, faces):
    """the fp64 distance from ONE query to every face [F], by the rules with numpy arrays over the faces (the same order of
    operations); used for the model's own search only"""
    a, b, c = (verts[faces[:, k]].astype(np.float64) for k in range(3))
    p = np.asarray(p, dtype=np.float64)

    def vdot(u, w):
        return (u[:, 0] * w[:, 0] + u[:, 1] * w[:, 1]) + u[:, 2] * w[:, 2]
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = vdot(ab, ap), vdot(ac, ap), vdot(ab, bp), vdot(ac, bp), vdot(ab, cp), vdot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4

    def w8(num, den):
        with np.errstate(all='ignore'):
            t = num / den
        return np.where((den == 0.0) | (t != t), 0.0, t)
    den = (va + vb) + vc
    v, w = w8(vb, den), w8(vc, den)
    for holds, rv, rw in reversed([((d1 <= 0) & (d2 <= 0), 0.0, 0.0), ((d3 >= 0) & (d4 <= d3), 1.0, 0.0),
                                   ((vc <= 0) & (d1 >= 0) & (d3 <= 0), w8(d1, d1 - d3), 0.0), ((d6 >= 0) & (d5 <= d6), 0.0, 1.0),
                                   ((vb <= 0) & (d2 >= 0) & (d6 <= 0), 0.0, w8(d2, d2 - d6)),
                                   ((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), None, w8(d4 - d3, (d4 - d3) + (d5 - d6)))]):
        v, w = np.where(holds, 1.0 - rw if rv is None else rv, v), np.where(holds, rw, w)
    v = np.minimum(np.maximum(v, 0.0), 1.0)
    w = np.minimum(np.maximum(w, 0.0), 1.0 - v)
    e = p - ((a + v[:, None] * ab) + w[:, None] * ac)
    return np.sqrt(vdot(e, e))


def nearest_faces(q, verts, faces):
    """the model's own search: per query the face of the least fp64 distance, the lowest id among equals"""
    verts = np.ascontiguousarray(verts, dtype=F32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    q = np.ascontiguousarray(q, dtype=F32).reshape(-1, 3)
    out = np.zeros(q.shape[0], dtype=np.int32)
    for i in range(q.shape[0]):
        if np.isfinite(q[i]).all():
            out[i] = int(np.argmin(distances(q[i], verts, faces)))
    return out


def closest(q, verts, faces, face=None, faults=()):
    """geobi_closest_on_faces -> Closest.  face: the face of every query (None: ``nearest_faces``)"""
    assert all(f in CLOSEST_FAULTS for f in faults)
    q = np.ascontiguousarray(q, dtype=F32).reshape(-1, 3)
    verts = np.ascontiguousarray(verts, dtype=F32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    face = nearest_faces(q, verts, faces) if face is None else np.asarray(face, dtype=np.int32).reshape(-1)
    Q, V, F = q.shape[0], verts.shape[0], faces.shape[0]
    assert face.shape[0] == Q and V >= 1 and F >= 1
    bary, dist, regions = np.zeros((Q, 3), dtype=F32), np.zeros(Q, dtype=F32), [None] * Q
    for i in range(Q):
        f = int(face[i])
        if not 0 <= f < F:
            continue
        v, w, d = 0.0, 0.0, math.inf
        if np.isfinite(q[i]).all():
            a, b, c = (tuple(float(x) for x in verts[min(max(int(k), 0), V - 1)]) for k in faces[f])
            p = tuple(float(x) for x in q[i])
            v, w, regions[i] = region_weights(p, a, b, c, faults)
            v = min(max(v, 0.0), 1.0)
            w = min(max(w, 0.0), 1.0 - v)
            e = [p[k] - ((a[k] + v * (b[k] - a[k])) + w * (c[k] - a[k])) for k in range(3)]
            d = math.sqrt(dot(e, e))
        b0 = 1.0 - (v + w) if 'b0' in faults else (1.0 - v) - w
        with np.errstate(over='ignore'):
            bary[i], dist[i] = (F32(b0), F32(v), F32(w)), F32(d)
    return Closest(face.copy(), bary, bary_points(verts, faces, face, bary), dist, regions)


def apply(closest_or_remeshed, faces, other):
    """the counterpart of every projected point on a paired vertex array: bary_points(other, faces, face, bary)"""
    c = closest_or_remeshed
    face, bary = (c.face, c.bary) if isinstance(c, Closest) else (c.source_face, c.source_bary)
    return bary_points(other, faces, face, bary)


# ---------------------------------------------------------------------------------------------- move_to
def move_to(points, faces, target, lock, guard=True):
    """geobi_move_to -> (points' [V, 3] float32, counts (RELAX_KEYS)).  guard=False is the planted fault: no flip test and
    no revert"""
    points = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    target = np.ascontiguousarray(target, dtype=F32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    if faces.shape[0] == 0:
        return points.copy(), dict.fromkeys(R.RELAX_KEYS, 0)
    m = R.Mesh(points, faces)
    V = m.V
    out = m.points.copy()
    moved, refused = [False] * V, 0
    for v in range(V):
        if int(lock[v]) != 0 or len(m.nbrs[v]) < 3:
            continue
        to = target[v]
        if not all(np.isfinite(x) for x in to):
            refused += 1
        elif any(to[k] != m.points[v, k] for k in range(3)):
            if not guard or R.no_flip(m, v, (), tuple(float(x) for x in to)):
                moved[v] = True
                out[v] = to
            else:
                refused += 1

    def turned_faces(new):
        Pn = [tuple(float(x) for x in row) for row in new]
        found = []
        for f in range(m.F):
            if not m.t.included[f]:
                continue
            was = m.face_normal(f)
            if was[3] != 0.0 and not R.dot(was, m.face_normal(f, Pn)) > 0.0:
                found.append(f)
        return found
    back = set(c for f in turned_faces(out) for c in m.fv[f] if moved[c]) if guard else set()
    for v in back:
        out[v] = m.points[v]
    return out, dict(zip(R.RELAX_KEYS, (sum(moved), refused, len(back), len(turned_faces(out)))))


# ---------------------------------------------------------------------------------------------- the whole call
REMESH_FAULTS = ('relock',)


def iteration(points, faces, low, high, feature_angle=40.0, relax_lambda=0.5, max_rounds=64, sweeps=R.SWEEPS):
    """ONE iteration of remesh_model.remesh, split .. relax, restated because the fifth step needs what that call does not
    hand out: -> (points, faces, counts (ITERATION_KEYS), lock), lock the flags the relaxation ran under -- computed from the
    positions BEFORE it; the sharp bit depends on positions, so flags taken afterwards may differ -- or None without faces"""
    c = dict.fromkeys(R.ITERATION_KEYS, 0)
    try:
        refined = S.subdivide(points, faces, max_edge=high, max_rounds=max_rounds)
    except S.TooManyRounds as e:
        raise R.TooManyRounds(str(e))
    points, faces = refined.points, refined.faces
    c['splits'], c['split_passes'] = refined.counts['split'], refined.counts['passes']
    while faces.shape[0] > 0:
        lock = R.lock_flags(points, faces, feature_angle)[0]
        r = R.collapse_round(points, faces, low, high, lock, sweeps)
        if r.counts['collapses'] == 0 and r.counts['not_included'] == 0:
            break
        if c['collapse_rounds'] == max_rounds:
            raise R.TooManyRounds('%d collapse rounds' % max_rounds)
        points, faces = r.points, r.faces
        c['collapse_rounds'] += 1
        c['collapses'] += r.counts['collapses']
        if r.counts['collapses'] == 0:
            break
    while faces.shape[0] > 0:
        lock = R.lock_flags(points, faces, feature_angle)[0]
        r = R.flip_round(points, faces, lock, feature_angle, sweeps)
        if r.counts['flips'] == 0:
            break
        if c['flip_rounds'] == max_rounds:
            raise R.TooManyRounds('%d flip rounds' % max_rounds)
        faces = r.faces
        c['flip_rounds'] += 1
        c['flips'] += r.counts['flips']
    lock = None
    if faces.shape[0] > 0:
        lock = R.lock_flags(points, faces, feature_angle)[0]
        points, rc = R.relax(points, faces, lock, relax_lambda)
        c.update(rc)
    return points, faces, c, lock


def remesh(points, faces, L, iterations=5, feature_angle=40.0, relax_lambda=0.5, max_rounds=64, sweeps=R.SWEEPS, project=False,
           nearest_face=None, faults=()):
    """remesh_model.remesh with, for project=True, the fifth step after every relaxation -- under the relaxation's own lock
    flags -- and the source map at the end, as meshremesh.remesh(project=True) runs them.  nearest_face(q, verts, faces) ->
    face ids [Q]: whose search to use (None: ``nearest_faces``); everything else is computed here.  The planted fault
    'relock' takes the flags of the fifth step from the relaxed positions.  Remeshed.locks: the flags of every iteration"""
    assert all(f in REMESH_FAULTS for f in faults)
    points = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    if not project:
        out = R.remesh(points, faces, L, iterations, feature_angle, relax_lambda, max_rounds, sweeps)
        out.source_face = out.source_bary = None
        return out
    assert faces.shape[0] > 0
    in_points, in_faces = points, faces
    search = nearest_face or nearest_faces

    def on_input(q):
        return closest(q, in_points, in_faces, face=search(q, in_points, in_faces))
    low, high = R.band(L)
    out = R.Remeshed()
    out.low, out.high = low, high
    out.before = R.mesh_stats(points, faces, low, high)
    out.per_iteration, out.locks = [], []
    for _ in range(iterations):
        points, faces, c, lock = iteration(points, faces, low, high, feature_angle, relax_lambda, max_rounds, sweeps)
        c.update(dict.fromkeys(PROJECT_KEYS, 0))
        if faces.shape[0] > 0:
            after = R.lock_flags(points, faces, feature_angle)[0]
            out.locks.append((lock, after))
            points, pc = move_to(points, faces, on_input(points).points, after if 'relock' in faults else lock)
            c.update(zip(PROJECT_KEYS, (pc[k] for k in R.RELAX_KEYS)))
        out.per_iteration.append(c)
    out.points, out.faces = points, faces
    out.after = R.mesh_stats(points, faces, low, high)
    source = on_input(points)
    out.source_face, out.source_bary = source.face, source.bary
    return out


# ---------------------------------------------------------------------------------------------- comparison
def assert_same_closest(got, want, name=''):
    """face equal, bary / points / dist float32 and equal as uint32 patterns"""
    assert np.asarray(got.face).dtype == np.int32 and np.array_equal(got.face, want.face), '%s: faces differ' % name
    for field in ('bary', 'points', 'dist'):
        g, w = np.asarray(getattr(got, field)), np.asarray(getattr(want, field))
        assert g.dtype == F32 and g.shape == w.shape, '%s: %s %s %s' % (name, field, g.dtype, g.shape)
        rows = (bits(g) != bits(w)).reshape(g.shape[0], -1).any(axis=1)
        assert not rows.any(), '%s: %s differs in %d rows, first %d: %s != %s' % (
            name, field, int(rows.sum()), int(np.nonzero(rows)[0][0]), g[rows][0], w[rows][0])


def assert_same_move(got, want, name=''):
    """(points, counts) of a move_to"""
    assert dict(got[1]) == dict(want[1]), '%s: counts %s != %s' % (name, got[1], want[1])
    g, w = np.asarray(got[0]), np.asarray(want[0])
    assert g.dtype == F32 and g.shape == w.shape and np.array_equal(bits(g), bits(w)), '%s: points differ in %d rows' % (
        name, int((bits(g) != bits(w)).any(axis=1).sum()))


def assert_same(got, want, name=''):
    """a whole remesh(project=True): remesh_model.assert_same, and the source map exact"""
    R.assert_same(got, want, name)
    assert np.asarray(got.source_face).dtype == np.int32 and np.array_equal(got.source_face, want.source_face), name
    g, w = np.asarray(got.source_bary), np.asarray(want.source_bary)
    assert g.dtype == F32 and g.shape == w.shape and np.array_equal(bits(g), bits(w)), '%s: source_bary differs' % name


# ---------------------------------------------------------------------------------------------- facts and cases
def surface_bound(verts):
    """8 * 2^-24 * M, M the largest absolute coordinate of the mesh: how far a projected float32 point may lie from its
    plane triangle.  Per coordinate the position goes through three roundings of the chain fmaf(b2, c, fmaf(b1, b, b0 * a))
    and carries the three roundings of the weights, each at most 2^-24 * M; over the three coordinates that is times
    sqrt(3).  The roundings do not all reach their worst case at once: 8 is the stated constant, and it is not widened"""
    return 8.0 * 2.0 ** -24 * float(np.abs(np.asarray(verts, dtype=np.float64)).max())


def distance_to_faces(points, verts, faces, face):
    """the fp64 distance from points[i] to the triangle face[i], by ``distances``"""
    verts = np.ascontiguousarray(verts, dtype=F32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return np.array([distances(points[i], verts, faces[int(face[i]):int(face[i]) + 1])[0] for i in range(len(face))])


def distance_to_surface(points, verts, faces):
    verts = np.ascontiguousarray(verts, dtype=F32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return np.array([distances(p, verts, faces).min() for p in np.asarray(points)])


HAND_TRIANGLE = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], dtype=F32)


def hand_queries():
    """[(query x, y, region, v, w)] on the triangle (0,0) (4,0) (0,4) of the plane z = 0: one query in each of the seven
    regions, its (v, w) known by hand; every query is used at z = 0, +2 and -3"""
    return [(-1.0, -2.0, 'a', 0.0, 0.0), (6.0, -1.0, 'b', 1.0, 0.0), (1.0, -3.0, 'ab', 0.25, 0.0), (-1.0, 7.0, 'c', 0.0, 1.0),
            (-2.0, 3.0, 'ac', 0.0, 0.75), (4.0, 2.0, 'bc', 0.75, 0.25), (1.0, 2.0, 'inside', 0.25, 0.5)]


def degenerate_triangles():
    """{name: verts [3, 3]}: two equal corners (each pair), three equal corners, collinear corners"""
    return {'a_is_b': np.array([[1, 2, 3], [1, 2, 3], [4, 2, 3]], dtype=F32),
            'b_is_c': np.array([[1, 2, 3], [4, 2, 3], [4, 2, 3]], dtype=F32),
            'a_is_c': np.array([[1, 2, 3], [4, 2, 3], [1, 2, 3]], dtype=F32),
            'one_point': np.array([[1, 2, 3], [1, 2, 3], [1, 2, 3]], dtype=F32),
            'collinear': np.array([[0, 0, 0], [1, 1, 1], [3, 3, 3]], dtype=F32),
            'collinear_folded': np.array([[0, 0, 0], [3, 3, 3], [1, 1, 1]], dtype=F32)}


def degenerate_queries():
    return np.array([[0, 0, 0], [1, 2, 3], [2.5, 2, 3], [5, 5, 5], [2, 2, 2], [-1, 3, 0.5], [2, -7, 9]], dtype=F32)


def shell_queries(n, seed=0):
    """n points at 0.7 .. 1.3 radii around the origin"""
    rng = np.random.RandomState(seed)
    d = rng.randn(n, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * rng.uniform(0.7, 1.3, size=(n, 1))).astype(F32)


def bumpy_sphere(sigma=0.05, seed=1):
    """(points, faces): the 320-face icosphere with Gaussian noise of `sigma`: at feature_angle 40 some edges are sharp, and
    a relaxation changes which -- the flags before and after it differ"""
    import decim_model as D
    clean, faces = D.icosphere(4)
    return (clean + sigma * np.random.RandomState(seed).randn(*clean.shape)).astype(F32), faces


def noisy_sphere(seed):
    """(points, faces, target, lock): the 162 vertices of the 320-face icosphere displaced by Gaussian noise of sigma 0.1,
    their closest points on the clean sphere (the model's own search), no vertex locked"""
    import decim_model as D
    clean, faces = D.icosphere(4)
    assert faces.shape[0] == 320
    points = (clean + 0.1 * np.random.RandomState(seed).randn(*clean.shape)).astype(F32)
    return points, faces, closest(points, clean, faces).points, np.zeros(points.shape[0], dtype=np.int32)


NOISY_SPHERE_SEED = 0


def lifted_grid(n=8, seed=4):
    """(points, faces, flat, lock): remesh_model.jittered_grid with its interior vertices also lifted off the plane by
    multiples of 1 / 64 up to 1 / 16, the flat grid z = 0 it came from, and the lock flags of its rim"""
    points, faces = R.jittered_grid(n, seed)
    flat = S.grid(n, n)[0]
    lock = R.lock_flags(flat, faces, 180.0)[0]
    lift = np.random.RandomState(seed + 1).randint(-4, 5, size=points.shape[0]) / 64.0
    points[lock == 0, 2] += lift[lock == 0].astype(F32)
    return points, faces, flat, lock
