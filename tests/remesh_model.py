"""Sequential statement of the remeshing rules of include/geobi_hip.h (geobi_remesh_lock, geobi_decim_plan_short,
geobi_flip_*, geobi_relax), written from that text and not from the kernels: every step a Python loop over faces, edges or
vertices on subdiv_model.Table, the float work in Python floats (IEEE fp64, no contraction) from the float32 inputs.  Also
the whole call as meshremesh.remesh runs it, the comparison helper and the case builders of tests/test_gpu_remesh.py."""
import math

import numpy as np

import decim_model as D
import subdiv_model as S

F32 = np.float32
SWEEPS = 3                                     # GEOBI_FLIP_SWEEPS = GEOBI_DECIM_SWEEPS
NONE = 0x7fffffff
LOCK_KEYS = ('edges', 'boundary_vertices', 'sharp_edges', 'sharp_vertices')
FLIP_KEYS = ('edges', 'candidates', 'valid', 'flips', 'sweeps_selected')
RELAX_KEYS = ('moved', 'refused', 'reverted', 'turned')
FLIP_FAULTS = ('no_diagonal', 'no_fold', 'no_blocking', 'two_vertex', 'id_order')
COLLAPSE_FAULTS = ('no_high', 'no_blocking', 'id_order')
ITERATION_KEYS = ('splits', 'split_passes', 'collapses', 'collapse_rounds', 'flips', 'flip_rounds', 'moved', 'refused',
                  'reverted', 'turned')


def dot(u, w):
    return (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2]


def cos2(feature_angle):
    """-> (use_sharp, c2): the fp64 cos^2 of the feature angle in degrees, as the host forms it; 180 switches sharp off"""
    if float(feature_angle) == 180.0:
        return 0, 0.0
    c = math.cos(math.radians(float(feature_angle)))
    return 1, c * c


def band(L):
    """low = float32(0.8 * L), high = float32(4.0 * L / 3.0), the products and the quotient in fp64"""
    L = float(L)
    return F32(0.8 * L), F32(4.0 * L / 3.0)


class Mesh(object):
    """the tables of one round's input: t (subdiv_model.Table), P (points as tuples of Python floats), fv, nbrs (ascending),
    faces_at (the included faces at a vertex, ascending)"""

    def __init__(self, points, faces):
        self.points = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
        self.t = t = S.Table(faces)
        self.V, self.F, self.E = self.points.shape[0], t.faces.shape[0], t.E
        self.P = [tuple(float(x) for x in row) for row in self.points]
        self.fv = [tuple(int(x) for x in row) for row in t.faces]
        nbrs = [[] for _ in range(self.V)]
        for e in range(self.E):
            nbrs[int(t.lo[e])].append(int(t.hi[e]))
            nbrs[int(t.hi[e])].append(int(t.lo[e]))
        self.nbrs = [sorted(x) for x in nbrs]
        self.edge_set = set((int(t.lo[e]), int(t.hi[e])) for e in range(self.E))
        self.faces_at = [[] for _ in range(self.V)]
        for f in range(self.F):
            if t.included[f]:
                for c in self.fv[f]:
                    self.faces_at[c].append(f)

    def face_normal(self, f, P=None):
        P = P or self.P
        return D.normal(P[self.fv[f][0]], P[self.fv[f][1]], P[self.fv[f][2]])

    def sharp(self, e, use_sharp, c2):
        if not use_sharp or self.t.n[e] != 2:
            return False
        s0, s1 = self.t.claimants[e]
        n0, n1 = self.face_normal(s0 // 3), self.face_normal(s1 // 3)
        if n0[3] == 0.0 or n1[3] == 0.0:
            return False
        d = dot(n0, n1)
        return (not d > 0.0) or d * d < c2 * (n0[3] * n1[3])

    def direction(self, slot):
        """0 when the face of the slot walks lo -> hi"""
        f, k = slot // 3, slot % 3
        return 0 if self.fv[f][k] < self.fv[f][(k + 1) % 3] else 1

    def third(self, slot):
        f, k = slot // 3, slot % 3
        return self.fv[f][(k + 2) % 3]


# ---------------------------------------------------------------------------------------------- lock flags
def lock_flags(points, faces, feature_angle=40.0, mesh=None):
    m = mesh or Mesh(points, faces)
    use_sharp, c2 = cos2(feature_angle)
    lock = np.zeros(m.V, dtype=np.int32)
    sharp_edges = 0
    for e in range(m.E):
        lo, hi = int(m.t.lo[e]), int(m.t.hi[e])
        if m.t.n[e] != 2:
            lock[lo] |= 1
            lock[hi] |= 1
        elif m.sharp(e, use_sharp, c2):
            sharp_edges += 1
            lock[lo] |= 2
            lock[hi] |= 2
    return lock, dict(zip(LOCK_KEYS, (m.E, int((lock & 1 != 0).sum()), sharp_edges, int((lock & 2 != 0).sum()))))


# ---------------------------------------------------------------------------------------------- selection
def select(quads, rank, nbrs, V, sweeps=SWEEPS, blocking=True):
    """quads {candidate: its vertices}, rank {candidate: rank} -> (selected in sweep order, sweeps that selected)"""
    live, blocked, selected, sweeps_selected = set(rank), [False] * V, [], 0
    for _ in range(sweeps):
        m1 = [NONE] * V
        for e in live:
            for v in quads[e]:
                m1[v] = min(m1[v], rank[e])
        m2 = [min([m1[v]] + [m1[w] for w in nbrs[v]]) for v in range(V)]
        now = [e for e in sorted(live) if min(m2[v] for v in quads[e]) == rank[e]]
        sweeps_selected += 1 if now else 0
        selected += now
        if blocking:
            for e in now:
                for v in quads[e]:
                    blocked[v] = True
                    for w in nbrs[v]:
                        blocked[w] = True
        live = set(e for e in live if e not in now and not any(blocked[v] for v in quads[e]))
    return selected, sweeps_selected


# ---------------------------------------------------------------------------------------------- short-edge collapse
def no_flip(m, v, skip, at):
    for f in m.faces_at[v]:
        if f in skip:
            continue
        n = m.face_normal(f)
        if n[3] == 0.0:
            continue
        moved = D.normal(*[at if c == v else m.P[c] for c in m.fv[f]])
        if not dot(n, moved) > 0.0:
            return False
    return True


def collapse_round(points, faces, low, high, lock=None, sweeps=SWEEPS, faults=()):
    """one round of geobi_decim_plan_short + geobi_decim_emit -> decim_model.Round, with `refused` {(lo, hi): reason} for
    every edge below `low` that is no valid candidate"""
    assert all(f in COLLAPSE_FAULTS for f in faults)
    m = Mesh(points, faces)
    t, P, V, F, E = m.t, m.P, m.V, m.F, m.E
    low2, high2 = float(F32(low)) * float(F32(low)), float(F32(high)) * float(F32(high))
    locked = [False] * V
    for e in range(E):
        if t.n[e] != 2:
            locked[int(t.lo[e])] = locked[int(t.hi[e])] = True
    if lock is not None:
        locked = [a or int(b) != 0 for a, b in zip(locked, lock)]
    valid, refused = {}, {}
    for e in range(E):
        lo, hi = int(t.lo[e]), int(t.hi[e])
        dx, dy, dz = P[hi][0] - P[lo][0], P[hi][1] - P[lo][1], P[hi][2] - P[lo][2]
        len2 = (dx * dx + dy * dy) + dz * dz
        if not len2 < low2:
            continue
        if t.n[e] != 2 or (locked[lo] and locked[hi]):
            refused[(lo, hi)] = 'locked'
            continue
        code = 0 if locked[lo] else 1 if locked[hi] else 2
        at = (P[lo], P[hi], tuple(float(D.midpoint32(m.points[lo, k], m.points[hi, k])) for k in range(3)))[code]
        far = False
        for v in (lo, hi):
            for w in m.nbrs[v]:
                if w in (lo, hi):
                    continue
                ex, ey, ez = P[w][0] - at[0], P[w][1] - at[1], P[w][2] - at[2]
                far = far or (ex * ex + ey * ey) + ez * ez > high2
        if far and 'no_high' not in faults:
            refused[(lo, hi)] = 'high'
            continue
        shared = sorted(set(m.nbrs[lo]) & set(m.nbrs[hi]))
        if len(shared) != 2:
            refused[(lo, hi)] = 'link'
            continue
        if any(len(m.nbrs[w]) < 4 for w in shared):
            refused[(lo, hi)] = 'valence'
            continue
        claimants = [s // 3 for s in t.claimants[e]]
        if not (no_flip(m, lo, claimants, at) and no_flip(m, hi, claimants, at)):
            refused[(lo, hi)] = 'flip'
            continue
        valid[e] = (D.orderable(len2), e if 'id_order' in faults else D.edge_hash(lo, hi), code)
    order = sorted(valid, key=lambda e: (valid[e][0], valid[e][1], e))
    rank = {e: r for r, e in enumerate(order)}
    quads = {e: (int(t.lo[e]), int(t.hi[e])) for e in order}
    selected, sweeps_selected = select(quads, rank, m.nbrs, V, sweeps, 'no_blocking' not in faults)
    selected.sort(key=lambda e: rank[e])
    for e in order:
        if e not in selected:
            refused[quads[e]] = 'not selected'
    # emit: rule 9 of geobi_decim_*
    role, partner = [-1] * V, list(range(V))
    gone = np.zeros(F, dtype=bool) | ~t.included
    for e in selected:
        lo, hi = quads[e]
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
        out_points.append(m.points[v] if role[v] <= 0 else m.points[partner[v]] if role[v] == 1 else
                          D.midpoint32(m.points[v], m.points[partner[v]]))
    face_map = np.nonzero(~gone)[0].astype(np.int32)
    r = D.Round()
    r.points = np.asarray(out_points, dtype=F32).reshape(-1, 3)
    r.faces = vertex_map[t.faces[face_map]].astype(np.int32).reshape(-1, 3)
    r.face_map, r.vertex_map = face_map, vertex_map
    r.vertex_parents = np.asarray(parents, dtype=np.int32).reshape(-1, 2)
    r.place = np.asarray(place, dtype=np.int8)
    r.counts = dict(zip(D.COUNT_KEYS, (E, sum(locked), len(order), len(selected), rows, int(face_map.shape[0]),
                                       F - int(t.included.sum()), sweeps_selected)))
    r.collapsed = [quads[e] for e in selected]
    r.candidates = {quads[e]: rank[e] for e in order}
    r.refused, r.nbrs = refused, m.nbrs
    return r


# ---------------------------------------------------------------------------------------------- flips
def deviation(valence, lock_bits):
    return abs(valence - (4 if lock_bits & 1 else 6))


def total_deviation(faces, lock):
    m = Mesh(np.zeros((len(lock), 3), dtype=F32), faces)
    return sum(deviation(len(m.nbrs[v]), int(lock[v])) for v in range(m.V) if m.nbrs[v])


class FlipRound(object):
    """faces [F, 3] int32, counts (FLIP_KEYS), flipped [(a, b, c, d)] in rank order, quads {(a, b): (a, b, c, d)} and
    candidates {(a, b): rank} of the valid candidates, gains {(a, b): gain}, nbrs of the round's input"""


def flip_round(points, faces, lock, feature_angle=40.0, sweeps=SWEEPS, faults=()):
    assert all(f in FLIP_FAULTS for f in faults)
    m = Mesh(points, faces)
    t, P, V, E = m.t, m.P, m.V, m.E
    use_sharp, c2 = cos2(feature_angle)
    lock = [int(x) for x in lock]
    val = [len(x) for x in m.nbrs]
    n_candidates, valid, quad_of, gains = 0, {}, {}, {}
    for e in range(E):
        if t.n[e] != 2:
            continue
        s0, s1 = t.claimants[e]
        if m.direction(s0) == m.direction(s1) or m.sharp(e, use_sharp, c2):
            continue
        forth, back = (s0, s1) if m.direction(s0) == 0 else (s1, s0)
        a, b, c, d = int(t.lo[e]), int(t.hi[e]), m.third(forth), m.third(back)
        if c == d:
            continue
        before = sum(deviation(val[v], lock[v]) for v in (a, b, c, d))
        after = sum(deviation(val[v] - 1, lock[v]) for v in (a, b)) + sum(deviation(val[v] + 1, lock[v]) for v in (c, d))
        gain = before - after
        if gain <= 0:
            continue
        n_candidates += 1
        if val[a] < 4 or val[b] < 4:
            continue
        if 'no_diagonal' not in faults and (min(c, d), max(c, d)) in m.edge_set:
            continue
        n0, n1 = D.normal(P[a], P[b], P[c]), D.normal(P[b], P[a], P[d])
        m0, m1 = D.normal(P[a], P[d], P[c]), D.normal(P[b], P[c], P[d])
        fold = not (dot(n0, m0) > 0.0 and dot(n0, m1) > 0.0 and dot(n1, m0) > 0.0 and dot(n1, m1) > 0.0 and
                    dot(m0, m1) > 0.0)
        if fold and 'no_fold' not in faults:
            continue
        valid[e] = (16 - gain, e if 'id_order' in faults else D.edge_hash(a, b))
        quad_of[e], gains[(a, b)] = (a, b, c, d), gain
    order = sorted(valid, key=lambda e: (valid[e][0], valid[e][1], e))
    rank = {e: r for r, e in enumerate(order)}
    quads = {e: quad_of[e][:2] if 'two_vertex' in faults else quad_of[e] for e in order}
    selected, sweeps_selected = select(quads, rank, m.nbrs, V, sweeps, 'no_blocking' not in faults)
    selected.sort(key=lambda e: rank[e])
    out = t.faces.astype(np.int32).copy()
    for e in selected:
        a, b, c, d = quad_of[e]
        s0, s1 = t.claimants[e]
        forth, back = (s0, s1) if m.direction(s0) == 0 else (s1, s0)
        out[forth // 3] = (a, d, c)
        out[back // 3] = (b, c, d)
    r = FlipRound()
    r.faces = out
    r.counts = dict(zip(FLIP_KEYS, (E, n_candidates, len(order), len(selected), sweeps_selected)))
    r.flipped = [quad_of[e] for e in selected]
    r.quads = {quad_of[e][:2]: quad_of[e] for e in order}
    r.candidates = {quad_of[e][:2]: rank[e] for e in order}
    r.gains, r.nbrs = gains, m.nbrs
    return r


# ---------------------------------------------------------------------------------------------- relaxation
def relax(points, faces, lock, lam=0.5):
    """-> (points' [V, 3] float32, counts (RELAX_KEYS))"""
    m = Mesh(points, faces)
    P, V = m.P, m.V
    lam = float(lam)
    out = m.points.copy()
    moved, refused = [False] * V, 0
    with np.errstate(over='ignore'):
        for v in range(V):
            if int(lock[v]) != 0 or len(m.nbrs[v]) < 3:
                continue
            g = [0.0, 0.0, 0.0]
            for w in m.nbrs[v]:
                g = [g[k] + P[w][k] for k in range(3)]
            n = [0.0, 0.0, 0.0]
            for f in m.faces_at[v]:
                nf = m.face_normal(f)
                n = [n[k] + nf[k] for k in range(3)]
            s = dot(n, n)
            if s == 0.0:
                continue
            count = float(len(m.nbrs[v]))
            d = [g[k] / count - P[v][k] for k in range(3)]
            q = dot(n, d) / s
            to = [F32(P[v][k] + lam * (d[k] - n[k] * q)) for k in range(3)]
            if not all(np.isfinite(x) for x in to):
                refused += 1
            elif any(to[k] != m.points[v, k] for k in range(3)):
                if no_flip(m, v, (), tuple(float(x) for x in to)):
                    moved[v] = True
                    out[v] = to
                else:
                    refused += 1

    def turned_faces(new):
        Pn = [tuple(float(x) for x in row) for row in new]
        faces_turned = []
        for f in range(m.F):
            if not m.t.included[f]:
                continue
            was = m.face_normal(f)
            if was[3] != 0.0 and not dot(was, m.face_normal(f, Pn)) > 0.0:
                faces_turned.append(f)
        return faces_turned
    back = set(c for f in turned_faces(out) for c in m.fv[f] if moved[c])
    for v in back:
        out[v] = m.points[v]
    return out, dict(zip(RELAX_KEYS, (sum(moved), refused, len(back), len(turned_faces(out)))))


# ---------------------------------------------------------------------------------------------- statistics
def mesh_stats(points, faces, low, high):
    """edge-length min / mean / max (fp64 sqrt of len2), the share of edges inside [low, high] (as float32), the valence
    histogram 3 .. 12+ (index 0: valence 3; below 3 is not counted), the mean |valence - target| over the vertices with an
    edge (target 4 at an edge with n_e != 2, else 6)"""
    m = Mesh(points, faces)
    lens = np.array([math.sqrt(float(S.len2(m.points, int(m.t.lo[e]), int(m.t.hi[e])))) for e in range(m.E)], dtype=np.float64)
    val = np.array([len(x) for x in m.nbrs], dtype=np.int64)
    target = np.full(m.V, 6, dtype=np.int64)
    for e in range(m.E):
        if m.t.n[e] != 2:
            target[int(m.t.lo[e])] = target[int(m.t.hi[e])] = 4
    used = val > 0
    hist = [int((val == k).sum()) for k in range(3, 12)] + [int((val >= 12).sum())]
    inside = int(((lens >= float(F32(low))) & (lens <= float(F32(high)))).sum())
    return {'edges': m.E, 'edge_min': float(lens.min()) if m.E else 0.0, 'edge_mean': float(lens.mean()) if m.E else 0.0,
            'edge_max': float(lens.max()) if m.E else 0.0, 'inside': inside, 'share': inside / m.E if m.E else 0.0,
            'valence_hist': hist, 'valence_dev': float(np.abs(val - target)[used].mean()) if used.any() else 0.0}


# ---------------------------------------------------------------------------------------------- the whole call
class TooManyRounds(RuntimeError):
    pass


class Remeshed(object):
    pass


def remesh(points, faces, L, iterations=5, feature_angle=40.0, relax_lambda=0.5, max_rounds=64, sweeps=SWEEPS):
    """the whole call, as meshremesh.remesh runs it with target_edge = L"""
    points = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    low, high = band(L)
    out = Remeshed()
    out.low, out.high = low, high
    out.before = mesh_stats(points, faces, low, high)
    out.per_iteration = []
    for _ in range(iterations):
        c = dict.fromkeys(ITERATION_KEYS, 0)
        try:
            refined = S.subdivide(points, faces, max_edge=high, max_rounds=max_rounds)
        except S.TooManyRounds as e:
            raise TooManyRounds(str(e))
        points, faces = refined.points, refined.faces
        c['splits'], c['split_passes'] = refined.counts['split'], refined.counts['passes']
        while faces.shape[0] > 0:
            lock = lock_flags(points, faces, feature_angle)[0]
            r = collapse_round(points, faces, low, high, lock, sweeps)
            if r.counts['collapses'] == 0 and r.counts['not_included'] == 0:
                break
            if c['collapse_rounds'] == max_rounds:
                raise TooManyRounds('%d collapse rounds' % max_rounds)
            points, faces = r.points, r.faces
            c['collapse_rounds'] += 1
            c['collapses'] += r.counts['collapses']
            if r.counts['collapses'] == 0:
                break
        while faces.shape[0] > 0:
            lock = lock_flags(points, faces, feature_angle)[0]
            r = flip_round(points, faces, lock, feature_angle, sweeps)
            if r.counts['flips'] == 0:
                break
            if c['flip_rounds'] == max_rounds:
                raise TooManyRounds('%d flip rounds' % max_rounds)
            faces = r.faces
            c['flip_rounds'] += 1
            c['flips'] += r.counts['flips']
        if faces.shape[0] > 0:
            lock = lock_flags(points, faces, feature_angle)[0]
            points, rc = relax(points, faces, lock, relax_lambda)
            c.update(rc)
        out.per_iteration.append(c)
    out.points, out.faces = points, faces
    out.after = mesh_stats(points, faces, low, high)
    return out


# ---------------------------------------------------------------------------------------------- comparison
bits = S.bits


def assert_same_mesh(got_points, got_faces, want_points, want_faces, name=''):
    """faces int32 and equal, points float32 and equal as uint32 patterns"""
    g, w = np.asarray(got_faces), np.asarray(want_faces)
    assert g.dtype == np.int32, '%s faces: dtype %s' % (name, g.dtype)
    assert g.shape == w.shape and np.array_equal(g, w), '%s: faces differ' % name
    g, w = np.asarray(got_points), np.asarray(want_points)
    assert g.dtype == F32 and g.shape == w.shape, '%s: points %s %s' % (name, g.dtype, g.shape)
    assert np.array_equal(bits(g), bits(w)), '%s: points differ in %d rows' % (name, int((bits(g) != bits(w)).any(axis=1).sum()))


def assert_same_round(got, want, name=''):
    """one flip round: objects with faces and counts; the faces exact, the counts equal"""
    g, w = np.asarray(got.faces), np.asarray(want.faces)
    assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), '%s: faces differ' % name
    assert dict(got.counts) == dict(want.counts), '%s: counts %s != %s' % (name, got.counts, want.counts)


def assert_same(got, want, name=''):
    """a whole remesh: the mesh exact, the counts of every iteration equal, the statistics equal (the mean edge length, a
    sum in another order, to 1e-12 relative: E <= 10^4 positive terms at 2^-53 each)"""
    assert_same_mesh(got.points, got.faces, want.points, want.faces, name)
    assert list(got.per_iteration) == list(want.per_iteration), '%s: the counts of the iterations differ: %s != %s' % (
        name, got.per_iteration, want.per_iteration)
    for side in ('before', 'after'):
        g, w = dict(getattr(got, side)), dict(getattr(want, side))
        for key in ('edge_mean', 'valence_dev'):
            assert abs(g.pop(key) - w[key]) <= 1e-12 * abs(w.pop(key)), '%s: %s %s' % (name, side, key)
        assert g == w, '%s: %s statistics %s != %s' % (name, side, g, w)


# ---------------------------------------------------------------------------------------------- mesh facts and cases
def euler(points_or_V, faces):
    """V_used - E + F of the included faces"""
    t = S.Table(faces)
    used = np.unique(t.faces[t.included])
    return int(used.shape[0]) - t.E + int(t.included.sum())


def closed_manifold(faces):
    f = S.edge_facts(faces)
    return f['boundary'] == 0 and f['complex'] == 0 and f['repeated'] == 0


def scramble(points, faces, flips=300, seed=0):
    """apply up to `flips` random flips that keep a closed manifold (the diagonal must not exist, the ends keep valence >= 3,
    no geometric test): a mesh of the same V, F and Euler characteristic with a wide valence spread"""
    rng = np.random.RandomState(seed)
    faces = np.asarray(faces, dtype=np.int32).copy()
    done = 0
    for _ in range(20 * flips):
        if done == flips:
            break
        m = Mesh(points, faces)
        e = int(rng.randint(m.E))
        if m.t.n[e] != 2:
            continue
        s0, s1 = m.t.claimants[e]
        if m.direction(s0) == m.direction(s1):
            continue
        forth, back = (s0, s1) if m.direction(s0) == 0 else (s1, s0)
        a, b, c, d = int(m.t.lo[e]), int(m.t.hi[e]), m.third(forth), m.third(back)
        if c == d or (min(c, d), max(c, d)) in m.edge_set or len(m.nbrs[a]) < 4 or len(m.nbrs[b]) < 4:
            continue
        faces[forth // 3] = (a, d, c)
        faces[back // 3] = (b, c, d)
        done += 1
    return np.ascontiguousarray(points, dtype=F32), faces


def uv_sphere(n_lat=10, n_lon=24):
    """a sphere of latitude rings: the edges near the poles are far shorter than those at the equator, the poles have
    valence n_lon"""
    pts = [(0.0, 0.0, 1.0)]
    for i in range(1, n_lat):
        th = math.pi * i / n_lat
        for j in range(n_lon):
            ph = 2.0 * math.pi * j / n_lon
            pts.append((math.sin(th) * math.cos(ph), math.sin(th) * math.sin(ph), math.cos(th)))
    pts.append((0.0, 0.0, -1.0))
    south = len(pts) - 1

    def ring(i, j):
        return 1 + (i - 1) * n_lon + j % n_lon
    faces = []
    for j in range(n_lon):
        faces.append((0, ring(1, j), ring(1, j + 1)))
        faces.append((south, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)))
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            a, b, c, d = ring(i, j), ring(i + 1, j), ring(i + 1, j + 1), ring(i, j + 1)
            faces += [(a, b, c), (a, c, d)]
    return np.asarray(pts, dtype=F32), np.asarray(faces, dtype=np.int32)


def jittered_grid(n=8, seed=4):
    """the flat grid z = 0 on whole numbers with its interior vertices moved in the plane by multiples of 1 / 64"""
    pts, faces = S.grid(n, n)
    rng = np.random.RandomState(seed)
    interior = (pts[:, 0] > 0) & (pts[:, 0] < n) & (pts[:, 1] > 0) & (pts[:, 1] < n)
    jitter = rng.randint(-16, 17, size=(pts.shape[0], 2)) / 64.0
    pts[interior, :2] += jitter[interior].astype(F32)
    return pts, faces


def pillow():
    """(points, faces, lock): a closed lens whose flat side is the quad a d b c = 0 3 1 2 with the diagonal a - b, and whose
    other side already holds the edge c - d.  With a and b at target valence 4 the flip of a - b has gain 2 and passes the
    valence and the fold test: only the "diagonal exists" test refuses it"""
    pts = [(0, 1, 0), (0, -1, 0), (-1, 0, 0), (1, 0, 0), (-0.3, 0.4, 0.5), (0.3, 0.4, 0.5), (0.3, -0.4, 0.5), (-0.3, -0.4, 0.5)]
    faces = [(0, 1, 2), (1, 0, 3), (0, 2, 4), (0, 4, 5), (0, 5, 3), (2, 3, 4), (4, 3, 5), (1, 3, 6), (1, 6, 7), (1, 7, 2),
             (3, 2, 7), (3, 7, 6)]
    return np.asarray(pts, dtype=F32), np.asarray(faces, dtype=np.int32), np.array([1, 1, 0, 0, 0, 0, 0, 0], dtype=np.int32)


def rough_sphere(seed=1):
    """(points, faces, lock): the sphere of 2000 faces with isotropic noise of 0.3 mean edges, no vertex locked"""
    points, faces = D.icosphere(10)
    noise = 0.3 * mean_edge(points, faces) * np.random.RandomState(seed).randn(*points.shape)
    return (points + noise).astype(F32), faces, np.zeros(points.shape[0], dtype=np.int32)


def mean_edge(points, faces):
    return mesh_stats(points, faces, 0.0, 0.0)['edge_mean']
