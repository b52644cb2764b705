"""The winding-number rules of include/geobi_hip.h (geobi_winding_number, geobi_part_solids) restated in
numpy fp64, in the stated order of operations, and the outward rule of meshwind.orient_outward stated sequentially.

numpy evaluates every product, sum and difference on its own (no FMA), its sqrt and division are correctly rounded like the
device's; only atan2 may round differently, which moves a term by at most one quantum of 2^-40 when the quotient lies
across a rounding boundary (tests/test_wind_model_host.py holds the float error against a 60-digit evaluation)."""
import numpy as np

QUANTA = float(2 ** 40)            # quanta per full turn
FOUR_PI = 4.0 * np.pi              # the fp64 nearest to pi, times 4: exact
TILE = 256                         # faces per target tile
QUERY_BLOCK = 256                  # queries per workgroup: one per lane


# ------------------------------------------------------------------------------------------------ the term and the sum
def _dot(u, w):
    return (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]


def det3(a, b, c):
    return ((a[..., 0] * (b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1]) + a[..., 1] * (b[..., 2] * c[..., 0] - b[..., 0] * c[..., 2]))
            + a[..., 2] * (b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0]))


def thetas(q, tri):
    """q [Q, 3], tri [F, 3, 3] -> (theta [Q, F] fp64 with the det == 0 rule applied, det [Q, F])"""
    q = np.asarray(q, dtype=np.float32).astype(np.float64).reshape(-1, 1, 3)
    tri = np.asarray(tri, dtype=np.float32).astype(np.float64)
    a, b, c = tri[None, :, 0] - q, tri[None, :, 1] - q, tri[None, :, 2] - q
    det = det3(a, b, c)
    la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
    den = (la * (lb * lc) + _dot(b, c) * la) + (_dot(a, b) * lc + _dot(c, a) * lb)
    theta = 2.0 * np.arctan2(det, den)
    return np.where(det == 0.0, 0.0, theta), det


def included(faces, V, state=None):
    f = np.asarray(faces).reshape(-1, 3)
    ok = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0]) & (f >= 0).all(1) & (f < V).all(1)
    return ok if state is None else ok & (np.asarray(state) == 1)


def terms(q, verts, faces, state=None, face_part=None, query_part=None, chunk=256):
    """the int64 quanta of every pair [Q, F]: 0 for a face that does not take part and for a pair of equal parts"""
    verts = np.asarray(verts, dtype=np.float32)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    q = np.asarray(q, dtype=np.float32).reshape(-1, 3)
    inc = included(faces, verts.shape[0], state)
    tri = verts[np.where(inc[:, None], faces, 0)]
    out = np.zeros((q.shape[0], faces.shape[0]), dtype=np.int64)
    for i in range(0, q.shape[0], chunk):
        theta, _ = thetas(q[i:i + chunk], tri)
        out[i:i + chunk] = np.rint(theta / FOUR_PI * QUANTA).astype(np.int64)
    out[:, ~inc] = 0
    if face_part is not None and query_part is not None:
        out[np.asarray(query_part).reshape(-1, 1) == np.asarray(face_part).reshape(1, -1)] = 0
    return out


def winding(q, verts, faces, state=None, face_part=None, query_part=None):
    """w [Q] float64: the integer sum of the quanta times 2^-40"""
    return terms(q, verts, faces, state, face_part, query_part).sum(axis=1).astype(np.float64) * (1.0 / QUANTA)


def winding_plain(q, verts, faces):
    """the unquantised fp64 sum over 4 pi, faces in ascending order (what the tolerance check compares with mpmath)"""
    theta, _ = thetas(q, np.asarray(verts, dtype=np.float32)[np.asarray(faces)])
    return np.array([sum(row.tolist()) for row in theta]) / FOUR_PI


# ------------------------------------------------------------------------------------------------ components
def orient_labels(faces, state=None, V=None):
    """the labels and flips of meshtopo for tables whose edges have at most two claimants with different
    opposite corners: label = the lowest face of the component, flip = the parity of odd links on a path from it"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    F = faces.shape[0]
    inc = included(faces, faces.max() + 1 if V is None and F else (V or 0), state)
    edges = {}
    for f in np.flatnonzero(inc):
        for k in range(3):
            a, b = int(faces[f, k]), int(faces[f, (k + 1) % 3])
            edges.setdefault((min(a, b), max(a, b)), []).append((f, a < b))
    links = {f: [] for f in np.flatnonzero(inc)}
    for claim in edges.values():
        if len(claim) == 2:
            (f, df), (g, dg) = claim
            links[f].append((g, df == dg))
            links[g].append((f, df == dg))
    label, flip = np.full(F, -1, dtype=np.int32), np.zeros(F, dtype=np.int32)
    for f in np.flatnonzero(inc):
        if label[f] >= 0:
            continue
        label[f] = f
        todo = [f]
        while todo:
            x = todo.pop()
            for y, odd in links[x]:
                if label[y] < 0:
                    label[y], flip[y] = f, flip[x] ^ int(odd)
                    todo.append(y)
    return label, flip


def part_solids(verts, faces, label, state=None):
    """-> (volume6 [F] fp64, closed [F], consistent [F] int32) at the rows x == label[x], zeros elsewhere: the device's
    order -- the component's faces ascending, rank r into partial sum r mod 64, the 64 partial sums ascending from 0.0"""
    verts = np.asarray(verts, dtype=np.float32).astype(np.float64)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    label = np.asarray(label)
    F = faces.shape[0]
    inc = included(faces, verts.shape[0], state) & (label >= 0) & (label < F)
    volume6, closed, consistent = np.zeros(F), np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.int32)
    edges = {}
    for f in np.flatnonzero(inc):
        for k in range(3):
            a, b = int(faces[f, k]), int(faces[f, (k + 1) % 3])
            edges.setdefault((min(a, b), max(a, b)), []).append((f, a < b))
    for x in np.flatnonzero(inc & (label == np.arange(F))):
        members = np.flatnonzero(inc & (label == x))
        o = verts[faces[x, 0]]
        t = det3(verts[faces[members, 0]] - o, verts[faces[members, 1]] - o, verts[faces[members, 2]] - o)
        total = 0.0
        for lane in range(64):
            partial = 0.0
            for value in t[lane::64].tolist():
                partial += value
            total += partial
        volume6[x] = total
        closed[x], consistent[x] = 1, 1
    for claim in edges.values():
        if len(claim) != 2:
            for f, _ in claim:
                closed[label[f]] = 0
        elif claim[0][1] == claim[1][1]:
            for f, _ in claim:
                consistent[label[f]] = 0
    return volume6, closed, consistent


def flipped(faces, mask):
    out = np.array(faces, copy=True)
    out[mask] = out[mask][:, [0, 2, 1]]
    return out


def orient_outward(verts, faces, state=None):
    """The outward rule, one step after the other -> (faces, flip, label, counts): orient; turn the closed consistent
    components of negative volume; one query per such component (the first corner of its lowest face) against the others'
    faces, odd depth turns again; |w - depth| > 1/4 is ambiguous and stays."""
    verts = np.asarray(verts, dtype=np.float32)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    F = faces.shape[0]
    label, flip = orient_labels(faces, state, verts.shape[0])
    now = flipped(faces, flip == 1)
    volume6, closed, consistent = part_solids(verts, now, label, state)
    roots = np.flatnonzero(label == np.arange(F))
    solid = [x for x in roots if closed[x] and consistent[x] and volume6[x] != 0.0]
    turn_1 = np.zeros(F, dtype=bool)
    for x in solid:
        turn_1[x] = volume6[x] < 0.0
    now = flipped(now, (label >= 0) & turn_1[np.maximum(label, 0)])
    turn_2, ambiguous = np.zeros(F, dtype=bool), 0
    if solid:
        in_solid = np.isin(label, solid).astype(np.int32)
        w = winding(verts[now[solid, 0]], verts, now, in_solid, label, np.array(solid))
        for x, wx in zip(solid, w):
            d = np.rint(wx)
            if abs(wx - d) > 0.25:
                ambiguous += 1
            else:
                turn_2[x] = int(d) % 2 == 1
        now = flipped(now, (label >= 0) & turn_2[np.maximum(label, 0)])
    both = turn_1 ^ turn_2
    flip = flip ^ ((label >= 0) & both[np.maximum(label, 0)]).astype(np.int32)
    counts = {'components': len(roots), 'closed_components': len(solid), 'open_components': len(roots) - len(solid),
              'turned': int(both.sum()), 'ambiguous': ambiguous, 'flipped': int(flip.sum())}
    return now.astype(np.int32), flip, label, counts


# ------------------------------------------------------------------------------------------------ builders
def sphere(k, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """the octahedron subdivided k times and pushed to the sphere: F = 8 * 4^k, wound outward, corners rounded to float32"""
    v = [(1.0, 0, 0), (-1.0, 0, 0), (0, 1.0, 0), (0, -1.0, 0), (0, 0, 1.0), (0, 0, -1.0)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(k):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = np.add(v[a], v[b]) / 2.0
                v.append(tuple(m / np.linalg.norm(m)))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = nf
    pts = np.asarray(v, dtype=np.float64) * radius + np.asarray(centre, dtype=np.float64)
    return pts.astype(np.float32), np.asarray(f, dtype=np.int32)


def join(meshes):
    """several (points, faces) -> one; the faces of a part keep their order, the parts theirs"""
    pts, faces, base = [], [], 0
    for p, f in meshes:
        pts.append(p)
        faces.append(f + base)
        base += p.shape[0]
    return np.concatenate(pts), np.concatenate(faces).astype(np.int32)


NESTED = ((1.0, (0, 0, 0)), (0.5, (0, 0, 0)), (0.25, (0, 0, 0)), (0.5, (3.0, 0, 0)))
NESTED_SIGNS = (1, -1, 1, 1)          # the outward rule: the shell at depth 1 is a cavity


def nested():
    """spheres of 128 faces at radii 1, 0.5 and 0.25 about the origin and one of radius 0.5 about (3, 0, 0), all wound
    outward -> (points, faces); part p holds the faces 128 p .. 128 p + 127"""
    return join([sphere(2, r, c) for r, c in NESTED])


def cube():
    """the unit cube with integer corners, twelve faces wound outward"""
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float32)      # id = 4x + 2y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = []
    for a, b, c, d in quads:
        f += [(a, b, c), (a, c, d)]
    return v, np.asarray(f, dtype=np.int32)


def mean_edge(points, faces):
    f = np.asarray(faces, dtype=np.int64)
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    p = np.asarray(points, dtype=np.float64)
    return float(np.linalg.norm(p[e[:, 0]] - p[e[:, 1]], axis=1).mean())


def directions(n, seed):
    d = np.random.RandomState(seed).standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def signed_volume6(points, faces):
    p = np.asarray(points, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    return float(det3(p[:, 0], p[:, 1], p[:, 2]).sum())
