"""Mesh preprocessing (the reference's dataset.py process_one_submesh and data_util.py calc_weight /
build_facet_graph / center_and_scale, as csrc/meshprep.hip cites them) in plain fp64 numpy, written from the definitions and
not from the kernels or the host generator: nothing of this package is imported.  Inputs are the fp32 arrays the device
receives, upcast.  Domain: every face has three DISTINCT vertex ids in [0, V) (a repeated id is `clean`'s job).

    incidence   rowptr [V + 1], list [3 F]: the faces of a vertex, ascending; a face appears once per corner, so a face that is
                listed twice appears under both of its ids
    normals     face: e1 x e2 / max(|e1 x e2|, 1e-12); vertex: s / max(|s|, 1e-12), s = sum of the incident unit face normals,
                once per incidence in ascending face order
    graphs      kind 0: vertices sharing a face; kind 1: faces sharing a vertex; loop-free, (row, col)-sorted, unique
    weights     w = max(n_i . n_j, 1e-3) * exp(|dp|^2 / (-2 mean + 1e-12)), mean = sum |dp| / max(E + extra, 1)

The second half builds the meshes that reach the kernels' edges (tests/test_gpu_meshprep_edges.py); each returns a Mesh whose
`cancelling` lists the vertices whose incident face normals cancel by construction."""
import numpy as np

EPS = 2.0 ** -24                 # unit roundoff of fp32


# ------------------------------------------------------------------------------------------------ the model
def _faces(faces):
    return np.asarray(faces, dtype=np.int64).reshape(-1, 3)


def _points(points):
    return np.asarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)


def vertex_faces(faces, V):
    """-> (rowptr [V + 1] int64, list [3 F] int64), face ids ascending within a vertex."""
    faces = _faces(faces)
    vert = faces.reshape(-1)
    face = np.repeat(np.arange(faces.shape[0], dtype=np.int64), 3)
    order = np.argsort(vert, kind='stable')              # stable: the faces of a vertex stay ascending
    rowptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(vert, minlength=V), out=rowptr[1:])
    return rowptr, face[order]


def max_degree(rowptr):
    return int(np.diff(rowptr).max()) if rowptr.shape[0] > 1 else 0


def vf_padded(rowptr, lst):
    """-> [V, max(valence, 1)] int64, -1 padded."""
    V = rowptr.shape[0] - 1
    vf = -np.ones((V, max(max_degree(rowptr), 1)), dtype=np.int64)
    owner = np.repeat(np.arange(V), np.diff(rowptr))
    vf[owner, np.arange(lst.shape[0]) - rowptr[owner]] = lst
    return vf


def face_cross(points, faces):
    """-> (e1 x e2 [F, 3], |e1| |e2| [F]) in fp64."""
    p, faces = _points(points), _faces(faces)
    e1, e2 = p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]]
    return np.cross(e1, e2), np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)


def face_normals(points, faces):
    c, _ = face_cross(points, faces)
    return c / np.maximum(np.sqrt((c * c).sum(1, keepdims=True)), 1e-12)


def centroids(points, faces):
    return _points(points)[_faces(faces)].sum(1) / 3.0


def vertex_normals(points, faces, rowptr=None, lst=None):
    """-> (unit normals [V, 3], |s| [V])."""
    V = np.asarray(points).reshape(-1, 3).shape[0]
    if rowptr is None:
        rowptr, lst = vertex_faces(faces, V)
    fn = face_normals(points, faces)
    s = np.zeros((V, 3))
    deg = np.diff(rowptr)
    for k in range(max_degree(rowptr)):                 # k-th incident face of every vertex that has one: ascending order
        has = np.nonzero(deg > k)[0]
        s[has] += fn[lst[rowptr[has] + k]]
    norm = np.sqrt((s * s).sum(1))
    return s / np.maximum(norm, 1e-12)[:, None], norm


def ring_graph(kind, faces, V, rowptr=None, lst=None):
    """-> (rowptr_g [n + 1], row [E], col [E]) int64 over n = V (kind 0) or F (kind 1) nodes."""
    faces = _faces(faces)
    if kind == 0:
        n = V
        a = np.concatenate([faces[:, i] for i in (0, 0, 1, 1, 2, 2)])
        b = np.concatenate([faces[:, i] for i in (1, 2, 0, 2, 0, 1)])
    else:
        n = faces.shape[0]
        if rowptr is None:
            rowptr, lst = vertex_faces(faces, V)
        deg = np.diff(rowptr)
        owner = np.repeat(np.arange(V), deg)            # vertex of every incidence entry
        a_parts, b_parts = [], []
        for k in range(max_degree(rowptr)):             # pair every incidence entry with the k-th face of its vertex
            sel = deg[owner] > k
            a_parts.append(lst[sel])
            b_parts.append(lst[rowptr[owner[sel]] + k])
        a = np.concatenate(a_parts) if a_parts else np.zeros(0, np.int64)
        b = np.concatenate(b_parts) if b_parts else np.zeros(0, np.int64)
    keep = a != b
    key = np.unique(a[keep] * max(n, 1) + b[keep])
    row, col = key // max(n, 1), key % max(n, 1)
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=n), out=rp[1:])
    return rp, row, col


def edge_lengths(pos, row, col):
    p = _points(pos)
    d = p[row] - p[col]
    return np.sqrt((d * d).sum(1))


def mean_edge_length(pos, row, col, extra=0):
    return float(edge_lengths(pos, row, col).sum() / max(row.shape[0] + extra, 1))


class Weights(object):
    """w = dn * ex; dn = max(n_i . n_j, 1e-3), arg = |dp|^2 / (-2 mean + 1e-12), ex = exp(arg); mean per edge."""

    def __init__(self, dn, arg, mean):
        self.dn, self.arg, self.mean = dn, arg, mean
        self.ex = np.exp(arg)
        self.w = dn * self.ex

    def tol(self):
        """What fp32 arithmetic owes this weight: an absolute 4 eps for the three-term fp32 dot product, about 4 roundings in
        arg, up to 2 ulp of expf and the product's rounding, and the flush of denormal results."""
        return self.ex * (4 * EPS + self.dn * (8 + 6 * np.abs(self.arg)) * EPS) + 2.0 ** -126


def _weights(pos, normal32, row, col, mean):
    length = edge_lengths(pos, row, col)
    n = _points(normal32)
    dn = np.maximum((n[row] * n[col]).sum(1), 1e-3)
    return Weights(dn, length * length / (-2.0 * mean + 1e-12), mean)


def calc_weight(pos, normal32, row, col, extra):
    """normal32: the fp32 normals the device used.  -> Weights"""
    return _weights(pos, normal32, row, col, mean_edge_length(pos, row, col, extra))


def calc_weight_parts(pos, normal32, rowptr, row, col, node_ptr):
    """Every part (nodes node_ptr[p] .. node_ptr[p + 1]) with its own mean over its edges plus one zero-length loop per node."""
    node_ptr = np.asarray(node_ptr, dtype=np.int64)
    length = edge_lengths(pos, row, col)
    mean = np.zeros(row.shape[0])
    for p in range(node_ptr.shape[0] - 1):
        a, b = node_ptr[p], node_ptr[p + 1]
        e0, e1 = rowptr[a], rowptr[b]
        mean[e0:e1] = length[e0:e1].sum() / max((e1 - e0) + (b - a), 1)
    return _weights(pos, normal32, row, col, mean)


def dual_features(points, faces, centroid32, vnormal32, fnormal32, graph_v=None):
    """The feature matrices of build_dual_data around a given fp32 centroid: x = cat((pos - centroid) * scale, normal),
    scale = 1 / mean mesh-edge length.  -> (x_v, x_f, scale)"""
    V = np.asarray(points).reshape(-1, 3).shape[0]
    _, row, col = graph_v if graph_v is not None else ring_graph(0, faces, V)
    scale = 1.0 / mean_edge_length(points, row, col, 0)
    cen = np.asarray(centroid32, dtype=np.float64).reshape(1, 3)
    x_v = np.concatenate([(_points(points) - cen) * scale, _points(vnormal32)], 1)
    x_f = np.concatenate([(centroids(points, faces) - cen) * scale, _points(fnormal32)], 1)
    return x_v, x_f, scale


# ------------------------------------------------------------------------------------------------ the meshes
class Mesh(object):
    def __init__(self, name, points, faces, cancelling=()):
        self.name = name
        self.points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        self.faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        self.cancelling = np.asarray(sorted(cancelling), dtype=np.int64)
        self.V, self.F = self.points.shape[0], self.faces.shape[0]


def grid(W, H, edge=1.0, jitter=0.2, z_amp=0.2, shift=(0.0, 0.0, 0.0), seed=0, name=None, z_normal=False):
    """W x H vertices (vertex j + W i), every cell cut along the same diagonal; xy jittered by `jitter`, z uniform in
    +- z_amp (z_normal: z_amp * N(0, 1)), all in units of `edge`; then moved by `shift`.  fp64 until the final cast."""
    rng = np.random.RandomState(seed)
    j, i = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    p = np.stack([j.ravel(), i.ravel(), np.zeros(W * H)], 1)
    p[:, :2] += jitter * rng.uniform(-1, 1, (W * H, 2))
    p[:, 2] = z_amp * (rng.standard_normal(W * H) if z_normal else rng.uniform(-1, 1, W * H))
    p = p * edge + np.asarray(shift, dtype=np.float64)
    v = (np.arange(W - 1)[None, :] + W * np.arange(H - 1)[:, None]).ravel()
    faces = np.concatenate([np.stack([v, v + 1, v + W + 1], 1), np.stack([v, v + W + 1, v + W], 1)], 1).reshape(-1, 3)
    return Mesh(name or 'grid%dx%d' % (W, H), p, faces)


def fan(k, first=1, hub=0, closed=True):
    """Faces of a fan of k sectors around `hub` over the ring vertices first .. first + k - 1 (k + 1 if open)."""
    if closed:
        return [[hub, first + i, first + (i + 1) % k] for i in range(k)]
    return [[hub, first + i, first + i + 1] for i in range(k)]


def _ring_points(k, radius=1.0, z0=0.0, phase=0.0):
    ang = np.linspace(0, 2 * np.pi, k, endpoint=False) + phase
    return np.stack([radius * np.cos(ang), radius * np.sin(ang), z0 + 0.1 * np.sin(3 * ang)], 1)


def fan300():
    """A disc whose hub has valence 300: facet-graph rows of 299+ entries, incidence row of length 300."""
    p = np.concatenate([[[0, 0, 0.3]], _ring_points(300)], 0)
    return Mesh('fan300', p, fan(300))


def bowtie():
    """Two fans (7 and 5 sectors) that share only their hub."""
    p = np.concatenate([[[0, 0, 0]], _ring_points(7, 1.0, 1.0), _ring_points(5, 0.8, -1.0, 0.3)], 0)
    return Mesh('bowtie', p, fan(7, 1) + fan(5, 8))


def book():
    """Three faces on the edge (0, 1)."""
    p = [[0, 0, 0], [1, 0, 0], [0.5, 1, 0.1], [0.4, -0.6, 0.8], [0.6, -0.5, -0.9]]
    return Mesh('book', p, [[0, 1, 2], [0, 1, 3], [1, 0, 4]])


def doubled():
    """9 x 9 vertices (8 x 8 cells); every 5th face listed twice; then every listed face around two interior vertices listed
    once more, reversed: the unit normals at those two vertices cancel in pairs."""
    g = grid(9, 9, seed=5)
    faces = np.concatenate([g.faces, g.faces[::5]], 0)
    hubs = [2 + 9 * 2, 6 + 9 * 5]
    around = faces[np.isin(faces, hubs).any(1)]
    return Mesh('doubled', g.points, np.concatenate([faces, around[:, ::-1]], 0), cancelling=hubs)


def isolated():
    """A grid with face-less vertices at index 0, in the middle and as a trailing block of 300."""
    g = grid(6, 5, seed=2)
    mid = 17
    ids = np.arange(g.V)
    new_id = 1 + ids + (ids >= mid)                      # vertex 0 and vertex mid + 1 stay without faces
    rng = np.random.RandomState(9)
    p = 10 * rng.uniform(-1, 1, (g.V + 2 + 300, 3))
    p[new_id] = g.points
    return Mesh('isolated', p, new_id[g.faces])


def single():
    return Mesh('single', [[0, 0, 0], [1, 0.1, 0], [0.2, 1, 0.3]], [[0, 1, 2]])


def two_disjoint():
    p = [[0, 0, 0], [1, 0.1, 0], [0.2, 1, 0.3], [5, 5, 5], [5.5, 6, 5], [4, 5.5, 6]]
    return Mesh('two_disjoint', p, [[0, 1, 2], [5, 4, 3]])


def degenerate():
    """7 x 6 vertices on exact integer x, y with z a function of the row only, plus four zero-area faces of three distinct
    vertices of one row: both edge vectors are (integer, 0, 0), so the cross product is exactly 0 in any arithmetic."""
    W, H = 7, 6
    g = grid(W, H, jitter=0.0, z_amp=0.0)
    p = g.points.astype(np.float64)
    p[:, 2] = 0.37 * np.sin(1.3 * p[:, 1])
    flat = [[0 + W * 1, 1 + W * 1, 2 + W * 1], [6 + W * 3, 2 + W * 3, 4 + W * 3], [3 + W * 5, 5 + W * 5, 4 + W * 5],
            [1 + W * 0, 0 + W * 0, 5 + W * 0]]
    m = Mesh('degenerate', p, np.concatenate([g.faces[:20], flat[:2], g.faces[20:], flat[2:]], 0))
    m.flat_faces = np.asarray([20, 21, m.F - 2, m.F - 1])
    return m


def unit_grid(edge, rough=False):
    """The 40 x 40 grid in units of `edge`; rough: z amplitude 3 edges, where many edges sit on the 1e-3 clamp."""
    return grid(40, 40, edge=edge, z_amp=3.0 if rough else 0.2, seed=11, z_normal=rough,
                name='rough' if rough else 'unit%g' % edge)


def shifted(far=False):
    return grid(40, 40, shift=(1e4, 1e4, 1e4) if far else (1e3, -7e2, 3e2), seed=11, name='shifted1e4' if far else 'shifted')


SCAN_GRIDS = {'127x129': (127, 129), '128x128': (128, 128), '511x513': (511, 513), '512x512': (512, 512)}


def scan_grid(key):
    W, H = SCAN_GRIDS[key]
    return grid(W, H, seed=W, name='scan' + key)


SMALL = {'fan300': fan300, 'bowtie': bowtie, 'book': book, 'doubled': doubled, 'isolated': isolated, 'single': single,
         'two_disjoint': two_disjoint, 'degenerate': degenerate,
         'shifted': shifted, 'shifted1e4': lambda: shifted(True),
         'unit0.001': lambda: unit_grid(1e-3), 'unit1': lambda: unit_grid(1.0), 'unit20': lambda: unit_grid(20.0),
         'unit50': lambda: unit_grid(50.0), 'unit400': lambda: unit_grid(400.0), 'rough': lambda: unit_grid(1.0, True)}
