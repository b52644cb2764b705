"""Host model of geobi_sample_weights / geobi_sample_surface (include/geobi_hip.h): fp64 weights as numpy
rounds them, Python-integer cum / t, searchsorted(side='right'), float32 barycentrics, fp64 points.  Built on
noise_model.words_of and uniform.  Shared by tests/test_sample_model_host.py and tests/test_gpu_sample.py."""
import math

import numpy as np

import noise_model as NM

BLOCK = 2                                    # Philox block of the sampler (0 and 1 are the noise kernel's)


# ------------------------------------------------------------------------------------------------ the algorithm
def face_norms(points, faces):
    """d[f] = |e1 x e2| in fp64 from the float32 corners, every product and difference rounded on its own; non-finite
    -> 0."""
    p = np.asarray(points, np.float32).astype(np.float64)
    f = np.asarray(faces)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    e1, e2 = b - a, c - a
    with np.errstate(all='ignore'):
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        d = np.sqrt((cx * cx + cy * cy) + cz * cz)
    return np.where(np.isfinite(d), d, 0.0)


def weights(points, faces):
    """-> (weight int64 [F], cum int64 [F], exponent): weight = floor(ldexp(d, 32 - e)), frexp(max d) = m 2^e."""
    d = face_norms(points, faces)
    dmax = float(d.max()) if len(d) else 0.0
    e = math.frexp(dmax)[1] if dmax > 0 else 0
    w = np.floor(np.ldexp(d, 32 - e)).astype(np.int64)
    cum, total = np.empty(len(w), np.int64), 0
    for i, x in enumerate(w.tolist()):       # Python integers: no wrap to hide
        total += x
        cum[i] = total
    assert total < 2 ** 56
    return w, cum, e


def select(cum, n, seed, stream_id=0, draw=0, first=0):
    """-> (face int64 [n], (w2, w3) the two words the barycentrics take): t = (r * total) >> 64 in Python integers, face =
    the first f with cum[f] > t."""
    cum = np.asarray(cum, np.int64)
    total = int(cum[-1])
    w = NM.words_of(np.arange(first, first + n, dtype=np.uint64), seed, stream_id, draw, BLOCK)
    if total == 0:
        return np.full(n, -1, np.int64), (w[2], w[3])
    r = (w[0] << np.uint64(32)) | w[1]
    t = np.array([(int(x) * total) >> 64 for x in r.tolist()], dtype=np.int64)
    return np.searchsorted(cum, t, side='right').astype(np.int64), (w[2], w[3])


def bary32(w2, w3):
    """The fold and b = (1 - u1 - u2, u1, u2) with every operation in float32 -> float32 [n, 3]."""
    u1, u2 = NM.uniform(w2).astype(np.float32), NM.uniform(w3).astype(np.float32)
    one = np.float32(1.0)
    fold = (u1 + u2) > one
    u1, u2 = np.where(fold, one - u1, u1), np.where(fold, one - u2, u2)
    return np.stack([(one - u1) - u2, u1, u2], 1).astype(np.float32)


def bary64(w2, w3):
    """The same statement in fp64: what bary32 must equal exactly."""
    u1, u2 = NM.uniform(w2), NM.uniform(w3)
    fold = (u1 + u2) > 1.0
    u1, u2 = np.where(fold, 1.0 - u1, u1), np.where(fold, 1.0 - u2, u2)
    return np.stack([1.0 - u1 - u2, u1, u2], 1)


def combine(points, faces, face, bary):
    """fp64 points of the samples: sum_k bary[k] * corner k."""
    p = np.asarray(points, np.float32).astype(np.float64)
    f = np.asarray(faces)[face]
    b = np.asarray(bary, np.float64)
    return b[:, :1] * p[f[:, 0]] + b[:, 1:2] * p[f[:, 1]] + b[:, 2:] * p[f[:, 2]]


def sample(points, faces, n, seed, stream_id=0, draw=0, first=0, cum=None):
    """-> dict(points fp64 [n,3], face [n], bary float32 [n,3]).  cum: another scan to select by (the device's)."""
    if cum is None:
        cum = weights(points, faces)[1]
    face, (w2, w3) = select(cum, n, seed, stream_id, draw, first)
    bary = bary32(w2, w3)
    return {'points': combine(points, faces, face, bary), 'face': face, 'bary': bary}


# ------------------------------------------------------------------------------------------------ inputs
def strip(F, seed=0, grid=False, degenerate=(), offset=0.0, heavy=None):
    """A zig-zag strip of F triangles over F + 2 vertices with pseudo-random widths, so the areas differ.  grid:
    coordinates on the 1/8 grid below 64 (every intermediate of the weights is then exact).  degenerate: face ids whose
    third corner repeats the first.  heavy: a face id -- that face becomes a triangle of its own three vertices that holds
    90 % of the area.  -> points float32 [V,3], faces int32 [F,3]."""
    rng = np.random.default_rng(4000 + seed)
    nv = F + 2
    if grid:
        x = np.cumsum(rng.integers(1, 4, nv)) % 512 / 8.0
        y = np.where(np.arange(nv) % 2 == 0, 0.0, 1.0) * rng.integers(1, 64, nv) / 8.0
        z = rng.integers(0, 512, nv) / 8.0
    else:
        x = np.cumsum(rng.uniform(0.05, 1.0, nv)) * (8.0 / nv if nv > 64 else 1.0)
        y = np.where(np.arange(nv) % 2 == 0, 0.0, 1.0) * rng.uniform(0.2, 1.5, nv)
        z = 0.3 * np.sin(0.37 * np.arange(nv)) + rng.uniform(-0.1, 0.1, nv)
    p = np.stack([x, y, z], 1) + offset
    f = np.stack([np.arange(F), np.arange(F) + 1, np.arange(F) + 2], 1)
    f[1::2] = f[1::2][:, [1, 0, 2]]
    if heavy is not None:
        rest = np.delete(f, heavy, 0)
        area = 0.5 * np.linalg.norm(np.cross(p[rest[:, 1]] - p[rest[:, 0]], p[rest[:, 2]] - p[rest[:, 0]]), axis=1).sum()
        leg = math.sqrt(2 * 9.5 * area)          # a right triangle of 9.5 times the others' area: 90.5 % of the whole
        p = np.concatenate([p, np.array([[0, 0, 5.0], [leg, 0, 5.0], [0, leg, 5.0]]) + offset])
        f[heavy] = [len(p) - 3, len(p) - 2, len(p) - 1]
    for k in degenerate:
        f[k, 2] = f[k, 0]
    return p.astype(np.float32), f.astype(np.int32)


def box(nx=1, size=(1.0, 0.7, 0.4)):
    """The box [0, size] with an nx x nx grid per side (two triangles per cell), vertices shared along the edges.
    -> points float64 [V,3], faces int64 [F,3].  nx = 1: 8 vertices, 12 triangles; nx = 12: 866 vertices."""
    index, pts, faces = {}, [], []

    def vid(q):
        key = tuple(int(round(v * nx)) for v in q)
        if key not in index:
            index[key] = len(pts)
            pts.append([key[0] / nx * size[0], key[1] / nx * size[1], key[2] / nx * size[2]])
        return index[key]
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, 1):
            for i in range(nx):
                for j in range(nx):
                    def corner(di, dj):
                        q = [0.0, 0.0, 0.0]
                        q[axis], q[u], q[v] = float(side), (i + di) / nx, (j + dj) / nx
                        return vid(q)
                    a, b, c, d = corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)
                    faces += [(a, b, c), (a, c, d)] if side else [(a, c, b), (a, d, c)]
    return np.asarray(pts, np.float64), np.asarray(faces, np.int64)


def box_case(degrees=5.0):
    """The alignment experiment of DESIGN.md 4l: target = the 1 x 0.7 x 0.4 box as 12 triangles (float32), source = the
    same box with a 12 x 12 grid per side, turned by `degrees` about (1, 2, 3) and shifted by (0.02, -0.01, 0.015).
    -> source float32 [866,3], source faces, target float32 [8,3], target faces, R_true (of source -> target)."""
    import icp_model as M
    tp, tf = box(1)
    sp, sf = box(12)
    R = M.rotation((1, 2, 3), degrees)
    src = (sp @ R + np.array([0.02, -0.01, 0.015])).astype(np.float32)
    return src, sf, tp.astype(np.float32), tf, R.T


def residual_angle(R_found, R_true):
    """Angle in degrees between the rotation ICP found and the true one."""
    import icp_model as M
    return M.rotation_angle(np.asarray(R_found) @ np.asarray(R_true).T)


def folded_quad(h=0.3):
    """The quad (0,0,0), (1,0,h), (1,1,0), (0,1,h) cut along one diagonal and along the other: two meshes that share all
    four vertices and are h apart in the middle.  -> points float32 [4,3], faces A, faces B (int32 [2,3])."""
    p = np.array([[0, 0, 0], [1, 0, h], [1, 1, 0], [0, 1, h]], np.float32)
    return p, np.array([[0, 1, 2], [0, 2, 3]], np.int32), np.array([[0, 1, 3], [1, 2, 3]], np.int32)
