"""fp64 / numpy statement of the sampled surface Chamfer loss: the per-part sampler as sample_model applied
part by part with offset faces, the points on faces, the inverse-list backward written as explicit loops, and the SCD value
and gradient with given index maps.  Shared by tests/test_scd_model_host.py and tests/test_gpu_scd.py."""
import numpy as np

import sample_model as S
from chamfer_model import _argmin64


# ------------------------------------------------------------------------------------------------ the batched sampler
def weights_parts(points, faces, fptr):
    """-> (weight int64 [F], cum int64 [F], exponent [P]): sample_model.weights of every part on its own.  The faces hold
    global vertex ids, so a part's rows index the union's points as they are."""
    faces = np.asarray(faces)
    w, cum, e = [], [], []
    for a, b in zip(fptr[:-1], fptr[1:]):
        wk, ck, ek = S.weights(points, faces[a:b])
        w.append(wk), cum.append(ck), e.append(ek)
    return np.concatenate(w), np.concatenate(cum), np.asarray(e, np.int64)


def sample_parts(points, faces, fptr, n, seed, stream_ids, draw=0, first=0, cum=None):
    """n samples per part, row p * n + i = sample i of part p: sample_model.sample of the part alone with stream_ids[p],
    its face plus fptr[p].  cum: another scan to select by (the device's, the union's [F]).
    -> dict(points fp64 [P n, 3], face [P n], bary float32 [P n, 3])"""
    faces = np.asarray(faces)
    out = {'points': [], 'face': [], 'bary': []}
    for p, (a, b) in enumerate(zip(fptr[:-1], fptr[1:])):
        s = S.sample(points, faces[a:b], n, seed, stream_ids[p], draw, first, cum=None if cum is None else cum[a:b])
        out['points'].append(s['points'])
        out['face'].append(np.where(s['face'] >= 0, s['face'] + a, -1))
        out['bary'].append(s['bary'])
    return {k: np.concatenate(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ points on faces
def bary_points64(points, faces, face, bary):
    """x_i = sum_k bary[i, k] * points[faces[face[i], k]] in fp64; a row with face = -1 is zeros."""
    p, f = np.asarray(points, np.float64), np.asarray(faces)
    face, b = np.asarray(face, np.int64), np.asarray(bary, np.float64)
    on = face >= 0
    corners = p[f[np.where(on, face, 0)]]                       # [n, 3 corners, 3]
    return np.where(on[:, None], (b[:, :, None] * corners).sum(1), 0.0)


def inverse_lists(faces, face, V):
    """vertex -> the entries e = 3 i + k with faces[face[i], k] == v, ascending (a row with face = -1 is in no list)."""
    lists = [[] for _ in range(V)]
    f = np.asarray(faces)
    for i, fi in enumerate(np.asarray(face).tolist()):
        if fi < 0:
            continue
        for k in range(3):
            lists[int(f[fi, k])].append(3 * i + k)
    return lists


def bary_points_bwd_loops(faces, face, bary, gx, V):
    """gp[v] = sum over the entries e = 3 i + k of v's list, in ascending order, of bary[i, k] * gx[i], in fp64."""
    b, gx = np.asarray(bary, np.float64).reshape(-1), np.asarray(gx, np.float64)
    gp = np.zeros((V, 3))
    for v, entries in enumerate(inverse_lists(faces, face, V)):
        acc = np.zeros(3)
        for e in entries:
            acc = acc + b[e] * gx[e // 3]
        gp[v] = acc
    return gp


# ------------------------------------------------------------------------------------------------ the loss
def scd64(p, faces, face, bary, y, n, maps=None):
    """SCD of a union batch with the samples given: X = bary_points64(p, faces, face, bary) [P n, 3] against the target
    samples y [P n, 3], part k = rows k n .. (k + 1) n; mean over the parts of mean_i |x_i - y_a(i)|^2 + mean_j
    |x_b(j) - y_j|^2.  maps = (a, b): the two index maps as global rows (the device's); None: the fp64 arg-mins.
    -> value, gradient to p [V, 3], gradient to X"""
    p, y = np.asarray(p, np.float64), np.asarray(y, np.float64)
    x = bary_points64(p, faces, face, bary)
    P = len(x) // n
    value, gx = 0.0, np.zeros_like(x)
    for k in range(P):
        r = slice(k * n, (k + 1) * n)
        if maps is None:
            a, b = _argmin64(x[r], y[r])[0], _argmin64(y[r], x[r])[0]
        else:
            a, b = np.asarray(maps[0])[r] - k * n, np.asarray(maps[1])[r] - k * n
        xk, yk = x[r], y[r]
        value += (((xk - yk[a]) ** 2).sum(1).mean() + ((xk[b] - yk) ** 2).sum(1).mean()) / P
        g = (2.0 / n) * (xk - yk[a])
        np.add.at(g, b, (2.0 / n) * (xk[b] - yk))
        gx[r] = g / P
    return value, bary_points_bwd_loops(faces, face, bary, gx, len(p)), gx


def scd_of_meshes(p, t, faces, fptr, n, seed, stream_ids, draw=0):
    """The whole loss on the host: the prediction drawn with 2 draw + 1, the target with 2 draw -> value, gradient to p."""
    sp = sample_parts(np.asarray(p, np.float32), faces, fptr, n, seed, stream_ids, 2 * draw + 1)
    st = sample_parts(np.asarray(t, np.float32), faces, fptr, n, seed, stream_ids, 2 * draw)
    value, gp, _ = scd64(np.asarray(p, np.float32), faces, sp['face'], sp['bary'], st['points'], n)
    return value, gp


def folded_pair(h=0.3):
    """The folded quad of DESIGN.md 4l as a prediction and a target that share ONE face table, as the loss takes them: the
    target is the prediction's rows rolled by one, which turns the table's diagonal 0-2 into the diagonal 1-3.  The two
    vertex SETS are equal; the surfaces are h apart in the middle.  -> p, t float32 [4,3], faces int32 [2,3]"""
    p, fa, fb = S.folded_quad(h)
    t = np.roll(p, -1, axis=0)
    assert {tuple(sorted(r)) for r in ((fa + 1) % 4).tolist()} == {tuple(sorted(r)) for r in fb.tolist()}
    return p, t, fa


def fan(n_faces=64, seed=0):
    """n_faces triangles around the hub vertex 0 (a closed fan, slightly out of plane): every sample touches the hub.
    -> points float32 [n_faces + 1, 3], faces int32 [n_faces, 3]"""
    rng = np.random.default_rng(7000 + seed)
    ang = 2 * np.pi * np.arange(n_faces) / n_faces
    rim = np.stack([np.cos(ang), np.sin(ang), 0.2 * rng.standard_normal(n_faces)], 1) * rng.uniform(0.8, 1.2, (n_faces, 1))
    pts = np.concatenate([[[0.0, 0.0, 0.5]], rim]).astype(np.float32)
    k = np.arange(n_faces)
    return pts, np.stack([np.zeros(n_faces, np.int64), 1 + k, 1 + (k + 1) % n_faces], 1).astype(np.int32)
