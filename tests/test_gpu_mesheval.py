"""Nearest-vertex / point-to-surface distances (csrc/dist.hip), eval_pair and the denoise / eval command line on the
device.  The fp64 statements the kernels are compared against are the numpy functions of this file."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5                      # the project's bar (tests/test_gpu_kernels.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


# ------------------------------------------------------------------ fp64 statements (numpy)
def _mean_edge(points, faces):
    from geobi_gnn_amd import meshgen
    ev = meshgen.mesh_edges(np.asarray(faces))
    p = np.asarray(points, dtype=np.float64)
    return float(np.linalg.norm(p[ev[:, 0]] - p[ev[:, 1]], axis=1).mean())


def _nearest_fp64(q, t, chunk=256):
    q, t = np.asarray(q, dtype=np.float64), np.asarray(t, dtype=np.float64)
    out = np.empty(q.shape[0])
    for i in range(0, q.shape[0], chunk):
        d = q[i:i + chunk, None, :] - t[None, :, :]
        out[i:i + chunk] = np.sqrt((d * d).sum(-1).min(1))
    return out


def _dot(a, b):
    return (a * b).sum(-1)


def _tri_dist_fp64(p, a, b, c):
    """Distance from p to triangle (a, b, c), broadcasting over leading axes: the region-classifying closest point
    (Ericson, Real-Time Collision Detection 5.1.5), every dot product formed from its own difference vectors."""
    p, a, b, c = [np.asarray(x, dtype=np.float64) for x in (p, a, b, c)]
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(all='ignore'):
        den = va + vb + vc
        v, w = vb / den, vc / den
        m = (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)
        t = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        v, w = np.where(m, 1 - t, v), np.where(m, t, w)
        m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        v, w = np.where(m, 0.0, v), np.where(m, d2 / (d2 - d6), w)
        m = (d6 >= 0) & (d5 <= d6)
        v, w = np.where(m, 0.0, v), np.where(m, 1.0, w)
        m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        v, w = np.where(m, d1 / (d1 - d3), v), np.where(m, 0.0, w)
        m = (d3 >= 0) & (d4 <= d3)
        v, w = np.where(m, 1.0, v), np.where(m, 0.0, w)
        m = (d1 <= 0) & (d2 <= 0)
        v, w = np.where(m, 0.0, v), np.where(m, 0.0, w)
    e = ap - v[..., None] * ab - w[..., None] * ac
    return np.sqrt(_dot(e, e))


def _surface_fp64(q, verts, faces, chunk=64):
    q, verts = np.asarray(q, dtype=np.float64), np.asarray(verts, dtype=np.float64)
    a, b, c = verts[faces[:, 0]][None], verts[faces[:, 1]][None], verts[faces[:, 2]][None]
    out = np.empty(q.shape[0])
    for i in range(0, q.shape[0], chunk):
        out[i:i + chunk] = _tri_dist_fp64(q[i:i + chunk, None, :], a, b, c).min(1)
    return out


def _segment_dist_fp64(p, a, b):
    p, a, b = [np.asarray(x, dtype=np.float64) for x in (p, a, b)]
    ab = b - a
    t = np.clip(_dot(p - a, ab) / _dot(ab, ab), 0.0, 1.0)
    e = p - a - t[..., None] * ab
    return np.sqrt(_dot(e, e))


def _rel(d_gpu, d_ref, e):
    return float((np.abs(np.asarray(d_gpu, dtype=np.float64) - d_ref) / (d_ref + e)).max())


def _t(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


_CASES = {
    'n9_on_n8': (9, 0.2, 8, None, False),
    'n13_on_n12': (13, 0.1, 12, None, False),
    # distances of ~0.1 edge lengths at coordinates of ~60: where |q|^2 + |t|^2 - 2 q.t would cancel
    'n13_on_n12_both_moved': (13, 0.1, 12, (50.0, -30.0, 20.0), True),
    # the targets alone moved: large distances
    'n13_on_n12_targets_moved': (13, 0.1, 12, (50.0, -30.0, 20.0), False),
}


def _case(name):
    from geobi_gnn_amd import meshgen
    nq, sigma, nt, shift, move_queries = _CASES[name]
    q = meshgen.noisy_icosphere(nq, sigma, seed=3)[0].astype(np.float64)
    verts, faces = meshgen.icosphere(nt)
    verts = np.asarray(verts, dtype=np.float64)
    faces = np.asarray(faces)
    e = _mean_edge(verts, faces)
    if shift is not None:
        verts = verts + np.asarray(shift) * e
        if move_queries:
            q = q + np.asarray(shift) * e
    q32, v32 = q.astype(np.float32), verts.astype(np.float32)      # the fp64 statements start from the same float32 inputs
    return q32, v32, faces, _mean_edge(v32, faces)


@pytest.mark.parametrize('name', sorted(_CASES))
def test_accuracy_and_index_against_fp64(dev, name):
    """|d_gpu - d_fp64| / (d_fp64 + e) <= 1e-5 for every query, e = the target's mean edge length, for the
    nearest-vertex and the point-to-surface distance; the fp64 distance to the RETURNED target is within the same bar
    of the fp64 minimum (the inputs hold exact ties, so the index itself is not compared)."""
    from geobi_gnn_amd import mesheval
    q, verts, faces, e = _case(name)
    d_ref = _nearest_fp64(q, verts)
    s_ref = _surface_fp64(q, verts, faces)
    d, idx = mesheval.nearest_point(_t(q, dev), _t(verts, dev))
    s, face = mesheval.point_to_mesh(_t(q, dev), _t(verts, dev), _t(faces, dev, torch.int32))
    d, idx, s, face = d.cpu().numpy(), idx.cpu().numpy(), s.cpu().numpy(), face.cpu().numpy()
    print('%s: mean nearest-vertex %.4f e, mean surface %.4f e' % (name, d_ref.mean() / e, s_ref.mean() / e))
    print('%s: rel err nearest-vertex %.3e, surface %.3e' % (name, _rel(d, d_ref, e), _rel(s, s_ref, e)))
    assert d.dtype == np.float32 and idx.dtype == np.int32 and face.dtype == np.int32
    assert idx.min() >= 0 and idx.max() < verts.shape[0] and face.min() >= 0 and face.max() < faces.shape[0]
    d_at = np.linalg.norm(q.astype(np.float64) - verts.astype(np.float64)[idx], axis=1)
    f = faces[face]
    s_at = _tri_dist_fp64(q, verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]])
    print('%s: rel err at returned index %.3e, at returned face %.3e' % (name, _rel(d_at, d_ref, e), _rel(s_at, s_ref, e)))
    assert _rel(d, d_ref, e) <= TOL
    assert _rel(s, s_ref, e) <= TOL
    assert _rel(d_at, d_ref, e) <= TOL
    assert _rel(s_at, s_ref, e) <= TOL


def test_ties_go_to_the_lowest_index_and_order_does_not_matter(dev):
    from geobi_gnn_amd import mesheval
    q, verts, faces, _ = _case('n13_on_n12')
    qd, td, fd = _t(q, dev), _t(verts, dev), _t(faces, dev, torch.int32)
    T, F = verts.shape[0], faces.shape[0]
    d0, i0 = mesheval.nearest_point(qd, td)
    d1, i1 = mesheval.nearest_point(qd, torch.cat([td, td]))
    assert torch.equal(d0, d1) and torch.equal(i0, i1) and int(i1.max()) < T
    s0, f0 = mesheval.point_to_mesh(qd, td, fd)
    s1, f1 = mesheval.point_to_mesh(qd, td, torch.cat([fd, fd]))
    assert torch.equal(s0, s1) and torch.equal(f0, f1) and int(f1.max()) < F
    perm = torch.from_numpy(np.random.default_rng(7).permutation(T)).to(dev)
    d2, i2 = mesheval.nearest_point(qd, td[perm].contiguous())
    assert torch.equal(d0, d2)
    assert int(i2.min()) >= 0 and int(i2.max()) < T
    fperm = torch.from_numpy(np.random.default_rng(8).permutation(F)).to(dev)
    s2, _ = mesheval.point_to_mesh(qd, td, fd[fperm].contiguous())
    assert torch.equal(s0, s2)


def test_results_do_not_depend_on_the_slice_count(dev):
    """The library cuts the targets into more slices for a small query set than for a large one; a query's distance
    and index must be the same bits either way."""
    from geobi_gnn_amd import _lib as L, mesheval, meshgen
    noisy, clean, faces = meshgen.noisy_icosphere(64, 0.2, seed=5)           # V = 40 962, F = 81 920
    qd, td, fd = _t(noisy, dev), _t(clean, dev), _t(faces, dev, torch.int32)
    V, F = clean.shape[0], faces.shape[0]
    lib = L.lib()
    d_all, i_all = mesheval.nearest_point(qd, td)
    s_all, f_all = mesheval.point_to_mesh(qd, td, fd)
    seen_p, seen_t = {lib.geobi_nearest_slices(V, V, 0)}, {lib.geobi_nearest_slices(V, F, 1)}
    for n in (1, 63, 1000, 5000):
        seen_p.add(lib.geobi_nearest_slices(n, V, 0))
        seen_t.add(lib.geobi_nearest_slices(n, F, 1))
        d, i = mesheval.nearest_point(qd[:n].contiguous(), td)
        s, f = mesheval.point_to_mesh(qd[:n].contiguous(), td, fd)
        assert torch.equal(d, d_all[:n]) and torch.equal(i, i_all[:n])
        assert torch.equal(s, s_all[:n]) and torch.equal(f, f_all[:n])
    print('slice counts: points %s, triangles %s' % (sorted(seen_p), sorted(seen_t)))
    assert len(seen_p) >= 2 and len(seen_t) >= 2


def test_edge_sizes_and_a_triangle_without_area(dev):
    from geobi_gnn_amd import mesheval
    q, verts, faces, e = _case('n9_on_n8')
    qd, td, fd = _t(q, dev), _t(verts, dev), _t(faces, dev, torch.int32)
    # Q = 1 and T = 1
    d, i = mesheval.nearest_point(qd[:1].contiguous(), td[5:6].contiguous())
    ref = np.linalg.norm(q[0].astype(np.float64) - verts[5])
    assert int(i[0]) == 0 and abs(float(d[0]) - ref) <= TOL * (ref + e)
    s, f = mesheval.point_to_mesh(qd[:1].contiguous(), td, fd[7:8].contiguous())
    ref = _tri_dist_fp64(q[0], verts[faces[7, 0]], verts[faces[7, 1]], verts[faces[7, 2]])
    assert int(f[0]) == 0 and abs(float(s[0]) - ref) <= TOL * (ref + e)
    # Q = 812 is no multiple of 64, T = 1500 (points) / 300 (triangles) no multiple of the tiles
    rng = np.random.default_rng(1)
    t2 = rng.standard_normal((1500, 3)).astype(np.float32)
    d, _ = mesheval.nearest_point(qd, _t(t2, dev))
    assert _rel(d.cpu().numpy(), _nearest_fp64(q, t2), e) <= TOL
    s, _ = mesheval.point_to_mesh(qd, td, fd[:300].contiguous())
    assert _rel(s.cpu().numpy(), _surface_fp64(q, verts, faces[:300]), e) <= TOL
    # triangles without area: three collinear corners (the longest edge is each of the three in turn), two equal
    # corners, three equal corners -- finite, and the fp64 point-segment distance
    a, b = np.array([0.25, -0.5, 0.75]), np.array([1.25, 0.5, -0.25])
    m = 0.5 * (a + b)                                        # exactly representable midpoint
    dv = np.stack([a, b, m]).astype(np.float32)
    qq = (rng.standard_normal((500, 3)) * 1.5).astype(np.float32)
    for tri, seg in (((0, 1, 2), (a, b)), ((0, 2, 1), (a, b)), ((2, 0, 1), (a, b)), ((0, 0, 1), (a, b)),
                     ((0, 1, 1), (a, b)), ((2, 2, 2), (m, m))):
        s, f = mesheval.point_to_mesh(_t(qq, dev), _t(dv, dev), _t(np.array([tri]), dev, torch.int32))
        s = s.cpu().numpy()
        assert np.isfinite(s).all()
        ref = _segment_dist_fp64(qq, seg[0], seg[1]) if seg[0] is not seg[1] else np.linalg.norm(qq.astype(np.float64) - m, axis=1)
        assert _rel(s, ref, float(np.linalg.norm(b - a))) <= TOL, tri


def test_properties(dev):
    from geobi_gnn_amd import mesheval
    q, verts, faces, e = _case('n13_on_n12')
    qd, td, fd = _t(q, dev), _t(verts, dev), _t(faces, dev, torch.int32)
    d, _ = mesheval.nearest_point(qd, td)
    s, _ = mesheval.point_to_mesh(qd, td, fd)
    assert bool((s <= d + TOL * e).all())                     # the vertices are part of the surface
    # a query AT a target vertex: exactly 0.0 from both
    d, i = mesheval.nearest_point(td, td)
    assert bool((d == 0).all()) and torch.equal(i.long(), torch.arange(verts.shape[0], device=dev))
    s, _ = mesheval.point_to_mesh(td, td, fd)
    assert bool((s == 0).all())
    # sum / max in fp64
    x = torch.cat([d, s, mesheval.nearest_point(qd, td)[0]] * 7)
    got = mesheval.dist_summary(x).cpu().numpy()
    ref = x.cpu().numpy().astype(np.float64)
    assert abs(got[0] - ref.sum()) <= 1e-12 * ref.sum() and got[1] == ref.max()
    one = mesheval.dist_summary(x[-1:].contiguous()).cpu().numpy()
    assert one[0] == float(x[-1]) and one[1] == float(x[-1])


# ------------------------------------------------------------------ the edges of the shared all-pairs walk
# Points: integer lattice coordinates in [-9, 9], so every squared distance (<= 3 * 18^2 = 972) is exact in fp32 and the
# reference is int64 numpy, whose arg-min is the lowest index.  Q sits around one query block (256 lanes x 4), T around
# one tile (512); (1025, 513) and (1025, 1025) are cut into 2 and 3 slices.
_WALK_Q, _WALK_T = (1, 1023, 1024, 1025), (1, 511, 512, 513, 1025)
_LATTICE = {}


def _lattice():
    """q, t [1025, 3] and the int64 squared distances of all pairs; a case takes the first Q / T rows."""
    if not _LATTICE:
        rng = np.random.default_rng(23)
        q = rng.integers(-9, 10, (1025, 3))
        t = rng.integers(-9, 10, (1025, 3))
        _LATTICE['qtd'] = (q.astype(np.float32), t.astype(np.float32), ((q[:, None, :] - t[None, :, :]) ** 2).sum(2))
    return _LATTICE['qtd']


@pytest.mark.parametrize('T', _WALK_T)
@pytest.mark.parametrize('Q', _WALK_Q)
def test_point_walk_edges_are_bit_exact(dev, Q, T):
    """nearest_parts with one part, the same rows as the second of two parts (behind a 7-row first part: q_begin and
    t_begin are not 0) and nearest_point: the index and d2 are the int64 statement's, bit for bit."""
    from geobi_gnn_amd import mesheval, ops
    q, t, d_all = _lattice()
    q, t, d = q[:Q], t[:T], d_all[:Q, :T]
    ref_idx, ref_d2 = d.argmin(1), d.min(1).astype(np.float32)
    ties = float(((d == d.min(1, keepdims=True)).sum(1) > 1).mean())
    slices = ops.nearest_parts_slices([0, Q], [0, T])
    print('Q = %d, T = %d: %d slices, %.0f %% of the queries have several equally near targets' % (Q, T, slices, 100 * ties))
    if T >= 511 and Q > 1:
        assert ties > 0.2                                     # the tie rule is exercised
    if Q == 1025 and T >= 513:
        assert slices == (2 if T == 513 else 3)               # and so is the slice reduction
    qd, td = _t(q, dev), _t(t, dev)
    d2, idx = ops.nearest_parts(qd, td)
    assert np.array_equal(idx.cpu().numpy(), ref_idx) and np.array_equal(d2.cpu().numpy(), ref_d2)
    head_q, head_t = _lattice()[0][500:507], _lattice()[1][600:607]
    d2, idx = ops.nearest_parts(_t(np.concatenate([head_q, q]), dev), _t(np.concatenate([head_t, t]), dev), [0, 7, 7 + Q],
                                [0, 7, 7 + T])
    assert np.array_equal(idx.cpu().numpy()[7:], ref_idx + 7) and np.array_equal(d2.cpu().numpy()[7:], ref_d2)
    assert int(idx[:7].min()) >= 0 and int(idx[:7].max()) < 7
    dist, idx = mesheval.nearest_point(qd, td)
    assert np.array_equal(idx.cpu().numpy(), ref_idx)
    ref = np.sqrt(d.min(1).astype(np.float64))
    assert (np.abs(dist.cpu().numpy().astype(np.float64) - ref) <= TOL * ref).all()


_SPHERE8 = {}


def _sphere8():
    """The frequency-8 icosphere (V = 642, F = 1280) and its noisy vertices as queries; fp64 surface distances per F'."""
    if not _SPHERE8:
        from geobi_gnn_amd import meshgen
        noisy, clean, faces = meshgen.noisy_icosphere(8, 0.2, seed=3)
        faces = np.asarray(faces)
        _SPHERE8['mesh'] = (noisy.astype(np.float32), clean.astype(np.float32), faces, _mean_edge(clean, faces))
    return _SPHERE8['mesh']


@pytest.mark.parametrize('F', (1, 255, 256, 257, 513))
def test_triangle_walk_edges_against_fp64(dev, F):
    """Q around one query block (256 lanes x 2), F' = faces[:F'] around one tile (256): every row within TOL of the
    fp64 surface distance, and so is the fp64 distance to the returned face."""
    from geobi_gnn_amd import mesheval
    q_all, verts, faces, e = _sphere8()
    assert verts.shape[0] == 642 and faces.shape[0] == 1280
    s_ref_all = _surface_fp64(q_all[:513], verts, faces[:F])          # once per F', shared by the four Q
    td, fd = _t(verts, dev), _t(faces[:F], dev, torch.int32)
    for Q in (1, 511, 512, 513):
        q, s_ref = q_all[:Q], s_ref_all[:Q]
        s, face = mesheval.point_to_mesh(_t(q, dev), td, fd)
        s, face = s.cpu().numpy(), face.cpu().numpy()
        assert s.shape == (Q,) and face.min() >= 0 and face.max() < F
        f = faces[face]
        s_at = _tri_dist_fp64(q, verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]])
        print('Q = %d, F = %d: rel err %.3e, at the returned face %.3e' % (Q, F, _rel(s, s_ref, e), _rel(s_at, s_ref, e)))
        assert _rel(s, s_ref, e) <= TOL
        assert _rel(s_at, s_ref, e) <= TOL


def _summary_vector(n=100000):
    """Fixed fp32 values over 2^-21 .. 2^21.  Their fp64 sum rounds at almost every addition (numpy's pairwise sum differs
    from the kernel's order in the last bit), so the two doubles of tests/golden/dist_summary_100k.npz pin the tree shape
    and the block order of the sum.  PROVENANCE: the file holds a numpy fp64 replay of the kernel's order (98 blocks,
    thread-strided sums, the 256-lane tree, blocks ascending); a run of the build before the shared helpers on an
    MI355X, which is where the value should come from, has not been possible yet."""
    i = np.arange(n, dtype=np.int64)
    u = ((i * 2654435761) % 1000003).astype(np.float32) / np.float32(1000003)
    return (u + np.float32(0.5)) * np.exp2(((i % 41) - 20).astype(np.float32))


@pytest.mark.parametrize('n', (1, 255, 256, 257, 1025))
def test_fixed_order_sums_at_the_block_edges(dev, n):
    """dist_summary and the Chamfer forward on n rows, around one block of 256 and its grid of cdiv(n, 1024) blocks."""
    from chamfer_model import _cd64
    from geobi_gnn_amd import mesheval, ops
    x = _summary_vector()[:n]
    got = mesheval.dist_summary(_t(x, dev)).cpu().numpy()
    ref = x.astype(np.float64)
    assert abs(got[0] - ref.sum()) <= 1e-12 * ref.sum() and got[1] == ref.max()
    q, verts, _, _ = _case('n13_on_n12')
    q, t = q[:n], verts[:n]
    cd = float(ops.chamfer_loss(_t(q, dev), _t(t, dev)))
    ref_cd, _ = _cd64(q, t)
    print('n = %d: CD %.9g (fp64 %.9g)' % (n, cd, ref_cd))
    assert abs(cd - ref_cd) <= TOL * abs(ref_cd)


def test_dist_summary_keeps_its_recorded_bits(dev):
    from geobi_gnn_amd import mesheval
    x = _summary_vector()
    got = mesheval.dist_summary(_t(x, dev)).cpu().numpy()
    want = np.load(os.path.join(ROOT, 'tests', 'golden', 'dist_summary_100k.npz'))['summary']
    ref = x.astype(np.float64)
    assert abs(got[0] - ref.sum()) <= 1e-12 * ref.sum() and got[1] == ref.max()
    assert got.dtype == np.float64 and np.array_equal(got, want), (got[0].hex(), want[0].hex())


def _eval_fp64(pr, po, faces):
    """code/data_util.py:591-611 in fp64 from the float32 inputs (+ surface distance and Hausdorff)."""
    pr, po = pr.astype(np.float64), po.astype(np.float64)

    def normals(p):
        n = np.cross(p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]])
        return n / np.linalg.norm(n, axis=1, keepdims=True)
    nr, no = normals(pr), normals(po)
    err_face = ((nr - no) ** 2).sum(1)
    ang = np.arccos(np.clip(1 - err_face / 2, -1, 1)) * 180 / np.pi
    scale = _mean_edge(po, faces)
    d = _nearest_fp64(pr, po)
    return {'num_f': faces.shape[0], 'err_face': err_face.mean(), 'angle': ang.mean(), 'num_v': pr.shape[0],
            'err_v': d.mean(), 'err_v_norm': d.mean() / scale, 'surf': _surface_fp64(pr, po, faces).mean(),
            'surf_norm': _surface_fp64(pr, po, faces).mean() / scale,
            'hausdorff': max(d.max(), _nearest_fp64(po, pr).max()), 'scale': scale}


def test_eval_pair_against_fp64(dev):
    from geobi_gnn_amd import mesheval, meshgen, network
    from geobi_gnn_amd.data_util import computer_face_normal
    noisy, clean, faces = meshgen.noisy_icosphere(12, 0.2, seed=2)
    got = mesheval.eval_pair(noisy, faces, clean, device=dev)
    ref = _eval_fp64(noisy, clean, faces)
    assert got['num_f'] == ref['num_f'] and got['num_v'] == ref['num_v']
    for k in ('err_face', 'angle', 'err_v', 'err_v_norm', 'surf', 'surf_norm', 'hausdorff', 'scale'):
        print('%s: %.9g (fp64 %.9g)' % (k, got[k], ref[k]))
        assert abs(got[k] - ref[k]) <= TOL * abs(ref[k]), k
    fd = _t(faces, dev, torch.int32)
    angle = network.error_n(computer_face_normal(_t(noisy, dev), fd), computer_face_normal(_t(clean, dev), fd))
    assert got['angle'] == float(angle)
    with pytest.raises(ValueError):
        mesheval.eval_pair(noisy[:-1], faces[:-5], clean, device=dev)


def test_denoise_and_eval_commands_end_to_end(dev, tmp_path):
    """python -m geobi_gnn_amd denoise on original/ico.obj + noisy/ico_n1.obj, ico_n2.obj, then eval: the written
    vertices are predict_mesh's bit for bit, the printed angles are predict_mesh's, ErrorInfo_h.txt holds eval_pair's
    numbers.  Each command is ONE child process; the second starts only after the first returned 0."""
    from geobi_gnn_amd import mesheval, meshgen, meshio, network, patches
    (tmp_path / 'original').mkdir()
    (tmp_path / 'noisy').mkdir()
    meshes = {}
    for k, sigma in ((1, 0.1), (2, 0.3)):
        noisy, clean, faces = meshgen.noisy_icosphere(8, sigma, seed=40 + k)
        meshes['ico_n%d' % k] = (noisy, clean, faces)
        meshio.write_obj(str(tmp_path / 'noisy' / ('ico_n%d.obj' % k)), noisy, faces)
    meshio.write_obj(str(tmp_path / 'original' / 'ico.obj'), clean, faces)
    torch.manual_seed(5)
    net = network.DualGNN()
    model = str(tmp_path / 'net.pt')
    torch.save(net.state_dict(), model)
    out_dir = tmp_path / 'out'
    run = subprocess.run([sys.executable, '-m', 'geobi_gnn_amd', 'denoise', '--model', model, '--data_dir', str(tmp_path),
                          '--out_dir', str(out_dir)], cwd=ROOT, timeout=300, capture_output=True, text=True)
    print(run.stdout)
    print(run.stderr)
    assert run.returncode == 0, run.stderr[-2000:]
    net = net.to(dev).eval()
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith('angle1:')]
    assert len(lines) == 2
    faces_total, sums = 0, np.zeros(2)
    for ln, name in zip(lines, sorted(meshes)):
        noisy, clean, faces = meshes[name]
        path = out_dir / (name + '-60.obj')
        assert path.exists() and ("'%s-60.obj'" % name) in ln
        pts, fv = meshio.read_obj(str(path))
        assert np.array_equal(fv, faces.astype(np.int32))
        with torch.no_grad():
            r = patches.predict_mesh(net, noisy, faces, sub_size=20000, n_iter=60, gt_points=clean, distributed=False)
        want = r['V_updated'].cpu().numpy()
        assert np.array_equal(pts.view(np.uint32), want.view(np.uint32))
        assert ln.startswith('angle1: %9.6f,  angle2: %9.6f,  faces: %6d,' % (r['angle1'], r['angle2'], faces.shape[0]))
        faces_total += faces.shape[0]
        sums += faces.shape[0] * np.array([r['angle1'], r['angle2']])
    assert ('Num_face: %6d,  angle_mean1: %.6f,  angle_mean2: %.6f' % (faces_total, sums[0] / faces_total,
                                                                     sums[1] / faces_total)) in run.stdout

    run = subprocess.run([sys.executable, '-m', 'geobi_gnn_amd', 'eval', '--result_dir', str(out_dir), '--original_dir',
                          str(tmp_path / 'original')], cwd=ROOT, timeout=300, capture_output=True, text=True)
    print(run.stdout)
    print(run.stderr)
    assert run.returncode == 0, run.stderr[-2000:]
    info = out_dir / 'ErrorInfo_h.txt'
    assert info.exists()
    rows = [ln.split() for ln in info.read_text().splitlines() if ln.strip()]
    assert len(rows) == 4 and rows[0][0] == 'Error_rst:'
    keys = ('num_f', 'err_face', 'angle', 'num_v', 'err_v', 'err_v_norm', 'surf', 'surf_norm', 'hausdorff')
    want_rows = []
    for row, name in zip(rows[2:], sorted(meshes)):
        assert row[0] == name + '-60.obj' and len(row) == 10
        pts, fv = meshio.read_obj(str(out_dir / row[0]))
        want = mesheval.eval_pair(pts, fv, clean, device=dev)
        want_rows.append(want)
        for k, tok in zip(keys, row[1:]):
            assert abs(float(tok) - want[k]) <= 0.51e-6, (k, tok, want[k])
    tot = mesheval.totals(want_rows)
    assert len(rows[1]) == 9
    for k, tok in zip(keys, rows[1]):
        assert abs(float(tok) - tot[k]) <= 0.51e-4, (k, tok, tot[k])


def test_denoise_skips_a_bad_file_and_goes_on(dev, tmp_path):
    """A folder without original/ and noisy/: every *.obj, no ground truth.  A file with a vertex that no face
    references is reported (file and count) and skipped, the other file is still denoised, the exit status is non-zero.
    One child process."""
    from geobi_gnn_amd import meshgen, meshio
    noisy, _, faces = meshgen.noisy_icosphere(6, 0.2, seed=4)
    meshio.write_obj(str(tmp_path / 'good.obj'), noisy, faces)
    meshio.write_obj(str(tmp_path / 'loose.obj'), np.concatenate([noisy, [[9.0, 9.0, 9.0]]]).astype(np.float32), faces)
    run = subprocess.run([sys.executable, '-m', 'geobi_gnn_amd', 'denoise', '--data_dir', str(tmp_path), '--n_iter', '10'],
                         cwd=ROOT, timeout=300, capture_output=True, text=True)
    print(run.stdout)
    print(run.stderr)
    assert run.returncode == 1
    assert 'loose.obj' in run.stderr and '1 of %d vertices' % (noisy.shape[0] + 1) in run.stderr
    assert (tmp_path / 'result' / 'good-10.obj').exists() and not (tmp_path / 'result' / 'loose-10.obj').exists()
    pts, fv = meshio.read_obj(str(tmp_path / 'result' / 'good-10.obj'))
    assert pts.shape == noisy.shape and np.isfinite(pts).all() and np.array_equal(fv, faces.astype(np.int32))
    assert "angle1:  0.000000,  angle2:  0.000000,  faces: %6d," % faces.shape[0] in run.stdout


def test_bad_arguments_raise(dev):
    from geobi_gnn_amd import mesheval
    from geobi_gnn_amd._lib import GeobiError
    q, verts, faces, _ = _case('n9_on_n8')
    qd, td, fd = _t(q, dev), _t(verts, dev), _t(faces, dev, torch.int32)
    with pytest.raises(GeobiError):
        mesheval.nearest_point(torch.from_numpy(q), td)
    with pytest.raises(GeobiError):
        mesheval.nearest_point(qd, torch.from_numpy(verts))
    with pytest.raises(GeobiError):
        mesheval.point_to_mesh(torch.from_numpy(q), td, fd)
    with pytest.raises(GeobiError):
        mesheval.point_to_mesh(qd, td, torch.from_numpy(faces))
    with pytest.raises(GeobiError):
        mesheval.nearest_point(qd, td[:0].contiguous())
    with pytest.raises(GeobiError):
        mesheval.point_to_mesh(qd, td, fd[:0].contiguous())
    bad = fd.clone()
    bad[3, 1] = verts.shape[0]
    with pytest.raises(GeobiError, match='outside'):
        mesheval.point_to_mesh(qd, td, bad)
    bad[3, 1] = -1
    with pytest.raises(GeobiError, match='outside'):
        mesheval.point_to_mesh(qd, td, bad)
    # an int64 id that the conversion to int32 would wrap into range (2^32 + 1 -> 1) is refused as it arrives
    p4 = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], dtype=np.float32)
    wrap = np.array([[0, 1, 2], [1, 2, 2 ** 32 + 1]], dtype=np.int64)
    with pytest.raises(GeobiError, match='outside'):
        mesheval.point_to_mesh(qd, _t(p4, dev), torch.from_numpy(wrap).to(dev))
    with pytest.raises(GeobiError, match='outside'):
        mesheval.eval_pair(p4, wrap, p4, device=dev)
    with pytest.raises(GeobiError, match='outside'):
        mesheval.eval_pair(p4, [[0, 1, 2], [1, 2, 3]], p4, gt_faces=wrap, device=dev)
