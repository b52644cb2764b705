"""The fp64 preprocessing model of tests/meshprep_model.py on the host: pinned to the reference project's own numbers
(tests/golden/pure_functions.npz), compared with the host generator where that is adequate (a unit icosphere), hand-computed
cases, and the mesh family of tests/test_gpu_meshprep_edges.py (counts, symmetry, cancelling vertices).  No device."""
import numpy as np
import pytest

import meshprep_model as M
from helpers import load_fixture


def _strip_loops_sorted(ei, w=None):
    ei = np.asarray(ei).astype(np.int64)
    keep = ei[0] != ei[1]
    r, c = ei[0][keep], ei[1][keep]
    order = np.argsort(r * (int(ei.max()) + 1) + c, kind='stable')
    return (r[order], c[order]) if w is None else (r[order], c[order], np.asarray(w)[keep][order])


def _is_symmetric(n, row, col):
    return np.array_equal(np.sort(row * n + col), np.sort(col * n + row))


# ------------------------------------------------------------------------------------------------ the reference's numbers
def test_pinned_by_the_reference():
    fx = load_fixture('pure_functions.npz')
    pts, faces = fx['points'], fx['faces']
    V = pts.shape[0]
    rowptr, lst = M.vertex_faces(faces, V)
    assert np.array_equal(M.vf_padded(rowptr, lst), fx['vf'].astype(np.int64))
    np.testing.assert_allclose(M.face_normals(pts, faces), fx['face_normal'], rtol=0, atol=2e-6)   # fp32 torch on their side
    vn, norm = M.vertex_normals(pts, faces)
    assert norm.min() > 1.0
    np.testing.assert_allclose(vn, fx['vnormal'], rtol=0, atol=2e-6)
    _, row, col = M.ring_graph(0, faces, V)
    r, c, w = _strip_loops_sorted(fx['edge_index'], fx['calc_weight'])
    assert np.array_equal(row, r) and np.array_equal(col, c)
    got = M.calc_weight(pts, fx['vnormal'], row, col, extra=V)                   # their edge list holds V self loops
    np.testing.assert_allclose(got.w, w, rtol=3e-6, atol=0)
    _, frow, fcol = M.ring_graph(1, faces, V)
    r, c = _strip_loops_sorted(fx['facet_graph_index'])
    assert np.array_equal(frow, r) and np.array_equal(fcol, c)
    assert abs(1.0 / M.mean_edge_length(pts, row, col) - float(fx['scale'])) <= 2e-6 * float(fx['scale'])


def test_matches_host_generator_on_an_icosphere():
    from geobi_gnn_amd import meshgen
    noisy, clean, faces = meshgen.noisy_icosphere(5, 0.2, seed=5)
    ref_v, ref_f = meshgen.build_dual_data(noisy, faces)
    V = noisy.shape[0]
    rowptr, lst = M.vertex_faces(faces, V)
    assert np.array_equal(M.vf_padded(rowptr, lst), ref_v.meta['vf_indices'].numpy())
    fn, (vn, _) = M.face_normals(noisy, faces), M.vertex_normals(noisy, faces)
    np.testing.assert_allclose(ref_f.x[:, 3:].numpy(), fn, rtol=0, atol=2.0 ** -23)
    np.testing.assert_allclose(ref_v.x[:, 3:].numpy(), vn, rtol=0, atol=2.0 ** -23)
    for kind, ref, pos, nrm in ((0, ref_v, noisy, ref_v.x[:, 3:].numpy()),
                                (1, ref_f, M.centroids(noisy, faces).astype(np.float32), ref_f.x[:, 3:].numpy())):
        rp, row, col = M.ring_graph(kind, faces, V)
        r, c, w = _strip_loops_sorted(ref.edge_index.numpy(), ref.edge_weight.numpy())
        assert np.array_equal(row, r) and np.array_equal(col, c) and rp[-1] == r.shape[0]
        np.testing.assert_allclose(M.calc_weight(pos, nrm, row, col, extra=rp.shape[0] - 1).w, w, rtol=3e-6, atol=0)
    _, row, col = M.ring_graph(0, faces, V)
    assert abs(1.0 / M.mean_edge_length(noisy, row, col) - ref_v.meta['scale']) <= 2e-6 * ref_v.meta['scale']


# ------------------------------------------------------------------------------------------------ hand cases
def test_one_triangle():
    pts, faces = [[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]]
    rowptr, lst = M.vertex_faces(faces, 3)
    assert rowptr.tolist() == [0, 1, 2, 3] and lst.tolist() == [0, 0, 0]
    assert M.vf_padded(rowptr, lst).tolist() == [[0], [0], [0]] and M.max_degree(rowptr) == 1
    assert M.face_normals(pts, faces).tolist() == [[0, 0, 1]]
    np.testing.assert_allclose(M.centroids(pts, faces), [[1 / 3, 1 / 3, 0]], rtol=1e-15)
    vn, norm = M.vertex_normals(pts, faces)
    assert vn.tolist() == [[0, 0, 1]] * 3 and norm.tolist() == [1, 1, 1]
    rp, row, col = M.ring_graph(0, faces, 3)
    assert rp.tolist() == [0, 2, 4, 6] and row.tolist() == [0, 0, 1, 1, 2, 2] and col.tolist() == [1, 2, 0, 2, 0, 1]
    rp, row_f, col_f = M.ring_graph(1, faces, 3)
    assert rp.tolist() == [0, 0] and row_f.size == 0 and col_f.size == 0
    total = 2 * (2 + np.sqrt(2))
    assert abs(M.mean_edge_length(pts, row, col) - total / 6) < 1e-15
    mean = total / 9                                                       # three zero-length loops join the mean
    w = M.calc_weight(pts, vn, row, col, extra=3)
    assert abs(w.mean - mean) < 1e-15 and w.dn.tolist() == [1] * 6
    np.testing.assert_allclose(w.w, np.exp(-np.array([1, 1, 1, 2, 1, 2]) / (2 * mean - 1e-12)), rtol=1e-14)
    empty = M.calc_weight(M.centroids(pts, faces), [[0, 0, 1]], row_f, col_f, extra=1)
    assert empty.w.size == 0 and empty.mean == 0.0
    assert M.mean_edge_length(pts, row_f, col_f, 0) == 0.0                 # max(E + extra, 1)


def test_tetrahedron():
    pts = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64)
    faces = [[1, 3, 2], [0, 2, 3], [0, 3, 1], [0, 1, 2]]                   # face k is opposite to vertex k, outward
    rowptr, lst = M.vertex_faces(faces, 4)
    assert M.vf_padded(rowptr, lst).tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]
    fn = M.face_normals(pts, faces)
    np.testing.assert_allclose(fn, -pts / np.sqrt(3), atol=1e-15)
    np.testing.assert_allclose(M.centroids(pts, faces), -pts / 3, atol=1e-15)
    vn, norm = M.vertex_normals(pts, faces)
    np.testing.assert_allclose(vn, pts / np.sqrt(3), atol=1e-15)
    np.testing.assert_allclose(norm, 1.0, atol=1e-15)                      # |n_a + n_b + n_c| = |-n_d| = 1
    full = [[b for b in range(4) if b != a] for a in range(4)]
    for kind in (0, 1):
        rp, row, col = M.ring_graph(kind, faces, 4)
        assert rp.tolist() == [0, 3, 6, 9, 12] and col.reshape(4, 3).tolist() == full
    w = M.calc_weight(pts, vn, row, col, extra=4)                          # as a vertex graph: edges 2 sqrt 2, n.n = -1/3
    mean = 12 * 2 * np.sqrt(2) / 16
    np.testing.assert_allclose(w.w, 1e-3 * np.exp(8 / (-2 * mean + 1e-12)), rtol=1e-14)
    wf = M.calc_weight(M.centroids(pts, faces), fn, row, col, extra=4)     # as the facet graph: a third of that
    np.testing.assert_allclose(wf.w, 1e-3 * np.exp((8 / 9) / (-2 * mean / 3 + 1e-12)), rtol=1e-6)   # thirds rounded to fp32
    np.testing.assert_allclose(wf.arg, (8 / 9) / (-2 * mean / 3), rtol=1e-6)


def test_bow_tie():
    pts = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [-1, 0, 0], [-1, -1, 1]]
    faces = [[0, 1, 2], [0, 3, 4]]
    rowptr, lst = M.vertex_faces(faces, 5)
    assert rowptr.tolist() == [0, 2, 3, 4, 5, 6] and lst.tolist() == [0, 1, 0, 0, 1, 1]
    assert M.vf_padded(rowptr, lst).tolist() == [[0, 1], [0, -1], [0, -1], [1, -1], [1, -1]]
    rp, row, col = M.ring_graph(0, faces, 5)
    assert rp.tolist() == [0, 4, 6, 8, 10, 12]
    assert col.tolist() == [1, 2, 3, 4, 0, 2, 0, 1, 0, 4, 0, 3]
    rp, row, col = M.ring_graph(1, faces, 5)
    assert rp.tolist() == [0, 1, 2] and row.tolist() == [0, 1] and col.tolist() == [1, 0]
    fn = M.face_normals(pts, faces)
    np.testing.assert_allclose(fn, [[0, 0, 1], [0, np.sqrt(0.5), np.sqrt(0.5)]], atol=1e-15)
    vn, norm = M.vertex_normals(pts, faces)
    np.testing.assert_allclose(norm[0], np.sqrt(2 + np.sqrt(2)), rtol=1e-15)
    np.testing.assert_allclose(vn[0], (fn[0] + fn[1]) / norm[0], atol=1e-15)


def test_face_with_its_reversed_copy():
    pts, faces = [[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2], [0, 2, 1]]
    rowptr, lst = M.vertex_faces(faces, 3)
    assert M.vf_padded(rowptr, lst).tolist() == [[0, 1]] * 3
    fn = M.face_normals(pts, faces)
    assert fn.tolist() == [[0, 0, 1], [0, 0, -1]]
    vn, norm = M.vertex_normals(pts, faces)
    assert norm.tolist() == [0, 0, 0] and not vn.any()
    rp, row, col = M.ring_graph(0, faces, 3)
    assert rp.tolist() == [0, 2, 4, 6]
    rp, row, col = M.ring_graph(1, faces, 3)
    assert row.tolist() == [0, 1] and col.tolist() == [1, 0]
    w = M.calc_weight(M.centroids(pts, faces), fn, row, col, extra=2)      # same centroid, opposite normals: the clamp
    assert w.w.tolist() == [1e-3, 1e-3] and w.arg.tolist() == [0, 0]
    same = M.vertex_faces([[0, 1, 2], [0, 1, 2]], 3)                       # a duplicated face sits under both of its ids
    assert same[1].tolist() == [0, 1] * 3


def test_parts_take_their_own_mean():
    a, b = M.bowtie(), M.unit_grid(20.0)
    parts, ptr, pos, nrm, rps, rows, cols, off, eoff = [], [0], [], [], [], [], [], 0, 0
    for m in (a, None, b):
        if m is not None:
            rp, row, col = M.ring_graph(0, m.faces, m.V)
            vn = M.vertex_normals(m.points, m.faces)[0].astype(np.float32)
            parts.append(M.calc_weight(m.points, vn, row, col, extra=m.V))
            pos.append(m.points); nrm.append(vn); rps.append(rp[:-1] + eoff); rows.append(row + off); cols.append(col + off)
            off, eoff = off + m.V, eoff + row.shape[0]
        ptr.append(off)
    rowptr = np.concatenate(rps + [[eoff]])
    got = M.calc_weight_parts(np.concatenate(pos), np.concatenate(nrm), rowptr, np.concatenate(rows), np.concatenate(cols), ptr)
    assert np.array_equal(got.w, np.concatenate([p.w for p in parts]))
    assert parts[0].mean != parts[1].mean


# ------------------------------------------------------------------------------------------------ the mesh family
EXPECT = {  # name: (V, F, E_v, E_f, max valence)
    'fan300': (301, 300, 1200, 300 * 299, 300),
    'bowtie': (13, 12, 48, 12 * 11, 12),
    'book': (5, 3, 14, 6, 3),
    'single': (3, 1, 6, 0, 1),
    'two_disjoint': (6, 2, 12, 0, 1),
}


@pytest.mark.parametrize('name', sorted(M.SMALL))
def test_family(name):
    m = M.SMALL[name]()
    V, F = m.V, m.F
    assert m.points.dtype == np.float32 and m.faces.dtype == np.int32 and np.isfinite(m.points).all()
    f = np.sort(m.faces, 1)
    assert m.faces.min() >= 0 and m.faces.max() < V and (f[:, 0] < f[:, 1]).all() and (f[:, 1] < f[:, 2]).all()
    rowptr, lst = M.vertex_faces(m.faces, V)
    inside = np.ones(3 * F - 1, dtype=bool)                                # lst[i] -> lst[i + 1] within one vertex's row
    inside[rowptr[(rowptr > 0) & (rowptr < 3 * F)] - 1] = False
    assert rowptr[-1] == 3 * F and (np.diff(lst)[inside] > 0).all()
    graphs = [M.ring_graph(kind, m.faces, V, rowptr, lst) for kind in (0, 1)]
    for n, (rp, row, col) in zip((V, F), graphs):
        assert _is_symmetric(n, row, col) and (row != col).all() and rp[-1] == row.shape[0]
        assert (np.diff(row * n + col) > 0).all()
    if name in EXPECT:
        assert (V, F, graphs[0][0][-1], graphs[1][0][-1], M.max_degree(rowptr)) == EXPECT[name]
    # the cancelling vertices are the ones the generator names, and only `doubled` names any
    _, norm = M.vertex_normals(m.points, m.faces, rowptr, lst)
    has_faces = np.diff(rowptr) > 0
    assert np.array_equal(np.nonzero(has_faces & (norm < 1e-3))[0], m.cancelling)
    assert (norm[has_faces & (norm >= 1e-3)] > 0.3).all()                  # nothing sits near the threshold
    assert (m.cancelling.size == 2) == (name == 'doubled') and (m.cancelling.size == 0) == (name != 'doubled')
    cross, scale = M.face_cross(m.points, m.faces)
    flat = np.sqrt((cross * cross).sum(1)) < 1e-6 * scale
    if name == 'degenerate':
        assert np.array_equal(np.nonzero(flat)[0], m.flat_faces) and not cross[flat].any()
        assert not np.cross(*(m.points[m.faces[flat][:, k]] - m.points[m.faces[flat][:, 0]] for k in (1, 2))).any()   # fp32 too
    else:
        assert not flat.any()
    if name == 'isolated':
        assert not has_faces[0] and not has_faces[18] and not has_faces[-300:].any() and has_faces.sum() == 30
    if name == 'doubled':
        pairs, counts = np.unique(np.sort(m.faces, 1), axis=0, return_counts=True)
        assert m.F == 128 + 26 + int(np.isin(m.faces[:154], m.cancelling).any(1).sum()) and counts.max() >= 2
        assert M.max_degree(rowptr) > 6
    if name == 'fan300':
        assert np.diff(graphs[1][0]).min() == 299
    if name.startswith('unit'):
        _, row, col = graphs[0]
        mean = M.mean_edge_length(m.points, row, col)
        edge = float(name[4:])
        assert 1.0 * edge < mean < 1.3 * edge
        w = M.calc_weight(m.points, M.vertex_normals(m.points, m.faces)[0].astype(np.float32), row, col, extra=V)
        if edge == 400:
            assert (w.w < 2.0 ** -149).mean() > 0.9 and w.w.max() < 1e-30   # nearly every weight underflows fp32
        if edge == 50:
            assert w.arg.min() < -40                                      # the exponent grows with the unit
    if name == 'rough':
        _, row, col = graphs[0]
        w = M.calc_weight(m.points, M.vertex_normals(m.points, m.faces)[0].astype(np.float32), row, col, extra=V)
        assert 0.05 < (w.dn == 1e-3).mean() < 0.4                          # a good share of the edges sits on the clamp
    if name.startswith('shifted'):
        base = M.unit_grid(1.0)
        assert np.array_equal(m.faces, base.faces) and np.abs(m.points).min() > 250


@pytest.mark.parametrize('key', sorted(M.SCAN_GRIDS))
def test_scan_grid_sizes(key):
    W, H = M.SCAN_GRIDS[key]
    assert W * H + 1 == {'127x129': 1 << 14, '128x128': (1 << 14) + 1, '511x513': 1 << 18, '512x512': (1 << 18) + 1}[key]
    if W > 200:
        return
    m = M.scan_grid(key)
    assert m.V == W * H and m.F == 2 * (W - 1) * (H - 1)
    rowptr, lst = M.vertex_faces(m.faces, m.V)
    assert M.max_degree(rowptr) == 6
    rp, row, col = M.ring_graph(0, m.faces, m.V, rowptr, lst)
    assert rp[-1] == 2 * ((W - 1) * H + W * (H - 1) + (W - 1) * (H - 1)) and _is_symmetric(m.V, row, col)
    rp, row, col = M.ring_graph(1, m.faces, m.V, rowptr, lst)
    assert _is_symmetric(m.F, row, col) and np.diff(rp).max() == 12
