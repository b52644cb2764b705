"""The grid in front of the nearest searches (csrc/grid.hip, geobi_gnn_amd/meshgrid.py) against the
all-pairs searches it stands in front of.  Every comparison is EXACT: the uint32 bit patterns of dist and the integers of
idx, against mesheval.nearest_point / point_to_mesh on the same tensors.  Every built table goes through the checkers of
tests/grid_model.py."""
import filecmp
import os

import numpy as np
import pytest
import torch

import grid_model as G
import project_model as P
import test_gpu_workspace as W
from train_cases import _run

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


def _t(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


def _same(got, want, name=''):
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32, name
    d = (got[0].view(torch.int32) != want[0].view(torch.int32)) | (got[1] != want[1])
    if bool(d.any()):
        k = int(torch.nonzero(d)[0])
        raise AssertionError('%s: query %d: grid (%r, %d), all pairs (%r, %d); %d rows differ'
                             % (name, k, float(got[0][k]), int(got[1][k]), float(want[0][k]), int(want[1][k]), int(d.sum())))


def _points_case(dev, targets, queries, name, cells=(None,), rings=(None, 0, 1)):
    """every (cells, max_rings) of a point case against the all-pairs call; the tables through the model -> the grids"""
    from geobi_gnn_amd import mesheval, meshgrid
    t, q = _t(targets, dev), _t(queries, dev)
    want = mesheval.nearest_point(q, t)
    grids = []
    for c in cells:
        g = meshgrid.PointGrid(t, cells=c)
        assert G.check_points(G.of_grid(g), np.asarray(targets, dtype=F32)) == [], (name, c)
        if c is not None:
            assert all(d in (1, c) for d in g.dims), (name, c, g.dims)
        for r in rings:
            _same(g.nearest(q, max_rings=r), want, '%s cells=%s max_rings=%s' % (name, c, r))
            if r == 0:
                assert g.left_over == q.shape[0]
        grids.append(g)
    _same(mesheval.nearest_point(q, t, index='grid'), want, name + " index='grid'")
    return grids


def _triangles_case(dev, verts, faces, queries, name, cells=(None,), rings=(None, 0, 1)):
    from geobi_gnn_amd import mesheval, meshgrid
    v, f, q = _t(verts, dev), _t(faces, dev, torch.int32), _t(queries, dev)
    want = mesheval.point_to_mesh(q, v, f)
    grids = []
    for c in cells:
        g = meshgrid.TriangleGrid(v, f, cells=c)
        assert G.check_triangles(G.of_grid(g), np.asarray(verts, dtype=F32), faces) == [], (name, c)
        assert g.records.shape == (f.shape[0], 16) and g.entries <= G.ENTRY_CAP * f.shape[0]
        for r in rings:
            _same(g.nearest(q, max_rings=r), want, '%s cells=%s max_rings=%s' % (name, c, r))
        grids.append(g)
    _same(mesheval.point_to_mesh(q, v, f, index='grid'), want, name + " index='grid'")
    return grids


# ---------------------------------------------------------------------------------------------- points
def test_random_points_across_the_block_edges(dev):
    rng = np.random.RandomState(0)
    targets, queries = rng.randn(257, 3).astype(F32), (1.5 * rng.randn(513, 3)).astype(F32)
    for T in (1, 2, 255, 256, 257):
        for Q in (1, 255, 256, 257, 513):
            _points_case(dev, targets[:T], queries[:Q], 'T = %d, Q = %d' % (T, Q), rings=(None,) if Q < 513 else (None, 0, 1))


def test_forced_resolutions_and_shell_budgets(dev):
    from geobi_gnn_amd import meshgrid
    rng = np.random.RandomState(1)
    targets, queries = rng.rand(257, 3).astype(F32), (rng.rand(257, 3) * 1.4 - 0.2).astype(F32)
    assert meshgrid.max_cells() == G.MAX_CELLS and meshgrid.default_rings() == G.DEFAULT_RINGS and meshgrid.entry_cap() == G.ENTRY_CAP
    one, seven, most = _points_case(dev, targets, queries, 'forced', cells=(1, 7, G.MAX_CELLS), rings=(None, 0, 1, 3))
    assert one.dims == (1, 1, 1) and seven.dims == (7, 7, 7) and most.dims == (G.MAX_CELLS,) * 3
    one.nearest(_t(queries, dev))
    assert one.left_over == 0                                # one cell IS the all-pairs walk: nothing is left over
    most.nearest(_t(queries, dev))
    assert most.left_over > 0                                # 256^3 cells for 257 points: the default budget runs out
    with pytest.raises(ValueError):
        meshgrid.PointGrid(_t(targets, dev), cells=G.MAX_CELLS + 1)
    with pytest.raises(ValueError):
        one.nearest(_t(queries, dev), max_rings=-2)


def test_lattice_ties_go_to_the_lowest_index(dev):
    """5 x 5 x 5 integer lattice; queries at cell centres (8 equally near targets), face centres (4) and edge midpoints (2),
    across the planes of the grid's cells; the same with the targets shuffled"""
    lattice = np.array([(x, y, z) for z in range(5) for y in range(5) for x in range(5)], dtype=F32)
    base = lattice[(lattice < 4).all(axis=1)]
    q = np.concatenate([base + F32(0.5)] + [base + np.array(o, dtype=F32) for o in
                                            ((0.5, 0.5, 0), (0.5, 0, 0.5), (0, 0.5, 0.5), (0.5, 0, 0), (0, 0.5, 0), (0, 0, 0.5))])
    for name, targets in (('lattice', lattice), ('shuffled', lattice[np.random.RandomState(2).permutation(125)])):
        for g in _points_case(dev, targets, q, name, cells=(None, 2, 4, 5)):
            d, i = g.nearest(_t(q, dev))
            d2 = ((q[:, None, :].astype(np.float64) - targets[None].astype(np.float64)) ** 2).sum(-1)
            assert np.array_equal(i.cpu().numpy(), d2.argmin(axis=1))            # argmin: the first of the equal minima
            ties = (d2 == d2.min(axis=1, keepdims=True)).sum(axis=1)
            assert sorted(set(ties.tolist())) == [2, 4, 8]


def test_degenerate_target_sets(dev):
    rng = np.random.RandomState(3)
    pts, q = rng.randn(128, 3).astype(F32), (2 * rng.randn(257, 3)).astype(F32)
    _points_case(dev, np.concatenate([pts, pts]), np.concatenate([q, pts]), 'every target twice', cells=(None, 3))
    _points_case(dev, np.tile(F32([[0.25, -1.5, 3.0]]), (257, 1)), q, 'one point', cells=(None, 4))
    plane = pts.copy()
    plane[:, 1] = F32(0.75)
    g = _points_case(dev, plane, q, 'a plane', cells=(None, 5))[1]
    assert g.dims == (5, 1, 5)
    line = np.zeros((200, 3), dtype=F32)
    line[:, 2] = rng.randn(200)
    g = _points_case(dev, line, q, 'a line', cells=(None, 6))[1]
    assert g.dims == (1, 1, 6)


def test_queries_on_around_and_far_from_the_box(dev):
    rng = np.random.RandomState(4)
    targets = rng.rand(257, 3).astype(F32)
    lo, hi = targets.min(axis=0), targets.max(axis=0)
    diag = float(np.linalg.norm(hi - lo))
    corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=F32)
    on_faces = rng.rand(96, 3).astype(F32) * (hi - lo) + lo
    for k in range(96):
        on_faces[k, k % 3] = (lo, hi)[(k // 3) % 2][k % 3]
    dirs = rng.randn(64, 3)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    far = np.concatenate([(0.5 + 50 * diag * dirs).astype(F32), (0.5 + 1e4 * diag * dirs).astype(F32)])
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.inf, -np.inf], [3e38, 0.5, 0.5]], dtype=F32)
    q = np.concatenate([corners, on_faces, far, bad, targets[:32]])
    g = _points_case(dev, targets, q, 'box', cells=(None, 6, 64))[0]
    d, i = g.nearest(_t(q, dev))
    n = len(corners) + len(on_faces) + len(far)
    assert torch.isinf(d[n:n + 5]).all() and not i[n:n + 5].any()              # (inf, 0), as the all-pairs search


def test_targets_that_are_not_finite(dev):
    rng = np.random.RandomState(5)
    targets, q = rng.randn(257, 3).astype(F32), (1.5 * rng.randn(257, 3)).astype(F32)
    targets[0, 0] = np.nan                                   # index 0: what a search that finds nothing answers
    targets[7] = np.inf
    targets[100, 2] = -np.inf
    targets[256, 1] = np.nan
    g = _points_case(dev, targets, q, 'some targets not finite', cells=(None, 4))[0]
    assert g.entries == g.finite == 253
    nothing = np.full((65, 3), np.nan, dtype=F32)
    nothing[1::2] = np.inf
    g = _points_case(dev, nothing, q, 'no target finite', cells=(None, 4))[0]
    assert g.entries == 0 and g.dims == (1, 1, 1)
    d, i = g.nearest(_t(q, dev))
    assert torch.isinf(d).all() and not i.any()


def test_a_set_shifted_to_ten_thousand_extents(dev):
    rng = np.random.RandomState(6)
    targets, q = rng.rand(257, 3).astype(F32), (rng.rand(257, 3) * 1.2 - 0.1).astype(F32)
    for shift in (F32([1e4, -1e4, 1e4]), F32([1e4, 0, 0])):
        grids = _points_case(dev, targets + shift, q + shift, 'shifted', cells=(None, 16))
        for g in grids:                                       # the cell edge never goes below 2^-14 of the magnitude
            assert all(d == 1 or c >= G.MIN_CELL_FRAC * g.magnitude * (1 - 1e-6) for d, c in zip(g.dims, g.cell))
        assert grids[1].dims[0] < 16


# ---------------------------------------------------------------------------------------------- triangles
def test_hand_triangle_and_triangles_without_area(dev):
    tri = np.array([[0, 1, 2]], dtype=np.int32)
    q = np.array([(x, y, z) for x, y, _, _, _ in P.hand_queries() for z in (0.0, 2.0, -3.0)], dtype=F32)
    _triangles_case(dev, P.HAND_TRIANGLE, tri, q, 'hand', cells=(None, 4))
    for name, verts in sorted(P.degenerate_triangles().items()):
        _triangles_case(dev, verts, tri, P.degenerate_queries(), name, cells=(None, 4))
    # all of them as one mesh: ties between a triangle and its copies stored as edges
    verts = np.concatenate([P.HAND_TRIANGLE] + [v for _, v in sorted(P.degenerate_triangles().items())])
    faces = np.arange(len(verts), dtype=np.int32).reshape(-1, 3)
    _triangles_case(dev, verts, faces, np.concatenate([q, P.degenerate_queries()]), 'together', cells=(None, 3, 8))


_ICO = {}


def _ico(n=4):
    from geobi_gnn_amd import meshgen
    if n not in _ICO:
        points, faces = meshgen.icosphere(n)
        ev = meshgen.mesh_edges(faces)
        _ICO[n] = (points.astype(F32), faces.astype(np.int32), float(np.linalg.norm(points[ev[:, 0]] - points[ev[:, 1]], axis=1).mean()))
    return _ICO[n]


def _big():
    """the 20 480-face icosphere, its 10 242 vertices and their noisy copies"""
    from geobi_gnn_amd import meshgen
    if 'big' not in _ICO:
        noisy, clean, faces = meshgen.noisy_icosphere(32, sigma=0.2, seed=1)
        assert faces.shape[0] == 20480 and noisy.shape[0] == 10242
        _ICO['big'] = (noisy.astype(F32), clean.astype(F32), faces.astype(np.int32))
    return _ICO['big']


def test_sphere_queries_across_the_block_edges(dev):
    points, faces, e = _ico()
    assert faces.shape[0] == 320
    q = P.shell_queries(513, seed=7)
    for shift in (np.zeros(3, dtype=F32), (np.array([50.0, -30.0, 20.0]) * e).astype(F32)):
        for Q in (1, 255, 256, 257, 513):
            _triangles_case(dev, points + shift, faces, q[:Q] + shift, 'Q = %d' % Q, rings=(None,) if Q < 513 else (None, 0, 1))


def test_long_walks_from_inside_the_sphere_take_the_fallback(dev):
    """the 20480-face sphere gets 36 cells across: from its centre the surface is 18 shells away, beyond the default budget"""
    from geobi_gnn_amd import mesheval, meshgrid
    _, clean, faces = _big()
    rng = np.random.RandomState(8)
    q = _t(np.concatenate([np.zeros((1, 3), dtype=F32), (0.05 * rng.randn(256, 3)).astype(F32)]), dev)
    v, f = _t(clean, dev), _t(faces, dev, torch.int32)
    g = meshgrid.TriangleGrid(v, f)
    want = mesheval.point_to_mesh(q, v, f)
    _same(g.nearest(q), want, 'the default budget')
    assert g.left_over == q.shape[0] and min(g.dims) >= 2 * (G.DEFAULT_RINGS + 4)
    _same(g.nearest(q, max_rings=G.MAX_CELLS), want, 'the whole walk')
    assert g.left_over == 0


def test_ties_at_vertices_and_edge_midpoints(dev):
    from geobi_gnn_amd import meshgen
    points, faces, _ = _ico()
    ev = meshgen.mesh_edges(faces)
    mid = ((points[ev[:, 0]].astype(np.float64) + points[ev[:, 1]]) / 2).astype(F32)
    q = np.concatenate([points, mid])
    for g in _triangles_case(dev, points, faces, q, 'ties', cells=(None, 2, 9)):
        d, i = g.nearest(_t(q, dev))
        i = i.cpu().numpy()[:len(points)]
        first = np.array([np.nonzero((faces == k).any(axis=1))[0][0] for k in range(len(points))])
        assert not d[:len(points)].any() and np.array_equal(i, first)       # of the 5 or 6 faces at a vertex: the first


def test_one_triangle_across_the_box_meets_the_entry_cap(dev):
    from geobi_gnn_amd import meshgrid
    points, faces, _ = _ico()
    verts = np.concatenate([points, F32([[-1, -1, -1], [1, 1, -1], [0, 1, 1]])])
    big = np.concatenate([faces[:100], [[162, 163, 164]], faces[101:]]).astype(np.int32)
    q = P.shell_queries(257, seed=9)
    plain, forced = _triangles_case(dev, verts, big, q, 'across', cells=(None, 64))
    assert forced.rounds > 1 and max(forced.dims) < 64 and forced.entries <= G.ENTRY_CAP * 320
    print('forced 64 -> %s after %d rounds, %d entries; the rule: %s, %d rounds, %d entries'
          % (forced.dims, forced.rounds, forced.entries, plain.dims, plain.rounds, plain.entries))
    alone = meshgrid.TriangleGrid(_t(verts, dev), _t([[162, 163, 164]], dev, torch.int32), cells=G.MAX_CELLS)
    assert alone.entries <= G.ENTRY_CAP and alone.rounds <= 9


def test_strips_and_a_face_with_a_corner_that_is_not_finite(dev):
    rng = np.random.RandomState(10)
    for n_faces in (255, 256, 257):
        V = n_faces + 2
        verts = np.stack([np.arange(V) * 0.5, (np.arange(V) % 2).astype(np.float64), 0.1 * rng.randn(V)], axis=1).astype(F32)
        faces = W._strip(V, torch.device('cpu')).numpy()
        q = (verts[rng.randint(0, V, 257)] + 0.3 * rng.randn(257, 3)).astype(F32)
        _triangles_case(dev, verts, faces, q, 'strip of %d' % n_faces, cells=(None, 5))
    verts[3, 1] = np.nan
    verts[100] = np.inf
    g = _triangles_case(dev, verts, faces, q, 'corners not finite', cells=(None, 5))[0]
    assert g.finite == 257 - 6


# ---------------------------------------------------------------------------------------------- further cases
def test_the_20480_face_sphere_against_its_noisy_vertices(dev):
    from geobi_gnn_amd import mesheval, meshgrid
    noisy, clean, faces = _big()
    q, v, f = _t(noisy, dev), _t(clean, dev), _t(faces, dev, torch.int32)
    gp, gt = meshgrid.PointGrid(v), meshgrid.TriangleGrid(v, f)
    assert G.check_points(G.of_grid(gp), clean.astype(F32)) == []
    assert G.check_triangles(G.of_grid(gt), clean.astype(F32), faces) == []
    first = gp.nearest(q), gt.nearest(q)
    print('points: dims %s, left over %d; triangles: dims %s, %d entries, %d rounds, left over %d'
          % (gp.dims, gp.left_over, gt.dims, gt.entries, gt.rounds, gt.left_over))
    _same(first[0], mesheval.nearest_point(q, v), 'points')
    _same(first[1], mesheval.point_to_mesh(q, v, f), 'triangles')
    # two equal calls give equal bits, and so does a grid built again
    _same(gp.nearest(q), first[0], 'points again')
    _same(meshgrid.TriangleGrid(v, f).nearest(q), first[1], 'triangles again')
    # a grid built before serves as index=; one over another set is refused
    _same(mesheval.nearest_point(q, v, index=gp), first[0], 'index = a PointGrid')
    _same(mesheval.point_to_mesh(q, v, f, index=gt), first[1], 'index = a TriangleGrid')
    with pytest.raises(ValueError):
        mesheval.nearest_point(q, v[:-1], index=gp)
    with pytest.raises(ValueError):
        mesheval.point_to_mesh(q, v, f, index=gp)


def case_grid(dev):
    from geobi_gnn_amd import meshgrid
    points, faces, _ = _ico()
    q = np.concatenate([P.shell_queries(255, seed=11), np.zeros((2, 3), dtype=F32)])         # two left over at 9 cells across
    v, f, q = _t(points, dev), _t(faces, dev, torch.int32), _t(q, dev)
    gp, gt = meshgrid.PointGrid(v, cells=9), meshgrid.TriangleGrid(v, f, cells=40)
    return [gp.cell_start, gp.order, gt.cell_start, gt.order, gt.records, gt.rounds, gp.nearest(q, max_rings=2), gt.nearest(q, max_rings=2),
            gp.left_over, gt.left_over]


def test_guard_band_and_short_workspace(dev, monkeypatch):
    name = 'grid_left_over'                          # a case of this module's beside that module's own 'grid'
    W.CASES[name] = case_grid
    try:
        W.test_guard_band(name, dev, monkeypatch)
        W.test_short_workspace(name, dev, monkeypatch)
    finally:
        del W.CASES[name]
        W._REF.pop(name, None)


def test_a_guard_band_around_the_outputs(dev):
    """dist, idx, left, left_q and count lie inside one buffer of sentinels; no byte outside them changes"""
    from geobi_gnn_amd import _lib as L
    from geobi_gnn_amd import meshgrid
    points, faces, _ = _ico()
    g = meshgrid.TriangleGrid(_t(points, dev), _t(faces, dev, torch.int32), cells=24)
    q = _t(np.concatenate([P.shell_queries(255, seed=12), np.zeros((2, 3), dtype=F32)]), dev)
    Q, pad = q.shape[0], 1024
    want = g.nearest(q, max_rings=2)
    assert 0 < g.left_over < Q
    sizes = (Q, Q, Q, 3 * Q, 1)
    at = [pad * (k + 1) + sum(sizes[:k]) for k in range(5)]
    buf = torch.full((at[-1] + 1 + pad,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    before = buf.clone()
    dist, idx, left, left_q, count = [buf[a:a + n] for a, n in zip(at, sizes)]
    ws = L.workspace(L.size_query('geobi_grid_nearest_ws_bytes', Q), dev)
    L.call('geobi_grid_nearest_triangle', L.ptr(q), L.ptr(g.records), Q, faces.shape[0], g.desc, L.ptr(g.cell_start), L.ptr(g.order), 2,
           L.ptr(dist), L.ptr(idx), L.ptr(left), L.ptr(left_q), L.ptr(count), L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    n = int(count[0])
    assert n == g.left_over
    rest = left[:n].long()
    assert bool((rest[1:] > rest[:-1]).all()) and torch.equal(left_q[:3 * n].view(torch.float32).view(n, 3), q[rest])
    done = torch.ones(Q, dtype=torch.bool, device=dev)
    done[rest] = False
    assert torch.equal(dist[done], want[0].view(torch.int32)[done]) and torch.equal(idx[done], want[1][done])
    assert bool((dist[~done] == 0x5A5A5A5A).all()) and bool((left[n:] == 0x5A5A5A5A).all())      # what is left over is not written
    outside = torch.ones_like(buf, dtype=torch.bool)
    for a, k in zip(at, sizes):
        outside[a:a + k] = False
    assert torch.equal(buf[outside], before[outside]), 'a byte outside the outputs changed'


# ---------------------------------------------------------------------------------------------- callers
def _pair(dev):
    points, faces, _ = _ico(4)
    other, other_faces, _ = _ico(8)
    rng = np.random.RandomState(13)
    return ((points + 0.03 * rng.randn(*points.shape)).astype(F32), faces, points, (other * F32(1.02)).astype(F32), other_faces)


def test_callers_return_the_same_bits_with_the_grid(dev):
    from geobi_gnn_amd import mesheval, meshproject, meshremesh
    noisy, faces, clean, other, other_faces = _pair(dev)
    assert mesheval.eval_pair(noisy, faces, clean, device=dev, index='grid') == mesheval.eval_pair(noisy, faces, clean, device=dev)
    assert (mesheval.eval_free(noisy, faces, other, other_faces, device=dev, index='grid')
            == mesheval.eval_free(noisy, faces, other, other_faces, device=dev))
    assert (mesheval.eval_sampled(noisy, faces, other, other_faces, 1000, device=dev, index='grid')
            == mesheval.eval_sampled(noisy, faces, other, other_faces, 1000, device=dev))
    got, want = meshproject.closest(noisy, other, other_faces, device=dev, index='grid'), meshproject.closest(noisy, other, other_faces, device=dev)
    for field in ('face', 'bary', 'points', 'dist'):
        assert torch.equal(getattr(got, field).view(torch.int32), getattr(want, field).view(torch.int32)), field
    moved = meshproject.project(noisy, other, other_faces, max_dist=0.02, device=dev, index='grid')
    plain = meshproject.project(noisy, other, other_faces, max_dist=0.02, device=dev)
    assert torch.equal(moved[0].view(torch.int32), plain[0].view(torch.int32)) and moved[1] == plain[1]
    for points, fv in ((clean, faces), (other, other_faces)):
        a = meshremesh.remesh(points, fv, iterations=2, feature_angle=180.0, project=True, device=dev, index='grid')
        b = meshremesh.remesh(points, fv, iterations=2, feature_angle=180.0, project=True, device=dev)
        assert a.per_iteration == b.per_iteration and a.after == b.after
        for field in ('points', 'faces', 'source_face', 'source_bary'):
            assert torch.equal(getattr(a, field).view(torch.int32), getattr(b, field).view(torch.int32)), field


def _same_tree(a, b):
    cmp = filecmp.dircmp(a, b)
    assert not cmp.left_only and not cmp.right_only and (cmp.common_files or cmp.common_dirs), (cmp.left_only, cmp.right_only)
    match, mismatch, errors = filecmp.cmpfiles(a, b, cmp.common_files, shallow=False)
    assert not mismatch and not errors, (mismatch, errors)
    for sub in cmp.common_dirs:
        _same_tree(os.path.join(a, sub), os.path.join(b, sub))


def test_commands_write_the_same_bytes_with_the_flag(dev, tmp_path):
    from geobi_gnn_amd import meshio
    noisy, faces, clean, other, other_faces = _pair(dev)
    roots = {}
    for word in ('none', 'grid'):
        root = roots[word] = str(tmp_path / word)
        for sub in ('data/original', 'data/noisy', 'result', 'gt'):
            os.makedirs(os.path.join(root, sub))
        meshio.write_obj(os.path.join(root, 'data', 'original', 'ball.obj'), clean, faces)
        meshio.write_obj(os.path.join(root, 'data', 'noisy', 'ball_n1.obj'), noisy, faces)
        meshio.write_obj(os.path.join(root, 'result', 'ball_n1.obj'), noisy, faces)
        meshio.write_obj(os.path.join(root, 'gt', 'ball.obj'), other, other_faces)
        flag = ['--index', word] if word == 'grid' else []
        runs = [_run(['eval', '--result_dir', os.path.join(root, 'result'), '--original_dir', os.path.join(root, 'gt'), '--free'] + flag),
                _run(['project', '--data_dir', os.path.join(root, 'result'), '--target_dir', os.path.join(root, 'gt')] + flag),
                _run(['remesh', '--data_dir', os.path.join(root, 'data'), '--iterations', '2', '--feature_angle', '180', '--project'] + flag)]
        assert all(r.returncode == 0 for r in runs), [r.stderr for r in runs]
        roots[word + ' out'] = [r.stdout.replace(root, 'ROOT') for r in runs]
    assert os.path.exists(os.path.join(roots['grid'], 'result', 'ErrorInfo_free.txt'))
    assert os.path.exists(os.path.join(roots['grid'], 'result', 'projected', 'ball_n1.obj'))
    assert os.path.exists(os.path.join(roots['grid'], 'data', 'remeshed', 'noisy', 'ball_n1.obj'))
    _same_tree(roots['none'], roots['grid'])
    for a, b in zip(roots['none out'], roots['grid out']):
        strip = lambda text: [l for l in text.splitlines() if 'seconds' not in l and ' s ' not in l]
        assert strip(a) == strip(b)
