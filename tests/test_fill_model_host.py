"""The plain statement of hole filling (tests/fill_model.py) pinned on facts that do not come from it, the comparison
helper of the GPU test caught on planted faults, and the parts of the feature that run without a GPU: the command line and
the size limits of the entry points."""
import copy
import ctypes

import numpy as np
import pytest

import fill_model as M
import topo_model
from train_cases import _run


def _euler(faces):
    c = topo_model.report_counts(faces)
    return c['vertices_used'] - c['edges'] + c['faces']


@pytest.mark.parametrize('n, k', [(3, 1), (4, 5), (6, 12)])
def test_icosphere_with_fans_removed_is_closed_again(n, k):
    points, faces, removed, each = M.sphere_without_fans(n, k)
    valences = sum(each)
    V, F = points.shape[0], faces.shape[0]
    before = topo_model.report_counts(faces)
    assert before['boundary_edges'] == valences and before['vertices_used'] == V - k
    r = M.fill_holes(points, faces)
    after = topo_model.report_counts(r.faces)
    assert (after['boundary_edges'], after['complex_edges'], after['inconsistent_edges']) == (0, 0, 0)
    assert _euler(r.faces) == 2
    assert r.points.shape[0] == V + k and r.faces.shape[0] - F == valences
    assert r.counts == dict(boundary_edges=valences, blocked_vertices=0, chain_edges=0, loops=k, longest_loop=max(each),
                            filled_loops=k, skipped_loops=0, new_faces=valences)
    assert np.array_equal(r.faces[:F], faces) and np.array_equal(M.bits(r.points[:V]), M.bits(points))
    # the new vertex of a hole lies where the removed one was, up to the flatness of its fan
    d = np.linalg.norm(r.points[V:, None, :].astype(np.float64) - points[removed][None, :, :], axis=2)
    assert d.min(axis=1).max() < 0.15 and sorted(d.argmin(axis=1).tolist()) == list(range(k))


def test_flat_grid_with_blocks_removed():
    blocks = [(2, 2, 5, 4), (7, 1, 8, 2), (7, 5, 11, 10), (1, 7, 3, 10)]
    points, faces = M.grid_with_holes(13, 12, blocks)
    V, F = points.shape[0], faces.shape[0]
    rim = 2 * (13 + 12)
    r = M.fill_holes(points, faces, max_hole_edges=rim - 1)
    assert r.counts['loops'] == 5 and r.counts['filled_loops'] == 4 and r.counts['skipped_loops'] == 1
    assert r.counts['longest_loop'] == rim and r.counts['blocked_vertices'] == 0 and r.counts['chain_edges'] == 0
    assert sorted(r.loops.length.tolist()) == sorted([2 * (x1 - x0 + y1 - y0) for x0, y0, x1, y1 in blocks] + [rim])
    assert topo_model.report_counts(r.faces)['boundary_edges'] == rim
    centres = sorted((0.5 * (x0 + x1), 0.5 * (y0 + y1), 0.0) for x0, y0, x1, y1 in blocks)
    assert sorted(tuple(float(x) for x in p) for p in r.points[V:]) == centres
    # the patch of every block: wound like the grid (normal + z) and of exactly the removed area, in fp64
    p = r.points.astype(np.float64)
    for j in range(4):
        tri = r.faces[F:][r.new_face_loop == r.new_vertex_loop[j]]
        cross = np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]])
        assert (cross[:, 2] > 0).all() and (cross[:, :2] == 0).all()
        cx, cy = r.points[V + j, 0], r.points[V + j, 1]
        x0, y0, x1, y1 = [b for b in blocks if (0.5 * (b[0] + b[2]), 0.5 * (b[1] + b[3])) == (cx, cy)][0]
        assert 0.5 * cross[:, 2].sum() == float((x1 - x0) * (y1 - y0))
    # with the limit at the rim's length the rim is closed too, from outside
    assert M.fill_holes(points, faces, max_hole_edges=rim).counts['filled_loops'] == 5
    assert M.fill_holes(points, faces, max_hole_edges=3).counts['filled_loops'] == 0


HAND = M.hand_cases()


@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_cases_have_the_counts_written_out(name):
    points, faces, counts = HAND[name]
    r = M.fill_holes(points, faces)
    assert r.counts == counts
    assert r.points.shape[0] == points.shape[0] + counts['filled_loops']
    assert r.faces.shape[0] == faces.shape[0] + counts['new_faces']
    assert np.array_equal(r.faces[:faces.shape[0]], faces)
    assert np.array_equal(M.bits(r.points[:points.shape[0]]), M.bits(points))
    assert int((r.loops.loop == -2).sum()) == counts['chain_edges']
    assert int((r.loops.loop >= -2).sum() - (r.loops.loop == -1).sum()) == counts['boundary_edges']
    after = topo_model.report_counts(r.faces)
    before = topo_model.report_counts(faces)
    assert after['boundary_edges'] == counts['chain_edges']
    assert after['complex_edges'] == before['complex_edges'] and after['inconsistent_edges'] == before['inconsistent_edges']


def test_cup_ranks_follow_the_rim_against_the_faces():
    n = 7
    points, faces, _ = HAND['cup7']
    loops = M.boundary_loops(faces, points.shape[0])
    assert loops.length.tolist() == [n] and loops.leader.tolist() == [1] and loops.loop_ptr.tolist() == [0, n]
    # face i = (0, 1 + i, 1 + (i + 1) % n) is walked from its third corner to its second: the rim in descending order
    assert [int(loops.rank[3 * i + 1]) for i in range(n)] == [(n - i) % n for i in range(n)]
    assert loops.loop_vertices.tolist() == [2, 1, 7, 6, 5, 4, 3]
    assert all(loops.loop[3 * i] == -1 and loops.loop[3 * i + 2] == -1 and loops.loop[3 * i + 1] == 0 for i in range(n))
    r = M.fill_holes(points, faces)
    assert r.faces[n:].tolist() == [[2, 1, 8], [1, 7, 8], [7, 6, 8], [6, 5, 8], [5, 4, 8], [4, 3, 8], [3, 2, 8]]
    assert r.new_vertex_loop.tolist() == [0] and r.new_face_loop.tolist() == [0] * n
    assert abs(float(r.points[8, 0])) < 1e-6 and abs(float(r.points[8, 1])) < 1e-6 and r.points[8, 2] == 0


def test_cylinder_has_two_loops_and_the_triangle_becomes_a_tetrahedron():
    points, faces, _ = HAND['cylinder6']
    r = M.fill_holes(points, faces)
    assert r.loops.length.tolist() == [6, 6] and r.loops.leader.tolist() == sorted(r.loops.leader.tolist())
    assert set(r.loops.loop_vertices[:6].tolist()) in ({0, 1, 2, 3, 4, 5}, {6, 7, 8, 9, 10, 11})
    assert _euler(r.faces) == 2
    points, faces, _ = HAND['isolated_triangle']
    r = M.fill_holes(points, faces)
    assert r.faces.tolist() == [[0, 1, 2], [1, 0, 3], [0, 2, 3], [2, 1, 3]] and _euler(r.faces) == 2
    assert r.loops.rank.tolist() == [0, 2, 1]


def test_a_closed_mesh_comes_back_as_it_is():
    points, faces, _ = HAND['closed']
    r = M.fill_holes(points, faces)
    assert np.array_equal(r.faces, faces) and np.array_equal(M.bits(r.points), M.bits(points))
    assert set(r.counts.values()) == {0} and (r.loops.loop == -1).all()
    assert np.array_equal(M.bits(M.apply(r, points)), M.bits(points))


def test_max_hole_edges_at_the_length_and_one_below():
    points, faces, _ = HAND['cup7']
    assert M.fill_holes(points, faces, max_hole_edges=7).counts['filled_loops'] == 1
    r = M.fill_holes(points, faces, max_hole_edges=6)
    assert (r.counts['filled_loops'], r.counts['skipped_loops'], r.counts['new_faces']) == (0, 1, 0)
    assert r.faces.shape == faces.shape and r.points.shape == points.shape


def test_apply_of_the_input_is_the_output():
    points, faces = M.cup(129, shuffle=5, mantissa=6)
    r = M.fill_holes(points, faces)
    assert np.array_equal(M.bits(M.apply(r, points)), M.bits(r.points))
    moved = M.apply(r, points * np.float32(3.0))
    assert not np.array_equal(M.bits(moved[-1]), M.bits(r.points[-1]))


def test_planted_faults_are_caught():
    points, faces = M.cup(129, shuffle=5, mantissa=6)
    F = faces.shape[0]
    want = M.fill_holes(points, faces)
    M.assert_same(copy.deepcopy(want), want)
    # a swapped winding of one new face
    bad = copy.deepcopy(want)
    bad.faces[F + 17] = bad.faces[F + 17, [1, 0, 2]]
    with pytest.raises(AssertionError, match='faces differ'):
        M.assert_same(bad, want)
    # two new faces in exchanged rows
    bad = copy.deepcopy(want)
    bad.faces[[F + 3, F + 4]] = bad.faces[[F + 4, F + 3]]
    with pytest.raises(AssertionError, match='faces differ'):
        M.assert_same(bad, want)
    # a centre summed in plain rank order: at 65 and more slots the 64 partial sums are another sequence of roundings
    rim = points[want.loops.loop_vertices].astype(np.float64)
    plain = np.zeros(3)
    for row in rim:
        plain = plain + row
    bad = copy.deepcopy(want)
    bad.points[-1] = (plain / rim.shape[0]).astype(np.float32)
    assert np.isfinite(bad.points[-1]).all() and np.isfinite(want.points[-1]).all()
    with pytest.raises(AssertionError, match='points differ'):
        M.assert_same(bad, want)
    # one flipped last bit
    bad = copy.deepcopy(want)
    bad.points.view(np.uint32)[-1, 1] ^= 1
    with pytest.raises(AssertionError, match='points differ'):
        M.assert_same(bad, want)
    # a rank off by one turn of the loop, a chain slot reported as no boundary
    bad = copy.deepcopy(want)
    on = bad.loops.rank >= 0
    bad.loops.rank[on] = (bad.loops.rank[on] + 1) % 129
    with pytest.raises(AssertionError, match='loops.rank differ'):
        M.assert_same(bad, want)
    points, faces, _ = HAND['bow_tie']
    want = M.fill_holes(points, faces)
    bad = copy.deepcopy(want)
    bad.loops.loop[0] = -1
    with pytest.raises(AssertionError, match='loops.loop differ'):
        M.assert_same(bad, want)


def test_fill_help_names_every_flag():
    run = _run(['fill', '--help'])
    assert run.returncode == 0
    for flag in ('--data_dir', '--out_dir', '--max_hole_edges', '--gpu'):
        assert flag in run.stdout, flag
    from geobi_gnn_amd.__main__ import parse_args
    for args in (['--max_hole_edges', '-1'], ['--max_hole_edges', '2.5'], ['--max_hole_edges', 'many']):
        with pytest.raises(SystemExit) as e:
            parse_args(['fill', '--data_dir', 'nowhere'] + args)
        assert e.value.code == 2, args
    with pytest.raises(SystemExit) as e:
        parse_args(['fill'])
    assert e.value.code == 2
    opt = parse_args(['fill', '--data_dir', 'd'])
    assert (opt.max_hole_edges, opt.out_dir, opt.gpu) == (0, '', -1)
    assert parse_args(['fill', '--data_dir', 'd', '--max_hole_edges', '30']).max_hole_edges == 30


def test_bad_arguments_are_value_errors_before_any_device_work():
    from geobi_gnn_amd import meshfill
    points, faces, _ = HAND['cup7']
    for value in (-1, 2.5, '3', None, True):
        with pytest.raises(ValueError, match='max_hole_edges'):
            meshfill.fill_holes(points, faces, max_hole_edges=value)
    with pytest.raises(ValueError, match='V = '):
        meshfill.boundary_loops(faces, -1)


def test_sizes_beyond_the_documented_limits_are_rejected():
    """geobi_fill_*: F or V above GEOBI_MAX_NODES, negative sizes and a negative max_hole_edges are refused before anything
    touches the device (no GPU needed)."""
    from geobi_gnn_amd import _lib as L
    lib = L.lib()
    big = (1 << 24)
    one = ctypes.c_void_p(256)                     # never dereferenced: the checks come first
    assert lib.geobi_fill_ws_bytes(big, 10) == 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
    assert lib.geobi_fill_ws_bytes(10, big) == 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
    assert lib.geobi_fill_ws_bytes(-1, 10) == 0 and b'negative' in lib.geobi_last_error()
    assert lib.geobi_fill_ws_bytes(10, -1) == 0 and b'negative' in lib.geobi_last_error()
    for F, V in ((big, 10), (10, big)):
        rc = lib.geobi_fill_plan(one, F, V, 0, one, one, one, one, one, None, one, 1 << 20, None)
        assert rc != 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
        rc = lib.geobi_fill_emit(one, one, F, V, V, F, one, one, one, one, one, 1 << 20, None)
        assert rc != 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
        rc = lib.geobi_fill_points(one, F, V, V, one, one, 1 << 20, None)
        assert rc != 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
    # a fill whose output would be too large: refused by emit before anything is written
    rc = lib.geobi_fill_emit(one, one, big - 1, 10, 11, big + 2, one, one, one, one, one, 1 << 20, None)
    assert rc != 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
    rc = lib.geobi_fill_points(one, 10, big - 1, big, one, one, 1 << 20, None)
    assert rc != 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
    # sizes no plan of these F, V gives
    rc = lib.geobi_fill_emit(one, one, 10, 10, 9, 10, one, one, one, one, one, 1 << 20, None)
    assert rc != 0 and b'can give' in lib.geobi_last_error()
    rc = lib.geobi_fill_emit(one, one, 10, 10, 21, 10, one, one, one, one, one, 1 << 20, None)
    assert rc != 0 and b'can give' in lib.geobi_last_error()
    rc = lib.geobi_fill_emit(one, one, 10, 10, 11, 41, one, one, one, one, one, 1 << 20, None)
    assert rc != 0 and b'can give' in lib.geobi_last_error()
    for F, V in ((-1, 10), (10, -1)):
        rc = lib.geobi_fill_plan(one, F, V, 0, one, one, one, one, one, None, one, 1 << 20, None)
        assert rc != 0 and b'negative' in lib.geobi_last_error()
    rc = lib.geobi_fill_plan(one, 10, 10, -1, one, one, one, one, one, None, one, 1 << 20, None)
    assert rc != 0 and b'max_hole_edges' in lib.geobi_last_error()
