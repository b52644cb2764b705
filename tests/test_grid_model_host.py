"""tests/grid_model.py on hand-made tables (no device): sound tables pass, every planted fault is flagged; the header
declares the grid's entry points; the commands accept and refuse --index; index= refuses unknown words."""
import numpy as np
import pytest
import torch

import grid_model as G


def _lattice():
    return np.array([(x, y, z) for z in range(5) for y in range(5) for x in range(5)], dtype=np.float64)


def _fan():
    """a 4 x 4 patch of a height field as 32 triangles, and one face with a corner that is not finite"""
    n = 5
    verts = np.array([(x, y, 0.25 * ((x * 7 + y * 3) % 4)) for y in range(n) for x in range(n)] + [(np.nan, 0.0, 0.0)],
                     dtype=np.float64)
    faces = []
    for y in range(n - 1):
        for x in range(n - 1):
            a = y * n + x
            faces += [(a, a + 1, a + n), (a + 1, a + n + 1, a + n)]
    faces.append((0, 1, n * n))
    return verts, np.array(faces, dtype=np.int64)


def _with(t, **fields):
    return t._replace(**fields)


def test_sound_point_tables_pass():
    pts = _lattice()
    for dims in ((1, 1, 1), (2, 2, 2), (4, 4, 4), (5, 3, 2)):
        t = G.host_point_tables(pts, dims)
        assert t.dims == dims and len(t.cell_start) == dims[0] * dims[1] * dims[2] + 1
        assert G.check_points(t, pts) == []
    pts = np.concatenate([pts, [[np.nan, 0, 0], [0, np.inf, 0]]])
    t = G.host_point_tables(pts, (3, 3, 3))
    assert len(t.order) == 125 and G.check_points(t, pts) == []
    flat = _lattice()
    flat[:, 2] = 7.0
    t = G.host_point_tables(flat, (4, 4, 4))
    assert t.dims == (4, 4, 1) and G.check_points(t, flat) == []


def test_an_entry_dropped_is_flagged():
    pts = _lattice()
    t = G.host_point_tables(pts, (4, 4, 4))
    k = 17
    cs = t.cell_start.copy()
    cs[np.searchsorted(cs, k, side='right'):] -= 1
    faults = G.check_points(_with(t, order=np.delete(t.order, k), cell_start=cs), pts)
    assert faults and 'permutation' in faults[0]


def test_two_indices_swapped_inside_a_cell_are_flagged():
    pts = _lattice()
    t = G.host_point_tables(pts, (2, 2, 2))
    k = int(t.cell_start[3])
    assert t.cell_start[4] - k >= 2
    order = t.order.copy()
    order[k], order[k + 1] = order[k + 1], order[k]
    faults = G.check_points(_with(t, order=order), pts)
    assert faults and 'is followed by' in faults[0]


def test_a_point_filed_one_cell_off_is_flagged():
    pts = _lattice() + 0.25                     # off the planes of the cells: a neighbour's box is a whole margin away
    pts[0] -= 0.25
    pts[-1] += 0.25
    t = G.host_point_tables(pts, (4, 4, 4))
    cell = G.cell_of_entry(t)
    k = int(np.nonzero(cell == 5)[0][0])        # move the first entry of cell 5 to the end of cell 4
    moved = t.order[k]
    assert moved > t.order[k - 1]               # indices still ascend inside cell 4: only the place is wrong
    cs = t.cell_start.copy()
    cs[5] += 1
    faults = G.check_points(_with(t, cell_start=cs), pts)
    assert faults and 'outside the widened box' in faults[0] and 'point %d ' % moved in faults[0]


def test_sound_triangle_tables_pass_and_a_missing_face_is_flagged():
    verts, faces = _fan()
    for dims in ((1, 1, 1), (4, 4, 2), (3, 3, 1)):
        t = G.host_triangle_tables(verts, faces, dims)
        assert G.check_triangles(t, verts, faces) == []
        assert not (t.order == len(faces) - 1).any()
    t = G.host_triangle_tables(verts, faces, (4, 4, 2))
    cell = G.cell_of_entry(t)
    # face 0 spans the cells its box meets; drop it from the one that holds its inside
    mn, mx, _ = G.face_boxes(verts, faces)
    k0, k1 = G.required_cells(t, mn, mx)
    assert (k0[0] <= k1[0]).all()
    want = (k0[0][2] * t.dims[1] + k0[0][1]) * t.dims[0] + k0[0][0]
    k = int(np.nonzero((cell == want) & (t.order == 0))[0][0])
    cs = t.cell_start.copy()
    cs[want + 1:] -= 1
    faults = G.check_triangles(_with(t, order=np.delete(t.order, k), cell_start=cs), verts, faces)
    assert faults and 'face 0 is not listed in cell %d' % want in faults[0]


def test_a_face_listed_twice_a_filed_face_that_is_not_finite_and_the_cap_are_flagged():
    verts, faces = _fan()
    t = G.host_triangle_tables(verts, faces, (4, 4, 2))
    k = int(t.cell_start[1]) - 1
    cs = t.cell_start.copy()
    cs[1:] += 1
    twice = _with(t, order=np.insert(t.order, k, t.order[k]), cell_start=cs)
    assert 'is followed by' in G.check_triangles(twice, verts, faces)[0]
    bad = _with(t, order=np.insert(t.order, k + 1, len(faces) - 1), cell_start=cs)
    assert 'not finite' in G.check_triangles(bad, verts, faces)[0]
    few = np.array([[0, 4, 24]], dtype=np.int64)                       # one face across the box
    alone = G.host_triangle_tables(verts, few, (8, 8, 8))
    assert len(alone.order) > G.ENTRY_CAP and any('beyond the cap' in f for f in G.check_triangles(alone, verts, few))
    among = np.concatenate([faces, few])
    big = G.host_triangle_tables(verts, among, (2, 2, 1))
    assert len(big.order) <= G.ENTRY_CAP * len(among) and G.check_triangles(big, verts, among) == []


def test_cell_start_must_cover_the_entries():
    pts = _lattice()
    t = G.host_point_tables(pts, (2, 2, 2))
    cs = t.cell_start.copy()
    cs[-1] -= 1
    assert 'cell_start' in G.check_points(_with(t, cell_start=cs), pts)[0]
    assert 'cell_start' in G.check_points(_with(t, cell_start=t.cell_start[:-1]), pts)[0]


def test_header_declares_the_entry_points():
    from geobi_gnn_amd import _lib
    protos = _lib.parse_header()
    for name in ('geobi_grid_points_plan', 'geobi_grid_points_build', 'geobi_grid_triangles_plan', 'geobi_grid_triangles_build',
                 'geobi_grid_nearest_point', 'geobi_grid_nearest_triangle', 'geobi_grid_scatter', 'geobi_grid_plan_ws_bytes',
                 'geobi_grid_points_build_ws_bytes', 'geobi_grid_triangles_build_ws_bytes', 'geobi_grid_nearest_ws_bytes',
                 'geobi_grid_default_rings', 'geobi_grid_max_cells', 'geobi_grid_entry_cap'):
        assert name in protos, name
    names = protos['geobi_grid_nearest_triangle'][2]
    assert names[:4] == ['q', 'records', 'Q', 'F'] and names[-3:] == ['ws', 'ws_bytes', 'stream'] and 'max_rings' in names
    assert protos['geobi_grid_points_plan'][2] == ['t', 'T', 'cells', 'desc', 'ws', 'ws_bytes', 'stream']


def test_the_commands_accept_and_refuse_index_values(capsys):
    from geobi_gnn_amd.__main__ import parse_args
    ev = ['eval', '--result_dir', 'r', '--original_dir', 'o']
    pr = ['project', '--data_dir', 'd', '--target_dir', 't']
    rm = ['remesh', '--data_dir', 'd']
    assert parse_args(ev).index == 'none' and parse_args(pr).index == 'none' and parse_args(rm).index == 'none'
    assert parse_args(ev + ['--free', '--index', 'grid']).index == 'grid'
    assert parse_args(pr + ['--index', 'grid']).index == 'grid'
    assert parse_args(rm + ['--project', '--index', 'grid']).index == 'grid'
    assert parse_args(rm + ['--project', '--index', 'none']).index == 'none'
    for argv in (ev + ['--index', 'auto'], pr + ['--index', 'bvh'], rm + ['--project', '--index', ''], rm + ['--index', 'grid']):
        with pytest.raises(SystemExit):
            parse_args(argv)
    assert '--index' in capsys.readouterr().err


def test_index_refuses_unknown_words_before_it_asks_for_a_device():
    from geobi_gnn_amd import mesheval, meshgrid, meshproject, meshremesh
    p = torch.zeros((3, 3))
    f = torch.tensor([[0, 1, 2]])
    for word in ('auto', 'none', 'GRID', 1, True):
        for call in (lambda: mesheval.nearest_point(p, p, index=word), lambda: mesheval.point_to_mesh(p, p, f, index=word),
                     lambda: mesheval.eval_pair(p, f, p, index=word), lambda: mesheval.eval_free(p, f, p, f, index=word),
                     lambda: mesheval.eval_sampled(p, f, p, f, 8, index=word), lambda: mesheval.eval_dirs('r', 'o', index=word),
                     lambda: meshproject.closest(p, p, f, index=word), lambda: meshproject.project(p, p, f, index=word),
                     lambda: meshremesh.remesh(p, f, project=True, index=word)):
            with pytest.raises(ValueError, match='index'):
                call()
    assert meshgrid.check_index(None) is None and meshgrid.check_index('grid') == 'grid'
    with pytest.raises(ValueError, match='project = True'):
        meshremesh.remesh(p, f, index='grid')
