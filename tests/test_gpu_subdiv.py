"""Mesh refinement on the device (csrc/subdiv.hip, geobi_gnn_amd/meshsubdiv.py) against the sequential model of
tests/subdiv_model.py, and the `subdivide` command end to end.

Every comparison is EXACT: faces, face_parent, vertex_parents and the counts equal as integers, the points equal as
uint32 bit patterns.  There are no tolerances."""
import os
import re

import numpy as np
import pytest
import torch

import subdiv_model as M
from train_cases import _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


class _Host(object):
    """a device result as numpy arrays"""

    def __init__(self, r):
        for field in ('points', 'faces', 'face_parent', 'vertex_parents'):
            t = getattr(r, field)
            assert t.is_cuda and t.is_contiguous(), field
            setattr(self, field, t.cpu().numpy())
        self.counts = r.counts


_MODELS = {}


def _check(dev, name, points, faces, **kw):
    """subdivide on the device against the model (computed once per named input), everything exact; apply with the input's
    points must reproduce the output bit for bit -> (device result, model result)"""
    from geobi_gnn_amd import meshsubdiv
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _MODELS:
        _MODELS[key] = M.subdivide(points, faces, **kw)
    want = _MODELS[key]
    got = meshsubdiv.subdivide(points, faces, device=dev, **kw)
    M.assert_same(_Host(got), want, name)
    assert [dict(p.counts, V=p.Vn, F=p.Fn) for p in got.passes] == want.per_pass, name
    again = meshsubdiv.apply(got, points)
    assert np.array_equal(M.bits(again.cpu().numpy()), M.bits(want.points)), name + ': apply(input points)'
    return got, want


HAND = M.hand_cases()


@pytest.mark.parametrize('name', sorted(HAND))
@pytest.mark.parametrize('scheme', ['midpoint', 'loop'])
def test_hand_cases(dev, name, scheme):
    points, faces = HAND[name]
    _check(dev, name, points, faces, levels=2, scheme=scheme)


@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_cases_max_edge(dev, name):
    points, faces = HAND[name]
    L = 0.4 * float(np.sqrt(M.longest_edge2(points, faces)))
    _, want = _check(dev, name, points, faces, max_edge=L)
    assert want.counts['passes'] >= 2


def test_hub_of_valence_200(dev):
    """longer than a wave; the rim is numbered in a shuffled order, so the ascending sum is not the order of the faces"""
    for closed in (True, False):
        points, faces = M.hub(200, closed=closed)
        _check(dev, 'hub200-%d' % closed, points, faces, levels=1, scheme='loop')
        _check(dev, 'hub200-%d' % closed, points, faces, levels=1, scheme='midpoint')


@pytest.mark.parametrize('n_faces', [85, 86, 255, 256, 257])
def test_strips_at_the_block_edges(dev, n_faces):
    """F and 3F across 256: the block edges of the face, slot and edge kernels"""
    points, faces = M.strip(n_faces)
    _check(dev, 'strip%d' % n_faces, points, faces, levels=1, scheme='midpoint')
    _check(dev, 'strip%d' % n_faces, points, faces, levels=1, scheme='loop')
    _check(dev, 'strip%d' % n_faces, points, faces, max_edge=0.8)


def test_all_four_templates_in_one_mesh(dev):
    points, faces, L = M.mixed_templates()
    _, want = _check(dev, 'mixed', points, faces, max_edge=L, max_rounds=16)
    first = np.bincount(M.one_pass(points, faces, False, L)[2])
    assert set(first.tolist()) == {1, 2, 3, 4}
    assert want.counts['passes'] >= 2


def test_an_edge_of_length_exactly_max_edge_stays(dev):
    points, faces, L = M.exact_length()
    from geobi_gnn_amd import meshsubdiv
    # one round by hand: the plan of round 1 alone (the longer edges need more rounds)
    m_points, m_faces, m_parent, m_vp, m_counts, _ = M.one_pass(points, faces, False, L)
    assert m_counts['split'] == 2
    r = meshsubdiv.subdivide(points, faces, max_edge=L, device=dev)
    first = r.passes[0]
    assert first.counts == m_counts and (first.Vn, first.Fn) == (m_points.shape[0], m_faces.shape[0])
    _check(dev, 'exact', points, faces, max_edge=L)
    # just below L the edge goes
    below = float(np.nextafter(np.float32(L), np.float32(0)))
    _, want = _check(dev, 'exact', points, faces, max_edge=below)
    assert want.per_pass[0]['split'] == 3


@pytest.mark.parametrize('variant', range(4))
def test_the_isosceles_tie_goes_to_the_lower_edge_id(dev, variant):
    points, faces, L = M.isosceles(variant)
    from geobi_gnn_amd import meshsubdiv
    m = M.one_pass(points, faces, False, L)
    assert m[4]['split'] == 2
    got = meshsubdiv.subdivide(points, faces, max_edge=4.0, device=dev)        # the legs (4.03) alone, one round
    want = M.subdivide(points, faces, max_edge=4.0)
    assert want.counts['passes'] == 1 and np.array_equal(want.faces, m[1])
    M.assert_same(_Host(got), want, 'isosceles%d' % variant)


@pytest.mark.parametrize('L, sizes', [(2.5, (16, 28, 1)), (1.2, (50, 96, 2)), (0.5, (242, 480, 4)), (0.2, (1794, 3584, 5))])
def test_box_max_edge_through_its_rounds(dev, L, sizes):
    points, faces = M.box()
    got, want = _check(dev, 'box', points, faces, max_edge=L)
    assert (got.points.shape[0], got.faces.shape[0], got.counts['passes']) == sizes
    assert M.longest_edge2(got.points.cpu().numpy(), got.faces.cpu().numpy()) <= np.float64(np.float32(L)) ** 2


@pytest.mark.parametrize('scheme', ['midpoint', 'loop'])
@pytest.mark.parametrize('mesh', ['icosahedron', 'grid'])
def test_three_levels(dev, mesh, scheme):
    points, faces = M.icosahedron() if mesh == 'icosahedron' else M.grid(7, 5, seed=1)
    got, _ = _check(dev, mesh, points, faces, levels=3, scheme=scheme)
    assert got.faces.shape[0] == 64 * faces.shape[0] and got.counts['passes'] == 3


@pytest.mark.parametrize('scheme', ['midpoint', 'loop'])
def test_apply_with_perturbed_points(dev, scheme):
    from geobi_gnn_amd import meshsubdiv
    points, faces = M.grid(7, 5, seed=1)
    noisy = (points + 0.05 * np.random.RandomState(8).randn(*points.shape)).astype(np.float32)
    got, want = _check(dev, 'grid', points, faces, levels=3, scheme=scheme)
    moved = meshsubdiv.apply(got, noisy)
    assert moved.is_cuda and moved.dtype == torch.float32
    assert np.array_equal(M.bits(moved.cpu().numpy()), M.bits(M.apply(want, noisy)))
    assert not np.array_equal(M.bits(moved.cpu().numpy()), M.bits(want.points))
    with pytest.raises(ValueError):
        meshsubdiv.apply(got, noisy[:-1])


def test_apply_after_max_edge_follows_the_plan_not_the_other_points(dev):
    from geobi_gnn_amd import meshsubdiv
    points, faces, L = M.mixed_templates()
    got, want = _check(dev, 'mixed', points, faces, max_edge=L)
    stretched = (points * np.float32(3.0)).astype(np.float32)
    moved = meshsubdiv.apply(got, stretched)
    assert moved.shape == got.points.shape
    assert np.array_equal(M.bits(moved.cpu().numpy()), M.bits(M.apply(want, stretched)))


@pytest.mark.parametrize('name', ['box', 'grid', 'three_on_an_edge'])
def test_mesh_report_gives_the_same_verdict(dev, name):
    from geobi_gnn_amd import meshsubdiv, meshtopo
    points, faces = {'box': M.box, 'grid': lambda: M.grid(7, 5, seed=1), 'three_on_an_edge': lambda: HAND['three_on_an_edge']}[name]()
    before = meshtopo.mesh_report(points, faces, weld_tol=None, device=dev)
    for kw in ({'levels': 2}, {'levels': 1, 'scheme': 'loop'}, {'max_edge': 0.45 * float(np.sqrt(M.longest_edge2(points, faces)))}):
        r = meshsubdiv.subdivide(points, faces, device=dev, **kw)
        after = meshtopo.mesh_report(r.points, r.faces, weld_tol=None, device=dev)
        for key in ('closed', 'components', 'nonorientable', 'degenerate', 'euler'):
            assert after[key] == before[key], (kw, key)
        assert (after['boundary_edges'] > 0) == (before['boundary_edges'] > 0)
        assert (after['complex_edges'] > 0) == (before['complex_edges'] > 0)
        assert after['vertices_used'] == r.points.shape[0] and after['faces'] == r.faces.shape[0]
        assert r.counts['boundary_edges'] == before['boundary_edges'] and r.counts['complex_edges'] == before['complex_edges']
        assert r.counts['edges'] == before['edges']


def test_max_rounds_is_an_error_and_the_next_call_works(dev):
    from geobi_gnn_amd import _lib as L
    from geobi_gnn_amd import meshsubdiv
    points, faces = M.box()
    with pytest.raises(L.GeobiError, match='max_rounds'):
        meshsubdiv.subdivide(points, faces, max_edge=1.2, max_rounds=1, device=dev)
    _check(dev, 'box', points, faces, max_edge=1.2, max_rounds=2)


def test_bad_arguments(dev):
    from geobi_gnn_amd import meshsubdiv
    points, faces = M.box()
    for kw in ({'levels': 0}, {'scheme': 'sqrt3'}, {'max_edge': 0.0}, {'max_edge': float('nan')}, {'max_rounds': 0},
               {'max_edge': 1.0, 'scheme': 'loop'}, {'max_edge': 1.0, 'levels': 3}):
        with pytest.raises(ValueError):
            meshsubdiv.subdivide(points, faces, device=dev, **kw)
    bad = points.copy()
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match='non-finite'):
        meshsubdiv.subdivide(bad, faces, device=dev)
    with pytest.raises(ValueError):
        meshsubdiv.subdivide(points.reshape(-1, 2), faces, device=dev)


def test_a_face_index_out_of_range_is_refused_before_any_launch(dev):
    from geobi_gnn_amd import meshsubdiv
    points, faces = M.box()
    for value in (8, -1, 2 ** 32 + 1):
        bad = faces.astype(np.int64)
        bad[5, 2] = value
        with pytest.raises(ValueError, match='outside'):
            meshsubdiv.subdivide(points, bad, device=dev)
        with pytest.raises(ValueError, match='outside'):
            meshsubdiv.subdivide(torch.from_numpy(points).to(dev), torch.from_numpy(bad).to(dev))


def test_no_faces(dev):
    from geobi_gnn_amd import meshsubdiv
    points = M.box()[0]
    for kw in ({'levels': 2}, {'max_edge': 0.5}):
        r = meshsubdiv.subdivide(points, np.zeros((0, 3), dtype=np.int32), device=dev, **kw)
        assert r.counts == {'edges': 0, 'split': 0, 'boundary_edges': 0, 'complex_edges': 0, 'passes': 0}
        assert r.faces.shape == (0, 3) and r.face_parent.shape == (0,) and r.passes == []
        assert np.array_equal(M.bits(r.points.cpu().numpy()), M.bits(points))
        assert r.vertex_parents.cpu().numpy().tolist() == [[v, v] for v in range(8)]
        assert np.array_equal(M.bits(meshsubdiv.apply(r, points).cpu().numpy()), M.bits(points))


def test_two_calls_are_bit_identical(dev):
    from geobi_gnn_amd import meshsubdiv
    points, faces = M.grid(24, 20, seed=6)
    for kw in ({'levels': 2, 'scheme': 'loop'}, {'max_edge': 0.3}):
        a, b = (meshsubdiv.subdivide(points, faces, device=dev, **kw) for _ in range(2))
        assert a.counts == b.counts
        for field in ('points', 'faces', 'face_parent', 'vertex_parents'):
            assert torch.equal(getattr(a, field).view(torch.int32), getattr(b, field).view(torch.int32)), field


def test_subdivide_command(dev, tmp_path):
    from geobi_gnn_amd import meshio
    root = str(tmp_path)
    os.makedirs(os.path.join(root, 'original'))
    os.makedirs(os.path.join(root, 'noisy'))
    points, faces = M.box()
    g_points, g_faces = M.grid(5, 4, seed=9)
    rng = np.random.RandomState(1)
    noisy = (points + 0.01 * rng.randn(*points.shape)).astype(np.float32)
    meshio.write_obj(os.path.join(root, 'original', 'box.obj'), points, faces)
    meshio.write_obj(os.path.join(root, 'noisy', 'box_n1.obj'), noisy, faces)
    meshio.write_obj(os.path.join(root, 'noisy', 'box_n2.obj'), g_points, g_faces)          # another size: skipped
    run = _run(['subdivide', '--data_dir', root, '--max_edge_diag', '0.3'])
    assert run.returncode == 1 and 'differ in size' in run.stderr and '1 files skipped' in run.stderr
    # the files as the command read them
    points, faces = meshio.read_obj(os.path.join(root, 'original', 'box.obj'))
    noisy = meshio.read_obj(os.path.join(root, 'noisy', 'box_n1.obj'))[0]
    L = 0.3 * float(np.sqrt(14.0))
    want = M.subdivide(points, faces, max_edge=L)
    out = os.path.join(root, 'subdivided')
    o_points, o_faces = meshio.read_obj(os.path.join(out, 'original', 'box.obj'))
    n_points, n_faces = meshio.read_obj(os.path.join(out, 'noisy', 'box_n1.obj'))
    assert not os.path.exists(os.path.join(out, 'noisy', 'box_n2.obj'))
    assert np.array_equal(o_faces, want.faces) and np.array_equal(n_faces, want.faces)
    assert np.array_equal(M.bits(o_points), M.bits(want.points))              # write_obj -> read_obj keeps a float32
    assert np.array_equal(M.bits(n_points), M.bits(M.apply(want, noisy)))
    lines = [l for l in run.stdout.splitlines() if l.startswith('V:')]
    pattern = (r"^V: +8 -> +%d,  F: +12 -> +%d,  edges: 18,  split: %d,  boundary: 0,  complex: 0,  passes: %d,  '%%s'$"
               % (want.points.shape[0], want.faces.shape[0], want.counts['split'], want.counts['passes']))
    assert len(lines) == 2 and re.match(pattern % r'box\.obj', lines[0]) and re.match(pattern % r'box_n1\.obj', lines[1]), lines
    # a plain folder, uniform Loop passes
    plain = os.path.join(root, 'plain')
    os.makedirs(plain)
    meshio.write_obj(os.path.join(plain, 'grid.obj'), g_points, g_faces)
    run = _run(['subdivide', '--data_dir', plain, '--out_dir', os.path.join(root, 'loop'), '--levels', '2', '--scheme', 'loop'])
    assert run.returncode == 0
    g_points, g_faces = meshio.read_obj(os.path.join(plain, 'grid.obj'))
    want = M.subdivide(g_points, g_faces, levels=2, scheme='loop')
    assert np.array_equal(meshio.read_obj(os.path.join(root, 'loop', 'grid.obj'))[1], want.faces)
