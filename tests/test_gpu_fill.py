"""Hole filling on the device (csrc/fill.hip, geobi_gnn_amd/meshfill.py) against the plain statement of
tests/fill_model.py, and the `fill` command end to end.

Every comparison is EXACT: faces, loop numbers, ranks, the loop tables and the counts equal as integers, the points equal as
uint32 bit patterns.  There are no tolerances."""
import os
import re

import numpy as np
import pytest
import torch

import fill_model as M
from train_cases import _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


class _HostLoops(object):
    def __init__(self, loops):
        for field in M.LOOP_FIELDS:
            t = getattr(loops, field)
            assert t.is_cuda and t.is_contiguous(), field
            setattr(self, field, t.cpu().numpy())
        self.counts = loops.counts


class _Host(object):
    """a device result as numpy arrays"""

    def __init__(self, r):
        for field in ('points', 'faces', 'new_vertex_loop', 'new_face_loop'):
            t = getattr(r, field)
            assert t.is_cuda and t.is_contiguous(), field
            setattr(self, field, t.cpu().numpy())
        self.counts, self.loops = r.counts, _HostLoops(r.loops)


_MODELS = {}


def _check(dev, name, points, faces, max_hole_edges=0):
    """fill_holes and boundary_loops on the device against the model (computed once per named input), everything exact;
    apply with the input's points must reproduce the output bit for bit -> (device result, model result)"""
    from geobi_gnn_amd import meshfill
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    key = (name, max_hole_edges)
    if key not in _MODELS:
        _MODELS[key] = M.fill_holes(points, faces, max_hole_edges)
    want = _MODELS[key]
    got = meshfill.fill_holes(points, faces, max_hole_edges=max_hole_edges, device=dev)
    M.assert_same(_Host(got), want, name)
    assert (got.V, got.F) == (points.shape[0], faces.shape[0])
    alone = meshfill.boundary_loops(faces, points.shape[0], device=dev)
    M.assert_same_loops(_HostLoops(alone), want.loops, name + ': boundary_loops')
    again = meshfill.apply(got, points)
    assert np.array_equal(M.bits(again.cpu().numpy()), M.bits(want.points)), name + ': apply(input points)'
    return got, want


RIMS = [3, 4, 5, 63, 64, 65, 128, 129, 257, 1025]


@pytest.mark.parametrize('n', RIMS)
def test_cups_across_the_lane_stride_and_the_powers_of_two(dev, n):
    """the rim numbered in order and shuffled (the leader is then not next to its successor in memory), with plain
    coordinates and with full 24-bit mantissas whose sum shows its order"""
    for shuffle in (None, 7):
        for mantissa in (None, 9):
            points, faces = M.cup(n, shuffle=shuffle, mantissa=mantissa)
            _, want = _check(dev, 'cup%d-%s-%s' % (n, shuffle, mantissa), points, faces)
            assert want.counts['loops'] == 1 and want.counts['longest_loop'] == n and want.counts['new_faces'] == n


def test_300_triangular_holes_in_one_sphere(dev):
    """more loops than one block of the loop tables and their scans"""
    points, faces = M.sphere_without_faces(16, 300)
    _, want = _check(dev, 'sphere300', points, faces)
    assert want.counts == dict(boundary_edges=900, blocked_vertices=0, chain_edges=0, loops=300, longest_loop=3,
                               filled_loops=300, skipped_loops=0, new_faces=900)
    _, want = _check(dev, 'sphere300', points, faces, max_hole_edges=2)
    assert want.counts['filled_loops'] == 0 and want.counts['skipped_loops'] == 300


@pytest.mark.parametrize('rims', [(85, 85, 85), (85, 85, 86), (85, 86, 86)])
def test_rims_of_85_and_86_across_the_block_edges(dev, rims):
    """255 / 256 / 257 faces: the block edges of the face, slot and loop kernels; the limit between the two lengths"""
    points, faces = M.rims_in_one_mesh(rims)
    assert faces.shape[0] == sum(rims)
    _check(dev, 'rims%d' % sum(rims), points, faces)
    _, want = _check(dev, 'rims%d' % sum(rims), points, faces, max_hole_edges=85)
    assert want.counts['filled_loops'] == rims.count(85) and want.counts['skipped_loops'] == rims.count(86)


HAND = M.hand_cases()


@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_cases(dev, name):
    points, faces, counts = HAND[name]
    got, want = _check(dev, name, points, faces)
    assert got.counts == counts


def test_max_hole_edges_at_the_length_and_one_below(dev):
    points, faces, _ = HAND['cup7']
    got, _ = _check(dev, 'cup7', points, faces, max_hole_edges=7)
    assert got.counts['filled_loops'] == 1 and got.faces.shape[0] == 14
    got, _ = _check(dev, 'cup7', points, faces, max_hole_edges=6)
    assert (got.counts['filled_loops'], got.counts['skipped_loops']) == (0, 1)
    assert got.faces.shape[0] == 7 and got.points.shape[0] == 8 and got.new_vertex_loop.shape[0] == 0


def test_one_face_and_no_faces(dev):
    from geobi_gnn_amd import meshfill
    points, faces, _ = HAND['isolated_triangle']
    got, _ = _check(dev, 'isolated_triangle', points, faces)
    assert got.faces.cpu().numpy().tolist() == [[0, 1, 2], [1, 0, 3], [0, 2, 3], [2, 1, 3]]
    r = meshfill.fill_holes(points, np.zeros((0, 3), dtype=np.int32), device=dev)
    assert set(r.counts.values()) == {0} and r.faces.shape == (0, 3) and r.loops.loop.shape == (0,)
    assert np.array_equal(M.bits(r.points.cpu().numpy()), M.bits(points))
    assert np.array_equal(M.bits(meshfill.apply(r, points).cpu().numpy()), M.bits(points))


def test_apply_with_perturbed_and_stretched_points(dev):
    from geobi_gnn_amd import meshfill
    points, faces, _, _ = M.sphere_without_fans(6, 12)
    got, want = _check(dev, 'sphere-fans', points, faces)
    noisy = (points + 0.05 * np.random.RandomState(8).randn(*points.shape)).astype(np.float32)
    stretched = (points * np.float32([3.0, 1.0, 0.25])).astype(np.float32)
    for other in (noisy, stretched):
        moved = meshfill.apply(got, other)
        assert moved.is_cuda and moved.dtype == torch.float32
        assert np.array_equal(M.bits(moved.cpu().numpy()), M.bits(M.apply(want, other)))
        assert not np.array_equal(M.bits(moved.cpu().numpy()), M.bits(want.points))
    with pytest.raises(ValueError):
        meshfill.apply(got, noisy[:-1])
    # a long rim whose sum shows its order
    points, faces = M.cup(257, shuffle=3, mantissa=4)
    got, want = _check(dev, 'cup257-apply', points, faces)
    other = M.full_mantissa(points.shape, 21)
    assert np.array_equal(M.bits(meshfill.apply(got, other).cpu().numpy()), M.bits(M.apply(want, other)))


def test_mesh_report_goes_from_open_to_closed(dev):
    from geobi_gnn_amd import meshfill, meshtopo
    points, faces, _, each = M.sphere_without_fans(6, 12)
    before = meshtopo.mesh_report(points, faces, weld_tol=None, device=dev)
    assert not before['closed'] and before['boundary_edges'] == sum(each)
    r = meshfill.fill_holes(points, faces, device=dev)
    after = meshtopo.mesh_report(r.points, r.faces, weld_tol=None, device=dev)
    assert after['closed'] and after['euler'] == 2 and after['components'] == 1
    for key in ('boundary_edges', 'complex_edges', 'inconsistent_edges', 'nonorientable', 'would_flip', 'degenerate'):
        assert after[key] == 0, key
    assert after['vertices_used'] == r.points.shape[0] - 12 and after['faces'] == r.faces.shape[0]      # the 12 removed ones stay
    # a closed mesh: nothing moves
    points, faces = M.icosphere(4)
    before = meshtopo.mesh_report(points, faces, weld_tol=None, device=dev)
    r = meshfill.fill_holes(points, faces, device=dev)
    assert set(r.counts.values()) == {0}
    assert np.array_equal(r.faces.cpu().numpy(), faces) and np.array_equal(M.bits(r.points.cpu().numpy()), M.bits(points))
    assert meshtopo.mesh_report(r.points, r.faces, weld_tol=None, device=dev) == before and before['closed']


def test_two_calls_are_bit_identical(dev):
    from geobi_gnn_amd import meshfill
    points, faces = M.hemisphere(12)
    a, b = (meshfill.fill_holes(points, faces, device=dev) for _ in range(2))
    assert a.counts == b.counts and a.counts['loops'] == 1 and a.counts['filled_loops'] == 1
    for field in ('points', 'faces', 'new_vertex_loop', 'new_face_loop'):
        assert torch.equal(getattr(a, field).view(torch.int32), getattr(b, field).view(torch.int32)), field
    _check(dev, 'hemisphere12', points, faces)


def test_bad_arguments(dev):
    from geobi_gnn_amd import meshfill
    points, faces, _ = HAND['cup7']
    for value in (-1, 1.5, '3', None):
        with pytest.raises(ValueError, match='max_hole_edges'):
            meshfill.fill_holes(points, faces, max_hole_edges=value, device=dev)
    bad = points.copy()
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match='non-finite'):
        meshfill.fill_holes(bad, faces, device=dev)
    with pytest.raises(ValueError):
        meshfill.fill_holes(points.reshape(-1, 2), faces, device=dev)
    with pytest.raises(ValueError):
        meshfill.boundary_loops(faces.reshape(-1), 8, device=dev)
    for value in (8, -1, 2 ** 32 + 1):
        wrong = faces.astype(np.int64)
        wrong[5, 2] = value
        with pytest.raises(ValueError, match='outside'):
            meshfill.fill_holes(points, wrong, device=dev)
        with pytest.raises(ValueError, match='outside'):
            meshfill.boundary_loops(torch.from_numpy(wrong).to(dev), 8)
    _check(dev, 'cup7', points, faces)                      # and the next call works


def test_a_workspace_that_is_too_small_is_refused(dev):
    from geobi_gnn_amd import _lib as L
    points, faces, _ = HAND['cup7']
    fv = torch.from_numpy(faces).to(dev)
    counts = torch.zeros(16, dtype=torch.int32, device=dev)
    for F, V in ((7, 8), (1, 0), (0, 0), (0, 5)):
        assert L.lib().geobi_fill_ws_bytes(F, V) >= 256, (F, V)
    ws = L.workspace(256, dev)
    with pytest.raises(L.GeobiError, match='workspace too small'):
        L.call('geobi_fill_plan', L.ptr(fv), 7, 8, 0, None, None, None, None, L.ptr(counts), None, L.ptr(ws), ws.numel(),
               L.stream())


def test_fill_command(dev, tmp_path):
    from geobi_gnn_amd import meshio
    root = str(tmp_path)
    os.makedirs(os.path.join(root, 'original'))
    os.makedirs(os.path.join(root, 'noisy'))
    points, faces, _, each = M.sphere_without_fans(4, 5)
    c_points, c_faces, _ = HAND['bow_tie']
    rng = np.random.RandomState(1)
    noisy = (points + 0.01 * rng.randn(*points.shape)).astype(np.float32)
    meshio.write_obj(os.path.join(root, 'original', 'ball.obj'), points, faces)
    meshio.write_obj(os.path.join(root, 'noisy', 'ball_n1.obj'), noisy, faces)
    meshio.write_obj(os.path.join(root, 'noisy', 'ball_n2.obj'), c_points, c_faces)        # another size: skipped
    run = _run(['fill', '--data_dir', root])
    assert run.returncode == 1 and 'differ in size' in run.stderr and '1 files skipped' in run.stderr
    # the files as the command read them
    points, faces = meshio.read_obj(os.path.join(root, 'original', 'ball.obj'))
    noisy = meshio.read_obj(os.path.join(root, 'noisy', 'ball_n1.obj'))[0]
    want = M.fill_holes(points, faces)
    out = os.path.join(root, 'filled')
    o_points, o_faces = meshio.read_obj(os.path.join(out, 'original', 'ball.obj'))
    n_points, n_faces = meshio.read_obj(os.path.join(out, 'noisy', 'ball_n1.obj'))
    assert not os.path.exists(os.path.join(out, 'noisy', 'ball_n2.obj'))
    assert np.array_equal(o_faces, want.faces) and np.array_equal(n_faces, want.faces)
    assert np.array_equal(M.bits(o_points), M.bits(want.points))              # write_obj -> read_obj keeps a float32
    assert np.array_equal(M.bits(n_points), M.bits(M.apply(want, noisy)))
    lines = [l for l in run.stdout.splitlines() if l.startswith('V:')]
    pattern = (r"^V: +%d -> +%d,  F: +%d -> +%d,  boundary: %d,  loops: 5,  filled: 5,  skipped: 0,  blocked: 0,  chain: 0,  '%%s'$"
               % (points.shape[0], want.points.shape[0], faces.shape[0], want.faces.shape[0], sum(each)))
    assert len(lines) == 2 and re.match(pattern % r'ball\.obj', lines[0]) and re.match(pattern % r'ball_n1\.obj', lines[1]), lines
    # a plain folder with a limit, and the hint on a mesh with a blocked vertex
    plain = os.path.join(root, 'plain')
    os.makedirs(plain)
    meshio.write_obj(os.path.join(plain, 'ball.obj'), points, faces)
    meshio.write_obj(os.path.join(plain, 'tie.obj'), c_points, c_faces)
    run = _run(['fill', '--data_dir', plain, '--out_dir', os.path.join(root, 'some'), '--max_hole_edges', '5'])
    assert run.returncode == 0
    want = M.fill_holes(points, faces, max_hole_edges=5)
    assert 0 < want.counts['filled_loops'] < 5
    assert np.array_equal(meshio.read_obj(os.path.join(root, 'some', 'ball.obj'))[1], want.faces)
    lines = [l for l in run.stdout.splitlines() if l.startswith('V:')]
    assert len(lines) == 2 and 'filled: %d,  skipped: %d,' % (want.counts['filled_loops'], want.counts['skipped_loops']) in lines[0]
    assert not lines[0].endswith('first') and 'blocked: 1,  chain: 6,' in lines[1]
    assert lines[1].endswith("'tie.obj',  run clean --orient first")
    assert np.array_equal(meshio.read_obj(os.path.join(root, 'some', 'tie.obj'))[1], c_faces)
