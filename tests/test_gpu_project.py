"""Closest points on given faces (csrc/project.hip), the guarded move (geobi_move_to of csrc/remesh.hip), their Python
layer (geobi_gnn_amd/meshproject.py, meshremesh.remesh(project=True)) and the two commands on the device, against the plain
statement of tests/project_model.py.

Every comparison with the model is EXACT -- faces and counts as integers, weights, points and distances as uint32 bit
patterns -- GIVEN the faces the device search returned: which of two faces that meet at the closest edge is returned is the
fp32 search's own choice, so the returned face is judged by the bar of tests/test_gpu_mesheval.py (TOL) and everything
behind it bit for bit."""
import os
import re

import numpy as np
import pytest
import torch

import decim_model as D
import project_model as P
import remesh_model as R
import subdiv_model as S
import test_gpu_workspace as W
from train_cases import _run

pytestmark = pytest.mark.gpu
F32 = np.float32
TOL = 1e-5                      # tests/test_gpu_mesheval.py


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


def _rel(d, d_ref, e):          # tests/test_gpu_mesheval.py: _rel
    return float((np.abs(np.asarray(d, dtype=np.float64) - d_ref) / (d_ref + e)).max())


def _t(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


class _Host(object):
    """a device Closest as numpy arrays"""

    def __init__(self, c):
        for field in ('face', 'bary', 'points', 'dist'):
            t = getattr(c, field)
            assert t.is_cuda and t.is_contiguous(), field
            setattr(self, field, t.cpu().numpy())


class _HostMesh(object):
    """a device Remeshed as numpy arrays"""

    def __init__(self, r):
        self.points, self.faces = r.points.cpu().numpy(), r.faces.cpu().numpy()
        self.per_iteration, self.before, self.after = r.per_iteration, r.before, r.after
        self.source_face = None if r.source_face is None else r.source_face.cpu().numpy()
        self.source_bary = None if r.source_bary is None else r.source_bary.cpu().numpy()


def _on_faces(dev, q, verts, faces, face):
    """geobi_closest_on_faces with the faces given -> a host object with the fields of a Closest"""
    from geobi_gnn_amd import meshproject
    bary, points, dist = meshproject.closest_on_faces(_t(q, dev), _t(verts, dev), _t(faces, dev, torch.int32),
                                                      _t(face, dev, torch.int32))
    assert bary.dtype == points.dtype == dist.dtype == torch.float32
    return P.Closest(np.asarray(face, dtype=np.int32), bary.cpu().numpy(), points.cpu().numpy(), dist.cpu().numpy(), None)


def _device_search(dev):
    def search(q, verts, faces):
        from geobi_gnn_amd import mesheval
        return mesheval.point_to_mesh(_t(q, dev), _t(verts, dev), _t(faces, dev, torch.int32))[1].cpu().numpy()
    return search


# ---- closest points on given faces
def test_hand_triangle_and_triangles_without_area(dev):
    tri = np.array([[0, 1, 2]], dtype=np.int32)
    q = np.array([(x, y, z) for x, y, _, _, _ in P.hand_queries() for z in (0.0, 2.0, -3.0)], dtype=F32)
    want = P.closest(q, P.HAND_TRIANGLE, tri, face=np.zeros(len(q), dtype=np.int32))
    assert want.regions == [r for _, _, r, _, _ in P.hand_queries() for _ in range(3)]
    P.assert_same_closest(_on_faces(dev, q, P.HAND_TRIANGLE, tri, want.face), want, 'hand')
    q = P.degenerate_queries()
    for name, verts in sorted(P.degenerate_triangles().items()):
        want = P.closest(q, verts, tri, face=np.zeros(len(q), dtype=np.int32))
        got = _on_faces(dev, q, verts, tri, want.face)
        P.assert_same_closest(got, want, name)
        assert np.isfinite(got.bary).all() and (got.bary >= 0).all() and (got.bary <= 1).all()


_ICO = {}


def _ico():
    if not _ICO:
        points, faces = D.icosphere(4)
        _ICO.update(points=points, faces=faces, e=R.mean_edge(points, faces), q=P.shell_queries(513, seed=7))
    return _ICO


@pytest.mark.parametrize('Q', [1, 255, 256, 257, 513])
def test_sphere_queries_across_the_block_edges(dev, Q):
    """queries at 0.7 .. 1.3 radii on the 320-face icosphere, at the origin and shifted by (50, -30, 20) mean edges: the
    device's face is a nearest one by the project's bar, everything behind it equals the model, bary_points gives the points
    back"""
    from geobi_gnn_amd import meshproject, ops
    c = _ico()
    for shift in (np.zeros(3, dtype=F32), (np.array([50.0, -30.0, 20.0]) * c['e']).astype(F32)):
        q, verts, faces = c['q'][:Q] + shift, c['points'] + shift, c['faces']
        got_dev = meshproject.closest(q, verts, faces, device=dev)
        got = _Host(got_dev)
        assert got.face.dtype == np.int32 and got.face.min() >= 0 and got.face.max() < faces.shape[0]
        want = P.closest(q, verts, faces, face=got.face)
        P.assert_same_closest(got, want, 'Q = %d' % Q)
        d_min = P.distance_to_surface(q, verts, faces)
        at_face = P.distance_to_faces(q, verts, faces, got.face)
        print('Q = %d: rel err at the returned face %.3e, of dist %.3e' % (Q, _rel(at_face, d_min, c['e']), _rel(got.dist, d_min, c['e'])))
        assert _rel(at_face, d_min, c['e']) <= TOL and _rel(got.dist, d_min, c['e']) <= TOL
        assert P.distance_to_faces(got.points, verts, faces, got.face).max() <= P.surface_bound(verts)
        again = ops.bary_points(_t(verts, dev), got_dev.faces, got_dev.face, got_dev.bary)
        assert torch.equal(again.view(torch.int32), got_dev.points.view(torch.int32))
        assert torch.equal(meshproject.apply(got_dev, verts).view(torch.int32), got_dev.points.view(torch.int32))


def test_a_mesh_projected_onto_itself_stays(dev):
    from geobi_gnn_amd import meshproject
    c = _ico()
    got = _Host(meshproject.closest(c['points'], c['points'], c['faces'], device=dev))
    assert (got.points == c['points']).all() and not got.dist.any()
    assert (np.sort(got.bary, axis=1) == np.array([0, 0, 1], dtype=F32)).all()
    P.assert_same_closest(got, P.closest(c['points'], c['points'], c['faces'], face=got.face), 'self')


def test_exceptions_and_a_guard_band_around_the_outputs(dev):
    """a face outside [0, F), queries that are not finite, ids to clamp; the three outputs lie inside one buffer of
    sentinels, and no byte outside them changes"""
    from geobi_gnn_amd import _lib as L
    points, faces = D.icosphere(2)
    q = np.concatenate([np.array([[0.1, 0.2, 2.0], [np.nan, 0, 0], [0, np.inf, 0], [0.3, 0.3, 0.3], [0.5, 0, 0], [0, -np.inf, np.nan]],
                                 dtype=F32), P.shell_queries(251, seed=9)])
    Q = q.shape[0]
    assert Q == 257
    face = (np.arange(Q) % faces.shape[0]).astype(np.int32)
    face[3], face[4] = -1, faces.shape[0]
    wild = faces.copy()
    wild[0], wild[1] = (0, 1, 99), (-5, 1, 2)
    want = P.closest(q, points, wild, face=face)
    assert not want.bary[3:5].any() and np.isinf(want.dist[[1, 2, 5]]).all() and (want.bary[[1, 2, 5]] == F32([1, 0, 0])).all()
    P.assert_same_closest(_on_faces(dev, q, points, wild, face), want, 'exceptions')
    pad = 1024                                                     # floats of sentinel before, between and behind
    buf = torch.full((4 * pad + 7 * Q,), float('nan'), dtype=torch.float32, device=dev)
    buf.view(torch.int32).fill_(0x5A5A5A5A)
    before = buf.clone()
    at = [pad, 2 * pad + 3 * Q, 3 * pad + 6 * Q]
    bary, pts, dist = buf[at[0]:at[0] + 3 * Q].view(Q, 3), buf[at[1]:at[1] + 3 * Q].view(Q, 3), buf[at[2]:at[2] + Q]
    ins = (_t(q, dev), _t(points, dev), _t(wild, dev, torch.int32), _t(face, dev, torch.int32))       # alive over the call
    L.call('geobi_closest_on_faces', L.ptr(ins[0]), L.ptr(ins[1]), L.ptr(ins[2]), L.ptr(ins[3]), Q, points.shape[0],
           faces.shape[0], L.ptr(bary), L.ptr(pts), L.ptr(dist), L.stream())
    torch.cuda.synchronize()
    got = P.Closest(face, bary.cpu().numpy(), pts.cpu().numpy(), dist.cpu().numpy(), None)
    P.assert_same_closest(got, want, 'inside the guard band')
    outside = torch.ones_like(buf, dtype=torch.bool)
    for start, n in zip(at, (3 * Q, 3 * Q, Q)):
        outside[start:start + n] = False
    assert torch.equal(buf.view(torch.int32)[outside], before.view(torch.int32)[outside]), 'a byte outside the outputs changed'


def test_bad_arguments_raise(dev):
    from geobi_gnn_amd import meshproject, meshremesh
    points, faces = D.icosphere(2)
    q = P.shell_queries(5)
    bad = points.copy()
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match='non-finite'):
        meshproject.closest(q, bad, faces, device=dev)
    with pytest.raises(ValueError, match='at least one'):
        meshproject.closest(q, points, np.zeros((0, 3), dtype=np.int32), device=dev)
    for value in (points.shape[0], -1, 2 ** 32 + 1):
        wrong = faces.astype(np.int64)
        wrong[5, 2] = value
        with pytest.raises(ValueError, match='outside'):
            meshproject.project(q, points, wrong, device=dev)
    c = meshproject.closest(q, points, faces, device=dev)
    with pytest.raises(ValueError, match='apply'):
        meshproject.apply(c, points[:-1])
    with pytest.raises(ValueError, match='target'):
        meshremesh.move_to(points, faces, points[:-1], device=dev)
    with pytest.raises(ValueError, match='lock'):
        meshremesh.move_to(points, faces, points, lock=np.zeros(5, dtype=np.int32), device=dev)
    with pytest.raises(ValueError, match='project'):
        meshremesh.remesh(points, np.zeros((0, 3), dtype=np.int32), target_edge=1.0, project=True, device=dev)
    r = meshremesh.remesh(points, faces, iterations=1, device=dev)
    with pytest.raises(ValueError, match='no map'):
        meshremesh.apply(r, points)
    r = meshremesh.remesh(points, faces, iterations=1, project=True, device=dev)
    with pytest.raises(ValueError, match='apply'):
        meshremesh.apply(r, points[:-1])


def test_project_keeps_the_rows_beyond_max_dist(dev):
    from geobi_gnn_amd import meshproject
    c = _ico()
    q = c['q'][:300].copy()
    q[7] = np.nan
    out, kept, closest = meshproject.project(q, c['points'], c['faces'], max_dist=0.1, device=dev)
    out, dist, pts = out.cpu().numpy(), closest.dist.cpu().numpy(), closest.points.cpu().numpy()
    far = ~(dist <= F32(0.1))
    assert kept == int(far.sum()) and far[7] and 20 < kept < 280
    assert np.array_equal(P.bits(out[far]), P.bits(q[far])) and np.array_equal(P.bits(out[~far]), P.bits(pts[~far]))
    out, kept, _ = meshproject.project(q, c['points'], c['faces'], device=dev)
    assert kept == 1 and np.array_equal(P.bits(out.cpu().numpy()[7]), P.bits(q[7]))


# ---- move_to
def _move_to(dev, name, points, faces, target, lock):
    from geobi_gnn_amd import meshremesh
    want = P.move_to(points, faces, target, lock)
    got, counts = meshremesh.move_to(points, faces, target, lock=lock, device=dev)
    assert got.dtype == torch.float32 and got.shape == (points.shape[0], 3)
    P.assert_same_move((got.cpu().numpy(), counts), want, name)
    return want


def test_move_to_refuses_and_reverts_on_the_noisy_sphere(dev):
    points, faces, target, lock = P.noisy_sphere(P.NOISY_SPHERE_SEED)
    _, counts = _move_to(dev, 'noisy sphere', points, faces, target, lock)
    assert counts['refused'] > 0 and counts['reverted'] > 0
    lock[:40] = 1
    target[50] = np.nan
    target[51, 2] = np.inf
    _move_to(dev, 'noisy sphere, locks and proposals that are not finite', points, faces, target, lock)
    # the lock flags computed by the call itself
    from geobi_gnn_amd import meshremesh
    got, counts = meshremesh.move_to(points, faces, target, feature_angle=180.0, device=dev)
    P.assert_same_move((got.cpu().numpy(), counts), P.move_to(points, faces, target, np.zeros_like(lock)), 'no lock given')


def test_move_to_on_the_flat_grid_keeps_the_plane_and_the_rim(dev):
    """the jittered grid, lifted off its plane, projected onto the flat grid: z is exactly 0 again and the rim stays"""
    from geobi_gnn_amd import meshproject
    points, faces, flat, lock = P.lifted_grid(8)
    closest = _Host(meshproject.closest(points, flat, faces, device=dev))
    P.assert_same_closest(closest, P.closest(points, flat, faces, face=closest.face), 'grid')
    out, counts = _move_to(dev, 'lifted grid', points, faces, closest.points, lock)
    assert not out[:, 2].any() and (P.bits(out[lock != 0]) == P.bits(points[lock != 0])).all()
    assert counts['moved'] > 30 and counts['refused'] == counts['reverted'] == 0


@pytest.mark.parametrize('n_faces', [255, 256, 257])
def test_move_to_on_strips_moves_nothing(dev, n_faces):
    """F across 256; every vertex is on the boundary and locked"""
    points, faces = S.strip(n_faces)
    lock = R.lock_flags(points, faces, 180.0)[0]
    target = (points + F32(0.01)).astype(F32)
    out, counts = _move_to(dev, 'strip%d' % n_faces, points, faces, target, lock)
    assert counts == dict.fromkeys(R.RELAX_KEYS, 0) and np.array_equal(P.bits(out), P.bits(points))
    # without the flags: no vertex of a strip has more than 4 neighbours, the ends have 2
    _move_to(dev, 'strip%d unlocked' % n_faces, points, faces, target, np.zeros_like(lock))


def test_move_to_without_faces_and_with_a_short_workspace(dev, monkeypatch):
    from geobi_gnn_amd import _lib as L
    from geobi_gnn_amd import meshremesh
    points, none = S.box()[0], np.zeros((0, 3), dtype=np.int32)
    got, counts = meshremesh.move_to(points, none, points + 1, device=dev)
    assert counts == dict.fromkeys(R.RELAX_KEYS, 0) and np.array_equal(P.bits(got.cpu().numpy()), P.bits(points))
    pts, out = torch.from_numpy(points).to(dev), torch.zeros((8, 3), dtype=torch.float32, device=dev)
    fv = torch.zeros((1, 3), dtype=torch.int32, device=dev)
    lock = torch.zeros(8, dtype=torch.int32, device=dev)
    cnt = torch.full((4,), -1, dtype=torch.int32, device=dev)
    elsewhere = pts + 1
    L.call('geobi_move_to', L.ptr(fv), L.ptr(pts), L.ptr(elsewhere), L.ptr(lock), 0, 8, L.ptr(out), L.ptr(cnt), None, None, 0,
           L.stream())
    assert torch.equal(out.view(torch.int32), pts.view(torch.int32)) and L.read_i32(cnt, 4) == [0] * 4
    # the workspace: whole with a guard band, then 512 bytes short
    points, faces, target, lock = P.noisy_sphere(P.NOISY_SPHERE_SEED)
    want = P.move_to(points, faces, target, lock)
    guard = W._Guarded().install(monkeypatch)
    got, counts = meshremesh.move_to(points, faces, target, lock=lock, device=dev)
    assert guard.sentinels_whole() and list(guard.entries.values()) == ['geobi_move_to']
    P.assert_same_move((got.cpu().numpy(), counts), want, 'guarded')
    monkeypatch.undo()
    guard = W._Guarded(short_at=0).install(monkeypatch)
    with pytest.raises(L.GeobiError) as e:
        meshremesh.move_to(points, faces, target, lock=lock, device=dev)
    monkeypatch.undo()
    assert guard.sentinels_whole()
    give, nbytes = guard.requests[0][1:]
    m = re.search(r'geobi_move_to failed: move_to: workspace too small \((\d+) bytes given, (\d+) needed\)', str(e.value))
    assert m and int(m.group(1)) == give and give < int(m.group(2)) <= nbytes, str(e.value)


# ---- the loop with its fifth step
_SPHERES = {}


def _sphere(name):
    if name not in _SPHERES:
        points, faces = R.uv_sphere() if name == 'uv' else D.icosphere(4)
        _SPHERES[name] = (points, faces, (1.0 if name == 'uv' else 0.6) * R.mean_edge(points, faces))
    return _SPHERES[name]


@pytest.mark.parametrize('name', ['uv', 'ico'])
def test_remesh_with_projection_against_the_model(dev, name):
    """the UV sphere at its mean edge, the 320-face icosphere at 0.6 mean edges, no feature edges: points, faces, counts and
    the source map equal the model run with the device's search; two calls give the same bits; without project the call is
    remesh_model.remesh; a noisy copy goes through the map onto its own surface"""
    from geobi_gnn_amd import meshremesh
    points, faces, L = _sphere(name)
    got = meshremesh.remesh(points, faces, target_edge=L, feature_angle=180.0, project=True, device=dev)
    want = P.remesh(points, faces, L, feature_angle=180.0, project=True, nearest_face=_device_search(dev))
    host = _HostMesh(got)
    P.assert_same(host, want, name)
    assert set(got.per_iteration[0]) == set(meshremesh.ITERATION_KEYS + meshremesh.PROJECT_KEYS)
    last = got.per_iteration[-1]
    assert last['projected'] > 0 and last['project_refused'] == 0 and last['project_reverted'] == 0
    assert R.closed_manifold(host.faces) and R.euler(0, host.faces) == 2
    drift = P.distance_to_surface(host.points, points, faces)
    assert drift.max() <= P.surface_bound(points)
    again = meshremesh.remesh(points, faces, target_edge=L, feature_angle=180.0, project=True, device=dev)
    assert again.per_iteration == got.per_iteration and again.after == got.after
    for field in ('points', 'faces', 'source_face', 'source_bary'):
        assert torch.equal(getattr(again, field).view(torch.int32), getattr(got, field).view(torch.int32)), field
    # the map on a paired array
    noisy = (points + 0.02 * np.random.RandomState(2).randn(*points.shape)).astype(F32)
    carried = meshremesh.apply(got, noisy).cpu().numpy()
    assert carried.dtype == F32 and np.array_equal(P.bits(carried), P.bits(P.apply(want, faces, noisy)))
    assert P.distance_to_faces(carried, noisy, faces, host.source_face).max() <= P.surface_bound(noisy)
    # the default path
    plain = meshremesh.remesh(points, faces, target_edge=L, feature_angle=180.0, iterations=2, device=dev)
    R.assert_same(_HostMesh(plain), R.remesh(points, faces, L, iterations=2, feature_angle=180.0), name + ' without project')
    assert plain.source_face is None and plain.source_bary is None
    assert all(tuple(c) == meshremesh.ITERATION_KEYS for c in plain.per_iteration)
    assert P.distance_to_surface(plain.points.cpu().numpy(), points, faces).max() > drift.max()


def test_the_fifth_step_runs_under_the_lock_flags_of_the_relaxation(dev):
    """the bumpy sphere at the default 40 degrees, where the flags taken after the relaxation differ from those it ran under:
    the device equals the model that carries the relaxation's own flags, and not the one that takes them afterwards"""
    from geobi_gnn_amd import meshremesh
    points, faces = P.bumpy_sphere()
    L = R.mean_edge(points, faces)
    got = _HostMesh(meshremesh.remesh(points, faces, target_edge=L, iterations=2, project=True, device=dev))
    want = P.remesh(points, faces, L, iterations=2, feature_angle=40.0, project=True, nearest_face=_device_search(dev))
    assert sum(int((before != after).sum()) for before, after in want.locks) > 0
    P.assert_same(got, want, 'bumpy sphere')
    wrong = P.remesh(points, faces, L, iterations=2, feature_angle=40.0, project=True, nearest_face=_device_search(dev),
                     faults=('relock',))
    with pytest.raises(AssertionError):
        P.assert_same(got, wrong, 'relock')


def test_no_iterations_give_the_identity_map(dev):
    from geobi_gnn_amd import meshremesh
    points, faces, L = _sphere('ico')
    r = meshremesh.remesh(points, faces, target_edge=L, iterations=0, project=True, device=dev)
    assert r.per_iteration == [] and np.array_equal(P.bits(r.points.cpu().numpy()), P.bits(points))
    assert (np.sort(r.source_bary.cpu().numpy(), axis=1) == np.array([0, 0, 1], dtype=F32)).all()
    other = np.random.RandomState(3).randn(*points.shape).astype(F32)
    assert (meshremesh.apply(r, other).cpu().numpy() == other).all()


def test_remesh_with_projection_keeps_features_and_boundaries(dev):
    """locked vertices stay under the projection too, and are part of the map: the dyadic box at 40 degrees, an open grid"""
    from geobi_gnn_amd import meshremesh
    for name, (points, faces), L, angle in (('box', D.dyadic_box(), 0.3, 40.0), ('grid', S.grid(9, 7, seed=1), 1.4, 40.0)):
        got = meshremesh.remesh(points, faces, target_edge=L, iterations=2, feature_angle=angle, project=True, device=dev)
        want = P.remesh(points, faces, L, iterations=2, feature_angle=angle, project=True, nearest_face=_device_search(dev))
        P.assert_same(_HostMesh(got), want, name)
        assert got.source_face.shape[0] == got.points.shape[0]
        assert sum(c['projected'] for c in got.per_iteration) > 0


# ---- the commands
def test_project_and_remesh_project_commands(dev, tmp_path):
    from geobi_gnn_amd import meshio
    root = str(tmp_path)
    for sub in ('original', 'noisy', 'moved'):
        os.makedirs(os.path.join(root, sub))
    points, faces = D.icosphere(4)
    noisy = (points + 0.02 * np.random.RandomState(4).randn(*points.shape)).astype(F32)
    meshio.write_obj(os.path.join(root, 'original', 'ball.obj'), points, faces)
    meshio.write_obj(os.path.join(root, 'noisy', 'ball_n1.obj'), noisy, faces)
    meshio.write_obj(os.path.join(root, 'noisy', 'ball_n2.obj'), *D.icosphere(2))                  # another size: refused
    with open(os.path.join(root, 'original', 'broken.obj'), 'w') as f:
        f.write('v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 9\n')
    L = 0.6 * R.mean_edge(points, faces)
    run = _run(['remesh', '--data_dir', root, '--target_edge', repr(L), '--iterations', '2', '--feature_angle', '180', '--project'])
    assert run.returncode == 1, run.stderr
    assert 'not carried along' not in run.stdout and 'projected' in run.stdout
    assert run.stderr.count('skipped: ') == 2 and '2 files skipped' in run.stderr
    out = os.path.join(root, 'remeshed')
    points, faces = meshio.read_obj(os.path.join(root, 'original', 'ball.obj'))                    # the files as the command read them
    noisy = meshio.read_obj(os.path.join(root, 'noisy', 'ball_n1.obj'))[0]
    want = P.remesh(points, faces, L, iterations=2, feature_angle=180.0, project=True, nearest_face=_device_search(dev))
    o_points, o_faces = meshio.read_obj(os.path.join(out, 'original', 'ball.obj'))
    R.assert_same_mesh(o_points, o_faces.astype(np.int32), want.points, want.faces, 'remesh --project')
    n_points, n_faces = meshio.read_obj(os.path.join(out, 'noisy', 'ball_n1.obj'))
    R.assert_same_mesh(n_points, n_faces.astype(np.int32), P.apply(want, faces, noisy), want.faces, 'carried')
    assert not os.path.exists(os.path.join(out, 'noisy', 'ball_n2.obj')) and not os.path.exists(os.path.join(out, 'original', 'broken.obj'))
    lines = [l for l in run.stdout.splitlines() if l.startswith('V:')]
    assert len(lines) == 2 and lines[0].endswith("'ball.obj'") and lines[1].endswith("'ball_n1.obj'")
    m = re.search(r'drift mean: (\S+),  max: (\S+),', lines[0])
    # the printed drift is the fp32 search's distance: within the project's bar of the true one, which is within the bound
    bound = P.surface_bound(points)
    assert m and 0.0 <= float(m.group(1)) <= float(m.group(2)) <= bound + TOL * (bound + R.mean_edge(points, faces))
    # `project`: the noisy sphere and a far copy onto the clean one, a source that does not parse
    meshio.write_obj(os.path.join(root, 'moved', 'ball_n1.obj'), noisy, faces)
    meshio.write_obj(os.path.join(root, 'moved', 'ball_far.obj'), noisy + F32(5.0), faces)
    with open(os.path.join(root, 'moved', 'ball_bad.obj'), 'w') as f:
        f.write('v 0 0 0\nf 1 2 3\n')
    run = _run(['project', '--data_dir', os.path.join(root, 'moved'), '--target_dir', os.path.join(root, 'original'),
                '--max_dist', '0.5'])
    assert run.returncode == 1 and '1 of 3 files skipped' in run.stderr, run.stderr
    out = os.path.join(root, 'moved', 'projected')
    p_points, p_faces = meshio.read_obj(os.path.join(out, 'ball_n1.obj'))
    want = P.closest(noisy, points, faces, face=_device_search(dev)(noisy, points, faces))
    R.assert_same_mesh(p_points, p_faces.astype(np.int32), want.points, faces.astype(np.int32), 'project')
    far = meshio.read_obj(os.path.join(out, 'ball_far.obj'))[0]
    assert np.array_equal(P.bits(far), P.bits(meshio.read_obj(os.path.join(root, 'moved', 'ball_far.obj'))[0]))
    lines = [l for l in run.stdout.splitlines() if l.startswith('V:')]
    V = points.shape[0]
    assert len(lines) == 2 and re.match(r"^V: +%d,  kept: +%d,  moved mean: \S+,  max: \S+,  'ball_far\.obj'$" % (V, V), lines[0])
    m = re.match(r"^V: +%d,  kept: +0,  moved mean: (\S+),  max: (\S+),  'ball_n1\.obj'$" % V, lines[1])
    assert m and 0.0 < float(m.group(1)) <= float(m.group(2)) < 0.1
    assert not os.path.exists(os.path.join(out, 'ball_bad.obj'))
