"""Isotropic remeshing on the device (csrc/remesh.hip, geobi_decim_plan_short of csrc/decim.hip,
geobi_gnn_amd/meshremesh.py) against the sequential model of tests/remesh_model.py, and the `remesh` command end to end.

Every comparison is EXACT and made round by round: lock flags, faces and counts equal as integers, the points equal as
uint32 bit patterns.  The one tolerance is that of remesh_model.assert_same for the MEAN edge length of the statistics, a
sum taken in another order."""
import os
import re

import numpy as np
import pytest
import torch

import decim_model as D
import remesh_model as R
import subdiv_model as S
import test_gpu_workspace as W
from train_cases import _run

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


class _Host(object):
    """a device Remeshed as numpy arrays"""

    def __init__(self, r):
        assert r.points.is_cuda and r.points.is_contiguous() and r.faces.is_cuda and r.faces.is_contiguous()
        self.points, self.faces = r.points.cpu().numpy(), r.faces.cpu().numpy()
        self.per_iteration, self.before, self.after = r.per_iteration, r.before, r.after


class _Round(object):
    def __init__(self, faces, counts):
        self.faces, self.counts = faces, counts


def _lock(dev, name, points, faces, angle):
    """lock flags on the device against the model -> the flags (numpy)"""
    from geobi_gnn_amd import meshremesh
    want, want_counts = R.lock_flags(points, faces, angle)
    got, counts = meshremesh.lock_flags(points, faces, feature_angle=angle, device=dev)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), name + ': lock flags'
    assert counts == want_counts, (name, counts, want_counts)
    return want


def _flip_rounds(dev, name, points, faces, angle=180.0, max_rounds=64, stop_after=None):
    """flip rounds to exhaustion (or stop_after rounds: an apex of valence n loses one edge per round), each compared with
    the model and continued from the model's faces -> (faces, rounds)"""
    from geobi_gnn_amd import meshremesh
    for k in range(max_rounds):
        if k == stop_after:
            return faces, k
        lock = _lock(dev, name, points, faces, angle)
        want = R.flip_round(points, faces, lock, angle)
        got, counts = meshremesh.flip_edges(points, faces, lock=lock, feature_angle=angle, device=dev)
        R.assert_same_round(_Round(got.cpu().numpy(), counts), want, '%s round %d' % (name, k))
        if want.counts['flips'] == 0:
            return faces, k
        faces = want.faces
    raise AssertionError('%s: the flip rounds did not end' % name)


def _collapse_rounds(dev, name, points, faces, L, angle=180.0, max_rounds=64):
    """short-collapse rounds to exhaustion, each compared with the model -> (points, faces, rounds)"""
    from geobi_gnn_amd import meshremesh
    low, high = R.band(L)
    for k in range(max_rounds):
        lock = _lock(dev, name, points, faces, angle)
        want = R.collapse_round(points, faces, low, high, lock)
        g_points, g_faces, counts = meshremesh.collapse_short(points, faces, float(low), float(high), lock=lock, device=dev)
        assert counts == want.counts, ('%s round %d' % (name, k), counts, want.counts)
        if want.counts['collapses'] == 0 and want.counts['not_included'] == 0:
            return points, faces, k
        R.assert_same_mesh(g_points.cpu().numpy(), g_faces.cpu().numpy(), want.points, want.faces, '%s round %d' % (name, k))
        points, faces = want.points, want.faces
        if want.counts['collapses'] == 0:
            return points, faces, k + 1
    raise AssertionError('%s: the collapse rounds did not end' % name)


def _relax(dev, name, points, faces, lam=0.5, angle=180.0, lock=None):
    from geobi_gnn_amd import meshremesh
    lock = _lock(dev, name, points, faces, angle) if lock is None else lock
    want, want_counts = R.relax(points, faces, lock, lam)
    got, counts = meshremesh.relax(points, faces, lock=lock, relax_lambda=lam, device=dev)
    assert got.dtype == torch.float32 and got.shape == (points.shape[0], 3)
    assert counts == want_counts, (name, counts, want_counts)
    assert np.array_equal(R.bits(got.cpu().numpy()), R.bits(want)), '%s: relaxed points differ in %d rows' % (
        name, int((R.bits(got.cpu().numpy()) != R.bits(want)).any(axis=1).sum()))
    return want, want_counts


def _all_steps(dev, name, points, faces, L=None, angle=180.0, stop_after=None):
    points, faces = np.asarray(points, dtype=F32).reshape(-1, 3), np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    L = R.mean_edge(points, faces) * 1.5 if L is None else L
    flipped = _flip_rounds(dev, name, points, faces, angle, stop_after=stop_after)
    collapsed = _collapse_rounds(dev, name, points, faces, L, angle)
    relaxed = _relax(dev, name, points, faces, 0.5, angle)
    return flipped, collapsed, relaxed


HAND = dict(D.hand_cases(), sharp_1_2_3=S.hand_cases()['sharp_1_2_3'], pillow=R.pillow()[:2])


@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_cases(dev, name):
    """a tetrahedron, an octahedron, an icosahedron, one and two triangles, three and four faces on one edge, a duplicated
    face, a face with repeated corners, an unreferenced vertex, the lens whose diagonal exists"""
    points, faces = HAND[name]
    for angle in (180.0, 40.0):
        (_, flip_rounds), _, _ = _all_steps(dev, name, points, faces, angle=angle)
        if name in ('tetrahedron', 'octahedron', 'one_triangle', 'two_consistent', 'two_inconsistent'):
            assert flip_rounds == 0
    if name == 'pillow':
        from geobi_gnn_amd import meshremesh
        lock = R.pillow()[2]
        want = R.flip_round(points, faces, lock, 180.0)
        got, counts = meshremesh.flip_edges(points, faces, lock=lock, feature_angle=180.0, device=dev)
        R.assert_same_round(_Round(got.cpu().numpy(), counts), want, name)
        assert (0, 1) not in want.candidates and want.counts['flips'] == 1


@pytest.mark.parametrize('rim', [85, 86, 128])
def test_bipyramids_at_the_block_edges(dev, rim):
    """255 / 258 / 384 edges: around the 256-lane block edge of the per-edge kernels; apexes of valence `rim`"""
    points, faces = D.bipyramid(rim)
    assert S.edge_facts(faces)['E'] == 3 * rim
    (_, flip_rounds), (_, c_faces, collapse_rounds), _ = _all_steps(dev, 'bipyramid%d' % rim, points, faces, L=1.2, stop_after=3)
    assert flip_rounds >= 1 and collapse_rounds >= 1 and c_faces.shape[0] < faces.shape[0]


def test_hub_of_valence_200_with_a_shuffled_rim(dev):
    """neighbour lists longer than a wave, and not in the order of the walk around the apexes"""
    points, faces = D.bipyramid(200, shuffled=True)
    (_, flip_rounds), (_, _, collapse_rounds), (_, relax_counts) = _all_steps(dev, 'hub200', points, faces, L=1.2, stop_after=3)
    assert flip_rounds >= 1 and collapse_rounds >= 1 and relax_counts['moved'] >= 2


@pytest.mark.parametrize('n_faces', [255, 256, 257])
def test_strips_have_nothing_to_do(dev, n_faces):
    """F across 256; every vertex is on the boundary: target valence 4, every vertex locked"""
    points, faces = S.strip(n_faces)
    (f_faces, _), (c_points, c_faces, collapse_rounds), (relaxed, relax_counts) = _all_steps(dev, 'strip%d' % n_faces, points, faces)
    assert collapse_rounds == 0 and np.array_equal(c_faces, faces) and f_faces.shape == faces.shape
    assert relax_counts == dict.fromkeys(R.RELAX_KEYS, 0) and np.array_equal(R.bits(relaxed), R.bits(points))


@pytest.mark.parametrize('frequency,flips', [(2, 200), (8, 400)])
def test_scrambled_spheres(dev, frequency, flips):
    """icosphere(2) and the 1280-face sphere after random flips: valences 3 .. 12 and more, many rounds"""
    points, faces = R.scramble(*D.icosphere(frequency), flips=flips, seed=frequency)
    lock = np.zeros(points.shape[0], dtype=np.int32)
    start = R.total_deviation(faces, lock)
    out, rounds = _flip_rounds(dev, 'scrambled%d' % frequency, points, faces)
    assert rounds >= 3 and R.total_deviation(out, lock) < start and R.closed_manifold(out)


def test_noisy_sphere_relaxation_refuses_and_reverts(dev):
    points, faces, lock = R.rough_sphere()
    assert faces.shape[0] == 2000
    _, counts = _relax(dev, 'rough_sphere', points, faces, 0.5, lock=lock)
    assert counts['refused'] > 0 and counts['reverted'] > 0
    _flip_rounds(dev, 'rough_sphere', points, faces, 40.0, max_rounds=64)
    _collapse_rounds(dev, 'rough_sphere', points, faces, 1.5 * R.mean_edge(points, faces), 40.0)


def test_flat_grid(dev):
    """the regular grid: nothing flips, nothing moves; the jittered grid relaxes inside its plane; the collapse keeps the
    rim and the area"""
    points, faces = S.grid(8, 8)
    (_, flip_rounds), (c_points, c_faces, _), (_, relax_counts) = _all_steps(dev, 'grid', points, faces, L=1.5, angle=40.0)
    assert flip_rounds == 0 and relax_counts['moved'] == 0 and S.area(c_points, c_faces) == 64.0
    points, faces = R.jittered_grid(8)
    relaxed, counts = _relax(dev, 'jittered_grid', points, faces, 0.5, 40.0)
    assert counts['moved'] > 20 and not relaxed[:, 2].any()
    _flip_rounds(dev, 'jittered_grid', points, faces, 40.0)


@pytest.mark.parametrize('angle', [40.0, 180.0])
def test_dyadic_box(dev, angle):
    from geobi_gnn_amd import meshremesh
    points, faces = D.dyadic_box()
    lock = _lock(dev, 'dyadic_box', points, faces, angle)
    assert int((lock != 0).sum()) == (0 if angle == 180.0 else 12 * 8 - 4)      # 96 edge segments, 8 corners shared by 3
    want = R.remesh(points, faces, 0.3, iterations=2, feature_angle=angle)
    got = meshremesh.remesh(points, faces, target_edge=0.3, iterations=2, feature_angle=angle, device=dev)
    R.assert_same(_Host(got), want, 'dyadic_box %g' % angle)
    if angle == 40.0:
        assert D.volume(want.points, want.faces) == 6.0


_WHOLE = {}


def _whole(scale, iterations):
    if scale not in _WHOLE:
        points, faces = D.icosphere(8)
        L = scale * R.mean_edge(points, faces)
        _WHOLE[scale] = (points, faces, L, R.remesh(points, faces, L, iterations=iterations))
    return _WHOLE[scale]


@pytest.mark.parametrize('scale,iterations', [(1.5, 3), (0.6, 2)])
def test_remesh_the_1280_face_sphere(dev, scale, iterations):
    from geobi_gnn_amd import meshremesh
    points, faces, L, want = _whole(scale, iterations)
    got = meshremesh.remesh(points, faces, target_edge=L, iterations=iterations, device=dev)
    R.assert_same(_Host(got), want, 'sphere %g' % scale)
    assert (np.float32(got.low), np.float32(got.high)) == (want.low, want.high)
    assert want.after['share'] > 0.8 > want.before['share'] and len(got.per_iteration) == iterations
    assert R.closed_manifold(want.faces) and R.euler(0, want.faces) == 2
    if scale == 1.5:
        assert want.per_iteration[0]['collapses'] > 100 and want.per_iteration[0]['flips'] > 0
    else:
        assert want.per_iteration[0]['splits'] > 1000


def test_default_and_diagonal_target(dev):
    """target_edge = None is the mean edge length of meshnoise; target_edge_diag is times the bounding-box diagonal"""
    from geobi_gnn_amd import meshnoise, meshremesh
    points, faces = D.icosphere(4)
    a = meshremesh.remesh(points, faces, iterations=1, device=dev)
    L = meshnoise.MeshGeometry(points, faces, dev).mean_edge
    assert abs(L - R.mean_edge(points, faces)) < 1e-5 * L
    R.assert_same(_Host(a), R.remesh(points, faces, L, iterations=1), 'default target')
    b = meshremesh.remesh(points, faces, target_edge_diag=0.2, iterations=1, device=dev)
    R.assert_same(_Host(b), R.remesh(points, faces, 0.2 * meshremesh.bbox_diagonal(points), iterations=1), 'diagonal target')


@pytest.mark.parametrize('name', ['icosphere4', 'grid', 'three_on_an_edge'])
def test_mesh_report_before_and_after(dev, name):
    from geobi_gnn_amd import meshremesh, meshtopo
    points, faces = {'icosphere4': lambda: D.icosphere(4), 'grid': lambda: S.grid(9, 7, seed=1),
                     'three_on_an_edge': lambda: HAND['three_on_an_edge']}[name]()
    before = meshtopo.mesh_report(points, faces, weld_tol=None, device=dev)
    r = meshremesh.remesh(points, faces, target_edge=1.4 * R.mean_edge(points, faces), iterations=2, device=dev)
    after = meshtopo.mesh_report(r.points, r.faces, weld_tol=None, device=dev)
    for key in ('closed', 'components', 'nonorientable', 'degenerate', 'euler', 'complex_edges'):
        assert after[key] == before[key], key
    assert after['vertices_used'] == r.points.shape[0] and after['faces'] == r.faces.shape[0]
    assert r.before['edges'] == before['edges'] and r.after['edges'] == after['edges']
    if name != 'three_on_an_edge':
        assert sum(c['collapses'] for c in r.per_iteration) > 0 and r.after['share'] > r.before['share']


def test_two_calls_are_bit_identical(dev):
    from geobi_gnn_amd import meshremesh
    points, faces = S.grid(24, 20, seed=6)
    a, b = (meshremesh.remesh(points, faces, target_edge=1.6, iterations=2, device=dev) for _ in range(2))
    assert a.per_iteration == b.per_iteration and a.after == b.after and a.per_iteration[0]['collapses'] > 0
    for field in ('points', 'faces'):
        assert torch.equal(getattr(a, field).view(torch.int32), getattr(b, field).view(torch.int32)), field


def test_errors(dev):
    from geobi_gnn_amd import _lib as L
    from geobi_gnn_amd import meshremesh
    points, faces = D.icosphere(2)
    for kw in ({'target_edge': 1.0, 'target_edge_diag': 0.5}, {'target_edge': 0.0}, {'iterations': -1}, {'feature_angle': 120.0},
               {'relax_lambda': -0.5}, {'max_rounds': 0}):
        with pytest.raises(ValueError, match='remesh: '):
            meshremesh.remesh(points, faces, device=dev, **kw)
    bad = points.copy()
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match='non-finite'):
        meshremesh.remesh(bad, faces, target_edge=0.5, device=dev)
    with pytest.raises(ValueError):
        meshremesh.remesh(points.reshape(-1, 2), faces, target_edge=0.5, device=dev)
    for value in (points.shape[0], -1, 2 ** 32 + 1):
        wrong = faces.astype(np.int64)
        wrong[5, 2] = value
        with pytest.raises(ValueError, match='outside'):
            meshremesh.remesh(points, wrong, target_edge=0.5, device=dev)
        with pytest.raises(ValueError, match='outside'):
            meshremesh.flip_edges(points, wrong, device=dev)
    with pytest.raises(ValueError, match='lock'):
        meshremesh.relax(points, faces, lock=np.zeros(5, dtype=np.int32), device=dev)
    with pytest.raises(ValueError, match='low'):
        meshremesh.collapse_short(points, faces, 1.0, 0.5, device=dev)
    L_edge = 2.5 * R.mean_edge(points, faces)
    with pytest.raises(R.TooManyRounds):
        R.remesh(points, faces, L_edge, iterations=1, max_rounds=1)
    with pytest.raises(L.GeobiError, match='max_rounds'):
        meshremesh.remesh(points, faces, target_edge=L_edge, iterations=1, max_rounds=1, device=dev)
    got = meshremesh.remesh(points, faces, target_edge=L_edge, iterations=1, device=dev)      # and the next call works
    R.assert_same(_Host(got), R.remesh(points, faces, L_edge, iterations=1), 'after the errors')


def test_no_faces(dev):
    from geobi_gnn_amd import _lib as L
    from geobi_gnn_amd import meshremesh
    points, none = S.box()[0], np.zeros((0, 3), dtype=np.int32)
    r = meshremesh.remesh(points, none, target_edge=1.0, iterations=2, device=dev)
    assert r.faces.shape == (0, 3) and np.array_equal(R.bits(r.points.cpu().numpy()), R.bits(points))
    assert r.per_iteration == [dict.fromkeys(R.ITERATION_KEYS, 0)] * 2 and r.after['edges'] == 0 and r.after == r.before
    lock, counts = meshremesh.lock_flags(points, none, device=dev)
    assert lock.tolist() == [0] * 8 and counts == dict.fromkeys(R.LOCK_KEYS, 0)
    assert meshremesh.flip_edges(points, none, device=dev)[1] == dict.fromkeys(R.FLIP_KEYS, 0)
    assert meshremesh.relax(points, none, device=dev)[1] == dict.fromkeys(R.RELAX_KEYS, 0)
    assert meshremesh.collapse_short(points, none, 1.0, 2.0, device=dev)[2]['V'] == 8
    # the entry points themselves with F == 0
    pts = torch.from_numpy(points).to(dev)
    fv = torch.zeros((1, 3), dtype=torch.int32, device=dev)
    lock = torch.full((8,), 7, dtype=torch.int32, device=dev)
    counts = torch.full((8,), -1, dtype=torch.int32, device=dev)
    L.call('geobi_remesh_lock', L.ptr(fv), L.ptr(pts), 0, 8, 1, 0.5, L.ptr(lock), L.ptr(counts), None, 0, L.stream())
    assert lock.tolist() == [0] * 8 and L.read_i32(counts, 4) == [0] * 4
    L.call('geobi_flip_plan', L.ptr(fv), L.ptr(pts), L.ptr(lock), 0, 8, 1, 0.5, L.ptr(counts), None, None, 0, L.stream())
    assert L.read_i32(counts, 5) == [0] * 5
    L.call('geobi_flip_emit', L.ptr(fv), 0, 8, L.ptr(fv), None, 0, L.stream())
    out = torch.zeros_like(pts)
    L.call('geobi_relax', L.ptr(fv), L.ptr(pts), L.ptr(lock), 0, 8, 0.5, L.ptr(out), L.ptr(counts), None, None, 0, L.stream())
    assert torch.equal(out.view(torch.int32), pts.view(torch.int32)) and L.read_i32(counts, 4) == [0] * 4
    L.call('geobi_decim_plan_short', L.ptr(fv), L.ptr(pts), None, 0, 8, 1.0, 2.0, L.ptr(counts), None, None, 0, L.stream())
    assert L.read_i32(counts) == [0, 0, 0, 0, 8, 0, 0, 0]


# ---- the workspaces, in the manner of tests/test_gpu_workspace.py
def _workspace_case(dev):
    from geobi_gnn_amd import meshremesh
    points, faces = D.icosphere(4)
    r = meshremesh.remesh(points, faces, target_edge=1.5 * 0.3, iterations=1, device=dev)
    return [r.points, r.faces, r.per_iteration, r.before, r.after]


def test_guard_band(dev, monkeypatch):
    """No launcher writes behind the size its query gave, and the carve's layout does not change a result."""
    want = W._flat(_workspace_case(dev), [])
    guard = W._Guarded().install(monkeypatch)
    got = W._flat(_workspace_case(dev), [])
    assert all(nbytes > W.SHORT_BY for _, _, nbytes in guard.requests)
    assert set(guard.entries.values()) >= {'geobi_remesh_lock', 'geobi_decim_plan_short', 'geobi_flip_plan', 'geobi_relax',
                                           'geobi_remesh_stats'}
    assert guard.sentinels_whole(), 'a launcher wrote behind its workspace'
    assert got == want, 'outputs differ from the call made with the library allocator'


def test_short_workspace(dev, monkeypatch):
    """every launcher of the call refuses a workspace 512 bytes short of its size, naming itself and both sizes"""
    from geobi_gnn_amd import _lib as L
    guard = W._Guarded().install(monkeypatch)
    _workspace_case(dev)
    entries = dict(guard.entries)
    monkeypatch.undo()
    first = {}
    for k in sorted(entries):
        first.setdefault(entries[k], k)
    assert set(first) >= {'geobi_remesh_lock', 'geobi_decim_plan_short', 'geobi_flip_plan', 'geobi_relax', 'geobi_remesh_stats'}
    for entry, k in sorted(first.items()):
        if not entry.startswith(('geobi_remesh', 'geobi_decim_plan_short', 'geobi_flip', 'geobi_relax')):
            continue
        guard = W._Guarded(short_at=k).install(monkeypatch)
        with pytest.raises(L.GeobiError) as e:
            _workspace_case(dev)
        monkeypatch.undo()
        assert guard.sentinels_whole(), '%s: a launcher wrote behind the end it was given' % entry
        give, nbytes = guard.requests[k][1:]
        m = re.search(r'(\w+): workspace too small \((\d+) bytes given, (\d+) needed\)', str(e.value))
        assert m and 'geobi_' + m.group(1) == entry and entry + ' failed' in str(e.value), str(e.value)
        assert int(m.group(2)) == give and give < int(m.group(3)) <= nbytes
    # flip_emit over a short copy of a plan's workspace
    from geobi_gnn_amd import meshremesh
    points, faces = R.scramble(*D.icosphere(2), flips=50, seed=1)
    pts, fv = torch.from_numpy(points).to(dev), torch.from_numpy(faces).to(dev)
    lock = torch.zeros(pts.shape[0], dtype=torch.int32, device=dev)
    ws, c = meshremesh._flip_plan(fv, pts, lock, 0, 0.0)
    assert c['flips'] > 0
    guard = W._Guarded(short_at=0)
    short = guard(ws.numel(), dev)
    short.copy_(ws[:short.numel()])
    out = torch.empty_like(fv)
    with pytest.raises(L.GeobiError, match=r'geobi_flip_emit failed: flip_emit: workspace too small \(%d bytes given' % short.numel()):
        L.call('geobi_flip_emit', L.ptr(fv), fv.shape[0], pts.shape[0], L.ptr(out), L.ptr(short), short.numel(), L.stream())
    assert guard.sentinels_whole()


def test_remesh_command(dev, tmp_path):
    from geobi_gnn_amd import meshio
    root = str(tmp_path)
    os.makedirs(os.path.join(root, 'original'))
    os.makedirs(os.path.join(root, 'noisy'))
    points, faces = D.icosphere(4)
    meshio.write_obj(os.path.join(root, 'original', 'ball.obj'), points, faces)
    meshio.write_obj(os.path.join(root, 'noisy', 'ball_n1.obj'), points, faces)
    L = 1.5 * R.mean_edge(points, faces)
    run = _run(['remesh', '--data_dir', root, '--target_edge', repr(L), '--iterations', '2'])
    assert run.returncode == 0, run.stderr
    assert run.stdout.count('noisy/ is not carried along') == 1 and '`noise`' in run.stdout
    out = os.path.join(root, 'remeshed')
    assert not os.path.exists(os.path.join(out, 'noisy'))
    points, faces = meshio.read_obj(os.path.join(root, 'original', 'ball.obj'))          # the file as the command read it
    want = R.remesh(points, faces, L, iterations=2)
    o_points, o_faces = meshio.read_obj(os.path.join(out, 'original', 'ball.obj'))
    R.assert_same_mesh(o_points, o_faces.astype(np.int32), want.points, want.faces, 'command')
    lines = [l for l in run.stdout.splitlines() if l.startswith('V:')]
    pattern = (r"^V: +%d -> +%d,  F: +%d -> +%d,  in \[low, high\]: +%.1f%% -> +%.1f%%,  valence dev: %.3f -> %.3f,  "
               r"drift mean: (\S+),  max: (\S+),  'ball\.obj'$"
               % (points.shape[0], want.points.shape[0], faces.shape[0], want.faces.shape[0], 100 * want.before['share'],
                  100 * want.after['share'], want.before['valence_dev'], want.after['valence_dev']))
    m = re.match(pattern, lines[0]) if len(lines) == 1 else None
    assert m, lines
    assert 0.0 < float(m.group(1)) <= float(m.group(2)) < 0.1                            # on a unit sphere, L about 0.45
    # a plain folder, the default target, no feature edges
    plain = os.path.join(root, 'plain')
    os.makedirs(plain)
    g_points, g_faces = S.grid(6, 5, seed=2)
    meshio.write_obj(os.path.join(plain, 'grid.obj'), g_points, g_faces)
    run = _run(['remesh', '--data_dir', plain, '--out_dir', os.path.join(root, 'flat'), '--iterations', '1', '--feature_angle', '180'])
    assert run.returncode == 0 and 'not carried along' not in run.stdout
    assert os.path.exists(os.path.join(root, 'flat', 'grid.obj'))
