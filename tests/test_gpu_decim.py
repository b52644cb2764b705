"""Mesh simplification on the device (csrc/decim.hip, geobi_gnn_amd/meshdecim.py) against the sequential model of
tests/decim_model.py, and the `decimate` command end to end.

Every comparison is EXACT: faces, face_map, vertex_map, vertex_parents, place and the counts of every round equal as
integers, the points equal as uint32 bit patterns.  There are no tolerances."""
import os
import re

import numpy as np
import pytest
import torch

import decim_model as M
import subdiv_model as S
import test_gpu_workspace as W
from train_cases import _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


class _Host(object):
    """a device result as numpy arrays"""

    def __init__(self, d):
        for field in ('points', 'faces', 'face_map', 'vertex_map'):
            t = getattr(d, field)
            assert t.is_cuda and t.is_contiguous(), field
            setattr(self, field, t.cpu().numpy())
        self.counts = d.counts
        self.per_round = [p.counts for p in d.passes]


_MODELS = {}


def _model(name, points, faces, **kw):
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _MODELS:
        _MODELS[key] = M.decimate(points, faces, **kw)
    return _MODELS[key]


def _check(dev, name, points, faces, **kw):
    """decimate on the device against the model (computed once per named input), everything exact, round by round; apply
    with the input's points must reproduce the output bit for bit -> (device result, model result)"""
    from geobi_gnn_amd import meshdecim
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    want = _model(name, points, faces, **kw)
    got = meshdecim.decimate(points, faces, device=dev, **kw)
    M.assert_same(_Host(got), want, name)
    assert len(got.passes) == len(want.rounds)
    for k, (p, r) in enumerate(zip(got.passes, want.rounds)):
        assert p.place.dtype == torch.int8 and p.vertex_parents.dtype == torch.int32
        assert (p.V, p.Vn) == (r.vertex_map.shape[0], r.points.shape[0]), (name, k)
        assert np.array_equal(p.vertex_parents.cpu().numpy(), r.vertex_parents), (name, k)
        assert np.array_equal(p.place.cpu().numpy(), r.place), (name, k)
    again = meshdecim.apply(got, points)
    assert np.array_equal(M.bits(again.cpu().numpy()), M.bits(want.points)), name + ': apply(input points)'
    return got, want


HAND = M.hand_cases()


@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_cases(dev, name):
    """a tetrahedron, an octahedron, an icosahedron, one and two triangles, three faces on one edge, a duplicated face, a
    face with repeated corners, an unreferenced vertex"""
    points, faces = HAND[name]
    _, want = _check(dev, name, points, faces, ratio=0.5)
    _check(dev, name, points, faces, target_faces=1)
    _check(dev, name, points, faces, max_cost=1e-3)
    if name in ('octahedron', 'icosahedron'):
        assert want.counts['collapses'] >= 1 and want.counts['reached']
    if name in ('tetrahedron', 'one_triangle', 'two_consistent', 'two_inconsistent', 'three_on_an_edge'):
        assert want.counts['collapses'] == 0 and not want.counts['reached']


@pytest.mark.parametrize('rim', [85, 86, 128])
def test_bipyramids_at_the_block_edges(dev, rim):
    """255 / 258 / 384 edges: around the 256-lane block edge of the per-edge kernels"""
    points, faces = M.bipyramid(rim)
    assert S.edge_facts(faces)['E'] == 3 * rim
    got, want = _check(dev, 'bipyramid%d' % rim, points, faces, ratio=0.5)
    assert want.counts['reached'] and got.faces.shape[0] in (rim, rim - 1)


def test_hub_of_valence_200_with_a_shuffled_rim(dev):
    """neighbour lists longer than a wave, and not in the order of the walk around the apexes"""
    points, faces = M.bipyramid(200, shuffled=True)
    _, want = _check(dev, 'hub200', points, faces, ratio=0.5)
    assert want.counts['reached']
    _check(dev, 'hub200', points, faces, ratio=0.05, max_rounds=64)


@pytest.mark.parametrize('n_faces', [255, 256, 257])
def test_strips_have_nothing_to_do(dev, n_faces):
    """F across 256; every vertex is on the boundary, so every vertex is locked"""
    points, faces = S.strip(n_faces)
    got, want = _check(dev, 'strip%d' % n_faces, points, faces, ratio=0.5)
    assert want.counts == {'edges': 2 * n_faces + 1, 'locked': n_faces + 2, 'not_included': 0, 'collapses': 0, 'rounds': 0,
                           'reached': False}
    assert torch.equal(got.faces.cpu(), torch.from_numpy(faces))


@pytest.mark.parametrize('ratio', [0.5, 0.1])
def test_icosphere_2(dev, ratio):
    points, faces = M.icosphere(2)
    got, want = _check(dev, 'icosphere2', points, faces, ratio=ratio, max_rounds=64)
    assert want.counts['reached'] and got.faces.shape[0] == int(80 * ratio)


@pytest.mark.parametrize('frequency', [3, 8])
def test_icosphere_to_320_faces(dev, frequency):
    """meshgen.icosphere(3) has 180 faces, below the target already: no round.  The sphere of 1280 faces is frequency 8"""
    points, faces = M.icosphere(frequency)
    got, want = _check(dev, 'icosphere%d' % frequency, points, faces, target_faces=320, max_rounds=64)
    assert want.counts['reached'] and got.faces.shape[0] == min(320, faces.shape[0])
    assert (want.counts['rounds'] == 0) == (frequency == 3)


def test_noisy_sphere(dev):
    """costs without symmetry, and normals rough enough that the flip test refuses candidates in the first round"""
    from geobi_gnn_amd import meshgen
    noisy, _, faces = meshgen.noisy_icosphere(10, 0.6, seed=3)
    got, want = _check(dev, 'noisy_sphere', noisy, faces, ratio=0.2, max_rounds=64)
    assert want.per_round[0]['valid'] < want.per_round[0]['edges'] == 3000
    assert want.counts['reached'] and got.faces.shape[0] == 400


def test_flat_grid_all_ties(dev):
    """every cost is exactly 0: the order is the hash's"""
    points, faces = M.flat_grid(16)
    got, want = _check(dev, 'flat_grid', points, faces, max_cost=0.0, max_rounds=64)
    assert want.counts['reached'] and want.counts['locked'] == 64 and S.area(got.points.cpu().numpy(), want.faces) == 256.0


def test_dyadic_box(dev):
    points, faces = M.dyadic_box()
    got, want = _check(dev, 'dyadic_box', points, faces, max_cost=0.0, max_rounds=64)
    out = got.points.cpu().numpy()
    assert S.area(out, want.faces) == 22.0 and M.volume(out, want.faces) == 6.0


def test_budget_cuts_a_round(dev):
    points, faces = M.icosphere(2)
    whole = M.one_round(points, faces)
    assert whole.counts['collapses'] >= 3
    got, want = _check(dev, 'icosphere2', points, faces, target_faces=80 - 4)
    assert want.per_round == [dict(whole.counts, collapses=2, V=40, F=76)] and got.points.shape[0] == 40


@pytest.mark.parametrize('target', [41, 40, 39])
def test_a_target_above_and_below_an_achievable_count(dev, target):
    points, faces = M.icosphere(2)
    got, _ = _check(dev, 'icosphere2', points, faces, target_faces=target)
    assert got.faces.shape[0] == target - target % 2 and got.counts['reached']


def test_apply_with_other_points(dev):
    from geobi_gnn_amd import meshdecim
    points, faces = M.icosphere(2)
    got, want = _check(dev, 'icosphere2', points, faces, ratio=0.5, max_rounds=64)
    noisy = (points + 0.05 * np.random.RandomState(8).randn(*points.shape)).astype(np.float32)
    stretched = (points * np.float32(3.0)).astype(np.float32)
    for other in (noisy, stretched):
        moved = meshdecim.apply(got, other)
        assert moved.is_cuda and moved.dtype == torch.float32 and moved.shape == got.points.shape
        assert np.array_equal(M.bits(moved.cpu().numpy()), M.bits(M.apply(want, other)))
        assert not np.array_equal(M.bits(moved.cpu().numpy()), M.bits(want.points))
    moved = meshdecim.apply(got, torch.from_numpy(noisy).to(dev))
    assert np.array_equal(M.bits(moved.cpu().numpy()), M.bits(M.apply(want, noisy)))
    with pytest.raises(ValueError):
        meshdecim.apply(got, noisy[:-1])


@pytest.mark.parametrize('name', ['icosphere4', 'grid', 'three_on_an_edge'])
def test_mesh_report_before_and_after(dev, name):
    from geobi_gnn_amd import meshdecim, meshtopo
    points, faces = {'icosphere4': lambda: M.icosphere(4), 'grid': lambda: S.grid(9, 7, seed=1),
                     'three_on_an_edge': lambda: HAND['three_on_an_edge']}[name]()
    before = meshtopo.mesh_report(points, faces, weld_tol=None, device=dev)
    d = meshdecim.decimate(points, faces, ratio=0.5, device=dev)
    after = meshtopo.mesh_report(d.points, d.faces, weld_tol=None, device=dev)
    for key in ('closed', 'components', 'nonorientable', 'degenerate', 'euler', 'boundary_edges', 'complex_edges'):
        assert after[key] == before[key], key
    assert after['vertices_used'] == d.points.shape[0] and after['faces'] == d.faces.shape[0]
    assert d.counts['edges'] == before['edges']
    if name != 'three_on_an_edge':
        assert d.counts['collapses'] > 0 and after['faces'] == before['faces'] - 2 * d.counts['collapses']


def test_two_calls_are_bit_identical(dev):
    from geobi_gnn_amd import meshdecim
    points, faces = S.grid(24, 20, seed=6)
    a, b = (meshdecim.decimate(points, faces, ratio=0.3, device=dev) for _ in range(2))
    assert a.counts == b.counts and a.counts['collapses'] > 0
    for field in ('points', 'faces', 'face_map', 'vertex_map'):
        assert torch.equal(getattr(a, field).view(torch.int32), getattr(b, field).view(torch.int32)), field


def test_errors(dev):
    from geobi_gnn_amd import _lib as L
    from geobi_gnn_amd import meshdecim
    points, faces = M.icosphere(2)
    for kw in ({}, {'target_faces': 10, 'ratio': 0.5}, {'ratio': 1.5}, {'target_faces': -2}, {'max_cost': -1.0},
               {'ratio': 0.5, 'max_rounds': 0}):
        with pytest.raises(ValueError):
            meshdecim.decimate(points, faces, device=dev, **kw)
    bad = points.copy()
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match='non-finite'):
        meshdecim.decimate(bad, faces, ratio=0.5, device=dev)
    with pytest.raises(ValueError):
        meshdecim.decimate(points.reshape(-1, 2), faces, ratio=0.5, device=dev)
    with pytest.raises(ValueError):
        meshdecim.decimate(points, faces.reshape(-1, 2), ratio=0.5, device=dev)
    for value in (points.shape[0], -1, 2 ** 32 + 1):
        wrong = faces.astype(np.int64)
        wrong[5, 2] = value
        with pytest.raises(ValueError, match='outside'):
            meshdecim.decimate(points, wrong, ratio=0.5, device=dev)
    with pytest.raises(M.TooManyRounds):
        M.decimate(points, faces, ratio=0.5, max_rounds=1)
    with pytest.raises(L.GeobiError, match='max_rounds'):
        meshdecim.decimate(points, faces, ratio=0.5, max_rounds=1, device=dev)
    _check(dev, 'icosphere2', points, faces, ratio=0.5, max_rounds=64)      # and the next call works


def test_no_faces(dev):
    from geobi_gnn_amd import meshdecim
    points = S.box()[0]
    d = meshdecim.decimate(points, np.zeros((0, 3), dtype=np.int32), ratio=0.5, device=dev)
    assert d.counts == {'edges': 0, 'locked': 0, 'not_included': 0, 'collapses': 0, 'rounds': 0, 'reached': True}
    assert d.faces.shape == (0, 3) and d.face_map.shape == (0,) and d.passes == []
    assert d.vertex_map.cpu().numpy().tolist() == list(range(8))
    assert np.array_equal(M.bits(d.points.cpu().numpy()), M.bits(points))
    assert np.array_equal(M.bits(meshdecim.apply(d, points).cpu().numpy()), M.bits(points))
    # the entry points themselves with F == 0: V' = V, every row stays
    from geobi_gnn_amd import _lib as L
    pts = torch.from_numpy(points).to(dev)
    fv = torch.zeros((1, 3), dtype=torch.int32, device=dev)
    counts = torch.full((8,), -1, dtype=torch.int32, device=dev)
    L.call('geobi_decim_plan', L.ptr(fv), L.ptr(pts), 0, 8, 0, 0.0, -1, L.ptr(counts), None, None, 0, L.stream())
    assert L.read_i32(counts) == [0, 0, 0, 0, 8, 0, 0, 0]
    out, vmap = torch.empty_like(pts), torch.empty(8, dtype=torch.int32, device=dev)
    parents, place = torch.empty((8, 2), dtype=torch.int32, device=dev), torch.empty(8, dtype=torch.int8, device=dev)
    L.call('geobi_decim_emit', L.ptr(fv), L.ptr(pts), 0, 8, 8, 0, L.ptr(out), L.ptr(fv), L.ptr(fv), L.ptr(vmap), L.ptr(parents),
           L.ptr(place), None, 0, L.stream())
    assert torch.equal(out.view(torch.int32), pts.view(torch.int32)) and vmap.tolist() == list(range(8))
    assert parents.tolist() == [[v, v] for v in range(8)] and place.tolist() == [0] * 8


def test_emit_writes_no_row_beyond_the_sizes_it_is_given(dev):
    from geobi_gnn_amd import _lib as L
    from geobi_gnn_amd import meshdecim
    points, faces = M.icosphere(2)
    pts, fv = torch.from_numpy(points).to(dev), torch.from_numpy(faces).to(dev)
    ws, c = meshdecim._plan(fv, pts, None, None)
    Vn, Fn = c['V'] - 2, c['F'] - 4                                         # fewer rows than the plan has
    sentinel = 0x5a5a5a5a
    out = {'points': torch.full((c['V'], 3), 7.5, device=dev), 'faces': torch.full((c['F'], 3), sentinel, dtype=torch.int32, device=dev),
           'face_map': torch.full((c['F'],), sentinel, dtype=torch.int32, device=dev),
           'parents': torch.full((c['V'], 2), sentinel, dtype=torch.int32, device=dev),
           'place': torch.full((c['V'],), 0x5a, dtype=torch.int8, device=dev)}
    vmap = torch.empty(pts.shape[0], dtype=torch.int32, device=dev)
    L.call('geobi_decim_emit', L.ptr(fv), L.ptr(pts), fv.shape[0], pts.shape[0], Vn, Fn, L.ptr(out['points']), L.ptr(out['faces']),
           L.ptr(out['face_map']), L.ptr(vmap), L.ptr(out['parents']), L.ptr(out['place']), L.ptr(ws), ws.numel(), L.stream())
    assert bool((out['points'][Vn:] == 7.5).all()) and bool((out['points'][:Vn] != 7.5).any())
    assert bool((out['faces'][Fn:] == sentinel).all()) and bool((out['face_map'][Fn:] == sentinel).all())
    assert bool((out['parents'][Vn:] == sentinel).all()) and bool((out['place'][Vn:] == 0x5a).all())
    assert bool((out['faces'][:Fn] != sentinel).all()) and bool((out['parents'][:Vn] != sentinel).all())


# ---- the workspace of geobi_decim_plan / _emit, in the manner of tests/test_gpu_workspace.py
def _workspace_case(dev):
    from geobi_gnn_amd import meshdecim
    points, faces = M.icosphere(4)
    d = meshdecim.decimate(points, faces, ratio=0.5, device=dev)
    return [d.points, d.faces, d.face_map, d.vertex_map, d.counts, [p.counts for p in d.passes]]


def test_guard_band(dev, monkeypatch):
    """No launcher writes behind the size its query gave, and the carve's layout does not change a result."""
    want = W._flat(_workspace_case(dev), [])
    guard = W._Guarded().install(monkeypatch)
    got = W._flat(_workspace_case(dev), [])
    assert len(guard.requests) >= 2 and all(nbytes > W.SHORT_BY for _, _, nbytes in guard.requests)
    assert set(guard.entries.values()) == {'geobi_decim_plan'}
    assert guard.sentinels_whole(), 'a launcher wrote behind its workspace'
    assert got == want, 'outputs differ from the call made with the library allocator'


def test_short_workspace(dev, monkeypatch):
    """geobi_decim_plan and geobi_decim_emit refuse a workspace 512 bytes short of its size, naming themselves and both
    sizes"""
    from geobi_gnn_amd import _lib as L
    from geobi_gnn_amd import meshdecim
    for k in (0, 1):                                                        # the plans of the first two rounds
        guard = W._Guarded(short_at=k).install(monkeypatch)
        with pytest.raises(L.GeobiError) as e:
            _workspace_case(dev)
        assert guard.sentinels_whole(), 'request %d: a launcher wrote behind the end it was given' % k
        give, nbytes = guard.requests[k][1:]
        m = re.search(r'(\w+): workspace too small \((\d+) bytes given, (\d+) needed\)', str(e.value))
        assert m and m.group(1) == 'decim_plan' and 'geobi_decim_plan failed' in str(e.value), str(e.value)
        assert int(m.group(2)) == give and give < int(m.group(3)) <= nbytes
    monkeypatch.undo()
    points, faces = M.icosphere(4)
    pts, fv = torch.from_numpy(points).to(dev), torch.from_numpy(faces).to(dev)
    ws, c = meshdecim._plan(fv, pts, None, None)
    guard = W._Guarded(short_at=0)
    short = guard(ws.numel(), dev)
    short.copy_(ws[:short.numel()])
    out = [torch.empty((c['V'], 3), device=dev), torch.empty((c['F'], 3), dtype=torch.int32, device=dev),
           torch.empty(c['F'], dtype=torch.int32, device=dev), torch.empty(pts.shape[0], dtype=torch.int32, device=dev),
           torch.empty((c['V'], 2), dtype=torch.int32, device=dev), torch.empty(c['V'], dtype=torch.int8, device=dev)]
    with pytest.raises(L.GeobiError, match=r'geobi_decim_emit failed: decim_emit: workspace too small \(%d bytes given'
                                           % short.numel()):
        L.call('geobi_decim_emit', L.ptr(fv), L.ptr(pts), fv.shape[0], pts.shape[0], c['V'], c['F'], *[L.ptr(t) for t in out],
               L.ptr(short), short.numel(), L.stream())
    assert guard.sentinels_whole()


def test_decimate_command(dev, tmp_path):
    from geobi_gnn_amd import meshio
    root = str(tmp_path)
    os.makedirs(os.path.join(root, 'original'))
    os.makedirs(os.path.join(root, 'noisy'))
    points, faces = M.icosphere(2)
    g_points, g_faces = S.grid(5, 4, seed=9)
    rng = np.random.RandomState(1)
    noisy = (points + 0.01 * rng.randn(*points.shape)).astype(np.float32)
    meshio.write_obj(os.path.join(root, 'original', 'ball.obj'), points, faces)
    meshio.write_obj(os.path.join(root, 'noisy', 'ball_n1.obj'), noisy, faces)
    meshio.write_obj(os.path.join(root, 'noisy', 'ball_n2.obj'), g_points, g_faces)          # another size: skipped
    run = _run(['decimate', '--data_dir', root, '--ratio', '0.5'])
    assert run.returncode == 1 and 'differ in size' in run.stderr and '1 files skipped' in run.stderr
    # the files as the command read them
    points, faces = meshio.read_obj(os.path.join(root, 'original', 'ball.obj'))
    noisy = meshio.read_obj(os.path.join(root, 'noisy', 'ball_n1.obj'))[0]
    want = M.decimate(points, faces, ratio=0.5)
    out = os.path.join(root, 'decimated')
    o_points, o_faces = meshio.read_obj(os.path.join(out, 'original', 'ball.obj'))
    n_points, n_faces = meshio.read_obj(os.path.join(out, 'noisy', 'ball_n1.obj'))
    assert not os.path.exists(os.path.join(out, 'noisy', 'ball_n2.obj'))
    assert np.array_equal(o_faces, want.faces) and np.array_equal(n_faces, want.faces)
    assert np.array_equal(M.bits(o_points), M.bits(want.points))              # write_obj -> read_obj keeps a float32
    assert np.array_equal(M.bits(n_points), M.bits(M.apply(want, noisy)))
    lines = [l for l in run.stdout.splitlines() if l.startswith('V:')]
    pattern = (r"^V: +42 -> +%d,  F: +80 -> +40,  rounds: %d,  reached: yes,  '%%s'$" % (want.points.shape[0], want.counts['rounds']))
    assert len(lines) == 2 and re.match(pattern % r'ball\.obj', lines[0]) and re.match(pattern % r'ball_n1\.obj', lines[1]), lines
    # a plain folder, a face count and a cost bound that stops the rounds early
    plain = os.path.join(root, 'plain')
    os.makedirs(plain)
    f_points, f_faces = M.flat_grid(8)
    meshio.write_obj(os.path.join(plain, 'grid.obj'), f_points, f_faces)
    run = _run(['decimate', '--data_dir', plain, '--out_dir', os.path.join(root, 'flat'), '--faces', '100', '--max_cost', '0'])
    assert run.returncode == 0
    want = M.decimate(f_points, f_faces, target_faces=100, max_cost=0.0)
    assert np.array_equal(meshio.read_obj(os.path.join(root, 'flat', 'grid.obj'))[1], want.faces)
    assert "reached: %s" % ('yes' if want.counts['reached'] else 'no') in run.stdout
