"""Self-intersections on the device (csrc/selfx.hip: geobi_self_intersections), its Python layers (meshselfx,
meshtopo.mesh_report(intersections=True), meshclean.clean_mesh(drop_intersecting=True)) and the commands, against
tests/selfx_model.py: the exact statement of the definition wherever the coordinates are integers, the numpy restatement
of the kernel's order of operations everywhere.

Every comparison is EXACT: hits and the pair list as integer arrays, the counts as integers.  There are no tolerances.

Shapes: hand cases of two to four faces; integer soups of 96 faces over 24 vertices; the same generator at F = T - 1, T,
T + 1, 2 T + 1 = B + 1 (T = 256 faces per target tile, B = 512 faces per query block: one tile short of full, one full, two
slices, three slices and two query blocks); spheres of 180 and 1 280 faces."""
import os
import re

import numpy as np
import pytest
import torch

import selfx_model as X
import test_gpu_workspace as W
from train_cases import _run

pytestmark = pytest.mark.gpu

HAND = X.hand_cases()
EDGE_SIZES = (X.TILE - 1, X.TILE, X.TILE + 1, 2 * X.TILE + 1, X.QUERY_BLOCK + 1)
ALL = (1 << 20)                  # a pair list no case here fills


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


def _search(dev, verts, faces, state=None, max_pairs=ALL):
    from geobi_gnn_amd import meshselfx
    r = meshselfx.self_intersections(np.asarray(verts, dtype=np.float32), faces, state=state, max_pairs=max_pairs, device=dev)
    return r.hits.cpu().numpy(), r.pairs.cpu().numpy(), r.counts


def _assert_same(got, want, what):
    hits, pairs, counts = got
    assert counts == want.counts, (what, counts, want.counts)
    assert pairs.dtype == np.int32 and pairs.shape == want.pairs.shape and np.array_equal(pairs, want.pairs), what
    assert hits.dtype == np.int32 and np.array_equal(hits, want.hits), what


def _sphere(n):
    from geobi_gnn_amd import meshgen
    points, faces = meshgen.icosphere(n)
    return np.asarray(points, dtype=np.float32), np.asarray(faces, dtype=np.int32)


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_cases(dev, name):
    verts, faces, state, pairs = HAND[name]
    got = _search(dev, verts, faces, state)
    assert [tuple(p) for p in got[1]] == [p[:2] for p in pairs]
    assert got[2]['pairs_k2'] == sum(1 for p in pairs if p[2] == 2)
    assert X.exact_pairs(verts, faces, state) == pairs
    _assert_same(got, X.search(verts, faces, state), name)


@pytest.mark.parametrize('seed', X.SOUP_SEEDS)
def test_integer_soups_against_the_exact_statement(dev, seed):
    verts, faces = X.soup(seed)
    exact = X.exact_pairs(verts, faces)
    for v in (verts, X.scaled(verts)):
        got = _search(dev, v, faces)
        assert [tuple(p) for p in got[1]] == [p[:2] for p in exact]
        for k in (0, 1, 2):
            assert got[2]['pairs_k%d' % k] == sum(1 for p in exact if p[2] == k)
        _assert_same(got, X.search(v, faces), seed)


def test_tile_block_and_slice_edges(dev):
    from geobi_gnn_amd import _lib as L
    slices = {F: L.lib().geobi_self_intersections_slices(F) for F in EDGE_SIZES}
    assert slices[X.TILE - 1] == slices[X.TILE] == 1 and slices[X.TILE + 1] == 2 and max(slices.values()) > 1
    assert any(-(-F // X.QUERY_BLOCK) > 1 for F in EDGE_SIZES)          # more than one query block
    assert L.lib().geobi_self_intersections_slices(0) == 0
    for F in sorted(set(EDGE_SIZES)):
        verts, faces = X.soup(100 + F, F=F, V=max(24, F // 3), extent=12)
        want = X.search(verts, faces)
        assert want.counts['pairs'] > 0 and want.counts['degenerate'] > 0
        _assert_same(_search(dev, verts, faces), want, F)


@pytest.mark.parametrize('n, F', [(3, 180), (8, 1280)])
def test_a_closed_sphere_has_none_and_a_pushed_one_has_some(dev, n, F):
    points, faces = _sphere(n)
    assert faces.shape[0] == F
    hits, pairs, counts = _search(dev, points, faces)
    assert counts['pairs'] == 0 and pairs.shape == (0, 2) and not hits.any() and counts['faces_hit'] == 0
    assert counts['box_candidates'] >= 3 * F // 2 and counts['included'] == F          # every edge neighbour at least
    _assert_same((hits, pairs, counts), X.search(points, faces), 'sphere')
    pushed = X.pushed_sphere(points)
    want = X.search(pushed, faces)
    assert want.counts['pairs'] > 0
    _assert_same(_search(dev, pushed, faces), want, 'pushed sphere')


def test_max_pairs_determinism_and_symmetry(dev):
    from geobi_gnn_amd import _lib as L
    from geobi_gnn_amd import meshselfx
    verts, faces = X.soup(X.SOUP_SEEDS[0])
    want = X.search(verts, faces)
    total, cap = want.counts['pairs'], 100
    assert total > cap + 1
    v = torch.from_numpy(verts.astype(np.float32)).to(dev)
    fv = torch.from_numpy(faces).to(dev)
    F = fv.shape[0]
    rows = torch.full((cap + 8, 2), -7, dtype=torch.int32, device=dev)              # sentinel rows behind the capacity
    hits = torch.zeros(F, dtype=torch.int32, device=dev)
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    ws = L.workspace(L.size_query('geobi_self_intersections_ws_bytes', F, v.shape[0]), dev)
    L.call('geobi_self_intersections', L.ptr(v), L.ptr(fv), None, v.shape[0], F, L.ptr(hits), L.ptr(rows), cap, L.ptr(counts),
           L.ptr(ws), ws.numel(), L.stream())
    rows = rows.cpu().numpy()
    assert np.array_equal(rows[:cap], want.pairs[:cap]) and (rows[cap:] == -7).all()
    assert L.read_i64(counts) == [want.counts[k] for k in X.COUNT_KEYS]
    assert np.array_equal(hits.cpu().numpy(), want.hits)
    # no list at all
    none = meshselfx.self_intersections(verts.astype(np.float32), faces, max_pairs=0, device=dev)
    assert none.pairs.shape == (0, 2) and none.counts == want.counts and np.array_equal(none.hits.cpu().numpy(), want.hits)
    with pytest.raises(L.GeobiError, match='pairs is NULL'):
        L.call('geobi_self_intersections', L.ptr(v), L.ptr(fv), None, v.shape[0], F, L.ptr(hits), None, cap, L.ptr(counts),
               L.ptr(ws), ws.numel(), L.stream())
    with pytest.raises(ValueError, match='max_pairs'):
        meshselfx.self_intersections(verts, faces, max_pairs=-1, device=dev)
    with pytest.raises(ValueError, match='states for'):
        meshselfx.self_intersections(verts, faces, state=np.ones(3), device=dev)
    # the same call twice, and hits against the list
    one, two = _search(dev, verts, faces), _search(dev, verts, faces)
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1]) and one[2] == two[2]
    assert np.array_equal(one[0], np.bincount(one[1].reshape(-1), minlength=F))
    # nothing to search
    empty = meshselfx.self_intersections(np.zeros((3, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32), device=dev)
    assert empty.counts == dict.fromkeys(X.COUNT_KEYS, 0) and empty.hits.shape == (0,) and empty.pairs.shape == (0, 2)


def test_workspace_guard_band_and_a_short_one(dev, monkeypatch):
    from geobi_gnn_amd import _lib as L
    from geobi_gnn_amd import meshselfx
    verts, faces = X.soup(100 + X.TILE + 1, F=X.TILE + 1, V=85, extent=12)              # two slices
    want = X.search(verts, faces)
    guard = W._Guarded().install(monkeypatch)
    r = meshselfx.self_intersections(verts.astype(np.float32), faces, max_pairs=ALL, device=dev)
    assert guard.sentinels_whole() and list(guard.entries.values()) == ['geobi_self_intersections']
    _assert_same((r.hits.cpu().numpy(), r.pairs.cpu().numpy(), r.counts), want, 'guarded')
    monkeypatch.undo()
    guard = W._Guarded(short_at=0).install(monkeypatch)
    with pytest.raises(L.GeobiError) as e:
        meshselfx.self_intersections(verts.astype(np.float32), faces, max_pairs=ALL, device=dev)
    monkeypatch.undo()
    assert guard.sentinels_whole()
    give, nbytes = guard.requests[0][1:]
    m = re.search(r'geobi_self_intersections failed: self_intersections: workspace too small \((\d+) bytes given, (\d+) needed\)',
                  str(e.value))
    assert m and int(m.group(1)) == give and give < int(m.group(2)) <= nbytes, str(e.value)


# ------------------------------------------------------------------------------------------------ the Python layers
REPORT_KEYS = {'vertices_used', 'faces', 'degenerate', 'edges', 'boundary_edges', 'complex_edges', 'inconsistent_edges',
               'components', 'orient_components', 'nonorientable', 'would_flip', 'euler', 'closed'}
NEW_KEYS = ('intersecting_pairs', 'intersecting_faces', 'folded_pairs')


def _unwelded(points, faces):
    return points[faces].reshape(-1, 3), np.arange(3 * faces.shape[0], dtype=np.int32).reshape(-1, 3)


def test_mesh_report_on_a_welded_and_an_unwelded_copy(dev):
    from geobi_gnn_amd import meshtopo
    points, faces = _sphere(3)
    pushed = X.pushed_sphere(points)
    want = X.search(pushed, faces).counts
    today = meshtopo.mesh_report(pushed, faces, device=dev)
    assert set(today) == REPORT_KEYS and today == meshtopo.mesh_report(pushed, faces, device=dev, intersections=False)
    r = meshtopo.mesh_report(pushed, faces, device=dev, intersections=True)
    assert set(r) == REPORT_KEYS | set(NEW_KEYS) and {k: r[k] for k in today} == today
    assert (r['intersecting_pairs'], r['intersecting_faces'], r['folded_pairs']) == (want['pairs'], want['faces_hit'], want['pairs_k2'])
    assert r['intersecting_pairs'] > 0
    # every face with vertices of its own: the weld brings the shared ids back, and with them the same answer
    sp, sf = _unwelded(pushed, faces)
    assert {k: meshtopo.mesh_report(sp, sf, device=dev, intersections=True)[k] for k in NEW_KEYS} == {k: r[k] for k in NEW_KEYS}
    # without the weld no two faces share an id, and every pair of neighbours touches: why the search runs after it
    apart = X.search(sp, sf).counts
    u = meshtopo.mesh_report(sp, sf, weld_tol=None, device=dev, intersections=True)
    assert (u['intersecting_pairs'], u['intersecting_faces'], u['folded_pairs']) == (apart['pairs'], apart['faces_hit'], 0)
    assert u['intersecting_pairs'] > 3 * faces.shape[0] // 2 > r['intersecting_pairs'] and u['intersecting_faces'] == faces.shape[0]
    # a flat fold is reported under its own key
    verts, table, _, _ = HAND['k2_folded_flat']
    folded = meshtopo.mesh_report(verts.astype(np.float32), table, device=dev, intersections=True)
    assert (folded['intersecting_pairs'], folded['intersecting_faces'], folded['folded_pairs']) == (1, 2, 1)


def test_clean_mesh_drops_the_intersecting_faces_in_one_pass(dev):
    from geobi_gnn_amd import meshclean, meshselfx
    points, faces = _sphere(3)
    pushed = X.pushed_sphere(points)
    want = X.search(pushed, faces)
    plain = meshclean.clean_mesh(pushed, faces, device=dev)
    # the premise of the expectation below: the weld and the half-edge rule leave this sphere as it is
    assert plain.counts == {'welded': 0, 'degenerate': 0, 'nonmanifold': 0, 'unreferenced': 0, 'rounds': plain.counts['rounds']}
    assert plain.faces.shape[0] == faces.shape[0]
    got = meshclean.clean_mesh(pushed, faces, device=dev, drop_intersecting=True)
    left = np.flatnonzero(want.hits == 0)
    assert 0 < left.shape[0] < faces.shape[0]
    assert np.array_equal(got.face_map.cpu().numpy(), left)
    assert got.counts['intersecting'] == want.counts['faces_hit'] == faces.shape[0] - left.shape[0]
    # the counts of the same call without the option; a vertex whose faces all left is unreferenced now
    loose = points.shape[0] - np.unique(faces[left]).shape[0]
    assert {k: got.counts[k] for k in plain.counts} == dict(plain.counts, unreferenced=loose)
    src = got.vertex_src.cpu().numpy()
    assert np.array_equal(src, np.unique(faces[left])) and np.array_equal(src[got.faces.cpu().numpy()], faces[left])
    assert np.array_equal(got.points.cpu().numpy().view(np.int32), pushed[src].view(np.int32))
    # one pass is enough: what is left does not intersect
    again = meshselfx.self_intersections(got.points, got.faces, max_pairs=4, device=dev)
    assert again.counts['pairs'] == 0 and again.counts['included'] == left.shape[0]
    # a paired point array follows through the maps, both ways
    paired = np.random.RandomState(3).standard_normal(points.shape).astype(np.float32)
    assert np.array_equal(meshclean.apply(got, paired), paired[src])
    back = meshclean.scatter_back(got, meshclean.apply(got, paired) + 1, paired)
    assert np.array_equal(back[src], paired[src] + 1) and np.array_equal(np.delete(back, src, 0), np.delete(paired, src, 0))
    # with min_component behind it: the parts are counted on what the search left
    both = meshclean.clean_mesh(pushed, faces, device=dev, drop_intersecting=True, min_component=1)
    assert both.counts['intersecting'] == got.counts['intersecting'] and both.topology['faces_dropped'] == 0
    assert np.array_equal(both.face_map.cpu().numpy(), left)
    # without the option no key
    assert 'intersecting' not in plain.counts


# ------------------------------------------------------------------------------------------------ the commands
def _stabbed_sphere():
    """a closed sphere and one loose triangle that goes through the middle of its face 0"""
    points, faces = _sphere(3)
    c = points[faces[0]].astype(np.float64).mean(0)
    t = np.cross(c, [0.0, 0.0, 1.0])
    spike = np.stack([0.7 * c, 1.3 * c, 1.3 * c + 0.02 * t / np.linalg.norm(t)]).astype(np.float32)
    V = points.shape[0]
    return np.concatenate([points, spike]), np.concatenate([faces, np.array([[V, V + 1, V + 2]], dtype=np.int32)])


def test_commands(dev, tmp_path):
    from geobi_gnn_amd import __main__ as main
    from geobi_gnn_amd import meshio, meshtopo
    data = str(tmp_path / 'scan')
    os.makedirs(data)
    points, faces = _sphere(3)
    meshes = {'pushed': (X.pushed_sphere(points), faces), 'stabbed': _stabbed_sphere()}
    for name, (p, f) in meshes.items():
        meshio.write_obj(os.path.join(data, name + '.obj'), p, f)
        meshes[name] = meshio.read_obj(os.path.join(data, name + '.obj'))
    want = {name: X.search(p, f) for name, (p, f) in meshes.items()}
    assert want['stabbed'].counts['pairs'] == 1 and want['stabbed'].pairs.tolist() == [[0, 180]]
    today = r"V: +(\d+),  F: +(\d+),  vertices_used: \d+,  faces: \d+,  degenerate: \d+,  edges: \d+,  boundary_edges: (\d+),  " \
            r"complex_edges: \d+,  inconsistent_edges: \d+,  components: \d+,  orient_components: \d+,  nonorientable: \d+,  " \
            r"would_flip: \d+,  euler: -?\d+,  closed: (yes|no),  '%s\.obj'"
    # info: today's line without the flag, the three fields behind it with the flag
    run = _run(['info', '--data_dir', data])
    assert run.returncode == 0, run.stderr[-2000:]
    for name in meshes:
        assert re.search('^' + today % name + '$', run.stdout, re.M), run.stdout
    assert 'intersecting' not in run.stdout
    run = _run(['info', '--data_dir', data, '--intersections'])
    assert run.returncode == 0, run.stderr[-2000:]
    for name in meshes:
        c = want[name].counts
        tail = ',  intersecting_pairs: %d,  intersecting_faces: %d,  folded_pairs: %d' % (c['pairs'], c['faces_hit'], c['pairs_k2'])
        assert re.search('^' + today % name + re.escape(tail) + '$', run.stdout, re.M), run.stdout
    # clean --drop_intersecting: the model's faces, and the count on the line
    run = _run(['clean', '--data_dir', data, '--drop_intersecting'])
    assert run.returncode == 0, run.stderr[-2000:]
    for name, (p, f) in meshes.items():
        left = np.flatnonzero(want[name].hits == 0)
        used = np.unique(f[left])
        out_p, out_f = meshio.read_obj(os.path.join(data, 'clean', name + '.obj'))
        assert np.array_equal(out_p.view(np.int32), p[used].view(np.int32)) and np.array_equal(used[out_f], f[left]), name
        assert re.search(r"rounds: \d+,  '%s\.obj',  intersecting: %d$" % (name, want[name].counts['faces_hit']), run.stdout, re.M)
    # fill closes what that opened
    cleaned = meshio.read_obj(os.path.join(data, 'clean', 'stabbed.obj'))
    assert meshtopo.mesh_report(*cleaned, device=dev)['boundary_edges'] == 3
    holed = str(tmp_path / 'holed')
    os.makedirs(holed)
    os.replace(os.path.join(data, 'clean', 'stabbed.obj'), os.path.join(holed, 'stabbed.obj'))
    run = _run(['fill', '--data_dir', holed])
    assert run.returncode == 0, run.stderr[-2000:]
    filled = meshtopo.mesh_report(*meshio.read_obj(os.path.join(holed, 'filled', 'stabbed.obj')), device=dev, intersections=True)
    assert filled['boundary_edges'] == 0 and filled['closed'] and filled['intersecting_pairs'] == 0
    # denoise --clean --drop_intersecting hands the option on; the file keeps its numbering and faces
    one = str(tmp_path / 'one')
    os.makedirs(one)
    meshio.write_obj(os.path.join(one, 'stabbed.obj'), *meshes['stabbed'])
    run = _run(['denoise', '--method', 'bnf', '--data_dir', one, '--clean', '--drop_intersecting', '--n_iter', '2',
                '--normal_iters', '2'])
    assert run.returncode == 0, run.stderr[-2000:]
    assert 'faces: %6d' % (meshes['stabbed'][1].shape[0] - 2) in run.stdout
    got_p, got_f = meshio.read_obj(os.path.join(one, 'result', 'stabbed-2.obj'))
    assert np.array_equal(got_f, meshes['stabbed'][1]) and got_p.shape == meshes['stabbed'][0].shape
    assert np.array_equal(got_p[-3:].view(np.int32), meshes['stabbed'][0][-3:].view(np.int32))      # the spike kept its bits
    # the flag alone: as the other clean flags, not without --clean; and no key, no field, without it
    with pytest.raises(SystemExit):
        main.parse_args(['denoise', '--data_dir', one, '--drop_intersecting'])
    opt = main.parse_args(['clean', '--data_dir', one])
    assert not hasattr(opt, 'drop_intersecting') and main._topo_args(opt)['drop_intersecting'] is False
    assert main.parse_args(['info', '--data_dir', one]).intersections is False
