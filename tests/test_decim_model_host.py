"""The sequential model of the edge-collapse rules (tests/decim_model.py) pinned on facts that do not come from it, the
comparison helper of the GPU test caught on planted faults, and the parts of the feature that run without a GPU: the
argument checks, the command line and the size limits of the entry points."""
import copy
import ctypes

import numpy as np
import pytest

import decim_model as M
import subdiv_model as S
import topo_model
from train_cases import _run

CLOSED = {'icosahedron': S.icosahedron, 'icosphere2': lambda: M.icosphere(2), 'bipyramid85': lambda: M.bipyramid(85),
          'bipyramid200': lambda: M.bipyramid(200, shuffled=True), 'box': M.dyadic_box, 'neck': M.neck}


def _euler(faces):
    c = topo_model.report_counts(faces)
    return c['vertices_used'] - c['edges'] + c['faces']


def _rounds(points, faces, **kw):
    """the rounds of decimate one by one: [(input points, input faces, Round)]"""
    out = []
    for r in M.decimate(points, faces, **kw).rounds:
        out.append((points, faces, r))
        points, faces = r.points, r.faces
    return out


@pytest.mark.parametrize('name', sorted(CLOSED))
def test_closed_inputs_stay_closed_round_by_round(name):
    points, faces = CLOSED[name]()
    euler = _euler(faces)
    assert euler == 2
    rounds = _rounds(points, faces, ratio=0.25, max_rounds=64)
    assert rounds
    for p_in, f_in, r in rounds:
        facts, counts = S.edge_facts(r.faces), topo_model.report_counts(r.faces)
        assert facts['boundary'] == 0 and facts['complex'] == 0 and facts['repeated'] == 0
        assert counts['inconsistent_edges'] == 0 and counts['faces'] == r.faces.shape[0]
        assert _euler(r.faces) == euler and counts['vertices_used'] == r.points.shape[0]
        # V drops by the collapses and F by twice that
        assert r.counts['collapses'] >= 1 and r.counts['not_included'] == 0 and r.counts['locked'] == 0
        assert r.points.shape[0] == p_in.shape[0] - r.counts['collapses'] == r.counts['V']
        assert r.faces.shape[0] == f_in.shape[0] - 2 * r.counts['collapses'] == r.counts['F']
        assert r.vertex_map.shape == (p_in.shape[0],) and r.face_map.shape == (r.faces.shape[0],)
        assert np.array_equal(r.vertex_map[f_in[r.face_map]], r.faces)


@pytest.mark.parametrize('name', ['icosphere2', 'bipyramid200', 'box'])
def test_the_collapsed_edges_of_a_round_cannot_see_each_other(name):
    for _, _, r in _rounds(*CLOSED[name](), ratio=0.25, max_rounds=64):
        rings = [M.closed_ring(r.nbrs, lo) | M.closed_ring(r.nbrs, hi) for lo, hi in r.collapsed]
        for i, (lo, hi) in enumerate(r.collapsed):
            for j, ring in enumerate(rings):
                assert i == j or (lo not in ring and hi not in ring), (r.collapsed[i], r.collapsed[j])
        best = min(r.candidates, key=r.candidates.get)
        assert r.candidates[best] == 0 and best in r.collapsed
        assert sorted(r.candidates.values()) == list(range(len(r.candidates)))


def test_every_output_point_is_an_input_point_or_a_midpoint_of_the_round_before():
    points, faces = M.icosphere(2)
    seen = 0
    for p_in, _, r in _rounds(points, faces, ratio=0.1, max_rounds=64):
        for row, ((a, b), code) in enumerate(zip(r.vertex_parents.tolist(), r.place.tolist())):
            want = p_in[a] if code == 0 else p_in[b] if code == 1 else np.float32(0.5) * p_in[a] + np.float32(0.5) * p_in[b]
            assert (a == b and code == 0) or (a < b and (a, b) in r.collapsed)
            assert np.array_equal(M.bits(r.points[row]), M.bits(want))
            seen += code == 2
    assert seen > 0


@pytest.mark.parametrize('ratio', [0.5, 0.1])
def test_icosphere_reaches_its_target_within_the_cap(ratio):
    points, faces = M.icosphere(2)
    d = M.decimate(points, faces, ratio=ratio, max_rounds=64)              # the cap of 64 rounds is the issue's
    target = int(ratio * faces.shape[0])
    assert d.counts['reached'] and target - 1 <= d.faces.shape[0] <= target and d.counts['rounds'] <= 64
    assert d.points.shape[0] == points.shape[0] - d.counts['collapses']
    assert np.array_equal(M.bits(M.apply(d, points)), M.bits(d.points))
    # the maps composed over the rounds: every output face is its input face seen through vertex_map
    assert np.array_equal(d.vertex_map[faces[d.face_map]], d.faces)


@pytest.mark.parametrize('name', ['tetrahedron', 'one_triangle', 'two_consistent', 'strip'])
def test_inputs_with_nothing_to_collapse(name):
    points, faces = S.strip(40) if name == 'strip' else M.hand_cases()[name]
    d = M.decimate(points, faces, ratio=0.5)
    assert d.counts['rounds'] == 0 and d.counts['collapses'] == 0 and d.counts['reached'] is False
    assert np.array_equal(d.faces, faces) and np.array_equal(M.bits(d.points), M.bits(points))
    r = M.one_round(points, faces)
    assert r.counts['valid'] == 0 and r.counts['sweeps_selected'] == 0
    if name != 'tetrahedron':
        assert r.counts['locked'] == points.shape[0]                        # every vertex is on the boundary


def test_budget_lands_on_the_target_or_one_below():
    points, faces = M.icosphere(2)
    full = M.one_round(points, faces)
    assert full.counts['collapses'] >= 3
    cut = M.one_round(points, faces, budget=80 - 4)                          # two collapses of the round's many
    assert cut.counts['collapses'] == 2 and cut.collapsed == full.collapsed[:2] and cut.counts['valid'] == full.counts['valid']
    assert M.one_round(points, faces, budget=80 - 3).counts['F'] == 76       # an odd distance: one below
    assert M.one_round(points, faces, budget=80).counts['collapses'] == 0
    assert M.one_round(points, faces, budget=1000).counts['collapses'] == 0
    for target in (41, 40, 39):
        d = M.decimate(points, faces, target_faces=target)
        assert d.faces.shape[0] == target - target % 2 and d.counts['reached']


def test_open_grid_with_max_cost_0_keeps_its_rim_and_its_area():
    points, faces = M.flat_grid(16)
    d = M.decimate(points, faces, max_cost=0.0, max_rounds=64)
    assert d.counts['reached'] and d.counts['locked'] == 64 and d.faces.shape[0] < 128
    rim = np.nonzero((points[:, 0] == 0) | (points[:, 0] == 16) | (points[:, 1] == 0) | (points[:, 1] == 16))[0]
    assert rim.shape[0] == 64
    assert np.array_equal(M.bits(d.points[d.vertex_map[rim]]), M.bits(points[rim]))
    assert len(set(d.vertex_map[rim].tolist())) == 64
    assert S.area(d.points, d.faces) == 256.0
    assert S.edge_facts(d.faces)['boundary'] == 64 and S.edge_facts(d.faces)['complex'] == 0
    # all costs are equal: without the hash the ranks follow the ids and a round selects far fewer edges
    first = M.one_round(points, faces, max_cost=0.0)
    by_id = M.one_round(points, faces, max_cost=0.0, faults=('id_order',))
    assert first.counts['valid'] == by_id.counts['valid'] and first.counts['collapses'] > 2 * by_id.counts['collapses']


def test_dyadic_box_with_max_cost_0_keeps_area_volume_and_corners():
    points, faces = M.dyadic_box()
    assert faces.shape[0] == 768 and S.area(points, faces) == 22.0 and M.volume(points, faces) == 6.0
    d = M.decimate(points, faces, max_cost=0.0, max_rounds=64)
    assert d.counts['reached'] and d.faces.shape[0] < 100
    assert S.area(d.points, d.faces) == 22.0 and M.volume(d.points, d.faces) == 6.0
    corners = set(map(tuple, S.box()[0].tolist()))
    assert corners <= set(map(tuple, d.points.tolist()))
    facts = S.edge_facts(d.faces)
    assert facts['boundary'] == 0 and facts['complex'] == 0 and facts['repeated'] == 0


def test_faces_that_are_not_included_are_dropped_and_counted():
    points, faces = M.hand_cases()['repeated_corner']
    d = M.decimate(points, faces, ratio=0.5)
    assert d.counts['not_included'] == 3 and d.counts['rounds'] == 1 and d.counts['collapses'] == 0
    assert d.face_map.tolist() == [0, 2] and np.array_equal(d.faces, faces[[0, 2]]) and d.counts['reached']
    assert np.array_equal(M.bits(d.points), M.bits(points))                # unreferenced vertices keep their rows


@pytest.mark.parametrize('fault, case', [('no_link', 'neck'), ('no_valence', 'tetrahedron'), ('no_blocking', 'icosphere2'),
                                         ('id_order', 'icosphere2')])
def test_planted_faults_are_caught(fault, case):
    points, faces = S.tetrahedron() if case == 'tetrahedron' else CLOSED[case]()
    want = M.decimate(points, faces, ratio=0.4)
    M.assert_same(copy.deepcopy(want), want)
    bad = M.decimate(points, faces, ratio=0.4, faults=(fault,))
    with pytest.raises(AssertionError, match='differ|counts'):
        M.assert_same(bad, want)
    if fault in ('no_valence', 'no_blocking'):                              # and the surface is no longer a closed manifold
        facts = S.edge_facts(bad.faces)
        assert facts['boundary'] + facts['complex'] + facts['repeated'] > 0 or _euler(bad.faces) != 2 or bad.faces.shape[0] < 4


def test_one_flipped_bit_of_a_point_is_caught():
    points, faces = M.icosphere(2)
    want = M.decimate(points, faces, ratio=0.5)
    bad = copy.deepcopy(want)
    bad.points.view(np.uint32)[7, 1] ^= 1
    with pytest.raises(AssertionError, match='points differ in 1 rows'):
        M.assert_same(bad, want)
    bad = copy.deepcopy(want)
    bad.vertex_map[3] += 1
    with pytest.raises(AssertionError, match='vertex_map differ'):
        M.assert_same(bad, want)


def test_check_args():
    from geobi_gnn_amd import meshdecim
    assert meshdecim.check_args(target_faces=10) == (10, None, None)
    assert meshdecim.check_args(ratio=0.5, max_cost=1e-3) == (None, 0.5, float(np.float32(1e-3)))
    assert meshdecim.check_args(max_cost=0) == (None, None, 0.0)
    assert meshdecim.stop_target(81, ratio=0.5) == 40 and meshdecim.stop_target(81, target_faces=7) == 7
    assert M.stop_target(81, ratio=0.5) == 40 and meshdecim.stop_target(81) is None
    for kw in ({}, {'target_faces': 10, 'ratio': 0.5}, {'target_faces': -1}, {'target_faces': 2.5}, {'target_faces': True},
               {'ratio': 0.0}, {'ratio': 1.0}, {'ratio': float('nan')}, {'ratio': 'half'}, {'max_cost': -1.0},
               {'max_cost': float('nan')}, {'max_cost': float('inf')}, {'max_cost': 1e60}, {'ratio': 0.5, 'max_rounds': 0},
               {'ratio': 0.5, 'max_rounds': 1.5}):
        with pytest.raises(ValueError):
            meshdecim.check_args(**kw)
        with pytest.raises(ValueError):
            meshdecim.decimate(*S.box(), **kw)                              # before any device work


def test_decimate_help_names_every_flag():
    run = _run(['decimate', '--help'])
    assert run.returncode == 0
    for flag in ('--data_dir', '--out_dir', '--ratio', '--faces', '--max_cost', '--max_rounds', '--gpu'):
        assert flag in run.stdout, flag
    from geobi_gnn_amd.__main__ import parse_args
    for args in ([], ['--ratio', '0.5', '--faces', '10'], ['--ratio', '0'], ['--ratio', '1'], ['--faces', '-3'],
                 ['--ratio', '0.5', '--max_cost', '-1'], ['--ratio', '0.5', '--max_rounds', '0'], ['--max_cost', '0']):
        with pytest.raises(SystemExit) as e:
            parse_args(['decimate', '--data_dir', 'nowhere'] + args)
        assert e.value.code == 2, args
    opt = parse_args(['decimate', '--data_dir', 'd', '--faces', '20000', '--max_cost', '0.5'])
    assert (opt.ratio, opt.faces, opt.max_cost, opt.max_rounds, opt.out_dir, opt.gpu) == (None, 20000, 0.5, 256, '', -1)


def test_sizes_beyond_the_documented_limits_are_rejected():
    """geobi_decim_*: F or V above GEOBI_MAX_NODES is refused before anything touches the device (no GPU needed)."""
    from geobi_gnn_amd import _lib as L
    lib = L.lib()
    big = (1 << 24)
    one = ctypes.c_void_p(256)                     # never dereferenced: the size check comes first
    assert lib.geobi_decim_ws_bytes(big, 10) == 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
    assert lib.geobi_decim_ws_bytes(10, big) == 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
    for F, V in ((big, 10), (10, big)):
        rc = lib.geobi_decim_plan(one, one, F, V, 0, 0.0, -1, one, None, one, 1 << 20, None)
        assert rc != 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
        rc = lib.geobi_decim_emit(one, one, F, V, 10, 10, one, one, one, one, one, one, one, 1 << 20, None)
        assert rc != 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
    rc = lib.geobi_decim_emit(one, one, 10, 10, big, 10, one, one, one, one, one, one, one, 1 << 20, None)
    assert rc != 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
    for V, Vn in ((big, 10), (10, big)):
        rc = lib.geobi_decim_points(one, V, Vn, one, one, one, None)
        assert rc != 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
    rc = lib.geobi_decim_plan(one, one, -1, 10, 0, 0.0, -1, one, None, one, 1 << 20, None)
    assert rc != 0 and b'negative' in lib.geobi_last_error()
    rc = lib.geobi_decim_plan(one, one, 10, 10, 1, -1.0, -1, one, None, one, 1 << 20, None)
    assert rc != 0 and b'max_cost' in lib.geobi_last_error()
    # sizes no plan can give: more rows than the input, fewer faces gone than two per merged vertex
    for Vn, Fn in ((11, 10), (10, 11), (8, 7)):
        rc = lib.geobi_decim_emit(one, one, 10, 10, Vn, Fn, one, one, one, one, one, one, one, 1 << 20, None)
        assert rc != 0 and b'are not what a plan' in lib.geobi_last_error()
    rc = lib.geobi_decim_points(one, 10, 11, one, one, one, None)
    assert rc != 0 and b'rows from' in lib.geobi_last_error()
