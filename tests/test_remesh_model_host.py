"""tests/remesh_model.py pinned on facts that do not come from the model: closedness, Euler characteristic, the exact fall
of the valence deviation, independence of the selected quads, bit patterns of the collapsed points, the flat grid that stays
flat.  Also what of geobi_gnn_amd/meshremesh.py runs without a device: the argument checks, the command line, the size
limits.  No GPU."""
import itertools

import numpy as np
import pytest

import decim_model as D
import remesh_model as R
import subdiv_model as S

F32 = np.float32


def _closed_inputs():
    ico = S.icosahedron()
    return {'icosahedron': R.scramble(*ico, flips=12, seed=1),
            'icosphere2': R.scramble(*D.icosphere(2), flips=200, seed=2),
            'icosphere8': R.scramble(*D.icosphere(8), flips=400, seed=3),
            'bipyramid12': D.bipyramid(12), 'bipyramid85': D.bipyramid(85),
            'dyadic_box': (lambda r: (r.points, r.faces))(S.subdivide(*S.box(), levels=2))}


CLOSED = _closed_inputs()


def _no_lock(points):
    return np.zeros(np.asarray(points).shape[0], dtype=np.int32)


def _independent(r):
    """the quads of the flipped edges are pairwise outside each other's closed rings"""
    for p, q in itertools.combinations(r.flipped, 2):
        ring = set().union(*[D.closed_ring(r.nbrs, v) for v in p])
        assert not ring & set(q), (p, q)


@pytest.mark.parametrize('name', sorted(CLOSED))
def test_flips_keep_a_closed_manifold_and_lower_the_deviation_by_the_gains(name):
    points, faces = CLOSED[name]
    V, F, chi = points.shape[0], faces.shape[0], R.euler(0, faces)
    assert R.closed_manifold(faces)
    lock = _no_lock(points)
    for rounds in range(200):
        r = R.flip_round(points, faces, lock, feature_angle=180.0)
        if r.counts['valid'] == 0:
            assert r.counts['flips'] == 0
            break
        assert r.counts['flips'] >= 1 and 0 in [r.candidates[q[:2]] for q in r.flipped], 'rank 0 is selected'
        _independent(r)
        gains = sum(r.gains[q[:2]] for q in r.flipped)
        assert R.total_deviation(faces, lock) - R.total_deviation(r.faces, lock) == gains > 0
        faces = r.faces
        assert faces.shape[0] == F and R.closed_manifold(faces) and R.euler(0, faces) == chi
        assert np.unique(faces).shape[0] == V
    else:
        raise AssertionError('the flip rounds did not end')
    assert rounds >= 1 or name.startswith('dyadic'), 'the input had nothing to flip'


def test_scrambled_spheres_come_back_towards_valence_six():
    points, faces = CLOSED['icosphere8']
    lock = _no_lock(points)
    start = R.total_deviation(faces, lock)
    for _ in range(64):
        r = R.flip_round(points, faces, lock, feature_angle=180.0)
        if r.counts['flips'] == 0:
            break
        faces = r.faces
    assert R.total_deviation(faces, lock) < start // 2


@pytest.mark.parametrize('name', ['tetrahedron', 'octahedron', 'one_triangle', 'two_consistent', 'grid'])
def test_nothing_to_flip(name):
    points, faces = dict(D.hand_cases(), grid=S.grid(6, 5, regular=True))[name]
    lock = R.lock_flags(points, faces, 180.0)[0]
    r = R.flip_round(points, faces, lock, feature_angle=180.0)
    assert r.counts['flips'] == 0 and np.array_equal(r.faces, faces)
    if name in ('tetrahedron', 'octahedron', 'grid'):
        assert r.counts['valid'] == 0


def test_lock_flags_of_the_box():
    points, faces = D.dyadic_box()
    lock, counts = R.lock_flags(points, faces, 40.0)
    on_edges = ((points == 0) | (points == np.array([1, 2, 3], dtype=F32))).sum(axis=1) >= 2
    assert np.array_equal(lock != 0, on_edges) and not (lock & 1).any()
    assert counts['sharp_edges'] == 12 * 8 and counts['boundary_vertices'] == 0
    assert not R.lock_flags(points, faces, 180.0)[0].any()
    g_points, g_faces = S.grid(4, 3)
    lock, counts = R.lock_flags(g_points, g_faces, 40.0)
    assert counts['boundary_vertices'] == 14 and counts['sharp_edges'] == 0 and int((lock == 1).sum()) == 14


# ---- short-edge collapse
def _short_cases():
    sphere = D.icosphere(4)
    noisy = (sphere[0] + 0.02 * np.random.RandomState(5).randn(*sphere[0].shape)).astype(F32)
    return {'sphere': (noisy, sphere[1], 1.5 * R.mean_edge(noisy, sphere[1])),
            'uv_sphere': R.uv_sphere() + (0.35,), 'flat_grid': S.grid(8, 8) + (1.5,)}


SHORT = _short_cases()


@pytest.mark.parametrize('name', sorted(SHORT))
def test_short_collapse_rounds(name):
    points, faces, L = SHORT[name]
    low, high = R.band(L)
    rim = set(map(tuple, points[R.lock_flags(points, faces, 180.0)[0] != 0].tolist()))
    total = 0
    for _ in range(64):
        lock = R.lock_flags(points, faces, 180.0)[0]
        before = S.longest_edge2(points, faces)
        r = R.collapse_round(points, faces, low, high, lock)
        # every output point is an input point or the float32 midpoint of a collapsed edge
        allowed = set(map(tuple, S.bits(points).tolist()))
        for lo, hi in r.collapsed:
            allowed.add(tuple(S.bits(D.midpoint32(points[lo], points[hi])).tolist()))
        assert set(map(tuple, S.bits(r.points).tolist())) <= allowed
        if r.counts['collapses'] == 0:
            break
        total += r.counts['collapses']
        assert S.longest_edge2(r.points, r.faces) <= max(float(high) * float(high), before)
        for p, q in itertools.combinations(r.collapsed, 2):
            assert not (D.closed_ring(r.nbrs, p[0]) | D.closed_ring(r.nbrs, p[1])) & set(q)
        points, faces = r.points, r.faces
    else:
        raise AssertionError('the collapse rounds did not end')
    assert total > 0
    assert rim <= set(map(tuple, points.tolist())), 'a boundary vertex lost its point'
    # at exhaustion every edge still below low was refused for a reason the model names
    m = R.Mesh(points, faces)
    short = [(int(m.t.lo[e]), int(m.t.hi[e])) for e in range(m.E)
             if float(S.len2(points, int(m.t.lo[e]), int(m.t.hi[e]))) < float(low) * float(low)]
    assert set(short) == set(r.refused) and set(r.refused.values()) <= {'locked', 'high', 'link', 'valence', 'flip'}
    if name == 'flat_grid':
        assert S.area(points, faces) == 64.0


# ---- relaxation
def test_relaxation_keeps_locked_rows_and_the_plane():
    points, faces = R.jittered_grid(8)
    lock = R.lock_flags(points, faces, 40.0)[0]
    out, counts = R.relax(points, faces, lock, 0.5)
    assert counts['moved'] > 20 and counts['turned'] == 0
    assert np.array_equal(S.bits(out[lock != 0]), S.bits(points[lock != 0]))
    assert np.array_equal(S.bits(out[:, 2]), S.bits(np.zeros(out.shape[0], dtype=F32))), 'z left the plane'
    spread = lambda p: float(np.abs(p[:, :2] - S.grid(8, 8)[0][:, :2]).sum())
    assert spread(out) < spread(points)


def test_relaxation_of_a_regular_grid_moves_nothing():
    for points, faces in (S.grid(7, 6), S.grid(7, 6, regular=True)):
        lock = R.lock_flags(points, faces, 40.0)[0]
        out, counts = R.relax(points, faces, lock, 0.5)
        assert counts == {'moved': 0, 'refused': 0, 'reverted': 0, 'turned': 0}
        assert np.array_equal(S.bits(out), S.bits(points))


def test_relaxation_pulls_a_hub_towards_the_middle_of_its_rim_inside_the_plane():
    points, faces = S.hub(7)
    points = points.copy()
    points[:, 2] = 0
    points[0, :2] = (0.5, 0.25)
    lock = np.zeros(points.shape[0], dtype=np.int32)
    lock[1:] = 1
    out, counts = R.relax(points, faces, lock, 0.5)
    assert counts == {'moved': 1, 'refused': 0, 'reverted': 0, 'turned': 0}
    middle = points[1:].astype(np.float64).mean(axis=0)
    want = points[0] + 0.5 * (middle - points[0])
    assert np.allclose(out[0], want, rtol=0, atol=1e-6) and out[0, 2] == 0 and np.array_equal(S.bits(out[1:]), S.bits(points[1:]))


def test_relaxation_refuses_and_reverts_on_a_rough_sphere():
    """normals rough enough that a move would turn a face (refused), and that two moves together do (reverted)"""
    points, faces, lock = R.rough_sphere()
    out, counts = R.relax(points, faces, lock, 0.5)
    assert counts['refused'] > 0 and counts['reverted'] > 0 and counts['moved'] > counts['reverted']
    changed = (S.bits(out) != S.bits(points)).any(axis=1)
    assert int(changed.sum()) == counts['moved'] - counts['reverted']


# ---- the whole call
@pytest.mark.parametrize('name,scale', [('uv_sphere', 1.0), ('decimated_box', 1.0), ('icosphere4', 1.5)])
def test_remesh_keeps_the_surface_type_and_raises_the_share(name, scale):
    if name == 'uv_sphere':
        points, faces = R.uv_sphere()
    elif name == 'decimated_box':
        d = D.decimate(*D.dyadic_box(), ratio=0.4, max_rounds=64)
        points, faces = d.points, d.faces
    else:
        points, faces = D.icosphere(4)
    L = scale * R.mean_edge(points, faces)
    r = R.remesh(points, faces, L, iterations=5)
    assert R.closed_manifold(faces) and R.closed_manifold(r.faces) and R.euler(0, r.faces) == R.euler(0, faces) == 2
    assert len(r.per_iteration) == 5 and sum(c['turned'] for c in r.per_iteration) == 0
    assert r.after['share'] > r.before['share'], (r.before, r.after)
    assert r.after['edge_max'] <= max(float(r.high), r.before['edge_max'])
    if name == 'decimated_box':                       # the feature lines of the box keep its corners and its volume
        assert D.volume(r.points, r.faces) == 6.0


# ---- the comparison helper catches a wrong model
def _flip_rounds(points, faces, faults, rounds=3, lock=None):
    lock = _no_lock(points) if lock is None else lock
    out = []
    for _ in range(rounds):
        r = R.flip_round(points, faces, lock, feature_angle=180.0, faults=faults)
        out.append(r)
        faces = r.faces
    return out


@pytest.mark.parametrize('fault', R.FLIP_FAULTS)
def test_the_helper_catches_a_faulty_flip_model(fault):
    points, faces, lock = R.pillow()
    assert R.closed_manifold(faces) and R.euler(0, faces) == 2
    caught = False
    if fault == 'no_diagonal':                        # one more valid candidate: the counts of the round differ
        want, got = _flip_rounds(points, faces, (), 1, lock), _flip_rounds(points, faces, (fault,), 1, lock)
        assert (0, 1) not in want[0].candidates and (0, 1) in got[0].candidates
        with pytest.raises(AssertionError, match='counts'):
            R.assert_same_round(got[0], want[0])
        caught = True
    for name in ('icosphere2', 'icosphere8', 'bipyramid12', 'icosahedron'):
        points, faces = CLOSED[name]
        if name == 'icosphere8':                      # rough normals: the fold test has something to refuse
            points = (points + 0.2 * np.random.RandomState(7).randn(*points.shape)).astype(F32)
        want, got = _flip_rounds(points, faces, ()), _flip_rounds(points, faces, (fault,))
        try:
            for g, w in zip(got, want):
                R.assert_same_mesh(points, g, points, w, name)
        except AssertionError:
            caught = True
    assert caught, fault


def test_the_helper_catches_a_collapse_without_the_high_test_and_one_flipped_bit():
    points, faces, L = SHORT['uv_sphere']
    low, high = R.band(L)
    want = R.collapse_round(points, faces, low, high)
    wrong = R.collapse_round(points, faces, low, high, faults=('no_high',))
    with pytest.raises(AssertionError):
        R.assert_same_mesh(wrong.points, wrong.faces, want.points, want.faces)
    R.assert_same_mesh(want.points.copy(), want.faces.copy(), want.points, want.faces)
    flipped = want.points.copy()
    flipped.view(np.uint32)[3, 1] ^= 1
    with pytest.raises(AssertionError, match='points differ in 1 rows'):
        R.assert_same_mesh(flipped, want.faces, want.points, want.faces)
    other = want.faces.copy()
    other[5] = other[5][[1, 2, 0]]
    with pytest.raises(AssertionError, match='faces differ'):
        R.assert_same_mesh(want.points, other, want.points, want.faces)


# ---- what runs without a device
def test_argument_checks():
    from geobi_gnn_amd import meshremesh
    for kw in ({'target_edge': 1.0, 'target_edge_diag': 0.1}, {'target_edge': 0.0}, {'target_edge': -1.0},
               {'target_edge': float('nan')}, {'target_edge_diag': 'x'}, {'iterations': -1}, {'iterations': 1.5},
               {'feature_angle': 120.0}, {'feature_angle': -1.0}, {'relax_lambda': 1.5}, {'relax_lambda': float('inf')},
               {'max_rounds': 0}, {'max_rounds': True}):
        with pytest.raises(ValueError, match='remesh: '):
            meshremesh.check_args(**kw)
    assert meshremesh.check_args(target_edge=2, feature_angle=180) == (2.0, None, 180.0, 0.5)
    assert meshremesh.cos2(180.0) == (0, 0.0) and meshremesh.cos2(40.0) == R.cos2(40.0) and meshremesh.cos2(90.0)[1] < 1e-32
    for L in (1.0, 0.3, 1e-3, 7.77):
        assert meshremesh.band(L) == tuple(float(x) for x in R.band(L))
    with pytest.raises(ValueError):
        meshremesh.check_band(1.0, 0.5)
    with pytest.raises(ValueError):
        meshremesh.check_band(0.0, 0.5)
    assert meshremesh.MAX_NODES == S.MAX_NODES


def test_command_line():
    from geobi_gnn_amd.__main__ import parse_args
    opt = parse_args(['remesh', '--data_dir', 'x'])
    assert (opt.target_edge, opt.target_edge_diag, opt.iterations, opt.feature_angle, opt.relax_lambda, opt.max_rounds,
            opt.gpu, opt.out_dir) == (None, None, 5, 40.0, 0.5, 64, -1, '')
    opt = parse_args(['remesh', '--data_dir', 'x', '--target_edge_diag', '0.02', '--iterations', '3', '--feature_angle', '180'])
    assert (opt.target_edge_diag, opt.iterations, opt.feature_angle) == (0.02, 3, 180.0)
    for bad in (['--target_edge', '1', '--target_edge_diag', '0.1'], ['--target_edge', '0'], ['--iterations', '-1'],
                ['--feature_angle', '100'], ['--relax_lambda', '2'], ['--max_rounds', '0']):
        with pytest.raises(SystemExit):
            parse_args(['remesh', '--data_dir', 'x'] + bad)


def test_size_limits():
    """the entry points refuse F or V beyond GEOBI_MAX_NODES before anything touches the device; the size query gives 0"""
    import ctypes
    from geobi_gnn_amd import _lib as L
    lib = L.lib()
    big = S.MAX_NODES + 1
    one = ctypes.c_void_p(256)                     # never dereferenced: the size check comes first
    for F, V in ((big, 10), (10, big)):
        assert lib.geobi_remesh_ws_bytes(F, V) == 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
        calls = (lambda: lib.geobi_remesh_lock(one, one, F, V, 1, 0.5, one, one, one, 1 << 20, None),
                 lambda: lib.geobi_decim_plan_short(one, one, one, F, V, 1.0, 2.0, one, None, one, 1 << 20, None),
                 lambda: lib.geobi_flip_plan(one, one, one, F, V, 1, 0.5, one, None, one, 1 << 20, None),
                 lambda: lib.geobi_flip_emit(one, F, V, one, one, 1 << 20, None),
                 lambda: lib.geobi_relax(one, one, one, F, V, 0.5, one, one, None, one, 1 << 20, None),
                 lambda: lib.geobi_remesh_stats(one, one, F, V, one, one, one, 1 << 20, None))
        for call in calls:
            assert call() != 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
    assert lib.geobi_remesh_ws_bytes(-1, 4) == 0 and lib.geobi_remesh_ws_bytes(100, 60) > 0
    assert lib.geobi_decim_plan_short(one, one, one, 10, 10, 2.0, 1.0, one, None, one, 1 << 20, None) != 0
    assert b'low' in lib.geobi_last_error()
    assert lib.geobi_flip_plan(one, one, one, 10, 10, 1, 1.5, one, None, one, 1 << 20, None) != 0
    assert b'c2' in lib.geobi_last_error()
    assert lib.geobi_relax(one, one, one, 10, 10, 1.5, one, one, None, one, 1 << 20, None) != 0
    assert b'lambda' in lib.geobi_last_error()
