"""tests/project_model.py -- the plain statement of geobi_closest_on_faces, geobi_move_to and the remeshing loop with its
projection step -- pinned on facts that do not come from it, and what of the projection runs without a device (the
argument checks, the command lines, the size limits of the entry points).

Whether a face is THE nearest is judged by the bar of tests/test_gpu_mesheval.py: |d - d_min| / (d_min + e) <= TOL with e
the mean edge of the surface."""
import numpy as np
import pytest

import decim_model as D
import project_model as P
import remesh_model as R
import subdiv_model as S

F32 = np.float32
TOL = 1e-5                      # tests/test_gpu_mesheval.py


def _rel(d, d_ref, e):          # tests/test_gpu_mesheval.py: _rel
    return float((np.abs(np.asarray(d, dtype=np.float64) - d_ref) / (d_ref + e)).max())


_SPHERES = {}


def _sphere(name):
    """(points, faces, L): the UV sphere at its mean edge, the 320-face icosphere at 0.6 mean edges"""
    if name not in _SPHERES:
        points, faces = R.uv_sphere() if name == 'uv' else D.icosphere(4)
        _SPHERES[name] = (points, faces, (1.0 if name == 'uv' else 0.6) * R.mean_edge(points, faces))
    return _SPHERES[name]


_REMESHED = {}


def _remeshed(name, project):
    if (name, project) not in _REMESHED:
        points, faces, L = _sphere(name)
        _REMESHED[name, project] = P.remesh(points, faces, L, feature_angle=180.0, project=project)
    return _REMESHED[name, project]


# ---- closest points
@pytest.mark.parametrize('z', [0.0, 2.0, -3.0])
def test_the_seven_regions_of_a_hand_triangle(z):
    """one query per region of the triangle (0,0) (4,0) (0,4), in, above and below its plane: the region's (v, w), the
    point and the distance known by hand (every number is exact in float32)"""
    for x, y, region, v, w in P.hand_queries():
        c = P.closest([[x, y, z]], P.HAND_TRIANGLE, [[0, 1, 2]])
        assert c.regions == [region] and c.face.tolist() == [0]
        assert c.bary[0].tolist() == [1.0 - v - w, v, w], (x, y, z, c.bary)
        assert c.points[0].tolist() == [4.0 * v, 4.0 * w, 0.0]
        assert c.dist[0] == F32(np.sqrt((x - 4.0 * v) ** 2 + (y - 4.0 * w) ** 2 + z * z))
    # the same triangle with its corners in another order: the weights follow the row
    c = P.closest([[1.0, 2.0, z]], P.HAND_TRIANGLE, [[2, 0, 1]])
    assert c.bary[0].tolist() == [0.5, 0.25, 0.25] and c.points[0].tolist() == [1.0, 2.0, 0.0]


def test_a_mesh_projected_onto_itself_stays():
    """every vertex is a corner of its nearest face: one-hot weights, the point equal to the vertex, distance 0"""
    for points, faces in (D.icosphere(4), R.uv_sphere(), S.grid(5, 4, seed=3)):
        c = P.closest(points, points, faces)
        assert (c.points == points).all() and not c.dist.any()
        assert (np.sort(c.bary, axis=1) == np.array([0, 0, 1], dtype=F32)).all()
        corner = np.asarray(faces)[c.face, np.argmax(c.bary, axis=1)]
        assert np.array_equal(corner, np.arange(points.shape[0]))
        assert (P.apply(c, faces, points) == points).all()
        assert all(r in ('a', 'b', 'c') for r in c.regions)


def test_projected_points_lie_on_their_triangle_and_the_face_is_the_nearest():
    points, faces = D.icosphere(4)
    e, bound = R.mean_edge(points, faces), P.surface_bound(points)
    q = P.shell_queries(300, seed=1)
    c = P.closest(q, points, faces)
    assert set(c.regions) >= {'ab', 'ac', 'bc', 'inside'}                   # the edges and the inside; the corners are the hand cases
    off = P.distance_to_faces(c.points, points, faces, c.face)
    print('off the triangle: max %.3e, bound %.3e' % (off.max(), bound))
    assert off.max() <= bound
    d_min = P.distance_to_surface(q, points, faces)
    assert _rel(P.distance_to_faces(q, points, faces, c.face), d_min, e) <= TOL
    assert _rel(c.dist, d_min, e) <= TOL
    # the distance is that to the float32 point, up to the bound
    assert np.abs(np.linalg.norm(q.astype(np.float64) - c.points, axis=1) - c.dist).max() <= bound + 2.0 ** -24 * 1.3
    assert (c.bary >= 0).all() and (c.bary <= 1).all() and np.abs(c.bary.astype(np.float64).sum(axis=1) - 1).max() <= 2.0 ** -23
    # far from the origin the same holds with the M of the shifted mesh
    shift = (np.array([50.0, -30.0, 20.0]) * e).astype(F32)
    moved = P.closest(q + shift, points + shift, faces)
    off = P.distance_to_faces(moved.points, points + shift, faces, moved.face)
    assert off.max() <= P.surface_bound(points + shift)


def test_triangles_without_area_answer_with_a_point_of_the_triangle():
    queries = P.degenerate_queries()
    for name, verts in sorted(P.degenerate_triangles().items()):
        c = P.closest(queries, verts, [[0, 1, 2]])
        assert np.isfinite(c.bary).all() and np.isfinite(c.points).all() and np.isfinite(c.dist).all(), name
        assert (c.bary >= 0).all() and (c.bary <= 1).all(), name
        lo, hi = verts.min(axis=0), verts.max(axis=0)
        assert ((c.points >= lo) & (c.points <= hi)).all(), name            # on the segment the corners span
        assert (np.abs(np.linalg.norm(queries.astype(np.float64) - c.points, axis=1) - c.dist) <= 1e-6).all(), name
    one = P.closest(queries, P.degenerate_triangles()['one_point'], [[0, 1, 2]])
    assert (one.points == F32([1, 2, 3])).all() and one.regions == ['a'] * len(queries)


def test_exceptions_of_the_rules():
    """a face outside [0, F): zeros; a query that is not finite: +inf, (1, 0, 0), the first corner; ids are clamped"""
    points, faces = D.icosphere(2)
    q = np.array([[0.1, 0.2, 2.0], [np.nan, 0, 0], [0, np.inf, 0], [0.3, 0.3, 0.3], [0.5, 0, 0]], dtype=F32)
    c = P.closest(q, points, faces, face=[3, 5, 7, -1, faces.shape[0]])
    assert not c.bary[3:].any() and not c.points[3:].any() and not c.dist[3:].any()
    assert np.isinf(c.dist[1:3]).all() and (c.bary[1:3] == F32([1, 0, 0])).all()
    assert (c.points[1] == points[faces[5, 0]]).all() and (c.points[2] == points[faces[7, 0]]).all()
    assert np.isfinite(c.dist[0]) and c.dist[0] > 0.9
    wild = np.array([[0, 1, 99], [-5, 1, 2]])
    ref = np.array([[0, 1, points.shape[0] - 1], [0, 1, 2]])
    P.assert_same_closest(P.closest(q[:1], points, wild, face=[0]), P.closest(q[:1], points, ref, face=[0]))
    P.assert_same_closest(P.closest(q[:1], points, wild, face=[1]), P.closest(q[:1], points, ref, face=[1]))


def test_the_float32_fma_rounds_once():
    """against the exact rational value, where a sum rounded to fp64 first would round twice"""
    from fractions import Fraction
    rng = np.random.RandomState(5)
    # 2^-24 (1 - 2^-36) + (1 + 2^-23): a hair below the middle of two float32 values, and the middle itself in fp64
    cases = [(F32(2.0 ** -24 * (1 + 2.0 ** -18)), F32(1 - 2.0 ** -18), F32(1 + 2.0 ** -23)), (F32(3), F32(1 / 3), F32(-1))]
    cases += [tuple(F32(x) for x in rng.randn(3) * 10.0 ** rng.randint(-3, 4, size=3)) for _ in range(2000)]
    for x, y, z in cases:
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        got = float(P.fma32(x, y, z))
        lo, hi = float(np.nextafter(F32(got), F32(-np.inf))), float(np.nextafter(F32(got), F32(np.inf)))
        assert abs(exact - Fraction(got)) <= min(abs(exact - Fraction(lo)), abs(exact - Fraction(hi))), (x, y, z)
    x, y, z = cases[0]
    assert P.fma32(x, y, z) == F32(1 + 2.0 ** -23) and F32(float(x) * float(y) + float(z)) == F32(1 + 2.0 ** -22)


# ---- move_to
def test_move_to_refuses_and_reverts_on_a_noisy_sphere():
    points, faces, target, lock = P.noisy_sphere(P.NOISY_SPHERE_SEED)
    out, counts = P.move_to(points, faces, target, lock)
    assert counts['refused'] > 0 and counts['reverted'] > 0 and counts['moved'] + counts['refused'] <= points.shape[0]
    stayed = (P.bits(out) == P.bits(points)).all(axis=1)
    went = (P.bits(out) == P.bits(target)).all(axis=1)
    assert (stayed | went).all() and int(went.sum()) == counts['moved'] - counts['reverted']
    assert R.closed_manifold(faces) and counts['turned'] <= 2
    # locked vertices and proposals that are not finite
    lock[:40] = 1
    target[50] = np.nan
    out2, counts2 = P.move_to(points, faces, target, lock)
    assert (P.bits(out2[:40]) == P.bits(points[:40])).all() and (P.bits(out2[50]) == P.bits(points[50])).all()
    assert counts2['moved'] < counts['moved']
    # a target equal to the points moves nothing and counts nothing
    assert P.move_to(points, faces, points, np.zeros_like(lock))[1] == dict.fromkeys(R.RELAX_KEYS, 0)
    assert P.move_to(points, np.zeros((0, 3), dtype=np.int32), target, lock)[1] == dict.fromkeys(R.RELAX_KEYS, 0)


def test_move_to_on_the_flat_grid_keeps_the_plane_and_the_rim():
    points, faces, flat, lock = P.lifted_grid(8)
    assert int((lock != 0).sum()) == 32 and int((points[:, 2] != 0).sum()) > 30
    target = P.closest(points, flat, faces).points
    assert not target[:, 2].any()
    out, counts = P.move_to(points, faces, target, lock)
    assert not out[:, 2].any() and (P.bits(out[lock != 0]) == P.bits(points[lock != 0])).all()
    assert counts['moved'] > 30 and counts['refused'] == counts['reverted'] == counts['turned'] == 0
    assert np.abs(out[:, :2] - points[:, :2]).max() <= 2.0 ** -20           # straight down: x and y to rounding


# ---- the loop with its fifth step
@pytest.mark.parametrize('name', ['uv', 'ico'])
def test_remesh_with_projection_stays_on_the_input_surface(name):
    points, faces, L = _sphere(name)
    got, plain = _remeshed(name, True), _remeshed(name, False)
    assert R.closed_manifold(got.faces) and R.euler(0, got.faces) == 2
    assert len(got.per_iteration) == 5 and set(got.per_iteration[0]) == set(R.ITERATION_KEYS + P.PROJECT_KEYS)
    assert set(plain.per_iteration[0]) == set(R.ITERATION_KEYS) and plain.source_face is None and plain.source_bary is None
    last = got.per_iteration[-1]
    assert last['project_refused'] == 0 and last['project_reverted'] == 0 and last['projected'] > 0
    drift, plain_drift = (P.distance_to_surface(r.points, points, faces) for r in (got, plain))
    print('%s: drift max %.3e (bound %.3e), without projection mean %.3e max %.3e; share %.3f / %.3f, valence dev %.3f / %.3f'
          % (name, drift.max(), P.surface_bound(points), plain_drift.mean(), plain_drift.max(), got.after['share'],
             plain.after['share'], got.after['valence_dev'], plain.after['valence_dev']))
    assert drift.max() <= P.surface_bound(points) < plain_drift.max()
    assert plain_drift.max() > 1e-2 and plain_drift.mean() > 1e-3
    assert got.after['share'] > got.before['share'] and got.after['share'] > 0.9
    # the source map: the output vertices come back from it, and a paired array goes through it
    assert got.source_face.shape == (got.points.shape[0],) and got.source_bary.shape == got.points.shape
    # (an output vertex lies within the bound of the surface, its closest point as float32 within the bound of that)
    assert np.linalg.norm(P.apply(got, faces, points).astype(np.float64) - got.points, axis=1).max() <= 2 * P.surface_bound(points)
    again = P.closest(got.points, points, faces, face=got.source_face)
    assert np.array_equal(P.bits(again.bary), P.bits(got.source_bary))
    assert np.array_equal(P.bits(P.apply(got, faces, points)), P.bits(again.points))
    noisy = (points + 0.02 * np.random.RandomState(2).randn(*points.shape)).astype(F32)
    carried = P.apply(got, faces, noisy)
    assert P.distance_to_faces(carried, noisy, faces, got.source_face).max() <= P.surface_bound(noisy)
    assert np.abs(carried - got.points).max() < 0.1


def test_the_fifth_step_runs_under_the_lock_flags_of_the_relaxation():
    """the bumpy sphere at 40 degrees: the sharp bit depends on positions, so the flags taken after the relaxation differ
    from those it ran under; the fifth step uses the latter, and a model that takes them afterwards is caught"""
    points, faces = P.bumpy_sphere()
    L = R.mean_edge(points, faces)
    want = P.remesh(points, faces, L, iterations=2, feature_angle=40.0, project=True)
    differ = [int((before != after).sum()) for before, after in want.locks]
    locked = [int((before != 0).sum()) for before, _ in want.locks]
    print('flags that differ after the relaxation: %s of %s locked' % (differ, locked))
    assert differ[0] > 0 and locked[0] > 10 and locked[0] < points.shape[0]
    # one iteration by hand: the vertices locked BEFORE the relaxation keep the bits the relaxation left them
    low, high = R.band(L)
    relaxed, fv, _, lock = P.iteration(points, faces, low, high, 40.0)
    moved, _ = P.move_to(relaxed, fv, P.closest(relaxed, points, faces).points, lock)
    assert (P.bits(moved[lock != 0]) == P.bits(relaxed[lock != 0])).all()
    after = R.lock_flags(relaxed, fv, 40.0)[0]
    freed = (lock != 0) & (after == 0)
    assert freed.any() or ((lock == 0) & (after != 0)).any()
    wrong = P.remesh(points, faces, L, iterations=2, feature_angle=40.0, project=True, faults=('relock',))
    with pytest.raises(AssertionError):
        P.assert_same(wrong, want, 'relock')
    P.assert_same(P.remesh(points, faces, L, iterations=2, feature_angle=40.0, project=True), want)


def test_no_iterations_give_the_identity_map():
    points, faces, L = _sphere('ico')
    r = P.remesh(points, faces, L, iterations=0, feature_angle=180.0, project=True)
    assert r.per_iteration == [] and np.array_equal(P.bits(r.points), P.bits(points)) and np.array_equal(r.faces, faces)
    assert (np.sort(r.source_bary, axis=1) == np.array([0, 0, 1], dtype=F32)).all()
    other = np.random.RandomState(3).randn(*points.shape).astype(F32)
    assert (P.apply(r, faces, other) == other).all()


def test_another_search_changes_nothing_else():
    """nearest_face is asked for the faces and for nothing else: the model's own search handed in gives the same result"""
    points, faces, L = _sphere('uv')
    calls = []

    def search(q, verts, fv):
        calls.append(q.shape[0])
        return P.nearest_faces(q, verts, fv)
    got = P.remesh(points, faces, L, iterations=2, feature_angle=180.0, project=True, nearest_face=search)
    want = P.remesh(points, faces, L, iterations=2, feature_angle=180.0, project=True)
    P.assert_same(got, want)
    assert len(calls) == 3 and calls[-1] == got.points.shape[0]


# ---- the comparison helper catches planted faults
def _closest_cases():
    points, faces = D.icosphere(4)
    cases = [(P.shell_queries(400, seed=4), points, faces)]
    cases += [(P.degenerate_queries(), verts, np.array([[0, 1, 2]])) for _, verts in sorted(P.degenerate_triangles().items())]
    return cases


@pytest.mark.parametrize('fault', P.CLOSEST_FAULTS)
def test_the_helper_catches_a_faulty_closest_model(fault):
    """the region priority swapped (edges asked before corners); b0 formed as 1 - (v + w)"""
    caught = 0
    for q, verts, faces in _closest_cases():
        face = P.nearest_faces(q, verts, faces)
        want = P.closest(q, verts, faces, face=face)
        P.assert_same_closest(P.closest(q, verts, faces, face=face), want)
        try:
            P.assert_same_closest(P.closest(q, verts, faces, face=face, faults=(fault,)), want, fault)
        except AssertionError as e:
            assert 'differs in' in str(e)
            caught += 1
    assert caught > 0


def test_the_helper_catches_a_move_without_its_guard_and_one_flipped_bit():
    points, faces, target, lock = P.noisy_sphere(P.NOISY_SPHERE_SEED)
    want = P.move_to(points, faces, target, lock)
    P.assert_same_move(P.move_to(points, faces, target, lock), want)
    bare = P.move_to(points, faces, target, lock, guard=False)
    assert bare[1]['refused'] == 0 and bare[1]['turned'] > want[1]['turned']
    with pytest.raises(AssertionError, match='counts'):
        P.assert_same_move(bare, want)
    with pytest.raises(AssertionError, match='points differ in'):
        P.assert_same_move((bare[0], want[1]), want)
    flipped = want[0].copy()
    flipped.view(np.uint32)[17, 1] ^= 1
    with pytest.raises(AssertionError, match='points differ in 1 rows'):
        P.assert_same_move((flipped, want[1]), want)
    c = P.closest(points, *D.icosphere(4))
    other = P.Closest(c.face, c.bary.copy(), c.points, c.dist, c.regions)
    other.bary.view(np.uint32)[5, 0] ^= 1
    with pytest.raises(AssertionError, match='bary differs in 1 rows'):
        P.assert_same_closest(other, c)


# ---- what runs without a device
def test_argument_checks():
    from geobi_gnn_amd import meshproject, meshremesh
    assert meshproject.MAX_NODES == S.MAX_NODES
    for bad in (np.zeros((4, 2)), np.zeros(3), np.zeros((0, 3)), np.zeros((2, 3, 1))):
        with pytest.raises(ValueError, match='closest: '):
            meshproject.check_queries(bad)
        with pytest.raises(ValueError, match='closest: '):
            meshproject.closest(bad, *D.icosphere(1))
        with pytest.raises(ValueError, match='project: '):
            meshproject.project(bad, *D.icosphere(1))
    assert tuple(meshproject.check_queries(np.zeros((5, 3))).shape) == (5, 3)
    for bad in (-1.0, float('nan'), 'far', -0.5):
        with pytest.raises(ValueError, match='max_dist'):
            meshproject.check_max_dist(bad)
        with pytest.raises(ValueError, match='max_dist'):
            meshproject.project(np.zeros((1, 3)), *D.icosphere(1), max_dist=bad)
    assert meshproject.check_max_dist(None) is None and meshproject.check_max_dist(0) == 0.0
    assert meshproject.check_max_dist(float('inf')) == float('inf')
    assert meshremesh.PROJECT_KEYS == P.PROJECT_KEYS and meshremesh.ITERATION_KEYS == R.ITERATION_KEYS
    plain = meshremesh.Remeshed(None, None, 0.8, 1.3, [], {}, {})
    assert plain.source_face is None and plain.source_bary is None
    with pytest.raises(ValueError, match='no map'):
        meshremesh.apply(plain, np.zeros((4, 3)))


def test_command_lines():
    from geobi_gnn_amd.__main__ import parse_args
    assert parse_args(['remesh', '--data_dir', 'x']).project is False
    opt = parse_args(['remesh', '--data_dir', 'x', '--project', '--iterations', '2'])
    assert opt.project is True and opt.iterations == 2
    opt = parse_args(['project', '--data_dir', 'x', '--target_dir', 'y'])
    assert (opt.out_dir, opt.max_dist, opt.max_dist_diag, opt.gpu) == ('', None, None, -1) and opt.fn.__name__ == 'project'
    assert parse_args(['project', '--data_dir', 'x', '--target_dir', 'y', '--max_dist', '0.5']).max_dist == 0.5
    assert parse_args(['project', '--data_dir', 'x', '--target_dir', 'y', '--max_dist_diag', '0.01', '--out_dir', 'o']).max_dist_diag == 0.01
    for bad in (['--max_dist', '1', '--max_dist_diag', '0.1'], ['--max_dist', '-1'], ['--max_dist_diag', 'nan']):
        with pytest.raises(SystemExit):
            parse_args(['project', '--data_dir', 'x', '--target_dir', 'y'] + bad)
    with pytest.raises(SystemExit):
        parse_args(['project', '--data_dir', 'x'])


def test_size_limits():
    """the new entry points refuse sizes beyond GEOBI_MAX_NODES, and an empty side, before anything touches the device"""
    import ctypes
    from geobi_gnn_amd import _lib as L
    lib = L.lib()
    big = S.MAX_NODES + 1
    one = ctypes.c_void_p(256)                     # never dereferenced: the size check comes first
    for Q, V, F in ((big, 10, 10), (10, big, 10), (10, 10, big)):
        assert lib.geobi_closest_on_faces(one, one, one, one, Q, V, F, one, one, one, None) != 0
        assert b'GEOBI_MAX_NODES' in lib.geobi_last_error()
    for Q, V, F in ((0, 10, 10), (10, 0, 10), (10, 10, 0)):
        assert lib.geobi_closest_on_faces(one, one, one, one, Q, V, F, one, one, one, None) != 0
        assert b'at least one' in lib.geobi_last_error()
    assert lib.geobi_closest_on_faces(one, one, one, None, 10, 10, 10, one, one, one, None) != 0
    assert b'face is NULL' in lib.geobi_last_error()
    for F, V in ((big, 10), (10, big)):
        assert lib.geobi_move_to(one, one, one, one, F, V, one, one, None, one, 1 << 20, None) != 0
        assert b'GEOBI_MAX_NODES' in lib.geobi_last_error()
    assert lib.geobi_move_to(one, one, None, one, 10, 10, one, one, None, one, 1 << 20, None) != 0
    assert b'target is NULL' in lib.geobi_last_error()
