"""The sequential model of the refinement rules (tests/subdiv_model.py) pinned on facts that do not come from it, the
comparison helper of the GPU test caught on planted faults, and the parts of the feature that run without a GPU: the
command line and the size limits of the entry points."""
import copy
import ctypes

import numpy as np
import pytest

import subdiv_model as M
from train_cases import _run

# coordinates on a dyadic grid: every midpoint of the passes below is exact in float32, so the pieces of a face tile it
# exactly and the fp64 area can only move by the rounding of its own sum (the 1e-12 below); with coordinates that use all
# 24 bits a + b already rounds and the area moves at the float32 level
CLOSED = {'box': M.box, 'icosahedron': lambda: M.icosahedron(snap=64), 'tetrahedron': M.tetrahedron}


def _euler(points, faces):
    used = np.unique(np.asarray(faces)).shape[0]
    return used - M.edge_facts(faces)['E'] + np.asarray(faces).shape[0]


@pytest.mark.parametrize('name', sorted(CLOSED))
@pytest.mark.parametrize('mode', ['midpoint', 'loop', 'max_edge'])
def test_closed_inputs_stay_closed_pass_by_pass(name, mode):
    points, faces = CLOSED[name]()
    euler, area = _euler(points, faces), M.area(points, faces)
    assert euler == 2
    L = 0.45 * float(np.sqrt(M.longest_edge2(points, faces)))
    for _ in range(3):
        points, faces, parent, vertex_parents, counts, _ = M.one_pass(points, faces, mode == 'loop', L if mode == 'max_edge' else None)
        facts = M.edge_facts(faces)
        assert _euler(points, faces) == euler and np.unique(faces).shape[0] == points.shape[0]
        assert facts['boundary'] == 0 and facts['complex'] == 0 and facts['repeated'] == 0
        assert counts['boundary_edges'] == 0 and counts['complex_edges'] == 0
        assert vertex_parents.shape == (points.shape[0], 2) and parent.shape == (faces.shape[0],)
        if mode != 'loop':
            assert abs(M.area(points, faces) - area) <= 1e-12 * area
    if mode == 'max_edge':
        assert M.subdivide(*CLOSED[name](), max_edge=L).counts['passes'] >= 2


def test_box_uniform_pass():
    r = M.subdivide(*M.box(), levels=1)
    assert (r.points.shape[0], r.faces.shape[0], M.edge_facts(r.faces)['E']) == (26, 48, 72)
    assert r.counts == {'edges': 18, 'split': 18, 'boundary_edges': 0, 'complex_edges': 0, 'passes': 1}


@pytest.mark.parametrize('L, want', [(2.5, (16, 28, 42, 1)), (1.2, (50, 96, 144, 2)), (0.5, (242, 480, 720, 4)),
                                     (0.2, (1794, 3584, 5376, 5))])
def test_box_max_edge(L, want):
    points, faces = M.box()
    r = M.subdivide(points, faces, max_edge=L)
    assert (r.points.shape[0], r.faces.shape[0], M.edge_facts(r.faces)['E'], r.counts['passes']) == want
    assert M.longest_edge2(r.points, r.faces) <= np.float64(np.float32(L)) ** 2
    assert abs(M.area(r.points, r.faces) - 22.0) <= 22.0 * 1e-12
    assert np.array_equal(np.bincount(r.face_parent, minlength=12) > 0, np.ones(12, dtype=bool))
    if want[3] > 1:
        with pytest.raises(M.TooManyRounds):
            M.subdivide(points, faces, max_edge=L, max_rounds=want[3] - 1)


def test_strict_comparison_and_templates():
    points, faces, L = M.exact_length()
    _, _, parent, vertex_parents, counts, _ = M.one_pass(points, faces, False, L)
    assert counts['split'] == 2 and [0, 1] not in vertex_parents[5:].tolist()     # the edge of length exactly 5 stays
    points, faces, L = M.mixed_templates()
    parent = M.one_pass(points, faces, False, L)[2]
    assert set(np.bincount(parent).tolist()) == {1, 2, 3, 4}
    tie = [M.one_pass(*M.isosceles(v)[:2], False, M.isosceles(v)[2])[1].tolist() for v in range(4)]
    # p = the midpoint of edge u + 1, q = of edge u + 2; the lower edge id wins the tie: (a, b, p) when it is edge u + 1
    assert tie[0][1:] == [[0, 1, 3], [1, 4, 3]] and tie[1][1:] == [[1, 0, 3], [1, 3, 4]]
    assert tie[2][1:] == [[1, 2, 3], [2, 4, 3]] and tie[3][1:] == [[2, 1, 3], [2, 3, 4]]


def test_loop_masks():
    # a regular planar grid: the interior valence-6 vertices stay, the plane stays a plane
    points, faces = M.grid(6, 5, regular=True)
    out = M.one_pass(points, faces, True)[0]
    interior = [i * 6 + j for i in range(1, 6) for j in range(1, 5)]
    assert np.array_equal(M.bits(out[interior]), M.bits(points[interior]))
    assert np.array_equal(out[:, 2].astype(np.float64), 0.5 * out[:, 0].astype(np.float64) - 0.25 * out[:, 1].astype(np.float64))
    # a boundary vertex: 3/4, 1/8, 1/8 of itself and its two boundary neighbours (vertex 2 on the side i = 0: 1 and 3)
    rough, _ = M.grid(6, 5, seed=4)
    got = M.one_pass(rough, faces, True)[0]
    r64 = rough.astype(np.float64)
    assert np.array_equal(got[2], (0.75 * r64[2] + 0.125 * (r64[1] + r64[3])).astype(np.float32))
    # a tetrahedron: valence 3 everywhere, beta = 3/16 -> 7/16 of the vertex and 3/16 of the sum of the others
    tp, tf = M.tetrahedron()
    t64 = tp.astype(np.float64)
    got = M.one_pass(tp, tf, True)[0]
    for v in range(4):
        others = [w for w in range(4) if w != v]
        want = (1.0 - 3 * (3.0 / 16.0)) * t64[v] + (3.0 / 16.0) * ((t64[others[0]] + t64[others[1]]) + t64[others[2]])
        assert np.array_equal(got[v], want.astype(np.float32))
    assert M.sharp_of(*M.sharp_counts()).tolist() == [3, 1, 1, 1, 0, 0, 0, 0, 0, 0, 2, 2, 2]


def test_apply_of_the_input_is_the_output():
    for scheme in ('midpoint', 'loop'):
        points, faces = M.grid(4, 3, seed=2)
        r = M.subdivide(points, faces, levels=2, scheme=scheme)
        assert np.array_equal(M.bits(M.apply(r, points)), M.bits(r.points))


def test_planted_faults_are_caught():
    points, faces, L = M.mixed_templates()
    want = M.subdivide(points, faces, max_edge=L)
    M.assert_same(copy.deepcopy(want), want)
    # a swapped diagonal in a two-split face: (a, b, p) (a, p, q) <-> (a, b, q) (b, p, q)
    parent = M.one_pass(points, faces, False, L)[2]
    f = int(np.nonzero(np.bincount(parent) == 3)[0][0])
    one = M.one_pass(points, faces, False, L)
    rows = np.nonzero(parent == f)[0]
    swapped = one[1].copy()
    (p, c, q), second, third = swapped[rows[0]], swapped[rows[1]], swapped[rows[2]]
    a, b = second[0], second[1]
    swapped[rows[1]], swapped[rows[2]] = ((a, b, q), (b, p, q)) if second[2] == p else ((a, b, p), (a, p, q))
    first_pass = M.Refined(one[0], one[1], one[2], one[3], one[4], None, None)
    bad = copy.deepcopy(first_pass)
    bad.faces = swapped
    with pytest.raises(AssertionError, match='faces differ'):
        M.assert_same(bad, first_pass)
    # the children of a face in another order
    bad = copy.deepcopy(first_pass)
    bad.faces[[rows[0], rows[1]]] = bad.faces[[rows[1], rows[0]]]
    with pytest.raises(AssertionError, match='faces differ'):
        M.assert_same(bad, first_pass)
    # a midpoint computed as (a + b) * 0.5 on a pair whose sum overflows
    big = np.array([[3e38, 0, 0], [3e38, 1, 0], [0, 0, 1]], dtype=np.float32)
    good = M.subdivide(big, [[0, 1, 2]])
    assert np.isfinite(good.points).all() and good.points[3, 0] == np.float32(3e38)
    bad = copy.deepcopy(good)
    with np.errstate(over='ignore'):
        bad.points[3] = (big[0] + big[1]) * np.float32(0.5)
    with pytest.raises(AssertionError, match='points differ'):
        M.assert_same(bad, good)
    # and one last bit of one coordinate
    bad = copy.deepcopy(good)
    bad.points.view(np.uint32)[4, 2] ^= 1
    with pytest.raises(AssertionError, match='points differ'):
        M.assert_same(bad, good)


def test_subdivide_help_names_every_flag():
    run = _run(['subdivide', '--help'])
    assert run.returncode == 0
    for flag in ('--data_dir', '--out_dir', '--levels', '--scheme', '--max_edge', '--max_edge_diag', '--max_rounds', '--gpu'):
        assert flag in run.stdout, flag
    from geobi_gnn_amd.__main__ import parse_args
    for args in (['--max_edge', '1', '--max_edge_diag', '0.1'], ['--max_edge', '1', '--levels', '2'],
                 ['--max_edge_diag', '0.1', '--scheme', 'loop'], ['--max_edge', '0'], ['--levels', '0'], ['--max_rounds', '0']):
        with pytest.raises(SystemExit) as e:
            parse_args(['subdivide', '--data_dir', 'nowhere'] + args)
        assert e.value.code == 2, args
    opt = parse_args(['subdivide', '--data_dir', 'd', '--max_edge_diag', '0.05'])
    assert (opt.levels, opt.scheme, opt.max_edge, opt.max_edge_diag, opt.max_rounds) == (1, 'midpoint', None, 0.05, 16)


def test_bad_arguments_are_value_errors_before_any_device_work():
    from geobi_gnn_amd import meshsubdiv
    points, faces = M.box()
    for kw in ({'levels': 0}, {'levels': 1.5}, {'scheme': 'butterfly'}, {'max_edge': 0.0}, {'max_edge': -1.0},
               {'max_edge': float('nan')}, {'max_edge': float('inf')}, {'max_edge': 1e-60}, {'max_rounds': 0},
               {'max_edge': 1.0, 'scheme': 'loop'}, {'max_edge': 1.0, 'levels': 2}):
        with pytest.raises(ValueError):
            meshsubdiv.subdivide(points, faces, **kw)


def test_sizes_beyond_the_documented_limits_are_rejected():
    """geobi_subdiv_*: F or V above GEOBI_MAX_NODES is refused before anything touches the device (no GPU needed)."""
    from geobi_gnn_amd import _lib as L
    lib = L.lib()
    big = (1 << 24)
    one = ctypes.c_void_p(256)                     # never dereferenced: the size check comes first
    assert lib.geobi_subdiv_ws_bytes(big, 10) == 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
    assert lib.geobi_subdiv_ws_bytes(10, big) == 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
    for F, V in ((big, 10), (10, big)):
        rc = lib.geobi_subdiv_plan(one, one, F, V, 0, 0, 0.0, one, None, one, 1 << 20, None)
        assert rc != 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
        rc = lib.geobi_subdiv_emit(one, one, F, V, 0, big, big, one, one, one, one, one, 1 << 20, None)
        assert rc != 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
        rc = lib.geobi_subdiv_points(one, one, F, V, 0, big, one, one, 1 << 20, None)
        assert rc != 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
    # a pass whose output would be too large: refused by emit before anything is written
    rc = lib.geobi_subdiv_emit(one, one, big - 1, 10, 0, 10 + 3 * (big - 1), 4 * (big - 1), one, one, one, one, one, 1 << 20, None)
    assert rc != 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
    rc = lib.geobi_subdiv_plan(one, one, -1, 10, 0, 0, 0.0, one, None, one, 1 << 20, None)
    assert rc != 0 and b'negative' in lib.geobi_last_error()
    rc = lib.geobi_subdiv_plan(one, one, 10, 10, 1, 1, 1.0, one, None, one, 1 << 20, None)
    assert rc != 0 and b'Loop' in lib.geobi_last_error()
