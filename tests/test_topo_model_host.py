"""Mesh topology on the host: the breadth-first statement of tests/topo_model.py against its plain simulation of the
synchronous hooking rounds, the hand cases, the point of the feature on a half-flipped sphere, and the command line's new
flags.  No device."""
import numpy as np
import pytest

import clean_model as M
import topo_model as T


def _both(faces, state=None):
    """labels, parities in orientable components, bad components: breadth-first walk == hooking rounds, for both link sets"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    F, inc = faces.shape[0], T.included(faces, state)
    out = []
    for link_list in T.links(faces, state):
        label, parity, bad = T.bfs(F, link_list, inc)
        label_r, parity_r, bad_r, rounds = T.rounds_result(F, link_list, inc)
        assert np.array_equal(label, label_r) and bad == bad_r
        good = inc & ~np.isin(label, sorted(bad))
        assert np.array_equal(parity[good], parity_r[good])
        out.append((label, parity, bad, rounds))
    return out


# ------------------------------------------------------------------------------------------------ hand cases
def test_hand_cases():
    for name, (V, faces) in sorted(T.HAND.items()):
        _both(faces)
    o = T.orient(T.HAND['two_consistent'][1])
    assert o.flip.tolist() == [0, 0] and o.label.tolist() == [0, 0] and o.counts['rounds'] == 1
    o = T.orient(T.HAND['two_inconsistent'][1])
    assert o.flip.tolist() == [0, 1] and o.faces.tolist() == [[0, 1, 2], [1, 3, 2]]
    o = T.orient(T.HAND['tetrahedron_face1_reversed'][1])
    assert o.flip.tolist() == [0, 1, 0, 0] and o.counts['components'] == 1
    for n in (5, 41):
        o = T.orient(T.moebius(n))
        assert o.counts == dict(o.counts, components=1, nonorientable=1, flipped=0) and not o.flip.any()
    o, c = T.orient(T.HAND['three_on_one_edge'][1]), T.components(T.HAND['three_on_one_edge'][1])
    assert o.label.tolist() == [0, 1, 2] and o.counts['rounds'] == 0 and c.label.tolist() == [0, 0, 0]
    for name in ('duplicate_same', 'duplicate_opposite'):
        o, c = T.orient(T.HAND[name][1]), T.components(T.HAND[name][1])
        assert o.label.tolist() == [0, 1] and not o.flip.any() and c.label.tolist() == [0, 0]
    c = T.components(T.HAND['bow_tie'][1])
    assert c.label.tolist() == [0, 1] and c.counts['components'] == 2
    o, c = T.orient(T.HAND['degenerate_between'][1]), T.components(T.HAND['degenerate_between'][1], None, 3)
    assert o.label.tolist() == [0, -1, 0, -1] and c.state.tolist() == [4, 3, 4, 3]
    assert c.counts == {'components': 1, 'components_dropped': 1, 'faces_dropped': 2, 'rounds': 1}
    o = T.orient([[0, 1, 2], [1, 2, 3]], state=[1, 2])
    assert o.label.tolist() == [0, -1] and o.counts['components'] == 1
    assert T.orient([]).counts == {'components': 0, 'nonorientable': 0, 'flipped': 0, 'rounds': 0}


def test_rounds_reproduce_the_walk_on_random_meshes():
    rng = np.random.RandomState(7)
    nonorientable, flipped, complex_edges = 0, 0, 0
    for k in range(400):
        V, F = rng.randint(3, 12), rng.randint(0, 40)
        faces = rng.randint(0, V, size=(F, 3))
        if k % 4 == 0:                                # a Moebius band on vertices of its own, in among the rest
            faces = np.concatenate([faces, T.mess_up(T.moebius(5 + 2 * (k % 3)) + V, k)])[rng.permutation(F + 5 + 2 * (k % 3))]
        state = rng.randint(1, 4, size=faces.shape[0]) if k % 2 else None
        (_, parity, bad, _), _ = _both(faces, state)
        nonorientable += len(bad)
        flipped += int(parity.sum())
        complex_edges += T.report_counts(faces, state)['complex_edges']
    assert nonorientable >= 100 and flipped > 200 and complex_edges > 200          # the sample reaches all of them


def test_rounds_stay_small_on_the_inputs_of_the_gpu_tests():
    names = []
    for name, faces, state in T.device_inputs():
        (_, _, _, rounds_o), (_, _, _, rounds_c) = _both(faces, state)
        assert rounds_o <= 32 and rounds_c <= 32, name
        names.append(name)
    assert len(names) == 11 + 11 + 5 + 20 + 1 and 'moebius41' in names and 'strip4096' in names
    points, faces = T.three_parts()                               # through clean_mesh: components of the KEPT faces
    for m in (20, 21, 81):
        assert T.clean(points, faces, min_component=m).topology['component_rounds'] <= 32
    ball, table, _ = T.command_ball()
    t = T.clean(ball, table, orient_faces=True, min_component=2).topology
    assert t['orient_rounds'] <= 32 and t['component_rounds'] <= 32
    assert T.clean(np.zeros((10, 3), np.float32) + np.arange(10)[:, None], T.displaced(),
                   min_component=2).topology['component_rounds'] <= 32
    assert T.orient(T.size_cases()['strip4096'][1]).counts['rounds'] > 8          # and they are not trivial either
    rng = np.random.RandomState(2025)
    for k in range(300):
        p, faces = T.fuzz_mesh(rng, k)
        t = T.clean(p, faces, weld_tol=(0.0, 1.0)[k % 2], orient_faces=True, min_component=2).topology
        assert t['orient_rounds'] <= 32 and t['component_rounds'] <= 32


def test_orienting_first_saves_the_faces_the_half_edge_rule_would_drop():
    p, faces = T.sphere(2)
    mixed = T.mess_up(faces, 102, shuffle=False)
    alone = M.clean(p, mixed)
    assert alone.counts['nonmanifold'] > 20 and alone.counts['rounds'] > 1
    both = T.clean(p, mixed, orient_faces=True)
    assert both.counts == {'welded': 0, 'degenerate': 0, 'nonmanifold': 0, 'unreferenced': 0, 'rounds': 1}
    assert both.faces.shape[0] == 80 and both.topology['flipped'] == int(both.face_flip.sum()) > 0
    # face 0 decides: the result is the sphere, or the sphere with every face reversed
    want = faces if np.array_equal(mixed[0], faces[0]) else faces[:, [0, 2, 1]]
    assert np.array_equal(both.faces, want)


def test_small_parts():
    p2, f2 = T.sphere(2)
    p1, f1 = T.sphere(1)
    faces = np.concatenate([f1, f2 + 12, [[54, 55, 56]]])
    c = T.components(faces, None, 20)
    assert c.counts == dict(c.counts, components=3, components_dropped=1, faces_dropped=1) and c.state.tolist() == [1] * 100 + [4]
    assert T.components(faces, None, 21).counts['faces_dropped'] == 21
    assert T.components(faces, None, 81).counts == dict(c.counts, components_dropped=3, faces_dropped=101)
    # face 0 takes 0 -> 1 from the strip's first face and is then dropped as a small part: that face stays dropped
    pts = (np.arange(30).reshape(10, 3) ** 2).astype(np.float32)
    r = T.clean(pts, np.concatenate([[[0, 1, 9]], T.strip(6)]), min_component=2)
    assert r.face_map.tolist() == [2, 3, 4, 5, 6] and r.counts['nonmanifold'] == 1
    assert r.topology == dict(r.topology, components=2, components_dropped=1, faces_dropped=1)
    assert r.vertex_map.tolist() == [-1, 0, 1, 2, 3, 4, 5, 6, -1, -1]


def test_report():
    p, faces = T.sphere(2)
    r = T.report(p, faces)
    assert r['closed'] and r['euler'] == 2 and r['components'] == 1 and r['edges'] == 120 and r['would_flip'] == 0
    r = T.report(p, faces[1:])
    assert not r['closed'] and r['boundary_edges'] == 3 and r['euler'] == 1
    r = T.report(np.arange(15, dtype=np.float32).reshape(5, 3) ** 2, T.moebius(5))
    assert r['nonorientable'] == 1 and r['euler'] == 0 and r['boundary_edges'] == 5 and r['inconsistent_edges'] == 5


# ------------------------------------------------------------------------------------------------ command line
def _parse(argv):
    from geobi_gnn_amd.__main__ import parse_args
    return parse_args(argv)


def test_clean_topology_flags():
    opt = _parse(['clean', '--data_dir', 'd'])
    assert not getattr(opt, 'orient', False) and getattr(opt, 'min_component', 0) == 0
    opt = _parse(['clean', '--data_dir', 'd', '--orient', '--min_component', '25'])
    assert opt.orient is True and opt.min_component == 25
    opt = _parse(['denoise', '--data_dir', 'd', '--method', 'bnf', '--clean', '--orient', '--min_component', '3'])
    assert opt.clean and opt.orient is True and opt.min_component == 3
    for argv in (['clean', '--data_dir', 'd', '--min_component', '-1'], ['clean', '--data_dir', 'd', '--min_component', 'x'],
                 ['denoise', '--data_dir', 'd', '--orient'], ['denoise', '--data_dir', 'd', '--min_component', '5'],
                 ['denoise', '--data_dir', 'd', '--clean', '--min_component', '-2']):
        with pytest.raises(SystemExit) as e:
            _parse(argv)
        assert e.value.code == 2, argv


def test_info_command_parses():
    opt = _parse(['info', '--data_dir', 'd'])
    assert opt.command == 'info' and opt.weld_tol == 0.0 and not opt.no_weld and opt.gpu == -1 and callable(opt.fn)
    opt = _parse(['info', '--data_dir', 'd', '--weld_tol', '0.5', '--gpu', '0'])
    assert opt.weld_tol == 0.5 and opt.gpu == 0
    assert _parse(['info', '--data_dir', 'd', '--no_weld']).no_weld
    with pytest.raises(SystemExit):
        _parse(['info', '--data_dir', 'd', '--weld_tol', '-1'])
    with pytest.raises(SystemExit):
        _parse(['info'])
