"""Mesh topology on the device (csrc/topo.hip, geobi_gnn_amd/meshtopo.py, clean_mesh(orient=, min_component=)) against
the sequential model of tests/topo_model.py, and the `clean --orient --min_component`, `denoise --clean --orient` and
`info` commands end to end.

Every comparison is EXACT: integer arrays equal, points bit-equal, the counts (the numbers of rounds included) equal.
There are no tolerances."""
import os

import numpy as np
import pytest
import torch

import clean_model as M
import topo_model as T
from train_cases import _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


def _pts(n, seed=0):
    rng = np.random.RandomState(seed)
    return (rng.rand(n, 3) + np.arange(n)[:, None]).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, name):
    assert got.dtype == torch.int32 and got.is_cuda, name
    assert np.array_equal(got.cpu().numpy(), np.asarray(want)), name


_MODELS = {}


def _model(name, faces, state=None, min_component=0):
    """the model's answers, computed once per named input"""
    key = (name, min_component)
    if key not in _MODELS:
        _MODELS[key] = (T.orient(faces, state), T.components(faces, state, min_component))
    return _MODELS[key]


def _check_topo(dev, name, V, faces, state=None, min_component=0):
    """orient_faces and face_components against the model, everything exact -> (device orient, device components)"""
    from geobi_gnn_amd import meshtopo
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    mo, mc = _model(name, faces, state, min_component)
    o = meshtopo.orient_faces(faces, V, state=state, device=dev)
    assert o.counts == mo.counts, name
    assert o.faces.shape == (faces.shape[0], 3)
    for field in ('faces', 'flip', 'label'):
        _same(getattr(o, field), getattr(mo, field), '%s %s' % (name, field))
    c = meshtopo.face_components(faces, V, state=state, min_component=min_component, device=dev)
    assert c.counts == mc.counts, name
    _same(c.label, mc.label, name + ' comp')
    _same(c.state, mc.state, name + ' state')
    return o, c


def _check_clean(dev, points, faces, model=None, **kw):
    """clean_mesh(orient=, min_component=) against the model's composition, every field and count"""
    from geobi_gnn_amd import meshclean
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    r = meshclean.clean_mesh(points, faces, weld_tol=kw.get('weld_tol', 0.0), manifold=kw.get('manifold', True),
                             orient=kw.get('orient', False), min_component=kw.get('min_component', 0), device=dev)
    m = model or T.clean(points, faces, weld_tol=kw.get('weld_tol', 0.0), manifold=kw.get('manifold', True),
                         orient_faces=kw.get('orient', False), min_component=kw.get('min_component', 0))
    assert r.counts == m.counts and r.topology == m.topology
    for name in ('canon', 'vertex_map', 'vertex_src', 'face_map', 'faces'):
        _same(getattr(r, name), getattr(m, name), name)
    assert np.array_equal(_bits(r.points.cpu().numpy()), _bits(m.points))
    if kw.get('orient', False):
        _same(r.face_flip, m.face_flip, 'face_flip')
    else:
        assert r.face_flip is None
    return r, m


# ------------------------------------------------------------------------------------------------ hand cases
@pytest.mark.parametrize('name', sorted(T.HAND))
def test_hand_cases(dev, name):
    V, faces = T.HAND[name]
    o, c = _check_topo(dev, name, V, faces)
    if name == 'two_consistent':
        assert o.flip.tolist() == [0, 0] and o.label.tolist() == [0, 0]
    if name == 'two_inconsistent':
        assert o.flip.tolist() == [0, 1] and o.faces.tolist() == [[0, 1, 2], [1, 3, 2]]
    if name == 'tetrahedron_face1_reversed':
        assert o.flip.tolist() == [0, 1, 0, 0] and o.counts['flipped'] == 1
    if name.startswith('moebius'):
        assert not bool(o.flip.any()) and o.counts['nonorientable'] == 1 and o.counts['components'] == 1
    if name == 'three_on_one_edge':
        assert o.label.tolist() == [0, 1, 2] and o.counts['rounds'] == 0 and c.label.tolist() == [0, 0, 0]
    if name.startswith('duplicate'):
        assert o.label.tolist() == [0, 1] and not bool(o.flip.any())
        # the half-edge rule treats duplicates as it does today
        today = M.clean(_pts(V), faces)
        r, _ = _check_clean(dev, _pts(V), faces, orient=True)
        assert r.counts == today.counts and np.array_equal(r.faces.cpu().numpy(), today.faces)
        assert np.array_equal(r.face_map.cpu().numpy(), today.face_map)
    if name == 'bow_tie':
        assert c.label.tolist() == [0, 1] and c.counts['components'] == 2
    if name == 'degenerate_between':
        assert o.label.tolist() == [0, -1, 0, -1] and c.label.tolist() == [0, -1, 0, -1] and c.state.tolist() == [1, 3, 1, 3]
    if name == 'no_faces':
        assert o.faces.shape == (0, 3) and o.flip.shape == (0,) and c.label.shape == (0,)
        assert o.counts == {'components': 0, 'nonorientable': 0, 'flipped': 0, 'rounds': 0}


def test_excluded_states(dev):
    V, faces, state = T.EXCLUDED
    o, c = _check_topo(dev, 'excluded', V, faces, state=np.array(state, dtype=np.int32), min_component=2)
    assert o.label.tolist() == [0, -1, 2, -1, 2] and o.flip.tolist() == [0, 0, 0, 0, 1]
    assert c.state.tolist() == [4, 2, 1, 3, 1] and c.counts['faces_dropped'] == 1


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize('name', sorted(T.size_cases()))
def test_sizes_against_the_model(dev, name):
    V, faces = T.size_cases()[name]
    o, c = _check_topo(dev, name, V, faces)
    assert o.counts['nonorientable'] == 0
    if name.startswith('strip') or name.startswith('sphere'):
        assert o.counts['components'] == 1 and 0 < o.counts['flipped'] < faces.shape[0] and o.counts['rounds'] >= 4
    if name == 'parts':
        assert o.counts['components'] == 3 and c.counts['components'] == 3
    if name == 'soup':
        assert o.counts['components'] == 80 and o.counts['rounds'] == 0 and c.counts['rounds'] == 0
        assert o.label.tolist() == list(range(80))


@pytest.mark.parametrize('n', [2, 32])
def test_orienting_a_half_flipped_sphere_saves_its_faces(dev, n):
    from geobi_gnn_amd import meshclean
    points, faces = T.sphere(n)
    mixed = T.size_cases()['sphere%d' % n][1]
    plain = meshclean.clean_mesh(points, mixed, device=dev)
    assert plain.counts['nonmanifold'] > 0
    mo, _ = _model('sphere%d' % n, mixed)
    model = T.clean(points, mixed, orient_faces=True) if n == 2 else None
    r = meshclean.clean_mesh(points, mixed, orient=True, device=dev)
    if model is not None:
        _check_clean(dev, points, mixed, model=model, orient=True)
    assert r.counts == {'welded': 0, 'degenerate': 0, 'nonmanifold': 0, 'unreferenced': 0, 'rounds': 1}
    _same(r.face_flip, mo.flip, 'flip')
    assert r.topology == {'flipped': mo.counts['flipped'], 'nonorientable': 0, 'orient_components': 1,
                          'orient_rounds': mo.counts['rounds']}
    # the original sphere's faces, up to the winding face 0 of the file decides for all
    def rows(f):
        f = np.asarray(f)
        k = f.argmin(axis=1)
        f = np.stack([f[np.arange(len(f)), (k + j) % 3] for j in range(3)], axis=1)       # rotated to start at the lowest corner
        return f[np.lexsort(f.T[::-1])]
    got = r.faces.cpu().numpy()
    assert np.array_equal(rows(got), rows(faces)) or np.array_equal(rows(got), rows(faces[:, [0, 2, 1]]))


def test_orientation_is_per_component(dev):
    points, faces = T.two_spheres_and_a_triangle()
    r, m = _check_clean(dev, points, faces, orient=True)
    assert r.counts['nonmanifold'] == 0 and r.faces.shape[0] == 101
    assert r.topology['orient_components'] == 3 and r.topology['nonorientable'] == 0 and r.topology['flipped'] > 0


# ------------------------------------------------------------------------------------------------ min_component
@pytest.mark.parametrize('m, kept', [(20, 100), (21, 80), (81, 0)])
def test_min_component(dev, m, kept):
    points, faces = T.three_parts()
    r, _ = _check_clean(dev, points, faces, min_component=m)
    assert r.faces.shape[0] == kept and r.topology['components'] == 3 and r.topology['faces_dropped'] == 101 - kept
    assert r.counts['unreferenced'] == {100: 3, 80: 15, 0: 57}[kept] and r.counts['nonmanifold'] == 0


def test_a_dropped_small_part_does_not_give_its_half_edges_back(dev):
    r, _ = _check_clean(dev, _pts(10), T.displaced(), min_component=2)
    assert r.face_map.tolist() == [2, 3, 4, 5, 6] and r.counts['nonmanifold'] == 1
    assert r.topology['components_dropped'] == 1 and r.topology['faces_dropped'] == 1


# ------------------------------------------------------------------------------------------------ fuzz, determinism
def test_fuzz_against_the_model(dev):
    rng = np.random.RandomState(2025)
    flipped = dropped = 0
    for k in range(300):
        p, faces = T.fuzz_mesh(rng, k)
        r, m = _check_clean(dev, p, faces, weld_tol=(0.0, 1.0)[k % 2], manifold=k % 7 != 6, orient=True, min_component=2)
        flipped += m.topology['flipped']
        dropped += m.topology['faces_dropped']
    assert flipped > 100 and dropped > 100          # the sample does reach both


def test_two_calls_are_bit_identical(dev):
    from geobi_gnn_amd import meshclean, meshtopo
    points, _ = T.sphere(32)
    mixed = T.size_cases()['sphere32'][1]
    a = meshclean.clean_mesh(points, mixed, orient=True, min_component=5, device=dev)
    b = meshclean.clean_mesh(points, mixed, orient=True, min_component=5, device=dev)
    assert a.counts == b.counts and a.topology == b.topology
    for name in ('points', 'faces', 'vertex_map', 'vertex_src', 'face_map', 'canon', 'face_flip'):
        assert torch.equal(getattr(a, name).view(torch.int32), getattr(b, name).view(torch.int32)), name
    V, strip = T.size_cases()['strip4096']
    x, y = meshtopo.orient_faces(strip, V, device=dev), meshtopo.orient_faces(strip, V, device=dev)
    assert x.counts == y.counts and torch.equal(x.flip, y.flip) and torch.equal(x.label, y.label)


def test_no_faces_through_clean_mesh(dev):
    """The stages hand on tables padded to one row; whatever that row holds, an empty table has no component."""
    from geobi_gnn_amd import meshclean
    for _ in range(4):                   # leave freed 12- and 4-byte blocks that hold a valid face and the state "kept"
        junk = [torch.tensor([[0, 1, 2]], dtype=torch.int32, device=dev) for _ in range(8)]
        junk += [torch.ones(1, dtype=torch.int32, device=dev) for _ in range(8)]
        torch.cuda.synchronize()
        del junk
        r, _ = _check_clean(dev, _pts(5), np.zeros((0, 3), dtype=np.int32), orient=True, min_component=2)
        assert r.counts == {'welded': 0, 'degenerate': 0, 'nonmanifold': 0, 'unreferenced': 5, 'rounds': 0}
        assert r.topology == {'flipped': 0, 'nonorientable': 0, 'orient_components': 0, 'orient_rounds': 0, 'components': 0,
                              'components_dropped': 0, 'faces_dropped': 0, 'component_rounds': 0}
        assert r.faces.shape == (0, 3) and r.face_flip.shape == (0,) and r.points.shape == (0, 3)


def test_defaults_leave_the_result_as_it_was(dev):
    from geobi_gnn_amd import meshclean
    sp, sf = M.soup(*T.sphere(2))
    r = meshclean.clean_mesh(sp, sf, device=dev)
    assert r.topology is None and r.face_flip is None
    assert r.counts == M.clean(sp, sf).counts and sorted(r.counts) == ['degenerate', 'nonmanifold', 'rounds', 'unreferenced',
                                                                       'welded']


# ------------------------------------------------------------------------------------------------ errors, report
def test_max_rounds_is_an_error_and_the_next_call_works(dev):
    from geobi_gnn_amd import meshclean, meshtopo
    from geobi_gnn_amd._lib import GeobiError
    V, strip = T.size_cases()['strip4096']
    mo, _ = _model('strip4096', strip)
    with pytest.raises(GeobiError, match='max_rounds'):
        meshtopo.orient_faces(strip, V, max_rounds=1, device=dev)
    with pytest.raises(GeobiError, match='max_rounds'):
        meshtopo.face_components(strip, V, max_rounds=1, device=dev)
    assert meshtopo.orient_faces(strip, V, device=dev).counts == mo.counts
    # exactly as many rounds as it takes is enough, one fewer is not
    assert meshtopo.orient_faces(strip, V, max_rounds=mo.counts['rounds'], device=dev).counts == mo.counts
    with pytest.raises(GeobiError, match='max_rounds'):
        meshtopo.orient_faces(strip, V, max_rounds=mo.counts['rounds'] - 1, device=dev)
    with pytest.raises(ValueError, match='max_rounds'):
        meshtopo.orient_faces(strip, V, max_rounds=0, device=dev)
    with pytest.raises(ValueError, match='min_component'):
        meshtopo.face_components(strip, V, min_component=-1, device=dev)
    with pytest.raises(ValueError, match='min_component'):
        meshclean.clean_mesh(_pts(V), strip, min_component=-1, device=dev)
    for wrong in ([[0, 1, V]], [[0, -1, 2]], np.array([[0, 1, 2 ** 32 + 1]], dtype=np.int64)):
        with pytest.raises(ValueError, match='outside'):
            meshtopo.orient_faces(wrong, V, device=dev)
    with pytest.raises(ValueError, match='states'):
        meshtopo.orient_faces(strip, V, state=[1, 1], device=dev)


def test_mesh_report(dev):
    from geobi_gnn_amd import meshtopo
    points, faces = T.sphere(2)
    r = meshtopo.mesh_report(points, faces, device=dev)
    assert r == T.report(points, faces)
    assert r['closed'] and r['euler'] == 2 and r['components'] == 1 and r['edges'] == 120 and r['vertices_used'] == 42
    r = meshtopo.mesh_report(points, faces[1:], device=dev)
    assert r == T.report(points, faces[1:])
    assert not r['closed'] and r['boundary_edges'] == 3 and r['euler'] == 1 and r['faces'] == 79
    r = meshtopo.mesh_report(_pts(5), T.moebius(5), device=dev)
    assert r == T.report(_pts(5), T.moebius(5))
    assert r['nonorientable'] == 1 and r['would_flip'] == 0 and r['inconsistent_edges'] == 5 and not r['closed']
    # a soup welds back to the sphere; without the weld it is 80 parts; a messy mesh: every count against the model
    sp, sf = M.soup(points, faces)
    assert meshtopo.mesh_report(sp, sf, device=dev) == dict(T.report(points, faces))
    r = meshtopo.mesh_report(sp, sf, weld_tol=None, device=dev)
    assert r['components'] == 80 and r['boundary_edges'] == 240 and r['vertices_used'] == 240
    for k, (p, f) in enumerate(T.report_fuzz()):
        assert meshtopo.mesh_report(p, f, device=dev) == T.report(p, f), k
    mixed = T.size_cases()['sphere2'][1]
    r = meshtopo.mesh_report(points, mixed, device=dev)
    assert r['would_flip'] == _model('sphere2', mixed)[0].counts['flipped'] and r['inconsistent_edges'] > 0 and r['closed']
    empty = meshtopo.mesh_report(np.zeros((0, 3)), np.zeros((0, 3)), device=dev)
    assert empty['faces'] == 0 and empty['euler'] == 0 and empty['closed']


# ------------------------------------------------------------------------------------------------ commands
def test_topology_commands(dev, tmp_path):
    from geobi_gnn_amd import meshio
    points, table, debris = T.command_ball()
    data = str(tmp_path / 'scan')
    os.makedirs(data)
    meshio.write_obj(os.path.join(data, 'ball.obj'), points, table)
    meshio.write_obj(os.path.join(data, 'tri.obj'), debris, np.array([[0, 1, 2]], dtype=np.int32))
    # without the flags: today's line, and the faces the half-edge rule costs
    run = _run(['clean', '--data_dir', data, '--out_dir', str(tmp_path / 'plain')])
    assert run.returncode == 0, run.stderr[-2000:]
    today = M.clean(points, table)
    assert today.counts['nonmanifold'] > 0
    line = ("V:     165 -> %7d,  F:     321 -> %7d,  welded: 0,  degenerate: 0,  nonmanifold: %d,  unreferenced: %d,  rounds: %d,  "
            "'ball.obj'\n" % (today.points.shape[0], today.faces.shape[0], today.counts['nonmanifold'],
                              today.counts['unreferenced'], today.counts['rounds']))
    assert line in run.stdout and 'flipped' not in run.stdout
    # with them: nothing lost but the debris; tri.obj has no faces left and is reported
    run = _run(['clean', '--data_dir', data, '--orient', '--min_component', '2'])
    assert run.returncode == 1 and run.stderr.count('skipped:') == 1 and 'no faces left' in run.stderr and 'tri.obj' in run.stderr
    m = T.clean(points, table, orient_faces=True, min_component=2)
    assert m.faces.shape[0] == 320 and m.points.shape[0] == 162
    assert ("V:     165 ->     162,  F:     321 ->     320,  welded: 0,  degenerate: 0,  nonmanifold: 0,  unreferenced: 3,  rounds: 1,  "
            "'ball.obj',  flipped: %d,  nonorientable: 0,  components: 2,  small: 1\n" % m.topology['flipped']) in run.stdout
    out_p, out_f = meshio.read_obj(os.path.join(data, 'clean', 'ball.obj'))
    assert np.array_equal(_bits(out_p), _bits(m.points)) and np.array_equal(out_f, m.faces)
    assert not os.path.exists(os.path.join(data, 'clean', 'tri.obj'))
    # denoise --clean --orient: the file's own faces and numbering; the debris keeps its bits
    one = str(tmp_path / 'one')
    os.makedirs(one)
    meshio.write_obj(os.path.join(one, 'ball.obj'), points, table)
    run = _run(['denoise', '--method', 'bnf', '--data_dir', one, '--clean', '--orient', '--min_component', '2'])
    assert run.returncode == 0, run.stderr[-2000:]
    got, got_faces = meshio.read_obj(os.path.join(one, 'result', 'ball-20.obj'))
    assert got.shape == points.shape and np.array_equal(got_faces, table)
    assert np.array_equal(_bits(got[162:]), _bits(debris)) and not np.array_equal(got[:162], points[:162])
    assert 'faces:    320' in run.stdout
    # info
    run = _run(['info', '--data_dir', data])
    assert run.returncode == 0, run.stderr[-2000:]
    rep = T.report(points, table)
    assert rep['components'] == 2 and rep['orient_components'] == 2 and rep['would_flip'] == m.topology['flipped']
    from geobi_gnn_amd.__main__ import INFO_KEYS
    assert ("V:     165,  F:     321,  %s,  closed: no,  'ball.obj'\n"
            % ',  '.join('%s: %d' % (k, rep[k]) for k in INFO_KEYS)) in run.stdout
    assert "boundary_edges: 3," in run.stdout and "'tri.obj'" in run.stdout
