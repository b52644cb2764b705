"""Mesh cleaning on the device (csrc/clean.hip, geobi_gnn_amd/meshclean.py) against the sequential model of
tests/clean_model.py, and the `clean` / `denoise --clean` commands end to end.

Every comparison is EXACT: integer arrays equal, points bit-equal, the counts (the number of Jacobi rounds included) equal.
There are no tolerances."""
import os

import numpy as np
import pytest
import torch

import clean_model as M
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


def _check(dev, points, faces, weld_tol=0.0, manifold=True, model=None):
    """clean_mesh against the model, everything exact -> (device result, model result)"""
    from geobi_gnn_amd import meshclean
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    r = meshclean.clean_mesh(points, faces, weld_tol=weld_tol, manifold=manifold, device=dev)
    m = M.clean(points, faces, weld_tol=weld_tol, manifold=manifold) if model is None else model
    assert r.counts == m.counts
    for name in ('canon', 'vertex_map', 'vertex_src', 'face_map', 'faces'):
        got = getattr(r, name)
        assert got.dtype == torch.int32 and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), getattr(m, name)), name
    assert r.points.dtype == torch.float32 and r.faces.shape == (m.faces.shape[0], 3)
    assert np.array_equal(_bits(r.points.cpu().numpy()), _bits(m.points))
    return r, m


def _sphere(n):
    from geobi_gnn_amd import meshgen
    pts, faces = meshgen.icosphere(n)
    return pts.astype(np.float32), faces.astype(np.int32)


_SOUPS = {}


def _sphere_soup(n):
    if n not in _SOUPS:
        sp, sf = M.soup(*_sphere(n))
        _SOUPS[n] = (sp, sf, M.clean(sp, sf))
    return _SOUPS[n]


# ------------------------------------------------------------------------------------------------ against the model
def test_clean_sphere_is_left_alone(dev):
    pts, faces = _sphere(2)
    r, _ = _check(dev, pts, faces)
    assert r.counts == {'welded': 0, 'degenerate': 0, 'nonmanifold': 0, 'unreferenced': 0, 'rounds': 1}
    assert r.vertex_map.tolist() == list(range(42)) and r.face_map.tolist() == list(range(80))
    assert r.canon.tolist() == list(range(42)) and np.array_equal(r.faces.cpu().numpy(), faces)


@pytest.mark.parametrize('n', [2, 32, 67])       # V + 1 on the one-block, the look-back and (above 2^18) the rocPRIM scan
def test_sphere_soup_welds_back(dev, n):
    sp, sf, model = _sphere_soup(n)
    r, _ = _check(dev, sp, sf, model=model)
    assert r.points.shape[0] == 10 * n * n + 2 and r.faces.shape[0] == 20 * n * n == sf.shape[0]
    assert r.counts['rounds'] == 1 and r.counts['welded'] == sp.shape[0] - (10 * n * n + 2)


HAND = {
    'chain': (5, [[0, 1, 3], [0, 1, 2], [1, 2, 4]], [0, 2]),
    'same_orientation': (3, [[0, 1, 2], [1, 2, 0]], [0]),
    'opposite_orientation': (3, [[0, 1, 2], [0, 2, 1]], [0, 1]),
    'unreferenced': (7, [[1, 2, 4], [2, 1, 5]], [0, 1]),
    'partly_surviving': (4, [[0, 1, 2], [0, 1, 3]], [0]),
    'clique': (42, [[0, 1, 2 + i] for i in range(40)], [0]),
    'no_faces': (3, [], []),
}


@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_cases(dev, name):
    V, faces, kept = HAND[name]
    r, m = _check(dev, _pts(V), faces)
    assert r.face_map.tolist() == kept
    if name == 'unreferenced':
        assert r.vertex_map.tolist() == [-1, 0, 1, -1, 2, 3, -1]
    if name == 'partly_surviving':
        assert r.vertex_map.tolist() == [0, 1, 2, -1]
    if name == 'clique':
        assert r.counts['nonmanifold'] == 39 and r.counts['rounds'] == 2


def test_weld_hand_cases(dev):
    p = _pts(4)
    p[3] = p[0]
    r, _ = _check(dev, p, [[0, 3, 1], [0, 1, 2]])                       # degenerate only after welding
    assert r.face_map.tolist() == [1] and r.counts['degenerate'] == 1 and r.counts['welded'] == 1
    r, _ = _check(dev, p, [[0, 3, 1], [0, 1, 2]], weld_tol=None)
    assert r.face_map.tolist() == [0, 1] and r.canon.tolist() == [0, 1, 2, 3]
    z = np.array([[0.0, 1.0, 2.0], [-0.0, 1.0, 2.0], [5.0, -0.0, 0.0], [5.0, 0.0, -0.0], [1.0, 1.0, 1.0]], dtype=np.float32)
    r, _ = _check(dev, z, [[0, 2, 4], [1, 3, 4]])
    assert r.canon.tolist() == [0, 0, 2, 2, 4] and r.face_map.tolist() == [0]
    assert np.array_equal(_bits(r.points.cpu().numpy()), _bits(z[[0, 2, 4]]))


def test_all_faces_dropped(dev):
    r, _ = _check(dev, _pts(4), [[0, 0, 1], [2, 3, 2], [1, 1, 1]])
    assert r.points.shape == (0, 3) and r.faces.shape == (0, 3) and r.vertex_map.tolist() == [-1] * 4
    assert r.counts == {'welded': 0, 'degenerate': 3, 'nonmanifold': 0, 'unreferenced': 4, 'rounds': 0}
    r, _ = _check(dev, np.zeros((0, 3)), np.zeros((0, 3)))
    assert r.points.shape == (0, 3) and r.canon.shape == (0,)


def test_strip_takes_one_round_per_face_and_max_rounds_is_an_error(dev):
    from geobi_gnn_amd import meshclean
    from geobi_gnn_amd._lib import GeobiError
    strip = [[i, i + 1, i + 2] for i in range(64)]
    r, _ = _check(dev, _pts(66), strip)
    assert r.face_map.tolist() == list(range(0, 64, 2)) and r.counts['rounds'] == 64
    with pytest.raises(GeobiError, match='max_rounds'):
        meshclean.clean_mesh(_pts(66), strip, max_rounds=8, device=dev)
    r, _ = _check(dev, _pts(66), strip)                                  # the call after the error works
    assert r.counts['rounds'] == 64
    assert meshclean.clean_mesh(_pts(66), strip, max_rounds=64, device=dev).counts['rounds'] == 64
    with pytest.raises(GeobiError, match='max_rounds'):
        meshclean.clean_mesh(_pts(66), strip, max_rounds=63, device=dev)


@pytest.mark.parametrize('n_vertices', [255, 256, 257, 511, 513])
def test_soups_across_the_workgroup_edges(dev, n_vertices):
    # a sphere's face list cut to n // 3 faces as a soup; the 0..2 vertices left over repeat the first ones and weld to them
    pts, faces = _sphere(4)
    sp, sf = M.soup(pts, faces[:n_vertices // 3])
    sp = np.concatenate([sp, sp[:n_vertices - sp.shape[0]]])
    assert sp.shape[0] == n_vertices
    r, _ = _check(dev, sp, sf)
    assert r.faces.shape[0] == n_vertices // 3 and r.counts['unreferenced'] == 0


def test_manifold_off(dev):
    p, faces = _pts(5), [[0, 1, 3], [0, 1, 2], [1, 2, 4], [0, 1, 3], [2, 2, 4]]
    r, _ = _check(dev, p, faces, manifold=False)
    assert r.face_map.tolist() == [0, 1, 2, 3] and r.counts['rounds'] == 0 and r.counts['degenerate'] == 1
    sp, sf, _ = _sphere_soup(2)
    _check(dev, sp, sf, weld_tol=None)
    _check(dev, sp, sf, weld_tol=None, manifold=False)


def test_grid_weld_on_exact_quotients(dev):
    # multiples of 1/8 divided by 0.5: every quotient is exact, so floor against truncation is all that can differ
    rng = np.random.RandomState(11)
    p = (rng.randint(-24, 25, size=(600, 3)) / 8.0).astype(np.float32)
    faces = rng.randint(0, 600, size=(900, 3))
    r, m = _check(dev, p, faces, weld_tol=0.5)
    assert m.counts['welded'] > 0 and (p < 0).any()
    keys = np.floor(p.astype(np.float64) / 0.5).astype(np.int64)
    assert np.array_equal(keys[r.canon.cpu().numpy()], keys)
    assert (np.trunc(p / 0.5) != np.floor(p / 0.5)).any()
    _check(dev, p, faces, weld_tol=0.125)


def test_errors(dev):
    from geobi_gnn_amd import _lib as L, meshclean
    p, faces = _pts(4), [[0, 1, 2], [1, 2, 3]]
    big = p.copy()
    big[2, 1] = 3.0e9
    with pytest.raises(L.GeobiError, match='int32'):
        meshclean.clean_mesh(big, faces, weld_tol=1.0, device=dev)
    with pytest.raises(L.GeobiError, match='int32'):
        meshclean.clean_mesh(-p, faces, weld_tol=1.0e-10, device=dev)
    _check(dev, big, faces)                                            # the same points weld exactly without a word
    bad = p.copy()
    bad[1, 0] = np.inf
    with pytest.raises(ValueError, match='finite'):
        meshclean.clean_mesh(bad, faces, device=dev)
    bad[1, 0] = np.nan
    with pytest.raises(ValueError, match='finite'):
        meshclean.clean_mesh(bad, faces, device=dev)
    for wrong in ([[0, 1, 4]], [[0, -1, 2]], np.array([[0, 1, 2 ** 32 + 1]], dtype=np.int64)):
        with pytest.raises(ValueError, match='outside'):
            meshclean.clean_mesh(p, wrong, device=dev)
    with pytest.raises(ValueError, match='weld_tol'):
        meshclean.clean_mesh(p, faces, weld_tol=-0.5, device=dev)
    with pytest.raises(ValueError, match='max_rounds'):
        meshclean.clean_mesh(p, faces, max_rounds=0, device=dev)
    # the size limit is checked at entry, before any pointer is used
    t = torch.zeros(16, dtype=torch.int32, device=dev)
    too_many = (1 << 24)
    assert L.lib().geobi_clean_weld_ws_bytes(too_many) == 0
    with pytest.raises(L.GeobiError, match='GEOBI_MAX_NODES'):
        L.call('geobi_clean_weld', L.ptr(t), too_many, 1, 0.0, L.ptr(t), L.ptr(t), L.ptr(t), 64, L.stream())
    with pytest.raises(L.GeobiError, match='GEOBI_MAX_NODES'):
        L.call('geobi_clean_compact', L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), 4, too_many, L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t),
               L.ptr(t), L.ptr(t), L.ptr(t), 64, L.stream())


def test_fuzz_against_the_model(dev):
    rng = np.random.RandomState(2024)
    values = np.array([0.0, 0.75, -1.5], dtype=np.float32)
    seen_rounds, dropped = 0, 0
    for k in range(300):
        V, F = rng.randint(1, 41), rng.randint(0, 81)
        p = values[rng.randint(0, 3, size=(V, 3))]
        if k % 3 == 0:
            p = p + (np.arange(V) // 3)[:, None].astype(np.float32) * 4.0          # fewer welds: longer chains survive
        faces = rng.randint(0, V, size=(F, 3))
        r, m = _check(dev, p, faces, weld_tol=(0.0, 1.0)[k % 2], manifold=k % 7 != 6)
        seen_rounds = max(seen_rounds, m.counts['rounds'])
        dropped += m.counts['nonmanifold']
    assert seen_rounds >= 3 and dropped > 100        # the sample does reach conflicts and chains


def test_two_calls_are_bit_identical(dev):
    from geobi_gnn_amd import meshclean
    sp, sf, _ = _sphere_soup(32)
    sf = np.concatenate([sf, sf[::7], sf[::5, ::-1]])              # copies, and flipped copies: their half-edges are the neighbours'
    a = meshclean.clean_mesh(sp, sf, device=dev)
    b = meshclean.clean_mesh(sp, sf, device=dev)
    assert a.counts == b.counts and a.counts['nonmanifold'] == 2926 + 4096
    for name in ('points', 'faces', 'vertex_map', 'vertex_src', 'face_map', 'canon'):
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name


def test_round_trip(dev):
    from geobi_gnn_amd import meshclean
    sp, sf, _ = _sphere_soup(2)
    sp = np.concatenate([_pts(2, seed=4) + 50.0, sp, _pts(1, seed=5) - 50.0])            # loose vertices at both ends
    sf = sf + 2
    r, m = _check(dev, sp, sf)
    assert r.counts['unreferenced'] == 3
    other = torch.from_numpy(_pts(sp.shape[0], seed=9)).to(dev)
    picked = meshclean.apply(r, other)
    assert torch.equal(picked, other[r.vertex_src.long()])
    back = meshclean.scatter_back(r, picked, other)
    assert torch.equal(back, other[r.canon.long()])            # every member holds its canonical vertex's position
    moved = picked + 1.0
    back = meshclean.scatter_back(r, moved, other)
    vm = r.vertex_map.long()
    assert torch.equal(back[vm >= 0], moved[vm[vm >= 0]])
    assert torch.equal(back[vm < 0].view(torch.int32), other[vm < 0].view(torch.int32)) and int((vm < 0).sum()) == 3
    assert torch.equal(meshclean.apply(r, torch.from_numpy(sp).to(dev)).view(torch.int32), r.points.view(torch.int32))


# ------------------------------------------------------------------------------------------------ commands
def test_denoise_clean_and_clean_commands(dev, tmp_path):
    from geobi_gnn_amd import meshgen, meshio
    noisy, clean, faces = meshgen.noisy_icosphere(4, 0.2, seed=3)
    sp, sf = M.soup(np.asarray(noisy, dtype=np.float32), np.asarray(faces))
    loose = np.array([[7.0, -8.0, 9.5]], dtype=np.float32)
    sp = np.concatenate([sp[:100], loose, sp[100:]])                 # one vertex no face lists, in the middle
    sf = np.where(sf >= 100, sf + 1, sf).astype(np.int32)
    data = str(tmp_path / 'soup')
    os.makedirs(data)
    meshio.write_obj(os.path.join(data, 'ball.obj'), sp, sf)
    # today's behaviour, pinned: the file is refused for its loose vertex
    run = _run(['denoise', '--method', 'bnf', '--data_dir', data])
    assert run.returncode == 1 and 'skipped:' in run.stderr and 'referenced by no face' in run.stderr
    assert os.listdir(os.path.join(data, 'result')) == []
    run = _run(['denoise', '--method', 'bnf', '--data_dir', data, '--clean'])
    assert run.returncode == 0, run.stderr[-2000:]
    got, got_faces = meshio.read_obj(os.path.join(data, 'result', 'ball-20.obj'))
    assert got.shape == sp.shape and np.array_equal(got_faces, sf)             # the input's numbering and faces
    assert np.array_equal(_bits(got[100]), _bits(loose[0]))                     # the loose vertex did not move
    m = M.clean(sp, sf)
    assert m.points.shape[0] == 162 and m.faces.shape[0] == 320 and m.counts['unreferenced'] == 1
    assert np.array_equal(_bits(got), _bits(got[m.canon]))                      # a weld group shares one position
    used = m.vertex_map >= 0
    assert not np.array_equal(got[used], sp[used])                              # and the filter did move the mesh
    assert 'faces:    320' in run.stdout
    # clean: original/ + noisy/ -> the same layout, the noisy file through the ORIGINAL's maps
    pair = str(tmp_path / 'pair')
    os.makedirs(os.path.join(pair, 'original'))
    os.makedirs(os.path.join(pair, 'noisy'))
    osp, _ = M.soup(np.asarray(clean, dtype=np.float32), np.asarray(faces))
    osp = np.concatenate([osp[:100], loose, osp[100:]])
    rng = np.random.RandomState(8)
    nsp = (osp + rng.normal(0, 0.01, size=osp.shape)).astype(np.float32)        # duplicates carry independent noise
    meshio.write_obj(os.path.join(pair, 'original', 'ball.obj'), osp, sf)
    meshio.write_obj(os.path.join(pair, 'noisy', 'ball_n1.obj'), nsp, sf)
    meshio.write_obj(os.path.join(pair, 'noisy', 'ball_n2.obj'), nsp[:-3], sf[:-1])      # another size: skipped
    run = _run(['clean', '--data_dir', pair])
    assert run.returncode == 1 and run.stderr.count('skipped:') == 1 and 'ball_n2.obj' in run.stderr
    mo = M.clean(osp, sf)
    out_p, out_f = meshio.read_obj(os.path.join(pair, 'clean', 'original', 'ball.obj'))
    assert np.array_equal(_bits(out_p), _bits(mo.points)) and np.array_equal(out_f, mo.faces)
    out_p, out_f = meshio.read_obj(os.path.join(pair, 'clean', 'noisy', 'ball_n1.obj'))
    assert np.array_equal(_bits(out_p), _bits(nsp[mo.vertex_src])) and np.array_equal(out_f, mo.faces)
    assert M.clean(nsp, sf).points.shape[0] > mo.points.shape[0]                # welding the noisy file itself would not do
    assert sorted(os.listdir(os.path.join(pair, 'clean', 'noisy'))) == ['ball_n1.obj']
    assert 'V:     961 ->     162,  F:     320 ->     320,  welded: 798,  degenerate: 0,  nonmanifold: 0,  unreferenced: 1,' \
        in run.stdout
