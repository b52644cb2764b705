"""Mesh cleaning on the host: the sequential model of tests/clean_model.py on hand cases, its `rounds` against a plain
simulation of the round-parallel form, meshclean.apply / scatter_back on numpy stand-ins, and the command line's new flags.
No device."""
import numpy as np
import pytest

import clean_model as M


def _pts(n, seed=0):
    """n distinct points"""
    rng = np.random.RandomState(seed)
    return (rng.rand(n, 3) + np.arange(n)[:, None]).astype(np.float32)


# ------------------------------------------------------------------------------------------------ hand cases
def test_chain_keeps_the_outer_two():
    # f0 has 0->1; f1 has 0->1 and 1->2; f2 has 1->2: f1 is dropped, owns nothing, so f2 is kept
    r = M.clean(_pts(5), [[0, 1, 3], [0, 1, 2], [1, 2, 4]])
    assert r.face_map.tolist() == [0, 2]
    assert r.counts == {'welded': 0, 'degenerate': 0, 'nonmanifold': 1, 'unreferenced': 0, 'rounds': 3}
    assert r.faces.tolist() == [[0, 1, 3], [1, 2, 4]] and r.vertex_map.tolist() == [0, 1, 2, 3, 4]


def test_same_orientation_duplicate_is_dropped():
    r = M.clean(_pts(3), [[0, 1, 2], [1, 2, 0]])
    assert r.face_map.tolist() == [0] and r.counts['nonmanifold'] == 1 and r.counts['rounds'] == 2


def test_opposite_orientation_pair_is_kept():
    r = M.clean(_pts(3), [[0, 1, 2], [0, 2, 1]])
    assert r.face_map.tolist() == [0, 1] and r.counts['nonmanifold'] == 0 and r.counts['rounds'] == 1


def test_manifold_off_keeps_duplicates():
    r = M.clean(_pts(3), [[0, 1, 2], [1, 2, 0], [0, 0, 1]], manifold=False)
    assert r.face_map.tolist() == [0, 1] and r.counts['degenerate'] == 1 and r.counts['rounds'] == 0


def test_degenerate_only_after_welding():
    p = _pts(4)
    p[3] = p[0]
    faces = [[0, 3, 1], [0, 1, 2]]
    r = M.clean(p, faces)
    assert r.canon.tolist() == [0, 1, 2, 0] and r.face_map.tolist() == [1]
    assert r.counts == {'welded': 1, 'degenerate': 1, 'nonmanifold': 0, 'unreferenced': 0, 'rounds': 1}
    assert r.vertex_map.tolist() == [0, 1, 2, 0]
    r = M.clean(p, faces, weld_tol=None)
    assert r.face_map.tolist() == [0, 1] and r.counts['welded'] == 0 and r.counts['degenerate'] == 0


def test_signed_zeros_weld():
    p = np.array([[0.0, 1.0, 2.0], [-0.0, 1.0, 2.0], [5.0, -0.0, 0.0], [5.0, 0.0, -0.0], [1.0, 1.0, 1.0]], dtype=np.float32)
    r = M.clean(p, [[0, 2, 4], [1, 3, 4]])
    assert r.canon.tolist() == [0, 0, 2, 2, 4] and r.counts['welded'] == 2
    assert r.face_map.tolist() == [0] and r.counts['nonmanifold'] == 1
    assert (r.points.view(np.uint32) == p[[0, 2, 4]].view(np.uint32)).all()         # the lowest member's own bits


def test_unreferenced_vertices_at_start_middle_end():
    r = M.clean(_pts(7), [[1, 2, 4], [2, 1, 5]])
    assert r.vertex_map.tolist() == [-1, 0, 1, -1, 2, 3, -1] and r.vertex_src.tolist() == [1, 2, 4, 5]
    assert r.faces.tolist() == [[0, 1, 2], [1, 0, 3]] and r.counts['unreferenced'] == 3


def test_a_face_only_some_of_whose_vertices_survive():
    # f1 repeats 0->1 and is dropped: its vertex 3 goes with it, 0 and 1 stay through f0
    r = M.clean(_pts(4), [[0, 1, 2], [0, 1, 3]])
    assert r.vertex_map.tolist() == [0, 1, 2, -1] and r.face_map.tolist() == [0]


def test_grid_weld_floors_negative_coordinates():
    p = np.array([[-0.125, 0.0, 0.0], [-0.5, 0.25, 0.375], [0.125, 0.0, 0.0], [0.375, 0.49, 0.0], [-0.625, 0, 0]], np.float32)
    assert M.weld_keys(p, 0.5).tolist() == [[-1, 0, 0], [-1, 0, 0], [0, 0, 0], [0, 0, 0], [-2, 0, 0]]
    assert M.clean(p, np.zeros((0, 3)), weld_tol=0.5).canon.tolist() == [0, 0, 2, 2, 4]
    with pytest.raises(ValueError):
        M.weld_keys(np.array([[3.0e9, 0, 0]], np.float32), 1.0)
    with pytest.raises(ValueError):
        M.weld_keys(np.array([[-1.0, 0, 0]], np.float32), 1.0e-10)


def test_soup_of_a_sphere_welds_back():
    from geobi_gnn_amd import meshgen
    pts, faces = meshgen.icosphere(2)
    sp, sf = M.soup(pts.astype(np.float32), faces)
    assert sp.shape == (240, 3)
    r = M.clean(sp, sf)
    assert r.points.shape[0] == 42 and r.faces.shape[0] == 80 and r.counts['welded'] == 198 and r.counts['rounds'] == 1
    # the welded soup is the sphere itself, up to the order its vertices are first met in
    assert (r.points[r.faces] == pts.astype(np.float32)[faces]).all()


def test_same_winding_strip_takes_one_round_per_face():
    r = M.clean(_pts(66), [[i, i + 1, i + 2] for i in range(64)])
    assert r.face_map.tolist() == list(range(0, 64, 2)) and r.counts['rounds'] == 64


# ------------------------------------------------------------------------------------------------ rounds
def _jacobi(faces_canon):
    """The round-parallel form on the host: every undecided face looks at the EARLIER claimants of its three half-edges
    in the previous round's state -- one kept: dropped; all dropped: kept; else undecided.  -> (kept mask, rounds)"""
    F = len(faces_canon)
    edges = [[(a, b), (b, c), (c, a)] for a, b, c in faces_canon]
    state = [3 if len({a, b, c}) < 3 else 0 for a, b, c in faces_canon]       # 0 undecided, 1 kept, 2 dropped, 3 degenerate
    claim = {}
    for f in range(F):
        if state[f] == 0:
            for e in edges[f]:
                claim.setdefault(e, []).append(f)
    rounds = 0
    while 0 in state:
        rounds += 1
        new = list(state)
        for f in range(F):
            if state[f] != 0:
                continue
            seen = [state[g] for e in edges[f] for g in claim[e] if g < f]
            new[f] = 2 if 1 in seen else (0 if 0 in seen else 1)
        state = new
    return [s == 1 for s in state], rounds


def test_model_rounds_are_the_round_parallel_forms():
    rng = np.random.RandomState(5)
    worst = 0
    for _ in range(400):
        V, F = rng.randint(3, 12), rng.randint(0, 40)
        faces = rng.randint(0, V, size=(F, 3))
        r = M.clean(_pts(V), faces)
        kept, rounds = _jacobi(faces.tolist())
        assert np.nonzero(kept)[0].tolist() == r.face_map.tolist()
        assert rounds == r.counts['rounds']
        worst = max(worst, rounds)
    assert worst >= 4                        # the sample does exercise chains


# ------------------------------------------------------------------------------------------------ apply / scatter_back
def test_apply_and_scatter_back_on_numpy():
    from geobi_gnn_amd import meshclean
    p = _pts(7)
    p[5] = p[1]
    m = M.clean(p, [[1, 2, 4], [2, 5, 6]])
    r = meshclean.CleanResult(m.points, m.faces, m.vertex_map, m.vertex_src, m.face_map, m.canon, m.counts)
    assert m.vertex_map.tolist() == [-1, 0, 1, -1, 2, 0, 3]
    other = _pts(7, seed=3)
    got = meshclean.apply(r, other)
    assert (got == other[[1, 2, 4, 6]]).all()
    assert (meshclean.apply(r, p) == m.points).all()
    moved = got + np.float32(10.0)
    back = meshclean.scatter_back(r, moved, other)
    assert (back[[1, 2, 4, 6]] == moved).all() and (back[5] == moved[0]).all()       # the welded duplicate shares it
    assert (back[[0, 3]].view(np.uint32) == other[[0, 3]].view(np.uint32)).all()     # untouched rows bit for bit
    assert back is not other and (other == _pts(7, seed=3)).all()
    with pytest.raises(ValueError):
        meshclean.apply(r, other[:6])
    with pytest.raises(ValueError):
        meshclean.scatter_back(r, moved[:3], other)


# ------------------------------------------------------------------------------------------------ command line
def _parse(argv):
    from geobi_gnn_amd.__main__ import parse_args
    return parse_args(argv)


def test_clean_command_parses():
    opt = _parse(['clean', '--data_dir', 'd'])
    assert opt.command == 'clean' and opt.out_dir == '' and opt.weld_tol == 0.0 and not opt.no_weld and not opt.no_manifold
    assert opt.gpu == -1 and callable(opt.fn)
    opt = _parse(['clean', '--data_dir', 'd', '--out_dir', 'o', '--weld_tol', '0.25', '--no_manifold', '--no_weld', '--gpu', '0'])
    assert (opt.out_dir, opt.weld_tol, opt.no_manifold, opt.no_weld, opt.gpu) == ('o', 0.25, True, True, 0)
    with pytest.raises(SystemExit):
        _parse(['clean', '--data_dir', 'd', '--weld_tol', '-1'])
    with pytest.raises(SystemExit):
        _parse(['clean', '--data_dir', 'd', '--weld_tol', 'nan'])


def test_denoise_clean_flags():
    opt = _parse(['denoise', '--data_dir', 'd', '--method', 'bnf', '--clean'])
    assert opt.clean and opt.weld_tol == 0.0 and not opt.no_weld and not opt.no_manifold
    opt = _parse(['denoise', '--data_dir', 'd', '--clean', '--weld_tol', '0.5', '--no_manifold'])
    assert opt.clean and opt.weld_tol == 0.5 and opt.no_manifold and opt.method == 'gnn'
    for extra in (['--weld_tol', '0'], ['--weld_tol', '0.5'], ['--no_weld'], ['--no_manifold']):
        with pytest.raises(SystemExit) as e:
            _parse(['denoise', '--data_dir', 'd'] + extra)
        assert e.value.code == 2


def test_denoise_defaults_are_unchanged():
    opt = vars(_parse(['denoise', '--data_dir', 'd']))
    fn = opt.pop('fn')
    assert fn.__name__ == 'denoise'
    assert not opt.pop('clean') and opt.pop('weld_tol') == 0.0 and not opt.pop('no_weld') and not opt.pop('no_manifold')
    assert opt == {'command': 'denoise', 'method': 'gnn', 'model': '', 'data_dir': 'd', 'out_dir': '', 'sub_size': 20000,
                   'n_iter': 60, 'normal_iters': 20, 'sigma_r': 0.35, 'sigma_s': 1.0, 'data_type': 'Synthetic', 'wei_param': 2,
                   'force_depth': False, 'pool_type': 'max', 'gpu': -1}
