"""The fp64 ICP model (tests/icp_model.py) anchored on the CPU, and the conditions under which tests/test_gpu_icp.py may
compare the device against it, established for the inputs that file uses.  Also the `align` command's parser and pairing.

Numbers this file re-establishes for the committed builders (printed by the tests):
  loop inputs (n, pose, scale)             iterations   outcome
  4,  10 deg, T 0.05, 1                    5            true pose recovered
  8,   5 deg, T 0.02, 1.2 (scale on)       5            true pose recovered
  8,  10 deg, T 0.05, 1                    11           another local minimum
  16,  5 deg, T 0.02, 1                    9            another local minimum
smallest nearest-gap 3.3e-5, smallest singular-value gap 1.58, every relative change >= 2.6e-5 except the last of each run,
which is exactly 0 because idx repeats."""
import numpy as np
import pytest

import icp_model as M

THR = 1e-6


# ------------------------------------------------------------------------------------------------ (a) Umeyama
def _exact_pairs(mirror=False, scale=1.7):
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, (40, 3)) * np.array([1.0, 0.6, 0.3])
    R = M.rotation((1, -2, 0.5), 37.0)
    if mirror:
        R = np.diag([1.0, 1.0, -1.0]) @ R
    T = np.array([0.3, -0.2, 0.9])
    return x, scale * x @ R + T, R, T, scale


def test_umeyama_returns_a_known_similarity():
    x, y, R, T, s = _exact_pairs()
    Rm, Tm, sm, rmse, gap, _ = M.umeyama(x, y, estimate_scale=True)
    assert np.abs(Rm - R).max() <= 1e-12 and np.abs(Tm - T).max() <= 1e-12 and abs(sm - s) <= 1e-12 and rmse <= 1e-12
    assert gap >= 1e-2
    x, y, R, T, _ = _exact_pairs(scale=1.0)
    Rm, Tm, sm, rmse, _, _ = M.umeyama(x, y)
    assert np.abs(Rm - R).max() <= 1e-12 and np.abs(Tm - T).max() <= 1e-12 and sm == 1.0 and rmse <= 1e-12
    assert np.allclose(M.transform(x, Rm, Tm, sm), y, atol=1e-12)
    assert abs(M.rotation_angle(R) - 37.0) <= 1e-9


def test_umeyama_on_a_mirrored_set_with_and_without_reflection():
    x, y, R, T, s = _exact_pairs(mirror=True)
    assert np.linalg.det(R) < 0
    Rm, Tm, sm, rmse, _, _ = M.umeyama(x, y, estimate_scale=True, allow_reflection=True)
    assert np.abs(Rm - R).max() <= 1e-12 and np.abs(Tm - T).max() <= 1e-12 and abs(sm - s) <= 1e-12 and rmse <= 1e-12
    Rp, _, _, rmse_p, _, _ = M.umeyama(x, y, estimate_scale=True)
    assert abs(np.linalg.det(Rp) - 1) <= 1e-12 and np.abs(Rp.T @ Rp - np.eye(3)).max() <= 1e-12
    assert rmse_p > 0.05                                    # a proper rotation cannot undo the mirror


def test_umeyama_scale_of_a_set_without_extent_is_one():
    x = np.full((6, 3), 0.25)
    y = np.random.default_rng(0).uniform(-1, 1, (6, 3))
    _, _, s, _, _, _ = M.umeyama(x, y, estimate_scale=True)
    assert s == 1.0


# ------------------------------------------------------------------------------------------------ (b)-(e) the loop inputs
@pytest.mark.parametrize('k', range(len(M.LOOP_INPUTS)))
def test_loop_inputs_meet_the_conditions_the_gpu_tests_rely_on(k):
    x, y, R, T, s, est = M.loop_input(k)
    run = M.loop_model(k)
    trace = run['trace']
    nn_gap = min(float(t['nn_gap'].min()) for t in trace)
    sv_gap = min(t['gap'] for t in trace)
    rels = [t['rel'] for t in trace[1:]]
    print('input %d: Q = %d, %d iterations, converged %s, rmse %.3g, smallest nearest-gap %.3g, smallest singular-value gap '
          '%.3g, relative changes %s' % (k, len(x), run['iterations'], run['converged'], run['rmse'], nn_gap, sv_gap,
                                         ' '.join('%.3g' % r for r in rels)))
    assert run['converged'] and run['iterations'] == (5, 5, 11, 9)[k]
    assert nn_gap >= 1e-5                                                                       # (b)
    for t in trace[1:]:                                                                         # (c)
        assert t['rel'] >= 2 * THR or (t['same_idx'] and t['rel'] == 0.0)
    assert all(not t['same_idx'] for t in trace[:-1]) and trace[-1]['same_idx']
    assert sv_gap >= 1e-2                                                                       # (d)
    err_R = np.abs(run['R'] - R).max()
    print('  |R - R_true| %.3g, |T - T_true| %.3g, s %.9g (true %.9g)' % (err_R, np.abs(run['T'] - T).max(), run['s'], s))
    if M.LOOP_INPUTS[k][5]:                                                                     # (e)
        assert err_R <= 1e-6 and np.abs(run['T'] - T).max() <= 1e-6 and abs(run['s'] - s) <= 1e-6
    else:
        assert err_R > 1e-2                                 # a model-comparison case, not a recovery case


def test_max_iterations_cuts_the_eleven_iteration_input():
    x, y, _, _, _, _ = M.loop_input(2)
    run = M.icp(x, y, max_iterations=2)
    assert run['iterations'] == 2 and not run['converged']
    assert np.array_equal(run['trace'][1]['idx'], M.loop_model(2)['trace'][1]['idx'])


def test_injected_inputs_are_well_conditioned():
    """The random-idx inputs of the GPU test: R is compared only where the singular-value gap is >= 1e-2, which the sizes
    with more than 3 rows reach."""
    for Q, M_, seed, offset in ((255, None, 1, 0.0), (256, None, 2, 0.0), (257, None, 3, 0.0), (5000, 4000, 4, 0.0),
                                (262145, None, 7, 0.0), (42, 50, 5, 0.0), (700, 700, 6, 1000.0)):
        x, y, idx = M.injected(Q, M_, seed, offset)
        for est in (False, True):
            st = M.step(x, y, idx, est)
            assert st['gap'] >= 1e-2, (Q, st['gap'])
        assert idx.min() >= 0 and idx.max() < len(y)


def test_small_part_inputs_of_the_launch_boundary_test_are_well_conditioned():
    for k in range(33):
        x, y, idx = M.injected(42, 50, 100 + k)
        assert M.step(x, y, idx, True)['gap'] >= 1e-2, k


def test_eval_and_command_inputs_take_one_path_on_both_sides():
    """The posed noisy icosphere of the eval_pair test and the two pairs of the command test: conditions (b) and (c), and
    the scaled pair comes back with s = 1 / 1.1."""
    from geobi_gnn_amd import meshgen
    noisy, clean, _ = meshgen.noisy_icosphere(8, 0.1, seed=3)
    (p8, _), (p6, _) = M.bumpy(8), M.bumpy(6)
    runs = {'eval_pair': M.icp(M.pose(noisy, degrees=5.0, translation=0.02)[0], clean.astype(np.float32)),
            'a_1': M.icp(M.pose(p8, degrees=4.0, translation=0.02)[0], p6, estimate_scale=True),
            'b': M.icp(M.pose(p6, degrees=3.0, translation=0.01, scale=1.1)[0], p6, estimate_scale=True)}
    for name, run in runs.items():
        nn_gap = min(float(t['nn_gap'].min()) for t in run['trace'])
        print('%s: %d iterations, converged %s, rmse %.3g, s %.6f, smallest nearest-gap %.3g, relative changes %s'
              % (name, run['iterations'], run['converged'], run['rmse'], run['s'], nn_gap,
                 ' '.join('%.3g' % t['rel'] for t in run['trace'][1:])))
        assert run['converged'] and run['iterations'] < 100 and nn_gap >= 1e-5
        assert all(t['rel'] >= 2 * THR or (t['same_idx'] and t['rel'] == 0.0) for t in run['trace'][1:])
    assert abs(runs['b']['s'] - 1 / 1.1) <= 1e-6


def test_bumpy_sphere_has_no_rotation_that_fits_it_twice():
    p, faces = M.bumpy(4)
    assert p.dtype == np.float32 and p.shape == (162, 3) and faces.shape == (320, 3)
    r = np.linalg.norm(p.astype(np.float64), axis=1)
    assert r.max() - r.min() > 0.3


# ------------------------------------------------------------------------------------------------ the command's parser
def _parse(argv):
    from geobi_gnn_amd.__main__ import parse_args
    return parse_args(argv)


def test_align_parser_accepts_what_the_command_documents():
    opt = _parse(['align', '--data_dir', 'a', '--target_dir', 'b'])
    assert (opt.out_dir, opt.scale, opt.reflect, opt.max_iter, opt.rmse_thr, opt.gpu) == ('', False, False, 100, 1e-6, -1)
    opt = _parse(['align', '--data_dir', 'a', '--target_dir', 'b', '--out_dir', 'c', '--scale', '--reflect', '--max_iter', '1',
                  '--rmse_thr', '0', '--gpu', '0'])
    assert (opt.out_dir, opt.scale, opt.reflect, opt.max_iter, opt.rmse_thr, opt.gpu) == ('c', True, True, 1, 0.0, 0)
    opt = _parse(['eval', '--result_dir', 'a', '--original_dir', 'b'])
    assert (opt.align, opt.scale, opt.free) == (False, False, False)
    opt = _parse(['eval', '--result_dir', 'a', '--original_dir', 'b', '--align', '--scale', '--free'])
    assert (opt.align, opt.scale, opt.free) == (True, True, True)
    assert _parse(['eval', '--result_dir', 'a', '--original_dir', 'b', '--free']).free


@pytest.mark.parametrize('argv, text', [
    (['eval', '--result_dir', 'a', '--original_dir', 'b', '--scale'], '--scale needs --align'),
    (['align', '--data_dir', 'a', '--target_dir', 'b', '--max_iter', '0'], '--max_iter'),
    (['align', '--data_dir', 'a', '--target_dir', 'b', '--rmse_thr', '-1e-3'], '--rmse_thr'),
    (['align', '--data_dir', 'a'], '--target_dir'),
])
def test_align_parser_rejects(argv, text, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(argv)
    assert e.value.code == 2 and text in capsys.readouterr().err


def test_align_list_pairs_as_pair_files_and_falls_back_to_the_same_name(tmp_path):
    from geobi_gnn_amd.__main__ import align_list
    src, dst = tmp_path / 'src', tmp_path / 'dst'
    src.mkdir()
    dst.mkdir()
    for name in ('a_1.obj', 'a_2.obj', 'a.obj', 'b.obj', 'c_x.txt'):
        (src / name).write_text('')
    for name in ('a.obj', 'b.obj', 'c.obj'):
        (dst / name).write_text('')
    jobs = [(s[len(str(src)) + 1:], t[len(str(dst)) + 1:]) for s, t in align_list(str(src), str(dst))]
    assert jobs == [('a_1.obj', 'a.obj'), ('a_2.obj', 'a.obj'), ('b.obj', 'b.obj')]


def test_icp_bindings_refuse_cpu_tensors():
    import torch
    from geobi_gnn_amd import _lib as L
    from geobi_gnn_amd import ops
    x = torch.zeros(4, 3)
    with pytest.raises(L.GeobiError, match='no CPU fallback'):
        ops.icp(x, x)
    with pytest.raises(L.GeobiError, match='no CPU fallback'):
        ops.icp_align(x, x)
    protos = L.parse_header()
    for name in ('geobi_icp_ws_bytes', 'geobi_icp_init', 'geobi_icp_apply', 'geobi_icp_step'):
        assert name in protos
