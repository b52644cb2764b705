"""Rigid ICP on the MI355X (geobi_icp_*, ops.icp / icp_align, mesheval.align / eval_free, the `align` command) against
the fp64 model of tests/icp_model.py.  tests/test_icp_model_host.py establishes, on the CPU, the conditions these
comparisons rest on for the same inputs: every nearest-gap >= 1e-5, every relative change of the rmse >= 2x the threshold
or exactly 0 because idx repeats, every singular-value gap >= 1e-2 where R is compared.

Tolerances (for a singular-value gap >= 1e-2): R abs 1e-9, T and rmse abs 1e-9 max|y|, s rel 1e-9 -- the fp64 sums and the
Jacobi SVD give about 1e-13, over a gap of 1e-2 that bounds the rotation error near 1e-11, and 1e-9 leaves two decades --
and xt within 2 float32 ulps of max|y| of the model's.  Every test prints what it measured before it asserts."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import icp_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5                      # the project's bar (tests/test_gpu_kernels.py)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


def _t(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


def _ulps(y):
    return 2 * float(np.spacing(np.float32(np.abs(y).max())))


def _one_step(dev, x, y, idx, xptr=None, yptr=None, **kw):
    """geobi_icp_step on a fresh state -> (state [P, 24] float64, xt float32) on the host."""
    from geobi_gnn_amd import ops
    P = 1 if xptr is None else len(xptr) - 1
    xd, yd = _t(x, dev), _t(y, dev)
    state = ops.icp_init(P, dev)
    xt = torch.full_like(xd, float('nan'))
    ops.icp_step(xd, yd, _t(idx, dev, torch.int32), state, xt, xptr, yptr, **kw)
    return state.cpu().numpy(), xt.cpu().numpy()


def _compare(st, xt, x, y, idx, what, est=False, compare_R=None, **kw):
    """One part's state and xt against the model's step.  rmse and s always; R, T and xt where the gap is >= 1e-2."""
    ref = M.step(x, y, idx, estimate_scale=est, **kw)
    ymax = float(np.abs(y).max())
    R = st[:9].reshape(3, 3)
    err = {'R': np.abs(R - ref['R']).max(), 'T': np.abs(st[9:12] - ref['T']).max() / ymax,
           's': abs(st[12] - ref['s']) / ref['s'], 'rmse': abs(st[13] - ref['rmse']) / ymax,
           'xt': np.abs(xt.astype(np.float64) - ref['xt'].astype(np.float64)).max() / _ulps(y) * 2}
    print('%s: gap %.3g, errors R %.2e, T %.2e max|y|, s %.2e, rmse %.2e max|y|, xt %.2f ulp, orth %.2e'
          % (what, ref['gap'], err['R'], err['T'], err['s'], err['rmse'], err['xt'], np.abs(R.T @ R - np.eye(3)).max()))
    assert err['rmse'] <= 1e-9 and err['s'] <= 1e-9, what
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - (1 if not kw.get('allow_reflection') else
                                                                                 np.sign(np.linalg.det(R)))) <= 1e-12
    if ref['gap'] >= 1e-2 if compare_R is None else compare_R:
        assert err['R'] <= 1e-9 and err['T'] <= 1e-9 and err['xt'] <= 2.0, what
    assert st[15] == 1.0 and st[14] == 0.0 and st[16] == (1.0 if st[13] == 0.0 else 0.0)
    assert abs(st[17] - ref['sratio']) <= 1e-9
    return ref


# ------------------------------------------------------------------------------------------------ 1. one step, injected idx
@pytest.mark.parametrize('Q, M_, seed, offset', [(1, 5, 11, 0.0), (2, 5, 12, 0.0), (3, 5, 13, 0.0), (255, None, 1, 0.0),
                                                 (256, None, 2, 0.0), (257, None, 3, 0.0), (5000, 4000, 4, 0.0),
                                                 (262145, None, 7, 0.0), (700, 700, 6, 1000.0)])
def test_step_with_injected_idx_matches_the_model(dev, Q, M_, seed, offset):
    """One part; idx is random, not searched.  255 / 256 / 257 rows: the block edge; 5 000: several blocks; 262 145: the
    grid-stride walk wraps (64 blocks x 256 threads x 16 + 1); offset 1000 with extent 1: the pivot."""
    x, y, idx = M.injected(Q, M_, seed, offset)
    for est in (False, True):
        st, xt = _one_step(dev, x, y, idx, estimate_scale=est)
        _compare(st[0], xt, x, y, idx, 'Q = %d, offset %g, scale %s' % (Q, offset, est), est=est)
    st_r, xt_r = _one_step(dev, x, y, idx, allow_reflection=True)
    # three points span a plane at most: with reflections allowed its mirror image fits as well, R is not compared
    _compare(st_r[0], xt_r, x, y, idx, 'Q = %d, reflections allowed' % Q, compare_R=None if Q > 3 else False,
             allow_reflection=True)
    again, xt_again = _one_step(dev, x, y, idx, estimate_scale=True)
    assert np.array_equal(again, st) and np.array_equal(xt_again, xt)                     # two runs, bit for bit


@pytest.mark.parametrize('P', [2, 32, 33])
def test_step_over_the_launch_boundary(dev, P):
    """P parts of 42 rows against 50 targets each (32 parts ride in one launch): every part against the model."""
    parts = [M.injected(42, 50, 100 + k) for k in range(P)]
    xptr, yptr = [42 * k for k in range(P + 1)], [50 * k for k in range(P + 1)]
    x, y = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    idx = np.concatenate([p[2] + 50 * k for k, p in enumerate(parts)]).astype(np.int32)
    st, xt = _one_step(dev, x, y, idx, xptr, yptr, estimate_scale=True)
    for k, (xk, yk, ik) in enumerate(parts):
        _compare(st[k], xt[42 * k:42 * k + 42], xk, yk, ik, 'part %d of %d' % (k, P), est=True)


def test_step_clamps_a_foreign_idx_into_the_part(dev):
    """Indices outside the part's rows of y are clamped before the gather: the result is the clamped array's."""
    x, y, idx = M.injected(300, 200, 21)
    xptr, yptr = [0, 100, 300], [0, 80, 200]
    idx = np.concatenate([np.clip(idx[:100], 0, 79), np.clip(idx[100:], 80, 199)]).astype(np.int32)
    wild = idx.copy()
    wild[5], wild[50], wild[150], wild[250] = -7, 10 ** 9, 3, 10 ** 6       # below, above, the other part, beyond y
    clamped = wild.copy()
    clamped[:100] = np.clip(wild[:100], 0, 79)
    clamped[100:] = np.clip(wild[100:], 80, 199)
    st_w, xt_w = _one_step(dev, x, y, wild, xptr, yptr)
    st_c, xt_c = _one_step(dev, x, y, clamped, xptr, yptr)
    assert np.array_equal(st_w, st_c) and np.array_equal(xt_w, xt_c) and np.isfinite(st_w).all()


# ------------------------------------------------------------------------------------------------ 2. degenerate parts
def test_degenerate_parts(dev):
    rng = np.random.default_rng(5)
    y5 = rng.uniform(-1, 1, (5, 3)).astype(np.float32)
    # one point: R = I, rmse = 0, converged at iteration 1
    x1 = np.array([[0.3, -0.2, 0.9]], np.float32)
    st, xt = _one_step(dev, x1, y5, np.array([3]))
    assert np.array_equal(st[0, :9].reshape(3, 3), np.eye(3)) and st[0, 13] == 0.0 and st[0, 15] == 1.0 and st[0, 16] == 1.0
    assert np.array_equal(xt[0], y5[3]) and st[0, 12] == 1.0
    # collinear and coincident sets: only rmse, det R and orthonormality
    t = np.linspace(0, 1, 7)[:, None]
    line_x = (t * np.array([1.0, 2.0, 3.0])).astype(np.float32)
    line_y = (t * np.array([3.0, -1.0, 2.0]) + 0.01 * rng.standard_normal((7, 3))).astype(np.float32)
    same = np.full((7, 3), 0.25, np.float32)
    for what, x, y, est in (('collinear', line_x, line_y, False), ('collinear, scale', line_x, line_y, True),
                            ('coincident x', same, line_y, False), ('coincident y', line_x, same, False),
                            ('both coincident', same, same + 1, False)):
        st, xt = _one_step(dev, x, y, np.arange(7), estimate_scale=est)
        _compare(st[0], xt, x, y, np.arange(7), what, est=est, compare_R=False)
    # zero-extent x with estimate_scale: s = 1
    st, _ = _one_step(dev, same, line_y, np.arange(7), estimate_scale=True)
    assert st[0, 12] == 1.0
    # a planar 5 x 5 grid: rank 2, R still determined
    g = np.stack(np.meshgrid(np.arange(5.0), np.arange(5.0)), -1).reshape(-1, 2)
    grid = np.concatenate([g, np.zeros((25, 1))], 1).astype(np.float32)
    moved = (grid.astype(np.float64) @ M.rotation((1, 2, 3), 33.0) + 0.2).astype(np.float32)
    st, xt = _one_step(dev, grid, moved, np.arange(25))
    ref = _compare(st[0], xt, grid, moved, np.arange(25), 'planar grid', compare_R=True)
    assert ref['gap'] >= 1e-2 and ref['sratio'] <= 1e-7 and st[0, 13] <= 1e-6


# ------------------------------------------------------------------------------------------------ 3. the loop
def _assert_indices(got, ref, gap, what):
    keep = gap >= 1e-5
    left_out = int((~keep).sum())
    if left_out:
        print('%s: %d of %d rows left out (fp64 gap below 1e-5)' % (what, left_out, len(ref)))
    assert left_out <= 1e-3 * len(ref)
    assert np.array_equal(np.asarray(got)[keep], ref[keep]), what


_ALONE = {}


def _alone(dev, k):
    """ops.icp on loop input k alone (computed once, never changed)."""
    from geobi_gnn_amd import ops
    if k not in _ALONE:
        x, y, _, _, _, est = M.loop_input(k)
        _ALONE[k] = ops.icp(_t(x, dev), _t(y, dev), estimate_scale=est)
    return _ALONE[k]


@pytest.mark.parametrize('k', range(len(M.LOOP_INPUTS)))
def test_loop_matches_the_model(dev, k):
    """nearest_parts -> icp_step written out: idx of every iteration equals the model's on the rows with an fp64 gap >= 1e-5
    (at most 0.1 % may be left out), the same iterations and converged flag, the final state within the tolerances of the
    one-step test; ops.icp gives the written-out loop's bits; the recovery inputs reach the true pose to 1e-4."""
    from geobi_gnn_amd import ops
    x, y, R_true, T_true, s_true, est = M.loop_input(k)
    ref = M.loop_model(k)
    xd, yd = _t(x, dev), _t(y, dev)
    state = ops.icp_init(1, dev)
    xt = ops.icp_apply(xd, state)
    assert torch.equal(xt, xd)                                         # the identity leaves every bit alone
    for it, tr in enumerate(ref['trace'], 1):
        _, idx = ops.nearest_parts(xt, yd)
        _assert_indices(idx.cpu().numpy(), tr['idx'], tr['nn_gap'], 'input %d, iteration %d' % (k, it))
        ops.icp_step(xd, yd, idx, state, xt, estimate_scale=est)
        st = state.cpu().numpy()[0]
        assert st[15] == it and bool(st[16]) == (it == ref['iterations'] and ref['converged'])
        if tr['rel'] is not None:
            assert abs(st[14] - tr['rel']) <= 1e-6 * max(abs(tr['rel']), 1e-3) or (tr['rel'] == 0.0 and st[14] == 0.0)
    st = state.cpu().numpy()[0]
    R, ymax = st[:9].reshape(3, 3), float(np.abs(y).max())
    err_xt = np.abs(xt.cpu().numpy().astype(np.float64) - ref['xt']).max() / _ulps(y) * 2
    print('input %d: %d iterations, rmse %.9g (model %.9g), errors R %.2e, T %.2e, s %.2e, xt %.2f ulp; to the true pose R %.2e'
          % (k, st[15], st[13], ref['rmse'], np.abs(R - ref['R']).max(), np.abs(st[9:12] - ref['T']).max(),
             abs(st[12] - ref['s']), err_xt, np.abs(R - R_true).max()))
    assert np.abs(R - ref['R']).max() <= 1e-9 and np.abs(st[9:12] - ref['T']).max() <= 1e-9 * ymax
    assert abs(st[12] - ref['s']) <= 1e-9 * ref['s'] and abs(st[13] - ref['rmse']) <= 1e-9 * ymax and err_xt <= 2.0
    res = _alone(dev, k)
    assert torch.equal(res.xt, xt) and torch.equal(res.state, state)
    assert int(res.iterations[0]) == ref['iterations'] and bool(res.converged[0]) == ref['converged']
    assert res.R.shape == (1, 3, 3) and res.T.shape == (1, 3) and float(res.rmse[0]) == st[13] and float(res.s[0]) == st[12]
    if M.LOOP_INPUTS[k][5]:
        assert np.abs(R - R_true).max() <= 1e-4 and np.abs(st[9:12] - T_true).max() <= 1e-4 and abs(st[12] - s_true) <= 1e-4


# ------------------------------------------------------------------------------------------------ 4. / 5. union, freezing
UNION = (0, 2, 3)                 # loop inputs without scale: 5, 11 and 9 iterations


def _union_inputs(dev):
    xs, ys = [M.loop_input(k)[0] for k in UNION], [M.loop_input(k)[1] for k in UNION]
    xptr, yptr = np.cumsum([0] + [len(a) for a in xs]).tolist(), np.cumsum([0] + [len(a) for a in ys]).tolist()
    return _t(np.concatenate(xs), dev), _t(np.concatenate(ys), dev), xptr, yptr


def test_union_parts_equal_the_parts_alone_bit_for_bit(dev):
    from geobi_gnn_amd import ops
    xd, yd, xptr, yptr = _union_inputs(dev)
    res = ops.icp(xd, yd, xptr, yptr)
    print('union of inputs %s: iterations %s, converged %s' % (UNION, res.iterations.tolist(), res.converged.tolist()))
    assert res.iterations.tolist() == [M.loop_model(k)['iterations'] for k in UNION] and bool(res.converged.all())
    for p, k in enumerate(UNION):
        alone = _alone(dev, k)
        assert torch.equal(res.xt[xptr[p]:xptr[p + 1]], alone.xt), k
        assert torch.equal(res.state[p], alone.state[0]), k
        assert torch.equal(res.R[p], alone.R[0]) and torch.equal(res.T[p], alone.T[0])


def test_thirty_three_small_parts_equal_the_parts_alone(dev):
    """33 posed copies of the 42-vertex bumpy sphere (one launch carries 32 parts)."""
    from geobi_gnn_amd import ops
    y, _ = M.bumpy(2)
    assert len(y) == 42
    xs = [M.pose(y, axis=(1 + k % 3, 2, 3 - k % 5), degrees=2.0 + 0.4 * k, translation=0.01 + 0.001 * k)[0] for k in range(33)]
    ptr = [42 * k for k in range(34)]
    res = ops.icp(_t(np.concatenate(xs), dev), _t(np.tile(y, (33, 1)), dev), ptr, ptr, estimate_scale=True)
    print('33 parts: iterations %s' % res.iterations.tolist())
    assert len(set(res.iterations.tolist())) > 1
    yd = _t(y, dev)
    for k in range(33):
        alone = ops.icp(_t(xs[k], dev), yd, estimate_scale=True)
        assert torch.equal(res.xt[ptr[k]:ptr[k + 1]], alone.xt) and torch.equal(res.state[k], alone.state[0]), k


def test_check_every_does_not_change_a_bit_and_converged_parts_stay_frozen(dev):
    from geobi_gnn_amd import ops
    xd, yd, xptr, yptr = _union_inputs(dev)
    runs = [ops.icp(xd, yd, xptr, yptr, check_every=c) for c in (1, 4, 7)]
    for r in runs[1:]:
        assert torch.equal(r.xt, runs[0].xt) and torch.equal(r.state, runs[0].state)
    # the loop written out, three iterations beyond the last part's: part 0 (done at 5) and part 2 (done at 9) are not written
    iters = [M.loop_model(k)['iterations'] for k in UNION]
    state = ops.icp_init(3, dev)
    xt = ops.icp_apply(xd, state, xptr)
    frozen = {}
    for it in range(1, max(iters) + 4):
        _, idx = ops.nearest_parts(xt, yd, xptr, yptr)
        ops.icp_step(xd, yd, idx, state, xt, xptr, yptr)
        for p in range(3):
            if p in frozen:
                assert torch.equal(state[p], frozen[p][0]) and torch.equal(xt[xptr[p]:xptr[p + 1]], frozen[p][1]), (p, it)
            elif it == iters[p]:
                assert float(state[p, 16]) == 1.0
                frozen[p] = (state[p].clone(), xt[xptr[p]:xptr[p + 1]].clone())
            else:
                assert float(state[p, 16]) == 0.0 and float(state[p, 15]) == it
    assert sorted(frozen) == [0, 1, 2] and iters[0] < iters[2] < iters[1]
    assert torch.equal(state, runs[0].state) and torch.equal(xt, runs[0].xt)


# ------------------------------------------------------------------------------------------------ 6. max_iterations
def test_max_iterations_two_on_the_eleven_iteration_input(dev):
    from geobi_gnn_amd import ops
    x, y, _, _, _, _ = M.loop_input(2)
    for c in (1, 4):
        res = ops.icp(_t(x, dev), _t(y, dev), max_iterations=2, check_every=c)
        assert res.iterations.tolist() == [2] and res.converged.tolist() == [False]
    ref = M.icp(x, y, max_iterations=2)
    assert abs(float(res.rmse[0]) - ref['rmse']) <= 1e-9 * float(np.abs(y).max())


# ------------------------------------------------------------------------------------------------ 7. apply, gradient
def test_apply_reproduces_xt_and_the_gradient_is_the_transposed_linear_part(dev):
    from geobi_gnn_amd import network, ops
    k = 1                                                              # the input with a scale
    x, y, _, _, _, est = M.loop_input(k)
    ref, res = M.loop_model(k), _alone(dev, k)
    xd, yd = _t(x, dev), _t(y, dev)
    assert torch.equal(ops.icp_apply(xd, res.state, mode=0), res.xt)
    p = xd.clone().requires_grad_()
    out = ops.icp_align(p, yd, estimate_scale=est)
    assert torch.equal(out.detach(), res.xt)
    out.sum().backward()
    want = (ref['s'] * np.ones((1, 3)) @ ref['R'].T).astype(np.float32)           # s 1 R^T, the same for every row
    got = p.grad.cpu().numpy()
    print('gradient row %s (model %s)' % (got[0], want[0]))
    assert np.abs(got - want).max() <= _ulps(want)
    g = torch.from_numpy(np.random.default_rng(3).standard_normal(x.shape).astype(np.float32)).to(dev)
    back = ops.icp_apply(g, res.state, mode=1).cpu().numpy()
    want = ref['s'] * g.cpu().numpy().astype(np.float64) @ ref['R'].T
    assert np.abs(back - want).max() <= _ulps(want)
    # the composition the documents name: a Chamfer loss in the aligned frame
    q = xd.clone().requires_grad_()
    loss = network.loss_v(ops.icp_align(q, yd, estimate_scale=est), yd, 'CD')
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(q.grad).all())
    with pytest.raises(NotImplementedError):
        network.loss_v(xd, yd, 'CD', apply_icp=True)


# ------------------------------------------------------------------------------------------------ 8. eval_pair(align=True)
def _eval_input():
    from geobi_gnn_amd import meshgen
    noisy, clean, faces = meshgen.noisy_icosphere(8, 0.1, seed=3)
    posed, _, _ = M.pose(noisy, degrees=5.0, translation=0.02)
    return posed, clean.astype(np.float32), faces


def test_eval_pair_with_align_scores_the_aligned_points(dev):
    """A posed copy of a noisy icosphere (5 degrees, T 0.02; the model: 6 iterations, smallest nearest-gap 2.9e-4): every
    column within 1e-5 relative of eval_pair on the points the fp64 model aligned; without the flag, today's keys."""
    from geobi_gnn_amd import mesheval
    posed, clean, faces = _eval_input()
    ref = M.icp(posed, clean)
    assert min(float(t['nn_gap'].min()) for t in ref['trace']) >= 1e-5
    assert all(t['rel'] >= 2e-6 or (t['same_idx'] and t['rel'] == 0.0) for t in ref['trace'][1:])
    got = mesheval.eval_pair(posed, faces, clean, device=dev, align=True)
    want = mesheval.eval_pair(ref['xt'], faces, clean, device=dev)
    plain = mesheval.eval_pair(posed, faces, clean, device=dev)
    keys = ('num_f', 'err_face', 'angle', 'num_v', 'err_v', 'err_v_norm', 'surf', 'surf_norm', 'hausdorff', 'scale')
    assert tuple(want) == keys and tuple(plain) == keys
    assert set(got) == set(keys) | {'icp_rmse', 'icp_iterations', 'icp_converged'}
    for key in keys:
        print('%s: %.9g (model-aligned %.9g, not aligned %.9g)' % (key, got[key], want[key], plain[key]))
        assert abs(got[key] - want[key]) <= TOL * abs(want[key]), key
    assert got['icp_iterations'] == ref['iterations'] and got['icp_converged'] is True
    assert abs(got['icp_rmse'] - ref['rmse']) <= 1e-9
    assert plain['err_v'] > 1.5 * got['err_v']                          # the pose was the larger part of the error
    res = mesheval.align(posed, clean, device=dev)
    info = mesheval.align_info(res)
    assert abs(info['icp_angle'] - M.rotation_angle(ref['R'])) <= 1e-6 and abs(info['icp_shift'] - np.linalg.norm(ref['T'])) <= 1e-9
    with pytest.raises(ValueError):
        mesheval.eval_pair(posed[:-1], faces, clean, device=dev, align=True)


# ------------------------------------------------------------------------------------------------ 9. eval_free
def test_eval_free_against_the_numpy_statement(dev):
    """The frequency-8 bumpy sphere as result against the frequency-6 one as ground truth.  Distances and angle to 1e-5
    relative.  The nearest ground-truth face of a result centroid: equal to the fp64 arg-min on the rows whose fp64 gap to
    the second-nearest face is >= 1e-5 (relative).  Here the rows below that are NOT rounding cases but exact ties -- 16 of
    1280 centroids (1.25 %) have their closest point on an edge two triangles share, at the same fp64 distance from both --
    so the 0.1 % cap of the point searches cannot hold for any implementation; on those rows the returned face must be an
    fp64 minimiser to the distance bar instead, and the angle's reference takes the returned face there."""
    from geobi_gnn_amd import mesheval
    from geobi_gnn_amd.data_util import face_centroids
    from test_gpu_mesheval import _tri_dist_fp64
    (pr, fr), (po, fo) = M.bumpy(8), M.bumpy(6)
    got = mesheval.eval_free(pr, fr, po, fo, device=dev)
    ref, face64, gap = M.eval_free64(pr, fr, po, fo)
    prd, frd = _t(pr, dev), _t(fr, dev, torch.int32)
    dist, face = mesheval.point_to_mesh(face_centroids(prd, frd), _t(po, dev), _t(fo, dev, torch.int32))
    face = face.cpu().numpy()
    keep = gap >= 1e-5
    print('nearest face: %d of %d rows with an fp64 gap below 1e-5 (smallest %.3g)' % ((~keep).sum(), len(gap), gap.min()))
    assert np.array_equal(face[keep], face64[keep])
    p64, o64 = pr.astype(np.float64), po.astype(np.float64)
    cent = (p64[fr[:, 0]] + p64[fr[:, 1]] + p64[fr[:, 2]]) / 3
    f = fo[face]
    d_at = _tri_dist_fp64(cent, o64[f[:, 0]], o64[f[:, 1]], o64[f[:, 2]])
    f = fo[face64]
    d_min = _tri_dist_fp64(cent, o64[f[:, 0]], o64[f[:, 1]], o64[f[:, 2]])
    assert (np.abs(d_at - d_min) / (d_min + ref['scale'])).max() <= TOL

    def normals(p, t):
        n = np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
        return n / np.linalg.norm(n, axis=1, keepdims=True)
    err = ((normals(p64, fr) - normals(o64, fo)[np.where(keep, face64, face)]) ** 2).sum(1)
    ref['angle'] = (np.arccos(np.clip(1 - err / 2, -1, 1)) * 180 / np.pi).mean()
    assert set(got) == set(ref)
    for key in ('num_f', 'num_v', 'num_f_gt', 'num_v_gt'):
        assert got[key] == ref[key]
    for key in ('angle', 'surf', 'surf_back', 'hausdorff', 'scale', 'surf_norm', 'surf_back_norm'):
        print('%s: %.9g (fp64 %.9g)' % (key, got[key], ref[key]))
        assert abs(got[key] - ref[key]) <= TOL * abs(ref[key]), key
    with pytest.raises(ValueError):
        mesheval.eval_pair(pr, fr, po, gt_faces=fo, device=dev)         # the paired scoring still refuses the pair


# ------------------------------------------------------------------------------------------------ 10. commands
def _run(args):
    run = subprocess.run([sys.executable, '-m', 'geobi_gnn_amd'] + args, cwd=ROOT, timeout=300, capture_output=True, text=True)
    print(run.stdout)
    print(run.stderr)
    return run


def test_align_and_eval_commands(dev, tmp_path):
    """`align` on a folder with a posed bumpy sphere of another frequency (a_1), a same-name file (b) and a broken file, then
    `eval --align --free` on the first folder.  One child process after the other, the next only after the one before
    returned what it should."""
    from geobi_gnn_amd import mesheval, meshio
    src, dst, out = tmp_path / 'src', tmp_path / 'dst', tmp_path / 'out'
    src.mkdir()
    dst.mkdir()
    (p8, f8), (p6, f6) = M.bumpy(8), M.bumpy(6)
    posed8, _, _ = M.pose(p8, degrees=4.0, translation=0.02)
    posed6, _, _ = M.pose(p6, degrees=3.0, translation=0.01, scale=1.1)
    meshio.write_obj(str(dst / 'a.obj'), p6, f6)
    meshio.write_obj(str(dst / 'b.obj'), p6, f6)
    meshio.write_obj(str(src / 'a_1.obj'), posed8, f8)
    meshio.write_obj(str(src / 'b.obj'), posed6, f6)
    run = _run(['align', '--data_dir', str(src), '--target_dir', str(dst), '--out_dir', str(out), '--scale'])
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith('iterations:')]
    assert len(lines) == 2 and "'a_1.obj'" in lines[0] and "'b.obj'" in lines[1] and all('converged: yes' in ln for ln in lines)
    for name, posed, faces in (('a_1.obj', posed8, f8), ('b.obj', posed6, f6)):
        pts, fv = meshio.read_obj(str(out / name))
        assert np.array_equal(fv, faces.astype(np.int32))
        want = mesheval.align(posed, p6, device=dev, estimate_scale=True)
        assert np.array_equal(pts.view(np.uint32), want.xt.cpu().numpy().view(np.uint32))
    assert ('scale: %.6f' % float(want.s[0])) in lines[1] and abs(float(want.s[0]) - 1 / 1.1) <= 1e-4
    # a pair that hits --max_iter is written and reported, not failed; a broken file is skipped, counted, exit status 1
    (src / 'a_2.obj').write_text('v 0 0 0\nf 1 2 3\n')
    run = _run(['align', '--data_dir', str(src), '--target_dir', str(dst), '--out_dir', str(out), '--max_iter', '1'])
    assert run.returncode == 1 and 'skipped:' in run.stderr and '1 of 3 files skipped' in run.stderr
    assert run.stdout.count('converged: no') == 2 and run.stdout.count('iterations:   1') == 2
    os.remove(str(src / 'a_2.obj'))

    run = _run(['eval', '--result_dir', str(src), '--original_dir', str(dst), '--align', '--free'])
    assert run.returncode == 0, run.stderr[-2000:]
    rows = [ln.split() for ln in (src / 'ErrorInfo_free.txt').read_text().splitlines() if ln.strip()]
    assert rows[0][0] == 'Error_free:' and len(rows) == 3 and rows[2][0] == 'a_1.obj' and len(rows[2]) == 11
    want = mesheval.eval_free(posed8, f8, p6, f6, device=dev, align=True)
    cols = ('num_f', 'num_v', 'num_f_gt', 'num_v_gt', 'angle', 'surf', 'surf_norm', 'surf_back', 'surf_back_norm', 'hausdorff')
    for key, tok in zip(cols, rows[2][1:]):
        assert abs(float(tok) - want[key]) <= 0.51e-6, (key, tok, want[key])
    info = [ln.split() for ln in (src / 'AlignInfo.txt').read_text().splitlines() if ln.strip()]
    assert info[0][0] == 'Align:' and len(info) == 2 and info[1][0] == 'a_1.obj' and len(info[1]) == 7
    assert int(info[1][1]) == want['icp_iterations'] and info[1][2] == 'yes'
    assert abs(float(info[1][3]) - want['icp_rmse']) <= 1e-6 * want['icp_rmse']
    assert not (src / 'ErrorInfo_h.txt').exists()
    # without --free a pair of different size is still an error of the command
    run = _run(['eval', '--result_dir', str(src), '--original_dir', str(dst), '--align'])
    assert run.returncode == 1 and 'differ in size' in run.stderr
