"""Correspondence-free losses on the MI355X: the per-mesh nearest-point search (geobi_nearest_parts), the Chamfer vertex
loss (geobi_chamfer_*) and the sided normal loss, against fp64 statements written in numpy; one training epoch and the
``train`` command with ``--loss_v CD --loss_n sided``.

Inputs (checked on the CPU when the tests were written): the frequency-n icosphere as target, a copy jittered by s mean
edge lengths (default_rng(5)) as prediction, (n, s) = (8, 0.5), (16, 0.5), (24, 0.3).  In both search directions the fp64
relative gap between the best and the second-best squared distance is >= 1.58e-5 on every row (>= 6.6e-5 for the face
centroids), far above what fp32 loses in one squared distance, so every index must match the fp64 arg-min.  The index
comparisons still state the condition instead of relying on it: rows with an fp64 gap below 1e-5 are left out, and they
may be at most 0.1 % of the rows."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

from chamfer_model import _argmin64, _cd64, _input, _sided64, _union
from helpers import rel_err
from train_cases import _epoch, _options, _train_command, _write_split

pytestmark = pytest.mark.gpu

TOL = 1e-5                      # the project's bar (tests/test_gpu_kernels.py)
INPUTS = ((8, 0.5), (16, 0.5), (24, 0.3))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------ fp64 statements
def _assert_indices(got, ref, gap, what):
    keep = gap >= 1e-5
    left_out = int((~keep).sum())
    print('%s: %d rows, %d left out (fp64 gap below 1e-5), smallest gap %.3g' % (what, len(ref), left_out, gap.min()))
    assert left_out <= 1e-3 * len(ref)
    assert np.array_equal(np.asarray(got)[keep], ref[keep]), what


# ------------------------------------------------------------------------------------------------ 1. search
def _case_parts(case):
    if case == 'union3':
        return [_input(n, s) for n, s in INPUTS]
    return [_input(*INPUTS[int(case)])]


@pytest.mark.parametrize('case', ['0', '1', '2', 'union3'])
def test_search_matches_fp64_and_the_single_mesh_kernel(dev, case):
    """Both directions: idx = the fp64 arg-min of the row's own part = mesheval.nearest_point on that part alone (offset
    added); sqrt(d2) agrees with its dist to TOL; every index lies in its part."""
    from geobi_gnn_amd import mesheval, ops
    parts = _case_parts(case)
    q, t, _, vptr, _ = _union(parts)
    qd, td = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
    ptr = vptr if len(parts) > 1 else None
    for a, b, what in ((qd, td, 'prediction -> target'), (td, qd, 'target -> prediction')):
        d2, idx = ops.nearest_parts(a, b, ptr, ptr)
        assert d2.dtype == torch.float32 and idx.dtype == torch.int32 and d2.shape == idx.shape == (a.shape[0],)
        idx_h, d2_h = idx.cpu().numpy(), d2.cpu().numpy()
        for k in range(len(parts)):
            lo, hi = vptr[k], vptr[k + 1]
            assert idx_h[lo:hi].min() >= lo and idx_h[lo:hi].max() < hi
            ref, ref_d2, gap = _argmin64(a[lo:hi].cpu().numpy(), b[lo:hi].cpu().numpy())
            _assert_indices(idx_h[lo:hi] - lo, ref, gap, '%s, part %d' % (what, k))
            assert np.abs(d2_h[lo:hi] - ref_d2).max() <= TOL * ref_d2.max()
            dist, alone = mesheval.nearest_point(a[lo:hi], b[lo:hi])
            assert torch.equal(alone, idx[lo:hi] - lo)
            assert rel_err(d2[lo:hi].sqrt(), dist) <= TOL


def test_search_stays_inside_its_part_when_parts_coincide(dev):
    """The same sphere twice, laid over each other: part 1 answers with part 1's rows, the same ones shifted."""
    from geobi_gnn_amd import ops
    q, t, _ = _input(8, 0.5)
    n = len(q)
    qd, td = torch.from_numpy(np.concatenate([q, q])).to(dev), torch.from_numpy(np.concatenate([t, t])).to(dev)
    d2, idx = ops.nearest_parts(qd, td, [0, n, 2 * n], [0, n, 2 * n])
    assert int(idx[:n].min()) >= 0 and int(idx[:n].max()) < n
    assert int(idx[n:].min()) >= n and int(idx[n:].max()) < 2 * n
    assert torch.equal(idx[n:], idx[:n] + n) and torch.equal(d2[n:], d2[:n])
    # unequal part sizes on the two sides: 2 queries parts of n rows against targets of n and n - 7 rows
    d2u, idxu = ops.nearest_parts(qd, td[:2 * n - 7], [0, n, 2 * n], [0, n, 2 * n - 7])
    assert torch.equal(idxu[:n], idx[:n])
    assert int(idxu[n:].min()) >= n and int(idxu[n:].max()) < 2 * n - 7


# ------------------------------------------------------------------------------------------------ 2. exact ties
def _lattice_ref(q, t):
    d = ((q[:, None, :].astype(np.int64) - t[None, :, :].astype(np.int64)) ** 2).sum(2)
    return d.argmin(1), d.min(1)                      # numpy's arg-min is the first = the lowest index


def test_exact_ties_go_to_the_lowest_index(dev):
    """Integer lattice coordinates: every squared distance is exact in fp32, and many targets are equally near (the lattice
    is small, points repeat).  The lowest index wins, on every call, also when the library cuts the targets into slices."""
    from geobi_gnn_amd import ops
    rng = np.random.default_rng(17)
    for Q, T, span in ((700, 900, 3), (50, 40000, 12)):
        q = rng.integers(-span, span + 1, (Q, 3)).astype(np.float32)
        t = rng.integers(-span, span + 1, (T, 3)).astype(np.float32)
        ref_idx, ref_d2 = _lattice_ref(q, t)
        ties = ((q[:, None, :] - t[None, :, :]) ** 2).sum(2) == ref_d2[:, None]
        assert (ties.sum(1) > 1).mean() > 0.5                      # most queries have several equally near targets
        slices = ops.nearest_parts_slices([0, Q], [0, T])
        print('Q = %d, T = %d: %d slices, %.1f equally near targets per query' % (Q, T, slices, ties.sum(1).mean()))
        if T == 40000:
            assert slices > 1
        qd, td = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
        d2, idx = ops.nearest_parts(qd, td)
        assert np.array_equal(idx.cpu().numpy(), ref_idx) and np.array_equal(d2.cpu().numpy(), ref_d2.astype(np.float32))
        for _ in range(3):
            d2_again, idx_again = ops.nearest_parts(qd, td)
            assert torch.equal(idx_again, idx) and torch.equal(d2_again, d2)
    # two parts whose slice counts differ (50 x 40000 next to 700 x 900 of the last draws would need other arrays: build it)
    q2 = rng.integers(-12, 13, (750, 3)).astype(np.float32)
    t2 = rng.integers(-12, 13, (40900, 3)).astype(np.float32)
    qptr, tptr = [0, 50, 750], [0, 40000, 40900]
    d2, idx = ops.nearest_parts(torch.from_numpy(q2).to(dev), torch.from_numpy(t2).to(dev), qptr, tptr)
    for k in range(2):
        ref_idx, ref_d2 = _lattice_ref(q2[qptr[k]:qptr[k + 1]], t2[tptr[k]:tptr[k + 1]])
        assert np.array_equal(idx[qptr[k]:qptr[k + 1]].cpu().numpy(), ref_idx + tptr[k])
        assert np.array_equal(d2[qptr[k]:qptr[k + 1]].cpu().numpy(), ref_d2.astype(np.float32))


def test_forty_parts_take_two_launches(dev):
    """More parts than one launch carries (32): every part still answers as it does alone."""
    from geobi_gnn_amd import ops
    rng = np.random.default_rng(3)
    sizes_q, sizes_t = rng.integers(1, 60, 40), rng.integers(1, 700, 40)
    qptr, tptr = np.cumsum([0] + sizes_q.tolist()).tolist(), np.cumsum([0] + sizes_t.tolist()).tolist()
    q = rng.integers(-6, 7, (qptr[-1], 3)).astype(np.float32)
    t = rng.integers(-6, 7, (tptr[-1], 3)).astype(np.float32)
    d2, idx = ops.nearest_parts(torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev), qptr, tptr)
    for k in range(40):
        ref_idx, ref_d2 = _lattice_ref(q[qptr[k]:qptr[k + 1]], t[tptr[k]:tptr[k + 1]])
        assert np.array_equal(idx[qptr[k]:qptr[k + 1]].cpu().numpy(), ref_idx + tptr[k]), k
        assert np.array_equal(d2[qptr[k]:qptr[k + 1]].cpu().numpy(), ref_d2.astype(np.float32)), k


def test_nan_coordinates_never_give_an_index_outside_the_part(dev):
    from geobi_gnn_amd import ops
    q, t, _ = _input(8, 0.5)
    n = len(q)
    q2 = np.concatenate([q, q])
    q2[n + 5, 1] = np.nan
    qd, td = torch.from_numpy(q2).to(dev), torch.from_numpy(np.concatenate([t, t])).to(dev)
    ptr = [0, n, 2 * n]
    d2, idx = ops.nearest_parts(qd, td, ptr, ptr)
    assert float(d2[n + 5]) == float('inf') and n <= int(idx[n + 5]) < 2 * n
    loss = ops.chamfer_loss(qd.clone().requires_grad_(), td, ptr, ptr)
    assert not bool(torch.isfinite(loss))
    d2b, idxb = ops.nearest_parts(td, qd, ptr, ptr)                # a NaN TARGET is never anybody's nearest
    assert int(idxb[n:].min()) >= n and int(idxb[n:].max()) < 2 * n and not bool((idxb == n + 5).any())


# ------------------------------------------------------------------------------------------------ 3. Chamfer distance
def _cd_device(q, t, ptr, dev):
    from geobi_gnn_amd import ops
    p = torch.from_numpy(q).to(dev).requires_grad_()
    loss = ops.chamfer_loss(p, torch.from_numpy(t).to(dev), ptr, ptr)
    loss.backward()
    return loss.detach(), p.grad


@pytest.mark.parametrize('case', ['0', '1', '2', 'union3'])
def test_chamfer_value_and_gradient_match_fp64(dev, case):
    parts = _case_parts(case)
    q, t, _, vptr, _ = _union(parts)
    loss, grad = _cd_device(q, t, vptr if len(parts) > 1 else None, dev)
    B = len(parts)
    ref, ref_grad, singles = 0.0, [], []
    for qk, tk, _ in parts:
        c, g = _cd64(qk, tk)
        ref += c / B
        ref_grad.append(g / B)
        singles.append(float(_cd_device(qk, tk, None, dev)[0]))
    ref_grad = torch.from_numpy(np.concatenate(ref_grad))
    print('CD %.9g (fp64 %.9g), gradient rel err %.3g' % (float(loss), ref, rel_err(grad.cpu(), ref_grad)))
    assert abs(float(loss) - ref) <= TOL * abs(ref)
    assert rel_err(grad.cpu(), ref_grad) <= TOL
    assert abs(float(loss) - float(np.mean(singles))) <= TOL * abs(ref)        # batch = mean of the single-mesh values
    again, grad_again = _cd_device(q, t, vptr if len(parts) > 1 else None, dev)
    assert torch.equal(again, loss) and torch.equal(grad_again, grad)           # two runs, bit for bit


def test_chamfer_of_a_set_with_itself_is_exactly_zero(dev):
    _, t, _, vptr, _ = _union(_case_parts('union3'))
    for ptr in (None, vptr):
        loss, grad = _cd_device(t, t, ptr, dev)
        assert float(loss) == 0.0 and bool((grad == 0).all())


def test_chamfer_ignores_the_order_of_the_target_rows_and_l2_does_not(dev):
    from geobi_gnn_amd import network
    q, t, _ = _input(16, 0.5)
    perm = np.random.default_rng(2).permutation(len(t))
    qd = torch.from_numpy(q).to(dev)
    td, tp = torch.from_numpy(t).to(dev), torch.from_numpy(t[perm]).to(dev)
    cd, cd_perm = float(network.loss_v(qd, td, 'CD')), float(network.loss_v(qd, tp, 'CD'))
    l2, l2_perm = float(network.loss_v(qd, td, 'L2')), float(network.loss_v(qd, tp, 'L2'))
    print('CD %.9g -> %.9g under a permutation of the target rows; L2 %.6g -> %.6g' % (cd, cd_perm, l2, l2_perm))
    assert abs(cd - cd_perm) < 1e-6 * cd
    assert abs(l2 - l2_perm) > 0.5 * l2


# ------------------------------------------------------------------------------------------------ 4. sided normal loss
@pytest.mark.parametrize('case', ['0', '1', '2', 'union3'])
def test_sided_value_and_gradient_match_fp64(dev, case):
    """Face centroids and unit normals of the noisy (prediction) and the clean (ground truth) mesh, formed on the device;
    the fp64 statement searches in the same centroids."""
    from geobi_gnn_amd import ops
    from geobi_gnn_amd.data_util import computer_face_normal, face_centroids
    from geobi_gnn_amd.parallel import _mesh_weights
    parts = _case_parts(case)
    q, t, faces, _, fptr = _union(parts)
    qd, td = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
    fv = torch.from_numpy(faces).to(dev)
    fc_p, fc = face_centroids(qd, fv), face_centroids(td, fv)
    normals = computer_face_normal(td, fv).contiguous()
    B = len(parts)
    weights = None
    if B > 1:
        bag = argparse.Namespace(mesh_ptr=torch.tensor(fptr), y=normals)
        weights = _mesh_weights(bag)

    def run():
        np_ = computer_face_normal(qd, fv).detach().clone().requires_grad_()
        loss = ops.sided_loss(np_, normals, fc_p, fc, fptr if B > 1 else None, weights)
        loss.backward()
        return np_, loss.detach(), np_.grad
    np_, loss, grad = run()
    ref, ref_grad = 0.0, []
    for k in range(B):
        lo, hi = fptr[k], fptr[k + 1]
        s, g = _sided64(np_[lo:hi].detach().cpu().numpy(), normals[lo:hi].cpu().numpy(), fc_p[lo:hi].cpu().numpy(),
                        fc[lo:hi].cpu().numpy())
        ref += s / B
        ref_grad.append(g / B)
        _, idx = ops.nearest_parts(fc_p[lo:hi], fc[lo:hi])
        ref_idx, _, gap = _argmin64(fc_p[lo:hi].cpu().numpy(), fc[lo:hi].cpu().numpy())
        _assert_indices(idx.cpu().numpy(), ref_idx, gap, 'centroids, part %d' % k)
    ref_grad = torch.from_numpy(np.concatenate(ref_grad))
    print('sided %.9g (fp64 %.9g), gradient rel err %.3g' % (float(loss), ref, rel_err(grad.cpu(), ref_grad)))
    assert abs(float(loss) - ref) <= TOL * abs(ref)
    assert rel_err(grad.cpu(), ref_grad) <= TOL
    _, again, grad_again = run()
    assert torch.equal(again, loss) and torch.equal(grad_again, grad)


# ------------------------------------------------------------------------------------------------ 5. surface
def test_network_losses_reach_the_kernels_and_batched_losses_agrees(dev):
    from geobi_gnn_amd import network, ops
    from geobi_gnn_amd.data_util import computer_face_normal, face_centroids
    from geobi_gnn_amd.parallel import batched_losses
    parts = _case_parts('union3')
    singles_v, singles_n = [], []
    for q, t, faces in parts:
        qd, td, fv = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(faces).to(dev)
        p = qd.clone().requires_grad_()
        lv = network.loss_v(p, td, 'CD')
        lv.backward()
        assert torch.equal(lv.detach(), ops.chamfer_loss(qd, td).detach()) and bool(p.grad.abs().sum() > 0)
        np_ = computer_face_normal(qd, fv).detach().clone().requires_grad_()
        n_ = computer_face_normal(td, fv).contiguous()
        ln = network.loss_n(np_, n_, 'sided', face_centroids(qd, fv), face_centroids(td, fv))
        ln.backward()
        assert bool(np_.grad.abs().sum() > 0)
        singles_v.append(float(lv))
        singles_n.append(float(ln))
    q, t, faces, vptr, fptr = _union(parts)
    qd, td, fv = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(faces).to(dev)
    dv = argparse.Namespace(y=td, mesh_ptr=torch.tensor(vptr))
    df = argparse.Namespace(y=computer_face_normal(td, fv).contiguous(), mesh_ptr=torch.tensor(fptr), fv_indices=fv)
    npred = computer_face_normal(qd, fv).contiguous()
    lv, ln = batched_losses(qd, npred, dv, df, 'CD', 'sided')
    assert abs(float(lv) - np.mean(singles_v)) <= TOL * np.mean(singles_v)
    assert abs(float(ln) - np.mean(singles_n)) <= TOL * np.mean(singles_n)
    # the CPU statement of the same call (torch ops) agrees with the device
    dv_c = argparse.Namespace(y=td.cpu(), mesh_ptr=torch.tensor(vptr))
    df_c = argparse.Namespace(y=df.y.cpu(), mesh_ptr=torch.tensor(fptr), fv_indices=fv.cpu())
    lv_c, ln_c = batched_losses(qd.cpu(), npred.cpu(), dv_c, df_c, 'CD', 'sided')
    assert abs(float(lv) - float(lv_c)) <= TOL * float(lv_c) and abs(float(ln) - float(ln_c)) <= TOL * float(ln_c)


def test_documented_errors(dev):
    from geobi_gnn_amd import _lib as L
    from geobi_gnn_amd import network, ops
    from geobi_gnn_amd.parallel import batched_losses
    q, t, faces = _input(8, 0.5)
    n = len(q)
    qd, td = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
    with pytest.raises(ValueError, match='centroids'):
        network.loss_n(qd, td, 'sided')
    with pytest.raises(ValueError, match='L1, L2, CD'):
        network.loss_v(qd, td, 'nonsense')
    bag = argparse.Namespace(y=td, fv_indices=torch.from_numpy(faces).to(dev))
    with pytest.raises(ValueError, match='L1, L2, sided'):
        batched_losses(qd, qd, bag, bag, 'CD', 'nonsense')
    with pytest.raises(NotImplementedError):
        network.loss_v(qd, td, 'EMD')
    with pytest.raises(NotImplementedError):
        network.loss_v(qd, td, 'CD', apply_icp=True)
    with pytest.raises(L.GeobiError, match='empty'):                       # an empty part is an error, not a launch
        ops.nearest_parts(qd, td, [0, 0, n], [0, 10, n])
    with pytest.raises(L.GeobiError, match='empty'):
        ops.chamfer_loss(qd, td, [0, 10, n], [0, n, n])
    with pytest.raises(L.GeobiError, match='empty'):
        ops.nearest_parts(qd[:0], td)
    with pytest.raises(L.GeobiError, match='does not cover'):              # a pointer that does not end at the row count
        ops.nearest_parts(qd, td, [0, n + 5], [0, n])
    with pytest.raises(L.GeobiError, match='parts'):
        ops.nearest_parts(qd, td, [0, 10, n], [0, n])
    with pytest.raises(L.GeobiError, match='no CPU fallback'):             # CPU tensors handed to the device path
        ops.nearest_parts(qd.cpu(), td.cpu())
    with pytest.raises(L.GeobiError, match='no CPU fallback'):
        ops.chamfer_loss(qd.cpu(), td)
    with pytest.raises(L.GeobiError, match='no CPU fallback'):
        ops.sided_loss(qd.cpu(), td, qd, td)
    ok, _ = ops.nearest_parts(qd, td)                                      # the library still answers after the errors
    assert bool(torch.isfinite(ok).all())


# ------------------------------------------------------------------------------------------------ 6. one training epoch
def test_train_epoch_with_cd_and_sided_equals_the_loop_written_out(dev, tmp_path):
    """4 frequency-8 samples, batch 2: trainer.train_epoch with loss_v='CD', loss_n='sided' leaves the flat parameters
    bit-identical to forward, batched_losses, dual_loss, backward, step called one after the other; two runs agree bit
    for bit; the L1 / L1 epoch ends elsewhere; evaluation yields finite numbers."""
    from geobi_gnn_amd import network, train_util, trainer
    from geobi_gnn_amd.data import union_batch_graphs
    from geobi_gnn_amd.dataset import DualDataset
    from geobi_gnn_amd.parallel import FlatParameters, batched_losses, shard_indices
    root = str(tmp_path)
    _write_split(root, 'train', ('a', 'b'), 8, (0.1, 0.3), seed0=900)
    ds = DualDataset(root, 'train', device=dev, cache=False)
    assert len(ds) == 4
    opt = _options(batch_size=2, loss_v='CD', loss_n='sided')
    got = _epoch(ds, dev, opt)
    assert torch.equal(got, _epoch(ds, dev, opt))
    assert not torch.equal(got, _epoch(ds, dev, _options(batch_size=2)))

    torch.manual_seed(11)
    net = network.DualGNN().to(dev)
    flat = FlatParameters(net)
    optimizer = train_util.make_optimizer(opt, flat.parameters(), fused=True)
    start = flat.flat_param.detach().clone()
    net.train()
    order = shard_indices(len(ds), 0, 1, seed=opt.seed, epoch=1)
    for s in range(0, len(order), 2):
        dv, df = union_batch_graphs([ds[i] for i in order[s:s + 2]])
        flat.bucket.zero()
        vp, npred, _ = net((dv.shallow_copy(), df.shallow_copy()))
        lv, ln = batched_losses(vp, npred, dv, df, 'CD', 'sided')
        network.dual_loss(lv, ln, opt.loss_v_scale, opt.loss_n_scale).backward()
        optimizer.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(flat.flat_param).all())
    assert not torch.equal(start, flat.flat_param.detach())
    assert torch.equal(got, flat.flat_param.detach())
    res = trainer.evaluate(net, ds, opt)
    assert all(np.isfinite(v) for v in res.values()) and res['eval_loss_v'] > 0 and res['eval_loss_f'] > 0


# ------------------------------------------------------------------------------------------------ 7. command
def test_train_command_with_cd_and_sided(dev, tmp_path):
    """python -m geobi_gnn_amd train --loss_v CD --loss_n sided on the tiny split of test_train_command_end_to_end
    (frequency-8 icospheres, 6 train files, 2 test files), 5 epochs, batch 2.  Child processes one after the other, each
    under its own timeout, the next only after the one before returned what it should."""
    data = str(tmp_path / 'Synthetic')
    _write_split(data, 'train', ('s1', 's2', 's3'), 8, (0.1, 0.3), seed0=700)
    _write_split(data, 'test', ('t1',), 8, (0.1, 0.3), seed0=800)

    bad = _train_command(data, str(tmp_path / 'bad'), extra=('--no_predict', '--loss_v', 'nonsense'))
    assert bad.returncode != 0
    assert 'L1, L2, CD' in bad.stderr and 'samples from' not in bad.stdout          # before any mesh was read
    assert not os.path.exists(str(tmp_path / 'bad'))

    losses = ('--no_predict', '--loss_v', 'CD', '--loss_n', 'sided')
    out = str(tmp_path / 'run1')
    run = _train_command(data, out, extra=losses)
    assert run.returncode == 0, run.stderr[-2000:]
    sd = torch.load(os.path.join(out, 'GeoBi-GNN_Synthetic_model.pth'), map_location='cpu', weights_only=True)
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
    with open(os.path.join(out, 'GeoBi-GNN_Synthetic_params.json')) as fh:
        params = json.load(fh)
    assert params['loss_v'] == 'CD' and params['loss_n'] == 'sided'
    log = open(os.path.join(out, 'training_info.txt')).read()
    recs = [json.loads(ln) for ln in log.splitlines() if ln.startswith('{"epoch"')]
    assert [r['epoch'] for r in recs] == [0, 1, 2, 3, 4, 5]
    for r in recs:
        assert all(np.isfinite(v) for v in r.values() if isinstance(v, float)), r
    assert all(np.isfinite(r['train_loss']) for r in recs[1:])
    assert any(r['saved'] for r in recs[1:])

    out2 = str(tmp_path / 'run2')
    run2 = _train_command(data, out2, extra=losses)
    assert run2.returncode == 0, run2.stderr[-2000:]
    sd2 = torch.load(os.path.join(out2, 'GeoBi-GNN_Synthetic_model.pth'), map_location='cpu', weights_only=True)
    assert list(sd2) == list(sd)
    for k in sd:
        assert torch.equal(sd[k], sd2[k]), k
