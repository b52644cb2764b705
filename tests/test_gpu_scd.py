"""The sampled surface Chamfer loss on the MI355X: the batched sampler against the single-mesh sampler bit
for bit, the points on faces and their inverse-list backward against the fp64 model of tests/scd_model.py, the workspace
of the batched weights, the loss end to end, one training epoch and the ``train`` command with ``--loss_v SCD``.

Tolerances: where the issue is equality of two device paths the comparison is bit for bit; against fp64 it is the
project's TOL = 1e-5 (the backward sums in fp64 and rounds once, the forward is three float32 roundings)."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import sample_model as S
import scd_model as M
from chamfer_model import _input, _union
from helpers import rel_err
from train_cases import _epoch, _options, _train_command, _write_split

pytestmark = pytest.mark.gpu

TOL = 1e-5                      # the project's bar (tests/test_gpu_chamfer.py)
INPUTS = ((8, 0.5), (16, 0.5), (24, 0.3))          # tests/test_gpu_chamfer.py's
PAD, SENTINEL, SHORT_BY = 4096, 0xA5, 512          # tests/test_gpu_workspace.py's guard band


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


def _t(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


def _degenerate(F):
    return (0, F // 2, F // 2 + 1, F // 2 + 2, F - 1) if F >= 8 else ()


def _strips(counts, degenerate=_degenerate):
    """One strip per face count -> [(points float32, faces int32 with LOCAL ids)], the union's points, faces (global ids),
    vptr, fptr."""
    meshes = [S.strip(F, seed=(F + 13 * k) % 97, degenerate=degenerate(F), offset=0.25 * k) for k, F in enumerate(counts)]
    vptr = np.cumsum([0] + [len(p) for p, _ in meshes]).tolist()
    fptr = np.cumsum([0] + [len(f) for _, f in meshes]).tolist()
    pts = np.concatenate([p for p, _ in meshes])
    faces = np.concatenate([f + o for (_, f), o in zip(meshes, vptr)]).astype(np.int32)
    return meshes, pts, faces, vptr, fptr


_SIX = {}


def _six():
    """Part face counts 1, 2, T - 1, T, T + 1, 2 T + 1 around the LDS table of the draw, built once."""
    if not _SIX:
        from geobi_gnn_amd import meshsample
        T = meshsample.table_entries()
        assert 8 <= T < 100000
        _SIX['u'] = _strips([1, 2, T - 1, T, T + 1, 2 * T + 1])
    return _SIX['u']


def _assert_parts_equal_singles(dev, union, n, first, stream_ids, seed=11, draw=3):
    """weights, cum, exponent, face, bary, points of the batched calls == the single-mesh calls on every part, bit for bit"""
    from geobi_gnn_amd import meshsample
    meshes, pts, faces, _, fptr = union
    pd, fd = _t(pts, dev), _t(faces, dev, torch.int32)
    weights = meshsample.surface_weights_parts(pd, fd, fptr)
    assert weights[0].dtype == torch.int64 and weights[1].dtype == torch.int64 and weights[2].dtype == torch.int32
    got = meshsample.sample_surface_parts(pd, fd, fptr, n, seed=seed, stream_ids=stream_ids, draw=draw, first=first,
                                          weights=weights)
    fresh = meshsample.sample_surface_parts(pd, fd, fptr, n, seed=seed, stream_ids=stream_ids, draw=draw, first=first)
    assert all(torch.equal(a, b) for a, b in zip(got, fresh))                    # weights given or built inside
    P = len(meshes)
    assert got.points.shape == (P * n, 3) and got.face.shape == (P * n,) and got.bary.shape == (P * n, 3)
    exps = weights[2].tolist()
    for k, (p, f) in enumerate(meshes):
        pk, fk = _t(p, dev), _t(f, dev, torch.int32)
        w1, cum1, e1 = meshsample.surface_weights(pk, fk)
        rows = slice(fptr[k], fptr[k + 1])
        assert torch.equal(weights[0][rows], w1) and torch.equal(weights[1][rows], cum1) and exps[k] == e1, k
        one = meshsample.sample_surface(pk, fk, n, seed=seed, stream_id=stream_ids[k], draw=draw, first=first)
        r = slice(k * n, (k + 1) * n)
        assert torch.equal(got.face[r], one.face + fptr[k]), k
        assert torch.equal(got.bary[r], one.bary) and torch.equal(got.points[r], one.points), k
    return got, weights


# ------------------------------------------------------------------------------------------------ 1. the batched sampler
@pytest.mark.parametrize('first', [0, 1000])
def test_batched_sampler_equals_the_single_mesh_sampler_bit_for_bit(dev, first):
    """Six meshes in one union, face counts around the LDS table, N = 3 000 per part, distinct stream ids; first = 1 000
    continues a draw: its rows are rows 1 000 .. of the longer draw."""
    from geobi_gnn_amd import meshsample
    union = _six()
    sid = [11, 3, 7, 0, 5, 2 ** 32 - 1]
    got, weights = _assert_parts_equal_singles(dev, union, 3000, first, sid)
    w = weights[0]
    assert bool((w[got.face.long()] > 0).all())                                  # never a zero-weight face
    if first:
        _, pts, faces, _, fptr = union
        whole = meshsample.sample_surface_parts(_t(pts, dev), _t(faces, dev, torch.int32), fptr, 4000, seed=11, stream_ids=sid,
                                                draw=3, weights=weights)
        for k in range(6):
            assert torch.equal(whole.points[k * 4000 + 1000:(k + 1) * 4000], got.points[k * 3000:(k + 1) * 3000])


def test_thirty_three_parts_take_two_launches(dev):
    union = _strips([1 + (k % 3) for k in range(33)])
    _assert_parts_equal_singles(dev, union, 300, 0, list(range(40, 73)))


def test_zero_weight_faces_beside_real_ones_are_never_drawn(dev):
    deg = (0, 5, 6, 11)
    union = _strips([12, 3], degenerate=lambda F: deg if F == 12 else ())
    got, weights = _assert_parts_equal_singles(dev, union, 3000, 0, [1, 2])
    w = weights[0].cpu().numpy()
    assert (w[list(deg)] == 0).all() and (np.delete(w, deg) > 0).all()
    face = got.face.cpu().numpy()
    assert not np.isin(face[:3000], deg).any() and (face[:3000] < 12).all() and (face[3000:] >= 12).all()
    assert (np.bincount(face, minlength=15)[np.delete(np.arange(15), deg)] > 0).all()      # every real face is drawn


def test_batched_sampler_refusals(dev):
    from geobi_gnn_amd import _lib, meshsample
    _, pts, faces, _, fptr = _strips([4, 2, 3], degenerate=lambda F: (0, 1) if F == 2 else ())
    pd, fd = _t(pts, dev), _t(faces, dev, torch.int32)
    with pytest.raises(_lib.GeobiError, match='part 1 is a mesh without area'):
        meshsample.sample_surface_parts(pd, fd, fptr, 10, seed=1, stream_ids=[0, 1, 2])
    ok = [0, 4, 9]                                                               # the flat part joined to its neighbour
    assert meshsample.sample_surface_parts(pd, fd, ok, 10, seed=1, stream_ids=[0, 1]).face.shape == (20,)
    with pytest.raises(_lib.GeobiError, match='no CPU fallback'):
        meshsample.sample_surface_parts(pd.cpu(), fd.cpu(), ok, 10, seed=1, stream_ids=[0, 1])
    with pytest.raises(_lib.GeobiError, match='no CPU fallback'):
        meshsample.surface_weights_parts(pd.cpu(), fd.cpu(), ok)
    bad = fd.clone()
    bad[3, 1] = pd.shape[0]
    for broken in (bad, -fd - 1):
        with pytest.raises(_lib.GeobiError, match='outside'):
            meshsample.sample_surface_parts(pd, broken, ok, 10, seed=1, stream_ids=[0, 1])
    with pytest.raises(ValueError, match='rows per draw'):
        meshsample.sample_surface_parts(pd, fd, ok, 1 << 23, seed=1, stream_ids=[0, 1])      # P * N = 2^24
    for short in ([0, 4, 8], [1, 4, 9], [0, 9, 4, 9]):
        with pytest.raises(_lib.GeobiError, match='does not cover|empty part'):
            meshsample.sample_surface_parts(pd, fd, short, 10, seed=1, stream_ids=[0] * (len(short) - 1))
    with pytest.raises(ValueError, match='stream ids'):
        meshsample.sample_surface_parts(pd, fd, ok, 10, seed=1, stream_ids=[0])
    # the library's own checks, behind the Python layer's
    import ctypes
    arr = (ctypes.c_int64 * 3)(0, 4, 4)
    with pytest.raises(_lib.GeobiError, match='part 1 of .* is empty'):
        _lib.call('geobi_sample_surface_parts', pd.data_ptr(), fd.data_ptr(), pd.data_ptr(), ctypes.cast(arr, ctypes.c_void_p), 2,
                  pd.shape[0], 10, 0, 1, ctypes.cast(arr, ctypes.c_void_p), 0, pd.data_ptr(), pd.data_ptr(), pd.data_ptr(),
                  _lib.stream())


# ------------------------------------------------------------------------------------------------ 2. points on faces
def test_bary_points_returns_the_samplers_points_bit_for_bit(dev):
    from geobi_gnn_amd import meshsample, ops
    _, pts, faces, _, fptr = _six()
    pd, fd = _t(pts, dev), _t(faces, dev, torch.int32)
    s = meshsample.sample_surface_parts(pd, fd, fptr, 3000, seed=5, stream_ids=list(range(6)), draw=1)
    assert torch.equal(ops.bary_points(pd, fd, s.face, s.bary), s.points)


def _bwd_case(name):
    """-> points float32 [V,3], faces int32 [F,3], face [n], bary float32 [n,3]"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == 'hub':                                   # 5 000 samples on a fan of 64 faces: ~5 000 entries in the hub's list
        p, f = M.fan(64)
        n = 5000
    elif name == 'V3':
        p, f = S.strip(1, seed=2)
        n = 100
    else:
        p, f = S.strip(40, seed=3)
        n = {'untouched': 300, 'minus1': 300}.get(name) or int(name)
    if name == 'untouched':                             # vertices no face names, first, last and in the middle
        extra = rng.standard_normal((3, 3)).astype(np.float32)
        p = np.concatenate([extra[:1], p[:20], extra[1:2], p[20:], extra[2:]])
        f = np.where(f < 20, f + 1, f + 2).astype(np.int32)
    face = rng.integers(0, len(f), n)
    if name == 'minus1':
        face[::7] = -1
    bary = rng.dirichlet(np.ones(3), n).astype(np.float32)
    return p, f, face, bary


@pytest.mark.parametrize('name', ['1', '255', '256', '257', 'hub', 'untouched', 'minus1', 'V3'])
def test_bary_points_backward_matches_the_fp64_model(dev, name):
    """Forward and backward under an injected gx against the loops of the model; two runs agree bit for bit, and so does a
    gx that arrives as a view."""
    from geobi_gnn_amd import ops
    p, f, face, bary = _bwd_case(name)
    n, V = len(face), len(p)
    gx = np.random.default_rng(9).standard_normal((n, 6)).astype(np.float32)
    fd, faced, baryd = _t(f, dev, torch.int32), _t(face, dev, torch.int32), _t(bary, dev)
    wide = _t(gx, dev)

    def run(g):
        pd = _t(p, dev).requires_grad_()
        x = ops.bary_points(pd, fd, faced, baryd)
        x.backward(g)
        return x.detach(), pd.grad
    x, gp = run(wide[:, :3].contiguous())
    x2, gp2 = run(wide[:, :3])                          # a view: made contiguous on the way in
    x3, gp3 = run(wide[:, :3].contiguous())
    assert torch.equal(gp, gp2) and torch.equal(gp, gp3) and torch.equal(x, x2) and torch.equal(x, x3)
    ref_x = M.bary_points64(p, f, face, bary)
    ref = M.bary_points_bwd_loops(f, face, bary, gx[:, :3], V)
    lists = M.inverse_lists(f, face, V)
    longest = max(len(v) for v in lists)
    err_x, err = rel_err(x.cpu(), torch.from_numpy(ref_x)), rel_err(gp.cpu(), torch.from_numpy(ref))
    print('%s: n = %d, V = %d, longest list %d entries, forward rel err %.3g, backward rel err %.3g'
          % (name, n, V, longest, err_x, err))
    assert err_x <= TOL and err <= TOL
    untouched = [v for v, entries in enumerate(lists) if not entries]
    assert bool((gp[untouched] == 0).all())                                      # exact zero rows
    if name == 'hub':
        assert longest == n
    if name == 'untouched':
        assert {0, 21, V - 1} <= set(untouched)
    if name == 'minus1':
        assert bool((x[::7] == 0).all())
        live = face >= 0                                                         # the -1 rows contribute nothing
        assert np.array_equal(ref, M.bary_points_bwd_loops(f, face[live], bary[live], gx[live, :3], V))
    if name == 'V3':
        assert V == 3


# ------------------------------------------------------------------------------------------------ 3. workspace
class _Guarded(object):
    """tests/test_gpu_workspace.py's replacement of _lib.workspace: the memory behind the workspace is the test's and
    holds 0xA5; short = True hands the request out 512 bytes short."""

    def __init__(self, short=False):
        self.short, self.requests = short, []

    def __call__(self, nbytes, device):
        nbytes = int(nbytes)
        give = nbytes - SHORT_BY if self.short else nbytes
        buf = torch.empty(nbytes + PAD, dtype=torch.uint8, device=device)
        buf[give:] = SENTINEL
        self.requests.append((buf, give, nbytes))
        return buf[:give]

    def sentinels_whole(self):
        torch.cuda.synchronize()
        return all(bool((buf[give:] == SENTINEL).all()) for buf, give, _ in self.requests)


def test_weights_parts_workspace_guard_band_and_short_request(dev, monkeypatch):
    from geobi_gnn_amd import _lib, meshsample
    _, pts, faces, _, fptr = _six()
    pd, fd = _t(pts, dev), _t(faces, dev, torch.int32)
    want = meshsample.surface_weights_parts(pd, fd, fptr)
    guard = _Guarded()
    monkeypatch.setattr(_lib, 'workspace', guard)
    got = meshsample.surface_weights_parts(pd, fd, fptr)
    assert len(guard.requests) == 1 and guard.requests[0][2] > SHORT_BY, 'one workspace, and a size query that answered'
    assert guard.sentinels_whole(), 'the launcher wrote behind its workspace'
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    short = _Guarded(short=True)
    monkeypatch.setattr(_lib, 'workspace', short)
    with pytest.raises(_lib.GeobiError) as e:
        meshsample.surface_weights_parts(pd, fd, fptr)
    assert short.sentinels_whole()
    m = re.search(r'sample_weights_parts: workspace too small \((\d+) bytes given, (\d+) needed\)', str(e.value))
    assert m, str(e.value)
    _, give, nbytes = short.requests[0]
    assert int(m.group(1)) == give and give < int(m.group(2)) <= nbytes


# ------------------------------------------------------------------------------------------------ 4. the loss end to end
def _case_parts(case):
    return [_input(n, s) for n, s in INPUTS] if case == 'union3' else [_input(*INPUTS[0])]


def _scd_device(q, t, faces, fptr, vptr, n, dev, sid, seed=3, draw=2):
    from geobi_gnn_amd import ops
    p = _t(q, dev).requires_grad_()
    loss = ops.sampled_chamfer_loss(p, _t(t, dev), _t(faces, dev, torch.int32), fptr, vptr, n, seed, sid, draw)
    loss.backward()
    return loss.detach(), p.grad


@pytest.mark.parametrize('case', ['0', 'union3'])
def test_scd_value_and_gradient_match_fp64(dev, case):
    """N = 2 000 per mesh.  The value against the fp64 model on the device's own samples (fp64 arg-mins); the gradient
    against the model that takes the device's two index maps (tests/test_gpu_chamfer.py checks the maps themselves); the
    batch value is the mean of the single-mesh values; two runs agree bit for bit."""
    from geobi_gnn_amd import meshsample, ops
    parts = _case_parts(case)
    q, t, faces, vptr, fptr = _union(parts)
    n, seed, draw, P = 2000, 3, 2, len(parts)
    sid = [5, 0, 9][:P]
    loss, grad = _scd_device(q, t, faces, fptr, vptr, n, dev, sid)
    again, grad_again = _scd_device(q, t, faces, fptr, vptr, n, dev, sid)
    assert torch.equal(again, loss) and torch.equal(grad_again, grad)

    qd, td, fd = _t(q, dev), _t(t, dev), _t(faces, dev, torch.int32)
    sp = meshsample.sample_surface_parts(qd, fd, fptr, n, seed=seed, stream_ids=sid, draw=2 * draw + 1)
    st = meshsample.sample_surface_parts(td, fd, fptr, n, seed=seed, stream_ids=sid, draw=2 * draw)
    sptr = [k * n for k in range(P + 1)]
    x = ops.bary_points(qd, fd, sp.face, sp.bary)
    ia, ib = ops.nearest_parts(x, st.points, sptr, sptr)[1], ops.nearest_parts(st.points, x, sptr, sptr)[1]
    face, bary, y = sp.face.cpu().numpy(), sp.bary.cpu().numpy(), st.points.cpu().numpy()
    ref, _, _ = M.scd64(q, faces, face, bary, y, n)
    _, ref_grad, _ = M.scd64(q, faces, face, bary, y, n, maps=(ia.cpu().numpy(), ib.cpu().numpy()))
    err = rel_err(grad.cpu(), torch.from_numpy(ref_grad))
    print('SCD %.9g (fp64 %.9g), gradient rel err %.3g' % (float(loss), ref, err))
    assert abs(float(loss) - ref) <= TOL * abs(ref)
    assert err <= TOL and bool((grad != 0).any())

    singles = []
    for k, (qk, tk, fk) in enumerate(parts):
        singles.append(float(_scd_device(qk, tk, fk, None, None, n, dev, [sid[k]])[0]))
    assert abs(float(loss) - float(np.mean(singles))) <= TOL * abs(ref)


def test_scd_of_a_mesh_with_itself(dev):
    """The same draw parity forced on both sides (the pieces called by hand): the two sample sets are equal bit for bit and
    the loss is exactly 0.  With the parities of the loss the sets differ: a small positive value, bounded by the spacing
    of N area-uniform samples (mean squared distance to the nearest of N samples on an area A ~ A / (pi N) per direction;
    ten times that is asserted)."""
    from geobi_gnn_amd import meshsample, ops
    _, t, faces, vptr, fptr = _union(_case_parts('union3'))
    td, fd = _t(t, dev), _t(faces, dev, torch.int32)
    n, P = 2000, 3
    s = meshsample.sample_surface_parts(td, fd, fptr, n, seed=3, stream_ids=[0, 1, 2], draw=4)
    sptr = [k * n for k in range(P + 1)]
    assert float(ops.chamfer_loss(ops.bary_points(td, fd, s.face, s.bary), s.points, sptr, sptr)) == 0.0
    value = float(ops.sampled_chamfer_loss(td, td, fd, fptr, vptr, n, 3, [0, 1, 2], 2))
    t64 = t.astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(t64[faces[:, 1]] - t64[faces[:, 0]], t64[faces[:, 2]] - t64[faces[:, 0]]), axis=1)
    spacing = np.mean([2 * area[a:b].sum() / (math.pi * n) for a, b in zip(fptr[:-1], fptr[1:])])
    print('SCD of a mesh with itself: %.6g (sample spacing term %.6g)' % (value, spacing))
    assert 0 < value < 10 * spacing


def test_folded_quad_on_the_device(dev):
    from geobi_gnn_amd import network
    p, t, faces = M.folded_pair(0.3)
    pd, td, fd = _t(p, dev).requires_grad_(), _t(t, dev), _t(faces, dev, torch.int32)
    cd = network.loss_v(pd, td, 'CD')
    cd.backward()
    assert float(cd.detach()) == 0.0 and bool((pd.grad == 0).all())
    pd.grad = None
    scd = network.loss_v(pd, td, 'SCD', faces=fd, samples=2000, seed=1)
    scd.backward()
    ref, _ = M.scd_of_meshes(p, t, faces, [0, 2], 2000, seed=1, stream_ids=[0])
    print('folded quad: SCD %.6g (host model %.6g), |gradient| per vertex %s' % (float(scd.detach()), ref, pd.grad.norm(dim=1).tolist()))
    assert abs(float(scd.detach()) - ref) <= TOL * ref                           # the host model draws the same points
    assert float(scd.detach()) > 1e-3 and bool((pd.grad.norm(dim=1) > 0).all())
    with pytest.raises(ValueError, match='faces'):
        network.loss_v(pd, td, 'SCD')


# ------------------------------------------------------------------------------------------------ 5. training
def test_train_epoch_with_scd_equals_the_loop_written_out(dev, tmp_path):
    """4 frequency-5 samples, batch 2, --loss_v SCD --loss_n sided --loss_lap_scale 0.5 with 500 samples: train_epoch
    leaves the flat parameters bit-identical to the pieces called one after the other with the documented rule (seed =
    opt.seed, draw = epoch, stream ids = the dataset indices of the batch); two runs agree; evaluation is repeatable."""
    from geobi_gnn_amd import network, train_util, trainer
    from geobi_gnn_amd.data import union_batch_graphs
    from geobi_gnn_amd.dataset import DualDataset
    from geobi_gnn_amd.parallel import FlatParameters, add_regularisers, batched_losses, shard_indices
    root = str(tmp_path)
    _write_split(root, 'train', ('a', 'b'), 5, (0.1, 0.3), seed0=900)
    ds = DualDataset(root, 'train', device=dev, cache=False)
    assert len(ds) == 4
    opt = _options(batch_size=2, loss_v='SCD', loss_n='sided', loss_lap_scale=0.5, loss_samples=500)
    got = _epoch(ds, dev, opt, epochs=2)
    assert torch.equal(got, _epoch(ds, dev, opt, epochs=2))
    assert not torch.equal(got, _epoch(ds, dev, _options(batch_size=2, loss_v='CD', loss_n='sided', loss_lap_scale=0.5), epochs=2))

    torch.manual_seed(11)
    net = network.DualGNN().to(dev)
    flat = FlatParameters(net)
    optimizer = train_util.make_optimizer(opt, flat.parameters(), fused=True)
    for epoch in (1, 2):
        net.train()
        order = shard_indices(len(ds), 0, 1, seed=opt.seed, epoch=epoch)
        for s in range(0, len(order), 2):
            batch = order[s:s + 2]
            dv, df = union_batch_graphs([ds[i] for i in batch])
            flat.bucket.zero()
            vp, npred, _ = net((dv.shallow_copy(), df.shallow_copy()))
            lv, ln = batched_losses(vp, npred, dv, df, 'SCD', 'sided',
                                    sampling=dict(n=500, seed=opt.seed, draw=epoch, stream_ids=[int(i) for i in batch]))
            loss, _ = add_regularisers(network.dual_loss(lv, ln, 1, 1), vp, dv, 0.5, 0)
            loss.backward()
            optimizer.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(flat.flat_param).all())
    assert torch.equal(got, flat.flat_param.detach())
    res, res2 = trainer.evaluate(net, ds, opt), trainer.evaluate(net, ds, opt)
    assert res == res2 and all(np.isfinite(v) for v in res.values()) and res['eval_loss_v'] > 0


def _model(out):
    return torch.load(os.path.join(out, 'GeoBi-GNN_Synthetic_model.pth'), map_location='cpu', weights_only=True)


def test_train_command_with_scd_and_the_cd_path_beside_it(dev, tmp_path):
    """python -m geobi_gnn_amd train --loss_v SCD --loss_samples 500 --loss_n sided on a tiny split, two epochs, run twice:
    identical model files, loss_samples in the params file.  Then --loss_v CD twice, one epoch: that path is what it was
    and repeats itself (its own tests are tests/test_gpu_chamfer.py, untouched).  Child processes one after the other,
    the next only after the one before returned 0."""
    from geobi_gnn_amd import train_util
    data = str(tmp_path / 'Synthetic')
    _write_split(data, 'train', ('s1', 's2'), 5, (0.1, 0.3), seed0=700)
    _write_split(data, 'test', ('t1',), 5, (0.1,), seed0=800)
    runs = {}
    for name, extra in (('scd1', ('--loss_v', 'SCD', '--loss_samples', '500', '--max_epoch', '2')),
                        ('scd2', ('--loss_v', 'SCD', '--loss_samples', '500', '--max_epoch', '2')),
                        ('cd1', ('--loss_v', 'CD', '--max_epoch', '1')), ('cd2', ('--loss_v', 'CD', '--max_epoch', '1'))):
        out = str(tmp_path / name)
        run = _train_command(data, out, extra=('--no_predict', '--loss_n', 'sided') + extra)
        assert run.returncode == 0, run.stderr[-2000:]
        with open(os.path.join(out, 'GeoBi-GNN_Synthetic_params.json')) as fh:
            runs[name] = (_model(out), json.load(fh), open(os.path.join(out, 'training_info.txt')).read())
    for a, b in (('scd1', 'scd2'), ('cd1', 'cd2')):
        sa, sb = runs[a][0], runs[b][0]
        assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa), (a, b)
        assert all(bool(torch.isfinite(v).all()) for v in sa.values())
    assert runs['scd1'][1]['loss_v'] == 'SCD' and runs['scd1'][1]['loss_samples'] == 500
    assert runs['cd1'][1]['loss_v'] == 'CD' and runs['cd1'][1]['loss_samples'] == 10000
    assert any(not torch.equal(runs['scd1'][0][k], runs['cd1'][0][k]) for k in runs['scd1'][0])
    recs = [json.loads(ln) for ln in runs['scd1'][2].splitlines() if ln.startswith('{"epoch"')]
    assert [r['epoch'] for r in recs] == [0, 1, 2]
    assert all(np.isfinite(v) for r in recs for v in r.values() if isinstance(v, float))
    events = str(tmp_path / 'scd1' / 'train')
    tags = {t for f in os.listdir(events) if f.startswith('events') for _, t, _ in train_util.read_scalars(os.path.join(events, f))}
    assert tags == {'loss_v', 'loss_f', 'dual_loss', 'error_v', 'error_f'}       # the TensorBoard tags do not change
