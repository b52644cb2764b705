"""Training from OBJ folders on the device: the per-mesh rotation kernel (geobi_rotate_parts) against fp64, the
resident dataset (dataset.DualDataset: unsplit, split and filtered, cached), the package loop (trainer.train_epoch)
against a loop written out here, and the `train` command end to end."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from train_cases import _assert_same_sample, _epoch, _options, _train_command, _write_split

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                  # unit roundoff of fp32


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------ rotation kernel
def _rotations(count, seed):
    from geobi_gnn_amd.data import RandomRotate
    return RandomRotate(z_rotated=False, rng=np.random.default_rng(seed)).matrices(count)


def _rotate_parts(ptr, mats64, x, x_triples, y, dd, n=None):
    from geobi_gnn_amd import _lib as L
    m32 = np.ascontiguousarray(np.asarray(mats64, dtype=np.float64).reshape(-1, 9).astype(np.float32))
    arr = (ctypes.c_int64 * len(ptr))(*ptr)
    L.call('geobi_rotate_parts', ctypes.cast(arr, ctypes.c_void_p), len(ptr) - 1, m32.ctypes.data, L.ptr(x), x.shape[1],
           x_triples, L.ptr(y), L.ptr(dd), ptr[-1] if n is None else n, L.stream())
    torch.cuda.synchronize()


def _check_triples(got, before, ptr, mats64, what):
    """Every output component within 5 u (|a| + |b| + |c|) of float64(in) @ R64: matrix entries are at most 1 in magnitude and
    rounded once to fp32, each of the three terms passes at most four roundings (entry, product, two sums) = 4 u, the fifth
    u absorbs second-order terms; fused or unfused multiply-add both fit."""
    got, before = got.cpu().numpy().astype(np.float64), before.cpu().numpy().astype(np.float64)
    worst = 0.0
    for p in range(len(ptr) - 1):
        a, b = ptr[p], ptr[p + 1]
        if a == b:
            continue
        want = before[a:b] @ mats64[p]
        bar = 5 * U * np.abs(before[a:b]).sum(1, keepdims=True)
        err = np.abs(got[a:b] - want)
        worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
        assert (err <= bar).all(), (what, p, float((err / np.maximum(bar, 1e-300)).max()))
    print('%s: worst error / bar = %.3f' % (what, worst))


@pytest.mark.parametrize('with_targets', [True, False])
def test_rotate_parts_against_fp64(dev, with_targets):
    """Three parts of different sizes, one of them empty, three different full rotations, ldx = 6, with and without y / dd.
    Rows beyond n and arrays that were not handed over stay bit-unchanged."""
    ptr = [0, 700, 700, 2011]
    n, tail = ptr[-1], 37
    mats = _rotations(3, seed=5)
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(n + tail, 6, generator=g) * 3).to(dev)
    y = torch.randn(n + tail, 3, generator=g).to(dev)
    dd = torch.nn.functional.normalize(torch.randn(n + tail, 3, generator=g), dim=1).to(dev)
    x0, y0, dd0 = x.clone(), y.clone(), dd.clone()
    _rotate_parts(ptr, mats, x, 2, y if with_targets else None, dd if with_targets else None)
    _check_triples(x[:n, 0:3], x0[:n, 0:3], ptr, mats, 'x[:, 0:3]')
    _check_triples(x[:n, 3:6], x0[:n, 3:6], ptr, mats, 'x[:, 3:6]')
    assert not torch.equal(x[:n], x0[:n])
    assert torch.equal(x[n:], x0[n:])
    if with_targets:
        _check_triples(y[:n], y0[:n], ptr, mats, 'y')
        _check_triples(dd[:n], dd0[:n], ptr, mats, 'dd')
        assert torch.equal(y[n:], y0[n:]) and torch.equal(dd[n:], dd0[n:])
    else:
        assert torch.equal(y, y0) and torch.equal(dd, dd0)


def test_rotate_parts_leaves_other_columns_alone(dev):
    """ldx = 9 with one and with two turned triples: the columns behind them are bit-unchanged."""
    ptr = [0, 300, 1000]
    mats = _rotations(2, seed=6)
    g = torch.Generator().manual_seed(2)
    for triples in (1, 2):
        x = torch.randn(1000, 9, generator=g).to(dev)
        x0 = x.clone()
        _rotate_parts(ptr, mats, x, triples, None, None)
        for t in range(triples):
            _check_triples(x[:, 3 * t:3 * t + 3], x0[:, 3 * t:3 * t + 3], ptr, mats, 'triple %d of %d' % (t, triples))
        assert torch.equal(x[:, 3 * triples:], x0[:, 3 * triples:])
        assert not torch.equal(x[:, :3 * triples], x0[:, :3 * triples])


def test_rotate_parts_forty_parts_take_two_launches(dev):
    """More than 32 parts: the entry point chunks them; every part still gets its own matrix (parts of uneven size, a few
    empty, the chunk boundary inside the run)."""
    rng = np.random.default_rng(3)
    sizes = rng.integers(1, 90, size=40)
    sizes[[4, 31, 32]] = 0
    ptr = [0] + np.cumsum(sizes).tolist()
    mats = _rotations(40, seed=7)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(ptr[-1], 6, generator=g).to(dev)
    y = torch.randn(ptr[-1], 3, generator=g).to(dev)
    x0, y0 = x.clone(), y.clone()
    _rotate_parts(ptr, mats, x, 2, y, None)
    _check_triples(x[:, 0:3], x0[:, 0:3], ptr, mats, 'x[:, 0:3]')
    _check_triples(x[:, 3:6], x0[:, 3:6], ptr, mats, 'x[:, 3:6]')
    _check_triples(y, y0, ptr, mats, 'y')


def test_rotate_parts_identity_changes_nothing(dev):
    ptr = [0, 129, 129, 640]
    g = torch.Generator().manual_seed(4)
    x = torch.randn(640, 6, generator=g).to(dev)
    y = torch.randn(640, 3, generator=g).to(dev)
    x0, y0 = x.clone(), y.clone()
    _rotate_parts(ptr, np.stack([np.eye(3)] * 3), x, 2, y, None)
    assert torch.equal(x, x0) and torch.equal(y, y0)


def test_rotate_union_turns_every_mesh_by_its_own_matrix(dev):
    """data.rotate_union on a union batch of three meshes: both graphs, x[:, 0:3], x[:, 3:6] and y, parts from mesh_ptr;
    a pair without mesh_ptr is one part."""
    from geobi_gnn_amd import meshgen, meshprep
    from geobi_gnn_amd.data import rotate_union, union_batch_graphs
    parts = []
    for i, n in enumerate((5, 3, 6)):
        noisy, clean, faces = meshgen.noisy_icosphere(n, 0.2, seed=20 + i)
        parts.append(meshprep.build_dual_data(noisy, faces, clean, device=dev))
    dv, df = union_batch_graphs(parts)
    mats = _rotations(3, seed=8)
    before = [(d.x.clone(), d.y.clone(), d.edge_weight.clone()) for d in (dv, df)]
    rotate_union(dv, df, mats)
    torch.cuda.synchronize()
    for d, (x0, y0, w0) in zip((dv, df), before):
        ptr = d.mesh_ptr.tolist()
        _check_triples(d.x[:, 0:3], x0[:, 0:3], ptr, mats, 'x pos')
        _check_triples(d.x[:, 3:6], x0[:, 3:6], ptr, mats, 'x normal')
        _check_triples(d.y, y0, ptr, mats, 'y')
        assert torch.equal(d.edge_weight, w0)
    with pytest.raises(ValueError):
        rotate_union(dv, df, mats[:2])
    sv, sf = parts[0][0].clone(), parts[0][1].clone()
    x0 = sv.x.clone()
    rotate_union(sv, sf, mats[1:2])
    torch.cuda.synchronize()
    _check_triples(sv.x[:, 0:3], x0[:, 0:3], [0, x0.shape[0]], mats[1:2], 'single pair')


# ------------------------------------------------------------------------------------------------ dataset
def test_dataset_unsplit_fresh_cached_and_uncached(dev, tmp_path):
    """Two names x two noise files, every mesh below the patch size: each sample is bit-identical to a direct
    meshprep.build_dual_data on the arrays read back from its files; a second construction loads processed_data/ (file
    mtimes unchanged) and yields the same x, y, CSR arrays and CSR-ordered weights -- and one train_epoch over it leaves
    the flat parameters bit-identical to one over the freshly built dataset; cache=False leaves no folder behind."""
    from geobi_gnn_amd import meshio, meshprep
    from geobi_gnn_amd.dataset import DualDataset
    root = str(tmp_path / 'cached')
    files = _write_split(root, 'train', ('ball', 'ball2'), 6, (0.1, 0.3), seed0=300)
    fresh = DualDataset(root, 'train', device=dev)
    assert fresh.names == ['ball_n1', 'ball_n2', 'ball2_n1', 'ball2_n2'] and fresh.skipped == 0      # `ball` does not take `ball2`'s
    want = {}
    for name, (noisy_file, original_file) in files.items():
        pts, faces = meshio.read_obj(noisy_file)
        gt, _ = meshio.read_obj(original_file)
        want[name] = meshprep.build_dual_data(pts, faces, points_gt=gt, device=dev)
    for i, name in enumerate(fresh.names):
        _assert_same_sample(fresh[i], want[name])
        assert fresh[i][0].graph().pos_in is not None and fresh[i][1].graph().pos_in is not None     # built once, resident
        assert fresh[i][1].fv_indices._geobi_fv[1].index is not None
    pt = sorted(os.listdir(os.path.join(root, 'train', 'processed_data')))
    assert pt == [n + '.pt' for n in sorted(files)]
    mtimes = [os.stat(os.path.join(root, 'train', 'processed_data', f)).st_mtime_ns for f in pt]

    loaded = DualDataset(root, 'train', device=dev)
    assert [os.stat(os.path.join(root, 'train', 'processed_data', f)).st_mtime_ns for f in pt] == mtimes
    assert loaded.names == fresh.names
    for i in range(len(loaded)):
        _assert_same_sample(loaded[i], fresh[i], edge_weight_as_stored=False)
        assert getattr(loaded[i][1].fv_indices, '_geobi_fv', None) is not None       # range-checked once, re-marked
    opt = _options(batch_size=2)
    assert torch.equal(_epoch(fresh, dev, opt), _epoch(loaded, dev, opt))

    root2 = str(tmp_path / 'uncached')
    _write_split(root2, 'train', ('ball',), 6, (0.2,), seed0=400)
    plain = DualDataset(root2, 'train', device=dev, cache=False)
    assert len(plain) == 1 and not os.path.exists(os.path.join(root2, 'train', 'processed_data'))


def _two_component_mesh():
    """A noisy frequency-16 icosphere (5 120 faces) and, far away, a frequency-1 icosphere (20 faces) scaled by 0.2 at
    x = 3.  Under the reference's growth rule with submesh_size 2000 the far component is the first seed and the only
    patch below filter_patch_count = 100 (sizes [20, 2000, 2000, ...]); the test asserts what it needs of that itself."""
    from geobi_gnn_amd import meshgen
    noisy, clean, faces = meshgen.noisy_icosphere(16, 0.2, seed=77)
    small, small_faces = meshgen.icosphere(1)
    small = (np.asarray(small, dtype=np.float64) * 0.2 + np.array([3.0, 0.0, 0.0])).astype(np.float32)
    V = noisy.shape[0]
    all_faces = np.concatenate([np.asarray(faces), np.asarray(small_faces) + V]).astype(np.int32)
    return np.concatenate([noisy, small]).astype(np.float32), np.concatenate([clean, small]).astype(np.float32), all_faces


def test_dataset_split_and_filtered(dev, tmp_path):
    from geobi_gnn_amd import meshio, meshprep, patches
    from geobi_gnn_amd.dataset import DualDataset
    root = str(tmp_path)
    for sub in ('original', 'noisy'):
        os.makedirs(os.path.join(root, 'train', sub))
    noisy, clean, faces = _two_component_mesh()
    meshio.write_obj(os.path.join(root, 'train', 'noisy', 'pair_n1.obj'), noisy, faces)
    meshio.write_obj(os.path.join(root, 'train', 'original', 'pair.obj'), clean, faces)
    sub_size, min_faces = 2000, 100

    # by hand, from the arrays read back: the whole noisy mesh's centroid and scale as patches.predict_mesh forms them
    pts_h, fv_h = meshio.read_obj(os.path.join(root, 'train', 'noisy', 'pair_n1.obj'))
    gt_h, _ = meshio.read_obj(os.path.join(root, 'train', 'original', 'pair.obj'))
    pts, gt, fv = torch.from_numpy(pts_h).to(dev), torch.from_numpy(gt_h).to(dev), torch.from_numpy(fv_h).to(dev)
    V = pts.shape[0]
    rowptr, lst = meshprep.vertex_faces(fv, V)
    g_v = meshprep.ring_graph(0, fv, rowptr, lst, V)
    centroid = pts.mean(0, keepdim=True)
    scale = float(1.0 / torch.tensor(meshprep.mean_edge_length(pts, g_v).tolist()[0], dtype=torch.float32))
    grown = [(sel.clone(), v_idx.clone(), f_sub.clone())
             for sel, v_idx, f_sub in patches.split_patches(pts, fv, sub_size, incidence=(rowptr, lst))]
    sizes = [int(sel.shape[0]) for sel, _, _ in grown]
    print('patch sizes', sizes)
    kept = [p for p in grown if p[0].shape[0] > min_faces]
    assert len(grown) - len(kept) >= 1 and len(kept) >= 3                # preconditions: something dropped, enough kept

    ds = DualDataset(root, 'train', submesh_size=sub_size, filter_patch_count=min_faces, device=dev)
    assert len(ds) == len(kept)
    assert ds.names == ['pair_n1-sub%d-%d' % (sub_size, int(sel[0])) for sel, _, _ in kept]
    for i, (sel, v_idx, f_sub) in enumerate(kept):
        idx = v_idx.long()
        want = meshprep.build_dual_data(pts[idx], f_sub, points_gt=gt[idx], centroid=centroid, scale=scale, device=dev)
        _assert_same_sample(ds[i], want)
        assert torch.equal(ds[i][0].y, (gt[idx] - centroid) * scale)     # the original's points, the noisy mesh's normalisation
    cached = sorted(os.listdir(os.path.join(root, 'train', 'processed_data')))
    assert cached == sorted(n + '.pt' for n in ds.names)
    for sel, _, _ in grown:
        if sel.shape[0] <= min_faces:
            assert 'pair_n1-sub%d-%d.pt' % (sub_size, int(sel[0])) not in cached
    # from the cache: same names (the growth still runs), same samples
    again = DualDataset(root, 'train', submesh_size=sub_size, filter_patch_count=min_faces, device=dev)
    assert again.names == ds.names
    for i in range(len(ds)):
        _assert_same_sample(again[i], ds[i], edge_weight_as_stored=False)


# ------------------------------------------------------------------------------------------------ loop
def test_train_epoch_equals_the_loop_written_out(dev, tmp_path):
    """6 samples, batch 2, no rotation, two epochs: trainer.train_epoch leaves the flat parameters bit-identical to the
    public pieces called one after the other in the same shard_indices order."""
    from geobi_gnn_amd import network, train_util
    from geobi_gnn_amd.data import union_batch_graphs
    from geobi_gnn_amd.dataset import DualDataset
    from geobi_gnn_amd.parallel import FlatParameters, batched_losses, shard_indices
    root = str(tmp_path)
    _write_split(root, 'train', ('a', 'b', 'c'), 5, (0.1, 0.3), seed0=500)
    ds = DualDataset(root, 'train', device=dev, cache=False)
    assert len(ds) == 6
    opt = _options(batch_size=2)
    got = _epoch(ds, dev, opt, epochs=2)

    torch.manual_seed(11)
    net = network.DualGNN().to(dev)
    flat = FlatParameters(net)
    optimizer = train_util.make_optimizer(opt, flat.parameters(), fused=True)
    start = flat.flat_param.detach().clone()
    for epoch in (1, 2):
        net.train()
        order = shard_indices(len(ds), 0, 1, seed=opt.seed, epoch=epoch)
        for s in range(0, len(order), 2):
            dv, df = union_batch_graphs([ds[i] for i in order[s:s + 2]])
            flat.bucket.zero()
            vp, npred, _ = net((dv.shallow_copy(), df.shallow_copy()))
            lv, ln = batched_losses(vp, npred, dv, df, opt.loss_v, opt.loss_n)
            network.dual_loss(lv, ln, opt.loss_v_scale, opt.loss_n_scale).backward()
            optimizer.step()
    torch.cuda.synchronize()
    assert not torch.equal(start, flat.flat_param.detach())
    assert torch.equal(got, flat.flat_param.detach())


def test_short_last_batch_steps_and_samples_are_never_written(dev, tmp_path):
    """5 samples, batch 2 (the last batch is one sample and still steps), full per-sample rotation: the rotation changes
    the result, the same seed repeats it bit for bit, and afterwards every resident sample still equals a fresh build."""
    from geobi_gnn_amd import meshio, meshprep, trainer
    from geobi_gnn_amd.dataset import DualDataset
    root = str(tmp_path)
    files = _write_split(root, 'train', ('a', 'b', 'c', 'd', 'e'), 4, (0.2,), seed0=600)
    ds = DualDataset(root, 'train', device=dev, cache=False)
    assert len(ds) == 5
    opt = _options(batch_size=2)
    plain = _epoch(ds, dev, opt)
    turned = _epoch(ds, dev, opt, rotate=trainer.make_rotation('full', opt.seed))
    again = _epoch(ds, dev, opt, rotate=trainer.make_rotation('full', opt.seed))
    assert torch.equal(turned, again) and not torch.equal(turned, plain)
    four = _epoch([ds[i] for i in range(4)], dev, opt)
    assert not torch.equal(four, plain)
    for i, name in enumerate(ds.names):
        pts, faces = meshio.read_obj(files[name][0])
        gt, _ = meshio.read_obj(files[name][1])
        _assert_same_sample(ds[i], meshprep.build_dual_data(pts, faces, points_gt=gt, device=dev))


# ------------------------------------------------------------------------------------------------ command
def test_train_command_end_to_end(dev, tmp_path):
    """python -m geobi_gnn_amd train on frequency-8 icospheres (6 train files, 2 test files), 5 epochs, batch 2: exit
    status, model, params, log, event files, denoised test meshes; a second run with the same seed gives the same state
    dict bit for bit; the best evaluation normal error is below that of the net before any step.  Two child processes,
    the second only after the first returned 0."""
    from geobi_gnn_amd import network, train_util
    data = str(tmp_path / 'Synthetic')
    _write_split(data, 'train', ('s1', 's2', 's3'), 8, (0.1, 0.3), seed0=700)
    _write_split(data, 'test', ('t1',), 8, (0.1, 0.3), seed0=800)
    out = str(tmp_path / 'run1')
    run = _train_command(data, out)
    assert run.returncode == 0, run.stderr[-2000:]

    model_file = os.path.join(out, 'GeoBi-GNN_Synthetic_model.pth')
    sd = torch.load(model_file, map_location='cpu', weights_only=True)
    net = network.DualGNN()
    net.load_state_dict(sd, strict=True)
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
    with open(os.path.join(out, 'GeoBi-GNN_Synthetic_params.json')) as fh:
        params = json.load(fh)
    assert params['seed'] == 31 and params['batch_size'] == 2 and params['sub_size'] == 20000 and params['rotate'] == 'full'
    assert params['force_depth'] is False

    log = open(os.path.join(out, 'training_info.txt')).read()
    recs = [json.loads(ln) for ln in log.splitlines() if ln.startswith('{"epoch"')]
    assert [r['epoch'] for r in recs] == [0, 1, 2, 3, 4, 5]                 # the untrained net, then one line per epoch
    assert all(ln in run.stdout for ln in log.splitlines())                # a copy of what was printed
    before, best = recs[0]['eval_error_f_deg'], min(r['eval_error_f_deg'] for r in recs[1:])
    print('evaluation normal error: before any step %.6f, best of 5 epochs %.6f' % (before, best))
    assert any(r['saved'] for r in recs[1:])

    train_events = [f for f in os.listdir(os.path.join(out, 'train')) if f.startswith('events.out.tfevents')]
    test_events = [f for f in os.listdir(os.path.join(out, 'test')) if f.startswith('events.out.tfevents')]
    assert len(train_events) == 1 and len(test_events) == 1
    tr = train_util.read_scalars(os.path.join(out, 'train', train_events[0]))
    te = train_util.read_scalars(os.path.join(out, 'test', test_events[0]))
    steps = sorted({s for s, _, _ in tr})
    assert steps == list(range(2, 31, 2))                                  # 3 steps of 2 samples per epoch, 5 epochs
    for s in steps:
        assert sorted(t for s2, t, _ in tr if s2 == s) == ['dual_loss', 'error_f', 'error_v', 'loss_f', 'loss_v']
    assert sorted({s for s, _, _ in te}) == [6, 12, 18, 24, 30]
    for s in (6, 12, 18, 24, 30):
        assert sorted(t for s2, t, _ in te if s2 == s) == ['error_f', 'error_v', 'loss_f', 'loss_v']

    results = sorted(os.listdir(os.path.join(out, 'result')))
    assert [f for f in results if f.endswith('.obj')] == ['t1_n1-60.obj', 't1_n2-60.obj']

    out2 = str(tmp_path / 'run2')
    run2 = _train_command(data, out2, extra=('--no_predict',))
    assert run2.returncode == 0, run2.stderr[-2000:]
    assert not os.path.exists(os.path.join(out2, 'result'))
    sd2 = torch.load(os.path.join(out2, 'GeoBi-GNN_Synthetic_model.pth'), map_location='cpu', weights_only=True)
    assert list(sd2) == list(sd)
    for k in sd:
        assert torch.equal(sd[k], sd2[k]), k
    # expected, not measured when the check was set: training for 15 steps beats the seed-initialised net (no margin)
    assert best < before, (best, before)
