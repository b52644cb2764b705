"""The training arena of the whole-network executor at its exact size (geobi_net_forward_train / geobi_net_backward /
geobi_net_train_groups, executor.py): the training forward reports the forward + backward need of a mesh, and an arena of
exactly that many bytes holds the step.

Bars: with the arena at the reported need the step runs without a retry and gives outputs, loss and every parameter
gradient BIT-identical to the step on a roomy arena and to the op-tape path; one alignment unit (256 bytes) less is
refused exactly once and the repeated step gives the same bits; a missing upstream gradient (NULL) gives the bits of an
explicit zero tensor."""
import pytest
import torch

import test_gpu_groups as G

pytestmark = pytest.mark.gpu

CASES = [(6, 'max', False), (9, 'mean', False), (8, 'max', True)]         # (mesh size, pooling, force_depth)
IDS = ['6-max', '9-mean', '8-max-depth']
_CACHE = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _step(net, dv, df, enabled):
    """One training step -> (verts, normals, loss, {name: gradient})."""
    from geobi_gnn_amd import network, executor
    was = executor.ENABLED
    executor.ENABLED = enabled
    try:
        net.zero_grad()
        vp, npred, _ = net((dv.shallow_copy(), df.shallow_copy()))
        loss = network.dual_loss(network.loss_v(vp, dv.y, 'L1'), network.loss_n(npred, df.y, 'L1'))
        loss.backward()
        torch.cuda.synchronize()
        return vp.detach().clone(), npred.detach().clone(), loss.item(), {k: p.grad.clone() for k, p in net.named_parameters()}
    finally:
        executor.ENABLED = was


def _same(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    assert a[3].keys() == b[3].keys()
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


def _case(dev, case):
    """Network, mesh, level-0 shape key, the op-tape step (the reference, computed once per case), the executor's step on
    its first, roomy arena and the need it reported."""
    if case not in _CACHE:
        from geobi_gnn_amd import network, meshgen, executor
        n, pool_type, force_depth = case
        torch.manual_seed(n)
        net = network.DualGNN(force_depth=force_depth, pool_type=pool_type).to(dev)
        dv, df = meshgen.synthetic_dual_data(n, 0.2, seed=n, data_type='Kinect_v1' if force_depth else 'Synthetic')
        dv, df = dv.to(dev), df.to(dev)
        lv_v, lv_f = executor._level0(dv, []), executor._level0(df, [])
        shape = (lv_v.N, lv_v.E, lv_f.N, lv_f.E)
        tape = _step(net, dv, df, False)
        executor._LEARNED.pop(shape, None)
        calls = executor.STATS['calls']
        roomy = _step(net, dv, df, True)
        assert executor.STATS['calls'] == calls + 1                    # the executor ran, not its fallback
        need = executor.STATS['train_need_bytes']
        assert 0 < need <= executor.STATS['train_arena_bytes']
        _same(roomy, tape)
        _CACHE[case] = (net, dv, df, shape, tape, roomy, need)
    return _CACHE[case]


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_the_reported_need_is_enough(dev, case):
    from geobi_gnn_amd import executor
    net, dv, df, shape, tape, roomy, need = _case(dev, case)
    before = dict(executor.STATS)
    try:
        executor._LEARNED[shape] = need
        exact = _step(net, dv, df, True)
    finally:
        executor._LEARNED.pop(shape, None)
    print('case %s: need %d bytes' % (case, need))
    assert executor.STATS['calls'] == before['calls'] + 1 and executor.STATS['fallback'] == before['fallback']
    assert executor.STATS['arena_retry'] == before['arena_retry']
    assert executor.STATS['train_arena_bytes'] == need and executor.STATS['train_need_bytes'] == need
    _same(exact, roomy)
    _same(exact, tape)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_one_alignment_unit_short_is_refused_once(dev, case):
    from geobi_gnn_amd import executor
    net, dv, df, shape, tape, roomy, need = _case(dev, case)
    before = dict(executor.STATS)
    try:
        executor._LEARNED[shape] = need - 256
        short = _step(net, dv, df, True)
    finally:
        executor._LEARNED.pop(shape, None)
    assert executor.STATS['calls'] == before['calls'] + 1 and executor.STATS['fallback'] == before['fallback']
    assert executor.STATS['arena_retry'] == before['arena_retry'] + 1
    assert executor.STATS['train_need_bytes'] == need and executor.STATS['train_arena_bytes'] > need
    _same(short, roomy)
    _same(short, tape)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_a_missing_upstream_gradient_is_a_zero_gradient(dev, case):
    """The library's zeros buffer: autograd always materialises a zero gradient, so only a direct call passes NULL.  The
    arena is at its exact size, and the run with the explicit zeros goes first: the block the allocator hands back for the
    NULL run then holds that run's gradients, not fresh memory."""
    from geobi_gnn_amd import executor
    net, dv, df, shape, _, _, need = _case(dev, case)
    params = list(net.parameters())
    gen = torch.Generator(device='cpu').manual_seed(17)
    g_v = torch.randn(dv.x.shape[0], 3, generator=gen).to(dev)
    g_n = torch.randn(df.x.shape[0], 3, generator=gen).to(dev)

    def run(gv, gn):
        try:
            executor._LEARNED[shape] = need
            _, _, rec = executor.forward_train(net, dv.shallow_copy(), df.shallow_copy())
        finally:
            executor._LEARNED.pop(shape, None)
        assert executor.STATS['train_arena_bytes'] == need
        grads = executor.backward(rec, gv, gn, params)
        torch.cuda.synchronize()
        rec.release()
        assert all(g is not None for g in grads)
        return [g.clone() for g in grads]

    retries = executor.STATS['arena_retry']
    for gv, gn in ((g_v, None), (None, g_n)):
        explicit = run(torch.zeros_like(g_v) if gv is None else gv, torch.zeros_like(g_n) if gn is None else gn)
        missing = run(gv, gn)
        assert any(bool(g.abs().max() > 0) for g in explicit)
        for p, a, b in zip(params, missing, explicit):
            assert torch.equal(a, b)
    assert executor.STATS['arena_retry'] == retries


def test_groups_at_their_reported_need(dev):
    """Two groups of different level-0 shapes, each on an arena of exactly the bytes it reported; then one of them 256
    bytes short."""
    from geobi_gnn_amd import executor
    net, bucket, pairs = G._setup(dev, freq=12)
    groups = [G._union(pairs, [0, 1, 2], dev), G._union(pairs, [3], dev)]
    tg = executor.TrainGroups(net, bucket).set_groups(groups)
    shapes = [pr['shape'] for pr in tg._prep]
    assert shapes[0] != shapes[1]                                     # the learned sizes are kept per shape
    for s in shapes:
        executor._LEARNED_GROUP.pop(s, None)
    tg.step(); torch.cuda.synchronize()
    assert tg.sequential_steps == 0
    g_ref, l_ref = bucket.flat.clone(), tg.losses.clone()
    used = [int(pr['out'].used_bytes) for pr in tg._prep]
    print('groups: need %s bytes' % used)

    def step_on(sizes):
        for pr, size in zip(tg._prep, sizes):
            pr['res']['arena'] = None
            executor._LEARNED_GROUP[pr['shape']] = size
        retries = executor.STATS['arena_retry']
        tg.step(); torch.cuda.synchronize()
        assert tg.sequential_steps == 0
        assert torch.equal(bucket.flat, g_ref) and torch.equal(tg.losses, l_ref)
        assert [int(pr['out'].used_bytes) for pr in tg._prep] == used
        return executor.STATS['arena_retry'] - retries

    try:
        assert step_on(used) == 0
        assert [pr['res']['arena'].numel() for pr in tg._prep] == used
        for k in range(2):
            sizes = list(used)
            sizes[k] -= 256
            assert step_on(sizes) == 1
            assert tg._prep[1 - k]['res']['arena'].numel() == used[1 - k]         # the other group kept its arena
    finally:
        for s in shapes:
            executor._LEARNED_GROUP.pop(s, None)
