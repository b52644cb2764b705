"""Mesh regularisers on the MI355X (csrc/reg.hip: geobi_mesh_reg_fwd / _bwd behind ops.mesh_reg) against the fp64
statements of tests/reg_model.py evaluated on the same fp32 inputs; the functions of network and parallel on top of them;
one training epoch and the ``train`` command with ``--loss_lap_scale`` / ``--loss_edge_scale``.

Inputs: meshgen.noisy_icosphere(n, s, seed=5) as prediction, its clean sphere as target, (n, s) = (2, 0.5), (8, 0.5),
(24, 0.3) -- V = 42 (less than one block), 642, 5762 -- both turned by a fixed rotation: an unrotated icosphere has vertex
normals with components that are exactly 0, and the sign of a projected Laplacian component would be a coin toss there.

Values: |got - fp64| <= TOL * |fp64|.  Gradients: max |got - fp64| over the compared rows <= TOL * the largest fp64
gradient entry.  The Laplacian term's gradient is a sum of signs: a vertex is left out of ITS comparison if it, or a
neighbour, has a component of d = lap(vp) - lap(v) with fp64 magnitude below 1e-5 max |d| (fp32 does not decide that sign);
at most 2 % of the vertices may be left out, and the count is printed.  On these inputs it is between 0 and 21 vertices
(tests/test_reg_model_host.py prints them on the CPU)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import reg_model as M
from geom_model import unit_depth
from train_cases import _epoch, _options, _train_command, _write_split

pytestmark = pytest.mark.gpu

TOL = 1e-5                      # the project's bar (tests/test_gpu_kernels.py)
INPUTS = ((2, 0.5), (8, 0.5), (24, 0.3))
LEFT_OUT = 0.02


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------ shared inputs
class Case(object):
    """One mesh pair on the host with its entries; the fp64 reference per (projected, weights) is computed once."""

    def __init__(self, vp, v, normal, faces):
        self.vp, self.v, self.normal, self.faces = vp, v, normal, np.asarray(faces)
        self.V = vp.shape[0]
        self.row, self.col = M.entries(self.faces, self.V)
        self._ref, self._graph = {}, None

    def ref(self, projected=False):
        if projected not in self._ref:
            self._ref[projected] = M.both(self.vp, self.v, self.row, self.col, self.normal if projected else None)
        return self._ref[projected]

    def graph(self, dev):
        from geobi_gnn_amd.graph import Graph
        if self._graph is None:
            self._graph = Graph.from_edge_index(M.edge_index(self.faces, self.V).to(dev), self.V)
            assert self._graph.symmetric is True and self._graph.E == self.row.numel()
            assert torch.equal(self._graph.col_out.cpu().long(), self.col)
        return self._graph


@functools.lru_cache(maxsize=None)
def _sphere(k, shift=None):
    return Case(*M.sphere_input(*INPUTS[k], shift=shift))


@functools.lru_cache(maxsize=None)
def _fan():
    """fan(200): a hub of valence 200, a rim, and a last vertex that no face uses (deg = 0); prediction: the fan jittered
    by 0.05, normals: random unit vectors.  Checked in fp64 on the CPU: the only vertex within the sign threshold is the one
    without edges (d = 0 exactly, sign 0 on both sides), so 1 of 202 is left out, plain and projected."""
    pts, faces = M.fan(200)
    rng = np.random.default_rng(9)
    vp = (pts.numpy() + 0.05 * rng.standard_normal(pts.shape)).astype(np.float32)
    return Case(torch.from_numpy(vp), pts.float(), unit_depth(pts.shape[0], seed=5).float(), faces.numpy())


def _run(dev, case, projected=False, terms=3, vp=None, w_lap=None, w_edge=None):
    """-> (L_lap, L_edge, grad of L_lap, grad of L_edge) through ops.mesh_reg; a term that is off has no gradient (None)."""
    from geobi_gnn_amd import ops
    p = (case.vp if vp is None else vp).to(dev).requires_grad_(True)
    normal = case.normal.to(dev) if projected else None
    a, b = ops.mesh_reg(p, case.v.to(dev), case.graph(dev), normal, w_lap, w_edge, terms)
    ga = torch.autograd.grad(a, p, retain_graph=True)[0] if terms & 1 else None
    gb = torch.autograd.grad(b, p, retain_graph=True)[0] if terms & 2 else None
    return a.detach(), b.detach(), ga, gb


def _assert_value(got, ref, what):
    print('%s: %.9g (fp64 %.9g), rel err %.3g' % (what, float(got), ref, abs(float(got) - ref) / abs(ref)))
    assert abs(float(got) - ref) <= TOL * abs(ref), what


def _assert_grad(got, ref, what, left_out=None):
    got = got.cpu().double()
    keep = torch.ones(ref.shape[0], dtype=torch.bool) if left_out is None else ~left_out
    n_out = int((~keep).sum())
    err = float((got - ref)[keep].abs().max() / ref.abs().max())
    print('%s: %d rows, %d left out, rel err %.3g' % (what, ref.shape[0], n_out, err))
    assert n_out <= LEFT_OUT * ref.shape[0], what
    assert bool(torch.isfinite(got).all()) and err <= TOL, what


def _check(dev, case, projected, what, **kw):
    r_lap, r_edge, rg_lap, rg_edge, d = case.ref(projected) if not kw else M.both(
        kw.get('vp', case.vp), case.v, case.row, case.col, case.normal if projected else None)
    a, b, ga, gb = _run(dev, case, projected, **kw)
    _assert_value(a, r_lap, what + ' L_lap')
    _assert_value(b, r_edge, what + ' L_edge')
    _assert_grad(ga, rg_lap, what + ' grad L_lap', M.undecided(d, case.row, case.col))
    _assert_grad(gb, rg_edge, what + ' grad L_edge')
    return a, b, ga, gb


# ------------------------------------------------------------------------------------------------ 1. values, gradients
@pytest.mark.parametrize('projected', [False, True], ids=['plain', 'projected'])
@pytest.mark.parametrize('k', [0, 1, 2])
def test_values_and_gradients_match_fp64(dev, k, projected):
    """Both terms and both gradients from one forward; the gradient of a weighted sum of the two outputs (one backward
    launch with both terms) is that sum of the two gradients."""
    from geobi_gnn_amd import ops
    case = _sphere(k)
    a, b, ga, gb = _check(dev, case, projected, 'n = %d' % INPUTS[k][0])
    p = case.vp.to(dev).requires_grad_(True)
    la, lb = ops.mesh_reg(p, case.v.to(dev), case.graph(dev), case.normal.to(dev) if projected else None)
    assert torch.equal(la.detach(), a) and torch.equal(lb.detach(), b)
    (0.75 * la + 1.5 * lb).backward()
    want = 0.75 * ga.double() + 1.5 * gb.double()
    assert float((p.grad.double() - want).abs().max()) <= 1e-6 * float(want.abs().max())


def test_more_rows_than_the_forward_grid_holds(dev):
    """23 copies of the n = 24 pair, copy k scaled by 1 + k / 64, as ONE mesh of 132 526 vertices: more than the 512 blocks
    of 256 rows the forward launches, so the first 1 454 threads walk a second row.  One forward, both values.  At this
    size the workspace (512 pairs of block sums) is large enough to be handed over 512 bytes short: the launcher refuses."""
    from geobi_gnn_amd import _lib as L, ops
    from geobi_gnn_amd.graph import Graph
    base = _sphere(2)
    copies = 23
    scale = lambda t: torch.cat([(t.double() * (1 + k / 64.0)).float() for k in range(copies)])
    vp, v = scale(base.vp), scale(base.v)
    V = vp.shape[0]
    assert V > 512 * 256
    off = (torch.arange(copies) * base.V).repeat_interleave(base.row.numel())
    row, col = base.row.repeat(copies) + off, base.col.repeat(copies) + off
    g = Graph.from_edge_index(torch.stack([row, col]).to(dev), V)
    assert g.symmetric is True and g.E == row.numel()
    ref_lap, ref_edge = float(M.laplacian_term(vp.double(), v.double(), row, col)), float(M.edge_term(vp.double(), v.double(), row, col))
    a, b = ops.mesh_reg(vp.to(dev), v.to(dev), g)
    _assert_value(a, ref_lap, 'V = %d L_lap' % V)
    _assert_value(b, ref_edge, 'V = %d L_edge' % V)
    nbytes = L.size_query('geobi_mesh_reg_ws_bytes', V)
    assert nbytes == 2 * 8 * 512 + 256
    p, t, out, u = vp.to(dev), v.to(dev), torch.empty(2, device=dev), torch.empty((V, 3), device=dev)
    ws = L.workspace(nbytes, dev)
    with pytest.raises(L.GeobiError, match=r'mesh_reg_fwd: workspace too small \(%d bytes given, %d needed\)' % (nbytes - 512, nbytes - 256)):
        L.call('geobi_mesh_reg_fwd', L.ptr(p), L.ptr(t), None, L.ptr(g.rowptr_out), L.ptr(g.col_out), V, g.E, None, None, 3,
               L.ptr(out), L.ptr(u), L.ptr(ws), nbytes - 512, L.stream())


# ------------------------------------------------------------------------------------------------ 2. edges
def test_identical_meshes_give_exact_zeros(dev):
    """vp == v bit for bit: both values are 0.0 and every gradient entry is zero, plain and projected."""
    case = _sphere(1)
    for projected in (False, True):
        a, b, ga, gb = _run(dev, case, projected, vp=case.v.clone())
        assert float(a) == 0.0 and float(b) == 0.0
        assert int(torch.count_nonzero(ga)) == 0 and int(torch.count_nonzero(gb)) == 0


@pytest.mark.parametrize('projected', [False, True], ids=['plain', 'projected'])
def test_hub_of_valence_200_and_a_vertex_without_edges(dev, projected):
    """fan(200): one row of 200 entries among rows of 3, and a last vertex with deg = 0, whose row is empty and ends at
    E: it adds nothing to either value and its gradient rows are exactly zero."""
    case = _fan()
    g = case.graph(dev)
    rp = g.rowptr_out.cpu()
    assert int(rp[1] - rp[0]) == 200 and int(rp[-1] - rp[-2]) == 0 and int(rp[-1]) == g.E
    a, b, ga, gb = _check(dev, case, projected, 'fan(200)')
    assert int(torch.count_nonzero(ga[-1])) == 0 and int(torch.count_nonzero(gb[-1])) == 0
    # the same mesh without its last vertex: the sums over rows are the same, the means differ by the vertex count
    from geobi_gnn_amd import ops
    from geobi_gnn_amd.graph import Graph
    V = case.V - 1
    g1 = Graph.from_edge_index(M.edge_index(case.faces, V).to(dev), V)
    a1, b1 = ops.mesh_reg(case.vp[:V].to(dev), case.v[:V].to(dev), g1, case.normal[:V].to(dev) if projected else None)
    assert abs(float(a1) * V - float(a) * case.V) <= 1e-6 * float(a) * case.V and float(b1) == float(b)


def test_coincident_predicted_vertices_have_a_finite_gradient(dev):
    """Two predicted vertices of one edge set equal: the entry counts in the value and adds no gradient, as in the model."""
    case = _sphere(0)
    vp = case.vp.clone()
    vp[int(case.col[0])] = vp[int(case.row[0])]
    _check(dev, case, False, 'coincident ends', vp=vp)


def test_far_from_the_origin(dev):
    """Both meshes moved by (100, -50, 25), ~170 edge lengths at n = 8: the sums are formed from coordinate differences, so
    the result still meets TOL against the model on the moved fp32 inputs."""
    case = _sphere(1, shift=(100.0, -50.0, 25.0))
    assert float(case.vp.abs().max()) > 99
    for projected in (False, True):
        _check(dev, case, projected, 'moved by (100, -50, 25)%s' % (' projected' if projected else ''))


# ------------------------------------------------------------------------------------------------ 3. union batch
def test_union_of_three_meshes_is_the_mean_of_the_three(dev):
    """The three inputs as one union batch with mesh_ptr, through parallel.batched_regularisers (per-mesh weights formed
    on the device) and through ops.mesh_reg with the model's weights: each value is the mean of the three single-mesh
    values, the gradient rows of part k are one third of the single-mesh gradient, to TOL; the values also match the
    fp64 model with the per-mesh weights."""
    from geobi_gnn_amd import ops, parallel
    from geobi_gnn_amd.data import Data
    cases = [_sphere(k) for k in range(3)]
    singles = [_run(dev, c) for c in cases]
    vp, faces, vptr, _ = M.union([(c.vp, torch.from_numpy(c.faces)) for c in cases])
    v = torch.cat([c.v for c in cases])
    V = vp.shape[0]
    row, col = M.entries(faces.numpy(), V)
    w_lap, w_edge = M.mesh_weights(vptr), M.edge_weights(row, vptr)
    ref_lap = float(M.laplacian_term(vp.double(), v.double(), row, col, None, w_lap))
    ref_edge = float(M.edge_term(vp.double(), v.double(), row, col, w_edge))

    def check(a, b, ga, gb, what):
        _assert_value(a, ref_lap, what + ' L_lap')
        _assert_value(b, ref_edge, what + ' L_edge')
        for k, (sa, sb, sga, sgb) in enumerate(singles):
            lo, hi = int(vptr[k]), int(vptr[k + 1])
            for got, single, name in ((ga, sga, 'lap'), (gb, sgb, 'edge')):
                err = float((got[lo:hi].double() - single.double() / 3).abs().max() / (single.double().abs().max() / 3))
                print('%s part %d grad %s: rel err %.3g' % (what, k, name, err))
                assert err <= TOL
        mean_a, mean_b = sum(float(s[0]) for s in singles) / 3, sum(float(s[1]) for s in singles) / 3
        assert abs(float(a) - mean_a) <= TOL * mean_a and abs(float(b) - mean_b) <= TOL * mean_b

    data = Data(vp.to(dev), M.edge_index(faces.numpy(), V).to(dev), y=v.to(dev))
    data.mesh_ptr = vptr
    p = data.x.clone().requires_grad_(True)
    a, b = parallel.batched_regularisers(p, data, True, True)
    ga, gb = torch.autograd.grad(a, p, retain_graph=True)[0], torch.autograd.grad(b, p)[0]
    check(a.detach(), b.detach(), ga, gb, 'batched_regularisers')
    assert torch.equal(data._edge_weights.cpu(), w_edge.float()) or float(
        (data._edge_weights.cpu().double() - w_edge).abs().max() / w_edge.max()) <= 1e-6
    only = parallel.batched_regularisers(p, data, False, True)
    assert only[0] is None and torch.equal(only[1].detach(), b.detach())

    g = data.graph()
    p2 = data.x.clone().requires_grad_(True)
    a2, b2 = ops.mesh_reg(p2, data.y, g, None, w_lap.float().to(dev), w_edge.float().to(dev))
    ga2, gb2 = torch.autograd.grad(a2, p2, retain_graph=True)[0], torch.autograd.grad(b2, p2)[0]
    check(a2.detach(), b2.detach(), ga2, gb2, 'mesh_reg with weights')


# ------------------------------------------------------------------------------------------------ 4. mask, determinism
def test_term_mask_and_bit_identical_repeats(dev):
    """With one term selected the other output is exactly 0 and takes no gradient: the gradient of a sum of both outputs
    is the selected term's alone, bit for bit what the two-term call gives for that term.  Two identical calls agree in
    every bit."""
    from geobi_gnn_amd import ops
    case = _sphere(2)
    a, b, ga, gb = _run(dev, case, True)
    again = _run(dev, case, True)
    for x, y in zip((a, b, ga, gb), again):
        assert torch.equal(x, y)
    for terms, keep_a, keep_b in ((ops.TERM_LAP, True, False), (ops.TERM_EDGE, False, True)):
        p = case.vp.to(dev).requires_grad_(True)
        la, lb = ops.mesh_reg(p, case.v.to(dev), case.graph(dev), case.normal.to(dev), terms=terms)
        assert torch.equal(la.detach(), a) if keep_a else float(la.detach()) == 0.0
        assert torch.equal(lb.detach(), b) if keep_b else float(lb.detach()) == 0.0
        (la + lb).backward()
        assert torch.equal(p.grad, ga if keep_a else gb)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(dev):
    from geobi_gnn_amd import _lib, ops
    from geobi_gnn_amd.graph import Graph
    case = _sphere(0)
    vp, v, g = case.vp.to(dev), case.v.to(dev), case.graph(dev)
    one_way = Graph.from_edge_index(torch.stack([case.row, case.col])[:, case.row < case.col].to(dev), case.V)
    assert one_way.symmetric is False
    with pytest.raises(_lib.GeobiError, match='symmetric'):
        ops.mesh_reg(vp, v, one_way)
    unknown = Graph.from_sorted(case.V, g.rowptr_out, g.ensure_rows(), g.col_out)       # nobody vouches for it
    with pytest.raises(_lib.GeobiError, match='symmetric'):
        ops.mesh_reg(vp, v, unknown)
    with pytest.raises(_lib.GeobiError, match=r'\[V, 3\]'):
        ops.mesh_reg(vp[:, :2], v[:, :2], g)
    with pytest.raises(_lib.GeobiError, match=r'\[V, 3\]'):
        ops.mesh_reg(vp, v[:-1], g)
    with pytest.raises(_lib.GeobiError, match='normal'):
        ops.mesh_reg(vp, v, g, case.normal[:-1].to(dev))
    with pytest.raises(_lib.GeobiError, match='w_edge'):
        ops.mesh_reg(vp, v, g, w_edge=torch.ones(case.V + 1, device=dev))
    with pytest.raises(_lib.GeobiError, match='nodes'):
        ops.mesh_reg(vp[:-1], v[:-1], g)
    with pytest.raises(_lib.GeobiError, match='terms'):
        ops.mesh_reg(vp, v, g, terms=0)
    with pytest.raises(_lib.GeobiError):
        ops.mesh_reg(vp.cpu(), v.cpu(), g)


# ------------------------------------------------------------------------------------------------ 6. surface
def test_network_functions_reach_the_kernel(dev):
    """network.laplacian_loss / edge_length_loss on device tensors, with the dataset's COO (self loops included): the
    kernel's values, i.e. the model's to TOL, with a gradient; the graph is cached on the edge_index tensor."""
    from geobi_gnn_amd import network
    case = _sphere(1)
    ei = M.edge_index(case.faces, case.V).to(dev)
    v = case.v.to(dev)
    for projected in (False, True):
        normal = case.normal.to(dev) if projected else None
        p = case.vp.to(dev).requires_grad_(True)
        lap = network.laplacian_loss(p, v, ei, normal)
        _assert_value(lap.detach(), case.ref(projected)[0], 'laplacian_loss')
        lap.backward()
        _assert_grad(p.grad, case.ref(projected)[2], 'laplacian_loss grad', M.undecided(case.ref(projected)[4], case.row, case.col))
    p = case.vp.to(dev).requires_grad_(True)
    edge = network.edge_length_loss(p, v, ei)
    _assert_value(edge.detach(), case.ref()[1], 'edge_length_loss')
    edge.backward()
    _assert_grad(p.grad, case.ref()[3], 'edge_length_loss grad')
    assert getattr(ei, '_geobi_graph', None) is not None


# ------------------------------------------------------------------------------------------------ 7. training
def test_train_epoch_with_regularisers(dev, tmp_path):
    """4 frequency-4 samples, batch 2, loss_v = CD, loss_n = sided, both scales 0.5: two runs leave bit-identical flat
    parameters, which differ from the run with both scales 0; that run is bit-identical to one whose options do not have
    the two attributes at all."""
    from geobi_gnn_amd.dataset import DualDataset
    root = str(tmp_path)
    _write_split(root, 'train', ('a', 'b'), 4, (0.1, 0.3), seed0=950)
    ds = DualDataset(root, 'train', device=dev, cache=False)
    assert len(ds) == 4
    kw = dict(batch_size=2, loss_v='CD', loss_n='sided')
    on = _options(loss_lap_scale=0.5, loss_edge_scale=0.5, **kw)
    got = _epoch(ds, dev, on)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, _epoch(ds, dev, on))
    off = _epoch(ds, dev, _options(loss_lap_scale=0, loss_edge_scale=0, **kw))
    assert not torch.equal(got, off)
    old = _options(**kw)
    del old.loss_lap_scale, old.loss_edge_scale
    assert torch.equal(off, _epoch(ds, dev, old))
    assert not torch.equal(off, _epoch(ds, dev, _options(loss_lap_scale=0.5, **kw)))
    assert not torch.equal(off, _epoch(ds, dev, _options(loss_edge_scale=0.5, **kw)))


def test_train_command_with_regularisers(dev, tmp_path):
    """python -m geobi_gnn_amd train with both flags on a frequency-4 split (4 train samples, 1 test sample), 5 epochs,
    batch 2: exit 0, both flags in the params file, the two extra tags beside the five in train/, test/ unchanged."""
    from geobi_gnn_amd import train_util
    data = str(tmp_path / 'Synthetic')
    _write_split(data, 'train', ('s1', 's2'), 4, (0.1, 0.3), seed0=960)
    _write_split(data, 'test', ('t1',), 4, (0.2,), seed0=970)
    out = str(tmp_path / 'run')
    run = _train_command(data, out, extra=('--no_predict', '--loss_v', 'CD', '--loss_n', 'sided', '--loss_lap_scale', '0.5',
                                           '--loss_edge_scale', '0.25'))
    assert run.returncode == 0, run.stderr[-2000:]
    with open(os.path.join(out, 'GeoBi-GNN_Synthetic_params.json')) as fh:
        params = json.load(fh)
    assert params['loss_lap_scale'] == 0.5 and params['loss_edge_scale'] == 0.25
    train_events = [f for f in os.listdir(os.path.join(out, 'train')) if f.startswith('events.out.tfevents')]
    test_events = [f for f in os.listdir(os.path.join(out, 'test')) if f.startswith('events.out.tfevents')]
    assert len(train_events) == 1 and len(test_events) == 1
    tr = train_util.read_scalars(os.path.join(out, 'train', train_events[0]))
    te = train_util.read_scalars(os.path.join(out, 'test', test_events[0]))
    steps = sorted({s for s, _, _ in tr})
    assert steps == list(range(2, 21, 2))                                  # 2 steps of 2 samples per epoch, 5 epochs
    for s in steps:
        at = {t: x for s2, t, x in tr if s2 == s}
        assert sorted(at) == ['dual_loss', 'error_f', 'error_v', 'loss_edge', 'loss_f', 'loss_lap', 'loss_v']
        assert all(np.isfinite(x) for x in at.values()) and at['loss_lap'] > 0 and at['loss_edge'] > 0
        want = at['loss_v'] + at['loss_f'] + 0.5 * at['loss_lap'] + 0.25 * at['loss_edge']
        assert abs(at['dual_loss'] - want) <= 1e-5 * want
    for s in sorted({s for s, _, _ in te}):
        assert sorted(t for s2, t, _ in te if s2 == s) == ['error_f', 'error_v', 'loss_f', 'loss_v']
