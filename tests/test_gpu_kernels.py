"""GPU parity tests, kernel by kernel: HIP path (through the C ABI) vs the CPU oracle.

Bars: integer / index outputs bit-exact; floating point within 1e-5 of the fp64 oracle, relative to
the tensor's max magnitude (the north star's "1e-5 relative fp32"), unless a test states otherwise.
"""
import ctypes

import numpy as np
import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


def _sym_graph(n, m, seed, loops=True):
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(0, n, (2, m), generator=g)
    ei = torch.cat([a, a.flip(0)], 1)
    key = torch.unique(ei[0] * n + ei[1])
    ei = torch.stack([key // n, key % n], 0)
    if loops:
        ei = torch.cat([ei, torch.arange(n).repeat(2, 1)], 1)
    return ei


# ------------------------------------------------------------------------------- CSR
def test_csr_from_coo_and_transpose(dev):
    from geobi_gnn_amd.graph import Graph
    n = 1000
    g0 = torch.Generator().manual_seed(0)
    ei = torch.randint(0, n, (2, 20000), generator=g0)            # directed, duplicates, self loops
    g = Graph.from_edge_index(ei.to(dev), n).ensure_in()
    keep = ei[0] != ei[1]
    r, c = ei[0][keep], ei[1][keep]
    order = torch.argsort(r * n + c, stable=True)
    assert g.E == int(keep.sum())
    assert torch.equal(g.col_out.cpu().long(), c[order])
    assert torch.equal(g.ensure_rows().cpu().long(), r[order])
    rp = torch.zeros(n + 1, dtype=torch.long); rp[1:] = torch.cumsum(torch.bincount(r, minlength=n), 0)
    assert torch.equal(g.rowptr_out.cpu().long(), rp)
    # original edge ids: the multiset of (r, c) must map back
    eid = g.eid_out.cpu().long()
    assert torch.equal(ei[0][eid], r[order]) and torch.equal(ei[1][eid], c[order])
    # transposed CSR
    order_t = torch.argsort(c[order] * n + r[order], stable=True)
    assert torch.equal(g.col_in.cpu().long(), r[order][order_t])
    rpt = torch.zeros(n + 1, dtype=torch.long); rpt[1:] = torch.cumsum(torch.bincount(c, minlength=n), 0)
    assert torch.equal(g.rowptr_in.cpu().long(), rpt)
    # pos_in: out-edge e sits at pos_in[e] of the in-CSR
    pos_in = g.pos_in.cpu().long()
    inv = torch.empty_like(order_t); inv[order_t] = torch.arange(order_t.numel())
    assert torch.equal(pos_in, inv)


def test_csr_empty_and_loops_only(dev):
    from geobi_gnn_amd.graph import Graph
    ei = torch.arange(5).repeat(2, 1).to(dev)
    g = Graph.from_edge_index(ei, 5).ensure_in()
    assert g.E == 0 and int(g.rowptr_in.abs().sum()) == 0 and int(g.rowptr_out.abs().sum()) == 0


# ------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize('M,N,K,transB', [(300, 32, 56, 0), (1000, 64, 576, 0), (257, 128, 1152, 0),
                                          (513, 1024, 32, 1), (129, 6, 300, 0), (77, 108, 64, 1),
                                          (1, 32, 4, 0)])
def test_gemm_nn(dev, M, N, K, transB):
    from geobi_gnn_amd import _lib as L
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g)
    B = torch.randn(N, K, generator=g) if transB else torch.randn(K, N, generator=g)
    bias = torch.randn(N, generator=g)
    ref = A.double() @ (B.double().t() if transB else B.double()) + bias.double()
    ref = torch.where(ref > 0, ref, ref * 0.2)
    Ad, Bd, bd = A.to(dev), B.to(dev), bias.to(dev)
    C = torch.empty(M, N, device=dev)
    L.call('geobi_gemm_nn', L.ptr(Ad), K, L.ptr(Bd), B.shape[1], transB, L.ptr(C), N, M, N, K, L.ptr(bd), 0.2,
           L.stream())
    assert rel_err(C.cpu(), ref) < TOL


@pytest.mark.parametrize('M,I,J', [(5000, 576, 32), (1000, 1152, 128), (4097, 9, 64), (300, 3, 1024), (7, 56, 32)])
def test_gemm_tn(dev, M, I, J):
    from geobi_gnn_amd import _lib as L
    g = torch.Generator().manual_seed(M + I + J)
    A = torch.randn(M, I + 3, generator=g)       # padded leading dimension
    B = torch.randn(M, J, generator=g)
    ref = A[:, :I].double().t() @ B.double()
    Ad, Bd = A.to(dev), B.to(dev)
    C = torch.empty(I, J, device=dev)
    ws = L.workspace(L.lib().geobi_gemm_tn_ws_bytes(I, J, M), dev)
    L.call('geobi_gemm_tn', L.ptr(Ad), I + 3, L.ptr(Bd), J, M, I, J, L.ptr(C), J, L.ptr(ws), ws.numel(), L.stream())
    assert rel_err(C.cpu(), ref) < TOL


# ------------------------------------------------------------------------- FeaSt conv
def _run_feast(dev, Cin, Cout, ei, n, slope, split, seed, xscale=1.0, x=None, fused=True):
    """fused=True / 16: the default path (aggregation + node transform in one kernel on 16-node tiles, feast_fused.hip);
    fused=32: the same kernels in the round-2 geometry (32-node tiles, geobi_set_tile_rows);
    fused=False: separate aggregation and GEMM kernels with z in HBM (GEOBI_FUSED=0)."""
    from geobi_gnn_amd import ops, _lib as L
    was = ops.FUSED
    ops.FUSED = bool(fused)
    try:
        if fused == 32:
            L.call('geobi_set_tile_rows', 32)
        return _run_feast_impl(dev, Cin, Cout, ei, n, slope, split, seed, xscale, x)
    finally:
        ops.FUSED = was
        L.call('geobi_set_tile_rows', 0)


def _run_feast_impl(dev, Cin, Cout, ei, n, slope, split, seed, xscale, x):
    from geobi_gnn_amd.feast_conv import FeaStConv
    from oracle import pyg_ops as P
    torch.manual_seed(seed)
    ora = P.FeaStConv(Cin, Cout, 9).double()
    hip = FeaStConv(Cin, Cout, 9).to(dev)
    hip.load_state_dict({k: v.float() for k, v in ora.state_dict().items()})
    if x is None:
        x = torch.randn(n, Cin, dtype=torch.double) * xscale
    x = x.double()
    gout = torch.randn(n, Cout, dtype=torch.double)
    xo = x.clone().requires_grad_(True)
    out_o = ora(xo, ei)
    if slope != 1.0:
        out_o = torch.nn.functional.leaky_relu(out_o, slope)
    out_o.backward(gout)
    eid = ei.to(dev)
    if split:
        xa = x[:, :Cin // 2].float().to(dev).requires_grad_(True)
        xb = x[:, Cin // 2:].float().to(dev).requires_grad_(True)
        out_h = hip(xa, eid, x2=xb, slope=slope)
    else:
        xa = x.float().to(dev).requires_grad_(True)
        out_h = hip(xa, eid, slope=slope)
    out_h.backward(gout.float().to(dev))
    torch.cuda.synchronize()
    errs = {'out': rel_err(out_h.detach().cpu(), out_o.detach())}
    gx = torch.cat([xa.grad, xb.grad], 1) if split else xa.grad
    errs['dx'] = rel_err(gx.cpu(), xo.grad)
    for (k, po), (_, ph) in zip(ora.named_parameters(), hip.named_parameters()):
        errs['d' + k] = rel_err(ph.grad.cpu(), po.grad)
    return errs


_FEAST_SHAPES = [(6, 32, 0.2, False), (12, 32, 0.2, False), (32, 64, 0.2, False),
                 (64, 128, 0.2, False), (128, 128, 0.2, False),
                 (128, 64, 1.0, False), (128, 64, 0.2, True),
                 (64, 32, 1.0, False), (64, 32, 0.2, True),
                 (6, 64, 0.2, True), (12, 128, 1.0, False), (32, 32, 0.2, False),
                 (12, 32, 0.2, True), (12, 128, 1.0, True)]     # 6 | 6: parts that cut a 16-B piece
# ... and the rest of the product the C ABI accepts, slopes alternating: with the three values of `fused` this reaches
# every leaf of the launchers' dispatch (forward, dx at one / two / four column tiles, every fused row pass, and the
# standalone row pass in both forms: Cin = 128 with Cout = 32, the 3 | 3 and 6 | 6 splits)
_FEAST_SHAPES += [(ci, co, (0.2, 1.0)[i % 2], sp) for i, (ci, co, sp) in enumerate(
    (ci, co, sp) for ci in (6, 12, 32, 64, 128) for co in (32, 64, 128) for sp in (False, True)
    if (ci, co, sp) not in {(a, b, d) for a, b, _, d in _FEAST_SHAPES})]


@pytest.mark.parametrize('fused', [True, 32, False])
@pytest.mark.parametrize('Cin,Cout,slope,split', _FEAST_SHAPES)
def test_feast_conv_random_graph(dev, Cin, Cout, slope, split, fused):
    n = 700          # 21 full tiles of 32 nodes + a ragged one
    ei = _sym_graph(n, 2500, seed=Cin + Cout)
    errs = _run_feast(dev, Cin, Cout, ei, n, slope, split, seed=Cin * 7 + Cout, fused=fused)
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize('Cin,Cout,split', [(64, 128, False), (64, 128, True), (128, 64, True), (128, 128, False),
                                            (128, 32, False)])
def test_feast_column_parts_are_bit_identical(dev, Cin, Cout, split):
    """Launches of layers that read 128 channels (forward: Cin = 128; input gradient: Cout = 128) with at most 512 tiles
    run every tile on TWO workgroups, each producing half of the output columns (feast_fused_kernel CS = 2,
    geobi_set_column_parts).  A part runs
    the unsplit kernel's accumulator chains, so forward, input gradient and every parameter gradient must agree with the
    one-part launch bit for bit; the one-part launch is checked against the fp64 oracle here (the default -- two parts at
    this size -- by every other test of this file)."""
    from geobi_gnn_amd import _lib as L
    from geobi_gnn_amd.feast_conv import FeaStConv
    n = 333
    g = torch.Generator().manual_seed(Cin + Cout)
    ei = torch.cat([torch.randint(0, n - 20, (2, 3000), generator=g),
                    torch.stack([torch.arange(1, 201), torch.zeros(200, dtype=torch.long)])], 1).to(dev)
    torch.manual_seed(3)
    conv = FeaStConv(Cin, Cout, 9).to(dev)
    x = torch.randn(n, Cin, generator=g)
    gout = torch.randn(n, Cout, generator=g).to(dev)
    got = {}
    try:
        for parts in (1, 2):
            L.call('geobi_set_column_parts', parts)
            conv.zero_grad()
            if split:
                xa = x[:, :Cin // 2].to(dev).requires_grad_(True)
                xb = x[:, Cin // 2:].to(dev).requires_grad_(True)
                out = conv(xa, ei, x2=xb, slope=0.2)
            else:
                xa = x.to(dev).requires_grad_(True)
                out = conv(xa, ei, slope=0.2)
            out.backward(gout)
            got[parts] = [out.detach().clone(), xa.grad.clone()] + ([xb.grad.clone()] if split else []) + \
                         [p_.grad.clone() for p_ in conv.parameters()]
            if parts == 1:
                errs = _run_feast(dev, Cin, Cout, ei.cpu(), n, 0.2, split, seed=5)
                assert max(errs.values()) < TOL, errs
    finally:
        L.call('geobi_set_column_parts', 0)
    for a, b in zip(got[1], got[2]):
        assert torch.equal(a, b)


@pytest.mark.parametrize('Cout,slope,split', [(32, 0.2, False), (32, 1.0, True), (64, 0.2, True), (128, 0.2, False),
                                              (128, 1.0, True)])
def test_feast_rowpass_forms_at_64_channels(dev, Cout, slope, split):
    """The fused backward row pass of a 64-channel layer has three forms (geobi_set_rowpass_form): lane-private row reads,
    rows staged through LDS by global_load_lds (default), and the channel-chunked 32-node-tile kernel (default at
    Cout = 128).  Every form against the fp64 oracle on a graph with isolated nodes and a hub of in-degree 200+ (several
    chunks of 16 items per node, ragged last tile); staged and lane-private run the same FMAs in the same order."""
    from geobi_gnn_amd import _lib as L
    n = 333
    g = torch.Generator().manual_seed(Cout)
    ei = torch.randint(0, n - 20, (2, 3000), generator=g)
    hub = torch.stack([torch.arange(1, 201), torch.zeros(200, dtype=torch.long)])
    ei = torch.cat([ei, hub], 1)
    got = {}
    try:
        for form in ((0, 0), (1, 0), (0, 1)):
            L.call('geobi_set_rowpass_form', *form)
            got[form] = _run_feast(dev, 64, Cout, ei, n, slope, split, seed=17 + Cout)
            assert max(got[form].values()) < TOL, (form, got[form])
    finally:
        L.call('geobi_set_rowpass_form', -1, -1)
    assert got[(0, 0)] == got[(1, 0)], (got[(0, 0)], got[(1, 0)])       # bit-identical results -> identical errors


def test_feast_conv_directed_graph_and_isolated_nodes(dev):
    """Non-symmetric edges, duplicate edges kept, nodes without neighbours, degree > 64."""
    n = 300
    g = torch.Generator().manual_seed(3)
    ei = torch.randint(0, n - 20, (2, 4000), generator=g)          # last 20 nodes isolated
    hub = torch.stack([torch.arange(1, 201), torch.zeros(200, dtype=torch.long)])   # node 0: in-degree 200+
    ei = torch.cat([ei, hub], 1)
    for fused in (True, False):
        errs = _run_feast(dev, 32, 64, ei, n, 0.2, False, seed=11, fused=fused)
        assert max(errs.values()) < TOL, (fused, errs)
    # 128 input channels: the fused backward keeps the partial dot products of a node's first 16 items in registers and
    # parks the rest (here up to 200 items of the hub, and its self loop) in the rows it overwrites at the end
    for cout, split in ((64, False), (128, True)):
        errs = _run_feast(dev, 128, cout, ei, n, 0.2, split, seed=13 + cout, fused=True)
        assert max(errs.values()) < TOL, (cout, split, errs)


def test_feast_conv_large_logits(dev):
    """Features of O(30) magnitude (positions scaled by 1 / mean edge length) stress the softmax."""
    n = 500
    ei = _sym_graph(n, 2000, seed=5)
    errs = _run_feast(dev, 12, 32, ei, n, 0.2, False, seed=5, xscale=30.0)
    assert max(errs.values()) < TOL, errs       # 6- / 12-channel layers evaluate u (x_j - x_i) per edge, like the reference


@pytest.mark.parametrize('which', ['vertex', 'facet'])
def test_feast_conv_level0_coordinates_far_from_origin(dev, which):
    """Level-0 inputs as the dataset delivers them for a patch of a large scan: positions in units of the mean
    edge length around the WHOLE mesh's centroid (dataset.py:140,179), i.e. coordinates of several hundred with
    neighbours ~1 apart.  Output and every gradient (u.weight included) stay within 1e-5 of the fp64 oracle."""
    from geobi_gnn_amd import meshgen
    dv, df = meshgen.synthetic_dual_data(8, 0.2, seed=2)
    d = dv if which == 'vertex' else df
    x = d.x.clone()
    x[:, :3] += torch.tensor([310.0, -205.0, 97.0])
    if which == 'facet':      # the facet branch's l_conv1 reads 12 channels: [x_f | centroid | normal]
        x = torch.cat([x, x[:, :3] + 0.01, x[:, 3:]], 1)
    errs = _run_feast(dev, x.shape[1], 32, d.edge_index, x.shape[0], 0.2, False, seed=3, x=x)
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize('which', ['vertex', 'facet'])
def test_feast_conv_level0_at_large_scan_size(dev, which):
    """l_conv1 (Cin 6 / 12 -> 32) on the level-0 graphs of BASELINE configs[3] (n = 87: V = 75 692, F = 151 380,
    1.97 M facet edges, |x| up to ~72): output and all gradients vs the fp64 oracle at 1e-5."""
    from geobi_gnn_amd import meshgen
    torch.set_num_threads(16)
    dv, df = meshgen.synthetic_dual_data(87, 0.2, seed=7)
    d = dv if which == 'vertex' else df
    x = d.x.clone()
    if which == 'facet':      # [x_f | centroid | normal] as network.py:335-337 assembles it (here from the input geometry)
        x = torch.cat([x, x[:, :3], x[:, 3:]], 1)
    errs = _run_feast(dev, x.shape[1], 32, d.edge_index, x.shape[0], 0.2, False, seed=4, x=x)
    print(which, errs)
    assert max(errs.values()) < TOL, errs


def test_feast_conv_deterministic(dev):
    from geobi_gnn_amd.feast_conv import FeaStConv
    torch.manual_seed(0)
    n = 2000
    ei = _sym_graph(n, 9000, seed=9).to(dev)
    conv = FeaStConv(64, 32, 9).to(dev)
    x = torch.randn(n, 64, device=dev, requires_grad=True)
    outs = []
    for _ in range(2):
        conv.zero_grad(); x.grad = None
        o = conv(x, ei, slope=0.2)
        o.square().sum().backward()
        outs.append((o.detach().clone(), x.grad.clone(), conv.lin.weight.grad.clone(), conv.c.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)        # no atomics anywhere: bitwise reproducible


# ---------------------------------------------------------------------- pooling kernels
def test_edge_weight_t10(dev):
    from geobi_gnn_amd import _lib as L
    for C in (32, 64, 6):
        g = torch.Generator().manual_seed(C)
        n, E = 400, 3000
        x = torch.randn(n, C, generator=g) * 0.5
        row = torch.randint(0, n, (E,), generator=g, dtype=torch.int32)
        col = torch.randint(0, n, (E,), generator=g, dtype=torch.int32)
        w = torch.rand(E, generator=g)
        ref = w.double() + ((x[row.long()].double() - x[col.long()].double()) ** 2).sum(1).div(-2).exp()
        out = torch.empty(E, device=dev)
        xd, rd, cd, wd = x.to(dev), row.to(dev), col.to(dev), w.to(dev)     # keep the operands alive
        L.call('geobi_edge_weight_t10', L.ptr(xd), C, L.ptr(rd), L.ptr(cd), L.ptr(wd), E, L.ptr(out), L.stream())
        assert rel_err(out.cpu(), ref) < TOL


def _greedy_sorted_oracle(n, rowptr, col, w):
    """oracle/oracle_c.c:oracle_greedy_sorted -- greedy matching in descending (w, min, max) order."""
    from oracle import pyg_ops as P
    lib = P._load_graclus_c()
    assert lib, 'oracle C helper not built'
    row = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
    mn, mx = torch.minimum(row, col), torch.maximum(row, col)
    # lexicographic: w desc, mn asc, mx asc  (stable sorts applied in reverse significance)
    order = torch.argsort(mx, stable=True)
    order = order[torch.argsort(mn[order], stable=True)]
    order = order[torch.argsort(-w[order].double(), stable=True)]
    out = torch.empty(n, dtype=torch.long)
    args = [t.contiguous() for t in (order, row, col)]
    lib.oracle_greedy_sorted(ctypes.c_int64(n), ctypes.c_int64(col.numel()), ctypes.c_void_p(args[0].data_ptr()),
                             ctypes.c_void_p(args[1].data_ptr()), ctypes.c_void_p(args[2].data_ptr()),
                             ctypes.c_void_p(out.data_ptr()))
    return out


@pytest.mark.parametrize('n,m,ties', [(500, 2000, False), (3000, 9000, True), (50, 40, False),
                                      (20000, 80000, True), (9000, 30000, False)])     # > 8192 nodes: multi-launch path
def test_matching_equals_sorted_greedy(dev, n, m, ties):
    from geobi_gnn_amd.graph import Graph
    from geobi_gnn_amd import net_util
    ei = _sym_graph(n, m, seed=n, loops=False)
    g = torch.Generator().manual_seed(n)
    # symmetric weights keyed by the undirected pair
    lo, hi = torch.minimum(ei[0], ei[1]), torch.maximum(ei[0], ei[1])
    _, inv = torch.unique(lo * n + hi, return_inverse=True)
    w = torch.rand(int(inv.max()) + 1, generator=g)[inv]
    if ties:
        w = (w * 4).floor() / 4
    gr = Graph.from_edge_index(ei.to(dev), n)
    ws = gr.weights_sorted(w.to(dev))
    cluster, status, state = net_util.hip_match(gr, ws, rounds=3)
    while int(status.item()) != 0:                       # resume from the saved state until converged
        cluster, status, state = net_util.hip_match(gr, ws, rounds=3, state=state)
    ref = _greedy_sorted_oracle(n, gr.rowptr_out.cpu().long(), gr.col_out.cpu().long(), ws.cpu())
    assert torch.equal(cluster.cpu().long(), ref)
    # validity (what graclus guarantees): clusters of <= 2 nodes, id = min member, pairs are edges
    c = cluster.cpu().long()
    assert int(torch.bincount(c, minlength=n).max()) <= 2
    assert bool((c <= torch.arange(n)).all())
    paired = torch.nonzero(c != torch.arange(n)).flatten()
    eset = set((ei[0] * n + ei[1]).tolist())
    assert all((int(c[u]) * n + int(u)) in eset for u in paired[:200])


# 5000: the one-block scan; 16384 / 16385: its boundary to the multi-block look-back scan; 70001: 18 look-back blocks
# with a ragged tail; 262144 / 262145: the boundary to rocPRIM
@pytest.mark.parametrize('n', [5000, 16384, 16385, 70001, 262144, 262145])
def test_relabel_matches_consecutive_cluster(dev, n):
    from geobi_gnn_amd import net_util
    from oracle import pyg_ops as P
    g = torch.Generator().manual_seed(1)
    cluster = torch.randint(0, n, (n,), generator=g)
    cnew, count = net_util.relabel(cluster.to(torch.int32).to(dev))
    ref, _ = P.consecutive_cluster(cluster)
    assert torch.equal(cnew.cpu().long(), ref) and int(count.item()) == int(ref.max()) + 1


@pytest.mark.parametrize('C', [3, 32, 64])
def test_segment_max_mean_unpool(dev, C):
    from geobi_gnn_amd import ops
    from oracle import pyg_ops as P
    g = torch.Generator().manual_seed(C)
    n, nseg = 3000, 1100
    seg = torch.randint(0, nseg - 50, (n,), generator=g)          # the last 50 segments stay empty
    x = torch.randn(n, C, generator=g)
    x[::7] = x[1::7][:x[::7].shape[0]]                             # exact ties between rows
    gout = torch.randn(nseg, C, generator=g)
    sidx = ops.SegmentIndex(seg.to(torch.int32).to(dev), nseg)
    for red, fn in (('max', ops.SegmentMaxFn), ('mean', ops.SegmentMeanFn)):
        xo = x.clone().requires_grad_(True)
        ref = P.scatter(xo, seg, dim=0, dim_size=nseg, reduce=red)
        ref.backward(gout)
        xh = x.to(dev).requires_grad_(True)
        out = fn.apply(xh, sidx)
        out.backward(gout.to(dev))
        if red == 'max':
            assert torch.equal(out.detach().cpu(), ref.detach())          # selection: bit-exact
            assert torch.equal(xh.grad.cpu(), xo.grad)
        else:
            assert rel_err(out.detach().cpu(), ref.detach()) < TOL
            assert rel_err(xh.grad.cpu(), xo.grad) < TOL
    # unpool gather + sorted-segment-sum backward
    xc = torch.randn(nseg, C, generator=g)
    gf = torch.randn(n, C, generator=g)
    xo = xc.clone().requires_grad_(True)
    xo[seg].backward(gf)
    xh = xc.to(dev).requires_grad_(True)
    out = ops.UnpoolFn.apply(xh, sidx)
    out.backward(gf.to(dev))
    assert torch.equal(out.detach().cpu(), xc[seg])
    assert rel_err(xh.grad.cpu(), xo.grad.double()) < TOL


def test_pool_edge_matches_oracle(dev):
    from geobi_gnn_amd import net_util
    from oracle import ref_model as R
    n = 2000
    ei = _sym_graph(n, 8000, seed=4)
    g = torch.Generator().manual_seed(4)
    w = torch.rand(ei.shape[1], generator=g)
    cluster = torch.randint(0, 700, (n,), generator=g)
    cluster = torch.unique(cluster, return_inverse=True)[1]          # consecutive ids
    ref_i, ref_w = R.pool_edge(cluster, ei, w)
    out_i, out_w = net_util.pool_edge(cluster.to(dev), ei.to(dev), w.to(dev))
    assert torch.equal(out_i.cpu(), ref_i)
    assert rel_err(out_w.cpu(), ref_w.double()) < 1e-6
    out_i2, none_w = net_util.pool_edge(cluster.to(dev), ei.to(dev))
    assert torch.equal(out_i2.cpu(), ref_i) and none_w is None
    # reference fixture (pool_edge / pool_face run through the reference's own net_util.py)
    from helpers import load_fixture
    fx = load_fixture('pure_functions.npz')
    t = lambda k: torch.from_numpy(fx[k])
    oi, ow = net_util.pool_edge(t('cluster').long().to(dev), t('edge_index').long().to(dev), t('calc_weight').to(dev))
    assert torch.equal(oi.cpu(), t('pool_edge_index').long())
    assert rel_err(ow.cpu(), t('pool_edge_weight').double()) < 1e-6
    assert torch.equal(net_util.pool_face(t('cluster').long().to(dev), t('faces').long().to(dev)).cpu(),
                       t('pool_face').long())


# ----------------------------------------------------------------- geometry and heads
def test_face_geom(dev):
    from geobi_gnn_amd import ops, meshgen
    from oracle import ref_model as R
    noisy, _, faces = meshgen.noisy_icosphere(6, 0.3, seed=2)
    verts = torch.from_numpy(noisy).double() * 7.0
    fv = torch.from_numpy(faces)
    xf = torch.randn(fv.shape[0], 6, dtype=torch.double)
    gout = torch.randn(fv.shape[0], 12, dtype=torch.double)
    vo = verts.clone().requires_grad_(True)
    ref = torch.cat((xf, vo[fv].mean(1), R.computer_face_normal(vo, fv)), 1)
    ref.backward(gout)
    fv32 = fv.to(torch.int32).to(dev)
    cidx = ops.SegmentIndex(fv32.view(-1), verts.shape[0])
    vh = verts.float().to(dev).requires_grad_(True)
    out = ops.FaceGeomFn.apply(vh, xf.float().to(dev), fv32, cidx)
    out.backward(gout.float().to(dev))
    assert rel_err(out.detach().cpu(), ref.detach()) < TOL
    assert rel_err(vh.grad.cpu(), vo.grad) < TOL
    # reference fixture for computer_face_normal
    from helpers import load_fixture
    fx = load_fixture('pure_functions.npz')
    pts, f32 = torch.from_numpy(fx['points']).to(dev), torch.from_numpy(fx['faces']).to(dev)
    c2 = ops.SegmentIndex(f32.view(-1), pts.shape[0])
    o2 = ops.FaceGeomFn.apply(pts, torch.zeros(f32.shape[0], 6, device=dev), f32, c2)
    assert rel_err(o2[:, 9:12].cpu(), torch.from_numpy(fx['face_normal']).double()) < TOL


@pytest.mark.parametrize('mode,nout', [(0, 3), (0, 1), (1, 3)])
def test_head(dev, mode, nout):
    from geobi_gnn_amd import ops
    torch.manual_seed(mode * 10 + nout)
    n = 777
    fc1, fc2 = torch.nn.Linear(32, 1024).double(), torch.nn.Linear(1024, nout).double()
    x = torch.randn(n, 32, dtype=torch.double)
    x6 = torch.randn(n, 6, dtype=torch.double)
    dd = torch.nn.functional.normalize(torch.randn(n, 3, dtype=torch.double), dim=1)
    gout = torch.randn(n, 3, dtype=torch.double)
    xo = x.clone().requires_grad_(True)
    y = fc2(torch.nn.functional.leaky_relu(fc1(xo), 0.2))
    if mode == 0:
        if nout == 1:
            y = y * dd
        ref = y + x6[:, :3]
    else:
        ref = torch.nn.functional.normalize(y, dim=1)
    ref.backward(gout)
    f = lambda t: t.detach().float().to(dev)
    xh = f(x).requires_grad_(True)
    ps = [f(p).requires_grad_(True) for p in (fc1.weight, fc1.bias, fc2.weight, fc2.bias)]
    out = ops.HeadFn.apply(xh, ps[0], ps[1], ps[2], ps[3], mode, f(dd) if (mode == 0 and nout == 1) else None,
                           f(x6) if mode == 0 else None)
    out.backward(f(gout))
    assert rel_err(out.detach().cpu(), ref.detach()) < TOL
    assert rel_err(xh.grad.cpu(), xo.grad) < TOL
    for ph, po in zip(ps, (fc1.weight, fc1.bias, fc2.weight, fc2.bias)):
        assert rel_err(ph.grad.cpu(), po.grad) < TOL


def test_errors_are_loud(dev):
    from geobi_gnn_amd import _lib as L
    from geobi_gnn_amd.feast_conv import FeaStConv
    with pytest.raises(L.GeobiError):
        FeaStConv(6, 32, 9)(torch.randn(10, 6), torch.zeros(2, 4, dtype=torch.long))      # CPU tensors
    conv = FeaStConv(6, 32, 9).to(dev)
    with pytest.raises(L.GeobiError):
        conv(torch.randn(10, 7, device=dev), torch.zeros(2, 4, dtype=torch.long, device=dev))   # wrong width
    with pytest.raises(L.GeobiError):
        L.call('geobi_gemm_nn', None, 1, None, 1, 0, None, 1, 1, 1, 1, None, 1.0, L.stream())
    # node ids outside [0, N) are caught when the adjacency is built, not by a faulting gather later
    bad = torch.tensor([[0, 1, 2, 11], [1, 0, 3, 2]], device=dev)
    with pytest.raises(L.GeobiError, match='outside'):
        conv(torch.randn(10, 6, device=dev), bad)
    neg = torch.tensor([[0, 1, -1], [1, 0, 2]], device=dev)
    with pytest.raises(L.GeobiError, match='outside'):
        conv(torch.randn(10, 6, device=dev), neg)
    with pytest.raises(NotImplementedError):
        FeaStConv(6, 32, 4)
    with pytest.raises(L.GeobiError):
        FeaStConv(16, 32, 9).to(dev)(torch.randn(10, 16, device=dev), torch.tensor([[0, 1], [1, 0]], device=dev))


def test_symmetric_graph_reverse_index(dev):
    """Symmetric graphs skip the transposition sort: in-CSR == out-CSR, pos_in by binary search."""
    from geobi_gnn_amd.graph import Graph
    n = 800
    ei = _sym_graph(n, 3000, seed=21)
    g = Graph.from_edge_index(ei.to(dev), n)
    assert g.symmetric is True
    g.ensure_in()
    assert g.col_in.data_ptr() == g.col_out.data_ptr()
    row, col = g.ensure_rows().cpu().long(), g.col_out.cpu().long()
    key = row * n + col
    rev = col * n + row
    expect = torch.searchsorted(key, rev)
    assert torch.equal(g.pos_in.cpu().long(), expect)
    # a directed graph is detected and takes the sort path
    g2 = Graph.from_edge_index(torch.tensor([[0, 1, 2], [1, 2, 0]]).to(dev), 3)
    assert g2.symmetric is False
    g2.ensure_in()
    assert g2.col_in.cpu().tolist() == [2, 0, 1]


def test_sort_free_inverse_lists(dev):
    """from_matching / compose agree with the radix-sort construction."""
    from geobi_gnn_amd import ops, net_util
    from geobi_gnn_amd.graph import Graph
    n = 4000
    ei = _sym_graph(n, 12000, seed=31, loops=False)
    gr = Graph.from_edge_index(ei.to(dev), n)
    w = torch.rand(gr.E, generator=torch.Generator().manual_seed(1)).to(dev)
    cnew1, g1, w1, raw1, _ = net_util._coarsen(gr, None)
    a = ops.SegmentIndex.from_matching(cnew1, raw1, g1.N)
    b = ops.SegmentIndex(cnew1, g1.N)
    assert torch.equal(a.segptr, b.segptr) and torch.equal(a.members, b.members)
    cnew2, g2, _, raw2, _ = net_util._coarsen(g1, None)
    a2 = ops.SegmentIndex.from_matching(cnew2, raw2, g2.N)
    comp = cnew2[cnew1.long()]
    c_fast = ops.SegmentIndex.compose(a, a2, comp)
    c_ref = ops.SegmentIndex(comp, g2.N)
    assert torch.equal(c_fast.segptr, c_ref.segptr)
    # same member SETS per segment (order inside a segment is fixed but not ascending)
    sp = c_ref.segptr.cpu().long()
    seg_of_slot = torch.repeat_interleave(torch.arange(g2.N), sp[1:] - sp[:-1])
    k_fast = torch.sort(seg_of_slot * n + c_fast.members.cpu().long())[0]
    k_ref = torch.sort(seg_of_slot * n + c_ref.members.cpu().long())[0]
    assert torch.equal(k_fast, k_ref)
    x = torch.randn(g2.N, 8, device=dev, requires_grad=True)
    gf = torch.randn(n, 8, device=dev)
    ops.UnpoolFn.apply(x, c_fast).backward(gf)
    g_fast = x.grad.clone(); x.grad = None
    ops.UnpoolFn.apply(x, c_ref).backward(gf)
    assert rel_err(g_fast.cpu(), x.grad.cpu()) < 1e-6


def test_sort_free_pool_edge_equals_radix_path(dev):
    """geobi_pool_edge_rows (bitonic merge per coarse node) vs geobi_pool_edge (global radix sort)."""
    from geobi_gnn_amd import net_util
    from geobi_gnn_amd.graph import Graph
    for n, m, seed in ((3000, 9000, 41), (500, 400, 42), (20000, 120000, 43)):
        ei = _sym_graph(n, m, seed=seed, loops=False)
        gr = Graph.from_edge_index(ei.to(dev), n)
        lo, hi = torch.minimum(ei[0], ei[1]), torch.maximum(ei[0], ei[1])
        w = gr.weights_sorted(torch.rand(n * 37 + 11, generator=torch.Generator().manual_seed(seed))[(lo * 31 + hi) % (n * 37 + 11)].to(dev))
        cnew, coarse, w_c, raw, sidx = net_util._coarsen(gr, w)                 # rows kernel
        cnew2, coarse2, w_c2, _, _ = net_util._coarsen(gr, w, cluster32=raw)     # radix path on the same clusters
        assert torch.equal(cnew, cnew2) and coarse.N == coarse2.N and coarse.E == coarse2.E
        assert torch.equal(coarse.rowptr_out, coarse2.rowptr_out)
        assert torch.equal(coarse.col_out, coarse2.col_out) and torch.equal(coarse.ensure_rows(), coarse2.ensure_rows())
        assert rel_err(w_c.cpu(), w_c2.cpu().double()) < 1e-6
    # a hub whose merged row exceeds 64 entries falls back to the radix path transparently
    hub = torch.stack([torch.zeros(200, dtype=torch.long), torch.arange(1, 201)])
    ei = torch.cat([hub, hub.flip(0)], 1)
    gr = Graph.from_edge_index(ei.to(dev), 201)
    cnew, coarse, _, raw, _ = net_util._coarsen(gr, None)
    assert coarse.N == 200 and coarse.E == 2 * 199


def test_feast_split_input_equals_concatenated_at_scale(dev):
    """A (skip, up) input pair gives the same layer as the concatenated input, forward and backward, on a
    graph large enough that the weight-gradient GEMMs of the two halves plan more node slices than the
    concatenated shape would (regression: their slab workspace was sized for the concatenated width only)."""
    from geobi_gnn_amd.feast_conv import FeaStConv
    n, cin, cout = 126000, 128, 64
    ei = _sym_graph(n, 300000, seed=9).to(dev)
    torch.manual_seed(3)
    conv = FeaStConv(cin, cout, 9).to(dev)
    x = torch.randn(n, cin, device=dev)
    gout = torch.randn(n, cout, device=dev)
    xa = x.clone().requires_grad_(True)
    out = conv(xa, ei, slope=0.2)
    out.backward(gout)
    ref = {k: p.grad.clone() for k, p in conv.named_parameters()}
    conv.zero_grad(set_to_none=True)
    h1 = x[:, :64].clone().requires_grad_(True)
    h2 = x[:, 64:].clone().requires_grad_(True)
    out2 = conv(h1, ei, x2=h2, slope=0.2)
    out2.backward(gout)
    assert rel_err(out2.detach(), out.detach()) < 1e-6
    assert rel_err(torch.cat([h1.grad, h2.grad], 1), xa.grad) < 1e-6
    for k, p in conv.named_parameters():
        assert rel_err(p.grad, ref[k]) < 1e-5, k


@pytest.mark.parametrize('n,m', [(700, 2500), (12000, 40000), (300000, 900000)])
def test_match_coarsen_equals_separate_calls(dev, n, m):
    """geobi_match_coarsen = geobi_match_heavy_edge + geobi_relabel_compact + geobi_segment_csr_pairs
    (every size here takes the scan-free kernel pair: it serves up to 256 * 4096 nodes; the commit + scans + lists form
    is held by tests/test_gpu_pool.py)."""
    from geobi_gnn_amd.graph import Graph
    from geobi_gnn_amd import net_util, ops
    ei = _sym_graph(n, m, seed=n + 1, loops=False)
    g = torch.Generator().manual_seed(n)
    lo, hi = torch.minimum(ei[0], ei[1]), torch.maximum(ei[0], ei[1])
    _, inv = torch.unique(lo * n + hi, return_inverse=True)
    w = torch.rand(int(inv.max()) + 1, generator=g)[inv]
    gr = Graph.from_edge_index(ei.to(dev), n)
    ws = gr.weights_sorted(w.to(dev))
    for rounds in (2, 8):                                   # 2 rounds leave undecided nodes behind
        cluster, status, _ = net_util.hip_match(gr, ws, rounds=rounds)
        cnew, count = net_util.relabel(cluster)
        ref = ops.SegmentIndex.from_matching(cnew, cluster, n)
        counters = torch.zeros(4, dtype=torch.int32, device=dev)
        cl2, cnew2, sidx, _ = net_util.hip_match_coarsen(gr, ws, counters, rounds=rounds)
        und, nc = counters[:2].tolist()
        assert und == int(status.item()) and nc == int(count.item())
        assert torch.equal(cl2, cluster) and torch.equal(cnew2, cnew)
        assert torch.equal(sidx.segptr[:nc + 1], ref.segptr[:nc + 1])
        assert torch.equal(sidx.members, ref.members)


def test_softmax_exp_against_fp64(dev):
    """feast_dev.h: exp_le0, the six-instruction exp of every softmax (arguments: differences to the row maximum, finite
    and <= 0), checked in isolation through geobi_debug_exp_le0: <= 2 ulp of the fp32 result where it is a normal number,
    and a flush to zero (never garbage) below 2^-126."""
    import numpy as np
    from geobi_gnn_amd import _lib as L
    xs = np.concatenate([np.linspace(-104.0, 0.0, 200001), -np.logspace(-30, 2, 4001), [0.0, -0.0, -87.33, -87.34, -103.9]])
    x = torch.tensor(xs[xs >= -104.0], dtype=torch.float32, device=dev)
    y = torch.empty_like(x)
    L.call('geobi_debug_exp_le0', L.ptr(x), L.ptr(y), x.numel(), L.stream())
    want = torch.exp(x.double().cpu())
    got = y.double().cpu()
    tiny = 2.0 ** -126
    normal = want >= tiny
    ulp = torch.tensor(np.spacing(want[normal].float().numpy()), dtype=torch.float64)
    err = (got[normal] - want[normal]).abs() / ulp
    assert float(err.max()) <= 2.0, float(err.max())
    # below the normal range the hardware exp2 flushes: the result is 0 or the true (denormal) value, never more than 2^-126 off
    assert float((got[~normal] - want[~normal]).abs().max()) <= tiny
    assert float(got[~normal].min()) >= 0.0 and bool(torch.isfinite(got).all())
    assert float(got[x.cpu() == 0].min()) == 1.0


def test_head_split_precision_forward(dev):
    """geobi_set_head_precision(1): the heads' 32 -> 1024 product as six bf16 products with fp32 accumulation.  Not
    bit-identical to the fp32 form, but no farther from fp64: the bar is 2 x the fp32 kernel's own distance (measured
    0.9 x), for both heads (3 outputs + normalisation; 1 output along depth_direction + residual)."""
    from geobi_gnn_amd import _lib as L
    lib = L.lib()
    torch.manual_seed(4)
    N = 5000
    x = torch.randn(N, 32, device=dev) * 3
    w1 = (torch.rand(1024, 32, device=dev) * 2 - 1) / 32 ** 0.5
    b1 = (torch.rand(1024, device=dev) * 2 - 1) / 32 ** 0.5
    resid = torch.randn(N, 6, device=dev)
    ddir = torch.nn.functional.normalize(torch.randn(N, 3, device=dev), dim=1)
    try:
        for nout, mode in ((3, 1), (3, 0), (1, 0)):
            w2 = (torch.rand(nout, 1024, device=dev) * 2 - 1) / 32
            b2 = (torch.rand(nout, device=dev) * 2 - 1) / 32
            pre = x.double() @ w1.double().t() + b1.double()
            want = torch.nn.functional.leaky_relu(pre, 0.2) @ w2.double().t() + b2.double()
            errs = []
            for prec in (0, 1):
                assert lib.geobi_set_head_precision(prec) == 0
                raw = torch.empty(N, nout, device=dev); out = torch.empty(N, 3, device=dev)
                L.call('geobi_head_fwd', L.ptr(x), 32, N, L.ptr(w1), L.ptr(b1), 1024, L.ptr(w2), L.ptr(b2), nout, 0.2, mode,
                       L.ptr(ddir) if nout == 1 else None, None if mode == 1 else L.ptr(resid), 6, None, L.ptr(raw), L.ptr(out),
                       L.stream())
                errs.append(float((raw.double() - want).abs().max() / want.abs().max()))
            assert errs[0] < 1e-5 and errs[1] <= 2.0 * errs[0] + 1e-8, errs
        assert lib.geobi_set_head_precision(2) != 0
    finally:
        lib.geobi_set_head_precision(0)
