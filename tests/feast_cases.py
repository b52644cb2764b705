"""What tests/test_gpu_feast_edges.py and tests/test_feast_cases_host.py share: graphs that put a node at every boundary of
the FeaSt kernels' control flow (chunks of G = 16 edges per node, the 16 register-held items of the 128-channel backward,
16- and 32-row tiles with a ragged last one, the launch grid padded to 8), the per-row metric, and the runners that return
the tensors of the oracle (fp64 or fp32) and of the HIP path on one set of fp32 numbers.  Nothing here needs a GPU until
run_gpu is called."""
import functools

import torch

from helpers import rel_err

BAR = 1e-5                  # the project's "1e-5 relative fp32", here per ROW for out and dx
FLOOR = 1e-3                # row_err: a row counts as at least this share of the tensor's maximum
KEYS = ('out', 'dx', 'dlin.weight', 'du.weight', 'dc', 'dbias')
ROW_KEYS = ('out', 'dx')

# in-degree of node i < L and out-degree of node L + i: around every multiple of the chunk (15..18, 31..34, 47..49,
# 63..65), the short rows the 4- and 2-edge gather steps leave ragged (0..5, 7..9), and a five-chunk row (80)
D = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 18, 31, 32, 33, 34, 47, 48, 49, 63, 64, 65, 80)
L = len(D)
POOL = 96
N_LADDER = 161
FEAST_PRODUCT = [(ci, co, (0.2, 1.0)[i % 2], sp) for i, (ci, co, sp) in enumerate(
    (ci, co, sp) for ci in (6, 12, 32, 64, 128) for co in (32, 64, 128) for sp in (False, True))]
RING_SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 128, 129)
RING_SHAPES = ((6, 32), (64, 64), (128, 128))
REVERSED_SHAPES = ((12, 32), (64, 32), (128, 64))       # on the ladder with every edge flipped; (128, 64) runs split


class GraphInfo(object):
    """Per-node in- and out-degree (self loops not counted) of an edge_index, for reports in the kernels' own terms."""

    def __init__(self, edge_index, n):
        self.n = n
        self.indeg = torch.bincount(edge_index[1], minlength=n)
        self.outdeg = torch.bincount(edge_index[0], minlength=n)

    def describe(self, i):
        return 'node %d (in-degree %d, out-degree %d, row %d of 16-row tile %d, row %d of 32-row tile %d)' % (
            i, int(self.indeg[i]), int(self.outdeg[i]), i % 16, i // 16, i % 32, i // 32)


@functools.lru_cache(maxsize=None)
def _ladder():
    src, dst = [], []
    for i, d in enumerate(D):
        for t in range(d):
            src.append(2 * L + (7 * i + t) % POOL); dst.append(i)              # node i: in-degree D[i]
            src.append(L + i); dst.append(2 * L + (11 * i + t) % POOL)         # node L + i: out-degree D[i]
    last = N_LADDER - 1         # alone in the ragged last tile of both geometries
    for t in range(33):
        src.append(2 * L + t); dst.append(last)
    for t in range(17):
        src.append(last); dst.append(2 * L + 40 + t)
    return torch.tensor([src, dst], dtype=torch.long)


def ladder_graph():
    """(edge_index, N, info): directed, no duplicates, no self loops, built from arithmetic.  Node i < L has in-degree D[i]
    (sources in the pool), node L + i out-degree D[i] (targets in the pool), the pool 2L .. 2L + 95 ends up with ordinary
    degrees, 144 .. 159 have the implicit self loop only, and N - 1 = 160 (in-degree 33, out-degree 17) is the only node of
    the last tile since N = 1 (mod 32)."""
    ei = _ladder().clone()
    return ei, N_LADDER, GraphInfo(ei, N_LADDER)


def ring_graph(n):
    """The symmetric ring on n nodes: no edge for n = 1, one pair for n = 2."""
    if n == 1:
        return torch.zeros(2, 0, dtype=torch.long)
    a = torch.arange(n)
    b = (a + 1) % n
    key = torch.unique(torch.cat([a * n + b, b * n + a]))
    return torch.stack([key // n, key % n], 0)


MULTI_N, MULTI_PAIRS, MULTI_TWICE = 37, 90, 30


@functools.lru_cache(maxsize=None)
def _multi():
    pairs = torch.combinations(torch.arange(MULTI_N))                                   # all 666 pairs u < v
    pick = pairs[torch.randperm(pairs.shape[0], generator=torch.Generator().manual_seed(37))[:MULTI_PAIRS]]
    und = torch.cat([pick, pick[:MULTI_TWICE]]).t()
    return torch.cat([und, und.flip(0)], 1).contiguous()


def multi_graph():
    """The symmetric MULTIgraph a face list gives before coalescing: 90 random pairs on 37 nodes, the first 30 listed
    twice, both directions of each (240 entries, no self loops).  On it the reverse-edge index is no permutation."""
    return _multi().clone()


def graph_of_name(name):
    """'ladder', 'ladder_rev' (every edge flipped), 'multi37' or 'ring<n>' -> (edge_index, N, info)"""
    if name == 'multi37':
        ei = multi_graph()
        return ei, MULTI_N, GraphInfo(ei, MULTI_N)
    if name == 'ladder':
        return ladder_graph()
    if name == 'ladder_rev':
        ei = _ladder().flip(0).contiguous()
        return ei, N_LADDER, GraphInfo(ei, N_LADDER)
    n = int(name[len('ring'):])
    ei = ring_graph(n)
    return ei, n, GraphInfo(ei, n)


# ------------------------------------------------------------------------------ metric
def row_errs(a, b):
    """[rows] max_c |a - b| over max(max_c |b_row|, FLOOR * max |b|)"""
    a, b = a.double(), b.double()
    rows = b.abs().amax(1)
    return (a - b).abs().amax(1) / torch.clamp(rows, min=FLOOR * float(b.abs().max()))


def row_err(a, b):
    """The largest per-row error.  The floor only keeps a row of zeros from dividing by nothing: floor_engages(b) must be
    False for every reference the bar is applied to."""
    return float(row_errs(a, b).max())


def row_share(b):
    """The smallest row of b as a share of the tensor's maximum."""
    b = b.double().abs()
    return float(b.amax(1).min() / b.max())


def floor_engages(b):
    return row_share(b) < FLOOR


def distances(got, ref):
    """{key: distance}: per row for out and dx, over the tensor's maximum for the parameter gradients"""
    return {k: (row_err if k in ROW_KEYS else rel_err)(got[k], ref[k]) for k in KEYS}


def worst_rows(a, b, info, k=6):
    """The k worst rows of a against b in the kernels' terms, for assertion messages."""
    e = row_errs(a, b)
    order = torch.argsort(e, descending=True)[:k]
    return '; '.join('%s: %.2e' % (info.describe(int(i)), float(e[i])) for i in order)


# ----------------------------------------------------------------------------- runners
@functools.lru_cache(maxsize=None)
def draw(Cin, Cout, n, seed):
    """Default-initialised parameters, x ~ N(0, 1) and the output gradient, all drawn as fp32 numbers."""
    from oracle import pyg_ops as P
    state = torch.get_rng_state()
    try:
        torch.manual_seed(seed)
        params = {k: v.detach().clone() for k, v in P.FeaStConv(Cin, Cout, 9).state_dict().items()}
        x = torch.randn(n, Cin)
        gout = torch.randn(n, Cout)
    finally:
        torch.set_rng_state(state)
    assert all(t.dtype == torch.float32 for t in list(params.values()) + [x, gout])
    return params, x, gout


def seed_of(Cin, Cout):
    return Cin * 7 + Cout


def run_oracle_on(edge_index, n, Cin, Cout, slope, seed, dtype=torch.double):
    """oracle.pyg_ops.FeaStConv (+ leaky_relu) forward and backward in `dtype` on the fp32 numbers of draw()"""
    from oracle import pyg_ops as P
    params, x, gout = draw(Cin, Cout, n, seed)
    conv = P.FeaStConv(Cin, Cout, 9)
    conv.load_state_dict(params)
    conv = conv.to(dtype)
    xo = x.to(dtype).clone().requires_grad_(True)           # a leaf of its own: draw()'s tensors stay as drawn
    out = conv(xo, edge_index)
    if slope != 1.0:
        out = torch.nn.functional.leaky_relu(out, slope)
    out.backward(gout.to(dtype))
    res = {'out': out.detach(), 'dx': xo.grad}
    for k, p in conv.named_parameters():
        res['d' + k] = p.grad
    return res


@functools.lru_cache(maxsize=None)
def _oracle(name, Cin, Cout, slope, seed, dtype):
    ei, n, _ = graph_of_name(name)
    return run_oracle_on(ei, n, Cin, Cout, slope, seed, dtype)


def run_oracle(name, Cin, Cout, slope, seed=None):
    """The fp64 reference on a named graph; computed once per process, callers leave it unchanged."""
    return _oracle(name, Cin, Cout, slope, seed_of(Cin, Cout) if seed is None else seed, torch.double)


def run_oracle_fp32(name, Cin, Cout, slope, seed=None):
    """The same oracle evaluated in fp32: the "fp32 model" printed next to the kernel."""
    return _oracle(name, Cin, Cout, slope, seed_of(Cin, Cout) if seed is None else seed, torch.float32)


def run_gpu(dev, name, Cin, Cout, slope, split, fused=True, seed=None, transpose=False):
    """The HIP path on the numbers of run_oracle(name, ...), tensors returned on the host.
    fused=True: aggregation + node transform in one kernel on 16-node tiles; fused=32: the same kernels on 32-node tiles
    (geobi_set_tile_rows); fused=False: separate aggregation and GEMM kernels (ops.FUSED = False).
    transpose=True (a symmetric graph): Graph.symmetric is forced to False before ensure_in(), so the in-CSR and pos_in come
    from geobi_csr_transpose instead of geobi_csr_reverse_index."""
    import torch.cuda                                    # noqa: F401
    from geobi_gnn_amd import ops, _lib as lib
    from geobi_gnn_amd.feast_conv import FeaStConv
    ei, n, _ = graph_of_name(name)
    params, x, gout = draw(Cin, Cout, n, seed_of(Cin, Cout) if seed is None else seed)
    was = ops.FUSED
    ops.FUSED = bool(fused)
    try:
        if fused == 32:
            lib.call('geobi_set_tile_rows', 32)
        conv = FeaStConv(Cin, Cout, 9).to(dev)
        conv.load_state_dict(params)
        eid = ei.to(dev)
        if transpose:
            from geobi_gnn_amd.graph import graph_of
            g = graph_of(eid, n)                         # cached on eid: the layer finds this graph
            assert g.symmetric
            g.symmetric, g.rowptr_in, g.col_in, g.pos_in = False, None, None, None
            g.ensure_in()
            assert g.rowptr_in is not g.rowptr_out
        if split:
            xa = x[:, :Cin // 2].contiguous().to(dev).requires_grad_(True)
            xb = x[:, Cin // 2:].contiguous().to(dev).requires_grad_(True)
            out = conv(xa, eid, x2=xb, slope=slope)
        else:
            xa = x.to(dev).requires_grad_(True)
            out = conv(xa, eid, slope=slope)
        out.backward(gout.to(dev))
        torch.cuda.synchronize()
        res = {'out': out.detach().cpu(), 'dx': (torch.cat([xa.grad, xb.grad], 1) if split else xa.grad).cpu()}
        for k, p in conv.named_parameters():
            res['d' + k] = p.grad.cpu()
        return res
    finally:
        ops.FUSED = was
        lib.call('geobi_set_tile_rows', 0)
