"""The dense products path by path: gemm_nn, gemm_tn (csrc/gemm.hip, through geobi_debug_gemm_nn / _tn, which take every
argument of the launchers and report the path a call took) and the fused heads (csrc/head_fused.hip) against the plain
statement of tests/gemm_model.py.

Exact operands need no tolerance: the operands are small integers and the slope a power of two, so every product and
every partial sum is a multiple of 2^-2 far below 2^24 and fp32 holds it exactly in ANY summation order.  The device must
give the fp64 expectation bit for bit -- whatever the tile shape, split, slab count or fold order -- over the WHOLE output
buffers (sentinel or prior content where nothing is addressed), with NaN in every operand element between the logical
width and the leading dimension.  One term dropped, doubled, mis-masked or mis-routed moves an element by >= 0.25.
A short pass with real operands and a derived per-element bound keeps the numerics honest (a reduced-precision product
would pass the integer cases)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import gemm_model as G
from helpers import rel_err

pytestmark = pytest.mark.gpu

SENT = -777.0
NAN = float('nan')
# the tile shapes of gemm_nn by their GEOBI_NN_CFG number: (digits WAVES_M WAVES_N TM TN, BK)
NN_SHAPES = {1: (2211, 32), 2: (2221, 32), 3: (2211, 64), 4: (2222, 16), 5: (4111, 32)}
TN_CASES = {141, 11, 12, 13, 21, 22, 23}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


def _draw(g, real, lo=-3, hi=3):
    if real:
        return lambda *s: torch.randn(*s, generator=g).float().double()          # fp32 values
    return lambda *s: torch.randint(lo, hi + 1, s, generator=g).double()


def _operand(vals, ld, offset, dev):
    """Logical [R, W] values as a device operand of row stride ld whose element [0, 0] sits `offset` floats behind an
    aligned allocation; every float that is not logical is NaN.  -> (tensor that owns the memory, base address)."""
    R, W = vals.shape
    buf = torch.full((offset + max(R, 1) * ld,), NAN)
    if R:
        buf[offset:offset + R * ld].view(R, ld)[:, :W] = vals.float()
    d = buf.to(dev)
    assert d.data_ptr() % 16 == 0
    return d, d.data_ptr() + 4 * offset


def _nan_bytes(nbytes, dev):
    """A workspace of exactly nbytes (rounded up to whole floats for the allocation only), every float NaN."""
    return torch.full(((int(nbytes) + 3) // 4 + 1,), NAN, device=dev)


def _align256(n):
    return (n + 255) // 256 * 256


# ====================================================================================== gemm_nn
def nn(cfg, M, N, K, tb, lda=0, aoff=0, ldb=0, ldc=0, bias='a', slope=0.25, split=False, ws=None, fixed=0, *, fast, shape,
       wide, slices=1, k_chunk=None):
    """A gemm_nn case.  lda / ldb / ldc: floats beyond the logical width; aoff: A starts one float behind an aligned
    address; bias 'n' none, 'a' aligned, 'o' offset by one float; split: the C1 output of the issue (N = 36, split 20,
    ldc 20, ldc1 16); ws: None, 'full' (the size gemm_nn_ws_bytes gives) or a byte count; then the path the case names."""
    return dict(cfg=cfg, M=M, N=N, K=K, tb=tb, lda=lda, aoff=aoff, ldb=ldb, ldc=ldc, bias=bias, slope=slope, split=split,
                ws=ws, fixed=fixed, fast=fast, shape=shape, wide=wide, slices=slices, k_chunk=K if k_chunk is None else k_chunk)


NN_TABLE = [
    # ---- every template x FAST x transB through cfg.  FAST needs lda, ldb, K (and N when B is not transposed) multiples
    # of 4 and aligned bases; the wide store needs ldc and N multiples of 4, an aligned bias or none, no C1, no split-K
    nn(1, 200, 132, 68, 0, fast=1, shape=1, wide=1),
    nn(1, 129, 6, 36, 1, lda=4, ldc=1, bias='o', slope=1.0, fast=1, shape=1, wide=0),
    nn(1, 31, 36, 3, 0, ldc=4, bias='n', fast=0, shape=1, wide=1),                       # K % 4
    nn(1, 129, 68, 132, 1, aoff=1, bias='o', fast=0, shape=1, wide=0),                   # A off alignment
    nn(2, 129, 68, 260, 0, lda=4, ldb=4, ldc=4, bias='n', slope=1.0, fast=1, shape=2, wide=1),
    nn(2, 200, 36, 4, 1, fast=1, shape=2, wide=1),
    nn(2, 1, 132, 36, 0, lda=1, ldc=1, fast=0, shape=2, wide=0),                         # lda % 4
    nn(2, 31, 6, 68, 1, ldb=1, bias='n', fast=0, shape=2, wide=0),                       # ldb % 4
    nn(3, 31, 32, 520, 0, fast=1, shape=3, wide=1),
    nn(3, 200, 68, 132, 1, ldb=4, ldc=1, bias='n', fast=1, shape=3, wide=0),
    nn(3, 129, 6, 260, 0, bias='o', slope=1.0, fast=0, shape=3, wide=0),                 # N % 4, B as it stands
    nn(3, 1, 36, 3, 1, ldc=4, fast=0, shape=3, wide=1),                                  # K % 4
    nn(4, 200, 132, 132, 0, lda=4, fast=1, shape=4, wide=1),
    nn(4, 129, 36, 68, 1, bias='o', fast=1, shape=4, wide=0),
    nn(4, 31, 68, 36, 0, aoff=1, ldc=4, bias='n', slope=1.0, fast=0, shape=4, wide=1),
    nn(4, 200, 132, 260, 1, lda=1, ldb=1, ldc=1, fast=0, shape=4, wide=0),
    nn(5, 200, 32, 36, 0, fast=1, shape=5, wide=1),
    nn(5, 129, 132, 4, 1, ldc=4, bias='n', fast=1, shape=5, wide=1),
    nn(5, 31, 4, 3, 0, ldc=1, fast=0, shape=5, wide=0),
    nn(5, 200, 6, 520, 1, aoff=1, bias='o', slope=1.0, fast=0, shape=5, wide=0),
    # ---- the launcher's own choice at these sizes: 128 x 32 up to N = 32, 64-deep k-tiles from K = 512, else 64 x 64
    nn(0, 1, 4, 4, 0, fast=1, shape=5, wide=1),
    nn(0, 200, 32, 260, 0, fast=1, shape=5, wide=1),
    nn(0, 129, 36, 520, 0, bias='n', fast=1, shape=3, wide=1),
    nn(0, 31, 68, 260, 1, lda=4, fast=1, shape=1, wide=1),
    nn(0, 200, 132, 36, 0, lda=1, ldc=1, fast=0, shape=1, wide=0),
    nn(0, 129, 6, 3, 1, fast=0, shape=5, wide=0),
    # ---- the split output, plain
    nn(0, 31, 36, 68, 0, split=True, fast=1, shape=1, wide=0),
    nn(2, 129, 36, 132, 1, aoff=1, split=True, bias='o', fast=0, shape=2, wide=0),
    nn(4, 200, 36, 36, 0, split=True, bias='n', slope=1.0, fast=1, shape=4, wide=0),
    # ---- split-K.  Automatic: few blocks, K >= 256 and a workspace: K / 128 = 2 slices of 192 (whole 64-wide k-tiles)
    nn(0, 129, 36, 260, 0, ws='full', fast=1, shape=1, wide=0, slices=2, k_chunk=192),
    nn(0, 200, 36, 260, 1, ws='full', split=True, fast=1, shape=1, wide=0, slices=2, k_chunk=192),
    # fixed_slices: ceil(520 / 2) -> 320 per slice; ceil(520 / 4) = 130 -> 192 per slice, which makes THREE slices
    nn(0, 129, 68, 520, 0, ws='full', fixed=2, fast=1, shape=3, wide=0, slices=2, k_chunk=320),
    nn(0, 31, 132, 520, 1, ws='full', fixed=4, bias='n', fast=1, shape=3, wide=0, slices=3, k_chunk=192),
    nn(1, 200, 36, 520, 0, lda=1, ws='full', fixed=2, fast=0, shape=1, wide=0, slices=2, k_chunk=320),
    nn(2, 129, 68, 520, 1, ws='full', fixed=2, bias='o', slope=1.0, fast=1, shape=2, wide=0, slices=2, k_chunk=320),
    nn(4, 129, 132, 520, 0, ws='full', fixed=4, fast=1, shape=4, wide=0, slices=3, k_chunk=192),
    nn(5, 31, 32, 520, 0, ws='full', fixed=2, fast=1, shape=5, wide=0, slices=2, k_chunk=320),
    nn(5, 200, 36, 520, 1, ldb=1, ws='full', fixed=2, split=True, fast=0, shape=5, wide=0, slices=2, k_chunk=320),
    # a workspace one float short of the slices falls back to ONE slice (and may then store wide); so do fixed_slices = 1
    # and a reduction below 256
    nn(0, 129, 36, 260, 0, ws=2 * 129 * 36 * 4 - 4, bias='n', fast=1, shape=1, wide=1),
    nn(0, 129, 68, 520, 0, ws=2 * 129 * 68 * 4 - 4, fixed=2, fast=1, shape=3, wide=1),
    nn(0, 129, 68, 520, 0, ws='full', fixed=1, fast=1, shape=3, wide=1),
    nn(0, 129, 36, 132, 0, ws='full', fast=1, shape=1, wide=1),
]


def _nn_id(c):
    return 'cfg%d-%dx%dx%d-%s%s%s' % (c['cfg'], c['M'], c['N'], c['K'], 'T' if c['tb'] else 'N',
                                     '-split' if c['split'] else '', '-k%d' % c['slices'] if c['slices'] > 1 else '')


def _run_nn(dev, c, seed, real=False):
    """-> (got {C, C1} device buffers, want {C, C1} fp64, plan dict, bound {C, C1} or None)"""
    from geobi_gnn_amd import _lib as L
    g = torch.Generator().manual_seed(seed)
    draw = _draw(g, real)
    M, N, K, tb = c['M'], c['N'], c['K'], c['tb']
    A = draw(M, K)
    B = draw(N, K) if tb else draw(K, N)
    bias = None if c['bias'] == 'n' else draw(N)
    lda, ldb = K + c['lda'], B.shape[1] + c['ldb']
    Ad, Ap = _operand(A, lda, c['aoff'], dev)
    Bd, Bp = _operand(B, ldb, 0, dev)
    bd, bp = (None, None) if bias is None else _operand(bias.view(1, N), N, 1 if c['bias'] == 'o' else 0, dev)
    if c['split']:
        assert N == 36
        split, ldc, ldc1 = 20, 20, 16
        C1p = torch.full((M * ldc1,), SENT)
    else:
        split, ldc, ldc1, C1p = 0, N + c['ldc'], 0, None
    Cp = torch.full((M * ldc,), SENT)
    Cd, C1d = Cp.to(dev), None if C1p is None else C1p.to(dev)
    ws_bytes = 0 if c['ws'] is None else (_align256(8 * M * N * 4) + 256 if c['ws'] == 'full' else c['ws'])
    ws = _nan_bytes(ws_bytes, dev) if ws_bytes else None
    plan = (ctypes.c_int64 * 8)()
    L.call('geobi_debug_gemm_nn', Ap, lda, Bp, ldb, tb, L.ptr(Cd), ldc, M, N, K, bp, c['slope'], L.ptr(C1d), split, ldc1,
           L.ptr(ws), ws_bytes, c['fixed'], c['cfg'], plan, L.stream())
    torch.cuda.synchronize()
    want = dict(zip(('C', 'C1'), G.nn_expected(A, B, tb, Cp, ldc, bias, c['slope'], C1p, split, ldc1)))
    bound = None
    if real:
        zero = lambda t: None if t is None else torch.zeros_like(t)
        sabs = G.nn_expected(A.abs(), B.abs(), tb, zero(Cp), ldc, None if bias is None else bias.abs(), 1.0, zero(C1p), split,
                             ldc1)
        bound = {k: None if s is None else (K + 16) * 2.0 ** -24 * s for k, s in zip(('C', 'C1'), sabs)}
    keys = ('fast', 'shape', 'tile', 'bk', 'slices', 'k_chunk', 'wide', 'reduce')
    return {'C': Cd, 'C1': C1d}, want, dict(zip(keys, list(plan))), bound


def _check_nn_plan(c, p):
    tile, bk = NN_SHAPES[c['shape']]
    want = dict(fast=c['fast'], shape=c['shape'], tile=tile, bk=bk, slices=c['slices'], k_chunk=c['k_chunk'], wide=c['wide'],
                reduce=int(c['slices'] > 1))
    assert p == want, 'the case did not take the path it names: %r, wanted %r' % (p, want)


@pytest.fixture(scope='module')
def nn_runs(dev):
    """Every case of NN_TABLE, launched once: the case tests and the coverage test read from here."""
    return [_run_nn(dev, c, seed=100 + k) for k, c in enumerate(NN_TABLE)]


@pytest.mark.parametrize('k', range(len(NN_TABLE)), ids=[_nn_id(c) for c in NN_TABLE])
def test_gemm_nn_exact(nn_runs, k):
    got, want, plan, _ = nn_runs[k]
    _check_nn_plan(NN_TABLE[k], plan)
    assert G.mismatches(got, want) == []


def test_gemm_nn_table_covers_every_path(nn_runs):
    """Keeps the table from rotting when a threshold moves: every tile shape as the FAST and the bounds-checked kernel,
    with B as it stands and transposed; both store forms; split-K on and off; the split output plain and under split-K."""
    plans = [(r[2], c) for r, c in zip(nn_runs, NN_TABLE)]
    seen = {(p['shape'], p['fast'], c['tb']) for p, c in plans}
    assert seen == {(s, f, t) for s in NN_SHAPES for f in (0, 1) for t in (0, 1)}, sorted(seen)
    assert {p['wide'] for p, _ in plans} == {0, 1}
    assert {p['reduce'] for p, _ in plans} == {0, 1}
    assert {(p['reduce'], int(c['split'])) for p, c in plans} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(s, p['reduce']) for p, _ in plans for s in [p['shape']]} >= {(s, 1) for s in NN_SHAPES}   # the `partial` branch


# ====================================================================================== gemm_tn
def tn(mode, M, I, J, pad=0, aoff=0, ldb=0, acc=0, ones_row=False, ones_col=False, sum_row=False, Cin=0, Cout=0, col0=0,
       c2=True, c34=True, *, case, slabs=None, bias_blocks=0):
    """A gemm_tn case.  I, J: the logical output size, implicit last row / column included; pad: lda minus A's data
    columns; extra_row / extra_col of the plain map follow the implicit row / column; case: the GEOBI_TN dispatch case
    (100 vector-A + 10 TI + TJ) the case names, slabs: blocks along the reduction."""
    return dict(mode=mode, M=M, I=I, J=J, pad=pad, aoff=aoff, ldb=ldb, acc=acc, ones_row=ones_row, ones_col=ones_col,
                sum_row=sum_row, Cin=Cin, Cout=Cout, col0=col0, c2=c2, c34=c34, case=case, slabs=slabs, bias_blocks=bias_blocks)


TN_MS = (0, 1, 2, 7, 8, 9, 255, 256, 257, 2500)
# (I, J, lda - data columns, ones_row, dispatch case, tiles_i x tiles_j is checked from the plan for the last one)
TN_SHAPES = [(96, 40, 0, False, 141), (97, 40, 0, True, 141), (9, 20, 3, False, 11), (24, 33, 0, False, 12),
             (24, 70, 0, False, 13), (40, 32, 0, False, 21), (40, 64, 0, False, 22), (40, 130, 0, False, 22),
             (40, 70, 0, False, 23), (200, 130, 3, False, 22)]


def _slabs(M):
    return max(1, (M + 255) // 256)           # at least 4 waves x 64 rows per block; these shapes never reach the cap


def _tn_table():
    t = []
    for s, (I, J, pad, orow, case) in enumerate(TN_SHAPES):
        # every reduction length on every shape (257: one slice partial and one empty; 2500: 10 slabs, the four-way fold of
        # the reduce kernel wraps; 0: zeros, or the prior content when accumulating), alternately overwriting and adding
        for m, M in enumerate(TN_MS):
            t.append(tn(G.PLAIN, M, I, J, pad, ldb=(s + m) % 2, acc=(s + m) % 2, ones_row=orow, case=case, slabs=_slabs(M)))
        # the ones column (-> C2) as the last of the J columns, on every shape
        for m, M in enumerate((0, 9, 257, 2500)):
            t.append(tn(G.PLAIN, M, I - orow, J, pad, ldb=m % 2, acc=(s + m + 1) % 2, ones_col=True, case=case,
                        slabs=_slabs(M)))
    # the column-sums row: beside the vector-A kernel and beside a scalar-A one; A off alignment turns 141 into 22
    for M in (1, 257, 2500):
        t.append(tn(G.PLAIN, M, 97, 40, sum_row=True, acc=M % 2, case=141, slabs=_slabs(M)))
        t.append(tn(G.PLAIN, M, 41, 64, sum_row=True, acc=M % 2, case=22, slabs=_slabs(M)))
    t.append(tn(G.PLAIN, 257, 96, 40, aoff=1, case=22, slabs=2))
    t.append(tn(G.PLAIN, 257, 96, 40, pad=1, case=22, slabs=2))
    # ---- the output maps at model-like sizes, overwriting and adding
    for acc in (0, 1):
        # lin.weight.grad / bias.grad from [z | 1]^T g: z has 9 Cin columns padded to a multiple of 4
        t.append(tn(G.LIN_UNPACK, 300, 57, 32, acc=acc, ones_row=True, Cin=6, Cout=32, case=21, slabs=2))
        t.append(tn(G.LIN_UNPACK, 2500, 289, 32, acc=acc, ones_row=True, Cin=32, Cout=32, case=141, slabs=10))
        # du / dc from [dp | dcs]^T [x | 1]
        t.append(tn(G.DU_DC, 300, 24, 7, acc=acc, ones_col=True, case=11, slabs=2))
        t.append(tn(G.DU_DC, 2500, 24, 33, acc=acc, ones_col=True, c2=bool(acc), case=12, slabs=10))
        # [x | sums]^T r': whole input / first half / second half (col0 = 16: no sums row), u and c gradients present and
        # absent, Cout = 20: a partial last bias block
        t.append(tn(G.RPRIME, 2500, 33, 9 * 32 + 24, acc=acc, sum_row=True, Cin=32, Cout=32, case=12, slabs=10, bias_blocks=4))
        t.append(tn(G.RPRIME, 300, 33, 9 * 20 + 24, acc=acc, sum_row=True, Cin=32, Cout=20, case=12, slabs=2, bias_blocks=3))
        t.append(tn(G.RPRIME, 300, 17, 9 * 20 + 24, acc=acc, sum_row=True, Cin=32, Cout=20, c34=False, case=12, slabs=2,
                    bias_blocks=3))
        t.append(tn(G.RPRIME, 300, 17, 9 * 32 + 24, acc=acc, sum_row=True, Cin=32, Cout=32, c2=False, case=12, slabs=2))
        t.append(tn(G.RPRIME, 2500, 16, 9 * 32 + 24, acc=acc, Cin=32, Cout=32, col0=16, c2=False, c34=bool(acc), case=12,
                    slabs=10))
    return t


TN_TABLE = _tn_table()


def _tn_id(c):
    extras = ('+1row' if c['ones_row'] else '') + ('+1col' if c['ones_col'] else '') + ('+sums' if c['sum_row'] else '')
    return '%s-%dx%d-m%d%s%s-c%d' % (('plain', 'lin', 'dudc', 'rprime')[c['mode']], c['I'], c['J'], c['M'], extras,
                                     '-acc' if c['acc'] else '', c['col0'])


def _run_tn(dev, c, seed, real=False):
    """-> (got {C, C2, C3, C4} device buffers, want fp64, plan dict, bound or None)"""
    from geobi_gnn_amd import _lib as L
    g = torch.Generator().manual_seed(seed)
    draw = _draw(g, real)
    mode, M, I, J = c['mode'], c['M'], c['I'], c['J']
    Id, Jd = I - int(c['ones_row'] or c['sum_row']), J - int(c['ones_col'])
    A, B = draw(M, Id), draw(M, Jd)
    lda, ldb = Id + c['pad'], Jd + c['ldb']
    Ad, Ap = _operand(A, lda, c['aoff'], dev)
    Bd, Bp = _operand(B, ldb, 0, dev)
    prior = (lambda n: _draw(g, False)(n)) if c['acc'] else (lambda n: torch.full((n,), SENT).double())
    extra_row = int(mode in (G.PLAIN, G.RPRIME) and (c['ones_row'] or c['sum_row']))
    extra_col = int(mode == G.PLAIN and c['ones_col'])
    Cin, Cout = c['Cin'], c['Cout']
    ldc = 0
    if mode == G.PLAIN:
        # two floats of padding per row, one row and one element that nothing addresses
        ldc = J - extra_col + 2
        P = {'C': prior((I - extra_row + 1) * ldc), 'C2': prior((J if extra_row else I) + 1) if extra_row or extra_col else None}
    elif mode == G.LIN_UNPACK:
        P = {'C': prior(G.H * Cout * Cin + 1), 'C2': prior(Cout + 1)}
    elif mode == G.DU_DC:
        ldc = J - 1 + 3                                          # du [9, Cin] with this operand's half at its columns
        P = {'C': prior(G.H * ldc), 'C2': prior(G.H + 1) if c['c2'] else None}
    else:
        P = {'C': prior(G.H * Cout * Cin + 1), 'C2': prior(Cout + 1) if c['c2'] and extra_row else None,
             'C3': prior(G.H * Cin + 1) if c['c34'] else None, 'C4': prior(G.H + 1) if c['c34'] and extra_row else None}
    P = {k: P.get(k) for k in ('C', 'C2', 'C3', 'C4')}
    D = {k: None if v is None else v.float().to(dev) for k, v in P.items()}
    ws_bytes = L.lib().geobi_gemm_tn_ws_bytes(I, J, M)
    ws = _nan_bytes(ws_bytes, dev)
    plan = (ctypes.c_int64 * 8)()
    L.call('geobi_debug_gemm_tn', Ap, lda, Bp, ldb, M, I, J, I - 1 if c['ones_row'] else -1, J - 1 if c['ones_col'] else -1,
           I - 1 if c['sum_row'] else -1, mode, L.ptr(D['C']), ldc, L.ptr(D['C2']), L.ptr(D['C3']), L.ptr(D['C4']), Cin, Cout,
           c['col0'], extra_row, extra_col, c['acc'], L.ptr(ws), ws_bytes, plan, L.stream())
    torch.cuda.synchronize()
    kw = dict(ldc=ldc, Cin=Cin, Cout=Cout, col0=c['col0'], extra_row=extra_row, extra_col=extra_col, ones_row=c['ones_row'],
              ones_col=c['ones_col'], sum_row=c['sum_row'])
    want = G.tn_expected(mode, A, B, P['C'], C2=P['C2'], C3=P['C3'], C4=P['C4'], accumulate=c['acc'], **kw)
    bound = None
    if real:
        assert not c['acc']
        Z = {k: None if v is None else torch.zeros_like(v) for k, v in P.items()}
        sabs = G.tn_expected(mode, A.abs(), B.abs(), Z['C'], C2=Z['C2'], C3=Z['C3'], C4=Z['C4'], **kw)
        # reduction length: the rows; nine heads of them for the bias gradient of the r' map
        n = {k: (G.H * M if (mode == G.RPRIME and k == 'C2') else M) for k in sabs}
        bound = {k: None if s is None else (n[k] + 16) * 2.0 ** -24 * s for k, s in sabs.items()}
    keys = ('va', 'ti', 'tj', 'tiles_i', 'tiles_j', 'slabs', 'm_per_slice', 'bias_blocks')
    return D, want, dict(zip(keys, list(plan))), bound


def _check_tn_plan(c, p):
    assert p['va'] * 100 + p['ti'] * 10 + p['tj'] == c['case'], 'the case did not take the path it names: %r' % (p,)
    I_mma = c['I'] - int(c['sum_row'])
    assert p['tiles_i'] == -(-I_mma // (32 * p['ti'])) and p['tiles_j'] == -(-c['J'] // (32 * p['tj']))
    if c['slabs'] is not None:
        assert p['slabs'] == c['slabs'], p
    assert 4 * p['slabs'] * p['m_per_slice'] >= c['M'] and p['m_per_slice'] % 8 == 0
    assert p['bias_blocks'] == c['bias_blocks']


@pytest.fixture(scope='module')
def tn_runs(dev):
    """Every case of TN_TABLE, launched once, each with a workspace of exactly geobi_gemm_tn_ws_bytes(I, J, M) bytes."""
    return [_run_tn(dev, c, seed=500 + k) for k, c in enumerate(TN_TABLE)]


@pytest.mark.parametrize('k', range(len(TN_TABLE)), ids=[_tn_id(c) for c in TN_TABLE])
def test_gemm_tn_exact(tn_runs, k):
    got, want, plan, _ = tn_runs[k]
    _check_tn_plan(TN_TABLE[k], plan)
    assert G.mismatches(got, want) == []


def test_gemm_tn_table_covers_every_path(tn_runs):
    plans = [(r[2], c) for r, c in zip(tn_runs, TN_TABLE)]
    assert {p['va'] * 100 + p['ti'] * 10 + p['tj'] for p, _ in plans} == TN_CASES
    # several tiles both ways, ten slabs, a partial bias block, every map overwriting and adding
    assert any(p['tiles_i'] > 1 and p['tiles_j'] > 1 for p, _ in plans)
    assert {p['slabs'] for p, _ in plans} >= {1, 2, 10}
    assert {p['bias_blocks'] for p, _ in plans} >= {0, 3, 4}
    assert {(c['mode'], c['acc']) for _, c in plans} == {(m, a) for m in range(4) for a in (0, 1)}
    assert {(p['va'], int(c['sum_row'])) for p, c in plans} >= {(1, 1), (0, 1)}
    assert {(p['va'], int(c['ones_row'])) for p, c in plans} >= {(1, 1), (0, 1)}


# ====================================================================================== real operands
# Short reductions make the bound sharp: a product rounded to 11 bits errs by about 2^-11 sum|ab| / sqrt(n), which is
# 2^13 / ((n + 16) sqrt(n)) of the bound -- 20 x the bound at n = 36, twice at n = 257, but only 0.07 at n = 2 500.  So
# every kernel runs a short case; the long ones add the slice and slab folds.
NN_REAL = [c for c in NN_TABLE if (c['cfg'], c['M'], c['N'], c['K']) in
           {(1, 200, 132, 68), (2, 200, 36, 4), (3, 200, 68, 132), (4, 129, 36, 68), (5, 200, 32, 36)}]
NN_REAL += [c for c in NN_TABLE if c['slices'] == 3 and c['cfg'] == 0]
TN_REAL = [tn(G.PLAIN, 257, 97, 40, ones_row=True, case=141, slabs=2),
           tn(G.PLAIN, 2500, 200, 130, pad=3, case=22, slabs=10),
           tn(G.RPRIME, 257, 33, 9 * 32 + 24, sum_row=True, Cin=32, Cout=32, case=12, slabs=2, bias_blocks=4),
           tn(G.PLAIN, 2500, 97, 40, ones_row=True, case=141, slabs=10),
           tn(G.PLAIN, 9, 200, 130, pad=3, case=22, slabs=1),
           tn(G.RPRIME, 2500, 33, 9 * 32 + 24, sum_row=True, Cin=32, Cout=32, case=12, slabs=10, bias_blocks=4)]


def _ratio(got, want, bound):
    """max over every element of |got - want| / bound; elements nothing addresses have bound 0 and must be equal."""
    worst = 0.0
    for k, w in want.items():
        if w is None:
            continue
        d = (got[k].detach().cpu().double().reshape(-1) - w).abs()
        b = bound[k]
        assert bool((d[b == 0] == 0).all()), k
        worst = max(worst, float((d[b > 0] / b[b > 0]).max()))
    return worst


def test_gemm_real_operands_within_the_summation_bound(dev):
    """Standard normal operands, fp64 reference on the fp32 values, PER ELEMENT:
        |got - ref| <= (n + 16) 2^-24 (sum_k |a_k b_k| + |bias|),   n = the reduction length
    -- the any-order summation bound of n fp32 additions of exact products' roundings (unit roundoff 2^-24), 16 more for
    the bias add, the slope, and the slice and slab folds; slope <= 1 makes the epilogue 1-Lipschitz.  Nothing is measured
    into the bar.  One case per gemm_nn tile shape (K = 4 .. 132), one with three split-K slices (K = 520); gemm_tn through
    the vector-A kernel, the 2 x 2 kernel and the r' map, each over a short reduction (9 or 257 rows) and over 2 500 rows
    in ten slabs.  The largest ratio to the bound is printed; seen on the MI355X: gemm_nn 0.099, gemm_tn 0.119."""
    assert len(NN_REAL) == 6
    worst = {'gemm_nn': 0.0, 'gemm_tn': 0.0}
    for k, c in enumerate(NN_REAL):
        got, want, plan, bound = _run_nn(dev, c, seed=900 + k, real=True)
        _check_nn_plan(c, plan)
        worst['gemm_nn'] = max(worst['gemm_nn'], _ratio(got, want, bound))
    for k, c in enumerate(TN_REAL):
        got, want, plan, bound = _run_tn(dev, c, seed=950 + k, real=True)
        _check_tn_plan(c, plan)
        worst['gemm_tn'] = max(worst['gemm_tn'], _ratio(got, want, bound))
    print('largest |got - ref| / bound: gemm_nn %.4f, gemm_tn %.4f' % (worst['gemm_nn'], worst['gemm_tn']))
    assert worst['gemm_nn'] <= 1.0 and worst['gemm_tn'] <= 1.0, worst


def test_gemm_is_deterministic(dev):
    """Ten slabs folded by tn_reduce_kernel, three split-K slices folded by splitk_reduce_kernel: the same bits twice."""
    for run, c in ((_run_tn, TN_REAL[1]), (_run_nn, NN_REAL[-1])):
        a, b = run(dev, c, seed=7, real=True), run(dev, c, seed=7, real=True)
        assert a[2] == b[2] and a[2]['slabs' if run is _run_tn else 'slices'] > 1
        for k, v in a[0].items():
            assert v is None or torch.equal(v, b[0][k])


# ====================================================================================== heads
def _head_operands(Cin, K, nout, N, seed, face=False):
    g = torch.Generator().manual_seed(seed)
    d = _draw(g, False, -2, 2)
    t = dict(x=d(N, Cin), w1=d(K, Cin), b1=d(K), w2=d(nout, K), b2=d(nout), resid=d(N, 6), gout=d(N, 3))
    # depth_direction: signed unit axes
    axis = torch.randint(0, 3, (N,), generator=g)
    sign = torch.randint(0, 2, (N,), generator=g).double() * 2 - 1
    t['dd'] = F.one_hot(axis, 3).double() * sign.unsqueeze(1)
    t['prior'] = dict(dw1=d(K, Cin), db1=d(K), dw2=d(nout, K), db2=d(nout))
    return t


def _head_reference(t, nout, mode, slope):
    p = {k: t[k].clone().requires_grad_(True) for k in ('x', 'w1', 'b1', 'w2', 'b2')}
    raw = F.linear(F.leaky_relu(F.linear(p['x'], p['w1'], p['b1']), slope), p['w2'], p['b2'])
    if mode == 0:
        out = (raw * t['dd'] if nout == 1 else raw) + t['resid'][:, :3]
    else:
        out = F.normalize(raw, dim=1)
    out.backward(t['gout'])
    return dict(raw=raw.detach(), out=out.detach(), dx=p['x'].grad, dw1=p['w1'].grad, db1=p['b1'].grad, dw2=p['w2'].grad,
                db2=p['b2'].grad)


def _head_device(dev, t, Cin, K, nout, N, mode, slope, accumulate, generic):
    from geobi_gnn_amd import _lib as L
    f = lambda v: v.float().contiguous().to(dev)
    x, w1, b1, w2, b2, resid, gout, dd = (f(t[k]) for k in ('x', 'w1', 'b1', 'w2', 'b2', 'resid', 'gout', 'dd'))
    h = torch.full((N, K), NAN, device=dev) if generic else None
    raw, out = torch.full((N, nout), NAN, device=dev), torch.full((N, 3), NAN, device=dev)
    L.call('geobi_head_fwd', L.ptr(x), Cin, N, L.ptr(w1), L.ptr(b1), K, L.ptr(w2), L.ptr(b2), nout, slope, mode, L.ptr(dd),
           L.ptr(resid), 6, L.ptr(h), L.ptr(raw), L.ptr(out), L.stream())
    got = dict(raw=raw, out=out)
    if accumulate is None:
        torch.cuda.synchronize()
        return got
    grads = {k: (f(t['prior'][k]) if accumulate else torch.full(t['prior'][k].shape, NAN, device=dev))
             for k in ('dw1', 'db1', 'dw2', 'db2')}
    dx = torch.full((N, Cin), NAN, device=dev)
    ws_bytes = L.lib().geobi_head_bwd_ws_bytes(N, Cin, K)
    ws = _nan_bytes(ws_bytes, dev)
    L.call('geobi_head_bwd', L.ptr(x), Cin, N, L.ptr(w1), L.ptr(b1), K, L.ptr(w2), nout, slope, mode, L.ptr(dd), L.ptr(h),
           L.ptr(raw), L.ptr(gout), L.ptr(dx), L.ptr(grads['dw1']), L.ptr(grads['db1']), L.ptr(grads['dw2']),
           L.ptr(grads['db2']), accumulate, L.ptr(ws), ws_bytes, L.stream())
    torch.cuda.synchronize()
    got.update(grads, dx=dx)
    return got


def _head_want(t, ref, accumulate):
    want = dict(ref)
    if accumulate:
        for k in ('dw1', 'db1', 'dw2', 'db2'):
            want[k] = ref[k] + t['prior'][k]
    return want


HEAD_N = 8229      # 258 tiles of 32 nodes for the 256 persistent blocks of the backward: two blocks take a second tile, and
                   # the last tile holds 5 nodes


@pytest.fixture(scope='module')
def head_refs():
    """Operands and fp64 autograd results of the exact head cases, shared by the tests below and left unchanged."""
    refs = {}
    for nout in (3, 1):
        t = _head_operands(32, 1024, nout, HEAD_N, seed=nout)
        refs[nout] = (t, _head_reference(t, nout, 0, 0.5))
    return refs


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('nout', [3, 1])
def test_fused_vertex_head_exact_over_258_tiles(dev, head_refs, nout, accumulate):
    """Integer operands in [-2, 2], slope 0.5, depth directions that are signed unit axes: raw, out, dx and the four
    parameter gradients bit for bit -- the sums a persistent block carries from its first tile to its second (dW1, dW2, db1
    in LDS, db2 in registers), the 5-node last tile, the fold of the 256 per-block slabs; with accumulate on top of integer
    prior gradients.  Largest sum of |terms| of any output: 87 517.5 (dW2), in steps of 0.5: far below 2^23."""
    t, ref = head_refs[nout]
    got = _head_device(dev, t, 32, 1024, nout, HEAD_N, 0, 0.5, accumulate, generic=False)
    assert G.mismatches(got, _head_want(t, ref, accumulate)) == []


@pytest.mark.parametrize('nout', [3, 1])
def test_fused_head_forward_split_precision_exact(dev, head_refs, nout):
    """geobi_set_head_precision(1): the operands are exactly representable in bf16 (their second and third pieces are 0),
    so the six-product form must give the fp32 form's bits."""
    from geobi_gnn_amd import _lib as L
    t, ref = head_refs[nout]
    try:
        assert L.lib().geobi_set_head_precision(1) == 0
        got = _head_device(dev, t, 32, 1024, nout, HEAD_N, 0, 0.5, None, generic=False)
    finally:
        L.lib().geobi_set_head_precision(0)
    assert G.mismatches(got, {k: ref[k] for k in ('raw', 'out')}) == []


def test_fused_face_head_over_258_tiles(dev):
    """The face head on the same operands: raw is exact; the normalisation is not, so out and what follows from its
    gradient meet the 1e-5 bar of test_head_all_paths (of each tensor's maximum)."""
    t = _head_operands(32, 1024, 3, HEAD_N, seed=5)
    ref = _head_reference(t, 3, 1, 0.5)
    got = _head_device(dev, t, 32, 1024, 3, HEAD_N, 1, 0.5, 0, generic=False)
    assert G.mismatches(got, {'raw': ref['raw']}) == []
    errs = {k: rel_err(got[k].cpu(), ref[k]) for k in ('out', 'dx', 'dw1', 'db1', 'dw2', 'db2')}
    print('face head, %d nodes: %s' % (HEAD_N, ' '.join('%s %.2e' % kv for kv in errs.items())))
    assert max(errs.values()) < 1e-5, errs


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('nout', [3, 1])
def test_generic_vertex_head_exact(dev, nout, accumulate):
    """(Cin, K) = (16, 512), 300 nodes, the hidden activation in memory: gemm_nn with nn.Linear's transposed weight and
    its bias / slope epilogue, and head_bwd's two gemm_tn products with the ones column (dW2 | db2 through the scalar-A
    kernel, dW1 | db1 through the vector-A kernel)."""
    N = 300
    t = _head_operands(16, 512, nout, N, seed=10 + nout)
    ref = _head_reference(t, nout, 0, 0.5)
    got = _head_device(dev, t, 16, 512, nout, N, 0, 0.5, accumulate, generic=True)
    assert G.mismatches(got, _head_want(t, ref, accumulate)) == []
