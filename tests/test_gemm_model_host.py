"""tests/gemm_model.py -- the statement tests/test_gpu_gemm.py compares gemm_nn / gemm_tn with, bit for bit -- pinned on
facts that do not come from csrc/gemm.hip: torch.autograd's gradients of the layers the output maps serve, hand-computed
2-3 element cases, and planted faults that the whole-buffer comparison must report.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import gemm_model as G

SENT = -777.0


def _ints(g, *shape, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


# ------------------------------------------------------------------------------ gemm_nn
@pytest.mark.parametrize('transB', [0, 1])
def test_nn_is_linear_plus_leaky_relu_and_keeps_the_padding(transB):
    g = torch.Generator().manual_seed(transB)
    M, N, K, ldc = 5, 7, 6, 9
    A, W, b = _ints(g, M, K), _ints(g, N, K), _ints(g, N)
    want = F.leaky_relu(F.linear(A, W, b), 0.25)
    C, C1 = G.nn_expected(A, W if transB else W.t().contiguous(), transB, torch.full((M * ldc,), SENT), ldc, b, 0.25)
    assert C1 is None
    assert torch.equal(C.view(M, ldc)[:, :N], want) and bool((C.view(M, ldc)[:, N:] == SENT).all())
    assert bool((want < 0).any()) and bool((want > 0).any())
    # split output: columns >= split in the second buffer, each with its own leading dimension
    C, C1 = G.nn_expected(A, W, 1, torch.full((M * 5,), SENT), 5, b, 0.25, torch.full((M * 4,), SENT), 4, 4)
    assert torch.equal(C.view(M, 5)[:, :4], want[:, :4]) and torch.equal(C1.view(M, 4)[:, :3], want[:, 4:])
    assert bool((C.view(M, 5)[:, 4:] == SENT).all()) and bool((C1.view(M, 4)[:, 3:] == SENT).all())


# ------------------------------------------------------------------------------ gemm_tn: the maps against autograd
def test_tn_plain_with_extra_col_is_dw_db_of_a_linear():
    """dW = g^T x, db = g^T 1 of y = x W^T + b: A = g [n, out], B = [x | 1] (head_bwd's two products)."""
    g = torch.Generator().manual_seed(1)
    n, cin, cout = 11, 5, 3
    x, gy = _ints(g, n, cin), _ints(g, n, cout)
    lin = torch.nn.Linear(cin, cout).double()
    lin(x).backward(gy)
    ldc = cin + 2
    out = G.tn_expected(G.PLAIN, gy, x, torch.full((cout * ldc,), SENT), ldc, C2=torch.full((cout + 1,), SENT),
                        extra_col=1, ones_col=True)
    assert torch.equal(out['C'].view(cout, ldc)[:, :cin], lin.weight.grad)
    assert bool((out['C'].view(cout, ldc)[:, cin:] == SENT).all())
    assert torch.equal(out['C2'][:cout], lin.bias.grad) and float(out['C2'][cout]) == SENT
    # the same through extra_row: A = [x | 1], B = g gives dW^T and db
    out = G.tn_expected(G.PLAIN, x, gy, torch.full((cin * cout,), SENT), cout, C2=torch.full((cout,), SENT), extra_row=1,
                        ones_row=True)
    assert torch.equal(out['C'].view(cin, cout), lin.weight.grad.t()) and torch.equal(out['C2'], lin.bias.grad)
    # sum_row states the same numbers as ones_row
    out2 = G.tn_expected(G.PLAIN, x, gy, torch.full((cin * cout,), SENT), cout, C2=torch.full((cout,), SENT), extra_row=1,
                         sum_row=True)
    assert torch.equal(out2['C'], out['C']) and torch.equal(out2['C2'], out['C2'])


@pytest.mark.parametrize('cin,cout', [(6, 4), (3, 5)])
def test_tn_lin_unpack_is_the_gradient_of_the_stacked_linear(cin, cout):
    """FeaStConv: out[n, o] = sum_h q[n, h] (lin x)[n, h Cout + o] + bias[o].  With z[n, h Cin + k] = q[n, h] x[n, k] (the
    9-head stacking, padded to a multiple of 4 columns) the map of [z | 1]^T g is lin.weight.grad and bias.grad."""
    g = torch.Generator().manual_seed(cin)
    n = 7
    x, q, gy = _ints(g, n, cin), _ints(g, n, G.H), _ints(g, n, cout)
    W = _ints(g, G.H * cout, cin).requires_grad_(True)
    b = _ints(g, cout).requires_grad_(True)
    y = F.linear(x, W).view(n, G.H, cout)
    ((q.unsqueeze(2) * y).sum(1) + b).backward(gy)
    kp = (G.H * cin + 3) // 4 * 4
    z = torch.full((n, kp), 5.0)                       # padding columns hold something: their rows must go nowhere
    z[:, :G.H * cin] = (q.unsqueeze(2) * x.unsqueeze(1)).reshape(n, G.H * cin)
    out = G.tn_expected(G.LIN_UNPACK, z, gy, torch.full((G.H * cout * cin,), SENT), C2=torch.full((cout,), SENT), Cin=cin,
                        Cout=cout, ones_row=True)
    assert torch.equal(out['C'].view(G.H * cout, cin), W.grad) and torch.equal(out['C2'], b.grad)


def test_tn_du_dc_by_hand():
    """A = [dp (9) | pad (3) | dcs (9) | pad (3)], B = [x | 1]: du[h, k] = sum_m dp[m, h] x[m, k], dc[h] = sum_m dcs[m, h];
    split input: the second half lands at column Ca of du and gives no dc."""
    A = torch.zeros(2, 24)
    A[0, 2], A[1, 2] = 3.0, -1.0            # dp, head 2
    A[0, 12 + 4], A[1, 12 + 4] = 2.0, 5.0   # dcs, head 4
    A[:, 9:12], A[:, 21:] = 100.0, 100.0    # padding rows: never routed
    xa, xb = torch.tensor([[1.0, 2.0], [3.0, 4.0]]), torch.tensor([[7.0], [-2.0]])
    du, dc = torch.full((27,), SENT), torch.full((9,), SENT)
    out = G.tn_expected(G.DU_DC, A, xa, du, 3, C2=dc, ones_col=True)
    want_du = torch.full((9, 3), SENT).double()
    want_du[:, :2] = 0
    want_du[2, 0], want_du[2, 1] = 3 * 1 - 1 * 3, 3 * 2 - 1 * 4
    want_dc = torch.zeros(9).double()
    want_dc[4] = 7
    assert torch.equal(out['C'].view(9, 3), want_du) and torch.equal(out['C2'], want_dc)
    out2 = G.tn_expected(G.DU_DC, A, xb, out['C'][2:], 3, C2=None, ones_col=True)     # C = du + Ca
    want_du[:, 2] = 0
    want_du[2, 2] = 3 * 7 + 1 * 2
    assert torch.equal(torch.cat([out['C'][:2], out2['C']]).view(9, 3), want_du) and out2['C2'] is None


def test_tn_rprime_by_hand():
    """[x | sums]^T [r (9 Cout) | dp 12 | dcs 12] with Cin = 2 input channels in two halves and Cout = 1."""
    r = torch.zeros(2, 9 + 24)
    r[0, 3], r[1, 3] = 5.0, 7.0             # r, head 3
    r[0, 8] = 2.0                            # r, head 8
    r[1, 9 + 2] = 4.0                        # dp, head 2
    r[0, 21 + 4], r[1, 21 + 4] = 1.0, 2.0    # dcs, head 4
    r[:, 18:21], r[:, 30:] = 100.0, 100.0    # padding columns: never routed
    xa, xb = torch.tensor([[1.0], [2.0]]), torch.tensor([[3.0], [-1.0]])
    prior = lambda n: torch.full((n,), SENT)
    out = G.tn_expected(G.RPRIME, xa, r, prior(18), C2=prior(1), C3=prior(18), C4=prior(9), Cin=2, Cout=1, col0=0,
                        extra_row=1, sum_row=True)
    dlin = torch.full((9, 2), SENT).double(); dlin[:, 0] = 0; dlin[3, 0] = 19; dlin[8, 0] = 2
    du = torch.full((9, 2), SENT).double(); du[:, 0] = 0; du[2, 0] = 8
    dc = torch.zeros(9).double(); dc[4] = 3
    assert torch.equal(out['C'].view(9, 2), dlin) and torch.equal(out['C3'].view(9, 2), du)
    assert torch.equal(out['C4'], dc) and torch.equal(out['C2'], torch.tensor([14.0]).double())   # 5 + 7 + 2
    # second half: col0 = 1, no sums row, no bias / c gradient, on top of the first call's buffers
    out2 = G.tn_expected(G.RPRIME, xb, r, out['C'], C3=out['C3'], Cin=2, Cout=1, col0=1)
    dlin[:, 1] = 0; dlin[3, 1] = 15 - 7; dlin[8, 1] = 6
    du[:, 1] = 0; du[2, 1] = -4
    assert torch.equal(out2['C'].view(9, 2), dlin) and torch.equal(out2['C3'].view(9, 2), du)
    assert out2['C2'] is None and out2['C4'] is None
    # absent C3 / C4: their elements go nowhere
    out3 = G.tn_expected(G.RPRIME, xa, r, prior(18), C2=prior(1), Cin=2, Cout=1, extra_row=1, sum_row=True)
    assert torch.equal(out3['C'], out['C']) and out3['C3'] is None and torch.equal(out3['C2'], out['C2'])


def test_tn_accumulate_adds_and_overwrite_keeps_what_is_not_addressed():
    g = torch.Generator().manual_seed(3)
    A, B = _ints(g, 6, 4), _ints(g, 6, 3)
    prior = _ints(g, 4 * 5)
    over = G.tn_expected(G.PLAIN, A, B, prior, 5)['C'].view(4, 5)
    acc = G.tn_expected(G.PLAIN, A, B, prior, 5, accumulate=1)['C'].view(4, 5)
    P = A.t() @ B
    assert torch.equal(over[:, :3], P) and torch.equal(over[:, 3:], prior.view(4, 5)[:, 3:])
    assert torch.equal(acc[:, :3], P + prior.view(4, 5)[:, :3]) and torch.equal(acc[:, 3:], prior.view(4, 5)[:, 3:])
    # no rows: zeros, or the prior content
    E = torch.zeros(0, 4), torch.zeros(0, 3)
    assert bool((G.tn_expected(G.PLAIN, *E, prior, 5)['C'].view(4, 5)[:, :3] == 0).all())
    assert torch.equal(G.tn_expected(G.PLAIN, *E, prior, 5, accumulate=1)['C'], prior)


def test_tn_workspace_query_with_no_rows():
    """geobi_gemm_tn_ws_bytes(I, J, 0) used to divide by zero on the host (rows per slice = 0); a product over no rows
    launches one block per tile, as one over a single row does."""
    from geobi_gnn_amd import _lib as L
    lib = L.lib()
    for I, J in ((40, 64), (97, 40), (9, 20)):
        assert lib.geobi_gemm_tn_ws_bytes(I, J, 0) == lib.geobi_gemm_tn_ws_bytes(I, J, 1) > 0


def test_header_declares_the_two_debug_entries_with_a_host_plan():
    import ctypes
    from geobi_gnn_amd import _lib as L
    protos = L.parse_header()
    for name, nargs in (('geobi_debug_gemm_nn', 21), ('geobi_debug_gemm_tn', 26)):
        _, argtypes, argnames = protos[name]
        assert len(argtypes) == nargs and argnames[-2:] == ['plan', 'stream']
        assert argtypes[-2] == ctypes.POINTER(ctypes.c_int64)


# ------------------------------------------------------------------------------ planted faults
def _tn_case():
    g = torch.Generator().manual_seed(5)
    A, B = _ints(g, 9, 4), _ints(g, 9, 4)
    kw = dict(C=_ints(g, 5 * 6), ldc=6, C2=_ints(g, 4), extra_row=1, accumulate=1, ones_row=True)
    return A, B, kw, G.tn_expected(G.PLAIN, A, B, **kw)


def _as_device(out):
    return {k: (None if v is None else v.float()) for k, v in out.items()}


def test_comparison_passes_on_the_expectation_itself():
    _, _, _, want = _tn_case()
    assert G.mismatches(_as_device(want), want) == []


def test_planted_fault_transposed_map():
    A, B, kw, want = _tn_case()
    got = _as_device(want)
    block = got['C'].view(5, 6)[:4, :4]
    assert not torch.equal(block, block.t())
    got['C'].view(5, 6)[:4, :4] = block.t().clone()
    assert [m.split(':')[0] for m in G.mismatches(got, want)] == ['C']


def test_planted_fault_ones_row_off_by_one():
    """The ones land one row early: the last data row of A reads as 1 and the true ones row as that data."""
    A, B, kw, want = _tn_case()
    shifted = torch.cat([A[:, :3], torch.ones(9, 1).double(), A[:, 3:]], 1)
    got = _as_device(G.tn_expected(G.PLAIN, shifted, B, **dict(kw, ones_row=False)))
    assert sorted(m.split(':')[0] for m in G.mismatches(got, want)) == ['C', 'C2']


def test_planted_fault_ignored_accumulate():
    A, B, kw, want = _tn_case()
    got = _as_device(G.tn_expected(G.PLAIN, A, B, **dict(kw, accumulate=0)))
    assert sorted(m.split(':')[0] for m in G.mismatches(got, want)) == ['C', 'C2']


@pytest.mark.parametrize('where', ['padding column', 'row that no rule addresses'])
def test_planted_fault_overwritten_sentinel(where):
    A, B, kw, want = _tn_case()
    got = _as_device(want)
    k = 1 * 6 + 5 if where == 'padding column' else 4 * 6 + 1       # ldc = 6 > J = 4; C holds 5 rows, the product 4 + 1
    assert float(want['C'][k]) == float(kw['C'][k])                   # the prior content
    got['C'][k] = 0.0 if float(want['C'][k]) != 0.0 else 1.0
    assert len(G.mismatches(got, want)) == 1


def test_planted_fault_one_dropped_term_and_nan():
    """One node row dropped from a 2 500-row reduction of integers moves an element by at least 1: exact operands need no
    tolerance to see it.  A NaN that leaks from the padding is a mismatch too."""
    g = torch.Generator().manual_seed(7)
    A, B = _ints(g, 2500, 4, lo=1), _ints(g, 2500, 3, lo=1)
    want = G.tn_expected(G.PLAIN, A, B, torch.zeros(12), 3)
    got = _as_device(G.tn_expected(G.PLAIN, A[:-1], B[:-1], torch.zeros(12), 3))
    assert len(G.mismatches(got, want)) == 1 and float(want['C'].abs().max()) < 2 ** 24
    leak = _as_device(want)
    leak['C'][5] = float('nan')
    assert len(G.mismatches(leak, want)) == 1
