"""Plain fp64 statements of the two dense products of csrc/gemm.hip as their launchers define them -- gemm_nn with its
epilogue (bias, leaky-relu slope, column-split output) and gemm_tn with its implicit last row / column and its four output
maps (TnOut of csrc/common.h) -- over WHOLE output buffers: what a call addresses is computed, everything else (padding
between the logical width and the leading dimension, rows a map never reaches) keeps its prior content.  No device, no
tile, no slice: tests/test_gpu_gemm.py compares the kernels with this, whichever path they took.

With small integer operands and a power-of-two slope every product and partial sum is an integer multiple of 2^-k far
below 2^24, so fp32 holds it exactly in any summation order and the fp64 values here are the bits the device must give.
The maps are pinned on torch.autograd's gradients of the layers they serve by tests/test_gemm_model_host.py."""
import numpy as np
import torch

H, HP = 9, 12                                       # FeaSt heads, and the row stride of per-node head vectors
PLAIN, LIN_UNPACK, DU_DC, RPRIME = 0, 1, 2, 3       # TnOut


def _f64(t):
    return torch.as_tensor(t).to(torch.float64)


# ------------------------------------------------------------------------------ gemm_nn
def nn_expected(A, B, transB, C, ldc, bias=None, slope=1.0, C1=None, split=0, ldc1=0):
    """C[m, n] = act(sum_k A[m, k] B[k, n] + bias[n]), act(v) = v if v > 0 else slope v.
    A [M, K]; B [K, N], or [N, K] when transB (nn.Linear.weight); C: prior content of the flat output buffer (M * ldc
    elements).  With C1 (prior content, M * ldc1 elements) columns n >= split go to C1[m * ldc1 + n - split] instead.
    -> (C, C1) fp64, flat, full length."""
    A, B = _f64(A), _f64(B)
    P = A @ (B.t() if transB else B)
    if bias is not None:
        P = P + _f64(bias)
    P = torch.where(P > 0, P, P * slope)
    M, N = P.shape
    C = _f64(C).clone()
    assert C.numel() == M * ldc
    if C1 is None:
        C.view(M, ldc)[:, :N] = P
        return C, None
    C1 = _f64(C1).clone()
    assert C1.numel() == M * ldc1 and 0 <= split <= N
    C.view(M, ldc)[:, :split] = P[:, :split]
    C1.view(M, ldc1)[:, :N - split] = P[:, split:]
    return C, C1


# ------------------------------------------------------------------------------ gemm_tn
def tn_product(A, B, ones_row=False, ones_col=False, sum_row=False):
    """The logical [I, J] product sum_m A[m, i] B[m, j] of the data operands A [M, Id], B [M, Jd]: with ones_row a last
    row as if A had a last column of ones, with ones_col a last column as if B had one, with sum_row a last row holding
    the column sums of B (of its ones column too).  ones_row and sum_row give the same numbers; they differ on the device."""
    A, B = _f64(A), _f64(B)
    assert not (ones_row and sum_row)
    one = torch.ones(A.shape[0], 1, dtype=torch.float64)
    if ones_col:
        B = torch.cat([B, one], 1)
    if ones_row or sum_row:
        A = torch.cat([A, one], 1)
    return A.t() @ B


def tn_routes(mode, I, J, ldc=0, Cin=0, Cout=0, col0=0, extra_row=0, extra_col=0, have=('C', 'C2', 'C3', 'C4')):
    """Where element (i, j) of the logical product goes: -> [(buffer name, offsets, i, j)], int64 arrays, every offset of
    a buffer named at most once.  Elements no rule names go nowhere.  `have`: the buffers the caller passes."""
    i, j = [a.reshape(-1) for a in np.meshgrid(np.arange(I, dtype=np.int64), np.arange(J, dtype=np.int64), indexing='ij')]
    routes = []

    def route(name, mask, off):
        if name in have and mask.any():
            routes.append((name, np.broadcast_to(off, i.shape)[mask], i[mask], j[mask]))

    if mode == PLAIN:
        # the implicit ones row / column is the last one and lands in C2; never both (C2 is one vector)
        assert not (extra_row and extra_col)
        er = (i == I - 1) if extra_row else np.zeros(i.shape, bool)
        ec = (j == J - 1) if extra_col else np.zeros(i.shape, bool)
        route('C2', er, j)
        route('C2', ec, i)
        route('C', ~er & ~ec, i * ldc + j)
    elif mode == LIN_UNPACK:
        # rows (head h, in-channel k) of z = the 9-head stacking, columns out-channels: lin.weight[h Cout + o, k]; the
        # last row (the ones row) is bias.grad.  Rows between 9 Cin and the last one (padding of z) go nowhere.
        h, k = i // Cin, i % Cin
        last = i == I - 1
        route('C2', last, j)
        route('C', ~last & (h < H), (h * Cout + j) * Cin + k)
    elif mode == DU_DC:
        # A = [dp (rows 0..8) | pad | dcs (rows 12..20) | pad], B = [x | 1]: du[h, j] = row h; dc[h] = row 12 + h of the
        # ones column
        route('C', (j < J - 1) & (i < H), i * ldc + j)
        route('C2', (j == J - 1) & (i >= HP) & (i < HP + H), i - HP)
    elif mode == RPRIME:
        # rows: input channels col0 + i (and the column-sums row when extra_row); columns r' = [r 9 Cout | dp 12 | dcs 12]
        HC = H * Cout
        sums = (i == I - 1) if extra_row else np.zeros(i.shape, bool)
        route('C', ~sums & (j < HC), j * Cin + col0 + i)
        route('C3', ~sums & (j >= HC) & (j < HC + H), (j - HC) * Cin + col0 + i)
        route('C4', sums & (j >= HC + HP) & (j < HC + HP + H), j - HC - HP)
    else:
        raise ValueError(mode)
    return routes


def tn_expected(mode, A, B, C, ldc=0, C2=None, C3=None, C4=None, Cin=0, Cout=0, col0=0, extra_row=0, extra_col=0,
                accumulate=0, ones_row=False, ones_col=False, sum_row=False):
    """gemm_tn's outputs: the product of tn_product routed by tn_routes into the flat buffers C, C2, C3, C4 (each given
    with its prior content, or None).  accumulate: added to the prior content; otherwise an addressed element is
    overwritten.  An element no rule addresses keeps its prior content either way.  TN_RPRIME with extra_row and C2:
    C2[c] = sum_h (last row)[h Cout + c], the bias gradient.  -> {'C': ..., 'C2': ...} fp64 (None where None came in)."""
    P = tn_product(A, B, ones_row, ones_col, sum_row)
    I, J = P.shape
    out = {k: (None if v is None else _f64(v).clone().reshape(-1)) for k, v in (('C', C), ('C2', C2), ('C3', C3), ('C4', C4))}
    have = [k for k, v in out.items() if v is not None]
    written = {k: np.zeros(out[k].numel(), bool) for k in have}
    for name, off, i, j in tn_routes(mode, I, J, ldc, Cin, Cout, col0, extra_row, extra_col, have):
        assert not written[name][off].any() and np.unique(off).size == off.size, 'two elements for one address'
        written[name][off] = True
        vals = P[torch.from_numpy(i), torch.from_numpy(j)]
        o = torch.from_numpy(np.ascontiguousarray(off))
        out[name][o] = out[name][o] + vals if accumulate else vals
    if mode == RPRIME and extra_row and out['C2'] is not None:
        t = P[I - 1, :H * Cout].view(H, Cout).sum(0)
        out['C2'][:Cout] = out['C2'][:Cout] + t if accumulate else t
    return out


# ------------------------------------------------------------------------------ the comparison
def mismatches(got, want):
    """Whole-buffer, bit-for-bit comparison of named fp32 buffers with their fp64 expectation (which must be exactly
    representable): -> one line per buffer that differs (empty: all equal)."""
    bad = []
    for name, w in want.items():
        if w is None:
            continue
        g = got[name].detach().cpu().reshape(-1)
        w = w.reshape(-1)
        w32 = w.to(torch.float32)
        assert torch.equal(w32.double(), w), 'the expectation of %s is not exact in fp32' % name
        if g.shape != w32.shape:
            bad.append('%s: %d elements, %d expected' % (name, g.numel(), w32.numel()))
        elif not torch.equal(g, w32):
            d = torch.nonzero(~((g == w32) | (torch.isnan(g) & torch.isnan(w32)))).reshape(-1)
            k = int(d[0])
            bad.append('%s: %d of %d elements differ, first at %d: %r, expected %r'
                       % (name, d.numel(), g.numel(), k, float(g[k]), float(w32[k])))
    return bad
