"""torch.autograd.Function wrappers over the C ABI (include/geobi_hip.h).

Each Function replaces one third-party op of the reference's hot path; the replaced call
site is cited in the docstring.  Tensors are allocated by PyTorch's caching allocator and
handed to the library as borrowed device pointers on torch's current HIP stream.
"""
import os

import torch
from torch.autograd import Function

from . import _lib as L

LEAK = 0.2
HP = 12   # GEOBI_HEAD_STRIDE
# GEOBI_FUSED=0: separate aggregation + GEMM kernels with the aggregated rows z [N, 9 Cin] written to HBM
# (the round-1 path, kept for A/B timing and as the second implementation the fused kernels are tested against)
FUSED = os.environ.get('GEOBI_FUSED', '1') == '1'


# ----------------------------------------------------------------------------- op tape
# DualGNN.forward issues ~70 differentiable ops per step.  Going through torch.autograd for each costs
# ~15 us of host time per node (Function.apply, graph bookkeeping, engine thread hops) -- more than
# the kernels of the coarse levels take.  Inside DualGNN the same Function classes are therefore
# driven through a minimal reverse-mode tape: the whole network is ONE autograd node
# (network.DualGNNFn) and the tape replays the per-op `backward`s in reverse order.  Outside of it
# (FeaStConv / PoolingLayer used on their own) the ops are ordinary autograd Functions.
class _TapeCtx(object):
    __slots__ = ('needs_input_grad', 'saved_tensors', '__dict__')

    def __init__(self, needs):
        self.needs_input_grad = needs
        self.saved_tensors = ()

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors


class Tape(object):
    """Reverse-mode tape over the Function classes of this module (forward called in no-grad mode)."""

    def __init__(self, record=True):
        self.record = record
        self.nodes = []
        self.live = set()              # ids of intermediate tensors that carry a gradient

    def needs(self, a):
        return torch.is_tensor(a) and a.is_floating_point() and (a.requires_grad or id(a) in self.live)

    def apply(self, fn, *args):
        needs = tuple(self.needs(a) for a in args)
        ctx = _TapeCtx(needs)
        out = fn.forward(ctx, *args)
        if self.record and any(needs):
            self.nodes.append((fn, ctx, args, out))
            self.live.add(id(out))
        return out

    def backward(self, seeds, clear=True):
        """seeds: {id(tensor): grad}.  Returns {id(leaf tensor): grad} for leaves with requires_grad.
        clear=False keeps the recorded nodes (and the tensors they saved) alive for the caller to drop."""
        grads = dict(seeds)
        leaf = {}
        for fn, ctx, args, out in reversed(self.nodes):
            g = grads.pop(id(out), None)
            if g is None:
                continue
            gins = fn.backward(ctx, g)
            for a, gi in zip(args, gins):
                if gi is None or not torch.is_tensor(a):
                    continue
                k = id(a)
                if k in self.live:
                    grads[k] = gi if k not in grads else grads[k] + gi
                elif a.requires_grad:
                    leaf[k] = gi if k not in leaf else leaf[k] + gi
        if clear:
            self.nodes = []
        return leaf


_ACTIVE_TAPE = [None]

# Deferred side-stream join (geobi_side_defer): while a list is installed here, backward ops park every
# buffer the side stream may still be reading (workspaces, incoming gradients) in it; whoever installed
# it joins the side stream and only then drops the list.
_SIDE_KEEP = [None]


class deferred_side_join(object):
    """with deferred_side_join(): ... -- weight-gradient GEMMs of all backward calls inside queue on the
    library's side stream without per-call joins; one join on exit."""

    def __init__(self, enable=True):
        self.enable = enable

    def __enter__(self):
        self.prev = _SIDE_KEEP[0]
        if self.enable and self.prev is None:
            _SIDE_KEEP[0] = []
            L.call('geobi_side_defer', 1)
        return self

    def __exit__(self, *exc):
        if self.enable and self.prev is None:
            try:
                L.call('geobi_side_defer', 0)
                L.call('geobi_side_join', L.stream())
            finally:
                _SIDE_KEEP[0] = None
        return False


def apply_op(fn, *args):
    """Run a Function through the active tape (inside DualGNN) or through torch.autograd."""
    tape = _ACTIVE_TAPE[0]
    return tape.apply(fn, *args) if tape is not None else fn.apply(*args)


class use_tape(object):
    def __init__(self, tape):
        self.tape = tape

    def __enter__(self):
        self.prev = _ACTIVE_TAPE[0]
        _ACTIVE_TAPE[0] = self.tape
        return self.tape

    def __exit__(self, *exc):
        _ACTIVE_TAPE[0] = self.prev
        return False


def _direct_grad(p):
    """Gradient buffer the kernels may write into directly.

    parallel.GradBucket(direct=True) marks parameters whose ``.grad`` is a persistent view of the
    flat bucket.  The backward kernels then ADD the gradient straight into that view (`accumulate`
    argument of geobi_feast_bwd / geobi_head_bwd) and autograd receives ``None`` -- this removes one
    accumulate kernel per parameter (76 per step) and keeps autograd's semantics: several backward
    passes between two ``bucket.zero()`` calls sum up (the reference's gradient accumulation,
    train_dual.py:211-218), and so do several uses of one parameter in a forward."""
    if not getattr(p, '_geobi_direct_grad', False):
        return None
    if p.grad is None or not p.grad.is_contiguous() or getattr(p, '_geobi_grad_ptr', None) != p.grad.data_ptr():
        raise L.GeobiError('a direct-gradient parameter lost its bucket view (optimizer.zero_grad(set_to_none=True) or '
                           'an assignment to .grad): zero the gradients with GradBucket.zero() instead')
    bucket = getattr(p, '_geobi_bucket', None)
    owner = None if bucket is None else bucket.owner
    if owner is not None and (owner.grad is None or owner.grad.data_ptr() != bucket.flat.data_ptr()):
        # FlatParameters: the optimizer steps ONE flat parameter.  zero_grad(set_to_none=True) on it leaves the
        # per-parameter views intact, the kernels would keep adding into the bucket and optimizer.step() would skip
        # the parameter without a word
        raise L.GeobiError('the flat parameter lost its gradient bucket (optimizer.zero_grad(set_to_none=True) or an '
                           'assignment to .grad): zero the gradients with GradBucket.zero() instead')
    return p.grad


def _f32c(t):
    if t.dtype != torch.float32:
        raise L.GeobiError('expected float32, got %s' % t.dtype)
    return t.contiguous()


# --------------------------------------------------------------------------- FeaSt conv
class FeastConvFn(Function):
    """torch_geometric.nn.FeaStConv forward/backward (network.py:271-299), optionally fused with
    the following leaky_relu (``slope``) and the skip concatenation (input given as xa | xb)."""

    @staticmethod
    def forward(ctx, xa, xb, lin_w, u_w, c, bias, graph, slope):
        L.require_device(xa, 'x')
        g = graph.ensure_in()
        ctx.param_refs = (lin_w, u_w, c, bias)
        xa = _f32c(xa)
        xb = None if xb is None else _f32c(xb)
        lin_w, u_w, c, bias = _f32c(lin_w), _f32c(u_w), _f32c(c), _f32c(bias)
        N, Ca = xa.shape
        Cb = 0 if xb is None else xb.shape[1]
        Cin, Cout = Ca + Cb, bias.shape[0]
        if N != g.N:
            raise L.GeobiError('FeaStConv: x has %d rows but the graph has %d nodes' % (N, g.N))
        if lin_w.shape != (9 * Cout, Cin) or u_w.shape != (9, Cin) or c.shape != (9,):
            raise L.GeobiError('FeaStConv: parameter shapes do not match heads=9, in=%d, out=%d' % (Cin, Cout))
        dev = xa.device
        lib = L.lib()
        ldz = L.size_query('geobi_feast_ldz', Cin)
        out = torch.empty((N, Cout), dtype=torch.float32, device=dev)
        p = torch.empty((N, HP), dtype=torch.float32, device=dev)
        z = None if FUSED else torch.empty((N, ldz), dtype=torch.float32, device=dev)
        # packed weights (Wf | W'), reused by the backward; not kept when nothing needs a gradient
        wf = None
        if any(ctx.needs_input_grad):
            wf = torch.empty(L.size_query('geobi_feast_wpack_floats', Cin, Cout), dtype=torch.float32, device=dev)
        ws = L.workspace(L.size_query('geobi_feast_fwd_ws_bytes', N, Cin, Cout), dev)
        L.call('geobi_feast_fwd', L.ptr(xa), L.ptr(xb), Ca, Cb, N, g.E, L.ptr(g.rowptr_in), L.ptr(g.col_in),
               L.ptr(lin_w), L.ptr(u_w), L.ptr(c), L.ptr(bias), Cout, float(slope), L.ptr(out), L.ptr(p), L.ptr(z),
               L.ptr(wf), L.ptr(ws), ws.numel(), L.stream())
        ctx.graph, ctx.slope, ctx.has_b, ctx.has_wf, ctx.has_z = g, float(slope), xb is not None, wf is not None, z is not None
        ctx.save_for_backward(xa, xb if xb is not None else xa, lin_w, u_w, c, out, p, z if z is not None else p,
                              wf if wf is not None else p)
        return out

    @staticmethod
    def backward(ctx, gout):
        xa, xb, lin_w, u_w, c, out, p, z, wf = ctx.saved_tensors
        if not ctx.has_wf:
            wf = None
        if not ctx.has_z:
            z = None
        g = ctx.graph
        if not ctx.has_b:
            xb = None
        N, Ca = xa.shape
        Cb = 0 if xb is None else xb.shape[1]
        Cin, Cout = Ca + Cb, out.shape[1]
        dev = xa.device
        gout = _f32c(gout)
        need_dx = ctx.needs_input_grad[0] or (xb is not None and ctx.needs_input_grad[1])
        dxa = torch.empty_like(xa) if need_dx else None
        dxb = torch.empty_like(xb) if (need_dx and xb is not None) else None
        direct = [_direct_grad(p_) for p_ in ctx.param_refs]
        if all(d is not None for d in direct):
            dlin, du, dc, dbias = direct
            ret = (None, None, None, None)
        else:
            dlin, du, dc = torch.empty_like(lin_w), torch.empty_like(u_w), torch.empty_like(c)
            dbias = torch.empty(Cout, dtype=torch.float32, device=dev)
            ret = (dlin, du, dc, dbias)
        ws = L.workspace(L.size_query('geobi_feast_bwd_ws_bytes', N, g.E, Cin, Cout), dev)
        L.call('geobi_feast_bwd', L.ptr(xa), L.ptr(xb), Ca, Cb, N, g.E, L.ptr(g.rowptr_in), L.ptr(g.col_in),
               L.ptr(g.rowptr_out), L.ptr(g.col_out), L.ptr(g.pos_in), L.ptr(lin_w), L.ptr(u_w), L.ptr(c), Cout,
               ctx.slope, L.ptr(out), L.ptr(gout), L.ptr(p), L.ptr(z), L.ptr(wf), L.ptr(dxa), L.ptr(dxb), L.ptr(dlin),
               L.ptr(du), L.ptr(dc), L.ptr(dbias), 1 if ret[0] is None else 0, L.ptr(ws), ws.numel(), L.stream())
        if _SIDE_KEEP[0] is not None:
            _SIDE_KEEP[0].append((ws, gout, dlin, du, dc, dbias))
        return (dxa, dxb) + ret + (None, None)


def feast_conv(x, graph, lin_w, u_w, c, bias, slope=1.0, x2=None):
    return apply_op(FeastConvFn, x, x2, lin_w, u_w, c, bias, graph, slope)


# ------------------------------------------------------------------ inverse lists / pooling
class SegmentIndex(object):
    """Inverse lists ``segment -> members`` of an int32 segment-id vector (sorted, deterministic)."""

    def __init__(self, seg32, nseg, build=True):
        L.require_device(seg32, 'segment ids')
        self.seg = seg32.contiguous()
        self.n = int(seg32.shape[0])
        self.nseg = int(nseg)
        dev = seg32.device
        self.segptr = torch.empty(self.nseg + 1, dtype=torch.int32, device=dev)
        self.members = torch.empty(max(self.n, 1), dtype=torch.int32, device=dev)[:self.n]
        if build:       # general path: radix sort of (segment, member) keys
            ws = L.workspace(L.size_query('geobi_segment_csr_ws_bytes', self.n), dev)
            L.call('geobi_segment_csr', L.ptr(self.seg), self.n, self.nseg, L.ptr(self.segptr),
                   L.ptr(self.members), L.ptr(ws), ws.numel(), L.stream())

    @staticmethod
    def view(seg32, nseg, segptr, members):
        """Lists that already exist (slices of arrays built with an upper bound on the sizes)."""
        self = SegmentIndex.__new__(SegmentIndex)
        self.seg, self.n, self.nseg = seg32, int(seg32.shape[0]), int(nseg)
        self.segptr, self.members = segptr, members
        return self

    @staticmethod
    def from_matching(cnew32, raw32, nseg):
        """Sort-free lists for a matching (clusters of <= 2 nodes, raw id = smaller member)."""
        self = SegmentIndex(cnew32, nseg, build=False)
        raw32 = raw32.contiguous()
        ws = L.workspace(L.size_query('geobi_segment_pairs_ws_bytes', self.nseg), cnew32.device)
        L.call('geobi_segment_csr_pairs', L.ptr(self.seg), L.ptr(raw32), self.n, self.nseg, L.ptr(self.segptr),
               L.ptr(self.members), L.ptr(ws), ws.numel(), L.stream())
        return self

    def narrow(self, nseg):
        """Lists built with an upper bound on the segment count: keep the first `nseg` segments."""
        self.nseg = int(nseg)
        self.segptr = self.segptr[:self.nseg + 1]
        return self

    @staticmethod
    def compose(first, second, composed_seg32):
        """Lists of fine -> coarse for `composed_seg32 = second.seg[first.seg]`."""
        self = SegmentIndex(composed_seg32, second.nseg, build=False)
        ws = L.workspace(L.size_query('geobi_segment_pairs_ws_bytes', self.nseg), composed_seg32.device)
        L.call('geobi_segment_csr_compose', L.ptr(first.segptr), L.ptr(first.members), L.ptr(second.segptr),
               L.ptr(second.members), self.nseg, self.n, L.ptr(self.segptr), L.ptr(self.members), L.ptr(ws),
               ws.numel(), L.stream())
        return self


class SegmentMaxFn(Function):
    """torch_scatter.scatter(x, cluster, dim=0, reduce='max') (net_util.py:134)."""

    @staticmethod
    def forward(ctx, x, sidx):
        x = _f32c(x)
        C = x.shape[1]
        out = torch.empty((sidx.nseg, C), dtype=torch.float32, device=x.device)
        arg = torch.empty((sidx.nseg, C), dtype=torch.int32, device=x.device)
        L.call('geobi_segment_max_fwd', L.ptr(x), C, L.ptr(sidx.segptr), L.ptr(sidx.members), sidx.nseg, L.ptr(out),
               L.ptr(arg), L.stream())
        ctx.save_for_backward(arg)
        ctx.n_fine, ctx.sidx = x.shape[0], sidx
        return out

    @staticmethod
    def backward(ctx, gout):
        (arg,) = ctx.saved_tensors
        gout = _f32c(gout)
        nseg, C = gout.shape
        gx = torch.empty((ctx.n_fine, C), dtype=torch.float32, device=gout.device)
        L.call('geobi_segment_max_bwd', L.ptr(gout), L.ptr(arg), L.ptr(ctx.sidx.seg), C, nseg, ctx.n_fine, L.ptr(gx),
               L.stream())
        return gx, None


class SegmentMeanFn(Function):
    """torch_scatter.scatter(..., reduce='mean') (net_util.py:132; pool_pos :136)."""

    @staticmethod
    def forward(ctx, x, sidx):
        x = _f32c(x)
        C = x.shape[1]
        out = torch.empty((sidx.nseg, C), dtype=torch.float32, device=x.device)
        L.call('geobi_segment_sum', L.ptr(x), C, L.ptr(sidx.segptr), L.ptr(sidx.members), sidx.nseg, 1, L.ptr(out),
               L.stream())
        ctx.sidx = sidx
        return out

    @staticmethod
    def backward(ctx, gout):
        sidx = ctx.sidx
        gout = _f32c(gout)
        C = gout.shape[1]
        gx = torch.empty((sidx.n, C), dtype=torch.float32, device=gout.device)
        L.call('geobi_segment_mean_bwd', L.ptr(gout), L.ptr(sidx.seg), L.ptr(sidx.segptr), C, sidx.n, L.ptr(gx),
               L.stream())
        return gx, None


class UnpoolFn(Function):
    """PoolingLayer.unpooling: ``x[unpooling_indices]`` (net_util.py:242-245); the backward is a
    sorted-segment sum through the inverse lists instead of an atomic index_add."""

    @staticmethod
    def forward(ctx, x, sidx):
        x = _f32c(x)
        C = x.shape[1]
        out = torch.empty((sidx.n, C), dtype=torch.float32, device=x.device)
        L.call('geobi_gather_rows', L.ptr(x), L.ptr(sidx.seg), C, sidx.n, L.ptr(out), L.stream())
        ctx.sidx = sidx
        return out

    @staticmethod
    def backward(ctx, gout):
        sidx = ctx.sidx
        gout = _f32c(gout)
        C = gout.shape[1]
        gx = torch.empty((sidx.nseg, C), dtype=torch.float32, device=gout.device)
        L.call('geobi_segment_sum', L.ptr(gout), C, L.ptr(sidx.segptr), L.ptr(sidx.members), sidx.nseg, 0,
               L.ptr(gx), L.stream())
        return gx, None


# ----------------------------------------------------------------------- geometry / heads
class FaceGeomFn(Function):
    """network.py:335-337 + data_util.computer_face_normal: x_f = cat(x_f, centroid, unit normal)."""

    @staticmethod
    def forward(ctx, verts, xf, fv32, corner_index):
        verts, xf = _f32c(verts), _f32c(xf)
        F = fv32.shape[0]
        out = torch.empty((F, 12), dtype=torch.float32, device=verts.device)
        L.call('geobi_face_geom_fwd', L.ptr(verts), L.ptr(fv32), L.ptr(xf), xf.shape[1], F, L.ptr(out), L.stream())
        ctx.save_for_backward(verts, fv32)
        ctx.corner_index = corner_index
        return out

    @staticmethod
    def backward(ctx, gout):
        verts, fv32 = ctx.saved_tensors
        cidx = ctx.corner_index.get() if hasattr(ctx.corner_index, 'get') else ctx.corner_index
        gout = _f32c(gout)
        F = fv32.shape[0]
        cg = torch.empty((3 * F, 3), dtype=torch.float32, device=gout.device)
        L.call('geobi_face_geom_bwd', L.ptr(verts), L.ptr(fv32), L.ptr(gout), F, L.ptr(cg), L.stream())
        gv = torch.empty((cidx.nseg, 3), dtype=torch.float32, device=gout.device)
        L.call('geobi_segment_sum', L.ptr(cg), 3, L.ptr(cidx.segptr), L.ptr(cidx.members), cidx.nseg, 0, L.ptr(gv),
               L.stream())
        return gv, None, None, None


class HeadFn(Function):
    """fc2(leaky_relu(fc1 x)) + finish (network.py:324-332 vertex head, :340-343 face head).

    Fused kernels (Cin = 32, K = 1024): the [N, 1024] hidden activation lives in MFMA accumulators
    only -- forward and backward (recomputed) -- and is never written to HBM.  Other widths fall
    back to the generic GEMM path with a materialised hidden tensor."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, mode, dd, resid):
        ctx.param_refs = (w1, b1, w2, b2)
        x, w1, b1, w2, b2 = _f32c(x), _f32c(w1), _f32c(b1), _f32c(w2), _f32c(b2)
        N, Cin = x.shape
        K, nout = w1.shape[0], w2.shape[0]
        dev = x.device
        fused = (Cin == 32 and K == 1024)
        h = None if fused else torch.empty((N, K), dtype=torch.float32, device=dev)
        raw = torch.empty((N, nout), dtype=torch.float32, device=dev)
        out = torch.empty((N, 3), dtype=torch.float32, device=dev)
        dd = None if dd is None else _f32c(dd)
        ld_resid = 0
        if resid is not None:
            if resid.stride(1) != 1:
                raise L.GeobiError('head: residual rows must be contiguous')
            ld_resid = resid.stride(0)
        L.call('geobi_head_fwd', L.ptr(x), Cin, N, L.ptr(w1), L.ptr(b1), K, L.ptr(w2), L.ptr(b2), nout, LEAK, mode,
               L.ptr(dd), None if resid is None else resid.data_ptr(), ld_resid, L.ptr(h), L.ptr(raw), L.ptr(out),
               L.stream())
        ctx.mode = mode
        ctx.has_dd, ctx.has_h = dd is not None, h is not None
        ctx.save_for_backward(x, w1, b1, w2, raw, dd if dd is not None else raw, h if h is not None else raw)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, w1, b1, w2, raw, dd, h = ctx.saved_tensors
        if not ctx.has_dd:
            dd = None
        if not ctx.has_h:
            h = None
        gout = _f32c(gout)
        N, Cin = x.shape
        K, nout = w1.shape[0], w2.shape[0]
        dev = x.device
        dx = torch.empty_like(x) if (ctx.needs_input_grad[0] or h is None) else None
        direct = [_direct_grad(p_) for p_ in ctx.param_refs]
        if all(d is not None for d in direct):
            dw1, db1, dw2, db2 = direct
            ret = (None, None, None, None)
        else:
            dw1, db1 = torch.empty_like(w1), torch.empty(K, dtype=torch.float32, device=dev)
            dw2, db2 = torch.empty_like(w2), torch.empty(nout, dtype=torch.float32, device=dev)
            ret = (dw1, db1, dw2, db2)
        ws = L.workspace(L.size_query('geobi_head_bwd_ws_bytes', N, Cin, K), dev)
        L.call('geobi_head_bwd', L.ptr(x), Cin, N, L.ptr(w1), L.ptr(b1), K, L.ptr(w2), nout, LEAK, ctx.mode,
               L.ptr(dd), L.ptr(h), L.ptr(raw), L.ptr(gout), L.ptr(dx), L.ptr(dw1), L.ptr(db1), L.ptr(dw2),
               L.ptr(db2), 1 if ret[0] is None else 0, L.ptr(ws), ws.numel(), L.stream())
        return (dx,) + ret + (None, None, None)


# ------------------------------------------------------------------------ losses / metrics
class RowLossFn(Function):
    """scale * sum_i w_i * term(a_i, b_i) over [n, 3] rows (network.py:364-413; kinds in geobi_hip.h)."""

    @staticmethod
    def forward(ctx, a, b, w, kind, scale):
        L.require_device(a, 'prediction')
        a, b = _f32c(a), _f32c(b.detach())
        if a.dim() != 2 or a.shape[1] != 3 or b.shape != a.shape:
            raise L.GeobiError('row loss expects two [n, 3] tensors, got %s and %s' % (tuple(a.shape), tuple(b.shape)))
        w = None if w is None else _f32c(w)
        n = a.shape[0]
        out = torch.empty(1, dtype=torch.float32, device=a.device)
        ws = L.workspace(L.size_query('geobi_row_loss_ws_bytes', n), a.device)
        L.call('geobi_row_loss_fwd', L.ptr(a), L.ptr(b), L.ptr(w), n, int(kind), float(scale), L.ptr(out), L.ptr(ws),
               ws.numel(), L.stream())
        ctx.kind, ctx.scale, ctx.has_w = int(kind), float(scale), w is not None
        ctx.save_for_backward(a, b, w if w is not None else a)
        return out.view(())

    @staticmethod
    def backward(ctx, gout):
        a, b, w = ctx.saved_tensors
        if ctx.kind > 1:
            raise L.GeobiError('error_v / error_n are metrics: no gradient is defined (the reference never needs one)')
        ga = torch.empty_like(a)
        g = gout.reshape(1).float().contiguous()
        L.call('geobi_row_loss_bwd', L.ptr(a), L.ptr(b), L.ptr(w) if ctx.has_w else None, L.ptr(g), a.shape[0],
               ctx.kind, ctx.scale, L.ptr(ga), L.stream())
        return ga, None, None, None, None


def row_loss(a, b, kind, weights=None, scale=None):
    n = a.shape[0]
    return RowLossFn.apply(a, b, weights, kind, (1.0 / n) if scale is None else scale)


# ------------------------------------------------------- correspondence-free losses (CD / sided)
def _part_ptr(ptr, n, what):
    """Host part pointer of a union batch -> list of ints; None is one part [0, n].  The ends must be 0 and n: the
    kernels take the pointer's word for where the rows are."""
    if ptr is None:
        lst = [0, int(n)]
    else:
        lst = [int(v) for v in (ptr.tolist() if torch.is_tensor(ptr) else ptr)]
    if len(lst) < 2 or lst[0] != 0 or lst[-1] != int(n):
        raise L.GeobiError('%s %r does not cover the %d rows it cuts (it must run from 0 to %d)' % (what, lst, n, n))
    return lst


def _c_ptr(lst):
    import ctypes
    arr = (ctypes.c_int64 * len(lst))(*lst)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def _points3(t, what):
    L.require_device(t, what)
    t = _f32c(t.detach())
    if t.dim() != 2 or t.shape[1] != 3:
        raise L.GeobiError('%s must be [n, 3], got %s' % (what, tuple(t.shape)))
    return t


def nearest_parts(q, t, qptr=None, tptr=None):
    """For every row of q [Q, 3] the nearest row of t [T, 3] AMONG THE ROWS OF ITS OWN PART (geobi_nearest_parts; the
    search under kaolin's chamfer_distance / sided_distance, code/network.py:370,386).  qptr / tptr: host part pointers
    [P + 1] (list or CPU tensor; None: one part); no part may be empty.
    -> (d2 float32 [Q]: SQUARED distance, idx int32 [Q]: row of t, the lowest among equally near ones)."""
    q, t = _points3(q, 'query points'), _points3(t, 'target points')
    Q, T = q.shape[0], t.shape[0]
    qp, tp = _part_ptr(qptr, Q, 'qptr'), _part_ptr(tptr, T, 'tptr')
    if len(qp) != len(tp):
        raise L.GeobiError('nearest_parts: %d query parts but %d target parts' % (len(qp) - 1, len(tp) - 1))
    P = len(qp) - 1
    (qa, qc), (ta, tc) = _c_ptr(qp), _c_ptr(tp)
    d2 = torch.empty(Q, dtype=torch.float32, device=q.device)
    idx = torch.empty(Q, dtype=torch.int32, device=q.device)
    ws = L.workspace(L.lib().geobi_nearest_parts_ws_bytes(qc, tc, P), q.device)
    L.call('geobi_nearest_parts', L.ptr(q), L.ptr(t), qc, tc, P, L.ptr(d2), L.ptr(idx), L.ptr(ws), ws.numel(), L.stream())
    return d2, idx


def nearest_parts_slices(qptr, tptr):
    """The largest number of target slices geobi_nearest_parts cuts a part into for these sizes (host computation)."""
    (qa, qc), (ta, tc) = _c_ptr([int(v) for v in qptr]), _c_ptr([int(v) for v in tptr])
    return int(L.lib().geobi_nearest_parts_slices(qc, tc, len(qptr) - 1))


class ChamferFn(Function):
    """kaolin's chamfer_distance(vp, v) as loss_v(..., dis='CD') calls it (code/network.py:369-370), per mesh of a union
    batch and averaged over the meshes: mean_i min_j |p_i - t_j|^2 + mean_j min_i |p_i - t_j|^2.  The two arg-min maps are
    constants of the gradient, which goes to the prediction only."""

    @staticmethod
    def forward(ctx, p, t, qptr, tptr):
        p, t = _points3(p, 'prediction'), _points3(t, 'target')
        qp, tp = _part_ptr(qptr, p.shape[0], 'qptr'), _part_ptr(tptr, t.shape[0], 'tptr')
        d2a, ia = nearest_parts(p, t, qp, tp)
        d2b, ib = nearest_parts(t, p, tp, qp)
        P = len(qp) - 1
        (qa, qc), (ta, tc) = _c_ptr(qp), _c_ptr(tp)
        out = torch.empty(1, dtype=torch.float32, device=p.device)
        ws = L.workspace(L.size_query('geobi_chamfer_ws_bytes', P), p.device)
        L.call('geobi_chamfer_fwd', L.ptr(d2a), L.ptr(d2b), qc, tc, P, L.ptr(out), L.ptr(ws), ws.numel(), L.stream())
        ctx.qp, ctx.tp = qp, tp
        ctx.save_for_backward(p, t, ia, ib)
        return out.view(())

    @staticmethod
    def backward(ctx, gout):
        p, t, ia, ib = ctx.saved_tensors
        sidx = SegmentIndex(ib, p.shape[0])          # prediction row -> the targets that chose it, ascending
        (qa, qc), (ta, tc) = _c_ptr(ctx.qp), _c_ptr(ctx.tp)
        gp = torch.empty_like(p)
        g = gout.reshape(1).float().contiguous()
        L.call('geobi_chamfer_bwd', L.ptr(p), L.ptr(t), L.ptr(ia), L.ptr(sidx.segptr), L.ptr(sidx.members), qc, tc,
               len(ctx.qp) - 1, L.ptr(g), L.ptr(gp), L.stream())
        return gp, None, None, None


def chamfer_loss(p, t, qptr=None, tptr=None):
    return ChamferFn.apply(p, t, qptr, tptr)


def sided_loss(np_, n, fc_p, fc, fptr=None, weights=None):
    """loss_n(np, n, 'sided', fc_p, fc) (code/network.py:385-388): every predicted normal against the ground-truth normal
    of the face whose centroid is nearest to the predicted face's, the search confined to the meshes of `fptr`;
    `weights`: per-row 1 / (B n_mesh) of a union batch (None: plain mean).  The gradient goes to np only."""
    L.require_device(np_, 'predicted normals')
    n = _f32c(n.detach())
    if n.dim() != 2 or n.shape[1] != 3 or n.shape[0] != fc.shape[0] or np_.shape[0] != fc_p.shape[0]:
        raise L.GeobiError('sided loss: normals %s / %s do not match centroids %s / %s'
                           % (tuple(np_.shape), tuple(n.shape), tuple(fc_p.shape), tuple(fc.shape)))
    _, idx = nearest_parts(fc_p, fc, fptr, fptr)
    ng = torch.empty((idx.shape[0], 3), dtype=torch.float32, device=n.device)
    L.call('geobi_gather_rows', L.ptr(n), L.ptr(idx), 3, idx.shape[0], L.ptr(ng), L.stream())
    return row_loss(np_, ng, 0, weights, 1.0 if weights is not None else None)


# ------------------------------------------------------- sampled surface Chamfer loss (SCD)
class BaryPointsFn(Function):
    """x_i = sum_k bary[i, k] * p[fv[face[i], k]] (geobi_bary_points: the sampler's own formula, so on the sampler's
    (face, bary) its points come back bit for bit; a row with face = -1 is zeros).  face and bary are constants of the
    gradient, which goes to p only: gp_v = the fp64 sum over the inverse lists vertex -> (sample, corner), built in the
    backward (geobi_bary_keys, SegmentIndex, geobi_bary_points_bwd); no atomics, the same bits for every run."""

    @staticmethod
    def forward(ctx, p, fv, face, bary):
        L.require_device(p, 'points')
        for what, t in (('faces', fv), ('sample faces', face), ('barycentrics', bary)):
            L.require_device(t, what)
        p, bary = _f32c(p.detach()), _f32c(bary.detach())
        fv, face = fv.to(torch.int32).contiguous(), face.to(torch.int32).contiguous()
        n = face.shape[0]
        if (p.dim() != 2 or p.shape[1] != 3 or fv.dim() != 2 or fv.shape[1] != 3 or face.dim() != 1
                or tuple(bary.shape) != (n, 3)):
            raise L.GeobiError('bary_points expects p [V,3], fv [F,3], face [n], bary [n,3], got %s, %s, %s, %s'
                               % (tuple(p.shape), tuple(fv.shape), tuple(face.shape), tuple(bary.shape)))
        if p.shape[0] == 0 or fv.shape[0] == 0:
            raise L.GeobiError('bary_points: an empty mesh (V = %d, F = %d)' % (p.shape[0], fv.shape[0]))
        out = torch.empty((n, 3), dtype=torch.float32, device=p.device)
        L.call('geobi_bary_points', L.ptr(p), L.ptr(fv), L.ptr(face), L.ptr(bary), p.shape[0], fv.shape[0], n, L.ptr(out),
               L.stream())
        ctx.V = p.shape[0]
        ctx.save_for_backward(fv, face, bary)
        return out

    @staticmethod
    def backward(ctx, gx):
        fv, face, bary = ctx.saved_tensors
        gx = _f32c(gx)
        n, V = face.shape[0], ctx.V
        keys = torch.empty(3 * n, dtype=torch.int32, device=gx.device)
        L.call('geobi_bary_keys', L.ptr(fv), L.ptr(face), V, fv.shape[0], n, L.ptr(keys), L.stream())
        sidx = SegmentIndex(keys, V)                 # vertex -> the entries 3 i + k that it carries, ascending
        gp = torch.empty((V, 3), dtype=torch.float32, device=gx.device)
        L.call('geobi_bary_points_bwd', L.ptr(bary), L.ptr(gx), L.ptr(sidx.segptr), L.ptr(sidx.members), V, n, L.ptr(gp),
               L.stream())
        return gp, None, None, None


def bary_points(p, fv, face, bary):
    return BaryPointsFn.apply(p, fv, face, bary)


def sampled_chamfer_loss(p, t, fv, fptr=None, vptr=None, n=10000, seed=0, stream_ids=None, draw=0, check=True):
    """The Chamfer distance between n points drawn by area on each predicted SURFACE and n on each ground-truth surface
    of a union batch (p, t [V,3]; fv [F,3] with global vertex ids; host pointers fptr [P+1] over the faces and vptr [P+1]
    over the vertices, None: one mesh), averaged over the meshes.  The ground truth is drawn with draw 2 * draw, the
    prediction with 2 * draw + 1 (the parities of mesheval.eval_sampled) and stream_ids[k] for mesh k (None: 0, 1, ...).
    The predicted samples are bary_points(p, ...) of (face, bary) drawn on p.detach(): constants of the gradient, as the two
    arg-min maps of chamfer_loss are; the gradient goes to p only.  check=False: fv is known to be in range (a dataset's
    own table), no host read for it."""
    from . import meshsample
    pd, t = _points3(p, 'prediction'), _points3(t, 'target')
    if t.shape != pd.shape:
        raise L.GeobiError('sampled_chamfer_loss: prediction %s and target %s share one face table'
                           % (tuple(pd.shape), tuple(t.shape)))
    fp = _part_ptr(fptr, fv.shape[0], 'fptr')
    _part_ptr(vptr, pd.shape[0], 'vptr')             # the face table holds global ids: vptr only has to cover the rows
    P, n = len(fp) - 1, int(n)
    if n < 1:
        raise ValueError('sampled_chamfer_loss: n = %d samples per mesh (at least one)' % n)
    sid = list(range(P)) if stream_ids is None else stream_ids
    sp = meshsample.sample_surface_parts(pd, fv, fp, n, seed=seed, stream_ids=sid, draw=2 * int(draw) + 1, check=check)
    st = meshsample.sample_surface_parts(t, fv, fp, n, seed=seed, stream_ids=sid, draw=2 * int(draw), check=False)
    sptr = [k * n for k in range(P + 1)]
    return chamfer_loss(bary_points(p, fv, sp.face, sp.bary), st.points, sptr, sptr)


# ------------------------------------------------------- mesh regularisers (Laplacian / edge length)
TERM_LAP, TERM_EDGE = 1, 2   # bits of `terms` (include/geobi_hip.h)


class MeshRegFn(Function):
    """(L_lap, L_edge) of include/geobi_hip.h, "mesh regularisers": the reference's laplacian_loss (code/network.py:347-361)
    and the edge-length term over the loop-free symmetric vertex CSR, both from one forward and one backward launch.  The
    gradient goes to the prediction only; a term that `terms` leaves out is 0 and takes no gradient."""

    @staticmethod
    def forward(ctx, vp, v, graph, normal, w_lap, w_edge, terms):
        L.require_device(vp, 'prediction')
        vp, v = _f32c(vp), _f32c(v.detach())
        if vp.dim() != 2 or vp.shape[1] != 3 or v.shape != vp.shape:
            raise L.GeobiError('mesh_reg expects two [V, 3] tensors, got %s and %s' % (tuple(vp.shape), tuple(v.shape)))
        V = vp.shape[0]
        terms = int(terms)
        if terms not in (TERM_LAP, TERM_EDGE, TERM_LAP | TERM_EDGE):
            raise L.GeobiError('mesh_reg: terms %r (TERM_LAP = 1, TERM_EDGE = 2 or both)' % (terms,))
        if graph.symmetric is not True:
            raise L.GeobiError('mesh_reg needs a graph known to be symmetric (its backward gathers over the rows that the '
                               'forward walked); this one has symmetric = %r' % (graph.symmetric,))
        if graph.N != V:
            raise L.GeobiError('mesh_reg: a graph of %d nodes for %d vertices' % (graph.N, V))
        rows = [('normal', normal), ('w_lap', w_lap), ('w_edge', w_edge)]
        for k, (what, t) in enumerate(rows):
            if t is None:
                continue
            L.require_device(t, what)
            t = _f32c(t.detach())
            if tuple(t.shape) != ((V, 3) if what == 'normal' else (V,)):
                raise L.GeobiError('mesh_reg: %s is %s for %d vertices' % (what, tuple(t.shape), V))
            rows[k] = (what, t)
        normal, w_lap, w_edge = (t for _, t in rows)
        dev = vp.device
        out = torch.empty(2, dtype=torch.float32, device=dev)
        u = torch.empty((V, 3), dtype=torch.float32, device=dev) if terms & TERM_LAP else None
        ws = L.workspace(L.size_query('geobi_mesh_reg_ws_bytes', V), dev)
        L.call('geobi_mesh_reg_fwd', L.ptr(vp), L.ptr(v), L.ptr(normal), L.ptr(graph.rowptr_out), L.ptr(graph.col_out), V,
               graph.E, L.ptr(w_lap), L.ptr(w_edge), terms, L.ptr(out), L.ptr(u), L.ptr(ws), ws.numel(), L.stream())
        ctx.graph, ctx.terms, ctx.has_u, ctx.has_w = graph, terms, u is not None, w_edge is not None
        ctx.save_for_backward(vp, v, u if u is not None else vp, w_edge if w_edge is not None else vp)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_lap, g_edge):
        vp, v, u, w_edge = ctx.saved_tensors
        g = ctx.graph
        gout = torch.stack([g_lap.reshape(()), g_edge.reshape(())]).float()
        gvp = torch.empty_like(vp)
        L.call('geobi_mesh_reg_bwd', L.ptr(vp), L.ptr(v), L.ptr(g.rowptr_out), L.ptr(g.col_out), vp.shape[0], g.E,
               L.ptr(u) if ctx.has_u else None, L.ptr(w_edge) if ctx.has_w else None, L.ptr(gout), ctx.terms, L.ptr(gvp),
               L.stream())
        return gvp, None, None, None, None, None, None


def mesh_reg(vp, v, graph, normal=None, w_lap=None, w_edge=None, terms=TERM_LAP | TERM_EDGE):
    """-> (L_lap, L_edge), two device scalars from one autograd node.  graph: graph.Graph of the vertices (loop-free,
    symmetric = True); normal [V, 3]: project the Laplacians on it (None: no projection); w_lap / w_edge [V]: per-row
    weights of a union batch, 1 / (B n_mesh) and 1 / (B E_mesh) (None: the plain means over vertices / CSR entries)."""
    return MeshRegFn.apply(vp, v, graph, normal, w_lap, w_edge, terms)


# ------------------------------------------------------- rigid ICP alignment (apply_icp's step)
ICP_STATE = 24   # GEOBI_ICP_STATE


class IcpResult(object):
    """What ops.icp returns.  xt float32 [Q, 3] on the device: the aligned points s x R + T; `state` the raw device
    float64 [P, GEOBI_ICP_STATE] (include/geobi_hip.h).  The rest is the final host read of that state, per part, as CPU
    tensors: R float64 [P, 3, 3], T float64 [P, 3], s, rmse float64 [P], iterations int64 [P], converged bool [P]."""
    __slots__ = ('xt', 'R', 'T', 's', 'rmse', 'iterations', 'converged', 'state', 'xptr')

    def __init__(self, xt, state, xptr):
        host = state.cpu()
        self.xt, self.state, self.xptr = xt, state, xptr
        self.R, self.T, self.s = host[:, :9].reshape(-1, 3, 3).clone(), host[:, 9:12].clone(), host[:, 12].clone()
        self.rmse, self.iterations, self.converged = host[:, 13].clone(), host[:, 15].long(), host[:, 16] != 0


def _icp_state(state, P):
    L.require_device(state, 'ICP state')
    if state.dtype != torch.float64 or tuple(state.shape) != (P, ICP_STATE) or not state.is_contiguous():
        raise L.GeobiError('ICP state must be a contiguous float64 [%d, %d] tensor, got %s %s'
                           % (P, ICP_STATE, state.dtype, tuple(state.shape)))
    return state


def icp_init(P, device, init=None):
    """A fresh state for P parts: the identity, or `init` [P, 13] = (R row-major, T, s) per part (array or tensor)."""
    state = torch.empty((int(P), ICP_STATE), dtype=torch.float64, device=device)
    L.require_device(state, 'ICP state')
    if init is not None:
        init = torch.as_tensor(init).to(device=device, dtype=torch.float64).contiguous()
        if tuple(init.shape) != (int(P), 13):
            raise L.GeobiError('icp: init must be [%d, 13] (R row-major, T, s per part), got %s' % (P, tuple(init.shape)))
    L.call('geobi_icp_init', L.ptr(state), int(P), L.ptr(init), L.stream())
    return state


def icp_apply(x, state, xptr=None, mode=0):
    """geobi_icp_apply: mode 0 -> s x R + T, mode 1 -> s x R^T (the gradient of mode 0 to x for a constant transform),
    per part of `xptr`, computed in fp64 and rounded once -> float32 [Q, 3]."""
    x = _points3(x, 'points')
    xp = _part_ptr(xptr, x.shape[0], 'xptr')
    P = len(xp) - 1
    _icp_state(state, P)
    if mode not in (0, 1):
        raise L.GeobiError('icp_apply: mode %r (0: s x R + T, 1: s x R^T)' % (mode,))
    (xa, xc) = _c_ptr(xp)
    out = torch.empty_like(x)
    L.call('geobi_icp_apply', L.ptr(x), xc, P, L.ptr(state), int(mode), L.ptr(out), L.stream())
    return out


def icp_step(x, y, idx, state, xt, xptr=None, yptr=None, relative_rmse_thr=1e-6, estimate_scale=False,
             allow_reflection=False):
    """geobi_icp_step: for every part that has not converged, the Umeyama alignment of the ORIGINAL x to y[idx], the new
    xt (written in place) and the new state (updated in place).  idx int32 [Q]: rows of y, as ops.nearest_parts(xt, y)
    returns them.  Nothing is read back: no sync."""
    x, y = _points3(x, 'points'), _points3(y, 'target points')
    Q = x.shape[0]
    xp, yp = _part_ptr(xptr, Q, 'xptr'), _part_ptr(yptr, y.shape[0], 'yptr')
    if len(xp) != len(yp):
        raise L.GeobiError('icp_step: %d point parts but %d target parts' % (len(xp) - 1, len(yp) - 1))
    P = len(xp) - 1
    _icp_state(state, P)
    L.require_device(idx, 'idx')
    L.require_device(xt, 'xt')
    if idx.dtype != torch.int32 or tuple(idx.shape) != (Q,) or not idx.is_contiguous():
        raise L.GeobiError('icp_step: idx must be a contiguous int32 [%d] tensor, got %s %s' % (Q, idx.dtype, tuple(idx.shape)))
    if xt.dtype != torch.float32 or xt.shape != x.shape or not xt.is_contiguous():
        raise L.GeobiError('icp_step: xt must be a contiguous float32 %s tensor, got %s %s'
                           % (tuple(x.shape), xt.dtype, tuple(xt.shape)))
    if xt.data_ptr() == x.data_ptr():
        raise L.GeobiError('icp_step: xt is x itself (every step aligns the ORIGINAL points; give xt its own storage)')
    if not relative_rmse_thr >= 0:
        raise L.GeobiError('icp_step: relative_rmse_thr %r is negative' % (relative_rmse_thr,))
    (xa, xc), (ya, yc) = _c_ptr(xp), _c_ptr(yp)
    ws = L.workspace(L.lib().geobi_icp_ws_bytes(xc, P), x.device)
    flags = (1 if estimate_scale else 0) | (2 if allow_reflection else 0)
    L.call('geobi_icp_step', L.ptr(x), L.ptr(y), L.ptr(idx), xc, yc, P, flags, float(relative_rmse_thr), L.ptr(state),
           L.ptr(xt), L.ptr(ws), ws.numel(), L.stream())


def icp(x, y, xptr=None, yptr=None, init=None, max_iterations=100, relative_rmse_thr=1e-6, estimate_scale=False,
        allow_reflection=False, check_every=4):
    """Rigid point-to-point ICP of x [Q, 3] onto y [M, 3], per part of a union batch (host part pointers as in
    nearest_parts): pytorch3d's iterative_closest_point as loss_v(..., apply_icp=True) calls it (code/network.py:364-367).
    xt = s x R + T; every iteration is nearest_parts(xt, y) followed by icp_step.  A part stops at iteration k >= 2 once
    (prev_rmse - rmse) / prev_rmse <= relative_rmse_thr, or when rmse == 0, and is frozen from then on; the loop ends when
    every part has stopped or after max_iterations.  The host reads the converged flags once every `check_every` iterations
    and once at the end; because converged parts are frozen the result does not depend on check_every.
    init: [P, 13] (R row-major, T, s) per part, applied to form the first xt only.  -> IcpResult."""
    x, y = _points3(x, 'points'), _points3(y, 'target points')
    xp, yp = _part_ptr(xptr, x.shape[0], 'xptr'), _part_ptr(yptr, y.shape[0], 'yptr')
    if len(xp) != len(yp):
        raise L.GeobiError('icp: %d point parts but %d target parts' % (len(xp) - 1, len(yp) - 1))
    if int(max_iterations) < 1 or int(check_every) < 1:
        raise L.GeobiError('icp: max_iterations and check_every are at least 1, got %r and %r' % (max_iterations, check_every))
    state = icp_init(len(xp) - 1, x.device, init)
    xt = icp_apply(x, state, xp, 0)
    for k in range(1, int(max_iterations) + 1):
        _, idx = nearest_parts(xt, y, xp, yp)
        icp_step(x, y, idx, state, xt, xp, yp, relative_rmse_thr, estimate_scale, allow_reflection)
        if k % int(check_every) == 0 and k < int(max_iterations) and bool((state[:, 16] != 0).all()):
            break
    return IcpResult(xt, state, xp)


class IcpAlignFn(Function):
    """x -> the ICP-aligned x with the transform treated as a CONSTANT: forward icp(x.detach(), y).xt, backward
    icp_apply(grad, mode=1) = s grad R^T.  pytorch3d differentiates through the SVD of the covariance; this does not
    (DESIGN.md 4j): the gradient is that of a fixed similarity, which is what moves vertices inside the aligned frame."""

    @staticmethod
    def forward(ctx, x, y, xptr, yptr, kw):
        res = icp(x.detach(), y, xptr, yptr, **kw)
        ctx.state, ctx.xp = res.state, res.xptr
        return res.xt

    @staticmethod
    def backward(ctx, gout):
        return icp_apply(gout, ctx.state, ctx.xp, 1), None, None, None, None


def icp_align(x, y, xptr=None, yptr=None, **kw):
    """The points x aligned to y by ops.icp (same keywords), differentiable with respect to x for a constant transform
    (IcpAlignFn).  network.loss_v(..., apply_icp=True) keeps raising; compose loss_v(ops.icp_align(vp, v), v, 'CD')."""
    return IcpAlignFn.apply(x, y, xptr, yptr, kw)
