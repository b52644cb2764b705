"""Data parallelism for the mesh path: one process per GPU, meshes sharded, gradients all-reduced.

The reference is single-device; its "batch_size" is gradient accumulation over sequential
single-mesh steps (/root/reference/code/train_dual.py:211-218).  Meshes are independent units
(no graph is ever split), so the only collective is ONE all-reduce of the flat fp32 gradient
bucket (939 128 elements = 3.76 MB) per optimiser step -- RCCL over xGMI with backend "nccl",
gloo on CPU for tests.  Eval metrics reduce as (sum, count) pairs like train_dual.py:246-259.
"""
import os

import torch
import torch.distributed as dist


def init_distributed(backend=None):
    """Reads RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* (torch.distributed.run); returns (rank, world, device)."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    use_cuda = torch.cuda.is_available()
    if use_cuda and os.environ.get('GEOBI_ALL_RANKS_ON_DEVICE0') == '1':
        local = 0          # rehearsal of the multi-rank path on a 1-GPU box (use with GEOBI_DIST_BACKEND=gloo)
    device = torch.device('cuda', local) if use_cuda else torch.device('cpu')
    if use_cuda:
        torch.cuda.set_device(device)
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29500')
        backend = backend or os.environ.get('GEOBI_DIST_BACKEND') or ('nccl' if use_cuda else 'gloo')
        kw = {}
        if use_cuda and backend == 'nccl':
            kw['device_id'] = device
        dist.init_process_group(backend, rank=rank, world_size=world, **kw)
    return rank, world, device


def shard_indices(num_items, rank, world, seed=0, epoch=0, shuffle=True):
    """Round-robin shard of a common permutation (same seed on every rank); every item appears
    on exactly one rank, ranks differ in length by at most one."""
    if shuffle:
        g = torch.Generator().manual_seed(seed * 1000003 + epoch)
        order = torch.randperm(num_items, generator=g).tolist()
    else:
        order = list(range(num_items))
    return order[rank::world]


def rank_world():
    """(rank, world size) of the default process group, (0, 1) without one."""
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def owns_patch(k, rank, world):
    """Inference on one large mesh across GPUs: patch k of the split (test_dual.py:53-58 runs them one
    after the other) belongs to rank k mod world."""
    return k % world == rank


def reduce_patch_sums(tensors, dst=0):
    """Sum the per-rank patch accumulators (Vp [V,3], Np [F,3], visit counts [V]) onto rank `dst`, in place there:
    the one collective of multi-GPU inference.  The buffers are packed into one fp32 message (counts are small
    integers, exact in fp32) so a mesh costs one reduction, not three."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return tensors
    flat = torch.cat([t.reshape(-1).to(torch.float32) for t in tensors])
    if flat.is_cuda and dist.get_backend() == 'gloo':
        # rehearsal of the multi-rank path on one device (GEOBI_DIST_BACKEND=gloo): gloo has no device-side reduce
        host = flat.cpu()
        dist.reduce(host, dst=dst, op=dist.ReduceOp.SUM)
        flat = host.to(flat.device)
    else:
        dist.reduce(flat, dst=dst, op=dist.ReduceOp.SUM)       # RCCL over xGMI
    if dist.get_rank() == dst:
        off = 0
        for t in tensors:
            n = t.numel()
            t.copy_(flat[off:off + n].view_as(t).to(t.dtype))
            off += n
    return tensors


class GradBucket(object):
    """All parameter gradients as views of one flat fp32 buffer: zeroing is one memset, the
    data-parallel reduction is one all-reduce, and nothing is copied in or out."""

    def __init__(self, params, direct=False):
        """direct=True lets the backward kernels ADD gradients straight into the bucket views
        (ops._direct_grad, `accumulate` in the C ABI): same semantics as autograd's accumulation into
        ``.grad`` -- backward passes between two `zero()` calls sum up -- without the per-parameter
        accumulate kernels."""
        self.params = [p for p in params if p.requires_grad]
        total = sum(p.numel() for p in self.params)
        ref = self.params[0]
        self.flat = torch.zeros(total, dtype=ref.dtype, device=ref.device)
        self.owner = None            # FlatParameters: the flat Parameter whose .grad must stay `self.flat`
        self._views = []
        off = 0
        for p in self.params:
            n = p.numel()
            v = self.flat[off:off + n].view_as(p)
            self._views.append(v)
            p.grad = v
            p._geobi_direct_grad = bool(direct)
            p._geobi_grad_ptr = v.data_ptr()
            p._geobi_bucket = self           # ops._direct_grad also checks the flat owner's .grad (FlatParameters)
            off += n

    def zero(self):
        """Zero every gradient (one memset) and re-attach any view an optimizer's
        ``zero_grad(set_to_none=True)`` or a stray assignment dropped since the last call."""
        self.flat.zero_()
        for p, v in zip(self.params, self._views):
            if p.grad is None or p.grad.data_ptr() != v.data_ptr():
                p.grad = v
        if self.owner is not None and self.owner.grad is not self.flat:
            self.owner.grad = self.flat

    def facet_offset(self, net):
        """Element offset in `flat` where the facet half (gnn_f, fc_f1, fc_f2) starts: DualGNN registers gnn_v, fc_v1,
        fc_v2 first, so the halves are two contiguous ranges.  Its gradients are final BEFORE the vertex branch's
        backward runs (the backward walks facet head -> gnn_f -> coupling -> vertex head -> gnn_v)."""
        first = next(net.gnn_f.parameters())
        off = 0
        for p in self.params:
            if p is first:
                return off
            off += p.numel()
        raise ValueError('the bucket does not hold the network\'s parameters')

    def all_reduce_mean_split(self, offset, events=None, comm_stream=None, _single_rank_too=False):
        """The same reduction as `all_reduce_mean` in two collectives: the tail [offset:] (the facet half) FIRST -- on
        `comm_stream` behind `events` (torch.cuda.Event list recorded by geobi_net_backward_facet_events) when given, so
        that it runs under the vertex branch's backward -- then the head [:offset].  Element-wise the same sums, so the
        reduced bucket is identical to the one-shot all-reduce."""
        if not (dist.is_available() and dist.is_initialized()):
            return self.flat
        if dist.get_world_size() == 1 and not _single_rank_too:      # (tests run the collectives on one rank as well)
            return self.flat
        world = dist.get_world_size()
        tail, head = self.flat[offset:], self.flat[:offset]
        # the early collective needs a backend that reduces on the device (RCCL); gloo stages through the host and only
        # makes sense one collective after the other (the rehearsal / CPU path)
        if events and self.flat.is_cuda and comm_stream is not None and dist.get_backend() == 'nccl':
            for ev in events:
                comm_stream.wait_event(ev)
            with torch.cuda.stream(comm_stream):
                work = dist.all_reduce(tail, op=dist.ReduceOp.SUM, async_op=True)
            dist.all_reduce(head, op=dist.ReduceOp.SUM)          # behind the whole backward, on the compute stream
            work.wait()                                          # the compute stream waits for the early collective
        else:
            dist.all_reduce(tail, op=dist.ReduceOp.SUM)
            dist.all_reduce(head, op=dist.ReduceOp.SUM)
        self.flat.div_(world)
        return self.flat

    def all_reduce_mean(self):
        """Sum over ranks then divide by the world size (= the reference's loss / batch_size)."""
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM)
            self.flat.div_(dist.get_world_size())
        return self.flat


class FlatParameters(object):
    """Parameters AND gradients as views of two flat buffers.

    The optimiser then updates ONE tensor (`flat_param`, 939 128 elements) instead of 76 small
    ones -- a handful of kernel launches per step -- and the module's own Parameter objects (and
    hence its state_dict) keep working because they alias the flat storage."""

    def __init__(self, module, direct=True):
        params = [p for p in module.parameters() if p.requires_grad]
        flat = torch.cat([p.detach().reshape(-1) for p in params])
        self.flat_param = torch.nn.Parameter(flat)
        off = 0
        for p in params:
            n = p.numel()
            p.data = self.flat_param.data[off:off + n].view_as(p)
            off += n
        self.bucket = GradBucket(params, direct=direct)
        self.bucket.owner = self.flat_param
        self.flat_param.grad = self.bucket.flat

    def parameters(self):
        return [self.flat_param]


def reduce_sums(values, device):
    """All-reduce a list of python/tensor scalars (sums and counts of the eval loop)."""
    t = torch.tensor([float(v) for v in values], dtype=torch.float64, device=device)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        if t.is_cuda:
            t = t.float()          # RCCL path: fp32 is plenty for six scalars
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t.double().tolist()


def _mesh_weights(data):
    """Per-row weights 1 / (B * n_mesh) of a disjoint-union batch (cached on the Data bag)."""
    ptr = getattr(data, 'mesh_ptr', None)
    if ptr is None or ptr.numel() <= 2:
        return None
    w = getattr(data, '_loss_weights', None)
    if w is None or w.device != data.y.device:
        dev = data.y.device
        counts = ptr[1:] - ptr[:-1]
        per_mesh = (1.0 / (counts.float() * counts.numel())).to(dev)
        if dev.type == 'cuda' and not ptr.is_cuda:
            # expand on the device (two small kernels) instead of on the host + a copy of N floats
            seg = torch.bucketize(torch.arange(int(ptr[-1]), device=dev), ptr[1:].to(dev), right=True)
            w = per_mesh[seg]
        else:
            w = torch.repeat_interleave(per_mesh, counts.to(dev))
        data._loss_weights = w
    return w


def _cpu_nearest(q, t, chunk=2048):
    """argmin_j |q_i - t_j|^2 by plain torch ops (the CPU statement of the search): chunks of queries against all the
    targets, distances from coordinate differences, torch.argmin's first minimum = the lowest index."""
    idx = torch.empty(q.shape[0], dtype=torch.long, device=q.device)
    for s in range(0, q.shape[0], chunk):
        d = q[s:s + chunk, None, :] - t[None, :, :]
        idx[s:s + chunk] = d.pow(2).sum(2).argmin(1)
    return idx


def _cpu_chamfer(p, t):
    """Chamfer distance of one mesh, gradient to p only with the two arg-min maps as constants."""
    t = t.detach()
    with torch.no_grad():
        a, b = _cpu_nearest(p, t), _cpu_nearest(t, p)
    return (p - t[a]).pow(2).sum(1).mean() + (p[b] - t).pow(2).sum(1).mean()


def batched_losses(vp, npred, data_v, data_f, loss_v='L1', loss_n='L1', sampling=None):
    """Per-mesh mean losses averaged over the meshes of a disjoint-union batch.

    Identical to accumulating ``loss / batch_size`` over sequential single-mesh steps
    (train_dual.py:204-212).  Without ``mesh_ptr`` it is the plain per-node mean.  On the MI355X
    this is the fused reduction kernel (geobi_row_loss_*), for 'CD' / 'sided' on top of the per-mesh search
    (geobi_nearest_parts, geobi_chamfer_*); CPU tensors (gloo tests) use torch ops.

    'SCD' (device only: the sampler has no CPU form) draws per mesh through the ``mesh_ptr`` of both bags over
    ``data_f.fv_indices``; sampling = dict(n, seed, draw, stream_ids) names the draw (ops.sampled_chamfer_loss; missing
    keys take its defaults)."""
    from . import network
    network.check_loss_names(loss_v, loss_n)
    if loss_v == 'SCD' and not vp.is_cuda:
        raise ValueError("batched_losses: loss_v = 'SCD' draws its points with the surface sampler, which runs on the device "
                         'only (no CPU fallback); the tensors are on %s' % vp.device)
    kinds = {'L1': 0, 'L2': 1}
    ptr_v, ptr_f = getattr(data_v, 'mesh_ptr', None), getattr(data_f, 'mesh_ptr', None)
    if vp.is_cuda:
        from . import ops
        wv, wn = _mesh_weights(data_v), _mesh_weights(data_f)
        if loss_v == 'CD':
            lv = ops.chamfer_loss(vp, data_v.y, ptr_v, ptr_v)
        elif loss_v == 'SCD':
            # the face table is the bag's own (union_batch_graphs offsets it with the vertices): no range check, no read
            lv = ops.sampled_chamfer_loss(vp, data_v.y, data_f.fv_indices, ptr_f, ptr_v, check=False, **(sampling or {}))
        else:
            lv = ops.row_loss(vp, data_v.y, kinds[loss_v], wv, 1.0 if wv is not None else None)
        if loss_n == 'sided':
            from .data_util import face_centroids
            fc_p, fc = face_centroids(vp, data_f.fv_indices), face_centroids(data_v.y, data_f.fv_indices)
            ln = ops.sided_loss(npred, data_f.y, fc_p, fc, ptr_f, wn)
        else:
            ln = ops.row_loss(npred, data_f.y, kinds[loss_n], wn, 1.0 if wn is not None else None)
        return lv, ln

    def per_node(a, b, kind):
        d = a - b
        return d.abs().sum(1) if kind == 'L1' else d.pow(2).sum(1)

    def reduce(vals, ptr):
        if ptr is None or ptr.numel() <= 2:
            return vals.mean()
        counts = (ptr[1:] - ptr[:-1]).to(vals.device)
        w = torch.repeat_interleave(1.0 / (counts.to(vals.dtype) * counts.numel()), counts)
        return (vals * w).sum()

    def spans(ptr, n):
        cut = [0, n] if ptr is None else [int(v) for v in ptr.tolist()]
        return list(zip(cut[:-1], cut[1:]))

    if loss_v == 'CD':
        sp = spans(ptr_v, vp.shape[0])
        lv = sum(_cpu_chamfer(vp[a:b], data_v.y[a:b]) for a, b in sp) / len(sp)
    else:
        lv = reduce(per_node(vp, data_v.y, loss_v), ptr_v)
    if loss_n == 'sided':
        fv = data_f.fv_indices.long()
        with torch.no_grad():
            fc_p, fc = vp.detach()[fv].sum(1) / 3.0, data_v.y[fv].sum(1) / 3.0
            idx = torch.cat([a + _cpu_nearest(fc_p[a:b], fc[a:b]) for a, b in spans(ptr_f, fc.shape[0])])
        ln = reduce(per_node(npred, data_f.y[idx], 'L1'), ptr_f)
    else:
        ln = reduce(per_node(npred, data_f.y, loss_n), ptr_f)
    return lv, ln


def _edge_weights(data, graph):
    """Per-row weights 1 / (B * E_mesh) of the CSR entries of a union batch, E_mesh = the entries of the row's own mesh:
    rowptr_out read at the mesh_ptr rows, on the device, nothing comes back to the host (cached on the Data bag)."""
    ptr = getattr(data, 'mesh_ptr', None)
    if ptr is None or ptr.numel() <= 2:
        return None
    w = getattr(data, '_edge_weights', None)
    if w is None or w.device != graph.rowptr_out.device:
        dev = graph.rowptr_out.device
        ptr_d = ptr.to(dev)
        ends = graph.rowptr_out[ptr_d]
        counts = (ends[1:] - ends[:-1]).float()
        per_mesh = torch.where(counts > 0, 1.0 / (counts * counts.numel()), torch.zeros_like(counts))
        seg = torch.bucketize(torch.arange(int(ptr[-1]), device=dev), ptr_d[1:], right=True)
        w = data._edge_weights = per_mesh[seg]
    return w


def batched_regularisers(vp, data_v, lap=True, edge=True):
    """The mesh regularisers of a prediction vp against data_v.y over data_v's vertex graph, as batched_losses forms the
    other losses: per-mesh means averaged over the meshes of a disjoint-union batch (mesh_ptr), the plain means without
    one.  -> (Laplacian term, edge-length term); a term that is switched off is None.  On the MI355X both come from ONE
    ops.mesh_reg call (geobi_mesh_reg_*); CPU tensors (gloo tests) use torch ops over data_v.edge_index."""
    if not (lap or edge):
        return None, None
    if vp.is_cuda:
        from . import ops
        g = data_v.graph()
        terms = (ops.TERM_LAP if lap else 0) | (ops.TERM_EDGE if edge else 0)
        l_lap, l_edge = ops.mesh_reg(vp, data_v.y, g, None, _mesh_weights(data_v) if lap else None,
                                     _edge_weights(data_v, g) if edge else None, terms)
        return (l_lap if lap else None), (l_edge if edge else None)
    from . import network
    ptr = getattr(data_v, 'mesh_ptr', None)
    cut = [0, vp.shape[0]] if ptr is None else [int(x) for x in ptr.tolist()]
    ei = data_v.edge_index
    terms = [[], []]
    for a, b in zip(cut[:-1], cut[1:]):
        inside = (ei[0] >= a) & (ei[0] < b)
        sub = ei[:, inside] - a
        if lap:
            terms[0].append(network.laplacian_loss(vp[a:b], data_v.y[a:b], sub))
        if edge:
            terms[1].append(network.edge_length_loss(vp[a:b], data_v.y[a:b], sub))
    return tuple(sum(t) / len(t) if t else None for t in terms)


def add_regularisers(loss, vp, data_v, lap_scale=0, edge_scale=0):
    """loss + lap_scale * L_lap + edge_scale * L_edge for the scales that are not 0 (batched_regularisers; with both 0 no
    call is made and `loss` comes back as it is).  -> (loss, the unscaled terms that are on, detached, in that order)"""
    if lap_scale == 0 and edge_scale == 0:
        return loss, []
    on = []
    for term, scale in zip(batched_regularisers(vp, data_v, lap_scale != 0, edge_scale != 0), (lap_scale, edge_scale)):
        if term is not None:
            loss = loss + scale * term
            on.append(term.detach())
    return loss, on
