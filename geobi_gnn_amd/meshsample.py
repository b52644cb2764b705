"""Points drawn uniformly by area on a mesh surface, on the MI355X (geobi_sample_weights, geobi_sample_surface): what
``sample`` writes, what ``eval --free --samples`` measures from and what ``align --samples`` aligns to.

The reference has no counterpart: every distance of its evaluation starts from a vertex (code/data_util.py:584-616),
which sees nothing of what happens inside a large triangle of a CAD model.

The face weights are integers and the generator is counter-based (Philox4x32-10, one counter per sample,
block 2 beside the noise kernel's 0 and 1), so a sample is a pure function of (mesh, seed, stream_id, draw, first + i):
it does not depend on how many samples a call draws or on how a draw is cut into calls.

surface_weights_parts / sample_surface_parts do the same for every mesh of a union batch in one call: what
the sampled Chamfer loss (ops.sampled_chamfer_loss, ``train --loss_v SCD``) draws from.
"""
import collections
import math

import torch

from . import _lib as L
from . import meshin

SurfaceSamples = collections.namedtuple('SurfaceSamples', 'points face bary')   # [n,3] float32, [n] int32, [n,3] float32


def table_entries():
    """Entries of ``cum`` a block of the draw kernel stages in LDS: at or below it the search never leaves LDS."""
    return int(L.lib().geobi_sample_table_entries())


def _mesh(points, faces, check):
    """Device points float32 [V,3] and faces int32 [F,3] as the kernels take them; the ids range-checked unless check=False
    (a table that came through meshin.device_mesh)."""
    L.require_device(points, 'points')
    L.require_device(faces, 'faces')
    if points.dim() != 2 or points.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError('points [V,3] and faces [F,3] expected, got %s and %s' % (tuple(points.shape), tuple(faces.shape)))
    if points.shape[0] == 0 or faces.shape[0] == 0:
        raise L.GeobiError('surface sampling: a mesh without area (V = %d, F = %d)' % (points.shape[0], faces.shape[0]))
    if check:
        meshin.check_faces(faces, points.shape[0])           # range-checked before a kernel walks it
    return points.detach().to(torch.float32).contiguous(), faces.to(torch.int32).contiguous()


def _weights(p, fv):
    """-> (weight int64 [F], cum int64 [F], exponent int32 [1]), all on the device, nothing read back."""
    F, dev = fv.shape[0], p.device
    weight = torch.empty(F, dtype=torch.int64, device=dev)
    cum = torch.empty(F, dtype=torch.int64, device=dev)
    exponent = torch.empty(1, dtype=torch.int32, device=dev)
    ws = L.workspace(L.size_query('geobi_sample_ws_bytes', F), dev)
    L.call('geobi_sample_weights', L.ptr(p), L.ptr(fv), F, p.shape[0], L.ptr(weight), L.ptr(cum), L.ptr(exponent), L.ptr(ws),
           ws.numel(), L.stream())
    return weight, cum, exponent


def _read_total(cum, *more):
    """cum[-1] (an int64 in two int32 halves) and the int32 device scalars of ``more``, in ONE host read."""
    host = L.read_i32(torch.cat([cum[-1:].view(torch.int32)] + [m.reshape(1).to(torch.int32) for m in more]))
    return [(host[0] & 0xffffffff) | (host[1] << 32)] + host[2:]


def surface_weights(points, faces, check=True):
    """Device mesh -> (weight int64 [F], cum int64 [F], exponent int): weight[f] = floor(|e1 x e2| * 2^(32 - exponent)) with
    2^exponent just above the largest |e1 x e2|, cum its inclusive scan.  A face without area has weight 0 and is never
    drawn.  One host read (the exponent)."""
    weight, cum, exponent = _weights(*_mesh(points, faces, check))
    return weight, cum, L.read_i32(exponent)[0]


def surface_info(weights):
    """(area, number of zero-weight faces) of surface_weights' result: area = ldexp(cum[-1], exponent - 33), the sum of
    the quantised face areas.  One host read."""
    weight, cum, exponent = weights
    total, zero = _read_total(cum, (weight == 0).sum())
    return math.ldexp(total, exponent - 33), zero


def sample_surface(points, faces, n, *, seed, stream_id=0, draw=0, first=0, weights=None, check=True):
    """n points drawn uniformly by area on the surface of a device mesh -> SurfaceSamples(points float32 [n,3], face
    int32 [n], bary float32 [n,3]): points[i] = sum_k bary[i,k] * corner k of faces[face[i]].  Sample i is a function of
    (mesh, seed, stream_id, draw, first + i) only: the first rows of a longer draw are the shorter draw, and
    ``first = k`` continues a draw at its row k.  weights: surface_weights' result for this mesh, to draw several times from
    one scan.  GeobiError for a CPU tensor, a face id outside [0, V) and a mesh without area (one read of cum[-1]);
    ValueError for a negative n or first, numbers out of range, first + n above the library's row limit."""
    p, fv = _mesh(points, faces, check)
    n, first = int(n), int(first)
    if n < 0 or first < 0:
        raise ValueError('sample_surface: n = %d, first = %d (neither may be negative)' % (n, first))
    if first + n > meshin.MAX_NODES:
        raise ValueError('sample_surface: first + n = %d exceeds %d rows per draw' % (first + n, meshin.MAX_NODES))
    if not 0 <= int(seed) < 2 ** 64 or not 0 <= int(stream_id) < 2 ** 32 or not 0 <= int(draw) < 2 ** 32:
        raise ValueError('sample_surface: seed is 64 bits, stream_id and draw are 32 bits, none negative')
    F, dev = fv.shape[0], p.device
    if weights is None:
        cum = _weights(p, fv)[1]
    else:
        cum = weights[1]
        L.require_device(cum, 'weights')
        if cum.dtype != torch.int64 or cum.shape != (F,):
            raise ValueError('sample_surface: weights of another mesh (cum %s %s for F = %d)' % (cum.dtype, tuple(cum.shape), F))
        cum = cum.contiguous()
    if _read_total(cum)[0] <= 0:
        raise L.GeobiError('surface sampling: a mesh without area (every one of its %d faces is degenerate)' % F)
    out = SurfaceSamples(torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                         torch.empty((n, 3), dtype=torch.float32, device=dev))
    L.call('geobi_sample_surface', L.ptr(p), L.ptr(fv), L.ptr(cum), F, p.shape[0], n, first, int(seed), int(stream_id),
           int(draw), L.ptr(out.points), L.ptr(out.face), L.ptr(out.bary), L.stream())
    return out


# ------------------------------------------------------------------------------- every mesh of a union batch in one call
def _face_ptr(fptr, F):
    """Host face pointer of a union batch -> (list of ints, ctypes array, its address); it must cut the F rows of the face
    table from 0 to F with no empty part."""
    import ctypes
    lst = [int(v) for v in (fptr.tolist() if torch.is_tensor(fptr) else fptr)]
    if len(lst) < 2 or lst[0] != 0 or lst[-1] != int(F):
        raise L.GeobiError('fptr %r does not cover the %d rows it cuts (it must run from 0 to %d)' % (lst, F, F))
    if any(b <= a for a, b in zip(lst[:-1], lst[1:])):
        raise L.GeobiError('surface sampling: fptr %r has an empty part (a mesh without area)' % (lst,))
    arr = (ctypes.c_int64 * len(lst))(*lst)
    return lst, arr, ctypes.cast(arr, ctypes.c_void_p)


def _weights_parts(p, fv, fp):
    """-> (weight int64 [F], cum int64 [F], exponent int32 [P]), all on the device, nothing read back."""
    lst, _arr, addr = fp
    F, P, dev = fv.shape[0], len(lst) - 1, p.device
    weight = torch.empty(F, dtype=torch.int64, device=dev)
    cum = torch.empty(F, dtype=torch.int64, device=dev)
    exponent = torch.empty(P, dtype=torch.int32, device=dev)
    ws = L.workspace(L.size_query('geobi_sample_parts_ws_bytes', F, P), dev)
    L.call('geobi_sample_weights_parts', L.ptr(p), L.ptr(fv), addr, P, p.shape[0], L.ptr(weight), L.ptr(cum),
           L.ptr(exponent), L.ptr(ws), ws.numel(), L.stream())
    return weight, cum, exponent


def surface_weights_parts(points, faces, fptr, check=True):
    """surface_weights for every mesh of a union batch (faces [F,3] with global vertex ids, host face pointer fptr [P+1]) in
    one call -> (weight int64 [F], cum int64 [F], exponent int32 [P]), all on the device, nothing read back: on the rows
    of part p, weight and cum are exactly what surface_weights gives on that mesh alone, exponent[p] its exponent."""
    p, fv = _mesh(points, faces, check)
    return _weights_parts(p, fv, _face_ptr(fptr, fv.shape[0]))


def sample_surface_parts(points, faces, fptr, n, *, seed, stream_ids, draw=0, first=0, weights=None, check=True):
    """n points per mesh of a union batch -> SurfaceSamples(points float32 [P*n,3], face int32 [P*n], bary float32 [P*n,3]):
    rows p*n .. (p+1)*n are sample_surface of mesh p alone with stream_id = stream_ids[p] and the same seed, draw and first,
    bit for bit; face is a row of ``faces`` (the single-mesh face plus fptr[p]).  weights: surface_weights_parts' result
    for this batch.  The refusals of sample_surface; the GeobiError for a mesh without area names the part (one host read
    of the P totals)."""
    p, fv = _mesh(points, faces, check)
    fp = _face_ptr(fptr, fv.shape[0])
    lst, P = fp[0], len(fp[0]) - 1
    n, first = int(n), int(first)
    if n < 0 or first < 0:
        raise ValueError('sample_surface_parts: n = %d, first = %d (neither may be negative)' % (n, first))
    if first + n > meshin.MAX_NODES or P * n > meshin.MAX_NODES:
        raise ValueError('sample_surface_parts: first + n = %d, P * n = %d: above %d rows per draw'
                         % (first + n, P * n, meshin.MAX_NODES))
    sid = [int(s) for s in (stream_ids.tolist() if torch.is_tensor(stream_ids) else stream_ids)]
    if len(sid) != P:
        raise ValueError('sample_surface_parts: %d stream ids for %d parts' % (len(sid), P))
    if not 0 <= int(seed) < 2 ** 64 or not 0 <= int(draw) < 2 ** 32 or not all(0 <= s < 2 ** 32 for s in sid):
        raise ValueError('sample_surface_parts: seed is 64 bits, stream_ids and draw are 32 bits, none negative')
    F, dev = fv.shape[0], p.device
    if weights is None:
        cum = _weights_parts(p, fv, fp)[1]
    else:
        cum = weights[1]
        L.require_device(cum, 'weights')
        if cum.dtype != torch.int64 or cum.shape != (F,):
            raise ValueError('sample_surface_parts: weights of another batch (cum %s %s for F = %d)'
                             % (cum.dtype, tuple(cum.shape), F))
        cum = cum.contiguous()
    ends = torch.tensor([e - 1 for e in lst[1:]], dtype=torch.int64, device=dev)
    # the P totals in one host read of one number: the first part without area, P if there is none
    flat = torch.where(cum[ends] <= 0, torch.arange(P, device=dev), torch.full((), P, device=dev)).min()
    k = L.read_i32(flat.to(torch.int32).reshape(1))[0]
    if k < P:
        raise L.GeobiError('surface sampling: part %d is a mesh without area (every one of its %d faces is degenerate)'
                           % (k, lst[k + 1] - lst[k]))
    out = SurfaceSamples(torch.empty((P * n, 3), dtype=torch.float32, device=dev),
                         torch.empty(P * n, dtype=torch.int32, device=dev),
                         torch.empty((P * n, 3), dtype=torch.float32, device=dev))
    import ctypes
    sid_arr = (ctypes.c_uint32 * P)(*sid)
    L.call('geobi_sample_surface_parts', L.ptr(p), L.ptr(fv), L.ptr(cum), fp[2], P, p.shape[0], n, first, int(seed),
           ctypes.cast(sid_arr, ctypes.c_void_p), int(draw), L.ptr(out.points), L.ptr(out.face), L.ptr(out.bary), L.stream())
    return out


def sample_normals(points, faces, samples):
    """Unit normal of every sample's face [n,3]: computer_face_normal followed by geobi_gather_rows."""
    from .data_util import computer_face_normal
    fn = computer_face_normal(points.detach(), faces).contiguous()
    out = torch.empty((samples.face.shape[0], 3), dtype=torch.float32, device=fn.device)
    if out.shape[0]:
        L.call('geobi_gather_rows', L.ptr(fn), L.ptr(samples.face), 3, out.shape[0], L.ptr(out), L.stream())
    return out
