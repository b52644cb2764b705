"""The one intake of a caller's mesh: arrays or tensors -> fp32 points and an int32 face table on the device, every
vertex id range-checked BEFORE a kernel gathers through it.  Every entry point that takes a mesh from outside comes
through here (filters, meshprep, meshclean, mesheval, meshnoise, patches, data_util, network).

The range check reads the table as it arrives -- where it lives, in its own dtype -- because the conversion to int32
wraps: the int64 id 2**32 + 1 becomes 1 and would pass a check made afterwards.

What the mesh tools' wrappers share beyond that is here too: the library's row limit, the test for a whole number, the
intake that also refuses non-finite points (``finite_mesh``), the paired array of an ``apply`` (``paired_points``).
"""
import numpy as np
import torch

from . import _lib as L

MAX_NODES = (1 << 24) - 1          # GEOBI_MAX_NODES of include/geobi_hip.h (tests/test_folders_host.py compares the two)


def whole(value):
    """whether value is a whole number: a Python or numpy integer, no bool"""
    return not isinstance(value, bool) and isinstance(value, (int, np.integer))


def bbox_diagonal(points):
    """the diagonal of the bounding box of points [V, 3] (an array or a tensor), in fp64 on the host (0 without points):
    the value of ``subdivide --max_edge_diag`` and ``remesh --target_edge_diag``"""
    p = np.asarray(points.detach().cpu().numpy() if torch.is_tensor(points) else points, dtype=np.float64).reshape(-1, 3)
    return float(np.sqrt(((p.max(axis=0) - p.min(axis=0)) ** 2).sum())) if p.shape[0] else 0.0


def as_tensor(a):
    """An array, a nested list or a tensor -> a tensor (a tensor as it is)."""
    return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a)


def to_device(a, device, dtype):
    """-> contiguous tensor of `dtype` on `device`; a tensor that already is one comes back itself (no copy)."""
    return as_tensor(a).to(device=device, dtype=dtype).contiguous()


def default_device(device, like=None):
    """The device a mesh tool works on: `device`, else that of the device tensor `like`, else the current one.
    GeobiError without a GPU or for a device that is none (there is no CPU fallback)."""
    if device is None and torch.is_tensor(like) and like.is_cuda:
        return like.device
    if not torch.cuda.is_available():
        raise L.GeobiError('the mesh tools run on the MI355X only (no CPU fallback)')
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != 'cuda':
        raise L.GeobiError('the mesh tools run on the MI355X only (no CPU fallback), got device %s' % dev)
    return dev


def check_faces(faces, num_vertices, what='faces', error=L.GeobiError):
    """Raise `error` unless every id of the table lies in [0, num_vertices).  The table is read as given -- before any
    conversion, on the device or the host it lives on: one reduction (the smallest and the largest id), and for a device
    table one host read that brings both (none for a host table).  An empty table passes."""
    t, V = as_tensor(faces), int(num_vertices)
    if t.numel() == 0:
        return
    if t.is_cuda:
        ends = torch.cat([e.reshape(1) for e in torch.aminmax(t)])
        if ends.dtype != torch.int32:       # cut to int32's range for the read: what was outside [0, V) stays outside
            ends = ends.clamp(-1, 2 ** 31 - 1).to(torch.int32)
        lo, hi = L.read_i32(ends)
    else:
        lo, hi = (e.item() for e in torch.aminmax(t))
    if not (lo >= 0 and hi < V):
        raise error('%s index vertices outside [0, %d)' % (what, V))


def device_mesh(points, faces, device=None, check=True, what='faces', error=L.GeobiError):
    """-> (points fp32 [V,3], faces int32 [F,3]) on the device (default_device(device, points)), contiguous; tensors that
    already fit come back themselves.  ValueError for other shapes; the face table is range-checked (check_faces, with
    `what` and `error`) unless check=False: a table this library produced."""
    pts, fv = as_tensor(points), as_tensor(faces)
    if pts.dim() != 2 or pts.shape[1] != 3 or fv.dim() != 2 or fv.shape[1] != 3:
        raise ValueError('points [V,3] and faces [F,3] expected, got %s and %s' % (tuple(pts.shape), tuple(fv.shape)))
    dev = default_device(device, pts)
    if check:
        check_faces(fv, pts.shape[0], what, error)
    return to_device(pts, dev, torch.float32), to_device(fv, dev, torch.int32)


def finite_mesh(points, faces, device, what):
    """``device_mesh`` for a mesh tool named `what`: a face index outside [0, V) and a non-finite coordinate are
    ValueErrors that name the tool."""
    pts, fv = device_mesh(points, faces, device, what='%s: faces' % what, error=ValueError)
    if pts.shape[0] > 0 and not bool(torch.isfinite(pts).all()):
        raise ValueError('%s: non-finite point coordinates' % what)
    return pts, fv


def paired_points(other, V, device, what):
    """The paired point array of an ``apply`` -> fp32 [V, 3] on the device; ValueError unless it has the V rows of the
    tool's input (`what`: 'a refinement of', ...)."""
    other = as_tensor(other)
    if other.dim() != 2 or other.shape[1] != 3 or other.shape[0] != V:
        raise ValueError('apply: points %s for %s %d vertices' % (tuple(other.shape), what, V))
    return to_device(other, device, torch.float32)
