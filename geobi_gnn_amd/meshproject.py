"""Closest points on a mesh surface on the MI355X: WHERE on the surface the nearest point of a
query lies -- the triangle (``mesheval.point_to_mesh``'s all-pairs search, unchanged), the barycentric weights in it, the
position and the distance (csrc/project.hip: geobi_closest_on_faces, one lane per query, fp64 in one stated order).

The (face, bary) address is a map: ``apply`` evaluates it on any other vertex array of the same mesh
(``ops.bary_points``), which gives the counterpart of every projected point on a paired file -- what lets
``meshremesh.remesh(project=True)`` carry ``noisy/`` along.  ``project`` snaps points -- a result, a scan, a sampled
cloud -- onto a reference surface.

The rules are stated in include/geobi_hip.h; tests/project_model.py restates them and reproduces every bit given the
search's faces.  No CPU fallback.
"""
import math

import torch

from . import _lib as L
from . import mesheval, meshgrid, meshin, ops

MAX_NODES = meshin.MAX_NODES


class Closest(object):
    """face [Q] int32, bary [Q, 3] float32, points [Q, 3] float32, dist [Q] float32 on the device; faces [F, 3] int32: the
    table the face ids index (for ``apply``), V: the vertices of the mesh"""

    def __init__(self, face, bary, points, dist, faces, V):
        self.face, self.bary, self.points, self.dist, self.faces, self.V = face, bary, points, dist, faces, V


def check_queries(points, what='closest'):
    """ValueError unless points is [Q, 3] with 1 <= Q <= GEOBI_MAX_NODES -> the tensor, where it lives"""
    q = meshin.as_tensor(points)
    if q.dim() != 2 or q.shape[1] != 3:
        raise ValueError('%s: points [Q, 3] expected, got %s' % (what, tuple(q.shape)))
    if not 1 <= q.shape[0] <= MAX_NODES:
        raise ValueError('%s: %d query points (at least one, at most GEOBI_MAX_NODES = %d)' % (what, q.shape[0], MAX_NODES))
    return q


def _surface(verts, faces, device, what):
    v, fv = meshin.finite_mesh(verts, faces, device, what)
    if v.shape[0] == 0 or fv.shape[0] == 0:
        raise ValueError('%s: a surface of %d vertices and %d faces (at least one of each)' % (what, v.shape[0], fv.shape[0]))
    if max(v.shape[0], fv.shape[0]) > MAX_NODES:
        raise ValueError('%s: %d vertices and %d faces, beyond GEOBI_MAX_NODES = %d' % (what, v.shape[0], fv.shape[0], MAX_NODES))
    return v, fv


def closest_on_faces(q, verts, fv, face):
    """geobi_closest_on_faces on device tensors as they are (q [Q, 3] and verts [V, 3] float32, fv [F, 3] and face [Q] int32,
    contiguous) -> (bary [Q, 3], points [Q, 3], dist [Q])"""
    Q = q.shape[0]
    bary = torch.empty((Q, 3), dtype=torch.float32, device=q.device)
    points = torch.empty((Q, 3), dtype=torch.float32, device=q.device)
    dist = torch.empty(Q, dtype=torch.float32, device=q.device)
    L.call('geobi_closest_on_faces', L.ptr(q), L.ptr(verts), L.ptr(fv), L.ptr(face), Q, verts.shape[0], fv.shape[0], L.ptr(bary),
           L.ptr(points), L.ptr(dist), L.stream())
    return bary, points, dist


def _closest(q, v, fv, index=None):
    """the search (index: as mesheval.point_to_mesh) and the step behind it on checked device tensors -> Closest"""
    face = mesheval.point_to_mesh(q, v, fv, index=index)[1]
    bary, points, dist = closest_on_faces(q, v, fv, face)
    return Closest(face, bary, points, dist, fv, v.shape[0])


def closest(points, verts, faces, device=None, index=None):
    """For every row of points [Q, 3] its closest point on the surface (verts [V, 3], faces [F, 3]) -> Closest.  Arrays or
    tensors; a query with a coordinate that is not finite gets dist = +inf and the first corner of its face.  ValueError:
    other shapes, no query, an empty surface, a face index outside [0, V), non-finite vertices, sizes beyond
    GEOBI_MAX_NODES.  index: None searches all pairs, 'grid' through a meshgrid.TriangleGrid built here, or through one
    built over this surface before; the same bits either way."""
    index = meshgrid.check_index(index)
    q = check_queries(points, 'closest')                  # before the device is asked for: checked without one
    dev = meshin.default_device(device, meshin.as_tensor(verts))
    v, fv = _surface(verts, faces, dev, 'closest')
    q = meshin.to_device(q, dev, torch.float32)
    with torch.cuda.device(dev):
        return _closest(q, v, fv, index)


def apply(closest, other_verts):
    """The counterpart of every projected point on another vertex array of the same mesh (other_verts [V, 3]):
    ``ops.bary_points(other_verts, faces, face, bary)`` -> float32 [Q, 3] on the device.  On the surface's own vertices this
    is ``closest.points`` bit for bit."""
    other = meshin.paired_points(other_verts, closest.V, closest.face.device, 'a projection onto')
    with torch.cuda.device(other.device):
        return ops.bary_points(other, closest.faces, closest.face, closest.bary)


def check_max_dist(max_dist, what='project'):
    """ValueError unless max_dist is None or a number that is not negative (inf allowed: no limit) -> float or None"""
    if max_dist is None:
        return None
    try:
        value = float(max_dist)
    except (TypeError, ValueError):
        raise ValueError('%s: max_dist = %r (a distance, not negative)' % (what, max_dist))
    if math.isnan(value) or value < 0.0:
        raise ValueError('%s: max_dist = %r (a distance, not negative)' % (what, max_dist))
    return value


def project(points, verts, faces, max_dist=None, device=None, index=None):
    """points [Q, 3] moved to their closest points on the surface -> (projected float32 [Q, 3] on the device, kept, Closest).
    A row whose distance is above ``max_dist`` (None: no limit) keeps its coordinates -- a query that is not finite always
    does -- and ``kept`` is the number of such rows.  index: as ``closest``."""
    index = meshgrid.check_index(index)
    max_dist = check_max_dist(max_dist)
    q = check_queries(points, 'project')
    dev = meshin.default_device(device, meshin.as_tensor(verts))
    v, fv = _surface(verts, faces, dev, 'project')
    q = meshin.to_device(q, dev, torch.float32)
    with torch.cuda.device(dev):
        c = _closest(q, v, fv, index)
        keep = ~torch.isfinite(c.dist) if max_dist is None else ~(c.dist <= max_dist)
        out = torch.where(keep[:, None], q, c.points)
        return out, int(keep.sum()), c
