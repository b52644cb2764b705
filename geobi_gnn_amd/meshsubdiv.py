"""Triangle-mesh refinement on the MI355X: make a mesh denser with correct connectivity, and keep a
paired point array (the noisy copy of an original) in row-by-row correspondence.

* **midpoint, uniform** (``levels=K``): every edge gets a vertex at its midpoint, every face becomes four; the surface is
  unchanged
* **Loop, uniform** (``scheme='loop'``): the same connectivity with Loop's masks (Warren's weights); an edge that is not
  shared by exactly two faces is a crease
* **max-edge, adaptive** (``max_edge=L``): only the edges longer than L are split, each face takes the template of its 0 / 1 /
  2 / 3 split edges, rounds repeat until no edge is longer than L.  A round conforms by construction: a midpoint belongs
  to the edge, so every face on the edge sees it

The rules -- which edge gets which vertex, the order and winding of the children, every rounding of a position -- are
stated in include/geobi_hip.h (geobi_subdiv_*); the topology is integer-exact and the positions reproducible bit for bit
(tests/subdiv_model.py).  No CPU fallback.
"""
import math

import numpy as np
import torch

from . import _lib as L
from . import meshin

SCHEMES = ('midpoint', 'loop')
MAX_NODES = meshin.MAX_NODES
COUNT_KEYS = ('edges', 'split', 'boundary_edges', 'complex_edges')


class Pass(object):
    """One pass as ``apply`` needs it: the face table it refined (device int32 [F, 3]), its sizes, and the workspace that
    holds the plan.  counts: edges, split, boundary_edges, complex_edges of this pass's input."""

    def __init__(self, faces, V, Vn, Fn, loop, ws, counts):
        self.faces, self.V, self.Vn, self.Fn, self.loop, self.ws, self.counts = faces, V, Vn, Fn, loop, ws, counts


class Refined(object):
    """points [V', 3] float32, faces [F', 3], face_parent [F'] (the INPUT's face every face came from, composed across the
    passes), vertex_parents [V', 2] (of the last pass: (v, v) for a row it kept, the two ends of the split edge for a row it
    added) int32, all on the device; counts: edges, boundary_edges, complex_edges of the input, split (edges split over all
    passes = V' - V), passes; passes: the Pass records."""

    def __init__(self, points, faces, face_parent, vertex_parents, counts, passes):
        self.points, self.faces, self.face_parent, self.vertex_parents = points, faces, face_parent, vertex_parents
        self.counts, self.passes = counts, passes


def check_args(levels=1, scheme='midpoint', max_edge=None, max_rounds=16):
    """ValueError for what ``subdivide`` does not take; -> max_edge as the float32 the device compares with (or None)."""
    if scheme not in SCHEMES:
        raise ValueError('subdivide: scheme = %r (one of %s)' % (scheme, ', '.join(SCHEMES)))
    if not meshin.whole(levels) or levels < 1:
        raise ValueError('subdivide: levels = %r (a whole number, at least 1)' % (levels,))
    if not meshin.whole(max_rounds) or max_rounds < 1:
        raise ValueError('subdivide: max_rounds = %r (a whole number, at least 1)' % (max_rounds,))
    if max_edge is None:
        return None
    if scheme == 'loop':
        raise ValueError('subdivide: max_edge splits at midpoints; it cannot be combined with the Loop scheme')
    if levels != 1:
        raise ValueError('subdivide: max_edge runs rounds until no edge is longer; it cannot be combined with levels')
    try:
        edge = float(np.float32(max_edge))
    except (TypeError, ValueError):
        raise ValueError('subdivide: max_edge = %r (a positive length)' % (max_edge,))
    if not (edge > 0.0 and math.isfinite(edge)):
        raise ValueError('subdivide: max_edge = %r (positive and finite as a float32)' % (max_edge,))
    return edge


def _plan(fv, pts, loop, max_edge, stage_ms=None):
    """geobi_subdiv_plan on a device mesh -> (workspace, [edges, split, boundary, complex, V', F']); one wait"""
    F, V = fv.shape[0], pts.shape[0]
    ws = L.workspace(L.size_query('geobi_subdiv_ws_bytes', F, V), fv.device)
    counts = torch.zeros(8, dtype=torch.int32, device=fv.device)
    L.call('geobi_subdiv_plan', L.ptr(fv), L.ptr(pts), F, V, int(loop), int(max_edge is not None), float(max_edge or 0.0),
           L.ptr(counts), stage_ms, L.ptr(ws), ws.numel(), L.stream())
    return ws, L.read_i32(counts, 6)


def _emit(fv, pts, loop, Vn, Fn, ws):
    dev, F, V = fv.device, fv.shape[0], pts.shape[0]
    faces = torch.empty((Fn, 3), dtype=torch.int32, device=dev)
    face_parent = torch.empty(Fn, dtype=torch.int32, device=dev)
    vertex_parents = torch.empty((Vn, 2), dtype=torch.int32, device=dev)
    points = torch.empty((Vn, 3), dtype=torch.float32, device=dev)
    L.call('geobi_subdiv_emit', L.ptr(fv), L.ptr(pts), F, V, int(loop), Vn, Fn, L.ptr(faces), L.ptr(face_parent),
           L.ptr(vertex_parents), L.ptr(points), L.ptr(ws), ws.numel(), L.stream())
    return points, faces, face_parent, vertex_parents


def subdivide(points, faces, levels=1, scheme='midpoint', max_edge=None, max_rounds=16, device=None):
    """(points [V, 3], faces [F, 3]) -> Refined.  ``levels`` uniform passes of ``scheme``, or with ``max_edge = L`` rounds
    that split the edges longer than L (compared as float32) until none is left.  ValueError: shapes other than [V, 3] and
    [F, 3], a face index outside [0, V), non-finite points, arguments outside their range, Loop together with max_edge;
    GeobiError: more than ``max_rounds`` rounds, or a pass whose output would exceed GEOBI_MAX_NODES rows (nothing of that
    pass is written)."""
    max_edge = check_args(levels, scheme, max_edge, max_rounds)
    pts, fv = meshin.finite_mesh(points, faces, device, 'subdivide')
    dev, V, F = pts.device, pts.shape[0], fv.shape[0]
    loop = scheme == 'loop'
    counts = dict.fromkeys(COUNT_KEYS + ('passes',), 0)
    passes = []
    with torch.cuda.device(dev):
        ids = torch.arange(V, dtype=torch.int32, device=dev)
        face_parent, vertex_parents = torch.arange(F, dtype=torch.int32, device=dev), torch.stack([ids, ids], dim=1)
        while F > 0 and (max_edge is not None or len(passes) < levels):
            ws, c = _plan(fv, pts, loop, max_edge)
            this = dict(zip(COUNT_KEYS, c[:4]))
            if not passes:
                counts.update(this, split=0)
            if max_edge is not None and this['split'] == 0:
                break
            if len(passes) == max_rounds and max_edge is not None:
                raise L.GeobiError('subdivide: edges longer than max_edge = %g are left after max_rounds = %d rounds'
                                   % (max_edge, max_rounds))
            Vn, Fn = c[4], c[5]
            if Vn > MAX_NODES or Fn > MAX_NODES:
                raise L.GeobiError('subdivide: pass %d would give %d vertices and %d faces, beyond GEOBI_MAX_NODES = %d per '
                                   'call' % (len(passes) + 1, Vn, Fn, MAX_NODES))
            passes.append(Pass(fv, pts.shape[0], Vn, Fn, loop, ws, this))
            pts, fv, parent, vertex_parents = _emit(fv, pts, loop, Vn, Fn, ws)
            face_parent = face_parent[parent.long()]
            counts['split'] += this['split']
            F = Fn
    counts['passes'] = len(passes)
    return Refined(pts, fv, face_parent, vertex_parents, counts, passes)


def apply(refined, other_points):
    """Another point array of the INPUT's size [V, 3] (the paired noisy points) -> [V', 3] float32 on the device: the
    same splits and the same masks, pass by pass, over the stored plans.  ``apply(refined, the input points)`` is
    bit-equal to ``refined.points``."""
    dev = refined.points.device
    pts = meshin.paired_points(other_points, refined.passes[0].V if refined.passes else refined.points.shape[0], dev,
                               'a refinement of')
    with torch.cuda.device(dev):
        for p in refined.passes:
            out = torch.empty((p.Vn, 3), dtype=torch.float32, device=dev)
            L.call('geobi_subdiv_points', L.ptr(p.faces), L.ptr(pts), p.faces.shape[0], p.V, int(p.loop), p.Vn, L.ptr(out),
                   L.ptr(p.ws), p.ws.numel(), L.stream())
            pts = out
    return pts
