"""Triangle-mesh simplification on the MI355X: make a mesh coarser by rounds of independent quadric
edge collapses, and keep a paired point array (the noisy copy of an original) in row-by-row correspondence.

A round collapses a set of edges that cannot see each other: every edge shared by exactly two faces gets the cheapest of
three placements (an end or the midpoint) under the sum of its ends' plane quadrics, is tested on the round's input (link
condition, valence, no flipped face), and the valid ones are ranked by (cost, hash, id); sweeps of a local-minimum rule
select edges whose ends lie outside each other's closed rings.  Vertices on a boundary or a complex edge keep their points.

The rules -- every rounding of a cost, the ranking, the selection, the order of the surviving rows -- are stated in
include/geobi_hip.h (geobi_decim_*); the topology is integer-exact and the result reproducible bit for bit
(tests/decim_model.py).  No CPU fallback.
"""
import math

import numpy as np
import torch

from . import _lib as L
from . import meshin

COUNT_KEYS = ('edges', 'locked', 'valid', 'collapses', 'V', 'F', 'not_included', 'sweeps_selected')


class Pass(object):
    """One round as ``apply`` needs it: the sizes V -> Vn, vertex_parents [Vn, 2] int32 and place [Vn] int8 on the device.
    counts: the eight counts of the round (COUNT_KEYS)."""

    def __init__(self, V, Vn, vertex_parents, place, counts):
        self.V, self.Vn, self.vertex_parents, self.place, self.counts = V, Vn, vertex_parents, place, counts


class Decimated(object):
    """points [V', 3] float32, faces [F', 3], face_map [F'] (the INPUT's face of every face), vertex_map [V] (input row ->
    output row) int32, both composed over the rounds, all on the device; counts: edges, locked, not_included of the input,
    collapses over all rounds (= V - V'), rounds, reached (the included face count is at or below the target; True when
    max_cost alone ends the rounds); passes: the Pass records."""

    def __init__(self, points, faces, face_map, vertex_map, counts, passes):
        self.points, self.faces, self.face_map, self.vertex_map = points, faces, face_map, vertex_map
        self.counts, self.passes = counts, passes


def check_args(target_faces=None, ratio=None, max_cost=None, max_rounds=256):
    """ValueError for what ``decimate`` does not take; -> (target_faces or None, ratio or None, max_cost as the float32 the
    device compares with or None)."""
    if not meshin.whole(max_rounds) or max_rounds < 1:
        raise ValueError('decimate: max_rounds = %r (a whole number, at least 1)' % (max_rounds,))
    if target_faces is not None and ratio is not None:
        raise ValueError('decimate: target_faces and ratio exclude each other')
    if target_faces is None and ratio is None and max_cost is None:
        raise ValueError('decimate: one of target_faces, ratio or max_cost must say when to stop')
    if target_faces is not None and (not meshin.whole(target_faces) or target_faces < 0):
        raise ValueError('decimate: target_faces = %r (a whole number, not negative)' % (target_faces,))
    if ratio is not None:
        try:
            ratio = float(ratio)
        except (TypeError, ValueError):
            raise ValueError('decimate: ratio = %r (above 0, below 1)' % (ratio,))
        if not 0.0 < ratio < 1.0:
            raise ValueError('decimate: ratio = %r (above 0, below 1)' % (ratio,))
    if max_cost is not None:
        try:
            with np.errstate(over='ignore'):
                max_cost = float(np.float32(max_cost))
        except (TypeError, ValueError):
            raise ValueError('decimate: max_cost = %r (a cost, not negative)' % (max_cost,))
        if not (max_cost >= 0.0 and math.isfinite(max_cost)):
            raise ValueError('decimate: max_cost = %r (not negative and finite as a float32)' % (max_cost,))
    return (int(target_faces) if target_faces is not None else None), ratio, max_cost


def stop_target(F, target_faces=None, ratio=None):
    """the face count the rounds run to: target_faces, or floor(ratio * F) of the F rows of the face table"""
    if target_faces is not None:
        return int(target_faces)
    return int(math.floor(ratio * F)) if ratio is not None else None


def _plan(fv, pts, max_cost, target, stage_ms=None):
    """geobi_decim_plan on a device mesh -> (workspace, the eight counts); one wait"""
    F, V = fv.shape[0], pts.shape[0]
    ws = L.workspace(L.size_query('geobi_decim_ws_bytes', F, V), fv.device)
    counts = torch.zeros(8, dtype=torch.int32, device=fv.device)
    L.call('geobi_decim_plan', L.ptr(fv), L.ptr(pts), F, V, int(max_cost is not None), float(max_cost or 0.0),
           -1 if target is None else int(target), L.ptr(counts), stage_ms, L.ptr(ws), ws.numel(), L.stream())
    return ws, dict(zip(COUNT_KEYS, L.read_i32(counts, 8)))


def _emit(fv, pts, Vn, Fn, ws):
    dev, F, V = fv.device, fv.shape[0], pts.shape[0]
    points = torch.empty((Vn, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((Fn, 3), dtype=torch.int32, device=dev)
    face_map = torch.empty(Fn, dtype=torch.int32, device=dev)
    vertex_map = torch.empty(V, dtype=torch.int32, device=dev)
    vertex_parents = torch.empty((Vn, 2), dtype=torch.int32, device=dev)
    place = torch.empty(Vn, dtype=torch.int8, device=dev)
    L.call('geobi_decim_emit', L.ptr(fv), L.ptr(pts), F, V, Vn, Fn, L.ptr(points), L.ptr(faces), L.ptr(face_map),
           L.ptr(vertex_map), L.ptr(vertex_parents), L.ptr(place), L.ptr(ws), ws.numel(), L.stream())
    return points, faces, face_map, vertex_map, vertex_parents, place


def decimate(points, faces, target_faces=None, ratio=None, max_cost=None, max_rounds=256, device=None):
    """(points [V, 3], faces [F, 3]) -> Decimated.  Rounds run until the count of included faces is at or below
    ``target_faces`` (or ``ratio`` times F; the result lands on the target or one below it), or, with ``max_cost`` alone,
    until no edge costs that little; with both, no edge above ``max_cost`` collapses on the way.  A round that collapses
    nothing ends the rounds as well: ``counts['reached']`` says which happened.  ValueError: shapes other than [V, 3] and
    [F, 3], a face index outside [0, V), non-finite points, arguments outside their range, not exactly one of target_faces /
    ratio / max_cost-alone; GeobiError: ``max_rounds`` rounds were not enough."""
    target_faces, ratio, max_cost = check_args(target_faces, ratio, max_cost, max_rounds)
    pts, fv = meshin.finite_mesh(points, faces, device, 'decimate')
    dev, V, F = pts.device, pts.shape[0], fv.shape[0]
    target = stop_target(F, target_faces, ratio)
    passes, first, included = [], None, F
    with torch.cuda.device(dev):
        face_map = torch.arange(F, dtype=torch.int32, device=dev)
        vertex_map = torch.arange(V, dtype=torch.int32, device=dev)
        while F > 0:
            ws, c = _plan(fv, pts, max_cost, target)
            first = first or c
            included = F - c['not_included']
            if c['collapses'] == 0 and c['not_included'] == 0:
                break
            if len(passes) == max_rounds:
                raise L.GeobiError('decimate: %d included faces are left after max_rounds = %d rounds%s'
                                   % (included, max_rounds, '' if target is None else ', above the target of %d' % target))
            pts, fv, fmap, vmap, vertex_parents, place = _emit(fv, pts, c['V'], c['F'], ws)
            passes.append(Pass(vmap.shape[0], c['V'], vertex_parents, place, c))
            face_map, vertex_map = face_map[fmap.long()], vmap[vertex_map.long()]
            F = included = c['F']
            if c['collapses'] == 0 or (target is not None and F <= target):
                break
    first = first or dict.fromkeys(COUNT_KEYS, 0)
    counts = {'edges': first['edges'], 'locked': first['locked'], 'not_included': first['not_included'],
              'collapses': sum(p.counts['collapses'] for p in passes), 'rounds': len(passes),
              'reached': bool(target is None or included <= target)}
    return Decimated(pts, fv, face_map, vertex_map, counts, passes)


def apply(decimated, other_points):
    """Another point array of the INPUT's size [V, 3] (the paired noisy points) -> [V', 3] float32 on the device: the
    same merges and the same placements, round by round.  ``apply(decimated, the input points)`` is bit-equal to
    ``decimated.points``."""
    dev = decimated.points.device
    pts = meshin.paired_points(other_points, decimated.passes[0].V if decimated.passes else decimated.points.shape[0], dev,
                               'a decimation of')
    with torch.cuda.device(dev):
        for p in decimated.passes:
            out = torch.empty((p.Vn, 3), dtype=torch.float32, device=dev)
            L.call('geobi_decim_points', L.ptr(pts), p.V, p.Vn, L.ptr(p.vertex_parents), L.ptr(p.place), L.ptr(out),
                   L.stream())
            pts = out
    return pts
