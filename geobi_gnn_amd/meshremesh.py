"""Isotropic remeshing on the MI355X: make a mesh REGULAR -- edge lengths around one target length
``L`` and valences near 6 -- by the loop of Botsch and Kobbelt.  One iteration splits the edges longer than ``high = 4/3 L``
(``meshsubdiv.subdivide(max_edge=high)``), collapses the edges shorter than ``low = 0.8 L`` in rounds of independent
collapses (the rounds of ``meshdecim`` ranked by length), flips edges towards the target valence in rounds of independent
flips, and relaxes every free vertex once towards the mean of its neighbours inside its tangent plane.

Vertices on a boundary, a complex edge or a feature edge (dihedral angle above ``feature_angle``) are locked: they keep
their points, so boundaries and feature lines only get denser.  By default the relaxed vertices are NOT projected back onto
the input surface, and relaxation is no replayable map: a paired point array cannot be carried along (use ``meshnoise`` on
the result).

``project=True`` adds the fifth step of the loop: after every relaxation the free vertices move to
their closest points on the INPUT surface (``meshproject``), under the guard of the relaxation (``move_to``).  Every output
vertex then carries a (face, barycentric) address on the input, ``Remeshed.source_face`` / ``source_bary``, and ``apply``
evaluates that map on a paired array of the input's vertices: ``noisy/`` can be carried along.

The rules are stated in include/geobi_hip.h (geobi_remesh_lock, geobi_decim_plan_short, geobi_flip_*, geobi_relax,
geobi_move_to); the topology is integer-exact and the result reproducible bit for bit (tests/remesh_model.py,
tests/project_model.py).  No CPU fallback.
"""
import math

import numpy as np
import torch

from . import _lib as L
from . import meshdecim, meshin, meshsubdiv

MAX_NODES = meshin.MAX_NODES
bbox_diagonal = meshin.bbox_diagonal
LOCK_KEYS = ('edges', 'boundary_vertices', 'sharp_edges', 'sharp_vertices')
FLIP_KEYS = ('edges', 'candidates', 'valid', 'flips', 'sweeps_selected')
RELAX_KEYS = ('moved', 'refused', 'reverted', 'turned')
ITERATION_KEYS = ('splits', 'split_passes', 'collapses', 'collapse_rounds', 'flips', 'flip_rounds', 'moved', 'refused',
                  'reverted', 'turned')
PROJECT_KEYS = ('projected', 'project_refused', 'project_reverted', 'project_turned')    # with project=True, beside them


class Remeshed(object):
    """points [V', 3] float32 and faces [F', 3] int32 on the device; low, high: the float32 band; per_iteration: one dict of
    ITERATION_KEYS per iteration (with project=True also PROJECT_KEYS); before, after: the statistics of input and output
    (``mesh_stats``).  With project=True, source_face [V'] int32 and source_bary [V', 3] float32 on the device: the closest
    point of every output vertex on the input surface, as a face of input_faces [F, 3] and the weights of its corners
    (``apply``); else None."""

    def __init__(self, points, faces, low, high, per_iteration, before, after, source_face=None, source_bary=None,
                 input_faces=None, input_V=None):
        self.points, self.faces, self.low, self.high = points, faces, low, high
        self.per_iteration, self.before, self.after = per_iteration, before, after
        self.source_face, self.source_bary, self.input_faces, self.input_V = source_face, source_bary, input_faces, input_V


def _number(name, value, what):
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError('remesh: %s = %r (%s)' % (name, value, what))
    if not math.isfinite(value):
        raise ValueError('remesh: %s = %r (%s)' % (name, value, what))
    return value


def cos2(feature_angle):
    """-> (use_sharp, c2): the fp64 cos^2 of the feature angle in degrees; 180 switches the sharp test off"""
    if feature_angle == 180.0:
        return 0, 0.0
    c = math.cos(math.radians(feature_angle))
    return 1, c * c


def band(target_edge):
    """-> (low, high) as the float32 values the device compares with: float32(0.8 * L) and float32(4.0 * L / 3.0), the
    products and the quotient in fp64"""
    edge = float(target_edge)
    with np.errstate(over='ignore'):
        return float(np.float32(0.8 * edge)), float(np.float32(4.0 * edge / 3.0))


def check_band(low, high, what='remesh'):
    low, high = _number('low', low, 'a positive length'), _number('high', high, 'a length, at least low')
    with np.errstate(over='ignore'):
        low, high = float(np.float32(low)), float(np.float32(high))
    if not (0.0 < low <= high and math.isfinite(high)):
        raise ValueError('%s: low = %r, high = %r (0 < low <= high, finite as float32)' % (what, low, high))
    return low, high


def check_args(target_edge=None, target_edge_diag=None, iterations=5, feature_angle=40.0, relax_lambda=0.5, max_rounds=64):
    """ValueError for what ``remesh`` does not take; -> (target_edge or None, target_edge_diag or None, feature_angle,
    relax_lambda) as Python floats."""
    if not meshin.whole(iterations) or iterations < 0:
        raise ValueError('remesh: iterations = %r (a whole number, not negative)' % (iterations,))
    if not meshin.whole(max_rounds) or max_rounds < 1:
        raise ValueError('remesh: max_rounds = %r (a whole number, at least 1)' % (max_rounds,))
    if target_edge is not None and target_edge_diag is not None:
        raise ValueError('remesh: target_edge and target_edge_diag exclude each other')
    for name, value in (('target_edge', target_edge), ('target_edge_diag', target_edge_diag)):
        if value is not None and not _number(name, value, 'a positive length') > 0.0:
            raise ValueError('remesh: %s = %r (a positive length)' % (name, value))
    feature_angle = _number('feature_angle', feature_angle, 'degrees in [0, 90], or 180 for no feature edges')
    if not (0.0 <= feature_angle <= 90.0 or feature_angle == 180.0):
        raise ValueError('remesh: feature_angle = %r (degrees in [0, 90], or 180 for no feature edges)' % (feature_angle,))
    relax_lambda = _number('relax_lambda', relax_lambda, 'in [0, 1]')
    if not 0.0 <= relax_lambda <= 1.0:
        raise ValueError('remesh: relax_lambda = %r (in [0, 1])' % (relax_lambda,))
    return (None if target_edge is None else float(target_edge), None if target_edge_diag is None else float(target_edge_diag),
            feature_angle, relax_lambda)


def _mesh(points, faces, device, what):
    pts, fv = meshin.finite_mesh(points, faces, device, what)
    if max(pts.shape[0], fv.shape[0]) > MAX_NODES:
        raise ValueError('%s: %d vertices and %d faces, beyond GEOBI_MAX_NODES = %d' % (what, pts.shape[0], fv.shape[0], MAX_NODES))
    return pts, fv


def _workspace(fv, pts):
    return L.workspace(L.size_query('geobi_remesh_ws_bytes', fv.shape[0], pts.shape[0]), fv.device)


def _lock(fv, pts, use_sharp, c2):
    F, V = fv.shape[0], pts.shape[0]
    lock = torch.zeros(V, dtype=torch.int32, device=fv.device)
    counts = torch.zeros(4, dtype=torch.int32, device=fv.device)
    if F == 0:                                      # no edge: no flag (and no pointer to hand over)
        return lock, counts
    ws = _workspace(fv, pts)
    L.call('geobi_remesh_lock', L.ptr(fv), L.ptr(pts), F, V, use_sharp, c2, L.ptr(lock), L.ptr(counts), L.ptr(ws), ws.numel(),
           L.stream())
    return lock, counts


def _plan_short(fv, pts, lock, low, high, stage_ms=None):
    """geobi_decim_plan_short on a device mesh -> (workspace, the eight counts of meshdecim); one wait"""
    F, V = fv.shape[0], pts.shape[0]
    ws = L.workspace(L.size_query('geobi_decim_ws_bytes', F, V), fv.device)
    counts = torch.zeros(8, dtype=torch.int32, device=fv.device)
    L.call('geobi_decim_plan_short', L.ptr(fv), L.ptr(pts), L.ptr(lock), F, V, low, high, L.ptr(counts), stage_ms, L.ptr(ws),
           ws.numel(), L.stream())
    return ws, dict(zip(meshdecim.COUNT_KEYS, L.read_i32(counts, 8)))


def _flip_plan(fv, pts, lock, use_sharp, c2, stage_ms=None):
    F, V = fv.shape[0], pts.shape[0]
    ws = _workspace(fv, pts)
    counts = torch.zeros(5, dtype=torch.int32, device=fv.device)
    L.call('geobi_flip_plan', L.ptr(fv), L.ptr(pts), L.ptr(lock), F, V, use_sharp, c2, L.ptr(counts), stage_ms, L.ptr(ws),
           ws.numel(), L.stream())
    return ws, dict(zip(FLIP_KEYS, L.read_i32(counts, 5)))


def _flip_emit(fv, V, ws):
    out = torch.empty_like(fv)
    L.call('geobi_flip_emit', L.ptr(fv), fv.shape[0], V, L.ptr(out), L.ptr(ws), ws.numel(), L.stream())
    return out


def _move_to(fv, pts, target, lock, stage_ms=None):
    F, V = fv.shape[0], pts.shape[0]
    ws = _workspace(fv, pts)
    out = torch.empty_like(pts)
    counts = torch.zeros(4, dtype=torch.int32, device=fv.device)
    L.call('geobi_move_to', L.ptr(fv), L.ptr(pts), L.ptr(target), L.ptr(lock), F, V, L.ptr(out), L.ptr(counts), stage_ms,
           L.ptr(ws), ws.numel(), L.stream())
    return out, dict(zip(RELAX_KEYS, L.read_i32(counts, 4)))


def _relax(fv, pts, lock, relax_lambda, stage_ms=None):
    F, V = fv.shape[0], pts.shape[0]
    ws = _workspace(fv, pts)
    out = torch.empty_like(pts)
    counts = torch.zeros(4, dtype=torch.int32, device=fv.device)
    L.call('geobi_relax', L.ptr(fv), L.ptr(pts), L.ptr(lock), F, V, relax_lambda, L.ptr(out), L.ptr(counts), stage_ms, L.ptr(ws),
           ws.numel(), L.stream())
    return out, dict(zip(RELAX_KEYS, L.read_i32(counts, 4)))


# ---------------------------------------------------------------------------------------------- the single steps
def lock_flags(points, faces, feature_angle=40.0, device=None):
    """-> (lock [V] int32 on the device, counts): bit 0 for a vertex on a boundary or complex edge, bit 1 for a vertex on
    an edge whose faces meet at more than ``feature_angle`` degrees (180: no such edge)."""
    feature_angle = check_args(feature_angle=feature_angle)[2]
    pts, fv = _mesh(points, faces, device, 'lock_flags')
    with torch.cuda.device(pts.device):
        lock, counts = _lock(fv, pts, *cos2(feature_angle))
        return lock, dict(zip(LOCK_KEYS, L.read_i32(counts, 4)))


def _as_lock(lock, V, dev):
    if lock is None:
        return None
    lock = meshin.to_device(lock, dev, torch.int32)
    if lock.dim() != 1 or lock.shape[0] != V:
        raise ValueError('lock %s for %d vertices' % (tuple(lock.shape), V))
    return lock


def collapse_short(points, faces, low, high, lock=None, device=None):
    """ONE round of short-edge collapses -> (points', faces', counts of ``meshdecim``): the edges shorter than ``low`` whose
    collapse makes no edge longer than ``high``; a vertex with a lock entry other than 0 keeps its point."""
    low, high = check_band(low, high, 'collapse_short')
    pts, fv = _mesh(points, faces, device, 'collapse_short')
    lock = _as_lock(lock, pts.shape[0], pts.device)
    with torch.cuda.device(pts.device):
        if fv.shape[0] == 0:
            return pts, fv, dict(dict.fromkeys(meshdecim.COUNT_KEYS, 0), V=pts.shape[0])
        ws, c = _plan_short(fv, pts, lock, low, high)
        if c['collapses'] == 0 and c['not_included'] == 0:
            return pts, fv, c
        out = meshdecim._emit(fv, pts, c['V'], c['F'], ws)
        return out[0], out[1], c


def flip_edges(points, faces, lock=None, feature_angle=40.0, device=None):
    """ONE round of edge flips towards valence 6 (4 on a boundary) -> (faces', counts).  lock: the flags of ``lock_flags``
    (computed here when None)."""
    feature_angle = check_args(feature_angle=feature_angle)[2]
    pts, fv = _mesh(points, faces, device, 'flip_edges')
    use_sharp, c2 = cos2(feature_angle)
    with torch.cuda.device(pts.device):
        if fv.shape[0] == 0:
            return fv, dict.fromkeys(FLIP_KEYS, 0)
        lock = _as_lock(lock, pts.shape[0], pts.device) if lock is not None else _lock(fv, pts, use_sharp, c2)[0]
        ws, c = _flip_plan(fv, pts, lock, use_sharp, c2)
        return (_flip_emit(fv, pts.shape[0], ws) if c['flips'] else fv), c


def relax(points, faces, lock=None, relax_lambda=0.5, feature_angle=40.0, device=None):
    """ONE tangential relaxation -> (points', counts).  lock: the flags of ``lock_flags`` (computed here when None)."""
    _, _, feature_angle, relax_lambda = check_args(feature_angle=feature_angle, relax_lambda=relax_lambda)
    pts, fv = _mesh(points, faces, device, 'relax')
    with torch.cuda.device(pts.device):
        if fv.shape[0] == 0:
            return pts, dict.fromkeys(RELAX_KEYS, 0)
        lock = _as_lock(lock, pts.shape[0], pts.device) if lock is not None else _lock(fv, pts, *cos2(feature_angle))[0]
        return _relax(fv, pts, lock, relax_lambda)


def move_to(points, faces, target, lock=None, feature_angle=40.0, device=None):
    """ONE guarded move of every free vertex to its row of ``target`` [V, 3] -> (points', counts of ``relax``): the
    protocol of the relaxation -- locked vertices and those of valence < 3 stay, a move that would turn a face at the vertex
    is refused, the moved vertices of a face that turned all the same go back -- with the given positions as proposals.
    lock: the flags of ``lock_flags`` (computed here when None).  A target row that is not finite is refused."""
    feature_angle = check_args(feature_angle=feature_angle)[2]
    pts, fv = _mesh(points, faces, device, 'move_to')
    target = meshin.as_tensor(target)
    if target.dim() != 2 or target.shape[1] != 3 or target.shape[0] != pts.shape[0]:
        raise ValueError('move_to: target %s for %d vertices' % (tuple(target.shape), pts.shape[0]))
    target = meshin.to_device(target, pts.device, torch.float32)
    with torch.cuda.device(pts.device):
        if fv.shape[0] == 0:
            return pts, dict.fromkeys(RELAX_KEYS, 0)
        lock = _as_lock(lock, pts.shape[0], pts.device) if lock is not None else _lock(fv, pts, *cos2(feature_angle))[0]
        return _move_to(fv, pts, target, lock)


def mesh_stats(points, faces, low, high, device=None):
    """The regularity of a mesh: edges, edge_min / edge_mean / edge_max (fp64), inside and share (the edges with low <=
    length <= high), valence_hist (valence 3 .. 11 and 12+), valence_dev (the mean |valence - target| over the vertices
    with an edge, target 4 on a boundary or complex edge, else 6)."""
    pts, fv = _mesh(points, faces, device, 'mesh_stats')
    F, V, dev = fv.shape[0], pts.shape[0], pts.device
    with torch.cuda.device(dev):
        lens = torch.full((3 * F,), -1.0, dtype=torch.float64, device=dev)
        valence = torch.zeros(V, dtype=torch.int32, device=dev)
        if F > 0:
            ws = _workspace(fv, pts)
            L.call('geobi_remesh_stats', L.ptr(fv), L.ptr(pts), F, V, L.ptr(lens), L.ptr(valence), L.ptr(ws), ws.numel(),
                   L.stream())
        lock = _lock(fv, pts, 0, 0.0)[0]
        lens = lens[lens >= 0.0]
        E = int(lens.shape[0])
        valence = valence.long()
        used = valence > 0
        target = torch.where((lock & 1) != 0, 4, 6)
        hist = torch.bincount(valence.clamp(max=12), minlength=13)[3:].tolist()
        inside = int(((lens >= low) & (lens <= high)).sum()) if E else 0
        return {'edges': E, 'edge_min': float(lens.min()) if E else 0.0, 'edge_mean': float(lens.mean()) if E else 0.0,
                'edge_max': float(lens.max()) if E else 0.0, 'inside': inside, 'share': inside / E if E else 0.0,
                'valence_hist': [int(x) for x in hist],
                'valence_dev': float((valence - target).abs()[used].double().mean()) if bool(used.any()) else 0.0}


# ---------------------------------------------------------------------------------------------- the whole call
def remesh(points, faces, target_edge=None, target_edge_diag=None, iterations=5, feature_angle=40.0, relax_lambda=0.5,
           max_rounds=64, device=None, project=False, index=None):
    """(points [V, 3], faces [F, 3]) -> Remeshed.  The target edge length L is ``target_edge``, or ``target_edge_diag`` times
    the diagonal of the bounding box, or by default the mean edge length of the input (``meshnoise.MeshGeometry``).  Every
    iteration runs: splits of the edges above high = 4/3 L to exhaustion, rounds of short-edge collapses (below low = 0.8
    L) until a round collapses nothing, rounds of flips until a round flips nothing, one relaxation.  project=True: every
    iteration ends with the closest points of the relaxed vertices on the INPUT mesh (``meshproject``) and one ``move_to``
    from the relaxed positions to them under the lock flags the relaxation used (counts: PROJECT_KEYS); after the last
    iteration the closest points of ALL output vertices on the input, locked ones included, fill ``source_face`` /
    ``source_bary`` -- a map only, no point moves (``iterations=0``: the one-hot map of the input onto itself).  Without
    project the launches and the dicts are what they were.  index (with project): None searches all pairs; 'grid' builds
    ONE meshgrid.TriangleGrid over the input surface for all these searches, one built over it before is used as it is;
    the output is the same bits.  ValueError: project for an input without faces, shapes
    other than [V, 3] and [F, 3], a face index outside [0, V), non-finite points, arguments outside their range;
    GeobiError: ``max_rounds`` rounds did not end one of the three inner loops."""
    target_edge, target_edge_diag, feature_angle, relax_lambda = check_args(target_edge, target_edge_diag, iterations,
                                                                            feature_angle, relax_lambda, max_rounds)
    if index is not None:
        from . import meshgrid
        index = meshgrid.check_index(index)
        if not project:
            raise ValueError('remesh: index = %r serves the searches of project = True' % (index,))
    pts, fv = _mesh(points, faces, device, 'remesh')
    dev = pts.device
    if project and fv.shape[0] == 0:
        raise ValueError('remesh: project = True needs a surface to project onto, the input has no faces')
    if project:
        from . import meshproject
        in_pts, in_fv = pts, fv
        if index is not None:
            with torch.cuda.device(dev):
                index = meshgrid.triangle_grid(index, in_pts, in_fv)     # one grid over the input for all its searches
    use_sharp, c2 = cos2(feature_angle)
    with torch.cuda.device(dev):
        if target_edge is None and target_edge_diag is not None:
            target_edge = target_edge_diag * bbox_diagonal(pts)
        elif target_edge is None:
            from . import meshnoise
            target_edge = meshnoise.MeshGeometry(pts, fv, dev).mean_edge if fv.shape[0] > 0 else 1.0
        low, high = band(target_edge)
        if not (0.0 < low <= high and math.isfinite(high)):
            raise ValueError('remesh: the target edge length %r gives the band [%r, %r]' % (target_edge, low, high))
        before = mesh_stats(pts, fv, low, high, dev)
        per_iteration = []
        for _ in range(iterations):
            c = dict.fromkeys(ITERATION_KEYS, 0)
            refined = meshsubdiv.subdivide(pts, fv, max_edge=high, max_rounds=max_rounds, device=dev)
            pts, fv = refined.points, refined.faces
            c['splits'], c['split_passes'] = refined.counts['split'], refined.counts['passes']
            lock = None                             # recomputed whenever the mesh has changed
            while fv.shape[0] > 0:
                lock = _lock(fv, pts, use_sharp, c2)[0]
                ws, r = _plan_short(fv, pts, lock, low, high)
                if r['collapses'] == 0 and r['not_included'] == 0:
                    break
                if c['collapse_rounds'] == max_rounds:
                    raise L.GeobiError('remesh: edges below low = %g still collapse after max_rounds = %d rounds'
                                       % (low, max_rounds))
                pts, fv = meshdecim._emit(fv, pts, r['V'], r['F'], ws)[:2]
                lock = None
                c['collapse_rounds'] += 1
                c['collapses'] += r['collapses']
                if r['collapses'] == 0:
                    break
            while fv.shape[0] > 0:
                lock = lock if lock is not None else _lock(fv, pts, use_sharp, c2)[0]
                ws, r = _flip_plan(fv, pts, lock, use_sharp, c2)
                if r['flips'] == 0:
                    break
                if c['flip_rounds'] == max_rounds:
                    raise L.GeobiError('remesh: edges still flip after max_rounds = %d rounds' % max_rounds)
                fv, lock = _flip_emit(fv, pts.shape[0], ws), None
                c['flip_rounds'] += 1
                c['flips'] += r['flips']
            if fv.shape[0] > 0:
                lock = lock if lock is not None else _lock(fv, pts, use_sharp, c2)[0]
                pts, r = _relax(fv, pts, lock, relax_lambda)
                c.update(r)
            if project:
                c.update(dict.fromkeys(PROJECT_KEYS, 0))
                if fv.shape[0] > 0:
                    pts, r = _move_to(fv, pts, meshproject._closest(pts, in_pts, in_fv, index).points, lock)
                    c.update(zip(PROJECT_KEYS, (r[k] for k in RELAX_KEYS)))
            per_iteration.append(c)
        after = mesh_stats(pts, fv, low, high, dev)
        source = meshproject._closest(pts, in_pts, in_fv, index) if project else None
    if project:
        return Remeshed(pts, fv, np.float32(low), np.float32(high), per_iteration, before, after, source.face, source.bary,
                        in_fv, in_pts.shape[0])
    return Remeshed(pts, fv, np.float32(low), np.float32(high), per_iteration, before, after)


def apply(remeshed, other_points):
    """The output vertices of a ``remesh(project=True)`` on a paired array of the INPUT's vertices (other_points [V, 3],
    the noisy copy of the input): ``ops.bary_points(other_points, input faces, source_face, source_bary)`` -> float32
    [V', 3] on the device.  ValueError for a result without the map (project=False) or another V."""
    if remeshed.source_face is None:
        raise ValueError('apply: this result carries no map onto its input (remesh(project=True) makes one)')
    from . import ops
    other = meshin.paired_points(other_points, remeshed.input_V, remeshed.source_face.device, 'a remeshing of')
    with torch.cuda.device(other.device):
        return ops.bary_points(other, remeshed.input_faces, remeshed.source_face, remeshed.source_bary)
