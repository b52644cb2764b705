"""Mesh topology on the MI355X: make the winding consistent, find the connected parts, report the
edges -- the stage between ``meshclean``'s weld / bad faces and the graphs of ``meshprep``.

A face is *included* when its state is 1 (all, without a state) and its three corners differ; the others have no links
and get label -1.  Faces are corners already taken through ``canon`` (``meshclean``).

* **orientation**: two faces are linked when they are the only two claimants of an undirected edge and their opposite
  corners differ (two copies of one triangle stay unlinked); the link is *odd* when both walk the edge in the same
  direction.  ``label`` = the lowest face of the component, ``flip`` = the parity of odd links on a path from it; the
  lowest face of a component keeps its winding and decides for the rest.  A component with a link that contradicts the
  parities (a Moebius band) is *non-orientable* and flips nothing
* **components**: faces that share an EDGE, whatever its direction and however many claimants it has; two fans that meet
  in one vertex only are two components.  ``min_component = m``: the faces of a component of fewer than m faces get state 4
* **report**: edges, boundary edges (one claimant), complex edges (three and more), inconsistent edges (two claimants
  that walk it the same way), and the counts of both kinds of component

Everything is integer-exact (geobi_topo_* in csrc/topo.hip); the number of rounds is a function of the input.  No CPU
fallback.
"""
import ctypes

import torch

from . import _lib as L
from . import meshclean, meshin


class Oriented(object):
    """faces [F, 3], flip [F], label [F] int32 on the device; counts: components, nonorientable, flipped, rounds."""

    def __init__(self, faces, flip, label, counts):
        self.faces, self.flip, self.label, self.counts = faces, flip, label, counts


class Components(object):
    """label [F], state [F] int32 on the device; counts: components, components_dropped, faces_dropped, rounds."""

    def __init__(self, label, state, counts):
        self.label, self.state, self.counts = label, state, counts


def _check_rounds(what, max_rounds):
    if int(max_rounds) < 1:
        raise ValueError('%s: max_rounds = %r (at least 1)' % (what, max_rounds))


def _faces_in(what, faces, V, state, device):
    """the caller's table, range-checked as it came in, and its state -> int32 on the device"""
    fv = meshin.as_tensor(faces).reshape(-1, 3)
    dev = meshin.default_device(device, fv)
    meshin.check_faces(fv, V, what='%s: faces' % what, error=ValueError)
    fv = meshin.to_device(fv, dev, torch.int32)
    if state is not None:
        state = meshin.to_device(meshin.as_tensor(state).reshape(-1), dev, torch.int32)
        if state.shape[0] != fv.shape[0]:
            raise ValueError('%s: %d states for %d faces' % (what, state.shape[0], fv.shape[0]))
    return dev, fv, state


def orient_device(fv, V, state=None, max_rounds=256, stage_ms=None):
    """geobi_topo_orient on a range-checked device table: -> (faces [max(F, 1), 3], flip, label [max(F, 1)], device counts
    [3] = components, nonorientable, flipped; rounds).  Waits for the device once per batch of rounds.  stage_ms: a
    (ctypes.c_float * 3)() that takes the milliseconds of the three stages (measurement; the call then waits for its end)."""
    dev, F = fv.device, fv.shape[0]
    f_out = meshclean._empty(F, 3, torch.int32, dev)
    flip, label = meshclean._empty(F, 0, torch.int32, dev), meshclean._empty(F, 0, torch.int32, dev)
    counts = torch.zeros(3, dtype=torch.int32, device=dev)
    rounds = (ctypes.c_int32 * 1)()
    ws = L.workspace(L.size_query('geobi_topo_ws_bytes', F, 0), dev)
    L.call('geobi_topo_orient', L.ptr(fv if F else f_out), L.ptr(state), F, int(V), int(max_rounds), L.ptr(f_out),
           L.ptr(flip), L.ptr(label), L.ptr(counts), rounds, stage_ms, L.ptr(ws), ws.numel(), L.stream())
    return f_out, flip, label, counts, int(rounds[0])


def components_device(fv, V, state=None, min_component=0, max_rounds=256, stage_ms=None):
    """geobi_topo_components on a range-checked device table: -> (label, state [max(F, 1)], device counts [3] = components,
    components_dropped, faces_dropped; rounds)."""
    dev, F = fv.device, fv.shape[0]
    label, st_out = meshclean._empty(F, 0, torch.int32, dev), meshclean._empty(F, 0, torch.int32, dev)
    counts = torch.zeros(3, dtype=torch.int32, device=dev)
    rounds = (ctypes.c_int32 * 1)()
    ws = L.workspace(L.size_query('geobi_topo_ws_bytes', F, 0), dev)
    L.call('geobi_topo_components', L.ptr(fv if F else label), L.ptr(state), F, int(V), int(min_component), int(max_rounds),
           L.ptr(label), L.ptr(st_out), L.ptr(counts), rounds, stage_ms, L.ptr(ws), ws.numel(), L.stream())
    return label, st_out, counts, int(rounds[0])


def orient_faces(faces, V, state=None, max_rounds=256, device=None):
    """faces [F, 3] of a mesh of V vertices (already through canon) -> Oriented.  ValueError: a face index outside [0, V),
    max_rounds < 1; GeobiError: more than ``max_rounds`` rounds."""
    _check_rounds('orient_faces', max_rounds)
    dev, fv, state = _faces_in('orient_faces', faces, V, state, device)
    F = fv.shape[0]
    with torch.cuda.device(dev):
        f_out, flip, label, counts, rounds = orient_device(fv, V, state, max_rounds)
        components, nonorientable, flipped = L.read_i32(counts)
    return Oriented(f_out[:F], flip[:F], label[:F], {'components': components, 'nonorientable': nonorientable,
                                                     'flipped': flipped, 'rounds': rounds})


def face_components(faces, V, state=None, min_component=0, max_rounds=256, device=None):
    """faces [F, 3] of a mesh of V vertices -> Components; with ``min_component = m > 0`` the faces of every component of
    fewer than m faces get state 4 (which the compaction of ``meshclean`` drops).  Errors as ``orient_faces``."""
    _check_rounds('face_components', max_rounds)
    if int(min_component) < 0:
        raise ValueError('face_components: min_component = %r (0 or more)' % (min_component,))
    dev, fv, state = _faces_in('face_components', faces, V, state, device)
    F = fv.shape[0]
    with torch.cuda.device(dev):
        label, st_out, counts, rounds = components_device(fv, V, state, min_component, max_rounds)
        components, components_dropped, faces_dropped = L.read_i32(counts)
    return Components(label[:F], st_out[:F], {'components': components, 'components_dropped': components_dropped,
                                              'faces_dropped': faces_dropped, 'rounds': rounds})


def mesh_report(points, faces, weld_tol=0.0, max_rounds=256, device=None, intersections=False, solid=False):
    """(points [V, 3], faces [F, 3]) -> dict: vertices_used, faces, degenerate; edges, boundary_edges, complex_edges,
    inconsistent_edges; components, orient_components, nonorientable, would_flip; euler = vertices_used - edges + faces;
    closed = no boundary and no complex edge.  Computed after the weld (``weld_tol`` as in ``clean_mesh``), degenerate
    faces excluded and no face dropped for its half-edges.  ``intersections``: also intersecting_pairs, intersecting_faces
    and folded_pairs (pairs that share an edge and lie flat on each other), from ``meshselfx``'s all-pairs search on the
    same welded table.  ``solid``: also volume (the sum of volume6 / 6 over the closed components as the file
    winds them), closed_components and inward_components (the components ``meshwind.orient_outward`` would leave reversed),
    from ``meshwind`` on the same welded table."""
    _check_rounds('mesh_report', max_rounds)
    dev = meshin.default_device(device)
    meshclean.check_weld_tol('mesh_report', weld_tol)
    pts, fv = meshin.finite_mesh(meshin.as_tensor(points).reshape(-1, 3), meshin.as_tensor(faces).reshape(-1, 3), dev,
                                 'mesh_report')
    V, F = pts.shape[0], fv.shape[0]
    with torch.cuda.device(dev):
        canon, wcounts = meshclean.weld(pts, weld_tol)
        _, bad = L.read_i32(wcounts)
        if bad:
            raise L.GeobiError('mesh_report: a coordinate divided by weld_tol = %g is outside the int32 range' % weld_tol)
        fc, state, _ = meshclean.resolve_faces(fv, canon, V, manifold=False)
        counts = torch.zeros(16, dtype=torch.int32, device=dev)
        rounds = (ctypes.c_int32 * 2)()
        ws = L.workspace(L.size_query('geobi_topo_ws_bytes', F, V), dev)
        L.call('geobi_topo_report', L.ptr(fc), L.ptr(state), F, V, int(max_rounds), L.ptr(counts), rounds, L.ptr(ws),
               ws.numel(), L.stream())
        c = L.read_i32(counts)
        if intersections:
            from . import meshselfx
            x = dict(zip(meshselfx.COUNT_KEYS, L.read_i64(meshselfx.search_device(pts, fc[:F], state[:F] if F else None)[2])))
        if solid:
            from . import meshwind
            s = {'volume': 0.0, 'closed_components': 0, 'inward_components': 0}
            if F:
                _, _, label, wc = meshwind.outward_device(pts, fc[:F].contiguous(), V, state[:F].contiguous(), max_rounds)
                # the file's own winding: the volume of a component the file winds inconsistently is not counted
                v6, is_closed, consistent = meshwind.part_solids_device(pts, fc[:F].contiguous(), label, state[:F].contiguous())
                whole = (is_closed[:F] != 0) & (consistent[:F] != 0) & (label == torch.arange(F, dtype=torch.int32, device=dev))
                s = {'volume': float((v6[:F] * whole).sum() / 6.0), 'closed_components': wc['closed_components'],
                     'inward_components': wc['turned']}
    report = {'vertices_used': c[4], 'faces': c[5], 'degenerate': c[6], 'edges': c[0], 'boundary_edges': c[1],
            'complex_edges': c[2], 'inconsistent_edges': c[3], 'components': c[7], 'orient_components': c[8],
            'nonorientable': c[9], 'would_flip': c[10], 'euler': c[4] - c[0] + c[5], 'closed': c[1] == 0 and c[2] == 0}
    if intersections:
        report.update(intersecting_pairs=x['pairs'], intersecting_faces=x['faces_hit'], folded_pairs=x['pairs_k2'])
    if solid:
        report.update(s)
    return report
