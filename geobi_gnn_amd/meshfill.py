"""Hole filling on the MI355X: find the boundary loops of a triangle mesh, close every loop (or
every loop of at most ``max_hole_edges`` edges) with a fan around one new vertex at the mean of its rim, and keep a paired
point array (the noisy copy of an original) in row-by-row correspondence.

The rules -- which slots are boundary slots, which vertices are simple, how the loops are numbered and ranked, which row
every new face gets and the order of the sum behind every new position -- are stated in include/geobi_hip.h
(geobi_fill_*); the topology is integer-exact and the positions reproducible bit for bit (tests/fill_model.py).  A rim that
runs through a blocked vertex (a bow-tie, faces wound against each other) is a chain and stays open: ``clean --orient``
first.  No CPU fallback.
"""
import torch

from . import _lib as L
from . import meshin

MAX_NODES = meshin.MAX_NODES
COUNT_KEYS = ('boundary_edges', 'blocked_vertices', 'chain_edges', 'loops', 'longest_loop', 'filled_loops', 'skipped_loops',
              'new_faces')


class Loops(object):
    """Per slot 3f + k: loop [3F] (the loop number, -1 for a slot that is no boundary slot, -2 for a chain slot) and rank
    [3F] (the steps from the loop's leader, -1 off the loops); per loop: length [L], leader [L] (its lowest slot), loop_ptr
    [L + 1] and loop_vertices (from(s) of the slots of loop i in rank order at loop_ptr[i] .. loop_ptr[i + 1]); int32 on the
    device.  counts: boundary_edges, blocked_vertices, chain_edges, loops, longest_loop."""

    def __init__(self, loop, rank, length, leader, loop_ptr, loop_vertices, counts):
        self.loop, self.rank, self.length, self.leader = loop, rank, length, leader
        self.loop_ptr, self.loop_vertices, self.counts = loop_ptr, loop_vertices, counts


class Filled(object):
    """points [V', 3] float32, faces [F', 3], new_vertex_loop [V' - V], new_face_loop [F' - F] (the loop number of every
    new row) int32, on the device; loops: the Loops of the input; counts: COUNT_KEYS; V, F: the input's sizes; ws: the
    workspace that holds the plan (``apply`` replays it)."""

    def __init__(self, points, faces, new_vertex_loop, new_face_loop, loops, counts, V, F, ws):
        self.points, self.faces, self.new_vertex_loop, self.new_face_loop = points, faces, new_vertex_loop, new_face_loop
        self.loops, self.counts, self.V, self.F, self.ws = loops, counts, V, F, ws


def check_args(max_hole_edges=0):
    """ValueError for what ``fill_holes`` does not take"""
    if not meshin.whole(max_hole_edges) or max_hole_edges < 0:
        raise ValueError('fill: max_hole_edges = %r (a whole number; 0 fills every loop)' % (max_hole_edges,))
    return min(int(max_hole_edges), 2 ** 31 - 1)      # the C int of the entry point; no loop is that long


def _plan(fv, V, max_hole_edges, stage_ms=None):
    """geobi_fill_plan on a device face table -> (workspace, Loops, the 10 counts of the header); one wait"""
    dev, F = fv.device, fv.shape[0]
    ws = L.workspace(L.size_query('geobi_fill_ws_bytes', F, V), dev)
    loop = torch.empty(3 * F, dtype=torch.int32, device=dev)
    rank = torch.empty(3 * F, dtype=torch.int32, device=dev)
    leader = torch.empty(F, dtype=torch.int32, device=dev)
    length = torch.empty(F, dtype=torch.int32, device=dev)
    counts = torch.zeros(16, dtype=torch.int32, device=dev)
    L.call('geobi_fill_plan', L.ptr(fv), F, V, max_hole_edges, L.ptr(loop), L.ptr(rank), L.ptr(leader), L.ptr(length),
           L.ptr(counts), stage_ms, L.ptr(ws), ws.numel(), L.stream())
    c = L.read_i32(counts, 10)
    n_loops = c[3]
    leader, length = leader[:n_loops].contiguous(), length[:n_loops].contiguous()
    # the rim vertices in rank order, composed from the per-slot arrays
    loop_ptr = torch.zeros(n_loops + 1, dtype=torch.int32, device=dev)
    loop_ptr[1:] = torch.cumsum(length, 0)
    slots = torch.nonzero(loop >= 0).reshape(-1)
    where = loop_ptr[loop[slots].long()].long() + rank[slots].long()
    frm = fv.reshape(-1)[3 * (slots // 3) + (slots % 3 + 1) % 3]
    loop_vertices = torch.empty(slots.shape[0], dtype=torch.int32, device=dev)
    loop_vertices[where] = frm
    return ws, Loops(loop, rank, length, leader, loop_ptr, loop_vertices, dict(zip(COUNT_KEYS[:5], c[:5]))), c


def _emit(fv, pts, Vn, Fn, ws):
    dev, F, V = fv.device, fv.shape[0], pts.shape[0]
    points = torch.empty((Vn, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((Fn, 3), dtype=torch.int32, device=dev)
    new_vertex_loop = torch.empty(Vn - V, dtype=torch.int32, device=dev)
    new_face_loop = torch.empty(Fn - F, dtype=torch.int32, device=dev)
    L.call('geobi_fill_emit', L.ptr(fv), L.ptr(pts), F, V, Vn, Fn, L.ptr(faces), L.ptr(points), L.ptr(new_vertex_loop),
           L.ptr(new_face_loop), L.ptr(ws), ws.numel(), L.stream())
    return points, faces, new_vertex_loop, new_face_loop


def boundary_loops(faces, V, device=None):
    """faces [F, 3] of a mesh of V vertices -> Loops.  ValueError: a shape other than [F, 3], V outside [0,
    GEOBI_MAX_NODES], a face index outside [0, V)."""
    if not meshin.whole(V) or not 0 <= V <= MAX_NODES:
        raise ValueError('boundary_loops: V = %r (a vertex count, at most GEOBI_MAX_NODES = %d)' % (V, MAX_NODES))
    fv = meshin.as_tensor(faces)
    if fv.dim() != 2 or fv.shape[1] != 3:
        raise ValueError('faces [F,3] expected, got %s' % (tuple(fv.shape),))
    dev = meshin.default_device(device, fv)
    meshin.check_faces(fv, V, 'boundary_loops: faces', ValueError)
    fv = meshin.to_device(fv, dev, torch.int32)
    with torch.cuda.device(dev):
        return _plan(fv, int(V), 0)[1]


def fill_holes(points, faces, max_hole_edges=0, device=None):
    """(points [V, 3], faces [F, 3]) -> Filled: every boundary loop of at most ``max_hole_edges`` edges (0: every loop)
    closed by a fan around a new vertex.  ValueError: shapes other than [V, 3] and [F, 3], a face index outside [0, V),
    non-finite points, a max_hole_edges that is no whole number >= 0; GeobiError: an output beyond GEOBI_MAX_NODES rows
    (nothing is written)."""
    max_hole_edges = check_args(max_hole_edges)
    pts, fv = meshin.finite_mesh(points, faces, device, 'fill')
    dev, V, F = pts.device, pts.shape[0], fv.shape[0]
    with torch.cuda.device(dev):
        ws, loops, c = _plan(fv, V, max_hole_edges)
        Vn, Fn = c[8], c[9]
        if Vn > MAX_NODES or Fn > MAX_NODES:
            raise L.GeobiError('fill: the fill would give %d vertices and %d faces, beyond GEOBI_MAX_NODES = %d per call'
                               % (Vn, Fn, MAX_NODES))
        out_points, out_faces, new_vertex_loop, new_face_loop = _emit(fv, pts, Vn, Fn, ws)
    return Filled(out_points, out_faces, new_vertex_loop, new_face_loop, loops, dict(zip(COUNT_KEYS, c[:8])), V, F, ws)


def apply(filled, other_points):
    """Another point array of the INPUT's size [V, 3] (the paired noisy points) -> [V', 3] float32 on the device: the old
    rows as they are, every new vertex at the mean of ITS rim in that array, over the stored plan.  ``apply(filled, the
    input points)`` is bit-equal to ``filled.points``."""
    dev = filled.points.device
    pts = meshin.paired_points(other_points, filled.V, dev, 'a fill of')
    Vn = filled.points.shape[0]
    out = torch.empty((Vn, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.call('geobi_fill_points', L.ptr(pts), filled.F, filled.V, Vn, L.ptr(out), L.ptr(filled.ws), filled.ws.numel(),
               L.stream())
    return out
