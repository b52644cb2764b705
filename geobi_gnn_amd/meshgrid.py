"""A uniform grid in front of the nearest-point and point-to-surface searches on the MI355X (DESIGN.md section 4u,
csrc/grid.hip).

``PointGrid`` and ``TriangleGrid`` build once over a target set and answer ``nearest(queries)`` with what
``mesheval.nearest_point`` / ``mesheval.point_to_mesh`` answer on the same tensors BIT FOR BIT: the same float32 distance
and the lowest index among equally near targets.  A pair's squared distance is the all-pairs text (csrc/dist_pairs.h); the
walk over the cells stops only when everything it has not visited is strictly farther than its best by the margin derived in
4u.  A query that exhausts its shell budget (``max_rings``) is finished by the all-pairs call itself, so the budget changes the
time and never a bit.  tests/grid_model.py states the invariants of the tables in plain numpy.  No CPU fallback.
"""
import ctypes
import struct

import torch

from . import _lib as L
from . import meshin

INDEX_WORDS = ('grid',)


def check_index(index, what='index'):
    """The ``index=`` keyword of the searches' callers: None (the all-pairs search, the default), 'grid', or a grid built
    before -> the value.  ValueError for anything else; needs no device."""
    if index is None or isinstance(index, (PointGrid, TriangleGrid)):
        return index
    if isinstance(index, str) and index in INDEX_WORDS:
        return index
    raise ValueError("%s = %r (None: all pairs; 'grid'; or a PointGrid / TriangleGrid built before)" % (what, index))


def check_index_word(index, what):
    """For a caller with more than one target: None or 'grid' only (a grid built before serves ONE target)"""
    if isinstance(check_index(index, what + ': index'), (PointGrid, TriangleGrid)):
        raise ValueError("%s: this call searches more than one target, a grid built before serves one (pass 'grid')" % what)
    return index


def _floats(words):
    return struct.unpack('3f', struct.pack('3i', *words))


class _Grid(object):
    """What the two grids share: the descriptor of the plan, the tables, the search behind ``nearest``"""

    def _take(self, desc):
        self.desc = desc
        d = list(desc)
        self.dims = tuple(d[0:3])
        self.lo, self.hi, self.cell = _floats(d[3:6]), _floats(d[6:9]), _floats(d[9:12])
        self.magnitude = struct.unpack('f', struct.pack('i', d[12]))[0]
        self.entries, self.rounds, self.finite = d[13], d[14], d[15]
        self.cells = self.dims[0] * self.dims[1] * self.dims[2]
        self.left_over = 0                      # of the last nearest(): the queries the all-pairs search finished

    def _queries(self, queries):
        from . import mesheval
        q = mesheval._points(queries, 'query points')
        if q.shape[0] == 0:
            raise L.GeobiError('%s.nearest: empty query set' % type(self).__name__)
        if q.device != self.cell_start.device:
            raise L.GeobiError('%s.nearest: the queries live on %s, the grid on %s' % (type(self).__name__, q.device,
                                                                                      self.cell_start.device))
        return q

    def _search(self, name, q, target, rows, order, max_rings, finish):
        Q, dev = q.shape[0], q.device
        rings = -1 if max_rings is None else int(max_rings)
        if rings < 0 and max_rings is not None:
            raise ValueError('max_rings = %r (None: the default of %d shells; 0: every query goes to the all-pairs search)'
                             % (max_rings, default_rings()))
        dist = torch.empty(Q, dtype=torch.float32, device=dev)
        idx = torch.empty(Q, dtype=torch.int32, device=dev)
        left = torch.empty(Q, dtype=torch.int32, device=dev)
        left_q = torch.empty((Q, 3), dtype=torch.float32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        ws = L.workspace(L.size_query('geobi_grid_nearest_ws_bytes', Q), dev)
        with torch.cuda.device(dev):
            L.call(name, L.ptr(q), L.ptr(target), Q, rows, self.desc, L.ptr(self.cell_start), L.ptr(order), rings,
                   L.ptr(dist), L.ptr(idx), L.ptr(left), L.ptr(left_q), L.ptr(count), L.ptr(ws), ws.numel(), L.stream())
            n = self.left_over = L.read_i32(count, 1)[0]
            if n > 0:
                d_in, i_in = finish(left_q[:n])
                L.call('geobi_grid_scatter', L.ptr(left), n, Q, L.ptr(d_in), L.ptr(i_in), L.ptr(dist), L.ptr(idx), L.stream())
        return dist, idx


def _cells_arg(cells):
    if cells is None:
        return 0
    c = int(cells)
    if not 1 <= c <= max_cells():
        raise ValueError('cells = %r (None: the rule of DESIGN.md 4u; 1 .. %d cells per axis)' % (cells, max_cells()))
    return c


def default_rings():
    return L.size_query('geobi_grid_default_rings')


def max_cells():
    return L.size_query('geobi_grid_max_cells')


def entry_cap():
    return L.size_query('geobi_grid_entry_cap')


class PointGrid(_Grid):
    """The grid over target points [T, 3] (a device tensor).  dims (nx, ny, nz), lo, hi, cell (the edge per axis), cells;
    cell_start [cells + 1] and order [entries] int32 on the device: cell c = (z * ny + y) * nx + x owns
    order[cell_start[c] : cell_start[c + 1]], indices ascending; a target with a coordinate that is not finite is in no
    cell.  cells=: that many cells on every axis with extent (tests)."""

    def __init__(self, points, cells=None):
        from . import mesheval
        force = _cells_arg(cells)
        t = self.points = mesheval._points(points, 'target points')
        T, dev = t.shape[0], t.device
        if T == 0:
            raise L.GeobiError('PointGrid: empty query or target set (T = 0)')
        desc = (ctypes.c_int32 * 16)()
        with torch.cuda.device(dev):
            ws = L.workspace(L.size_query('geobi_grid_plan_ws_bytes', 0), dev)
            L.call('geobi_grid_points_plan', L.ptr(t), T, force, desc, L.ptr(ws), ws.numel(), L.stream())
            self._take(desc)
            self.cell_start = torch.empty(self.cells + 1, dtype=torch.int32, device=dev)
            order = torch.empty(T, dtype=torch.int32, device=dev)
            ws = L.workspace(L.size_query('geobi_grid_points_build_ws_bytes', T), dev)
            L.call('geobi_grid_points_build', L.ptr(t), T, desc, L.ptr(self.cell_start), L.ptr(order), L.ptr(ws), ws.numel(),
                   L.stream())
        self.order, self._order_arg = order[:self.entries], order     # an empty slice has no pointer to hand over

    def nearest(self, queries, max_rings=None):
        """-> (dist float32 [Q], idx int32 [Q]): ``mesheval.nearest_point(queries, points)``, bit for bit"""
        from . import mesheval
        q = self._queries(queries)
        return self._search('geobi_grid_nearest_point', q, self.points, self.points.shape[0], self._order_arg, max_rings,
                            lambda rest: mesheval.nearest_point(rest, self.points))


class TriangleGrid(_Grid):
    """The grid over the triangles of (verts [V, 3], faces [F, 3]) (device tensors; the faces are range-checked).  As
    PointGrid, with a face filed in every cell its bounding box meets (entries <= entry_cap() * F: the plan halves the
    resolution until they fit, ``rounds`` counts) and records [F, 16] float32: what the search reads instead of corners.  A
    face with a corner that is not finite is in no cell."""

    def __init__(self, verts, faces, cells=None):
        from . import mesheval
        force = _cells_arg(cells)
        v = self.verts = mesheval._points(verts, 'mesh vertices')
        L.require_device(faces, 'faces')
        V, F, dev = v.shape[0], faces.shape[0], v.device
        if V == 0 or F == 0 or faces.dim() != 2 or faces.shape[1] != 3:
            raise L.GeobiError('TriangleGrid: empty query set or mesh (V = %d, faces %s)' % (V, tuple(faces.shape)))
        meshin.check_faces(faces, V)                             # range-checked before a kernel walks it
        fv = self.faces = faces.to(torch.int32).contiguous()
        desc = (ctypes.c_int32 * 16)()
        with torch.cuda.device(dev):
            ws = L.workspace(L.size_query('geobi_grid_plan_ws_bytes', F), dev)
            L.call('geobi_grid_triangles_plan', L.ptr(v), L.ptr(fv), V, F, force, desc, L.ptr(ws), ws.numel(), L.stream())
            self._take(desc)
            self.cell_start = torch.empty(self.cells + 1, dtype=torch.int32, device=dev)
            self.order = torch.empty(self.entries, dtype=torch.int32, device=dev)
            self.records = torch.empty((F, 16), dtype=torch.float32, device=dev)
            ws = L.workspace(L.size_query('geobi_grid_triangles_build_ws_bytes', F), dev)
            # an empty `order` (every face left out) still hands the call a pointer it never follows
            order = self.order if self.entries > 0 else torch.empty(1, dtype=torch.int32, device=dev)
            L.call('geobi_grid_triangles_build', L.ptr(v), L.ptr(fv), V, F, desc, L.ptr(self.cell_start), L.ptr(order),
                   L.ptr(self.records), L.ptr(ws), ws.numel(), L.stream())
            self._order_arg = order

    def nearest(self, queries, max_rings=None):
        """-> (dist float32 [Q], face int32 [Q]): ``mesheval.point_to_mesh(queries, verts, faces)``, bit for bit"""
        from . import mesheval
        q = self._queries(queries)
        return self._search('geobi_grid_nearest_triangle', q, self.records, self.faces.shape[0], self._order_arg, max_rings,
                            lambda rest: mesheval.point_to_mesh(rest, self.verts, self.faces))


def point_grid(index, points):
    """the PointGrid behind ``index`` for the targets ``points``: built now ('grid') or the one handed in, whose rows must
    be these"""
    if isinstance(index, PointGrid):
        if tuple(index.points.shape) != tuple(points.shape):
            raise ValueError('index: a PointGrid over %d points for a target set of %d' % (index.points.shape[0], points.shape[0]))
        return index
    if isinstance(index, TriangleGrid):
        raise ValueError('index: a TriangleGrid cannot serve a search among points')
    return PointGrid(points)


def triangle_grid(index, verts, faces):
    """the TriangleGrid behind ``index`` for the surface (verts, faces), as ``point_grid``"""
    if isinstance(index, TriangleGrid):
        if index.verts.shape[0] != verts.shape[0] or index.faces.shape[0] != faces.shape[0]:
            raise ValueError('index: a TriangleGrid over V = %d, F = %d for a surface of V = %d, F = %d'
                             % (index.verts.shape[0], index.faces.shape[0], verts.shape[0], faces.shape[0]))
        return index
    if isinstance(index, PointGrid):
        raise ValueError('index: a PointGrid cannot serve a search among triangles')
    return TriangleGrid(verts, faces)
