"""The invariants the grid search's correctness rests on, in plain numpy.  NOT the kernel's
arithmetic: the planes of a cell are formed in float64 from the grid's float32 numbers, and a target only has to lie within
the documented margin of where the device filed it.

A grid is a ``Tables``: dims (nx, ny, nz), lo, hi (the box), cell (the edge per axis), magnitude (the largest target
coordinate magnitude), cell_start [cells + 1], order [entries].  Cell (x, y, z) has the id (z * ny + y) * nx + x and owns
order[cell_start[id] : cell_start[id + 1]].

  check_tables     cell_start starts at 0, never descends and ends at len(order); indices ascend inside a cell (so no
                   target is listed twice in a cell); every entry names a target that is finite
  check_points     order is a permutation of exactly the finite points; every point lies inside its cell's box widened by
                   the margin
  check_triangles  every cell whose box, SHRUNK by the margin, meets the bounding box of a finite face lists that face; a
                   face with a corner that is not finite is listed nowhere; the entries stay within ENTRY_CAP * F

Every checker returns the list of what it found wrong, empty for a sound grid.  ``margin`` is the search's own: MARGIN_ULPS
* 2^-24 * (magnitude + box diagonal) for a target (its distance to the box is 0).  The outermost cells reach to infinity:
the device clamps a cell index into the grid."""
import collections

import numpy as np

MARGIN_ULPS = 32.0          # csrc/grid.hip: kMarginUlps
ENTRY_CAP = 8               # kEntryCap
MAX_CELLS = 256             # kMaxAxis
DEFAULT_RINGS = 8           # kDefaultRings
MIN_CELL_FRAC = 2.0 ** -14  # kMinCellFrac

Tables = collections.namedtuple('Tables', 'dims lo hi cell magnitude cell_start order')


def of_grid(g):
    """a device meshgrid.PointGrid / TriangleGrid -> Tables on the host"""
    return Tables(tuple(g.dims), np.array(g.lo, dtype=np.float64), np.array(g.hi, dtype=np.float64),
                  np.array(g.cell, dtype=np.float64), float(g.magnitude), g.cell_start.cpu().numpy().astype(np.int64),
                  g.order.cpu().numpy().astype(np.int64))


def margin(t):
    return MARGIN_ULPS * 2.0 ** -24 * (t.magnitude + float(np.sqrt(((t.hi - t.lo) ** 2).sum())))


def finite_rows(a):
    return np.isfinite(np.asarray(a, dtype=np.float64)).all(axis=1)


def ideal_cells(t, x):
    """the cell index per axis of coordinates x [n, 3] in exact arithmetic, clamped into the grid"""
    dims = np.array(t.dims)
    c = np.floor((np.asarray(x, dtype=np.float64) - t.lo) / t.cell).astype(np.int64)
    return np.clip(np.where(dims == 1, 0, c), 0, dims - 1)


def cell_ids(t, c):
    return (c[:, 2] * t.dims[1] + c[:, 1]) * t.dims[0] + c[:, 0]


def cell_of_entry(t):
    """the cell id of every row of order, from cell_start"""
    return np.repeat(np.arange(len(t.cell_start) - 1), np.diff(t.cell_start))


def check_tables(t, finite):
    """finite [n] bool: which targets are finite"""
    faults = []
    cells = t.dims[0] * t.dims[1] * t.dims[2]
    cs = t.cell_start
    if len(cs) != cells + 1:
        return ['cell_start has %d entries for %d cells' % (len(cs), cells)]
    if cs[0] != 0 or (np.diff(cs) < 0).any() or cs[-1] != len(t.order):
        return ['cell_start does not run from 0 to the %d entries without descending' % len(t.order)]
    if len(t.order) and (t.order.min() < 0 or t.order.max() >= len(finite)):
        return ['order names a target outside [0, %d)' % len(finite)]
    if not finite[t.order].all():
        faults.append('a target that is not finite is filed')
    cell = cell_of_entry(t)
    same = cell[1:] == cell[:-1]
    bad = same & (np.diff(t.order) <= 0)
    if bad.any():
        k = int(np.nonzero(bad)[0][0])
        faults.append('cell %d: index %d is followed by %d' % (cell[k], t.order[k], t.order[k + 1]))
    return faults


def check_points(t, points):
    points = np.asarray(points, dtype=np.float64)
    finite = finite_rows(points)
    faults = check_tables(t, finite)
    if faults:
        return faults
    if not np.array_equal(np.sort(t.order), np.nonzero(finite)[0]):
        faults.append('order is not a permutation of the %d finite targets' % int(finite.sum()))
        return faults
    cell = cell_of_entry(t)
    dims, m = np.array(t.dims), margin(t)
    c = np.stack([cell % dims[0], cell // dims[0] % dims[1], cell // (dims[0] * dims[1])], axis=1)
    x = points[t.order]
    low = np.where(c == 0, -np.inf, t.lo + c * t.cell - m)
    high = np.where(c == dims - 1, np.inf, t.lo + (c + 1) * t.cell + m)
    out = ((x < low) | (x > high)).any(axis=1)
    if out.any():
        k = int(np.nonzero(out)[0][0])
        faults.append('point %d lies outside the widened box of its cell %d' % (t.order[k], cell[k]))
    return faults


def face_boxes(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    f = np.clip(np.asarray(faces, dtype=np.int64), 0, len(v) - 1)            # the device clamps what it reads
    corners = v[f]
    return corners.min(axis=1), corners.max(axis=1), np.isfinite(corners).all(axis=(1, 2))


def required_cells(t, mn, mx):
    """per axis the first and last cell whose box, shrunk by the margin, meets [mn, mx] (first > last: none)"""
    dims, m = np.array(t.dims), margin(t)
    mn, mx = np.nan_to_num(mn, nan=0.0, posinf=0.0, neginf=0.0), np.nan_to_num(mx, nan=0.0, posinf=0.0, neginf=0.0)
    k0 = np.ceil((mn + m - t.lo) / t.cell - 1.0).astype(np.int64)            # lo + (k + 1) cell - m >= mn
    k1 = np.floor((mx - m - t.lo) / t.cell).astype(np.int64)                 # lo + k cell + m <= mx
    return np.clip(k0, 0, dims - 1), np.clip(k1, 0, dims - 1)                # the outermost cells have no outer plane


def check_triangles(t, verts, faces):
    mn, mx, finite = face_boxes(verts, faces)
    F = len(finite)
    faults = check_tables(t, finite)
    if faults:
        return faults
    if len(t.order) > ENTRY_CAP * F:
        faults.append('%d entries for %d faces: beyond the cap of %d F' % (len(t.order), F, ENTRY_CAP))
    listed = set((cell_of_entry(t) * F + t.order).tolist())
    filed = np.zeros(F, dtype=bool)
    filed[t.order] = True
    if (filed != finite).any():
        faults.append('face %d: finite = %s, filed = %s' % (int(np.nonzero(filed != finite)[0][0]), finite[filed != finite][0],
                                                            filed[filed != finite][0]))
    k0, k1 = required_cells(t, mn, mx)
    for f in np.nonzero(finite)[0]:
        if (k0[f] > k1[f]).any():
            continue
        z, y, x = np.meshgrid(*[np.arange(k0[f][a], k1[f][a] + 1) for a in (2, 1, 0)], indexing='ij')
        need = ((z * t.dims[1] + y) * t.dims[0] + x).ravel() * F + f
        missing = [k for k in need.tolist() if k not in listed]
        if missing:
            faults.append('face %d is not listed in cell %d, which its box meets' % (f, missing[0] // F))
            break
    return faults


# ---- tables made on the host, in exact arithmetic: what the hand-made cases of the host tests start from
def host_box(x, dims):
    x = np.asarray(x, dtype=np.float64)
    lo, hi = x.min(axis=0), x.max(axis=0)
    dims = np.where(hi > lo, np.array(dims), 1)
    cell = np.where(hi > lo, (hi - lo) / dims, 1.0)
    return tuple(int(d) for d in dims), lo, hi, cell, float(np.abs(x).max())


def _tables(dims, lo, hi, cell, mag, ids, items):
    keys = np.lexsort((items, ids))
    cells = dims[0] * dims[1] * dims[2]
    cell_start = np.searchsorted(ids[keys], np.arange(cells + 1)).astype(np.int64)
    return Tables(dims, lo, hi, cell, mag, cell_start, items[keys].astype(np.int64))


def host_point_tables(points, dims):
    points = np.asarray(points, dtype=np.float64)
    finite = finite_rows(points)
    dims, lo, hi, cell, mag = host_box(points[finite], dims)
    t = Tables(dims, lo, hi, cell, mag, None, None)
    items = np.nonzero(finite)[0]
    return _tables(dims, lo, hi, cell, mag, cell_ids(t, ideal_cells(t, points[items])), items)


def host_triangle_tables(verts, faces, dims):
    mn, mx, finite = face_boxes(verts, faces)
    corners = np.asarray(verts, dtype=np.float64)[np.asarray(faces)[finite]].reshape(-1, 3)
    dims, lo, hi, cell, mag = host_box(corners, dims)
    t = Tables(dims, lo, hi, cell, mag, None, None)
    ids, items = [], []
    for f in np.nonzero(finite)[0]:
        c0, c1 = ideal_cells(t, mn[f][None])[0], ideal_cells(t, mx[f][None])[0]
        z, y, x = np.meshgrid(*[np.arange(c0[a], c1[a] + 1) for a in (2, 1, 0)], indexing='ij')
        block = ((z * dims[1] + y) * dims[0] + x).ravel()
        ids.extend(block.tolist())
        items.extend([f] * len(block))
    return _tables(dims, lo, hi, cell, mag, np.array(ids, dtype=np.int64), np.array(items, dtype=np.int64))
