"""Wavefront OBJ in and out (host, numpy only): the file step around patches.predict_mesh that the reference does
with openmesh (om.read_trimesh / om.write_mesh, code/test_dual.py:30,73, code/data_util.py:579-580).

Vertex order and face order are the file's: the network's outputs are indexed by them.

Known difference: openmesh's read_trimesh drops a face that would make an edge non-manifold (and a degenerate or
duplicate one); this reader keeps every face the file lists.  meshclean.clean_mesh applies that rule (and welds vertices)
on the device: the `clean` command, `denoise --clean`.
"""
import math

import numpy as np


def _corner_index(token, n_vertices, path, lineno):
    """The vertex index of one face corner `i`, `i/t`, `i//n`, `i/t/n` (1-based, negative = relative) -> 0-based."""
    head = token.split('/', 1)[0]
    try:
        i = int(head)
    except ValueError:
        raise ValueError('%s:%d: face corner %r is not an index' % (path, lineno, token))
    k = i - 1 if i > 0 else n_vertices + i          # a relative index counts back from the vertices read so far
    if i == 0 or k < 0:
        raise ValueError('%s:%d: vertex index %d outside [1, %d]' % (path, lineno, i, n_vertices))
    return k                                        # positive ones are checked against the file's V at the end


def read_obj(path):
    """-> (points float32 [V, 3], faces int32 [F, 3]).

    `v x y z [w | r g b]` (extra fields ignored); `f` corners as `i`, `i/t`, `i//n`, `i/t/n`, negative (relative)
    indices; polygons are fan-triangulated (0, k, k+1) as openmesh's read_trimesh does; comments, blank lines, CRLF
    endings and every other record type are skipped.  ValueError (file and line) for an index outside [1, V], a face
    with fewer than 3 corners, a non-finite or unreadable coordinate."""
    points, faces, face_line = [], [], []
    with open(path, 'r', errors='replace') as fh:
        for lineno, line in enumerate(fh, 1):
            fields = line.split()
            if not fields:
                continue
            key = fields[0]
            if key == 'v':
                if len(fields) < 4:
                    raise ValueError('%s:%d: vertex with %d coordinates' % (path, lineno, len(fields) - 1))
                try:
                    xyz = (float(fields[1]), float(fields[2]), float(fields[3]))
                except ValueError:
                    raise ValueError('%s:%d: unreadable vertex coordinate in %r' % (path, lineno, line.strip()))
                if not (math.isfinite(xyz[0]) and math.isfinite(xyz[1]) and math.isfinite(xyz[2])):
                    raise ValueError('%s:%d: non-finite vertex coordinate in %r' % (path, lineno, line.strip()))
                points.append(xyz)
            elif key == 'f':
                if len(fields) < 4:
                    raise ValueError('%s:%d: face with %d corners (at least 3 needed)' % (path, lineno, len(fields) - 1))
                nv = len(points)
                c = [_corner_index(t, nv, path, lineno) for t in fields[1:]]
                for k in range(1, len(c) - 1):
                    faces.append((c[0], c[k], c[k + 1]))
                    face_line.append(lineno)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3).astype(np.float32)
    fv = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    bad = np.nonzero((fv >= pts.shape[0]).any(1))[0]
    if bad.size:
        raise ValueError('%s:%d: vertex index %d outside [1, %d]'
                         % (path, face_line[bad[0]], int(fv[bad[0]].max()) + 1, pts.shape[0]))
    return pts, fv.astype(np.int32)


def write_obj(path, points, faces, normals=None):
    """`v %.9g %.9g %.9g` and 1-based `f a b c`: nine significant digits identify a float32, so a float32 mesh survives
    write_obj -> read_obj bit for bit.  normals (optional, one row per point): a `vn %.9g %.9g %.9g` line per point after
    the `v` lines -- a point cloud with normals; read_obj skips them."""
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    fv = np.asarray(faces).reshape(-1, 3).astype(np.int64) + 1
    if normals is not None:
        vn = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
        if vn.shape != pts.shape:
            raise ValueError('%s: %d normals for %d points' % (path, vn.shape[0], pts.shape[0]))
    with open(path, 'w') as fh:
        fh.write(''.join('v %.9g %.9g %.9g\n' % (x, y, z) for x, y, z in pts.tolist()))
        if normals is not None:
            fh.write(''.join('vn %.9g %.9g %.9g\n' % (x, y, z) for x, y, z in vn.tolist()))
        fh.write(''.join('f %d %d %d\n' % (a, b, c) for a, b, c in fv.tolist()))


def unreferenced_vertices(num_vertices, faces):
    """How many of the num_vertices vertices no face references (the vertex update averages over a vertex's faces)."""
    used = np.zeros(int(num_vertices), dtype=bool)
    f = np.asarray(faces).reshape(-1)
    used[f] = True
    return int(num_vertices) - int(used.sum())
