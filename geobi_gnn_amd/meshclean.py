"""Mesh repair on the MI355X: weld vertices, drop bad faces, compact -- the step in front of
``meshprep`` for files that are not clean triangle meshes (scanner output, STL-derived triangle soups, CAD exports).

The reference reads OBJ through openmesh, whose ``read_trimesh`` refuses a face that is degenerate, duplicated or would
give a directed edge a second owner (code/test_dual.py:30, code/dataset.py:197); ``meshio.read_obj``
keeps every face.  ``clean_mesh`` applies that rule, after a weld openmesh does not have:

* **weld**: ``canon[v]`` = the lowest index among the vertices with v's key.  ``weld_tol=0.0``: the three float32 bit
  patterns (-0.0 as +0.0); ``weld_tol > 0``: the int32 triple ``floorf(x / weld_tol)``, i.e. cells of side weld_tol --
  this SNAPS TO A GRID, it is no epsilon-merge: two points closer than weld_tol can lie in two cells and stay apart;
  ``weld_tol=None``: no welding
* **degenerate faces** (two equal corners after welding) are dropped
* **half-edge rule** (``manifold=True``): walking the faces in ascending index, a face is kept iff none of its directed
  half-edges a->b, b->c, c->a is owned by a kept earlier face.  A second copy of a face is dropped, the same triangle
  with the opposite orientation is kept, a dropped face owns nothing.  openmesh's complex-VERTEX ("bow-tie") rule is not
  replicated
* **compaction**: kept faces and used vertices keep their relative order; a welded group keeps the coordinates of its
  lowest-index member (not a mean)

* **topology** (``orient=True``, ``min_component=m``; ``meshtopo``): after the weld and before the
  half-edge rule the faces are wound consistently per component -- two neighbours wound in opposite senses walk their
  common edge in the same direction, and the half-edge rule alone would drop one of them; after the rule, the faces of
  every edge-connected part of fewer than m kept faces are dropped too (state 4, not counted as nonmanifold)
* **self-intersections** (``drop_intersecting=True``; ``meshselfx``): after the half-edge rule and
  before ``min_component`` the kept faces that intersect another kept face are dropped together (state 5, counted under
  ``intersecting`` alone)

Everything is integer-exact (geobi_clean_* in csrc/clean.hip).  No CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from . import meshin


class CleanResult(object):
    """points [V', 3] float32, faces [F', 3] int32 (cleaned numbering), vertex_map [V] (new index of canon[v], or -1),
    vertex_src [V'] (input index of every cleaned vertex), face_map [F'] (input index of every kept face), canon [V];
    counts: welded, degenerate, nonmanifold, unreferenced, rounds (and intersecting with ``drop_intersecting``).  With ``orient`` / ``min_component``: topology, a dict of
    flipped, nonorientable, orient_components, orient_rounds (orient) and components, components_dropped, faces_dropped,
    component_rounds (min_component), turned and open_components (outward), else None; face_flip [F] (input numbering: 1 where the winding was reversed)."""

    def __init__(self, points, faces, vertex_map, vertex_src, face_map, canon, counts, topology=None, face_flip=None):
        self.points, self.faces = points, faces
        self.vertex_map, self.vertex_src, self.face_map, self.canon = vertex_map, vertex_src, face_map, canon
        self.counts = counts
        self.topology, self.face_flip = topology, face_flip


def _index(a, like):
    """the index array ``a`` in the form that indexes ``like``: an int64 tensor on its device, or an int64 numpy array"""
    if torch.is_tensor(like):
        return torch.as_tensor(a).to(like.device).long()
    return (a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.int64)


def apply(result, points_in):
    """Another position array of the INPUT's numbering [V, 3] (the paired noisy or ground-truth points) -> the cleaned
    numbering [V', 3]: the row of every cleaned vertex's canonical input vertex.  Tensors or numpy arrays."""
    if points_in.shape[0] != result.vertex_map.shape[0]:
        raise ValueError('apply: %d rows for a cleaning of %d vertices' % (points_in.shape[0], result.vertex_map.shape[0]))
    return points_in[_index(result.vertex_src, points_in)]


def scatter_back(result, points_clean, points_in):
    """Positions of the cleaned numbering [V', 3] -> the input's numbering [V, 3]: a row with vertex_map >= 0 takes
    points_clean[vertex_map] (all members of a weld group share it), the rest keep points_in bit for bit."""
    vm = _index(result.vertex_map, points_in)
    if points_in.shape[0] != vm.shape[0] or points_clean.shape[0] != result.vertex_src.shape[0]:
        raise ValueError('scatter_back: %d clean and %d input rows for a cleaning of %d -> %d vertices'
                         % (points_clean.shape[0], points_in.shape[0], vm.shape[0], result.vertex_src.shape[0]))
    out = points_in.clone() if torch.is_tensor(points_in) else np.array(points_in, copy=True)
    hit = vm >= 0
    out[hit] = points_clean[vm[hit]]
    return out


def _empty(n, width, dtype, dev):
    shape = (max(n, 1),) if width == 0 else (max(n, 1), width)
    return torch.empty(shape, dtype=dtype, device=dev)


def weld(pts, weld_tol):
    """Stage 1 on validated device points [V, 3]: -> (canon [max(V, 1)] int32, device counts [2] = groups, overflow flag);
    enqueued, nothing is read back."""
    dev, V = pts.device, pts.shape[0]
    canon = _empty(V, 0, torch.int32, dev)
    wcounts = torch.zeros(2, dtype=torch.int32, device=dev)
    mode = 0 if weld_tol is None else (1 if float(weld_tol) == 0.0 else 2)
    ws = L.workspace(L.size_query('geobi_clean_weld_ws_bytes', V), dev)
    L.call('geobi_clean_weld', L.ptr(pts if V else _empty(0, 3, torch.float32, dev)), V, mode, float(weld_tol or 0.0),
           L.ptr(canon), L.ptr(wcounts), L.ptr(ws), ws.numel(), L.stream())
    return canon, wcounts


def resolve_faces(fv, canon, V, manifold=True, max_rounds=1024):
    """Stage 2 on range-checked device faces [F, 3] int32 of a mesh of V vertices: -> (faces through canon [max(F, 1), 3], state [max(F, 1)]: 1 kept,
    2 dropped by the half-edge rule, 3 degenerate; rounds).  Waits for the device once per batch of rounds."""
    dev, F = fv.device, fv.shape[0]
    fc = _empty(F, 3, torch.int32, dev)
    state = _empty(F, 0, torch.int32, dev)
    rounds = (ctypes.c_int32 * 1)()
    ws = L.workspace(L.size_query('geobi_clean_faces_ws_bytes', F), dev)
    L.call('geobi_clean_faces', L.ptr(fv if F else fc), L.ptr(canon), F, int(V), 1 if manifold else 0, int(max_rounds),
           L.ptr(fc), L.ptr(state), rounds, L.ptr(ws), ws.numel(), L.stream())
    return fc, state, int(rounds[0])


def compact(pts, fc, state, canon, F):
    """Stage 3 (F: the number of faces, fc / state have at least one row): -> (points, faces, vertex_map, vertex_src, face_map) with room for V / F rows and the device counts [5] =
    V', F', degenerate, nonmanifold, unreferenced; enqueued, nothing is read back."""
    dev, V, F = pts.device, pts.shape[0], int(F)
    p_out, f_out = _empty(V, 3, torch.float32, dev), _empty(F, 3, torch.int32, dev)
    vmap, vsrc, fmap = _empty(V, 0, torch.int32, dev), _empty(V, 0, torch.int32, dev), _empty(F, 0, torch.int32, dev)
    counts = torch.zeros(5, dtype=torch.int32, device=dev)
    ws = L.workspace(L.size_query('geobi_clean_compact_ws_bytes', V, F), dev)
    L.call('geobi_clean_compact', L.ptr(pts if V else p_out), L.ptr(fc), L.ptr(state), L.ptr(canon), V, F, L.ptr(p_out),
           L.ptr(f_out), L.ptr(vmap), L.ptr(vsrc), L.ptr(fmap), L.ptr(counts), L.ptr(ws), ws.numel(), L.stream())
    return p_out, f_out, vmap, vsrc, fmap, counts


def check_weld_tol(what, weld_tol):
    if weld_tol is not None and not float(weld_tol) >= 0.0:
        raise ValueError('%s: weld_tol = %r (None, 0 or a positive cell size)' % (what, weld_tol))
    if weld_tol is not None and not np.isfinite(np.float32(weld_tol)):
        raise ValueError('%s: weld_tol = %r is not a finite float32' % (what, weld_tol))


def clean_mesh(points, faces, weld_tol=0.0, manifold=True, max_rounds=1024, device=None, orient=False, min_component=0,
               drop_intersecting=False, outward=False):
    """(points [V, 3], faces [F, 3]) -> CleanResult, on the device.  ValueError: non-finite points, a face index outside
    [0, V), weld_tol < 0, max_rounds < 1, min_component < 0.  GeobiError: the library's errors -- a grid quotient outside
    int32, more than ``max_rounds`` rounds of the half-edge rule (a chain of faces that each share a directed edge with the
    next takes one round per face), more than 256 rounds of the component search (``meshtopo``).

    ``orient``: weld, corners through canon, consistent winding per component (meshtopo.orient_device), then the
    half-edge rule on the oriented table.  ``min_component = m > 0``: after the rule, the kept faces of every
    edge-connected part of fewer than m faces are dropped (a face they displaced under the rule does not come back).
    ``drop_intersecting``: after the rule and before ``min_component``, every kept face that intersects another kept face
    (``meshselfx``) is dropped -- all of them together, in one pass -- and counted under ``intersecting``;
    ``meshfill`` closes the holes this opens.  ``outward``: implies ``orient``, and ``meshwind.outward_device`` stands in
    ``orient_device``'s place: every closed part is then wound so that its normals point out of the solid;
    ``face_flip`` carries both flips, ``topology`` gains ``turned`` and ``open_components``."""
    dev = meshin.default_device(device)
    orient = orient or bool(outward)
    check_weld_tol('clean_mesh', weld_tol)
    if int(max_rounds) < 1:
        raise ValueError('clean_mesh: max_rounds = %r (at least 1)' % (max_rounds,))
    if int(min_component) < 0:
        raise ValueError('clean_mesh: min_component = %r (0 or more)' % (min_component,))
    # the face table is range-checked as it came in (an int64 id must not wrap into range), BEFORE any kernel walks it
    pts, fv = meshin.finite_mesh(meshin.as_tensor(points).reshape(-1, 3), meshin.as_tensor(faces).reshape(-1, 3), dev,
                                 'clean_mesh')
    V, F = pts.shape[0], fv.shape[0]
    with torch.cuda.device(dev):
        canon, wcounts = weld(pts, weld_tol)
        groups, bad = L.read_i32(wcounts)
        if bad:
            raise L.GeobiError('clean_mesh: a coordinate divided by weld_tol = %g is outside the int32 range' % weld_tol)
        topology, face_flip, tcounts = None, None, []
        if orient or min_component > 0:
            from . import meshtopo
            topology = {}
        # the stages hand on tables padded to one row for F == 0: only their F rows [:F] are a mesh
        if orient:
            fc, _, _ = resolve_faces(fv, canon, V, False, max_rounds)           # the corners through canon
            if outward and F > 0:
                from . import meshwind
                oriented, face_flip, _, wcounts_host = meshwind.outward_device(pts, fc[:F].contiguous(), V)
                ocounts = torch.tensor([wcounts_host[k] for k in ('components', 'nonorientable', 'flipped')], dtype=torch.int32,
                                       device=dev)
                orient_rounds = wcounts_host['rounds']
                topology['turned'], topology['open_components'] = wcounts_host['turned'], wcounts_host['open_components']
            else:
                oriented, face_flip, _, ocounts, orient_rounds = meshtopo.orient_device(fc[:F], V)
            fv = oriented[:F]
            tcounts.append(ocounts)
            topology['orient_rounds'] = orient_rounds
        # canon is idempotent: on an oriented table it leaves every corner as it is
        fc, state, rounds = resolve_faces(fv, canon, V, manifold, max_rounds)
        if drop_intersecting:
            from . import meshselfx
            hits, _, xcounts = meshselfx.search_device(pts, fc[:F], state[:F] if F else None)
            # a state the compaction drops without counting it, as 4; only kept faces have hits
            state = torch.where(hits > 0, torch.full_like(state, meshselfx.STATE_INTERSECTING), state)
        if min_component > 0:
            _, state, ccounts, topology['component_rounds'] = meshtopo.components_device(fc[:F], V, state[:F], min_component)
            tcounts.append(ccounts)
        p_out, f_out, vmap, vsrc, fmap, counts = compact(pts, fc, state, canon, F)
        host = L.read_i32(torch.cat([counts] + tcounts) if tcounts else counts)      # one read for all counts
        v_new, f_new, degenerate, nonmanifold, unreferenced = host[:5]
        if orient:
            topology['orient_components'], topology['nonorientable'], topology['flipped'] = host[5:8]
            face_flip = face_flip[:F]
        if min_component > 0:
            topology['components'], topology['components_dropped'], topology['faces_dropped'] = host[-3:]
        if drop_intersecting:
            intersecting = dict(zip(meshselfx.COUNT_KEYS, L.read_i64(xcounts)))['faces_hit']
    result = {'welded': V - groups, 'degenerate': degenerate, 'nonmanifold': nonmanifold, 'unreferenced': unreferenced,
              'rounds': rounds}
    if drop_intersecting:
        result['intersecting'] = intersecting
    return CleanResult(p_out[:v_new], f_out[:f_new], vmap[:V], vsrc[:v_new], fmap[:f_new], canon[:V], result, topology,
                       face_flip)
