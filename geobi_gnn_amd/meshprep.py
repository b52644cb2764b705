"""Mesh -> the hot path's inputs, on the MI355X.

Device counterpart of ``meshgen.build_dual_data`` -- i.e. of what the reference's loader computes on
the CPU with openmesh + PyG before the network runs:

* /root/reference/code/dataset.py:197-233  ``process_one_submesh`` (normals, vertex graph
  ``to_undirected(ev.T)`` + self loops, facet graph, bilateral weights, pos / normal per node),
* /root/reference/code/data_util.py:383-398 ``calc_weight``, :436-456 ``build_facet_graph``,
  :201-230 ``center_and_scale`` (s_type 0),
* /root/reference/code/dataset.py:246-269  ``post_processing`` (feature assembly).

The graphs are emitted directly as the (row, col)-sorted, loop-free CSR the conv / pooling kernels walk
(``graph.Graph``) -- no COO round trip, no sort.  ``edge_weight`` is stored in that order.  The int64 COO
``edge_index`` the module surface exposes is materialised lazily (loop-free); pass
``reference_layout=True`` to get the reference's exact tensors instead (vertex graph: sorted pairs then
V appended self loops; facet graph: self loops inline; loop weights as calc_weight gives them).
"""
import torch

from . import _lib as L
from . import meshin
from .data import Data
from .data_util import depth_direction
from .graph import Graph, attach


def vertex_faces(faces, num_vertices):
    """Vertex -> face incidence of a triangle list: (rowptr [V+1], list [3F]) int32, faces ascending."""
    fv = faces
    dev = fv.device
    F, V = fv.shape[0], int(num_vertices)
    rowptr = torch.empty(V + 1, dtype=torch.int32, device=dev)
    lst = torch.empty(max(3 * F, 1), dtype=torch.int32, device=dev)
    ws = L.workspace(L.size_query('geobi_vertex_faces_ws_bytes', F, V), dev)
    L.call('geobi_vertex_faces', L.ptr(fv), F, V, L.ptr(rowptr), L.ptr(lst), L.ptr(ws), ws.numel(), L.stream())
    return rowptr, lst[:3 * F]


def max_valence(rowptr, num_vertices):
    """The largest valence as a device word [1] (enqueued): the width of the padded vf table, once it is read."""
    m = torch.zeros(1, dtype=torch.int32, device=rowptr.device)
    L.call('geobi_max_degree', L.ptr(rowptr), int(num_vertices), L.ptr(m), L.stream())
    return m


def vf_padded32_fill(rowptr, lst, num_vertices, maxval):
    """The padded table for the width read from max_valence (at least one column)."""
    maxval = max(maxval, 1)
    vf = torch.empty((int(num_vertices), maxval), dtype=torch.int32, device=rowptr.device)
    L.call('geobi_vf_padded', L.ptr(rowptr), L.ptr(lst), int(num_vertices), maxval, L.ptr(vf), L.stream())
    return vf


def vf_padded32(rowptr, lst, num_vertices):
    """openmesh ``vf_indices`` as int32: [V, max_valence], -1 padded (what the device ring growth walks)."""
    return vf_padded32_fill(rowptr, lst, num_vertices, L.read_i32(max_valence(rowptr, num_vertices), 1)[0])


def vf_padded(rowptr, lst, num_vertices):
    """openmesh ``vf_indices``: [V, max_valence] int64, -1 padded (what update_position2 takes)."""
    return vf_padded32(rowptr, lst, num_vertices).long()


def mesh_normals(points, faces, rowptr, lst):
    """-> (face normals [F,3], face centroids [F,3], vertex normals [V,3]) fp32."""
    dev = points.device
    F, V = faces.shape[0], points.shape[0]
    fn = torch.empty((F, 3), dtype=torch.float32, device=dev)
    cen = torch.empty((F, 3), dtype=torch.float32, device=dev)
    vn = torch.empty((V, 3), dtype=torch.float32, device=dev)
    L.call('geobi_mesh_normals', L.ptr(points), L.ptr(faces), F, V, L.ptr(rowptr), L.ptr(lst), L.ptr(fn),
           L.ptr(cen), L.ptr(vn), L.stream())
    return fn, cen, vn


def face_normals_centroids(points, faces):
    """mesh_normals without the incidence (so without vertex normals) -> (face normals [F,3], face centroids [F,3])."""
    F = faces.shape[0]
    fn = torch.empty((F, 3), dtype=torch.float32, device=points.device)
    cen = torch.empty((F, 3), dtype=torch.float32, device=points.device)
    L.call('geobi_mesh_normals', L.ptr(points), L.ptr(faces), F, points.shape[0], None, None, L.ptr(fn), L.ptr(cen), None,
           L.stream())
    return fn, cen


def ring_graph_count(kind, faces, rowptr, lst, num_nodes):
    """ring_graph's first step, enqueued: the graph's row pointer [n+1]; its last word is the edge count."""
    n = int(num_nodes)
    rp = torch.empty(n + 1, dtype=torch.int32, device=faces.device)
    ws = L.workspace(L.size_query('geobi_ring_graph_ws_bytes', n), faces.device)
    L.call('geobi_ring_graph_count', kind, L.ptr(faces), L.ptr(rowptr), L.ptr(lst), n, L.ptr(rp), L.ptr(ws),
           ws.numel(), L.stream())
    return rp


def ring_graph_fill(kind, faces, rowptr, lst, rp, E):
    """ring_graph's second step: the columns of the E edges counted in ``rp`` -> ``Graph``."""
    dev, n = faces.device, rp.numel() - 1
    col = torch.empty(max(E, 1), dtype=torch.int32, device=dev)[:E]
    if E > 0:         # a graph without edges (the facet graph of a one-face patch: found by tools/fuzz_mesh.py) has nothing to fill
        L.call('geobi_ring_graph_fill', kind, L.ptr(faces), L.ptr(rowptr), L.ptr(lst), n, L.ptr(rp), L.ptr(col),
               L.stream())
    g = Graph(n, dev)
    g.rowptr_out, g.col_out, g.E = rp, col, E
    g.symmetric = True                                      # sharing a face / a vertex is a symmetric relation
    return g


def ring_graph(kind, faces, rowptr, lst, num_nodes):
    """kind 0: vertex graph, 1: facet graph -> loop-free symmetric ``Graph`` ((row, col)-sorted CSR)."""
    rp = ring_graph_count(kind, faces, rowptr, lst, num_nodes)
    E = L.read_i32(rp[-1:], 1)[0]                           # one host read per graph (sizes the column array)
    return ring_graph_fill(kind, faces, rowptr, lst, rp, E)


def calc_weight(pos, normal, graph, extra_zero_edges=None, want_mean=False):
    """data_util.calc_weight over the loop-free edges of ``graph`` (CSR order).  The reference's edge list
    also holds one zero-length self loop per node, which enters its mean edge length: ``extra_zero_edges``
    (default N) adds them to the denominator."""
    dev = pos.device
    extra = graph.N if extra_zero_edges is None else int(extra_zero_edges)
    w = torch.empty(max(graph.E, 1), dtype=torch.float32, device=dev)[:graph.E]
    mean = torch.zeros(1, dtype=torch.float32, device=dev) if want_mean else None
    ws = L.workspace(L.size_query('geobi_calc_weight_ws_bytes'), dev)
    L.call('geobi_calc_weight', L.ptr(pos), L.ptr(normal), L.ptr(graph.ensure_rows()), L.ptr(graph.col_out), graph.E,
           extra, L.ptr(w), L.ptr(mean), L.ptr(ws), ws.numel(), L.stream())
    return (w, mean) if want_mean else w


def mean_edge_length(pos, graph):
    """Mean length of the mesh edges (center_and_scale's 1/scale, data_util.py:201-230) -> device scalar."""
    dev = pos.device
    mean = torch.zeros(1, dtype=torch.float32, device=dev)
    ws = L.workspace(L.size_query('geobi_calc_weight_ws_bytes'), dev)
    L.call('geobi_calc_weight', L.ptr(pos), None, L.ptr(graph.ensure_rows()), L.ptr(graph.col_out), graph.E, 0, None,
           L.ptr(mean), L.ptr(ws), ws.numel(), L.stream())
    return mean


def _reference_coo(graph, weight, normal, loops_inline):
    """The reference's COO + weights for a loop-free sorted graph: self loops appended (vertex graph,
    add_self_loops) or merged in row-major order (facet graph, coalesce).  calc_weight gives a loop
    clamp(n.n, 1e-3) * exp(0): 1 for unit normals, 1e-3 for the zero normal of a face-less vertex."""
    dev = graph.device
    n = graph.N
    row, col = graph.ensure_rows().long(), graph.col_out.long()
    loops = torch.arange(n, device=dev)
    r, c = torch.cat([row, loops]), torch.cat([col, loops])
    w = torch.cat([weight, (normal * normal).sum(1).clamp(min=0.001)])
    if loops_inline:
        order = torch.argsort(r * n + c)
        r, c, w = r[order], c[order], w[order]
    return torch.stack([r, c], 0), w


def calc_weight_parts(pos, normal, graph, node_ptr):
    """calc_weight over a disjoint union of meshes: ``node_ptr`` (device int32 [P+1]) cuts the nodes into parts and every
    part is normalised by ITS OWN mean edge length (geobi_calc_weight_parts: bit-identical to the part alone)."""
    dev = pos.device
    n_parts = int(node_ptr.numel()) - 1
    w = torch.empty(max(graph.E, 1), dtype=torch.float32, device=dev)[:graph.E]
    ws = L.workspace(L.size_query('geobi_calc_weight_parts_ws_bytes', n_parts), dev)
    L.call('geobi_calc_weight_parts', L.ptr(pos), L.ptr(normal), L.ptr(graph.rowptr_out), L.ptr(graph.ensure_rows()),
           L.ptr(graph.col_out), graph.E, L.ptr(node_ptr), n_parts, L.ptr(w), L.ptr(ws), ws.numel(), L.stream())
    return w


def _normalisation(pts, g_v, centroid, scale, points_gt, host_scale):
    """center_and_scale, s_type 0, as build_dual_data and refresh_dual_data share it: centroid = mean vertex [1,3] and
    scale = 1 / mean mesh-edge length, unless given; host_scale: the computed scale as a host float (one read), else it
    stays a device [1] tensor.  -> (centroid, scale, ground-truth points on the device, those normalised); None, None
    without points_gt."""
    if centroid is None:
        cen = pts.mean(0, keepdim=True)
    else:
        cen = torch.as_tensor(centroid, dtype=torch.float32).reshape(1, 3).to(pts.device)
    if scale is not None:
        sc = float(scale)
    else:
        sc = 1.0 / mean_edge_length(pts, g_v)
        if host_scale:
            sc = float(sc.item())
    if points_gt is None:
        return cen, sc, None, None
    pg = meshin.to_device(points_gt, pts.device, torch.float32)
    return cen, sc, pg, (pg - cen) * sc


def build_dual_data(points_noisy, faces, points_gt=None, name='mesh', data_type='Synthetic', device=None,
                    reference_layout=False, centroid=None, scale=None, trusted_faces=False, want_vf=True, parts=None):
    """(points [V,3], faces [F,3]) -> (data_v, data_f) as process_one_submesh + post_processing emit them,
    computed on the device.  Same fields as ``meshgen.build_dual_data`` (incl. ``data_v.meta``).
    ``centroid`` [1,3] / ``scale``: normalisation of the WHOLE mesh when this is one patch of it
    (dataset.py:177-178 overwrite the patch's own values).
    trusted_faces: the face table was produced by this library (a patch of geobi_submesh): no range check.
    want_vf=False: no padded vf table in ``data_v.meta`` (a patch is never vertex-updated on its own).
    parts: (vertex_ptr, face_ptr) host int lists when the input is a DISJOINT UNION of meshes (the patches of one network
    pass, vertices / faces of part k in [ptr[k], ptr[k+1])): one preprocessing for all of them -- every step is local to a
    connected component except the bilateral weights' mean edge length, which is taken per part; ``mesh_ptr`` is set."""
    # A face table from outside is range-checked BEFORE any kernel walks it (a bad vertex id is a faulting gather); one
    # produced by this library (a patch of geobi_submesh) is not.
    pts, fv = meshin.device_mesh(points_noisy, faces, meshin.default_device(device), check=not trusted_faces)
    dev, V, F = pts.device, pts.shape[0], fv.shape[0]
    # Everything else whose size the host must know before it can allocate comes back in ONE read: both graphs' edge
    # counts and the largest valence (width of the padded vf table).  Until round 4 these were separate reads.
    rowptr_vf, lst = vertex_faces(fv, V)
    rp_v = ring_graph_count(0, fv, rowptr_vf, lst, V)
    rp_f = ring_graph_count(1, fv, rowptr_vf, lst, F)
    size_words = [rp_v[-1:], rp_f[-1:]] + ([max_valence(rowptr_vf, V)] if want_vf else [])
    sizes = L.read_i32(torch.cat(size_words))
    fn, pos_f, vn = mesh_normals(pts, fv, rowptr_vf, lst)
    g_v = ring_graph_fill(0, fv, rowptr_vf, lst, rp_v, sizes[0])
    g_f = ring_graph_fill(1, fv, rowptr_vf, lst, rp_f, sizes[1])
    cen, sc, pg, y = _normalisation(pts, g_v, centroid, scale, points_gt, host_scale=True)

    if parts is None:
        ew_v = calc_weight(pts, vn, g_v)
        ew_f = calc_weight(pos_f, fn, g_f)
    else:
        ptr_dev = torch.tensor(list(parts[0]) + list(parts[1]), dtype=torch.int32).to(dev, non_blocking=True)
        nvp = len(parts[0])
        ew_v = calc_weight_parts(pts, vn, g_v, ptr_dev[:nvp])
        ew_f = calc_weight_parts(pos_f, fn, g_f, ptr_dev[nvp:])

    data_v = Data(torch.cat(((pts - cen) * sc, vn), 1), None, name=name + '-v')
    data_f = Data(torch.cat(((pos_f - cen) * sc, fn), 1), None, fv_indices=fv.long(), name=name + '-f')
    from .network import mark_face_table
    mark_face_table(data_f.fv_indices, fv, V)          # ids were range-checked above
    if reference_layout:
        ei_v, w_v = _reference_coo(g_v, ew_v, vn, loops_inline=False)
        ei_f, w_f = _reference_coo(g_f, ew_f, fn, loops_inline=True)
        data_v.edge_index, data_v.edge_weight = ei_v, w_v
        data_f.edge_index, data_f.edge_weight = ei_f, w_f
    else:
        data_v.set_graph(g_v); data_v.edge_weight = ew_v
        data_f.set_graph(g_f); data_f.edge_weight = ew_f
    data_v.depth_direction = depth_direction(pts, data_type)
    if pg is not None:
        data_v.y, data_f.y = y, face_normals_centroids(pg, fv)[0]
    vf = vf_padded32_fill(rowptr_vf, lst, V, sizes[2]).long() if want_vf else None
    data_v.meta = {'centroid': cen, 'scale': sc, 'vf_indices': vf, 'incidence': (rowptr_vf, lst)}
    if parts is not None:
        data_v.mesh_ptr = torch.tensor(list(parts[0]), dtype=torch.long)
        data_f.mesh_ptr = torch.tensor(list(parts[1]), dtype=torch.long)
    return data_v, data_f


def refresh_dual_data(data_v, data_f, points_noisy, points_gt, data_type='Synthetic', incidence=None, centroid=None,
                      scale=None):
    """New noisy points on the connectivity of an existing ``build_dual_data`` pair, in place: the graphs do not depend
    on the points, so both ``Graph`` objects (with their reverse-edge index), the face table and its validation mark stay
    as they are -- no CSR build, no host size read -- and only what moves is recomputed, by the calls ``build_dual_data``
    makes and in its order, so every value equals a fresh build bit for bit: normals, centroid and scale, both bilateral
    weight vectors, both feature matrices, ``depth_direction`` (Kinect types) and ``data_v.y``.  ``data_f.y`` (the
    normals of the ground truth) does not move.  incidence: (rowptr, list) of meshprep.vertex_faces; default: that of
    ``data_v.meta``, else recomputed.  ``data_v.meta`` -- where present -- takes the new centroid and scale (one host
    read, as the build; without it the scale stays on the device).  -> (data_v, data_f)"""
    g_v, g_f = data_v.graph(), data_f.graph()
    if g_v.eid_out is not None or g_f.eid_out is not None:
        raise L.GeobiError('refresh_dual_data: a pair in the reference layout (COO with self loops) is rebuilt, not refreshed')
    pts = meshin.to_device(points_noisy, g_v.device, torch.float32)
    cache = getattr(data_f.fv_indices, '_geobi_fv', None)
    V = g_v.N
    if cache is None or cache[2] != V:
        raise L.GeobiError('refresh_dual_data: the face table was not validated for %d vertices (not a build_dual_data pair)' % V)
    fv = cache[0]
    if pts.shape != (V, 3) or fv.shape[0] != g_f.N:
        raise ValueError('refresh_dual_data: %s points for a pair of %d vertices and %d faces' % (tuple(pts.shape), V, g_f.N))
    meta = getattr(data_v, 'meta', None)
    if incidence is None:
        incidence = meta['incidence'] if isinstance(meta, dict) and meta.get('incidence') is not None else vertex_faces(fv, V)
    rowptr_vf, lst = incidence
    fn, pos_f, vn = mesh_normals(pts, fv, rowptr_vf, lst)
    cen, sc, _, y = _normalisation(pts, g_v, centroid, scale, points_gt, host_scale=isinstance(meta, dict))
    ew_v = calc_weight(pts, vn, g_v)
    ew_f = calc_weight(pos_f, fn, g_f)
    data_v.x = torch.cat(((pts - cen) * sc, vn), 1)
    data_f.x = torch.cat(((pos_f - cen) * sc, fn), 1)
    data_v.edge_weight, data_f.edge_weight = ew_v, ew_f
    data_v.depth_direction = depth_direction(pts, data_type)
    if y is not None:
        data_v.y = y
    if isinstance(meta, dict):
        meta['centroid'], meta['scale'] = cen, sc
    return data_v, data_f
