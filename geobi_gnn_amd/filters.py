"""Model-free mesh denoising on the MI355X: bilateral normal filtering + the vertex update.

Zheng, Fu, Au, Tai, "Bilateral normal filtering for mesh denoising" (TVCG 2011), local iterative scheme.  The reference
has no call site for it -- its scratch code only lists result folders of classical filters beside its own
(code/data_util.py:732-745) -- so this is the baseline row a trained network is read against, and what
`denoise --method bnf` runs when there is no model.

Per face i of the mesh (points P, faces (a, b, c)):

    cr_i = (b - a) x (c - a),  A_i = |cr_i| / 2,  c_i = centroid,  n_i^0 = cr_i / max(|cr_i|, 1e-12)
    N(i)    = row i of the loop-free facet graph (faces sharing at least one vertex) plus i itself
    sigma_s = sigma_s-argument x mean |c_i - c_j| over the facet-graph edges (computed once, stays on the device)
    sweep:    w_ij = A_j exp(-|c_i - c_j|^2 / (2 sigma_s^2) - |n_i - n_j|^2 / (2 sigma_r^2))
              s_i = sum_{j in N(i)} w_ij n_j,  W_i = sum w_ij
              n_i' = s_i / |s_i| if |s_i| > 1e-6 W_i, else n_i

Sweeps are Jacobi (ping-pong buffers); the kernels are csrc/filter.hip.  The filtered normals go to the vertex update the
network path uses (data_util.update_position2).  The whole mesh goes in one pass: there is no patch split.
"""
import numpy as np
import torch

from . import _lib as L
from . import meshprep


def _check_params(normal_iters, sigma_r, sigma_s):
    if int(normal_iters) != normal_iters or normal_iters < 0:
        raise ValueError('normal_iters = %r: a whole number of sweeps, not negative' % (normal_iters,))
    for name, v in (('sigma_r', sigma_r), ('sigma_s', sigma_s)):
        if not (float(v) > 0.0 and float(v) < float('inf')):
            raise ValueError('%s = %r: positive and finite' % (name, v))


def _device_mesh(points, faces, device):
    """-> (points fp32 [V,3], faces int32 [F,3]) on the device, the face table range-checked before any kernel walks it."""
    if not torch.cuda.is_available():
        raise L.GeobiError('filters: the bilateral normal filter runs on the MI355X only (no CPU fallback)')
    if device is None:
        device = points.device if torch.is_tensor(points) and points.is_cuda else torch.device('cuda', torch.cuda.current_device())
    dev = torch.device(device)
    pts = torch.as_tensor(np.asarray(points) if not torch.is_tensor(points) else points)
    pts = pts.to(device=dev, dtype=torch.float32).contiguous()
    fv = torch.as_tensor(np.asarray(faces) if not torch.is_tensor(faces) else faces).to(device=dev, dtype=torch.int32)
    fv = fv.contiguous()
    if pts.dim() != 2 or pts.shape[1] != 3 or fv.dim() != 2 or fv.shape[1] != 3:
        raise ValueError('points [V,3] and faces [F,3] expected, got %s and %s' % (tuple(pts.shape), tuple(fv.shape)))
    V, F = pts.shape[0], fv.shape[0]
    if F == 0:
        raise ValueError('the mesh has no faces')
    lo, hi = L.read_i32(torch.cat([t.reshape(1) for t in torch.aminmax(fv)]))
    if lo < 0 or hi >= V:
        raise L.GeobiError('faces index vertices outside [0, %d)' % V)
    return pts, fv


def face_records(points, fv):
    """geobi_bnf_prepare: the filter's 16-byte face rows -> (rec_c [F,4] = centroid | area, rec_n [F,4] = start normal | 0).
    points fp32 [V,3] and fv int32 [F,3] on the device, fv range-checked by the caller."""
    F = fv.shape[0]
    rec_c = torch.empty((F, 4), dtype=torch.float32, device=points.device)
    rec_n = torch.empty((F, 4), dtype=torch.float32, device=points.device)
    L.call('geobi_bnf_prepare', L.ptr(points), L.ptr(fv), F, points.shape[0], L.ptr(rec_c), L.ptr(rec_n), L.stream())
    return rec_c, rec_n


def spatial_scale(points, fv, graph, sigma_s):
    """1 / (2 sigma_s^2) as a device scalar [1]: sigma_s = `sigma_s` x the mean centroid distance over the facet graph's
    edges; 0 when there is no edge (or no distance).  No host read."""
    if graph.E == 0:
        return torch.zeros(1, dtype=torch.float32, device=points.device)
    F = fv.shape[0]
    fn = torch.empty((F, 3), dtype=torch.float32, device=points.device)
    cen = torch.empty((F, 3), dtype=torch.float32, device=points.device)
    L.call('geobi_mesh_normals', L.ptr(points), L.ptr(fv), F, points.shape[0], None, None, L.ptr(fn), L.ptr(cen), None,
           L.stream())
    s = meshprep.mean_edge_length(cen, graph) * float(sigma_s)
    return torch.where(s > 0, 0.5 / (s * s), torch.zeros_like(s))


def filter_records(rec_c, rec_n, graph, inv2ss, sigma_r, n_sweeps):
    """geobi_bnf_filter: `n_sweeps` sweeps starting from the normals in rec_n -> [F,4] rows of rec_n's layout."""
    F = rec_c.shape[0]
    out = torch.empty_like(rec_n)
    ws = L.workspace(L.size_query('geobi_bnf_filter_ws_bytes', F, graph.E), rec_c.device)
    L.call('geobi_bnf_filter', L.ptr(rec_c), L.ptr(rec_n), L.ptr(graph.rowptr_out), L.ptr(graph.col_out), F, graph.E,
           L.ptr(inv2ss), 0.5 / (float(sigma_r) * float(sigma_r)), int(n_sweeps), L.ptr(out), L.ptr(ws), ws.numel(),
           L.stream())
    return out


def _bilateral_normals(pts, fv, normal_iters, sigma_r, sigma_s, incidence):
    rowptr, lst = incidence if incidence is not None else meshprep.vertex_faces(fv, pts.shape[0])
    graph = meshprep.ring_graph(1, fv, rowptr, lst, fv.shape[0])
    rec_c, rec_n = face_records(pts, fv)
    inv2ss = spatial_scale(pts, fv, graph, sigma_s)
    return filter_records(rec_c, rec_n, graph, inv2ss, sigma_r, int(normal_iters))[:, :3].contiguous()


def bilateral_normals(points, faces, normal_iters=20, sigma_r=0.35, sigma_s=1.0, incidence=None):
    """Filtered unit face normals [F,3] (fp32, on the device) of the mesh (points [V,3], faces [F,3]).
    incidence: (rowptr, list) of meshprep.vertex_faces for these faces, if the caller has it already.
    normal_iters = 0 returns the start normals."""
    _check_params(normal_iters, sigma_r, sigma_s)
    pts, fv = _device_mesh(points, faces, None)
    with torch.cuda.device(pts.device):
        return _bilateral_normals(pts, fv, normal_iters, sigma_r, sigma_s, incidence)


def bilateral_denoise(points, faces, normal_iters=20, sigma_r=0.35, sigma_s=1.0, n_iter=20, data_type='Synthetic',
                      gt_points=None, device=None):
    """Bilateral normal filtering, then `n_iter` sweeps of the vertex update towards the filtered normals.
    -> dict(Np, V_updated, angle1, angle2) with the meaning of patches.predict_mesh's keys: Np the filtered normals,
    V_updated the moved vertices; with gt_points, angle1 = mean angle (degrees) of Np against the ground truth's face
    normals, angle2 = that of the updated mesh's normals (None without).  Kinect data types move vertices along
    normalize(points) only, as predict_mesh does."""
    from . import network
    from .data_util import computer_face_normal, update_position2
    _check_params(normal_iters, sigma_r, sigma_s)
    if int(n_iter) != n_iter or n_iter < 0:
        raise ValueError('n_iter = %r: a whole number of sweeps, not negative' % (n_iter,))
    pts, fv = _device_mesh(points, faces, device)
    with torch.cuda.device(pts.device):
        V = pts.shape[0]
        rowptr, lst = meshprep.vertex_faces(fv, V)
        Np = _bilateral_normals(pts, fv, normal_iters, sigma_r, sigma_s, (rowptr, lst))
        dd = torch.nn.functional.normalize(pts, dim=1) if data_type in ('Kinect_v1', 'Kinect_v2') else None
        vf = meshprep.vf_padded32(rowptr, lst, V)
        Vu = update_position2(pts, fv, vf, Np, n_iter=int(n_iter), depth_direction=dd)
        out = {'Np': Np, 'V_updated': Vu, 'angle1': None, 'angle2': None}
        if gt_points is not None:
            gt = torch.as_tensor(np.asarray(gt_points) if not torch.is_tensor(gt_points) else gt_points)
            gt = gt.to(device=pts.device, dtype=torch.float32).contiguous()
            if gt.shape != pts.shape:
                raise ValueError('gt_points %s for points %s' % (tuple(gt.shape), tuple(pts.shape)))
            Nt = computer_face_normal(gt, fv)
            out['angle1'] = float(network.error_n(Np, Nt))
            out['angle2'] = float(network.error_n(computer_face_normal(Vu, fv), Nt))
    return out
