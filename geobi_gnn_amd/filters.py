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

Guided normal filtering (Zhang, Deng, Zhang, Bouaziz, Liu, "Guided Mesh Normal Filtering", Pacific Graphics 2015;
`denoise --method gnf`, csrc/guided.hip) is the same sweep with the range weight measured on a guidance normal g instead of
the noisy normal, which is what keeps an edge at high noise.  With the patch P_k = N(k) and an "edge pair" a pair of
different faces that share at least 2 distinct vertex ids, every sweep makes from the current normals n

    Phi_k = max_{j, m in P_k} |n_j - n_m|
    R_k   = max |n_j - n_m| / (1e-9 + sum |n_j - n_m|) over the edge pairs with both faces in P_k (0 without one)
    H_k   = Phi_k R_k,   sel_i = argmin_{k in N(i)} H_k (ties: the lowest index) -- the patches that contain i
    g_i   = normalised sum_{j in P_sel_i} A_j n_j (n_i when that sum has no length)
    w_ij  = A_j exp(-|c_i - c_j|^2 / (2 sigma_s^2) - |g_i - g_j|^2 / (2 sigma_r^2)),  then s_i, W_i, n_i' as above

The patch search costs sum_k |P_k|^2 normal comparisons per sweep; a call whose sum x sweeps exceeds GNF_COST_BUDGET is
refused before the first kernel of the filter runs.
"""
import torch

from . import _lib as L
from . import meshin, meshprep
from .data_util import denoise_tail


# Normal comparisons (sum_k |P_k|^2 x sweeps) one guided call may ask for: about one second of gnf_measure_kernel at the
# 1.0e11 per second it was measured to sustain on its slowest shape, a fan of valence 2048 whose every patch is the whole
# fan; on spheres it does 3 to 4.5e11 per second (profiles/filter_gnf.txt).
GNF_COST_BUDGET = 1.0e11


def _check_params(normal_iters, sigma_r, sigma_s):
    if int(normal_iters) != normal_iters or normal_iters < 0:
        raise ValueError('normal_iters = %r: a whole number of sweeps, not negative' % (normal_iters,))
    for name, v in (('sigma_r', sigma_r), ('sigma_s', sigma_s)):
        if not (float(v) > 0.0 and float(v) < float('inf')):
            raise ValueError('%s = %r: positive and finite' % (name, v))


def _nonempty_mesh(points, faces, device):
    """meshin.device_mesh; the filters refuse a mesh without faces."""
    pts, fv = meshin.device_mesh(points, faces, device)
    if fv.shape[0] == 0:
        raise ValueError('the mesh has no faces')
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
    s = meshprep.mean_edge_length(meshprep.face_normals_centroids(points, fv)[1], graph) * float(sigma_s)
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
    pts, fv = _nonempty_mesh(points, faces, None)
    with torch.cuda.device(pts.device):
        return _bilateral_normals(pts, fv, normal_iters, sigma_r, sigma_s, incidence)


def bilateral_denoise(points, faces, normal_iters=20, sigma_r=0.35, sigma_s=1.0, n_iter=20, data_type='Synthetic',
                      gt_points=None, device=None):
    """Bilateral normal filtering, then `n_iter` sweeps of the vertex update towards the filtered normals.
    -> dict(Np, V_updated, angle1, angle2) with the meaning of patches.predict_mesh's keys: Np the filtered normals,
    V_updated the moved vertices; with gt_points, angle1 = mean angle (degrees) of Np against the ground truth's face
    normals, angle2 = that of the updated mesh's normals (None without).  Kinect data types move vertices along
    normalize(points) only, as predict_mesh does."""
    return _denoise(_bilateral_normals, points, faces, normal_iters, sigma_r, sigma_s, n_iter, data_type, gt_points, device)


def _denoise(normals_fn, points, faces, normal_iters, sigma_r, sigma_s, n_iter, data_type, gt_points, device):
    _check_params(normal_iters, sigma_r, sigma_s)
    if int(n_iter) != n_iter or n_iter < 0:
        raise ValueError('n_iter = %r: a whole number of sweeps, not negative' % (n_iter,))
    pts, fv = _nonempty_mesh(points, faces, device)
    with torch.cuda.device(pts.device):
        V = pts.shape[0]
        rowptr, lst = meshprep.vertex_faces(fv, V)
        Np = normals_fn(pts, fv, normal_iters, sigma_r, sigma_s, (rowptr, lst))
        vf = meshprep.vf_padded32(rowptr, lst, V)
        Vu, angle1, angle2 = denoise_tail(pts, fv, vf, Np, int(n_iter), data_type, gt_points)
        out = {'Np': Np, 'V_updated': Vu, 'angle1': None if angle1 is None else float(angle1),
               'angle2': None if angle2 is None else float(angle2)}
    return out


# ------------------------------------------------------------------------------------------------ guided normal filter
def edge_flags(fv, graph):
    """geobi_gnf_edge_flags: uint8 [E], 1 where the two faces of the CSR entry share at least 2 distinct vertex ids."""
    flags = torch.empty(max(graph.E, 1), dtype=torch.uint8, device=fv.device)
    L.call('geobi_gnf_edge_flags', L.ptr(fv), L.ptr(graph.rowptr_out), L.ptr(graph.col_out), fv.shape[0], graph.E,
           L.ptr(flags), L.stream())
    return flags[:graph.E]


def patch_measure(rec_c, normals, graph, flags):
    """geobi_gnf_patch_measure: H [F] of the normals [F,4] (rows of rec_n's layout)."""
    F = rec_c.shape[0]
    H = torch.empty(F, dtype=torch.float32, device=rec_c.device)
    L.call('geobi_gnf_patch_measure', L.ptr(rec_c), L.ptr(normals), L.ptr(graph.rowptr_out), L.ptr(graph.col_out),
           L.ptr(flags), F, graph.E, L.ptr(H), L.stream())
    return H


def patch_cost(graph, F):
    """sum_k (deg_k + 1)^2, the normal comparisons of one patch search: summed on the device, one host read."""
    deg = (graph.rowptr_out[1:F + 1] - graph.rowptr_out[:F]).long() + 1
    total = (deg * deg).sum()
    lo, hi = L.read_i32(torch.stack([total & 0x7fffffff, total >> 31]).to(torch.int32))
    return (hi << 31) | lo


def _check_cost(graph, F, n_sweeps):
    cost = patch_cost(graph, F) * max(int(n_sweeps), 1)
    if cost > GNF_COST_BUDGET:
        raise L.GeobiError('guided filter: the patch search would take %d normal comparisons (sum of squared patch sizes '
                           'x %d sweeps), the budget is %d: a vertex of very high valence; use the bilateral filter'
                           % (cost, max(int(n_sweeps), 1), int(GNF_COST_BUDGET)))


def guided_records(rec_c, rec_n, fv, graph, inv2ss, sigma_r, n_sweeps, return_selection=False):
    """geobi_gnf_filter: `n_sweeps` sweeps starting from the normals in rec_n -> [F,4] rows of rec_n's layout; with
    return_selection also every sweep's selection, int32 [n_sweeps, F]."""
    F = rec_c.shape[0]
    out = torch.empty_like(rec_n)
    sel = torch.empty((int(n_sweeps), F), dtype=torch.int32, device=rec_c.device) if return_selection else None
    ws = L.workspace(L.size_query('geobi_gnf_filter_ws_bytes', F, graph.E), rec_c.device)
    L.call('geobi_gnf_filter', L.ptr(rec_c), L.ptr(rec_n), L.ptr(fv), L.ptr(graph.rowptr_out), L.ptr(graph.col_out), F,
           graph.E, L.ptr(inv2ss), 0.5 / (float(sigma_r) * float(sigma_r)), int(n_sweeps), L.ptr(out),
           L.ptr(sel) if sel is not None and sel.numel() else None, L.ptr(ws), ws.numel(), L.stream())
    return (out, sel) if return_selection else out


def _guided_normals(pts, fv, normal_iters, sigma_r, sigma_s, incidence, return_selection=False):
    rowptr, lst = incidence if incidence is not None else meshprep.vertex_faces(fv, pts.shape[0])
    graph = meshprep.ring_graph(1, fv, rowptr, lst, fv.shape[0])
    _check_cost(graph, fv.shape[0], normal_iters)
    rec_c, rec_n = face_records(pts, fv)
    inv2ss = spatial_scale(pts, fv, graph, sigma_s)
    r = guided_records(rec_c, rec_n, fv, graph, inv2ss, sigma_r, int(normal_iters), return_selection)
    if return_selection:
        return r[0][:, :3].contiguous(), r[1]
    return r[:, :3].contiguous()


def guided_normals(points, faces, normal_iters=20, sigma_r=0.35, sigma_s=1.0, incidence=None, return_selection=False):
    """Guided-filtered unit face normals [F,3] (fp32, on the device) of the mesh (points [V,3], faces [F,3]).
    incidence: (rowptr, list) of meshprep.vertex_faces for these faces, if the caller has it already.
    normal_iters = 0 returns the start normals.  return_selection: -> (normals, int32 [normal_iters, F]: the patch every
    face took its guidance from, per sweep)."""
    _check_params(normal_iters, sigma_r, sigma_s)
    pts, fv = _nonempty_mesh(points, faces, None)
    with torch.cuda.device(pts.device):
        return _guided_normals(pts, fv, normal_iters, sigma_r, sigma_s, incidence, return_selection)


def guided_denoise(points, faces, normal_iters=20, sigma_r=0.35, sigma_s=1.0, n_iter=20, data_type='Synthetic',
                   gt_points=None, device=None):
    """Guided normal filtering, then `n_iter` sweeps of the vertex update: bilateral_denoise's arguments and result."""
    return _denoise(_guided_normals, points, faces, normal_iters, sigma_r, sigma_s, n_iter, data_type, gt_points, device)
