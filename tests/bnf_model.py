"""Plain torch statement of the bilateral normal filter (geobi_gnn_amd/filters.py, csrc/filter.hip) on the CPU.
Dtype-agnostic: run in fp64 it is the reference of tests/test_gpu_filter.py, run in fp32 it is the yardstick for what fp32
arithmetic delivers on the same input.  Anchored by tests/test_bnf_model_host.py.

    cr_i = (b - a) x (c - a),  A_i = |cr_i| / 2,  c_i = centroid,  n_i^0 = cr_i / max(|cr_i|, 1e-12)
    N(i)    = faces sharing a vertex with i, i included (meshgen.facet_graph_index: its self loops are the j = i term)
    sigma_s = sigma_s-argument x mean |c_i - c_j| over the loop-free edges;  a = 1 / (2 sigma_s^2), 0 without an edge (or
              without a distance);  b = 1 / (2 sigma_r^2)
    sweep:    w_ij = A_j exp(-a |c_i - c_j|^2 - b |n_i - n_j|^2),  s_i = sum_j w_ij n_j,  W_i = sum_j w_ij
              n_i' = s_i / |s_i| if |s_i| > 1e-6 W_i, else n_i                                   (Jacobi)
"""
import numpy as np
import torch

from geobi_gnn_amd import meshgen


def facet_coo(faces, num_vertices):
    """(row, col) int64 tensors of the facet graph with its self loops, (row, col)-sorted."""
    f = np.asarray(faces, dtype=np.int64)
    ei = meshgen.facet_graph_index(f, meshgen.vertex_faces(f, int(num_vertices)))
    return torch.from_numpy(ei[0].astype(np.int64)), torch.from_numpy(ei[1].astype(np.int64))


def face_records(points, faces):
    """-> (centroid [F,3], area [F], start normal [F,3]) in the dtype of points."""
    tri = points[faces]
    cr = torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1)
    ln = cr.norm(dim=1)
    return tri.mean(1), ln / 2, cr / ln.clamp(min=1e-12)[:, None]


def spatial_scale(cen, row, col, sigma_s):
    """a = 1 / (2 sigma_s^2) as a 0-dim tensor of cen's dtype; 0 when no edge (or no distance) is there."""
    off = row != col
    if not bool(off.any()):
        return torch.zeros((), dtype=cen.dtype)
    s = (cen[row[off]] - cen[col[off]]).norm(dim=1).mean() * sigma_s
    return 0.5 / (s * s) if float(s) > 0 else torch.zeros((), dtype=cen.dtype)


def sweep(n, cen, area, row, col, a, b):
    F = n.shape[0]
    d2 = (cen[row] - cen[col]).pow(2).sum(1)
    dn2 = (n[row] - n[col]).pow(2).sum(1)
    w = area[col] * torch.exp(-a * d2 - b * dn2)
    s = torch.zeros_like(n).index_add_(0, row, w[:, None] * n[col])
    W = torch.zeros_like(area).index_add_(0, row, w)
    ln = s.norm(dim=1)
    ok = ln > 1e-6 * W
    return torch.where(ok[:, None], s / ln.clamp(min=1e-300 if n.dtype == torch.float64 else 1e-38)[:, None], n)


def bilateral_normals(points, faces, normal_iters=20, sigma_r=0.35, sigma_s=1.0, start=None, history=False):
    """points [V,3] (fp64 or fp32), faces [F,3] int64 -> filtered normals [F,3]; history: the list after 0, 1, ... sweeps.
    start: normals to begin with instead of n^0."""
    faces = torch.as_tensor(faces, dtype=torch.long)
    row, col = facet_coo(faces.numpy(), points.shape[0])
    cen, area, n = face_records(points, faces)
    if start is not None:
        n = start.to(points.dtype)
    a = spatial_scale(cen, row, col, sigma_s)
    b = 0.5 / (sigma_r * sigma_r)
    out = [n]
    for _ in range(int(normal_iters)):
        n = sweep(n, cen, area, row, col, a, b)
        out.append(n)
    return out if history else n


def mean_angle_deg(a, b):
    """Mean angle in degrees between the rows of a and b (unit rows)."""
    cos = (a * b).sum(1).clamp(-1, 1)
    return float(torch.rad2deg(torch.acos(cos)).mean())
