"""Plain torch statement of the guided normal filter (geobi_gnn_amd/filters.py, csrc/guided.hip) on the CPU.
Dtype-agnostic: run in fp64 it is the reference of tests/test_gpu_gnf.py, run in fp32 it is the yardstick for what fp32
arithmetic delivers on the same input.  Anchored by tests/test_gnf_model_host.py.  Built on bnf_model.facet_coo and
bnf_model.face_records; meant for test-sized meshes (it keeps a dense F x F table of edge pairs).

    cr_i, A_i, c_i, n_i^0, the facet graph, a = 1 / (2 sigma_s^2): bnf_model's;  b = 1 / (2 sigma_r^2)
    patch       P_k = faces sharing a vertex with k, k included (row k of facet_coo, ascending)
    edge pair   {j, m}, j != m, whose sets of distinct vertex ids have at least 2 ids in common
    measures    Phi_k = max_{j, m in P_k} |n_j - n_m|;  over the edge pairs with both faces in P_k:
                R_k = max |n_j - n_m| / (1e-9 + sum |n_j - n_m|), 0 without one;  H_k = Phi_k R_k
    selection   sel_i = argmin_{k in P_i} H_k, ties to the lowest index
    guidance    s = sum_{j in P_sel_i} A_j n_j;  g_i = s / |s| if |s| > 1e-6 sum A_j, else n_i
    sweep       w_ij = A_j exp(-a |c_i - c_j|^2 - b |g_i - g_j|^2) over j in P_i,  s_i = sum w_ij n_j,  W_i = sum w_ij,
                n_i' = s_i / |s_i| if |s_i| > 1e-6 W_i, else n_i                                         (Jacobi)

Everything is vectorised over rows padded to the longest patch.  The sum of R_k adds its terms in ascending order of value,
so two patches with the same terms get the same bits whatever places the terms have in the rows: a tie of congruent
patches is an exact tie.
"""
import numpy as np
import torch

import bnf_model as B

_CHUNK = 1 << 21            # elements of a [faces, Pmax, Pmax] block worked on at once


class Topology(object):
    """What depends on the face table alone: the COO with self loops, the padded patches and the edge pairs."""

    def __init__(self, faces, num_vertices):
        faces = torch.as_tensor(faces, dtype=torch.long)
        self.faces, self.F = faces, faces.shape[0]
        self.row, self.col = B.facet_coo(faces.numpy(), num_vertices)
        F = self.F
        count = torch.bincount(self.row, minlength=F)
        start = torch.cumsum(count, 0) - count
        self.pmax = int(count.max())
        slot = torch.arange(self.row.shape[0]) - start[self.row]
        self.patch = torch.full((F, self.pmax), -1, dtype=torch.long)          # ascending face ids, -1 padded
        self.patch[self.row, slot] = self.col
        self.valid = self.patch >= 0
        self.safe = self.patch.clamp(min=0)
        self.coo_flags = edge_pair_flags(faces, self.row, self.col)            # per COO entry, loops (False) included
        self.pairs = torch.zeros((F, F), dtype=torch.bool)
        self.pairs[self.row, self.col] = self.coo_flags

    def csr_flags(self):
        """The flags in the order of the loop-free CSR the device walks (uint8)."""
        return self.coo_flags[self.row != self.col].to(torch.uint8)


def edge_pair_flags(faces, row, col):
    """True per (row, col) entry when the two DIFFERENT faces share at least 2 distinct vertex ids."""
    a, b = faces[row], faces[col]
    new = torch.stack([torch.ones_like(a[:, 0], dtype=torch.bool), a[:, 1] != a[:, 0],
                       (a[:, 2] != a[:, 0]) & (a[:, 2] != a[:, 1])], 1)
    inb = (a[:, :, None] == b[:, None, :]).any(2)
    return ((new & inb).sum(1) >= 2) & (row != col)


def patch_measure(n, topo):
    """H [F] of the normals n [F,3] (in n's dtype)."""
    F, pm = topo.F, topo.pmax
    H = torch.zeros(F, dtype=n.dtype)
    upper = torch.triu(torch.ones((pm, pm), dtype=torch.bool), diagonal=1)
    step = max(1, _CHUNK // (pm * pm))
    for lo in range(0, F, step):
        P, ok = topo.safe[lo:lo + step], topo.valid[lo:lo + step]
        N = n[P]                                                               # [f, pm, 3]
        d = (N[:, :, None, :] - N[:, None, :, :]).pow(2).sum(3).sqrt()         # [f, pm, pm]
        both = ok[:, :, None] & ok[:, None, :]
        phi = torch.where(both, d, torch.zeros_like(d)).flatten(1).max(1).values
        edge = both & upper & topo.pairs[P[:, :, None], P[:, None, :]]
        phi_e = torch.where(edge, d, torch.zeros_like(d)).flatten(1)
        emax = phi_e.max(1).values
        esum = phi_e.sort(1).values.sum(1)                                     # ascending: the same terms, the same bits
        H[lo:lo + step] = phi * (emax / (1e-9 + esum))
    return H


def select(H, topo):
    """sel [F]: the patch of least H among those that contain the face, the lowest index among equals."""
    Hrow = torch.where(topo.valid, H[topo.safe], torch.full((), float('inf'), dtype=H.dtype))
    least = Hrow.min(1, keepdim=True).values
    big = torch.full_like(topo.patch, topo.F)
    return torch.where(Hrow == least, topo.patch, big).min(1).values


def guidance(n, area, sel, topo):
    P, ok = topo.safe[sel], topo.valid[sel]
    w = torch.where(ok, area[P], torch.zeros((), dtype=n.dtype))
    s = (w[:, :, None] * n[P]).sum(1)
    ln = s.norm(dim=1)
    keep = ln > 1e-6 * w.sum(1)
    tiny = 1e-300 if n.dtype == torch.float64 else 1e-38
    return torch.where(keep[:, None], s / ln.clamp(min=tiny)[:, None], n)


def sweep(n, g, cen, area, row, col, a, b):
    d2 = (cen[row] - cen[col]).pow(2).sum(1)
    dg2 = (g[row] - g[col]).pow(2).sum(1)
    w = area[col] * torch.exp(-a * d2 - b * dg2)
    s = torch.zeros_like(n).index_add_(0, row, w[:, None] * n[col])
    W = torch.zeros_like(area).index_add_(0, row, w)
    ln = s.norm(dim=1)
    ok = ln > 1e-6 * W
    return torch.where(ok[:, None], s / ln.clamp(min=1e-300 if n.dtype == torch.float64 else 1e-38)[:, None], n)


class Filter(object):
    """The filter one sweep at a time: .n are the current normals; step(selection) makes H and g from them and sweeps."""

    def __init__(self, points, faces, sigma_r=0.35, sigma_s=1.0, start=None, topo=None):
        faces = torch.as_tensor(faces, dtype=torch.long)
        self.topo = topo if topo is not None else Topology(faces, points.shape[0])
        self.cen, self.area, n = B.face_records(points, faces)
        self.n = n if start is None else start.to(points.dtype)
        self.a = B.spatial_scale(self.cen, self.topo.row, self.topo.col, sigma_s)
        self.b = 0.5 / (sigma_r * sigma_r)

    def measure(self):
        return patch_measure(self.n, self.topo)

    def step(self, selection=None):
        """One sweep; selection: sel [F] to replay instead of the filter's own.  -> the selection used."""
        sel = select(self.measure(), self.topo) if selection is None else torch.as_tensor(selection, dtype=torch.long)
        g = guidance(self.n, self.area, sel, self.topo)
        self.n = sweep(self.n, g, self.cen, self.area, self.topo.row, self.topo.col, self.a, self.b)
        return sel


def guided_normals(points, faces, normal_iters=20, sigma_r=0.35, sigma_s=1.0, start=None, history=False, selection=None,
                   return_selection=False, topo=None):
    """points [V,3] (fp64 or fp32), faces [F,3] -> filtered normals [F,3]; history: the list after 0, 1, ... sweeps.
    selection: [normal_iters, F] selections to replay (sweep t uses row t) instead of the filter's own.
    return_selection: -> (normals or history, [normal_iters, F] selections used)."""
    f = Filter(points, faces, sigma_r, sigma_s, start, topo)
    out, sels = [f.n], []
    for t in range(int(normal_iters)):
        sels.append(f.step(None if selection is None else selection[t]))
        out.append(f.n)
    res = out if history else f.n
    if return_selection:
        return res, (torch.stack(sels) if sels else torch.zeros((0, f.topo.F), dtype=torch.long))
    return res


# ------------------------------------------------------------------------------------------------ mesh builders
def cube(k):
    """Unit cube, k x k quads per side (two triangles each, outward), welded: 6 k^2 + 2 vertices, 12 k^2 faces.
    -> (points f64 -- multiples of 1/k: exact in fp32 for k a power of two --, faces i64)."""
    ids, pts, faces = {}, [], []

    def vid(p):
        key = tuple(int(round(v)) for v in p)
        if key not in ids:
            ids[key] = len(pts)
            pts.append([v / k for v in key])
        return ids[key]

    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, 1):
            for i in range(k):
                for j in range(k):
                    quad = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[u], p[v] = side * k, i + di, j + dj
                        quad.append(vid(p))
                    if side == 0:
                        quad.reverse()
                    faces += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    return torch.tensor(pts, dtype=torch.float64), torch.tensor(faces)


def noisy_cube(k, sigma, seed):
    """cube(k) with gaussian vertex noise of standard deviation sigma x the grid spacing -> (noisy f64 with f32 values,
    clean, faces)."""
    clean, faces = cube(k)
    rng = np.random.default_rng(seed)
    noisy = clean.numpy() + rng.normal(0.0, sigma / k, clean.shape)
    return torch.from_numpy(noisy.astype(np.float32).astype(np.float64)), clean, faces


def three_on_an_edge():
    """Three triangles on the edge 0-1 (a non-manifold edge) plus one that touches vertex 2 only."""
    pts = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 1.0, 0.0], [0.5, -0.5, 1.0], [0.5, -0.75, -0.5],
                        [1.5, 1.25, 0.5], [0.25, 2.0, 0.25]], dtype=torch.float64)
    return pts, torch.tensor([[0, 1, 2], [1, 0, 3], [0, 1, 4], [2, 5, 6]])
