"""Plain fp64 torch statements of the two mesh regularisers of csrc/reg.hip -- the Laplacian term (the reference's
laplacian_loss, code/network.py:347-361) and the edge-length term -- with torch.autograd for the gradients and the
per-mesh weighting of a union batch, and the inputs of tests/test_gpu_reg.py.  The graph is the loop-free symmetric set
of directed entries (row, col) of a mesh's vertex graph, (row, col)-sorted: what the device CSR holds.  Anchored to the
reference's own function by tests/test_reg_model_host.py."""
import numpy as np
import torch

from geom_model import fan, mesh_weights, union     # noqa: F401  (the builders the tests use)


# ------------------------------------------------------------------------------ graph
def entries(faces, num_vertices):
    """Directed entries (row, col) int64 of the vertex graph of `faces`: both directions of every edge, no loops, sorted."""
    f = np.asarray(faces, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    e = e[e[:, 0] != e[:, 1]]
    key = np.unique(np.concatenate([e[:, 0] * num_vertices + e[:, 1], e[:, 1] * num_vertices + e[:, 0]]))
    return torch.from_numpy(key // num_vertices), torch.from_numpy(key % num_vertices)


def edge_index(faces, num_vertices, loops=True):
    """The COO [2, E] int64 a dataset hands over: the entries, then one self loop per vertex (dataset.py:211-213)."""
    row, col = entries(faces, num_vertices)
    if loops:
        ids = torch.arange(num_vertices)
        row, col = torch.cat([row, ids]), torch.cat([col, ids])
    return torch.stack([row, col])


# ------------------------------------------------------------------------------ the two terms
def lap(p, row, col, normal=None):
    """lap(p)_i = (1 / max(deg_i, 1)) sum_{j in N(i)} (p_i - p_j), projected on normal_i when given."""
    n = p.shape[0]
    deg = torch.bincount(row, minlength=n).clamp(min=1).to(p.dtype).unsqueeze(1)
    out = torch.zeros_like(p).index_add_(0, row, p[row] - p[col]) / deg
    return out if normal is None else normal * (out * normal).sum(1, keepdim=True)


def lap_difference(vp, v, row, col, normal=None):
    """d [V, 3] = lap(vp) - lap(v)."""
    return lap(vp, row, col, normal) - lap(v, row, col, normal)


def laplacian_term(vp, v, row, col, normal=None, w=None):
    """sum_i w_i sum_c |d_ic|; w None: 1 / V (the reference's mean)."""
    t = lap_difference(vp, v, row, col, normal).abs().sum(1)
    return t.mean() if w is None else (t * w).sum()


def edge_term(vp, v, row, col, w=None):
    """sum over the entries (i, j) of w_i (|vp_i - vp_j| - |v_i - v_j|)^2; w None: 1 / E; 0 without entries.  The norm's
    gradient at 0 is 0 (torch's subgradient): an entry whose predicted ends coincide gives a value and no gradient."""
    if row.numel() == 0:
        return vp.sum() * 0
    t = ((vp[row] - vp[col]).norm(dim=1) - (v[row] - v[col]).norm(dim=1)).pow(2)
    return t.mean() if w is None else (t * w[row]).sum()


def edge_weights(row, mesh_ptr, dtype=torch.float64):
    """Per-row 1 / (B * E_mesh) of a union batch cut by mesh_ptr [B + 1], E_mesh = the entries whose row lies in the
    mesh (0 for a mesh without entries)."""
    ptr = torch.as_tensor(mesh_ptr, dtype=torch.long)
    B = ptr.numel() - 1
    per_row = torch.bincount(row, minlength=int(ptr[-1]))
    out = torch.zeros(int(ptr[-1]), dtype=dtype)
    for a, b in zip(ptr[:-1].tolist(), ptr[1:].tolist()):
        e = int(per_row[a:b].sum())
        out[a:b] = 1.0 / (B * e) if e else 0.0
    return out


def both(vp, v, row, col, normal=None, w_lap=None, w_edge=None):
    """fp64 values and gradients to vp of the two terms on the given (fp32-valued) inputs
    -> (L_lap, L_edge, grad_lap [V, 3], grad_edge [V, 3], d [V, 3])."""
    d64 = lambda t: None if t is None else t.detach().double()
    v, normal, w_lap, w_edge = d64(v), d64(normal), d64(w_lap), d64(w_edge)
    p = vp.detach().double().requires_grad_(True)
    l_lap = laplacian_term(p, v, row, col, normal, w_lap)
    l_edge = edge_term(p, v, row, col, w_edge)
    g_lap, = torch.autograd.grad(l_lap, p)
    g_edge, = torch.autograd.grad(l_edge, p, allow_unused=True)
    g_edge = torch.zeros_like(p) if g_edge is None else g_edge
    return float(l_lap.detach()), float(l_edge.detach()), g_lap, g_edge, lap_difference(p.detach(), v, row, col, normal)


def undecided(d, row, col, rel=1e-5):
    """Vertices whose Laplacian gradient fp32 cannot be held to: the vertex, or a neighbour, has a component of d with
    magnitude below rel * max |d| -- the sign of that component is not decided in fp32.  -> bool [V]"""
    small = (d.abs() < rel * d.abs().max()).any(1)
    out = small.clone()
    out[row[small[col]]] = True
    return out


# ------------------------------------------------------------------------------ inputs
def rotation():
    """The orthogonal factor of a fixed random matrix: turned icospheres have no vertex normal component that is exactly 0."""
    return np.linalg.qr(np.random.default_rng(3).standard_normal((3, 3)))[0]


def sphere_input(n, s, seed=5, shift=None):
    """noisy_icosphere(n, s, seed) as prediction, its clean sphere as target and the clean sphere's vertex normals, all
    turned by rotation() (and moved by `shift`), rounded to fp32 -> (vp, v, normal) float32 tensors, faces int64 array."""
    from geobi_gnn_amd import meshgen
    noisy, clean, faces = meshgen.noisy_icosphere(n, s, seed=seed)
    q = rotation()
    nrm = meshgen.vertex_normals(clean.astype(np.float64), faces) @ q
    turn = lambda a: a.astype(np.float64) @ q + (0.0 if shift is None else np.asarray(shift, dtype=np.float64))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32)))
    return t(turn(noisy)), t(turn(clean)), t(nrm), faces
