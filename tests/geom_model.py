"""Plain torch statements of what csrc/geom.hip computes -- row losses and metrics, the face-geometry coupling, the two
heads -- and the mesh builders that reach the kernels' edges.  Dtype-agnostic: run in fp64 it is the reference of
tests/test_gpu_geom.py, run in fp32 it is the yardstick for what fp32 arithmetic can deliver on the same input.  The
vertex update is not restated: oracle.ref_model.update_position2 is the reference.  Anchored to the reference project's
own numbers by tests/test_geom_model_host.py."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_model as R

LEAK = 0.2
update_position2 = R.update_position2


# ------------------------------------------------------------------------------ losses and metrics
def row_terms(a, b, kind):
    """Per-row term [n] of kind 0 (L1), 1 (L2), 2 (Euclidean distance), 3 (angle in degrees, error_n's expression)."""
    if kind == 0:
        return (a - b).abs().sum(1)
    if kind == 1:
        return (a - b).pow(2).sum(1)
    if kind == 2:
        return (a - b).pow(2).sum(1).pow(0.5)
    if kind == 3:
        val = torch.clamp(1 - (a - b).pow(2).sum(1) / 2, min=-1, max=1)
        return torch.acos(val) * 180 / math.pi
    raise ValueError(kind)


def row_loss(a, b, w, kind, scale):
    """scale * sum_i w_i term(a_i, b_i); w None = all ones."""
    t = row_terms(a, b, kind)
    return (t if w is None else t * w).sum() * scale


def mesh_weights(mesh_ptr, dtype=torch.float64):
    """Per-row 1 / (B * n_mesh) of a union batch cut by mesh_ptr [B + 1] (parallel._mesh_weights)."""
    ptr = torch.as_tensor(mesh_ptr, dtype=torch.long)
    counts = ptr[1:] - ptr[:-1]
    return torch.repeat_interleave(1.0 / (counts.to(dtype) * counts.numel()), counts)


def unequal_ptr(n, parts):
    """mesh_ptr that cuts n rows into min(parts, n) non-empty meshes of unequal size (sizes ~ 1 : 2 : 3 : ...)."""
    parts = min(parts, n)
    if parts == 1:
        return [0, n]
    cum = np.cumsum(np.arange(1, parts + 1, dtype=np.float64))
    cuts = np.floor(cum[:-1] / cum[-1] * n).astype(np.int64)
    cuts = np.maximum(cuts, np.arange(1, parts))                  # every mesh keeps at least one row
    cuts = np.minimum(cuts, n - parts + np.arange(1, parts))
    return [0] + [int(c) for c in cuts] + [n]


# ------------------------------------------------------------------------------ face geometry and heads
def face_geom(verts, fv, xf):
    """x_f = cat(x_f[:, :6], centroid, unit normal) of the predicted vertices."""
    return torch.cat((xf[:, :6], verts[fv].mean(1), R.computer_face_normal(verts, fv)), 1)


def head(x, w1, b1, w2, b2, mode, dd=None, resid=None):
    """fc2(leaky_relu(fc1 x)); mode 0 (vertex head): (* dd if one output) + resid[:, :3]; mode 1 (face head): normalize."""
    y = F.linear(F.leaky_relu(F.linear(x, w1, b1), LEAK), w2, b2)
    if mode == 0:
        if w2.shape[0] == 1:
            y = y * dd
        return y + resid[:, :3]
    return F.normalize(y, dim=1)


# ------------------------------------------------------------------------------ mesh builders
def _f32_values(p):
    """float64 tensor holding float32-representable values: both precisions start from the same numbers."""
    return torch.as_tensor(np.asarray(p, dtype=np.float32).astype(np.float64))


def fan(valence, seed=0):
    """Closed triangle fan: hub 0 of the chosen valence, rim 1..valence (two faces each), and one isolated vertex (the
    last) that no face uses.  -> (points [valence + 2, 3] f64 with f32 values, faces [valence, 3] i64)."""
    assert valence >= 3
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * (np.arange(valence) + 0.3 * rng.uniform(-1, 1, valence)) / valence
    rad = 1.0 + 0.2 * rng.uniform(-1, 1, valence)
    rim = np.stack([rad * np.cos(ang), rad * np.sin(ang), 0.3 * rng.uniform(-1, 1, valence)], 1)
    pts = np.concatenate([[[0.05, -0.02, 0.6]], rim, [[2.5, -1.5, 0.75]]], 0)
    k = np.arange(valence)
    faces = np.stack([np.zeros(valence, dtype=np.int64), 1 + k, 1 + (k + 1) % valence], 1)
    return _f32_values(pts), torch.from_numpy(faces)


def union(meshes):
    """Disjoint union of (points, faces) meshes -> (points, faces, vertex mesh_ptr, face mesh_ptr)."""
    pts, faces, vptr, fptr = [], [], [0], [0]
    for p, f in meshes:
        pts.append(p)
        faces.append(f + vptr[-1])
        vptr.append(vptr[-1] + p.shape[0])
        fptr.append(fptr[-1] + f.shape[0])
    return torch.cat(pts), torch.cat(faces), torch.tensor(vptr), torch.tensor(fptr)


def vertex_faces(faces, num_vertices):
    """Padded vertex -> face table (-1 filled), as the dataset hands it to the vertex update."""
    from geobi_gnn_amd import meshgen
    return torch.from_numpy(meshgen.vertex_faces(faces.numpy(), num_vertices))


def sphere(n, sigma=0.2, seed=0):
    """Noisy icosphere of frequency n -> (points f64 with f32 values, faces i64)."""
    from geobi_gnn_amd import meshgen
    noisy, _, faces = meshgen.noisy_icosphere(n, sigma, seed)
    return _f32_values(noisy), torch.from_numpy(faces)


def degenerate_sphere(n=3, seed=1):
    """Small noisy icosphere in which three faces are degenerate EXACTLY: two repeat a vertex index ([a, a, b] and
    [c, c, c]: one edge vector is exactly zero) and the three vertices of the third are moved to the collinear integer
    points (0,0,0), (1,0,0), (2,0,0).  Every other face keeps a healthy area (asserted by the host test).
    -> (points, faces, ids of the degenerate faces)."""
    pts, faces = sphere(n, 0.2, seed)
    faces = faces.clone()
    used = set()
    picked = []
    for f in range(faces.shape[0]):              # three faces without a common vertex
        vs = set(faces[f].tolist())
        if not (vs & used):
            picked.append(f)
            used |= vs
        if len(picked) == 3:
            break
    rows = [faces[f].clone() for f in picked]
    faces[picked[0]] = torch.stack([rows[0][0], rows[0][0], rows[0][1]])
    faces[picked[1]] = torch.stack([rows[1][2], rows[1][2], rows[1][2]])
    pts = pts.clone()
    pts[rows[2]] = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0]], dtype=pts.dtype)
    return pts, faces, torch.tensor(picked)


def cross_lengths(pts, faces):
    tri = pts[faces]
    return torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1).norm(dim=1)


def perturbed_normals(pts, faces, seed=0, amount=0.3):
    """Unit face normals away from the geometric ones (what a network hands to the vertex update); zero-area faces get a
    random unit vector.  f64 tensor with f32 values."""
    g = torch.Generator().manual_seed(seed)
    n = R.computer_face_normal(pts, faces) + amount * torch.randn(faces.shape[0], 3, generator=g, dtype=pts.dtype)
    return _f32_values(F.normalize(n, dim=1).numpy())


def unit_depth(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return _f32_values(F.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=1).numpy())


# ------------------------------------------------------------------------------ inputs of the metric's edges
def rows_at_angles(theta_deg, seed=0):
    """Unit rows (a, b), f32 tensors, with the given angles between them: a = cos(t) b + sin(t) u, u unit, u . b = 0."""
    g = torch.Generator().manual_seed(seed)
    th = torch.as_tensor(theta_deg, dtype=torch.float64) * math.pi / 180
    b = F.normalize(torch.randn(th.shape[0], 3, generator=g, dtype=torch.float64), dim=1)
    r = torch.randn(th.shape[0], 3, generator=g, dtype=torch.float64)
    u = F.normalize(r - (r * b).sum(1, keepdim=True) * b, dim=1)
    a = th.cos()[:, None] * b + th.sin()[:, None] * u
    return a.float(), b.float()


def exact_unit_rows(n):
    """Rows of length exactly 1 in fp32 (signed coordinate axes), cycling."""
    axes = torch.tensor([[1.0, 0, 0], [0, -1.0, 0], [0, 0, 1.0], [-1.0, 0, 0], [0, 1.0, 0], [0, 0, -1.0]])
    return axes[torch.arange(n) % 6].contiguous()
