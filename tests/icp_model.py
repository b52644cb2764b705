"""Rigid point-to-point ICP as the library specifies it (include/geobi_hip.h), written in numpy fp64 with
numpy.linalg.svd, and the inputs it is checked on.  Shared by tests/test_icp_model_host.py and tests/test_gpu_icp.py.

Convention: xt = s * x @ R + T, row vectors.  One iteration: idx = nearest row of y to every row of the current xt
(lowest index among equals); Umeyama alignment of the ORIGINAL x to y[idx]; xt = float32(s x R + T), rounded once as the
device does; rmse from the fp64 values before rounding.  The model records, per iteration, what the GPU tests condition
their comparisons on: idx, the relative gap between the best and the second-best squared distance of every row, the
relative change of rmse, and the singular-value gap (S1 + d S2) / S0 of the covariance, d = the sign the rotation's last
axis got -- the quantity that conditions R (a perturbation e of C turns R by about e / (S1 + d S2))."""
import numpy as np

from chamfer_model import _argmin64


# ------------------------------------------------------------------------------------------------ the algorithm
def umeyama(x, yy, estimate_scale=False, allow_reflection=False):
    """-> R [3,3], T [3], s, rmse, gap, smin_over_smax: x [Q,3] onto yy [Q,3] (row i to row i), fp64."""
    x, yy = np.asarray(x, np.float64), np.asarray(yy, np.float64)
    Q = len(x)
    mux, muy = x.mean(0), yy.mean(0)
    xc, yc = x - mux, yy - muy
    C = xc.T @ yc / Q
    U, S, Vt = np.linalg.svd(C)
    E = np.ones(3)
    if not allow_reflection and np.linalg.det(U @ Vt) < 0:
        E[2] = -1.0
    R = (U * E) @ Vt
    var = (xc ** 2).sum() / Q
    s = float((S * E).sum() / var) if estimate_scale and var > 0 else 1.0
    T = muy - s * mux @ R
    res = s * x @ R + T - yy
    rmse = float(np.sqrt((res ** 2).sum() / Q))
    gap = float((S[1] + E[2] * S[2]) / S[0]) if S[0] > 0 else 0.0
    return R, T, s, rmse, gap, (float(S[2] / S[0]) if S[0] > 0 else 0.0)


def transform(x, R, T, s):
    return s * np.asarray(x, np.float64) @ R + T


def step(x, y, idx, estimate_scale=False, allow_reflection=False):
    """geobi_icp_step of one part, without the convergence bookkeeping -> dict(R, T, s, rmse, gap, sratio, xt float32)."""
    R, T, s, rmse, gap, sratio = umeyama(x, np.asarray(y, np.float64)[idx], estimate_scale, allow_reflection)
    return {'R': R, 'T': T, 's': s, 'rmse': rmse, 'gap': gap, 'sratio': sratio,
            'xt': transform(x, R, T, s).astype(np.float32)}


def icp(x, y, init=None, max_iterations=100, relative_rmse_thr=1e-6, estimate_scale=False, allow_reflection=False):
    """The whole loop on one part.  -> dict: R, T, s, rmse, iterations, converged, xt (float32), and `trace`: one dict per
    iteration with idx, nn_gap [Q], rel (None at iteration 1), gap, same_idx (idx equals the iteration before's)."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    R, T, s = (np.eye(3), np.zeros(3), 1.0) if init is None else init
    xt = transform(x, R, T, s).astype(np.float32)
    out = {'R': R, 'T': T, 's': s, 'rmse': 0.0, 'iterations': 0, 'converged': False, 'trace': []}
    prev, prev_idx = 0.0, None
    for k in range(1, max_iterations + 1):
        idx, _, nn_gap = _argmin64(xt, y)
        st = step(x, y, idx, estimate_scale, allow_reflection)
        xt = st['xt']
        compare = k >= 2 and prev > 0
        rel = (prev - st['rmse']) / prev if compare else None
        out['trace'].append({'idx': idx, 'nn_gap': nn_gap, 'rel': rel, 'gap': st['gap'],
                             'same_idx': prev_idx is not None and np.array_equal(idx, prev_idx)})
        out.update(R=st['R'], T=st['T'], s=st['s'], rmse=st['rmse'], iterations=k)
        prev, prev_idx = st['rmse'], idx
        if (compare and rel <= relative_rmse_thr) or st['rmse'] == 0:
            out['converged'] = True
            break
    out['xt'] = xt
    return out


# ------------------------------------------------------------------------------------------------ inputs
def rotation(axis, degrees):
    """Rodrigues: the matrix R of the row-vector convention x @ R that turns by `degrees` about `axis`."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(degrees)
    return (np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K).T


def rotation_angle(R):
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))))


_BUMPY = {}


def bumpy(n):
    """meshgen.icosphere(n) with a smooth radial factor that has no symmetry (the plain sphere fits every rotation):
    r = 1 + 0.25 sin(3x + 1) cos(2y) + 0.15 z^3 + 0.1 xy.  -> points float32 [V,3], faces int64 [F,3]."""
    if n not in _BUMPY:
        from geobi_gnn_amd import meshgen
        p, faces = meshgen.icosphere(n)
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        r = 1 + 0.25 * np.sin(3 * x + 1) * np.cos(2 * y) + 0.15 * z ** 3 + 0.1 * x * y
        _BUMPY[n] = ((p * r[:, None]).astype(np.float32), faces)
    return _BUMPY[n]


def pose(points, axis=(1, 2, 3), degrees=10.0, translation=0.05, scale=1.0):
    """The float32 points moved by the pose: p -> scale * p @ R + t, t = translation * (1, -1, 0.5)."""
    R = rotation(axis, degrees)
    t = translation * np.array([1.0, -1.0, 0.5])
    return (scale * np.asarray(points, np.float64) @ R + t).astype(np.float32), R, t


# (n, degrees, translation, scale, estimate_scale, recovers the true pose)
LOOP_INPUTS = ((4, 10.0, 0.05, 1.0, False, True), (8, 5.0, 0.02, 1.2, True, True),
               (8, 10.0, 0.05, 1.0, False, False), (16, 5.0, 0.02, 1.0, False, False))
_LOOP = {}


def loop_input(k):
    """-> x (the posed copy: what is aligned), y (the bumpy sphere), R_true, T_true, s_true of x -> y, estimate_scale."""
    if k not in _LOOP:
        n, deg, tr, sc, est, _ = LOOP_INPUTS[k]
        y, _ = bumpy(n)
        x, R, t = pose(y, degrees=deg, translation=tr, scale=sc)
        # x = sc y R + t  =>  y = (1 / sc) x R^T - (1 / sc) t R^T
        _LOOP[k] = (x, y, R.T, -(t @ R.T) / sc, 1.0 / sc, est)
    return _LOOP[k]


_LOOP_RUN = {}


def loop_model(k):
    if k not in _LOOP_RUN:
        x, y, _, _, _, est = loop_input(k)
        _LOOP_RUN[k] = icp(x, y, estimate_scale=est)
    return _LOOP_RUN[k]


def injected(Q, M=None, seed=0, offset=0.0, noise=0.05):
    """x [Q,3], y [M,3] float32 and a RANDOM idx [Q] (not searched): y[idx[i]] is a posed x[i] plus noise where no later
    row overwrote it, so the covariance is well conditioned although the correspondence is arbitrary."""
    M = Q if M is None else M
    rng = np.random.default_rng(1000 + seed)
    x = (rng.uniform(-0.5, 0.5, (Q, 3)) * np.array([1.0, 0.7, 0.4]) + offset).astype(np.float32)
    idx = rng.integers(0, M, Q)
    R = rotation((2, -1, 1), 25.0)
    y = rng.uniform(-0.5, 0.5, (M, 3)) + offset
    y[idx] = 1.1 * (x.astype(np.float64) - offset) @ R + offset + 0.1 + noise * rng.standard_normal((Q, 3))
    return x, y.astype(np.float32), idx.astype(np.int32)


# ------------------------------------------------------------------------------------------------ eval_free
def eval_free64(pr, fr, po, fo):
    """mesheval.eval_free in fp64 from the float32 inputs, with the numpy statements of the mesheval tests -> (dict,
    nearest ground-truth face of every result centroid, its relative gap to the second-nearest face)."""
    from test_gpu_mesheval import _mean_edge, _tri_dist_fp64
    pr, po = np.asarray(pr, np.float64), np.asarray(po, np.float64)

    def normals(p, f):
        n = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
        return n / np.linalg.norm(n, axis=1, keepdims=True)

    def surface(q, verts, faces, chunk=64):
        a, b, c = verts[faces[:, 0]][None], verts[faces[:, 1]][None], verts[faces[:, 2]][None]
        dist, face, gap = np.empty(len(q)), np.empty(len(q), np.int64), np.empty(len(q))
        for i in range(0, len(q), chunk):
            d = _tri_dist_fp64(q[i:i + chunk, None, :], a, b, c)
            face[i:i + chunk] = d.argmin(1)
            two = np.partition(d, 1, axis=1)[:, :2]
            dist[i:i + chunk] = two[:, 0]
            gap[i:i + chunk] = (two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], 1e-300)
        return dist, face, gap
    nr, no = normals(pr, fr), normals(po, fo)
    cent = (pr[fr[:, 0]] + pr[fr[:, 1]] + pr[fr[:, 2]]) / 3
    _, face, gap = surface(cent, po, fo)
    err = ((nr - no[face]) ** 2).sum(1)
    ang = np.arccos(np.clip(1 - err / 2, -1, 1)) * 180 / np.pi
    d_ro, _, _ = surface(pr, po, fo)
    d_or, _, _ = surface(po, pr, fr)
    scale = _mean_edge(po, fo)
    return ({'num_f': len(fr), 'num_v': len(pr), 'num_f_gt': len(fo), 'num_v_gt': len(po), 'angle': ang.mean(),
             'surf': d_ro.mean(), 'surf_back': d_or.mean(), 'hausdorff': max(d_ro.max(), d_or.max()), 'scale': scale,
             'surf_norm': d_ro.mean() / scale, 'surf_back_norm': d_or.mean() / scale}, face, gap)
