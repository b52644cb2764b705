"""Scoring a denoised mesh against its ground truth: data_util.eval_denoising_result
(code/data_util.py:559-638) with its vertex metric on the MI355X.

The reference computes, per vertex of the result, the distance to the nearest ground-truth vertex by brute force on
CPU threads (code/my_hausdorff.py) and keeps the point-to-surface form commented out beside it (p2m, :601-603).  Both
are all-pairs HIP kernels here (csrc/dist.hip: geobi_nearest_point, geobi_nearest_triangle); sums and maxima are
reduced in fp64 on the device (geobi_dist_summary), and one read brings a pair's numbers to the host.
"""
import os

import torch

from . import _lib as L
from . import folders, meshgrid, meshin, meshio, meshnoise, meshprep, network, ops
from .data_util import computer_face_normal, face_centroids


def _points(t, what):
    L.require_device(t, what)
    t = t.detach().to(torch.float32).contiguous()
    if t.dim() != 2 or t.shape[1] != 3:
        raise L.GeobiError('%s must be [n, 3], got %s' % (what, tuple(t.shape)))
    return t


def _nearest_ws(Q, T, dev):
    return L.workspace(L.size_query('geobi_nearest_ws_bytes', Q, T), dev)


def nearest_point(a, b, index=None):
    """my_hausdorff.nearest_distance(a, b): for every row of a [Q, 3] the distance to the nearest row of b [T, 3] and
    that row's index (the lowest among equally near ones) -> (dist float32 [Q], idx int32 [Q]).  index: None walks all
    pairs; 'grid' builds a meshgrid.PointGrid over b first, a PointGrid built over b before is used as it is -- the same
    bits either way."""
    index = meshgrid.check_index(index)
    a, b = _points(a, 'query points'), _points(b, 'target points')
    Q, T = a.shape[0], b.shape[0]
    if Q == 0 or T == 0:
        raise L.GeobiError('nearest_point: empty query or target set (Q = %d, T = %d)' % (Q, T))
    if index is not None:
        return meshgrid.point_grid(index, b).nearest(a)
    dist = torch.empty(Q, dtype=torch.float32, device=a.device)
    idx = torch.empty(Q, dtype=torch.int32, device=a.device)
    ws = _nearest_ws(Q, T, a.device)
    L.call('geobi_nearest_point', L.ptr(a), L.ptr(b), Q, T, L.ptr(dist), L.ptr(idx), L.ptr(ws), ws.numel(), L.stream())
    return dist, idx


def point_to_mesh(points, verts, faces, index=None):
    """Distance from every row of points [Q, 3] to the surface (verts [V, 3], faces [F, 3]): the closest point of the
    closest triangle, interior, edge or corner -> (dist float32 [Q], face int32 [Q]).  index: None walks all pairs; 'grid'
    builds a meshgrid.TriangleGrid over the surface first, one built over it before is used as it is -- the same bits
    either way."""
    index = meshgrid.check_index(index)
    p, v = _points(points, 'query points'), _points(verts, 'mesh vertices')
    L.require_device(faces, 'faces')
    Q, V, F = p.shape[0], v.shape[0], faces.shape[0]
    if Q == 0 or V == 0 or F == 0 or faces.dim() != 2 or faces.shape[1] != 3:
        raise L.GeobiError('point_to_mesh: empty query set or mesh (Q = %d, V = %d, faces %s)' % (Q, V, tuple(faces.shape)))
    if index is not None:
        return meshgrid.triangle_grid(index, v, faces).nearest(p)
    meshin.check_faces(faces, V)                             # range-checked before a kernel walks it
    fv = faces.to(torch.int32).contiguous()
    dist = torch.empty(Q, dtype=torch.float32, device=p.device)
    face = torch.empty(Q, dtype=torch.int32, device=p.device)
    ws = _nearest_ws(Q, F, p.device)
    L.call('geobi_nearest_triangle', L.ptr(p), L.ptr(v), L.ptr(fv), Q, V, F, L.ptr(dist), L.ptr(face), L.ptr(ws),
           ws.numel(), L.stream())
    return dist, face


def dist_summary(dist):
    """(sum, max) of a float32 vector as a device float64 [2] tensor: fp64 accumulation in a fixed order."""
    L.require_device(dist, 'distances')
    d = dist.detach().to(torch.float32).contiguous().view(-1)
    if d.numel() == 0:
        raise L.GeobiError('dist_summary: empty vector')
    out = torch.empty(2, dtype=torch.float64, device=d.device)
    ws = L.workspace(L.size_query('geobi_dist_summary_ws_bytes', d.numel()), d.device)
    L.call('geobi_dist_summary', L.ptr(d), d.numel(), L.ptr(out), L.ptr(ws), ws.numel(), L.stream())
    return out


def mean_edge_length(points, faces):
    """Mean length of the mesh edges, each undirected edge once (code/data_util.py:595-597) -> device float [1].
    The vertex graph lists every edge in both directions, so its mean is the same number."""
    V = points.shape[0]
    rowptr, lst = meshprep.vertex_faces(faces, V)
    return meshprep.mean_edge_length(points, meshprep.ring_graph(0, faces, rowptr, lst, V))


def align_target(target_points, target_faces, samples, seed=1, stream_id=0, device=None):
    """The ICP target of align(samples=): the target's vertices followed by `samples` points drawn by area on its surface
    (meshsample.sample_surface, draw 0) -> device float32 [V + samples, 3]."""
    from . import meshsample
    if target_faces is None:
        raise ValueError('align: samples = %d needs target_faces (the surface to sample)' % samples)
    t, tf = meshin.device_mesh(target_points, target_faces, meshin.default_device(device, target_points))
    drawn = meshsample.sample_surface(t, tf, samples, seed=seed, stream_id=stream_id, draw=0, check=False)
    return torch.cat([_points(t, 'target points'), drawn.points])


def align(points, target_points, device=None, estimate_scale=False, allow_reflection=False, max_iterations=100,
          relative_rmse_thr=1e-6, target_faces=None, samples=0, seed=1, stream_id=0):
    """Rigid ICP of one point set onto another (ops.icp; arrays or tensors, sizes may differ) -> ops.IcpResult: xt the
    aligned points on the device, R [1,3,3], T [1,3], s, rmse, iterations, converged [1] on the host.
    samples > 0: the target is align_target(): its vertices followed by that many points drawn by area on its surface
    (target_faces) -- a CAD target of a few large triangles has no vertex inside a face to be nearest to.  The source stays
    its vertices; everything else is ops.icp as without samples."""
    dev = meshin.default_device(device, points)
    p = meshin.to_device(points, dev, torch.float32)
    if int(samples) < 0:
        raise ValueError('align: samples = %d is negative' % samples)
    if int(samples) > 0:
        t = align_target(target_points, target_faces, int(samples), seed, stream_id, dev)
    else:
        t = meshin.to_device(target_points, dev, torch.float32)
    return ops.icp(_points(p, 'points'), _points(t, 'target points'), estimate_scale=estimate_scale,
                   allow_reflection=allow_reflection, max_iterations=max_iterations, relative_rmse_thr=relative_rmse_thr)


def align_info(res):
    """The AlignInfo.txt fields of a single-pair IcpResult: iterations, converged, rmse, scale, the rotation angle in
    degrees and |T|."""
    import math
    cos = max(-1.0, min(1.0, (float(res.R[0].diagonal().sum()) - 1.0) / 2.0))
    return {'icp_iterations': int(res.iterations[0]), 'icp_converged': bool(res.converged[0]), 'icp_rmse': float(res.rmse[0]),
            'icp_scale': float(res.s[0]), 'icp_angle': math.degrees(math.acos(cos)), 'icp_shift': float(res.T[0].norm())}


_ALIGN_KEYS = ('icp_rmse', 'icp_iterations', 'icp_converged')
_align_points = align          # the scoring functions below take a flag of the same name


def eval_pair(result_points, faces, gt_points, gt_faces=None, device=None, align=False, estimate_scale=False, index=None):
    """The numbers of one (result, ground truth) pair, code/data_util.py:584-616.  Arrays or tensors; the work runs on
    `device` (default: the tensors' device, else the current one).  gt_faces defaults to `faces` (a denoised mesh keeps its
    connectivity).  align: the result points are first brought into the ground truth's frame by rigid ICP (align();
    estimate_scale: with a scale), and the dict gains icp_rmse, icp_iterations, icp_converged.  Returns a dict:

      num_f, err_face (mean |n_r - n_o|^2), angle (mean angle in degrees, network.error_n), num_v,
      err_v (mean distance to the nearest ground-truth vertex), err_v_norm (the same over `scale`, the ground truth's
      mean edge length)                                                   -- the reference's six
      surf, surf_norm (mean distance to the ground-truth SURFACE, raw and over `scale`),
      hausdorff (the larger of the two directed maxima of nearest-vertex distance), scale.

    index='grid': every search goes through a grid over its target (meshgrid), built once per target; the numbers are the
    same bits."""
    index = meshgrid.check_index_word(index, 'eval_pair')
    dev = meshin.default_device(device, result_points)
    pr, po = meshin.to_device(result_points, dev, torch.float32), meshin.to_device(gt_points, dev, torch.float32)
    fr = meshin.as_tensor(faces)
    fo = fr if gt_faces is None or gt_faces is faces else meshin.as_tensor(gt_faces)
    if pr.shape != po.shape or fr.shape != fo.shape:
        raise ValueError('result (V = %d, F = %d) and ground truth (V = %d, F = %d) differ in size'
                         % (pr.shape[0], fr.shape[0], po.shape[0], fo.shape[0]))
    same = fo is fr                                          # one table, also when handed in twice: one check
    fr = meshin.device_mesh(pr, fr, dev)[1]
    icp = None
    if align:
        icp = _align_points(pr, po, dev, estimate_scale=estimate_scale)
        pr = icp.xt
    fo = fr if same else meshin.device_mesh(po, fo, dev)[1]
    V, F = pr.shape[0], fr.shape[0]
    nr, no = computer_face_normal(pr, fr), computer_face_normal(po, fo)
    err_face = network.loss_n(nr, no, 'L2')
    angle = network.error_n(nr, no)
    scale = mean_edge_length(po, fo)
    d_ro, _ = nearest_point(pr, po, index=index)             # three targets, each searched once
    d_or, _ = nearest_point(po, pr, index=index)
    d_surf, _ = point_to_mesh(pr, po, fo, index=index)
    s_ro, s_or, s_surf = dist_summary(d_ro), dist_summary(d_or), dist_summary(d_surf)
    host = torch.cat([err_face.reshape(1).double(), angle.reshape(1).double(), scale.double(), s_ro, s_or, s_surf]).tolist()
    err_face, angle, scale = host[0], host[1], host[2]
    err_v, surf = host[3] / V, host[7] / V
    row = {'num_f': F, 'err_face': err_face, 'angle': angle, 'num_v': V, 'err_v': err_v, 'err_v_norm': err_v / scale,
           'surf': surf, 'surf_norm': surf / scale, 'hausdorff': max(host[4], host[6]), 'scale': scale}
    if icp is not None:
        info = align_info(icp)
        row.update((k, info[k]) for k in _ALIGN_KEYS)
    return row


def eval_free(result_points, result_faces, gt_points, gt_faces, device=None, align=False, estimate_scale=False, index=None):
    """The numbers of a pair whose vertex counts, face tables or numbering DIFFER (another tool's output, a scan against
    its CAD model): nothing here pairs row i with row i.  align / estimate_scale as in eval_pair.  Returns a dict:

      num_f, num_v, num_f_gt, num_v_gt,
      angle (mean over the result's faces of the angle, in degrees, between the face normal and the normal of the
      ground-truth triangle nearest to the face's centroid: point_to_mesh's face index, a gather, network.error_n),
      surf (mean distance from the result's vertices to the ground-truth SURFACE), surf_back (from the ground truth's
      vertices to the result's surface), hausdorff (the larger of the two directed maxima of those distances),
      scale (the ground truth's mean edge length), surf_norm, surf_back_norm (over scale),
      and with align: icp_rmse, icp_iterations, icp_converged.

    index='grid': the searches go through one grid per surface (meshgrid), the ground truth's serving both of its
    searches; the numbers are the same bits."""
    index = meshgrid.check_index_word(index, 'eval_free')
    dev = meshin.default_device(device, result_points)
    pr, fr = meshin.device_mesh(result_points, result_faces, dev)
    po, fo = meshin.device_mesh(gt_points, gt_faces, dev)
    if min(pr.shape[0], fr.shape[0], po.shape[0], fo.shape[0]) == 0:
        raise ValueError('eval_free: empty mesh (result V = %d, F = %d, ground truth V = %d, F = %d)'
                         % (pr.shape[0], fr.shape[0], po.shape[0], fo.shape[0]))
    icp = None
    if align:
        icp = _align_points(pr, po, dev, estimate_scale=estimate_scale)
        pr = icp.xt
    nr, no = computer_face_normal(pr, fr).contiguous(), computer_face_normal(po, fo).contiguous()
    g_o = meshgrid.TriangleGrid(_points(po, 'mesh vertices'), fo) if index is not None else None
    _, near = point_to_mesh(face_centroids(pr, fr), po, fo, index=g_o)
    ng = torch.empty_like(nr)
    L.call('geobi_gather_rows', L.ptr(no), L.ptr(near), 3, near.shape[0], L.ptr(ng), L.stream())
    angle = network.error_n(nr, ng)
    scale = mean_edge_length(po, fo)
    d_ro, _ = point_to_mesh(pr, po, fo, index=g_o)
    d_or, _ = point_to_mesh(po, pr, fr, index=index)
    host = torch.cat([angle.reshape(1).double(), scale.double(), dist_summary(d_ro), dist_summary(d_or)]).tolist()
    scale = host[1]
    surf, back = host[2] / pr.shape[0], host[4] / po.shape[0]
    row = {'num_f': fr.shape[0], 'num_v': pr.shape[0], 'num_f_gt': fo.shape[0], 'num_v_gt': po.shape[0], 'angle': host[0],
           'surf': surf, 'surf_back': back, 'hausdorff': max(host[3], host[5]), 'scale': scale, 'surf_norm': surf / scale,
           'surf_back_norm': back / scale}
    if icp is not None:
        info = align_info(icp)
        row.update((k, info[k]) for k in _ALIGN_KEYS)
    return row


def eval_signed(result_points, result_faces, gt_points, gt_faces, device=None, index=None):
    """Which SIDE of the ground truth a result lies on (meshwind) -- what no unsigned distance shows of a
    result that shrank.  Sizes may differ, as for eval_free.  Returns a dict:

      num_v, signed (mean over the result's vertices of their distance to the ground-truth surface, NEGATIVE for a vertex
      inside it: winding number above 1/2), signed_norm (over scale, the ground truth's mean edge length), inside (the share
      of vertices inside), volume, volume_gt (the volume the closed components enclose as each file winds them),
      volume_ratio (result over ground truth; None when either mesh has a component that is not closed or the ground
      truth encloses nothing), scale.

    The distances are point_to_mesh's (index='grid': through a grid, the same bits); the two sums go through
    dist_summary."""
    from . import meshwind
    index = meshgrid.check_index_word(index, 'eval_signed')
    dev = meshin.default_device(device, result_points)
    pr, fr = meshin.finite_mesh(result_points, result_faces, dev, 'eval_signed')
    po, fo = meshin.finite_mesh(gt_points, gt_faces, dev, 'eval_signed')
    if min(pr.shape[0], fr.shape[0], po.shape[0], fo.shape[0]) == 0:
        raise ValueError('eval_signed: empty mesh (result V = %d, F = %d, ground truth V = %d, F = %d)'
                         % (pr.shape[0], fr.shape[0], po.shape[0], fo.shape[0]))
    with torch.cuda.device(dev):
        dist, _ = point_to_mesh(pr, po, fo, index=index)
        within = meshwind.winding_device(pr, po, fo) > 0.5
        zero = torch.zeros_like(dist)
        scale = mean_edge_length(po, fo)
        host = torch.cat([scale.double(), dist_summary(torch.where(within, zero, dist)), dist_summary(torch.where(within, dist, zero)),
                          within.sum().double().reshape(1)]).tolist()
        vol_r, closed_r, parts_r = meshwind.enclosed_volume(pr, fr)
        vol_o, closed_o, parts_o = meshwind.enclosed_volume(po, fo)
    V, scale = pr.shape[0], host[0]
    signed = (host[1] - host[3]) / V
    ratio = vol_r / vol_o if closed_r == parts_r and closed_o == parts_o and vol_o != 0.0 else None
    return {'num_v': V, 'signed': signed, 'signed_norm': signed / scale, 'inside': host[5] / V, 'volume': vol_r,
            'volume_gt': vol_o, 'volume_ratio': ratio, 'scale': scale}


_SIGNED_COLUMNS = ('num_v', 'signed', 'signed_norm', 'inside', 'volume_ratio')
_SIGNED_FMT = '{0:<{1}}  {2:>7}  {3:10.6f}  {4:9.6f}  {5:.6f}  {6}\n'


def _ratio_text(ratio):
    return '-' if ratio is None else '%.6f' % ratio


def signed_totals(rows):
    """Vertex-count weighted means of eval_signed's columns; volume_ratio is the ratio of the summed volumes over the files
    that have one (None when none has)."""
    n = sum(r['num_v'] for r in rows)
    tot = {k: sum(r[k] * r['num_v'] for r in rows) / n for k in ('signed', 'signed_norm', 'inside')}
    with_ratio = [r for r in rows if r['volume_ratio'] is not None]
    tot.update(num_v=n, volume_ratio=(sum(r['volume'] for r in with_ratio) / sum(r['volume_gt'] for r in with_ratio)
                                      if with_ratio and sum(r['volume_gt'] for r in with_ratio) != 0.0 else None))
    return tot


def eval_sampled(result_points, result_faces, gt_points, gt_faces, n_samples, seed=1, stream_id=0, device=None, index=None):
    """eval_free's distances measured from points drawn by area on the two SURFACES (meshsample.sample_surface) instead of
    from their vertices: two meshes that share every vertex and differ inside their triangles are `surf = 0` to eval_free
    and not to this.  Returns a dict:

      num_s (= n_samples),
      surf_s (mean distance from n_samples points of the result's surface, draw 1, to the ground-truth surface),
      surf_back_s (from n_samples points of the ground truth's surface, draw 0, to the result's surface),
      hausdorff_s (the larger of the two directed maxima),
      angle_s (mean angle in degrees between a result sample's face normal and the normal of the ground-truth triangle
      nearest to the sample: area-weighted, so it does not depend on the tessellation),
      scale (the ground truth's mean edge length), surf_s_norm, surf_back_s_norm (over scale).

    The sums go through dist_summary; one host read brings the pair's numbers (beside the one read per sampled mesh that
    refuses a mesh without area).  index='grid': either search goes through a grid over its surface (meshgrid); the
    numbers are the same bits."""
    from . import meshsample
    index = meshgrid.check_index_word(index, 'eval_sampled')
    n = int(n_samples)
    if n < 1:
        raise ValueError('eval_sampled: n_samples = %d (at least one)' % n)
    dev = meshin.default_device(device, result_points)
    pr, fr = meshin.device_mesh(result_points, result_faces, dev)
    po, fo = meshin.device_mesh(gt_points, gt_faces, dev)
    if min(pr.shape[0], fr.shape[0], po.shape[0], fo.shape[0]) == 0:
        raise ValueError('eval_sampled: empty mesh (result V = %d, F = %d, ground truth V = %d, F = %d)'
                         % (pr.shape[0], fr.shape[0], po.shape[0], fo.shape[0]))
    sr = meshsample.sample_surface(pr, fr, n, seed=seed, stream_id=stream_id, draw=1, check=False)
    so = meshsample.sample_surface(po, fo, n, seed=seed, stream_id=stream_id, draw=0, check=False)
    d_ro, near = point_to_mesh(sr.points, po, fo, index=index)   # two targets, each searched once
    d_or, _ = point_to_mesh(so.points, pr, fr, index=index)
    no = computer_face_normal(po, fo).contiguous()
    ng = torch.empty((n, 3), dtype=torch.float32, device=dev)
    L.call('geobi_gather_rows', L.ptr(no), L.ptr(near), 3, n, L.ptr(ng), L.stream())
    angle = network.error_n(meshsample.sample_normals(pr, fr, sr), ng)
    scale = mean_edge_length(po, fo)
    host = torch.cat([angle.reshape(1).double(), scale.double(), dist_summary(d_ro), dist_summary(d_or)]).tolist()
    scale = host[1]
    surf, back = host[2] / n, host[4] / n
    return {'num_s': n, 'surf_s': surf, 'surf_back_s': back, 'hausdorff_s': max(host[3], host[5]), 'angle_s': host[0],
            'scale': scale, 'surf_s_norm': surf / scale, 'surf_back_s_norm': back / scale}


_SAMPLED_COLUMNS = ('num_s', 'angle_s', 'surf_s', 'surf_s_norm', 'surf_back_s', 'surf_back_s_norm', 'hausdorff_s')
_SAMPLED_FMT = '{0:<{1}}  {2:>7}  {3:9.6f}  {4:.6f}  {5:9.6f}  {6:.6f}  {7:9.6f}  {8:.6f}\n'


def sampled_totals(rows):
    """Sample-count weighted means of eval_sampled's columns; hausdorff_s is the maximum over the files."""
    n = sum(r['num_s'] for r in rows)
    tot = {k: sum(r[k] * r['num_s'] for r in rows) / n for k in _SAMPLED_COLUMNS[1:-1]}
    tot.update(num_s=n, hausdorff_s=max(r['hausdorff_s'] for r in rows))
    return tot


def pair_files(dir_result, dir_original):
    """The reference's pairing (code/data_util.py:563-567), sorted: every dir_original/NAME.obj with every
    dir_result/NAME_*.obj -> [(result file, original file)]."""
    return [(name_r, name) for name in folders.obj_files(dir_original)
            for name_r in folders.variants_of(dir_result, folders.stem_of(name))]


_FILE_FMT = '{0:<{1}}  {2:>7}  {3:.6f}  {4:9.6f}  {5:>7}  {6:9.6f}  {7:.6f}  {8:9.6f}  {9:.6f}  {10:9.6f}\n'
_TOTAL_FMT = '         {0:>8}  {1:.4f}   {2:7.4f}    {3:>8}   {4:7.4f}   {5:.4f}   {6:7.4f}   {7:.4f}   {8:7.4f} \n'


def totals(rows):
    """Face- / vertex-count weighted means over the files as in the reference (code/data_util.py:619-621); the
    Hausdorff column is the maximum over the files."""
    nf = sum(r['num_f'] for r in rows)
    nv = sum(r['num_v'] for r in rows)

    def mean(key, weight, n):
        return sum(r[key] * r[weight] for r in rows) / n
    return {'num_f': nf, 'err_face': mean('err_face', 'num_f', nf), 'angle': mean('angle', 'num_f', nf), 'num_v': nv,
            'err_v': mean('err_v', 'num_v', nv), 'err_v_norm': mean('err_v_norm', 'num_v', nv),
            'surf': mean('surf', 'num_v', nv), 'surf_norm': mean('surf_norm', 'num_v', nv),
            'hausdorff': max(r['hausdorff'] for r in rows)}


_COLUMNS = ('num_f', 'err_face', 'angle', 'num_v', 'err_v', 'err_v_norm', 'surf', 'surf_norm', 'hausdorff')


_FREE_COLUMNS = ('num_f', 'num_v', 'num_f_gt', 'num_v_gt', 'angle', 'surf', 'surf_norm', 'surf_back', 'surf_back_norm',
                 'hausdorff')
_FREE_FMT = '{0:<{1}}  {2:>7}  {3:>7}  {4:>7}  {5:>7}  {6:9.6f}  {7:.6f}  {8:9.6f}  {9:.6f}  {10:9.6f}  {11:.6f}\n'
_ALIGN_FMT = '{0:<{1}}  {2:>4}  {3:>3}  {4:.6e}  {5:.6f}  {6:10.6f}  {7:.6f}\n'


def free_totals(rows):
    """Face- / vertex-count weighted means of eval_free's columns (the back distances over the ground truth's vertices);
    hausdorff is the maximum over the files."""
    n = {k: sum(r[k] for r in rows) for k in ('num_f', 'num_v', 'num_f_gt', 'num_v_gt')}

    def mean(key, weight):
        return sum(r[key] * r[weight] for r in rows) / n[weight]
    n.update(angle=mean('angle', 'num_f'), surf=mean('surf', 'num_v'), surf_norm=mean('surf_norm', 'num_v'),
             surf_back=mean('surf_back', 'num_v_gt'), surf_back_norm=mean('surf_back_norm', 'num_v_gt'),
             hausdorff=max(r['hausdorff'] for r in rows))
    return n


def align_line(name, width, info):
    return _ALIGN_FMT.format(name, width, info['icp_iterations'], 'yes' if info['icp_converged'] else 'no', info['icp_rmse'],
                             info['icp_scale'], info['icp_angle'], info['icp_shift'])


def eval_dirs(dir_result, dir_original, device=None, stats=None, align=False, free=False, estimate_scale=False, samples=0,
              seed=1, index=None, signed=False):
    """eval_denoising_result(dir_result, dir_original): every pair of pair_files scored with eval_pair, the per-file
    and totals lines printed and written to dir_result/ErrorInfo_h.txt in the reference's format with three columns
    appended (surf, surf_norm, hausdorff).  A result whose V or F differs from its ground truth is a ValueError naming
    both files.  stats (optional dict): seconds spent in 'parse' (reading the OBJ files) and 'device' are added.
    align: every result is first aligned to its ground truth by rigid ICP (estimate_scale: with a scale) and
    dir_result/AlignInfo.txt lists per file: iterations, converged, rmse, scale, rotation angle in degrees, |T|.
    free: every pair is scored with eval_free instead (sizes may differ) and dir_result/ErrorInfo_free.txt is written;
    ErrorInfo_h.txt is not.  samples > 0 (with free): every pair is ALSO scored with eval_sampled from that many points
    per surface (seed; the Philox stream is meshnoise.stream_of the ground-truth file's stem) and
    dir_result/ErrorInfo_sampled.txt is written beside ErrorInfo_free.txt, whose bytes the flag does not change; with align
    as well, the alignment target is the ground truth's vertices followed by its draw-0 samples (align(samples=)), which
    is another alignment and so other numbers in both files.  Returns (rows, totals) -- rows carry 'file', and with
    samples eval_sampled's keys.  index='grid': the scoring searches go through grids (eval_pair, eval_free, eval_sampled);
    every file keeps its bytes.  signed (with free): every pair is ALSO scored with eval_signed and
    dir_result/ErrorInfo_signed.txt is written beside ErrorInfo_free.txt, whose bytes the flag does not change; the signed
    keys of a row and of the totals carry the suffix _sd where eval_free has a key of that name."""
    import time
    index = meshgrid.check_index_word(index, 'eval')
    if samples and not free:
        raise ValueError('eval: samples need the free scoring (eval_free pairs nothing by index; neither do samples)')
    if signed and not free:
        raise ValueError('eval: signed needs the free scoring (eval_signed pairs nothing by index)')
    signed_rows = []
    pairs = pair_files(dir_result, dir_original)
    if not pairs:
        print('--- empty data ---')
        return [], None
    dev = meshin.default_device(device)
    width = max(len(os.path.basename(r)) for r, _ in pairs)
    rows, infos = [], []
    for file_r, file_o in pairs:
        t0 = time.time()
        pr, fr = meshio.read_obj(file_r)
        po, fo = meshio.read_obj(file_o)
        t1 = time.time()
        if not free and (pr.shape != po.shape or fr.shape != fo.shape):
            raise ValueError('%s (V = %d, F = %d) and its ground truth %s (V = %d, F = %d) differ in size'
                             % (file_r, pr.shape[0], fr.shape[0], file_o, po.shape[0], fo.shape[0]))
        stream_id = meshnoise.stream_of(os.path.basename(file_o)[:-4]) if samples else 0
        if align:
            res = _align_points(pr, po, dev, estimate_scale=estimate_scale, target_faces=fo if samples else None,
                                samples=samples, seed=seed, stream_id=stream_id)
            infos.append(align_info(res))
            pr = res.xt
        row = (eval_free(pr, fr, po, fo, device=dev, index=index) if free
               else eval_pair(pr, fr, po, gt_faces=fo, device=dev, index=index))
        if samples:
            sampled = eval_sampled(pr, fr, po, fo, samples, seed=seed, stream_id=stream_id, device=dev, index=index)
            row.update((k, sampled[k]) for k in _SAMPLED_COLUMNS)
        if signed:
            signed_rows.append(eval_signed(pr, fr, po, fo, device=dev, index=index))
            row.update((k, signed_rows[-1][k]) for k in _SIGNED_COLUMNS[1:])
        if align:
            row.update((k, infos[-1][k]) for k in _ALIGN_KEYS)
        row['file'] = os.path.basename(file_r)
        rows.append(row)
        if stats is not None:
            stats['parse'] = stats.get('parse', 0.0) + (t1 - t0)
            stats['device'] = stats.get('device', 0.0) + (time.time() - t1)
        if free:
            print('{0:<{1}}  {2:>7}  {3:>7}  {4:>7}  {5:>7}  {6:7.4f}  {7:.4f}  {8:7.4f}  {9:.4f}  {10:7.4f}  {11:.4f}'.format(
                row['file'], width, *[row[k] for k in _FREE_COLUMNS]))
        else:
            print('{0:<{1}}  {2:>7}  {3:.4f}  {4:7.4f}  {5:>7}  {6:7.4f}  {7:.4f}  {8:7.4f}  {9:.4f}  {10:7.4f}'.format(
                row['file'], width, *[row[k] for k in _COLUMNS]))
    if align:
        file_txt = os.path.join(dir_result, 'AlignInfo.txt')
        with open(file_txt, 'w') as f:
            f.write('Align:  iterations  converged  rmse  scale  angle_deg  shift \n')
            for row, info in zip(rows, infos):
                f.write(align_line(row['file'], width, info))
        print('%s saved.' % file_txt)
    if free:
        tot = free_totals(rows)
        print('{0:>7}  {1:>7}  {2:>7}  {3:>7}  {4:7.4f}  {5:.4f}  {6:7.4f}  {7:.4f}  {8:7.4f}  {9:.4f} \n'.format(
            *[tot[k] for k in _FREE_COLUMNS]))
        file_txt = os.path.join(dir_result, 'ErrorInfo_free.txt')
        with open(file_txt, 'w') as f:
            f.write('Error_free:  num_f  num_v  num_f_gt  num_v_gt  angle_mean  surf  surf_norm  surf_back  surf_back_norm  hausdorff \n')
            f.write(_FREE_FMT.format('', width, *[tot[k] for k in _FREE_COLUMNS]))
            f.write('\n')
            for row in rows:
                f.write(_FREE_FMT.format(row['file'], width, *[row[k] for k in _FREE_COLUMNS]))
        print('%s saved.' % file_txt)
        if samples:
            tot_s = sampled_totals(rows)
            tot.update(tot_s)
            file_txt = os.path.join(dir_result, 'ErrorInfo_sampled.txt')
            with open(file_txt, 'w') as f:
                f.write('Error_sampled:  num_s  angle_mean  surf  surf_norm  surf_back  surf_back_norm  hausdorff \n')
                f.write(_SAMPLED_FMT.format('', width, *[tot_s[k] for k in _SAMPLED_COLUMNS]))
                f.write('\n')
                for row in rows:
                    f.write(_SAMPLED_FMT.format(row['file'], width, *[row[k] for k in _SAMPLED_COLUMNS]))
            print('%s saved.' % file_txt)
        if signed:
            tot_sd = signed_totals(signed_rows)
            tot.update((k, tot_sd[k]) for k in _SIGNED_COLUMNS[1:])
            file_txt = os.path.join(dir_result, 'ErrorInfo_signed.txt')
            with open(file_txt, 'w') as f:
                f.write('Error_signed:  num_v  signed  signed_norm  inside  volume_ratio \n')
                f.write(_SIGNED_FMT.format('', width, *[tot_sd[k] for k in _SIGNED_COLUMNS[:-1]] + [_ratio_text(tot_sd['volume_ratio'])]))
                f.write('\n')
                for row, sd in zip(rows, signed_rows):
                    f.write(_SIGNED_FMT.format(row['file'], width, *[sd[k] for k in _SIGNED_COLUMNS[:-1]] + [_ratio_text(sd['volume_ratio'])]))
            print('%s saved.' % file_txt)
        return rows, tot
    tot = totals(rows)
    print('{0:>8}  {1:.4f}  {2:7.4f}  {3:>8}  {4:7.4f}  {5:.4f}  {6:7.4f}  {7:.4f}  {8:7.4f} \n'.format(
        *[tot[k] for k in _COLUMNS]))
    file_txt = os.path.join(dir_result, 'ErrorInfo_h.txt')
    with open(file_txt, 'w') as f:
        f.write('Error_rst:  num_f   mean   angle_mean   num_v    err_dis    err_surf    hausdorff \n')
        f.write(_TOTAL_FMT.format(*[tot[k] for k in _COLUMNS]))
        f.write('\n')
        for row in rows:
            f.write(_FILE_FMT.format(row['file'], width, *[row[k] for k in _COLUMNS]))
    print('%s saved.' % file_txt)
    return rows, tot
