"""Scoring a denoised mesh against its ground truth: data_util.eval_denoising_result
(code/data_util.py:559-638) with its vertex metric on the MI355X.

The reference computes, per vertex of the result, the distance to the nearest ground-truth vertex by brute force on
CPU threads (code/my_hausdorff.py) and keeps the point-to-surface form commented out beside it (p2m, :601-603).  Both
are all-pairs HIP kernels here (csrc/dist.hip: geobi_nearest_point, geobi_nearest_triangle); sums and maxima are
reduced in fp64 on the device (geobi_dist_summary), and one read brings a pair's numbers to the host.
"""
import glob
import os

import torch

from . import _lib as L
from . import meshin, meshio, meshprep, network
from .data_util import computer_face_normal


def _points(t, what):
    L.require_device(t, what)
    t = t.detach().to(torch.float32).contiguous()
    if t.dim() != 2 or t.shape[1] != 3:
        raise L.GeobiError('%s must be [n, 3], got %s' % (what, tuple(t.shape)))
    return t


def _nearest_ws(Q, T, dev):
    return L.workspace(L.size_query('geobi_nearest_ws_bytes', Q, T), dev)


def nearest_point(a, b):
    """my_hausdorff.nearest_distance(a, b): for every row of a [Q, 3] the distance to the nearest row of b [T, 3] and
    that row's index (the lowest among equally near ones) -> (dist float32 [Q], idx int32 [Q])."""
    a, b = _points(a, 'query points'), _points(b, 'target points')
    Q, T = a.shape[0], b.shape[0]
    if Q == 0 or T == 0:
        raise L.GeobiError('nearest_point: empty query or target set (Q = %d, T = %d)' % (Q, T))
    dist = torch.empty(Q, dtype=torch.float32, device=a.device)
    idx = torch.empty(Q, dtype=torch.int32, device=a.device)
    ws = _nearest_ws(Q, T, a.device)
    L.call('geobi_nearest_point', L.ptr(a), L.ptr(b), Q, T, L.ptr(dist), L.ptr(idx), L.ptr(ws), ws.numel(), L.stream())
    return dist, idx


def point_to_mesh(points, verts, faces):
    """Distance from every row of points [Q, 3] to the surface (verts [V, 3], faces [F, 3]): the closest point of the
    closest triangle, interior, edge or corner -> (dist float32 [Q], face int32 [Q])."""
    p, v = _points(points, 'query points'), _points(verts, 'mesh vertices')
    L.require_device(faces, 'faces')
    Q, V, F = p.shape[0], v.shape[0], faces.shape[0]
    if Q == 0 or V == 0 or F == 0 or faces.dim() != 2 or faces.shape[1] != 3:
        raise L.GeobiError('point_to_mesh: empty query set or mesh (Q = %d, V = %d, faces %s)' % (Q, V, tuple(faces.shape)))
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


def eval_pair(result_points, faces, gt_points, gt_faces=None, device=None):
    """The numbers of one (result, ground truth) pair, code/data_util.py:584-616.  Arrays or tensors; the work runs on
    `device` (default: the tensors' device, else the current one).  gt_faces defaults to `faces` (a denoised mesh keeps its
    connectivity).  Returns a dict:

      num_f, err_face (mean |n_r - n_o|^2), angle (mean angle in degrees, network.error_n), num_v,
      err_v (mean distance to the nearest ground-truth vertex), err_v_norm (the same over `scale`, the ground truth's
      mean edge length)                                                   -- the reference's six
      surf, surf_norm (mean distance to the ground-truth SURFACE, raw and over `scale`),
      hausdorff (the larger of the two directed maxima of nearest-vertex distance), scale."""
    dev = meshin.default_device(device, result_points)
    pr, po = meshin.to_device(result_points, dev, torch.float32), meshin.to_device(gt_points, dev, torch.float32)
    fr = meshin.as_tensor(faces)
    fo = fr if gt_faces is None or gt_faces is faces else meshin.as_tensor(gt_faces)
    if pr.shape != po.shape or fr.shape != fo.shape:
        raise ValueError('result (V = %d, F = %d) and ground truth (V = %d, F = %d) differ in size'
                         % (pr.shape[0], fr.shape[0], po.shape[0], fo.shape[0]))
    same = fo is fr                                          # one table, also when handed in twice: one check
    fr = meshin.device_mesh(pr, fr, dev)[1]
    fo = fr if same else meshin.device_mesh(po, fo, dev)[1]
    V, F = pr.shape[0], fr.shape[0]
    nr, no = computer_face_normal(pr, fr), computer_face_normal(po, fo)
    err_face = network.loss_n(nr, no, 'L2')
    angle = network.error_n(nr, no)
    scale = mean_edge_length(po, fo)
    d_ro, _ = nearest_point(pr, po)
    d_or, _ = nearest_point(po, pr)
    d_surf, _ = point_to_mesh(pr, po, fo)
    s_ro, s_or, s_surf = dist_summary(d_ro), dist_summary(d_or), dist_summary(d_surf)
    host = torch.cat([err_face.reshape(1).double(), angle.reshape(1).double(), scale.double(), s_ro, s_or, s_surf]).tolist()
    err_face, angle, scale = host[0], host[1], host[2]
    err_v, surf = host[3] / V, host[7] / V
    return {'num_f': F, 'err_face': err_face, 'angle': angle, 'num_v': V, 'err_v': err_v, 'err_v_norm': err_v / scale,
            'surf': surf, 'surf_norm': surf / scale, 'hausdorff': max(host[4], host[6]), 'scale': scale}


def pair_files(dir_result, dir_original):
    """The reference's pairing (code/data_util.py:563-567), sorted: every dir_original/NAME.obj with every
    dir_result/NAME_*.obj -> [(result file, original file)]."""
    pairs = []
    for name in sorted(glob.glob(os.path.join(glob.escape(dir_original), '*.obj'))):
        stem = os.path.basename(name)[:-4]
        for name_r in sorted(glob.glob(os.path.join(glob.escape(dir_result), glob.escape(stem) + '_*.obj'))):
            pairs.append((name_r, name))
    return pairs


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


def eval_dirs(dir_result, dir_original, device=None, stats=None):
    """eval_denoising_result(dir_result, dir_original): every pair of pair_files scored with eval_pair, the per-file
    and totals lines printed and written to dir_result/ErrorInfo_h.txt in the reference's format with three columns
    appended (surf, surf_norm, hausdorff).  A result whose V or F differs from its ground truth is a ValueError naming
    both files.  stats (optional dict): seconds spent in 'parse' (reading the OBJ files) and 'device' are added.
    Returns (rows, totals) -- rows carry 'file'."""
    import time
    pairs = pair_files(dir_result, dir_original)
    if not pairs:
        print('--- empty data ---')
        return [], None
    width = max(len(os.path.basename(r)) for r, _ in pairs)
    rows = []
    for file_r, file_o in pairs:
        t0 = time.time()
        pr, fr = meshio.read_obj(file_r)
        po, fo = meshio.read_obj(file_o)
        t1 = time.time()
        if pr.shape != po.shape or fr.shape != fo.shape:
            raise ValueError('%s (V = %d, F = %d) and its ground truth %s (V = %d, F = %d) differ in size'
                             % (file_r, pr.shape[0], fr.shape[0], file_o, po.shape[0], fo.shape[0]))
        row = eval_pair(pr, fr, po, gt_faces=fo, device=device)
        row['file'] = os.path.basename(file_r)
        rows.append(row)
        if stats is not None:
            stats['parse'] = stats.get('parse', 0.0) + (t1 - t0)
            stats['device'] = stats.get('device', 0.0) + (time.time() - t1)
        print('{0:<{1}}  {2:>7}  {3:.4f}  {4:7.4f}  {5:>7}  {6:7.4f}  {7:.4f}  {8:7.4f}  {9:.4f}  {10:7.4f}'.format(
            row['file'], width, *[row[k] for k in _COLUMNS]))
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
