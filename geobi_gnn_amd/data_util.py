"""Geometry helpers of the reference's ``data_util`` that sit directly on either side of the network.

* ``computer_face_normal``  /root/reference/code/data_util.py:182-198 (called inside DualGNN.forward)
* ``face_centroids``        the centroids the reference's driver would hand to ``loss_n(..., 'sided', fc_p, fc)``
* ``update_position2``      /root/reference/code/data_util.py:529-556 (called at test_dual.py:63-72 right
  after the network; the reference moves the prediction to the CPU for it -- here it stays on the GPU)
* ``denoise_tail``          what follows every denoise, the network's or a filter's (test_dual.py:63-87): that vertex
  update and the two angular errors, with ``depth_direction``, the rule for the Kinect data types
Same names and argument meaning; tensors must live on the MI355X.
"""
import torch

from . import _lib as L
from . import meshin, network, ops


def computer_face_normal(points, fv_indices):
    """points [N,3], fv_indices [M,3] -> unit face normals [M,3] (differentiable)."""
    L.require_device(points, 'points')
    fv32 = fv_indices.to(torch.int32).contiguous()
    cidx = ops.SegmentIndex(fv32.view(-1), points.shape[0]) if points.requires_grad else None
    xf = torch.zeros((fv32.shape[0], 6), dtype=torch.float32, device=points.device)
    if cidx is None:
        out = torch.empty((fv32.shape[0], 12), dtype=torch.float32, device=points.device)
        L.call('geobi_face_geom_fwd', L.ptr(points.contiguous()), L.ptr(fv32), L.ptr(xf), 6, fv32.shape[0],
               L.ptr(out), L.stream())
        return out[:, 9:12]
    return ops.FaceGeomFn.apply(points, xf, fv32, cidx)[:, 9:12]


def face_centroids(points, fv_indices):
    """points [N,3], fv_indices [M,3] -> face centroids [M,3], detached: what loss_n(..., norm='sided', fc_p, fc)
    (code/network.py:385-388) searches in.  The centroid columns of the geometry-coupling kernel."""
    L.require_device(points, 'points')
    cache = getattr(fv_indices, '_geobi_fv', None)        # network.mark_face_table: the validated int32 form
    if cache is not None and cache[2] == points.shape[0]:
        fv32 = cache[0]
    else:
        meshin.check_faces(fv_indices, points.shape[0], 'fv_indices')     # the kernel gathers through it
        fv32 = fv_indices.to(torch.int32).contiguous()
    xf = torch.zeros((fv32.shape[0], 6), dtype=torch.float32, device=points.device)
    out = torch.empty((fv32.shape[0], 12), dtype=torch.float32, device=points.device)
    L.call('geobi_face_geom_fwd', L.ptr(points.detach().float().contiguous()), L.ptr(fv32), L.ptr(xf), 6, fv32.shape[0],
           L.ptr(out), L.stream())
    return out[:, 6:9].contiguous()


def update_position2(points, fv_indices, vf_indices, face_normals, n_iter=20, depth_direction=None):
    """n_iter Jacobi sweeps moving every vertex onto the planes of its adjacent faces.

    points [N,3], fv_indices [F,3], vf_indices [N, max_valence] (-1 padded), face_normals [F,3]."""
    L.require_device(points, 'points')
    pts = points.detach().float().contiguous()
    fv32 = fv_indices.to(torch.int32).contiguous()
    vf32 = vf_indices.to(torch.int32).contiguous()
    nrm = face_normals.detach().float().contiguous()
    dd = None if depth_direction is None else depth_direction.detach().float().contiguous()
    V, F = pts.shape[0], fv32.shape[0]
    out = torch.empty_like(pts)
    ws = L.workspace(L.size_query('geobi_update_position_ws_bytes', V, F), pts.device)
    L.call('geobi_update_position2', L.ptr(pts), L.ptr(fv32), L.ptr(vf32), vf32.shape[1], L.ptr(nrm), L.ptr(dd), V, F,
           int(n_iter), L.ptr(out), L.ptr(ws), ws.numel(), L.stream())
    return out


def depth_direction(points, data_type):
    """The Kinect data types move a vertex along its viewing ray only (code/test_dual.py:69-71): -> normalize(points) for
    them, None for every other type.  points: [N,3], or a list of such (the meshes of a union; joined only when needed)."""
    if data_type not in ('Kinect_v1', 'Kinect_v2'):
        return None
    if not torch.is_tensor(points):
        points = points[0] if len(points) == 1 else torch.cat(list(points))
    return torch.nn.functional.normalize(points, dim=1)


def angular_errors(normals, points_updated, fv_indices, gt_points=None, gt_normals=None):
    """-> (angle1, angle2), device scalars in degrees: network.error_n of `normals`, and of the normals of the updated
    mesh, against the ground truth's face normals -- `gt_normals`, else those of `gt_points` (arrays or tensors) on these
    faces.  (None, None) without ground truth."""
    if gt_normals is None:
        if gt_points is None:
            return None, None
        gt = meshin.to_device(gt_points, points_updated.device, torch.float32)
        if gt.shape != points_updated.shape:
            raise ValueError('gt_points %s for points %s' % (tuple(gt.shape), tuple(points_updated.shape)))
        gt_normals = computer_face_normal(gt, fv_indices)
    return (network.error_n(normals, gt_normals),
            network.error_n(computer_face_normal(points_updated, fv_indices), gt_normals))


def denoise_tail(points, fv_indices, vf_indices, normals, n_iter, data_type, gt_points=None, ray_points=None):
    """What follows every denoise: `n_iter` sweeps of update_position2 moving `points` towards `normals` -- for the Kinect
    data types along depth_direction(ray_points; default: points) only -- then angular_errors of the result.
    -> (V_updated, angle1, angle2); the angles stay on the device (a caller reads them when it wants them)."""
    dd = depth_direction(points if ray_points is None else ray_points, data_type)
    Vu = update_position2(points, fv_indices, vf_indices, normals, n_iter=n_iter, depth_direction=dd)
    return (Vu,) + angular_errors(normals, Vu, fv_indices, gt_points)
