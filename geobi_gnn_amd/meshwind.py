"""Winding numbers on the MI355X: which side of a surface is INSIDE -- the question neither the
orientation of ``meshtopo`` (consistent, but "its lowest face decides") nor the distances of ``mesheval`` /
``meshproject`` (unsigned) answer.

The generalised winding number of a point (Jacobson et al. 2013) is the sum of the signed solid angles of all faces seen
from it, over 4 pi: 1 inside and 0 outside a closed surface wound counter-clockwise seen from outside, and a little off
those where the surface has a hole or a few bad faces.  All pairs, brute force (csrc/winding.hip: geobi_winding_number):
the term in fp64 in one stated order, the sum in integers of 2^-40 of a turn, so that a query gets the same bits alone and
in a batch.  The rules are stated in include/geobi_hip.h; tests/wind_model.py restates them.  No CPU fallback.

* ``winding_number`` / ``inside`` / ``signed_distance``: the primitive, the test ``w > threshold`` and the distance of
  ``meshproject.closest`` with a minus sign inside
* ``part_solids``: signed volume (times 6) and closedness of every component of ``meshtopo``'s labels
* ``orient_outward``: ``meshtopo.orient_device``, then every closed component turned so that its volume is positive, then
  every component nested at odd depth in the others turned back: a cavity points into the void
"""
import torch

from . import _lib as L
from . import meshclean, meshin

MAX_FACES = 1 << 23         # geobi_winding_number: |term| <= 2^39 quanta, the int64 sum stays within 2^62


def winding_device(q, v, fv, state=None, face_part=None, query_part=None):
    """geobi_winding_number on device tensors as they are (q [Q, 3] and v [V, 3] float32, fv [F, 3] int32 range-checked,
    state / face_part [F] and query_part [Q] int32 or None) -> w float64 [Q]; enqueued, nothing is read back."""
    dev, Q, V, F = q.device, q.shape[0], v.shape[0], fv.shape[0]
    w = torch.zeros(Q, dtype=torch.float64, device=dev)
    if Q == 0 or F == 0:
        return w
    ws = L.workspace(L.size_query('geobi_winding_number_ws_bytes', Q, F), dev)
    L.call('geobi_winding_number', L.ptr(q), L.ptr(v), L.ptr(fv), L.ptr(state), L.ptr(face_part), L.ptr(query_part), Q, V, F,
           L.ptr(w), L.ptr(ws), ws.numel(), L.stream())
    return w


def _queries(points, what):
    q = meshin.as_tensor(points)
    if q.dim() != 2 or q.shape[1] != 3:
        raise ValueError('%s: points [Q, 3] expected, got %s' % (what, tuple(q.shape)))
    if q.shape[0] > meshin.MAX_NODES:
        raise ValueError('%s: %d query points (at most GEOBI_MAX_NODES = %d)' % (what, q.shape[0], meshin.MAX_NODES))
    return q


def _state(state, F, dev, what):
    if state is None:
        return None
    state = meshin.to_device(meshin.as_tensor(state).reshape(-1), dev, torch.int32)
    if state.shape[0] != F:
        raise ValueError('%s: %d states for %d faces' % (what, state.shape[0], F))
    return state if F else None


def winding_number(points, verts, faces, state=None, device=None):
    """points [Q, 3] against the mesh (verts [V, 3], faces [F, 3]) -> w float64 [Q] on the device.  ``state`` [F]: only the
    faces with state 1 take part (None: all).  ValueError: other shapes, non-finite vertices or queries, a face index
    outside [0, V), a state of another length, more than 2^23 faces."""
    q = _queries(points, 'winding_number')
    dev = meshin.default_device(device, meshin.as_tensor(verts))
    v, fv = meshin.finite_mesh(meshin.as_tensor(verts).reshape(-1, 3), meshin.as_tensor(faces).reshape(-1, 3), dev,
                               'winding_number')
    if fv.shape[0] > MAX_FACES:
        raise ValueError('winding_number: %d faces (at most 2^23 = %d)' % (fv.shape[0], MAX_FACES))
    q = meshin.to_device(q, dev, torch.float32)
    if q.shape[0] > 0 and not bool(torch.isfinite(q).all()):
        raise ValueError('winding_number: non-finite query coordinates')
    state = _state(state, fv.shape[0], dev, 'winding_number')
    with torch.cuda.device(dev):
        return winding_device(q, v, fv, state)


def inside(points, verts, faces, threshold=0.5, device=None):
    """-> bool [Q] on the device: ``winding_number(points, verts, faces) > threshold``."""
    return winding_number(points, verts, faces, device=device) > float(threshold)


def signed_distance(points, verts, faces, index=None, threshold=0.5, device=None):
    """-> (sd float32 [Q], w float64 [Q]) on the device: |sd| is the distance of ``meshproject.closest`` (its bits
    untouched; ``index`` is passed through to it), negative where ``w > threshold``."""
    from . import meshproject
    c = meshproject.closest(points, verts, faces, device=device, index=index)
    dev = c.dist.device
    w = winding_number(points, verts, faces, device=dev)
    return torch.where(w > float(threshold), -c.dist, c.dist), w


def part_solids_device(v, fv, label, state=None):
    """geobi_part_solids on device tensors as they are -> (volume6 float64, closed int32, consistent int32), each
    [max(F, 1)] and valid at the rows x == label[x]; enqueued, nothing is read back."""
    dev, V, F = v.device, v.shape[0], fv.shape[0]
    volume6 = torch.zeros(max(F, 1), dtype=torch.float64, device=dev)
    closed = torch.zeros(max(F, 1), dtype=torch.int32, device=dev)
    consistent = torch.zeros(max(F, 1), dtype=torch.int32, device=dev)
    if F == 0:
        return volume6, closed, consistent
    ws = L.workspace(L.size_query('geobi_part_solids_ws_bytes', F), dev)
    L.call('geobi_part_solids', L.ptr(v), L.ptr(fv), L.ptr(state), L.ptr(label), V, F, L.ptr(volume6), L.ptr(closed),
           L.ptr(consistent), L.ptr(ws), ws.numel(), L.stream())
    return volume6, closed, consistent


def part_solids(verts, faces, label, state=None, device=None):
    """Per component of ``label`` [F] (``meshtopo``'s: the lowest face of the component, -1 for a face that is none's; with
    the ``state`` given there) -> (volume6 float64 [F], closed int32 [F], consistent int32 [F]) on the device, valid at the
    rows x == label[x]: six times the signed volume about the first corner of face x (fp64, one stated order), whether
    every edge of the component has exactly two claimants, and whether every such pair walks its edge in opposite
    directions."""
    dev = meshin.default_device(device, meshin.as_tensor(verts))
    v, fv = meshin.finite_mesh(meshin.as_tensor(verts).reshape(-1, 3), meshin.as_tensor(faces).reshape(-1, 3), dev,
                               'part_solids')
    F = fv.shape[0]
    label = meshin.to_device(meshin.as_tensor(label).reshape(-1), dev, torch.int32)
    if label.shape[0] != F:
        raise ValueError('part_solids: %d labels for %d faces' % (label.shape[0], F))
    state = _state(state, F, dev, 'part_solids')
    with torch.cuda.device(dev):
        volume6, closed, consistent = part_solids_device(v, fv, label, state)
    return volume6[:F], closed[:F], consistent[:F]


def enclosed_volume(v, fv, max_rounds=256):
    """(v [V, 3] float32, fv [F, 3] int32 range-checked, on the device) -> (volume, closed components, components): the sum of
    volume6 / 6 over the components that are closed and consistently wound AS THE TABLE WINDS THEM -- a cavity wound into
    the void subtracts -- on the host; one read beside the orientation's."""
    from . import meshtopo
    F = fv.shape[0]
    if F == 0:
        return 0.0, 0, 0
    label = meshtopo.orient_device(fv, v.shape[0], None, max_rounds)[2][:F].contiguous()
    volume6, closed, consistent = part_solids_device(v, fv, label)
    root = label == torch.arange(F, dtype=torch.int32, device=fv.device)
    whole = root & (closed[:F] != 0) & (consistent[:F] != 0)
    host = torch.stack([(volume6[:F] * whole).sum() / 6.0, whole.sum().double(), root.sum().double()]).tolist()
    return host[0], int(host[1]), int(host[2])


def flip_device(fv, label, flip_of_label, flip):
    """geobi_flip_faces: -> the table with corners 1 and 2 swapped in every face whose component is marked in
    flip_of_label [F]; ``flip`` [F] is toggled there, in place."""
    F = fv.shape[0]
    out = torch.empty_like(fv)
    if F:
        L.call('geobi_flip_faces', L.ptr(fv), L.ptr(label), L.ptr(flip_of_label), F, L.ptr(out), L.ptr(flip), L.stream())
    return out


def outward_device(v, fv, V, state=None, max_rounds=256):
    """``orient_outward`` on checked device tensors (v [V, 3] float32, fv [F, 3] int32 range-checked, F >= 1) -> (faces
    [F, 3], flip [F], label [F], counts dict).  Reads the device three times: the orientation's rounds, the roots of the
    closed components, the counts."""
    from . import meshtopo
    F = fv.shape[0]
    f_out, flip, label, ocounts, rounds = meshtopo.orient_device(fv, V, state, max_rounds)
    f_out, flip, label = f_out[:F].contiguous(), flip[:F].contiguous(), label[:F].contiguous()
    volume6, closed, consistent = part_solids_device(v, f_out, label, state)
    rows = torch.arange(F, dtype=torch.int32, device=fv.device)
    root = label == rows
    solid = root & (closed[:F] != 0) & (consistent[:F] != 0) & (volume6[:F] != 0.0)      # volume6 == 0 counts as open
    # 2. every closed orientable component with a negative volume is turned
    turn_1 = (solid & (volume6[:F] < 0.0)).to(torch.int32)
    f_now = flip_device(f_out, label, turn_1, flip)
    # 3. one query per closed component, the first corner of its lowest face, against the faces of all closed components
    # as they now are; parts are the labels: a component does not see itself
    roots = torch.nonzero(solid).reshape(-1)
    turn_2 = torch.zeros(F, dtype=torch.int32, device=fv.device)
    ambiguous = torch.zeros((), dtype=torch.int32, device=fv.device)
    if roots.numel() > 0:
        q = v[f_now[roots, 0].long()].contiguous()
        in_solid = solid.to(torch.int32)[label.clamp(min=0).long()] * (label >= 0).to(torch.int32)
        w = winding_device(q, v, f_now, in_solid.contiguous(), label, roots.to(torch.int32).contiguous())
        depth = torch.round(w)
        unclear = (w - depth).abs() > 0.25                # the shells intersect: the component stays as it is
        odd = (torch.remainder(depth, 2.0) == 1.0) & ~unclear
        turn_2[roots] = odd.to(torch.int32)
        ambiguous = unclear.sum().to(torch.int32)
        f_now = flip_device(f_now, label, turn_2, flip)
    turned = ((turn_1 ^ turn_2) != 0).sum().to(torch.int32)
    tail = torch.stack([solid.sum().to(torch.int32), root.sum().to(torch.int32), turned, ambiguous.reshape(()),
                        flip.sum().to(torch.int32)])
    host = L.read_i32(torch.cat([ocounts, tail]))
    counts = {'components': host[0], 'nonorientable': host[1], 'flipped': host[7], 'rounds': rounds,
              'closed_components': host[3], 'open_components': host[4] - host[3], 'turned': host[5], 'ambiguous': host[6]}
    return f_now, flip, label, counts


def orient_outward(verts, faces, V=None, state=None, max_rounds=256, device=None):
    """(verts [V, 3], faces [F, 3] already through canon) -> ``meshtopo.Oriented`` whose closed components point outward:

    1. ``meshtopo.orient_device`` winds every component consistently
    2. every closed orientable component whose signed volume is negative is turned
    3. every such component gets one query, the first corner of its lowest face, against the faces of all the OTHER closed
       components; ``llrint(w)`` is its nesting depth, and a component at odd depth is turned again: a cavity points into
       the void.  A ``w`` farther than 1/4 from an integer means the shells intersect: the component stays and is counted
       under ``ambiguous``
    4. open and non-orientable components, and those of volume 0, stay as ``orient_device`` left them

    counts: those of ``orient_faces`` (``flipped``: the faces whose winding differs from the input's), and
    closed_components, open_components, turned (the components steps 2 and 3 left reversed), ambiguous."""
    from . import meshtopo
    meshtopo._check_rounds('orient_outward', max_rounds)
    dev = meshin.default_device(device, meshin.as_tensor(verts))
    v, fv = meshin.finite_mesh(meshin.as_tensor(verts).reshape(-1, 3), meshin.as_tensor(faces).reshape(-1, 3), dev,
                               'orient_outward')
    if V is not None and int(V) != v.shape[0]:
        raise ValueError('orient_outward: V = %r for %d vertices' % (V, v.shape[0]))
    F = fv.shape[0]
    state = _state(state, F, dev, 'orient_outward')
    if F == 0:
        empty = meshclean._empty(0, 0, torch.int32, dev)[:0]
        return meshtopo.Oriented(fv, empty, empty.clone(), dict.fromkeys(
            ('components', 'nonorientable', 'flipped', 'rounds', 'closed_components', 'open_components', 'turned', 'ambiguous'), 0))
    with torch.cuda.device(dev):
        f_now, flip, label, counts = outward_device(v, fv, v.shape[0], state, max_rounds)
    return meshtopo.Oriented(f_now, flip, label, counts)
