"""Self-intersections of a mesh on the MI355X: which faces pass through each other -- the one defect
a denoiser, a decimator or a remesher can introduce that ``meshtopo.mesh_report`` does not show.

Two included faces that share k vertex IDS intersect when their closed triangles share a point (k = 0), a point other than
the shared vertex (k = 1), a point off the shared edge (k = 2: a face folded flat onto its neighbour); two copies of one
face (k = 3) never do.  Touching counts.  Adjacency is by id, so the search belongs on a welded table: ``mesh_report`` and
``clean_mesh`` run it there (``intersections=True``, ``drop_intersecting=True``).

All pairs, brute force (csrc/selfx.hip: geobi_self_intersections): a float32 box test per pair, then fp64 predicates in one
stated order for the pairs whose boxes overlap.  The rules are stated in include/geobi_hip.h; tests/selfx_model.py
restates them and reproduces every output.  Integer coordinates of magnitude up to 2^14 are decided exactly.  No CPU
fallback.
"""
import torch

from . import _lib as L
from . import meshin

COUNT_KEYS = ('pairs', 'pairs_k0', 'pairs_k1', 'pairs_k2', 'faces_hit', 'degenerate', 'included', 'box_candidates')
STATE_INTERSECTING = 5      # the state ``clean_mesh(drop_intersecting=True)`` gives a face: geobi_clean_compact keeps state 1
                            # alone and counts 2 (nonmanifold) and 3 (degenerate) only, as for state 4 (small part)


class SelfIntersections(object):
    """hits [F] int32: the number of faces every face intersects; pairs [min(total, max_pairs), 2] int32: the intersecting
    pairs (a < b) in ascending order, both on the device; counts: a dict over COUNT_KEYS (``pairs`` is the full total)."""

    def __init__(self, hits, pairs, counts):
        self.hits, self.pairs, self.counts = hits, pairs, counts


def search_device(v, fv, state=None, max_pairs=0):
    """geobi_self_intersections on device tensors as they are (v [V, 3] float32, fv [F, 3] int32 range-checked, state [F]
    int32 or None) -> (hits [max(F, 1)], pairs [max(max_pairs, 1), 2], device counts [8] int64); enqueued, nothing is read
    back."""
    dev, V, F = v.device, v.shape[0], fv.shape[0]
    hits = torch.zeros(max(F, 1), dtype=torch.int32, device=dev)
    pairs = torch.empty((max(int(max_pairs), 1), 2), dtype=torch.int32, device=dev)
    counts = torch.empty(len(COUNT_KEYS), dtype=torch.int64, device=dev)
    ws = L.workspace(L.size_query('geobi_self_intersections_ws_bytes', F, V), dev)
    L.call('geobi_self_intersections', L.ptr(v), L.ptr(fv), L.ptr(state), V, F, L.ptr(hits),
           L.ptr(pairs) if max_pairs else None, int(max_pairs), L.ptr(counts), L.ptr(ws), ws.numel(), L.stream())
    return hits, pairs, counts


def self_intersections(points, faces, state=None, max_pairs=0, device=None):
    """(points [V, 3], faces [F, 3]) -> SelfIntersections.  ``state`` [F]: only the faces with state 1 take part (None:
    all); ``max_pairs``: the rows of the pair list at most (0: no list).  ValueError: other shapes, non-finite points, a face
    index outside [0, V), a state of another length, max_pairs < 0."""
    if not meshin.whole(max_pairs) or not 0 <= max_pairs < 2 ** 31:
        raise ValueError('self_intersections: max_pairs = %r (a number of rows, 0 .. 2^31 - 1)' % (max_pairs,))
    dev = meshin.default_device(device, meshin.as_tensor(points))
    v, fv = meshin.finite_mesh(meshin.as_tensor(points).reshape(-1, 3), meshin.as_tensor(faces).reshape(-1, 3), dev,
                               'self_intersections')
    F = fv.shape[0]
    if state is not None:
        state = meshin.to_device(meshin.as_tensor(state).reshape(-1), dev, torch.int32)
        if state.shape[0] != F:
            raise ValueError('self_intersections: %d states for %d faces' % (state.shape[0], F))
    with torch.cuda.device(dev):
        hits, pairs, counts = search_device(v, fv, state if F else None, int(max_pairs))
        c = dict(zip(COUNT_KEYS, L.read_i64(counts)))
    return SelfIntersections(hits[:F], pairs[:min(c['pairs'], int(max_pairs))], c)
