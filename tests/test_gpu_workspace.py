"""Every workspace-carrying launcher through its public Python wrapper, with ``geobi_gnn_amd._lib.workspace`` replaced
(monkeypatch, inside the test) by an allocator that owns the memory behind the workspace it hands out.

Guard band   the replacement allocates nbytes + 4096, fills the tail with 0xA5 and hands out the first nbytes.  Asserted:
             after one synchronise every tail is still 0xA5, and every output equals, bit for bit, the output of the same
             call made with the library's own allocator.
Short        request k of a case gets its first nbytes - 512 bytes (the requests before it are whole).  A size is
             align_up(needed) + 256, so nbytes - 512 < needed: the launcher behind request k must raise GeobiError with
             "workspace too small", its own name and both numbers.  The memory behind the declared end is still the
             test's, so a launcher that did not check would overwrite a sentinel, not fault: the sentinels are asserted
             here too.
             The exceptions are the requests listed in TAKES_LESS: their size is a maximum over paths (the caller of the
             query does not say which path it will take) and the path taken needs less than that maximum by more than
             512 bytes, or nothing at all.  For those the assertion is the opposite one: the call succeeds, with the same
             bits and whole sentinels.

Shapes: the icosphere of meshgen.icosphere(2) (42 vertices, 80 faces), for subdivide, decimate and the remeshing steps with its
vertices jittered by a fixed seed, so that edges are short and long and (after the collapses) valences flip; node, edge, row and segment counts of 63, 64 and 65
(4 n crosses a 256-byte line between 64 and 65); 2^18 + 1 for relabel, match_coarsen, vertex_faces, segment_csr and the
grid search, whose scan or sort temporary comes from rocPRIM above 2^18; 33 parts (two launches of 32) for the part tables; FeaSt at
(6, 32) and (128, 128) with 65 nodes; the heads at the fused width (32, 1024) and at (8, 2048), 65 rows; row_loss also at
65 * 1024 + 1 rows, the first count whose workspace is larger than 512 bytes."""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PAD, SENTINEL, SHORT_BY = 4096, 0xA5, 512
BIG = (1 << 18) + 1
COUNTS = (63, 64, 65)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


_REAL = {}


class _Guarded(object):
    """Replacement of _lib.workspace; short_at = k hands request k out 512 bytes short."""

    def __init__(self, short_at=None):
        self.short_at, self.requests, self.entries = short_at, [], {}

    def __call__(self, nbytes, device):
        nbytes = int(nbytes)
        k = len(self.requests)
        give = nbytes - SHORT_BY if (k == self.short_at and nbytes > SHORT_BY) else nbytes
        buf = torch.empty(nbytes + PAD, dtype=torch.uint8, device=device)
        buf[give:] = SENTINEL
        self.requests.append((buf, give, nbytes))
        return buf[:give]

    def install(self, monkeypatch):
        """also notes which entry point every request went to (the call that carries its pointer)"""
        from geobi_gnn_amd import _lib
        real_call = _REAL.setdefault('call', _lib.call)

        def call(entry, *args):
            for k, (buf, _, _) in enumerate(self.requests):
                if k not in self.entries and buf.data_ptr() in args:
                    self.entries[k] = entry
            return real_call(entry, *args)
        monkeypatch.setattr(_lib, 'call', call)
        monkeypatch.setattr(_lib, 'workspace', self)
        return self

    def sentinels_whole(self):
        torch.cuda.synchronize()
        return all(bool((buf[give:] == SENTINEL).all()) for buf, give, _ in self.requests)


def _flat(x, out, depth=0):
    """every tensor / array / number reachable from a wrapper's result, as (shape, bytes) items in a fixed order"""
    assert depth < 6
    if torch.is_tensor(x):
        a = x.detach().cpu().contiguous().numpy()
        out.append((a.shape, str(a.dtype), a.tobytes()))
    elif isinstance(x, np.ndarray):
        out.append((x.shape, str(x.dtype), np.ascontiguousarray(x).tobytes()))
    elif isinstance(x, (list, tuple)):
        for v in x:
            _flat(v, out, depth + 1)
    elif isinstance(x, dict):
        for key in sorted(x, key=str):
            _flat(x[key], out, depth + 1)
    elif x is None or isinstance(x, (int, float, str, bool)):
        out.append(x)
    elif hasattr(x, '__dict__'):
        _flat({k: v for k, v in vars(x).items() if not k.startswith('_') and not callable(v)}, out, depth + 1)
    else:
        raise AssertionError('unexpected result %r' % type(x))
    return out


def _t(a, dev, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)


def _rand(dev, seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32)).to(dev)


def _sphere(dev):
    from geobi_gnn_amd import meshgen
    pts, faces = meshgen.icosphere(2)
    return _t(pts, dev, torch.float32), _t(faces, dev, torch.int64)


def _strip(n_vertices, dev):
    """a triangle strip: V vertices, V - 2 faces"""
    i = np.arange(n_vertices - 2)
    return _t(np.stack([i, i + 1, i + 2], 1), dev, torch.int32)


def _cycle(n, dev, symmetric=True):
    """Graph of the cycle over n nodes: 2 n directed edges, or the n edges i -> i + 1 alone"""
    from geobi_gnn_amd.graph import Graph
    i = np.arange(n)
    src, dst = (np.concatenate([i, i]), np.concatenate([(i + 1) % n, (i - 1) % n])) if symmetric else (i, (i + 1) % n)
    return Graph.from_edge_index(_t(np.stack([src, dst]), dev, torch.int64), n)


def _graph_fields(g):
    return [g.N, g.E, g.rowptr_out, g.col_out, g.rowptr_in, g.col_in, g.pos_in]


# ------------------------------------------------------------------------------------------------------ the cases
def case_clean(dev):
    from geobi_gnn_amd import meshclean
    pts, faces = _sphere(dev)
    # every face twice (the second copy loses under the half-edge rule) and one degenerate face
    faces = torch.cat([faces, faces, faces[:1] * 0])
    return meshclean.clean_mesh(pts, faces, weld_tol=0.0, orient=True, min_component=2, device=dev)


def case_topo(dev):
    from geobi_gnn_amd import meshtopo
    pts, faces = _sphere(dev)
    V = pts.shape[0]
    return [meshtopo.orient_faces(faces, V, device=dev), meshtopo.face_components(faces, V, min_component=3, device=dev),
            meshtopo.mesh_report(pts, faces, device=dev)]


def _jittered_sphere(dev):
    """the sphere with every vertex moved by a fixed normal draw of sigma 0.05, a tenth of an edge: some edges fall below
    0.8 of the mean and some lie above it -> points, faces, the mean edge length"""
    from geobi_gnn_amd import meshgen
    pts, faces = meshgen.icosphere(2)
    pts = (np.asarray(pts, np.float64) + 0.05 * np.random.RandomState(7).standard_normal(pts.shape)).astype(np.float32)
    f = np.asarray(faces, np.int64)
    edges = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    mean_edge = float(np.linalg.norm(pts[edges[:, 0]].astype(np.float64) - pts[edges[:, 1]], axis=1).mean())
    return _t(pts, dev, torch.float32), _t(faces, dev, torch.int64), mean_edge


def case_subdiv(dev):
    """one pass of each form (for max_edge: its rounds), and the stored plans replayed by ``apply``"""
    from geobi_gnn_amd import meshsubdiv
    pts, faces, mean_edge = _jittered_sphere(dev)
    out = []
    for kwargs in ({'scheme': 'midpoint'}, {'scheme': 'loop'}, {'max_edge': mean_edge}):
        r = meshsubdiv.subdivide(pts, faces, levels=1, device=dev, **kwargs)
        assert r.counts['split'] > 0
        out += [r.points, r.faces, r.face_parent, r.vertex_parents, r.counts, meshsubdiv.apply(r, pts)]
    return out


def case_decim(dev):
    """one round: the budget of F - 2 faces is one collapse"""
    from geobi_gnn_amd import meshdecim
    pts, faces, _ = _jittered_sphere(dev)
    r = meshdecim.decimate(pts, faces, target_faces=faces.shape[0] - 2, device=dev)
    assert r.counts['rounds'] == 1 and r.counts['collapses'] == 1
    return [r.points, r.faces, r.face_map, r.vertex_map, r.counts, meshdecim.apply(r, pts)]


def case_remesh(dev):
    """every single step once, each on the result of the one before: the collapsed mesh has the valences that flip"""
    from geobi_gnn_amd import meshremesh
    pts, faces, mean_edge = _jittered_sphere(dev)
    low, high = meshremesh.band(mean_edge)
    lock, lock_counts = meshremesh.lock_flags(pts, faces, device=dev)
    pts, faces, collapse_counts = meshremesh.collapse_short(pts, faces, low, high, lock=lock, device=dev)
    faces, flip_counts = meshremesh.flip_edges(pts, faces, device=dev)
    assert collapse_counts['collapses'] > 0 and flip_counts['flips'] > 0
    pts, relax_counts = meshremesh.relax(pts, faces, device=dev)
    assert relax_counts['moved'] > 0
    return [lock, lock_counts, collapse_counts, flip_counts, relax_counts, pts, faces,
            meshremesh.mesh_stats(pts, faces, low, high, device=dev)]


def case_fill(dev):
    """the sphere without three faces: three loops, found alone and then closed"""
    from geobi_gnn_amd import meshfill
    pts, faces = _sphere(dev)
    faces = faces[[f for f in range(faces.shape[0]) if f not in (0, 30, 60)]]
    loops = meshfill.boundary_loops(faces, pts.shape[0], device=dev)
    r = meshfill.fill_holes(pts, faces, device=dev)
    assert loops.counts['loops'] > 0 and r.counts['filled_loops'] > 0
    return [loops, r.points, r.faces, r.new_vertex_loop, r.new_face_loop, r.loops, r.counts]      # not r.ws, the plan's memory


def case_selfx(dev):
    """the sphere and two triangles that pass through it (and through each other)"""
    from geobi_gnn_amd import meshselfx
    pts, faces = _sphere(dev)
    V = pts.shape[0]
    extra = _t([[-2, -2, 0.1], [2, -2, 0.1], [0, 3, 0.1], [0.2, -2, -2], [0.2, 2, -2], [0.2, 0, 3]], dev, torch.float32)
    crossing = _t([[V, V + 1, V + 2], [V + 3, V + 4, V + 5]], dev, torch.int64)
    r = meshselfx.self_intersections(torch.cat([pts, extra]), torch.cat([faces, crossing]), max_pairs=65, device=dev)
    assert r.counts['pairs'] > 0
    return r


def case_sample(dev):
    from geobi_gnn_amd import meshsample
    pts, faces = _sphere(dev)
    out = [meshsample.sample_surface(pts, faces, 65, seed=11)]
    # 33 strips of 1 .. 3 faces over vertices of their own: two launches of the 32-part table
    n_faces = [1 + (k % 3) for k in range(33)]
    fptr = [0] + [int(v) for v in np.cumsum(n_faces)]
    first_vertex = np.cumsum([0] + [n + 2 for n in n_faces])
    union = torch.cat([_strip(n + 2, dev) + int(v0) for n, v0 in zip(n_faces, first_vertex)])
    out.append(meshsample.sample_surface_parts(_rand(dev, 8, int(first_vertex[-1]), 3), union, fptr, 5, seed=11,
                                               stream_ids=list(range(33))))
    return out


def case_grid(dev):
    """both grids over the sphere, 65 queries each; 2^18 + 1 queries: the rank scan of the search takes its temporary from
    rocPRIM"""
    from geobi_gnn_amd import meshgrid
    pts, faces = _sphere(dev)
    points, triangles = meshgrid.PointGrid(pts), meshgrid.TriangleGrid(pts, faces)
    q = _rand(dev, 9, 65, 3)
    return [points.cell_start, points.order, triangles.cell_start, triangles.order, triangles.records,
            points.nearest(q), triangles.nearest(q), points.nearest(_rand(dev, 10, BIG, 3))]


def case_meshprep(dev):
    from geobi_gnn_amd import meshprep
    out = []
    pts, faces = _sphere(dev)
    fv, V, F = faces.to(torch.int32).contiguous(), pts.shape[0], faces.shape[0]
    rowptr, lst = meshprep.vertex_faces(fv, V)
    g_v, g_f = meshprep.ring_graph(0, fv, rowptr, lst, V), meshprep.ring_graph(1, fv, rowptr, lst, F)
    fn, pos_f, vn = meshprep.mesh_normals(pts, fv, rowptr, lst)
    ptr33 = _t(np.linspace(0, V, 34).astype(np.int64), dev, torch.int32)          # 33 parts, none empty
    out += [rowptr, lst, g_v.rowptr_out, g_v.col_out, g_f.rowptr_out, g_f.col_out,
            meshprep.calc_weight(pts, vn, g_v, want_mean=True), meshprep.calc_weight(pos_f, fn, g_f),
            meshprep.mean_edge_length(pts, g_v), meshprep.calc_weight_parts(pts, vn, g_v, ptr33)]
    for n in (63, 64, 65, 66, 67):                  # V = n and F = n - 2: both kinds of ring graph cross 63 / 64 / 65
        fs = _strip(n, dev)
        rp, ls = meshprep.vertex_faces(fs, n)
        out += [rp, ls, meshprep.ring_graph_count(0, fs, rp, ls, n), meshprep.ring_graph_count(1, fs, rp, ls, n - 2)]
    out += list(meshprep.vertex_faces(_strip(67, dev), BIG))
    return out


def case_submesh(dev):
    from geobi_gnn_amd import patches
    pts, faces = _sphere(dev)
    fv = faces.to(torch.int32).contiguous()
    return [patches.submesh(fv, torch.arange(5, 5 + n, dtype=torch.int32, device=dev), pts.shape[0]) for n in COUNTS]


def case_mesheval(dev):
    from geobi_gnn_amd import mesheval
    pts, faces = _sphere(dev)
    out = []
    for n in COUNTS:
        q = _rand(dev, n, n, 3)
        d, i = mesheval.nearest_point(q, pts)
        out += [d, i, mesheval.point_to_mesh(q, pts, faces), mesheval.dist_summary(d)]
    return out


def _parts33(dev):
    sizes = np.array([1 + (k % 3) for k in range(33)])
    ptr = [0] + [int(v) for v in np.cumsum(sizes)]
    return _rand(dev, 1, ptr[-1], 3), _rand(dev, 2, ptr[-1], 3), ptr


def case_parts(dev):
    from geobi_gnn_amd import ops
    x, y, ptr = _parts33(dev)
    p = x.clone().requires_grad_(True)
    loss = ops.chamfer_loss(p, y, ptr, ptr)
    loss.backward()
    res = ops.icp(x, y, ptr, ptr, max_iterations=3)
    return [ops.nearest_parts(x, y, ptr, ptr), loss, p.grad, res.xt, res.state]


def case_filters(dev):
    from geobi_gnn_amd import filters
    pts, faces = _sphere(dev)
    noisy = pts + 0.02 * _rand(dev, 3, *pts.shape)
    return [filters.bilateral_normals(noisy, faces, normal_iters=3), filters.guided_normals(noisy, faces, normal_iters=3)]


def case_vertex_update(dev):
    from geobi_gnn_amd import data_util, meshprep
    pts, faces = _sphere(dev)
    fv = faces.to(torch.int32).contiguous()
    rowptr, lst = meshprep.vertex_faces(fv, pts.shape[0])
    fn = meshprep.mesh_normals(pts, fv, rowptr, lst)[0]
    return data_util.update_position2(pts + 0.02 * _rand(dev, 4, *pts.shape), faces,
                                      meshprep.vf_padded(rowptr, lst, pts.shape[0]), fn, n_iter=3)


def case_graph(dev):
    out = []
    for n in COUNTS:
        out += _graph_fields(_cycle(n, dev, symmetric=False).ensure_in())         # csr_from_coo and csr_transpose, E = n
    return out


def _pool_front_end(g, dev, seed):
    """matching, relabel, every SegmentIndex builder and both forms of pool_edge over one graph"""
    from geobi_gnn_amd import net_util, ops
    w = _rand(dev, seed, g.E).abs() + 0.1
    cluster, status, state = net_util.hip_match(g, w)
    cnew, count = net_util.relabel(cluster, rep_is_self=True)
    nseg = int(count.item())
    first = ops.SegmentIndex.from_matching(cnew, cluster, nseg)
    seg2 = torch.arange(nseg, dtype=torch.int32, device=dev) // 2
    second = ops.SegmentIndex(seg2, (nseg + 1) // 2)                              # segment_csr
    both = ops.SegmentIndex.compose(first, second, seg2[cnew.long()].contiguous())
    counters = torch.zeros(8, dtype=torch.int32, device=dev)
    raw, cnew2, sidx, state2 = net_util.hip_match_coarsen(g, w, counters)
    count_e, overflow = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    rows = net_util._pool_edge_rows(cnew2, sidx, g, w, counters[1:2], count_e, overflow)
    ne = int(count_e.item())
    general = net_util._pool_edge_raw(cnew2, g, w)
    ng = int(general[4].item())
    return [cluster, status, state, cnew, count, first.segptr, first.members, second.segptr, second.members, both.segptr,
            both.members, raw, cnew2, counters, state2, sidx.segptr[:int(counters[1].item()) + 1], sidx.members,
            rows[0][:nseg + 1], rows[1][:ne], rows[2][:ne], rows[3][:ne], count_e, overflow,
            general[0][:nseg + 1], general[1][:ng], general[2][:ng], general[3][:ng], general[4]]


def case_pool(dev):
    out = []
    for n in COUNTS:
        out += _pool_front_end(_cycle(n, dev), dev, n)
    return out


def case_pool_big(dev):
    """2^18 + 1: the scans of relabel and match_coarsen and the sort of segment_csr take their temporaries from rocPRIM"""
    from geobi_gnn_amd import net_util, ops
    g = _cycle(BIG, dev)
    w = _rand(dev, 5, g.E).abs() + 0.1
    counters = torch.zeros(8, dtype=torch.int32, device=dev)
    raw, cnew, sidx, state = net_util.hip_match_coarsen(g, w, counters)
    cnew_r, count = net_util.relabel(raw, rep_is_self=True)
    seg = torch.arange(BIG, dtype=torch.int32, device=dev) % 1000
    built = ops.SegmentIndex(seg, 1000)
    return [raw, cnew, state, counters, sidx.segptr[:int(counters[1].item()) + 1], sidx.members, cnew_r, count,
            built.segptr, built.members]


def _feast(dev, Cin, Cout, grad, fused=True):
    from geobi_gnn_amd import ops
    if not fused:                           # the path that writes the aggregated rows z and runs the node GEMM
        was, ops.FUSED = ops.FUSED, False
        try:
            return _feast(dev, Cin, Cout, grad)
        finally:
            ops.FUSED = was
    g = _cycle(65, dev)
    x = _rand(dev, 6, 65, Cin).requires_grad_(grad)
    prm = [(0.1 * _rand(dev, 7 + k, *shape)).requires_grad_(grad)
           for k, shape in enumerate(((9 * Cout, Cin), (9, Cin), (9,), (Cout,)))]
    with torch.set_grad_enabled(grad):
        out = ops.feast_conv(x, g, prm[0], prm[1], prm[2], prm[3], slope=0.2)
    if not grad:
        return [out]
    (out * _rand(dev, 11, 65, Cout)).sum().backward()
    return [out, x.grad] + [p.grad for p in prm]


def case_feast_small(dev):
    return _feast(dev, 6, 32, False) + _feast(dev, 6, 32, True)


def case_feast_wide(dev):
    return _feast(dev, 128, 128, False, fused=False) + _feast(dev, 128, 128, True)


def _head(dev, Cin, K):
    from geobi_gnn_amd import ops
    x = _rand(dev, 12, 65, Cin).requires_grad_(True)
    prm = [(0.1 * _rand(dev, 13 + k, *shape)).requires_grad_(True) for k, shape in enumerate(((K, Cin), (K,), (3, K), (3,)))]
    out = ops.apply_op(ops.HeadFn, x, prm[0], prm[1], prm[2], prm[3], 1, None, None)
    (out * _rand(dev, 17, 65, 3)).sum().backward()
    return [out, x.grad] + [p.grad for p in prm]


def case_head_fused(dev):
    return _head(dev, 32, 1024)


def case_head_unfused(dev):
    return _head(dev, 8, 2048)


def case_row_loss(dev):
    from geobi_gnn_amd import ops
    # 65 * 1024 + 1 rows: 66 partial sums, the first count whose size (264 bytes, aligned, + 256) is above 512
    return [ops.row_loss(_rand(dev, n, n, 3), _rand(dev, n + 1, n, 3), 0) for n in COUNTS + (65 * 1024 + 1,)]


CASES = {f.__name__[5:]: f for f in (case_clean, case_topo, case_subdiv, case_decim, case_remesh, case_fill, case_selfx, case_sample,
                                     case_grid, case_meshprep, case_submesh, case_mesheval, case_parts,
                                     case_filters, case_vertex_update, case_graph, case_pool, case_pool_big,
                                     case_feast_small, case_feast_wide, case_head_fused, case_head_unfused, case_row_loss)}

# (case, entry point, which of the case's requests for that entry point): the requests that cannot fail 512 bytes short.
# The forward without a gradient comes first in the FeaSt cases (fused at (6, 32), where the fused path sets the size;
# unfused at (128, 128), where the unfused one does) and must fail like every other request.
TAKES_LESS = {
    # the forward with a gradient: the weights go to the buffer kept for the backward, the fused forward takes nothing
    # from its workspace
    ('feast_small', 'geobi_feast_fwd', 1), ('feast_wide', 'geobi_feast_fwd', 1),
    # geobi_feast_bwd_ws_bytes is the size of ANY path (dz and a recomputed z, [N, 9 Cin] each); these shapes take the
    # fused row pass and want an input gradient, so neither array is taken
    ('feast_small', 'geobi_feast_bwd', 0), ('feast_wide', 'geobi_feast_bwd', 0),
}

_REF = {}


def _reference(name, dev):
    if name not in _REF:
        _REF[name] = _flat(CASES[name](dev), [])
        torch.cuda.synchronize()
    return _REF[name]


@pytest.mark.parametrize('name', sorted(CASES))
def test_guard_band(name, dev, monkeypatch):
    """No launcher writes behind the size its query gave, and the carve's layout does not change a result."""
    want = _reference(name, dev)
    guard = _Guarded().install(monkeypatch)
    got = _flat(CASES[name](dev), [])
    assert guard.requests, 'the case asked for no workspace'
    assert all(nbytes > 0 for _, _, nbytes in guard.requests), 'a size query answered 0'
    assert guard.sentinels_whole(), 'a launcher wrote behind its workspace'
    assert got == want, 'outputs differ from the call made with the library allocator'


@pytest.mark.parametrize('name', sorted(CASES))
def test_short_workspace(name, dev, monkeypatch):
    """Every launcher refuses a workspace 512 bytes short of its size, naming itself and both sizes."""
    from geobi_gnn_amd import _lib
    want = _reference(name, dev)
    probe = _Guarded().install(monkeypatch)
    CASES[name](dev)
    raised = 0
    for k, (_, _, nbytes) in enumerate(probe.requests):
        if nbytes <= SHORT_BY:
            continue
        guard = _Guarded(short_at=k).install(monkeypatch)
        try:
            got, err = _flat(CASES[name](dev), []), None
        except _lib.GeobiError as e:
            got, err = None, str(e)
        assert guard.sentinels_whole(), 'request %d: a launcher wrote behind the end it was given' % k
        give, entry = guard.requests[k][1], guard.entries[k]
        print('%s request %d %s: %d of %d bytes -> %s' % (name, k, entry, give, nbytes, err))
        nth = sum(1 for j in range(k) if guard.entries[j] == entry)
        if (name, entry, nth) in TAKES_LESS:
            assert err is None and got == want, (k, entry, err)
            continue
        assert err is not None, 'request %d (%s): %d of %d bytes were accepted' % (k, entry, give, nbytes)
        m = re.search(r'(\w+): workspace too small \((\d+) bytes given, (\d+) needed\)', err)
        assert m, err
        assert 'geobi_' + m.group(1) == entry and entry + ' failed' in err, err
        assert int(m.group(2)) == give and give < int(m.group(3)) <= nbytes, err
        raised += 1
    assert raised > 0
