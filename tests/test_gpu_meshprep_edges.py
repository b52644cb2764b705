"""The mesh-preprocessing kernels (csrc/meshprep.hip behind meshprep.py), one at a time, against the fp64 model of
tests/meshprep_model.py on the meshes where such kernels go wrong: valence 300, non-manifold vertices and edges, duplicated
and reversed faces, exactly degenerate faces, face-less vertices (also as the last thread blocks), coordinates far from the
origin, other units (the weights' exponent grows with the unit), the clamp of the normal product, the path boundaries of the
scan, and unions with empty, edge-less and large parts.  Then the whole of build_dual_data / refresh_dual_data.

Bars (eps = 2^-24), derived from the arithmetic and not from what the kernels give:
    integers       exact; two runs of everything are bit-identical
    face normal    2^-23 per component where |e1 x e2| >= 1e-6 |e1| |e2| (fp64 kernel, one cast); constructed flat faces give 0
    centroid       3 eps max|coordinate| per component: (a + b) + c in fp32 is off by <= (2 + 3) eps max, a third of that
                   after the division, whose own rounding adds <= 1 eps max
    vertex normal  2^-23 + 1e-13 / |s| where the model's |s| >= 1e-3; finite and norm <= 1 + 2^-22 at the cancelling vertices,
                   which are exactly the ones `doubled` constructs; exactly 0 at a face-less vertex
    mean, scale    6 eps relative, on the raw fp32 points: dx, the squares, the sums and sqrtf come to about 4 eps, one cast
                   (scale: one more division)
    weight         ex (4 eps + dn (8 + 6 |arg|) eps) + 2^-126 (meshprep_model.Weights.tol)
The worst err / tol per quantity and family is printed at the end of the module (DESIGN.md section 4b holds the table)."""
import collections

import numpy as np
import pytest
import torch

import meshprep_model as M

pytestmark = pytest.mark.gpu

EPS = M.EPS
WORST = collections.OrderedDict()       # (quantity, family) -> worst err / tol seen


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    yield torch.device('cuda:0')
    if WORST:
        print('\nworst err / tol per quantity and family')
        for (quantity, family), r in WORST.items():
            print('  %-14s %-10s %.3f' % (quantity, family, r))


def _family(name):
    if name.startswith('unit') or name.startswith('shifted') or name in ('rough', 'parts'):
        return name
    return 'scan' if name.startswith('scan') else 'topology'


def _bar(quantity, name, err, tol):
    """err <= tol everywhere; keeps the worst ratio."""
    err, tol = np.asarray(err, dtype=np.float64), np.asarray(tol, dtype=np.float64)
    ratio = float((err / tol).max()) if err.size else 0.0
    key = (quantity, _family(name))
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    assert np.isfinite(err).all() and ratio <= 1.0, '%s of %s: err / tol = %.3f' % (quantity, name, ratio)


_MODELS = {}


def _model(name):
    """Mesh + everything the model says about it that does not depend on device results; built once per module."""
    if name not in _MODELS:
        m = M.SMALL[name]() if name in M.SMALL else M.scan_grid(name)
        rowptr, lst = M.vertex_faces(m.faces, m.V)
        m.rowptr, m.lst = rowptr, lst
        m.vf = M.vf_padded(rowptr, lst)
        m.graph = [M.ring_graph(kind, m.faces, m.V, rowptr, lst) for kind in (0, 1)]
        _MODELS[name] = m
    return _MODELS[name]


def _np(t):
    return t.detach().cpu().numpy()


def _run_kernels(dev, m):
    """Every kernel once, through its own wrapper -> dict of host arrays."""
    from geobi_gnn_amd import meshprep as P
    pts, fv = torch.from_numpy(m.points).to(dev), torch.from_numpy(m.faces).to(dev)
    rowptr, lst = P.vertex_faces(fv, m.V)
    vf = P.vf_padded32(rowptr, lst, m.V)
    fn, cen, vn = P.mesh_normals(pts, fv, rowptr, lst)
    g_v = P.ring_graph(0, fv, rowptr, lst, m.V)
    g_f = P.ring_graph(1, fv, rowptr, lst, m.F)
    w_v, mean_v = P.calc_weight(pts, vn, g_v, want_mean=True)
    w_f, mean_f = P.calc_weight(cen, fn, g_f, want_mean=True)
    out = dict(rowptr=rowptr, lst=lst, vf=vf, fn=fn, cen=cen, vn=vn, rp_v=g_v.rowptr_out, row_v=g_v.ensure_rows(),
               col_v=g_v.col_out, rp_f=g_f.rowptr_out, row_f=g_f.ensure_rows(), col_f=g_f.col_out, w_v=w_v, w_f=w_f,
               mean_v=mean_v, mean_f=mean_f, mean_edge=P.mean_edge_length(pts, g_v))
    out = {k: _np(v) for k, v in out.items()}
    out['E'] = (g_v.E, g_f.E)
    return out


def _check_integers(m, d):
    assert np.array_equal(d['rowptr'], m.rowptr) and np.array_equal(d['lst'], m.lst)
    assert d['vf'].shape == m.vf.shape and np.array_equal(d['vf'], m.vf)          # the width is the largest valence
    for tag, (rp, row, col), E in zip('vf', m.graph, d['E']):
        assert E == rp[-1] == d['col_' + tag].shape[0]
        assert np.array_equal(d['rp_' + tag], rp) and np.array_equal(d['col_' + tag], col)
        assert np.array_equal(d['row_' + tag], row)


@pytest.mark.parametrize('name', sorted(M.SMALL))
def test_kernels_against_the_model(dev, name):
    m = _model(name)
    d = _run_kernels(dev, m)
    _check_integers(m, d)
    again = _run_kernels(dev, m)
    for k in d:
        assert d[k].tobytes() == again[k].tobytes() if k != 'E' else d[k] == again[k], k

    # face normals and centroids
    cross, scale = M.face_cross(m.points, m.faces)
    fn = M.face_normals(m.points, m.faces)
    sound = np.sqrt((cross * cross).sum(1)) >= 1e-6 * scale
    _bar('face normal', name, np.abs(d['fn'] - fn)[sound], 2.0 ** -23)
    flat = getattr(m, 'flat_faces', np.zeros(0, dtype=np.int64))
    assert np.array_equal(np.nonzero(~sound)[0], flat) and not d['fn'][flat].any()
    corner = np.abs(m.points.astype(np.float64)[m.faces]).max(1)                   # [F, 3]: per component over the corners
    _bar('centroid', name, np.abs(d['cen'] - M.centroids(m.points, m.faces)), 3 * EPS * corner + 2.0 ** -149)

    # vertex normals
    vn, norm = M.vertex_normals(m.points, m.faces, m.rowptr, m.lst)
    has_faces = np.diff(m.rowptr) > 0
    good = has_faces & (norm >= 1e-3)
    _bar('vertex normal', name, np.abs(d['vn'] - vn)[good], (2.0 ** -23 + 1e-13 / norm[good])[:, None])
    assert np.array_equal(np.nonzero(has_faces & ~good)[0], m.cancelling)
    assert m.cancelling.size == (2 if name == 'doubled' else 0)
    rest = d['vn'][m.cancelling].astype(np.float64)
    assert np.isfinite(d['vn']).all() and (np.sqrt((rest * rest).sum(1)) <= 1 + 2.0 ** -22).all()
    assert not d['vn'][~has_faces].any()

    # mean edge lengths: the mesh edges alone (1 / scale), and either graph with its self loops in the denominator
    (_, row_v, col_v), (_, row_f, col_f) = m.graph
    for key, pos, row, col, extra in (('mean_edge', m.points, row_v, col_v, 0), ('mean_v', m.points, row_v, col_v, m.V),
                                      ('mean_f', d['cen'], row_f, col_f, m.F)):
        ref = M.mean_edge_length(pos, row, col, extra)
        assert d[key].shape == (1,)
        _bar('mean length', name, abs(float(d[key][0]) - ref), 6 * EPS * ref + (ref == 0) * 1e-300)

    # weights, from the fp32 positions and normals the weight kernel read
    for tag, pos, nrm, row, col, n in (('v', m.points, d['vn'], row_v, col_v, m.V), ('f', d['cen'], d['fn'], row_f, col_f, m.F)):
        w = M.calc_weight(pos, nrm, row, col, extra=n)
        _bar('weight', name, np.abs(d['w_' + tag] - w.w), w.tol())
    if name == 'unit400':
        assert (d['w_v'] == 0).mean() > 0.9                                       # the underflow is a clean zero
    if name == 'rough':
        assert (d['w_v'] <= np.float32(0.001)).mean() > 0.05


@pytest.fixture(scope='module', params=sorted(M.SCAN_GRIDS))
def scan_case(request):
    """The model of a scan-boundary grid, built outside the test that compares."""
    return _model(request.param)


def test_scan_path_boundaries(dev, scan_case):
    """V + 1 = 2^14 (last one-block scan), 2^14 + 1 (first look-back), 2^18 (last look-back), 2^18 + 1 (first rocPRIM)."""
    from geobi_gnn_amd import meshprep as P
    m = scan_case
    fv = torch.from_numpy(m.faces).to(dev)
    rowptr, lst = P.vertex_faces(fv, m.V)
    vf = P.vf_padded32(rowptr, lst, m.V)
    assert np.array_equal(_np(rowptr), m.rowptr) and np.array_equal(_np(lst), m.lst)
    assert tuple(vf.shape) == m.vf.shape == (m.V, 6) and np.array_equal(_np(vf), m.vf)
    for kind, n in ((0, m.V), (1, m.F)):
        g = P.ring_graph(kind, fv, rowptr, lst, n)
        rp, _, col = m.graph[kind]
        assert g.E == rp[-1] and np.array_equal(_np(g.rowptr_out), rp) and np.array_equal(_np(g.col_out), col)


# ------------------------------------------------------------------------------------------------ calc_weight_parts
def _part(m, kind):
    """(pos, normal, rowptr, row, col) of one graph of a mesh, from the model (fp32 as the device would hold them)."""
    rp, row, col = M.ring_graph(kind, m.faces, m.V)
    if kind == 0:
        return m.points, M.vertex_normals(m.points, m.faces)[0].astype(np.float32), rp, row, col
    return M.centroids(m.points, m.faces).astype(np.float32), M.face_normals(m.points, m.faces).astype(np.float32), rp, row, col


def _graph(dev, n, rp, row, col):
    from geobi_gnn_amd.graph import Graph
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    return Graph.from_sorted(n, t(rp), t(row), t(col), symmetric=True)


def _union(parts):
    """parts: list of _part tuples or None (a part without nodes) -> (pos, normal, rowptr, row, col, node_ptr)."""
    pos, nrm, rps, rows, cols, ptr, off, eoff = [], [], [], [], [], [0], 0, 0
    for p in parts:
        if p is not None:
            pos.append(p[0]); nrm.append(p[1]); rps.append(p[2][:-1] + eoff); rows.append(p[3] + off); cols.append(p[4] + off)
            off, eoff = off + p[0].shape[0], eoff + p[3].shape[0]
        ptr.append(off)
    return (np.concatenate(pos), np.concatenate(nrm), np.concatenate(rps + [np.asarray([eoff])]), np.concatenate(rows),
            np.concatenate(cols), np.asarray(ptr))


def _weights_of_union(dev, u):
    from geobi_gnn_amd import meshprep as P
    pos, nrm, rp, row, col, ptr = u
    g = _graph(dev, pos.shape[0], rp, row, col)
    node_ptr = torch.from_numpy(ptr.astype(np.int32)).to(dev)
    return _np(P.calc_weight_parts(torch.from_numpy(pos).to(dev), torch.from_numpy(nrm).to(dev), g, node_ptr))


def _weights_alone(dev, p):
    from geobi_gnn_amd import meshprep as P
    pos, nrm, rp, row, col = p
    g = _graph(dev, pos.shape[0], rp, row, col)
    return _np(P.calc_weight(torch.from_numpy(pos).to(dev), torch.from_numpy(nrm).to(dev), g))


def test_parts_empty_edgeless_and_beyond_one_sweep(dev):
    big = _part(M.grid(112, 112, edge=2.0, seed=4), 0)
    assert big[3].shape[0] > 256 * 256                            # a second sweep of the 256 x 256 stride loop
    lone = _part(M.single(), 1)
    assert lone[0].shape[0] == 1 and lone[3].shape[0] == 0        # one node, no edge
    parts = [None, _part(M.bowtie(), 0), lone, _part(M.unit_grid(20.0), 1), None, big, _part(M.book(), 0),
             _part(M.doubled(), 1), lone, _part(M.two_disjoint(), 0), None]
    u = _union(parts)
    got = _weights_of_union(dev, u)
    assert got.tobytes() == _weights_of_union(dev, u).tobytes()
    ref = M.calc_weight_parts(*u)
    _bar('weight', 'parts', np.abs(got - ref.w), ref.tol())
    e = 0
    for p in parts:
        if p is not None:
            n = p[3].shape[0]
            assert got[e:e + n].tobytes() == _weights_alone(dev, p).tobytes()
            e += n
    assert e == got.shape[0]


def _triangles(n, seed=7):
    """n triangles of their own size and place, as vertex graphs."""
    rng = np.random.RandomState(seed)
    size = np.exp(rng.uniform(np.log(1e-2), np.log(30.0), (n, 1, 1)))
    pos = (rng.uniform(-1, 1, (n, 3, 3)) * size + 10 * rng.uniform(-1, 1, (n, 1, 3))).astype(np.float32)
    nrm = rng.standard_normal((n, 3, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=2, keepdims=True)).astype(np.float32)
    rp = np.asarray([0, 2, 4, 6])
    row, col = np.asarray([0, 0, 1, 1, 2, 2]), np.asarray([1, 2, 0, 2, 0, 1])
    return [(pos[i], nrm[i], rp, row, col) for i in range(n)]


def test_part_count_limit(dev):
    from geobi_gnn_amd._lib import GeobiError
    tris = _triangles(4097)
    u = _union(tris[:4096])
    got = _weights_of_union(dev, u)
    ref = M.calc_weight_parts(*u)
    _bar('weight', 'parts', np.abs(got - ref.w), ref.tol())
    for i in (0, 2047, 4095):
        assert got[6 * i:6 * i + 6].tobytes() == _weights_alone(dev, tris[i]).tobytes()
    with pytest.raises(GeobiError):
        _weights_of_union(dev, _union(tris))
    torch.cuda.synchronize()                                       # refused on the host: nothing ran, nothing faulted


def test_loud_errors(dev):
    from geobi_gnn_amd import meshprep as P
    from geobi_gnn_amd._lib import GeobiError
    pts = M.single().points
    none = np.zeros((0, 3), dtype=np.int64)
    for p, f in ((pts, none), (pts[:0], [[0, 1, 2]]), (pts[:0], none), (pts, [[0, 1, 3]]), (pts, [[0, -1, 2]])):
        with pytest.raises(GeobiError):
            P.build_dual_data(p, np.asarray(f, dtype=np.int64).reshape(-1, 3), device=dev)
    # an int64 id that the conversion to int32 would wrap into range (2^32 + 1 -> 1) is refused as it arrives
    p4 = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], dtype=np.float32)
    wrap = np.array([[0, 1, 2], [1, 2, 2 ** 32 + 1]], dtype=np.int64)
    for f in (wrap, torch.from_numpy(wrap), torch.from_numpy(wrap).to(dev)):
        with pytest.raises(GeobiError, match='outside'):
            P.build_dual_data(p4, f, device=dev)
    torch.cuda.synchronize()
    dv, df = P.build_dual_data(pts, np.asarray([[0, 1, 2]]), device=dev)           # and the device is as it was
    assert dv.graph().E == 6 and df.graph().E == 0


# ------------------------------------------------------------------------------------------------ the whole path
@pytest.mark.parametrize('name', ['fan300', 'bowtie', 'doubled', 'shifted', 'unit50'])
def test_build_and_refresh_dual_data(dev, name):
    from geobi_gnn_amd import meshprep as P
    m = _model(name)
    d = _run_kernels(dev, m)
    faces64 = m.faces.astype(np.int64)
    dv, df = P.build_dual_data(m.points, faces64, device=dev, reference_layout=False)
    # integers: graphs, padded incidence
    for data, (rp, row, col), n in ((dv, m.graph[0], m.V), (df, m.graph[1], m.F)):
        g = data.graph()
        assert g.N == n and g.E == rp[-1] and g.symmetric
        assert np.array_equal(_np(g.rowptr_out), rp) and np.array_equal(_np(g.col_out), col)
        assert np.array_equal(_np(data.edge_index), np.stack([row, col]))
    assert np.array_equal(_np(dv.meta['vf_indices']), m.vf) and np.array_equal(_np(df.fv_indices), faces64)
    # what the kernels gave one at a time is what the whole path holds, bit for bit (those were held to the model above)
    x_v, x_f = _np(dv.x), _np(df.x)
    assert x_v[:, 3:].tobytes() == d['vn'].tobytes() and x_f[:, 3:].tobytes() == d['fn'].tobytes()
    assert _np(dv.edge_weight).tobytes() == d['w_v'].tobytes() and _np(df.edge_weight).tobytes() == d['w_f'].tobytes()
    for tag, pos, nrm, (_, row, col), n, data in (('v', m.points, d['vn'], m.graph[0], m.V, dv),
                                                  ('f', d['cen'], d['fn'], m.graph[1], m.F, df)):
        w = M.calc_weight(pos, nrm, row, col, extra=n)
        _bar('weight', name, np.abs(_np(data.edge_weight) - w.w), w.tol())
    # scale, and the features around the centroid the device took.  The centroid is torch's mean, in an order of its own:
    # any order of V fp32 additions stays within (V - 1) eps mean|p|, and the division adds one rounding.
    cen32 = _np(dv.meta['centroid'])
    p64 = m.points.astype(np.float64)
    assert (np.abs(cen32 - p64.mean(0)) <= m.V * EPS * np.abs(p64).mean(0)).all()
    mx_v, mx_f, scale = M.dual_features(m.points, m.faces, cen32, d['vn'], d['fn'], m.graph[0])
    _bar('scale', name, abs(dv.meta['scale'] - scale), 6 * EPS * scale)
    # x = fl(fl(p - c) * scale): one rounding each, scale within 6 eps; a facet's p is its fp32 centroid (3 eps max|corner|)
    _bar('x position', name, np.abs(x_v[:, :3] - mx_v[:, :3]), 9 * EPS * np.abs(mx_v[:, :3]) + 2.0 ** -126)
    corner = np.abs(p64[m.faces]).max(1)
    _bar('x position', name, np.abs(x_f[:, :3] - mx_f[:, :3]),
         9 * EPS * np.abs(mx_f[:, :3]) + 3 * EPS * corner * scale * (1 + 9 * EPS) + 2.0 ** -126)

    # a refresh onto the same points is the build again
    ev, ef = P.build_dual_data(m.points + np.float32(0.25), faces64, device=dev)
    P.refresh_dual_data(ev, ef, m.points, None)
    for a, b in ((ev, dv), (ef, df)):
        assert torch.equal(a.x, b.x) and torch.equal(a.edge_weight, b.edge_weight)
        assert _np(a.x).tobytes() == _np(b.x).tobytes() and _np(a.edge_weight).tobytes() == _np(b.edge_weight).tobytes()
    assert ev.meta['scale'] == dv.meta['scale'] and torch.equal(ev.meta['centroid'], dv.meta['centroid'])
