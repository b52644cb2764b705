"""The index builders under every kernel -- geobi_csr_from_coo, geobi_csr_transpose, geobi_csr_reverse_index,
geobi_expand_rowptr, geobi_gather_f32, geobi_segment_csr, geobi_concat32 -- through the C ABI against the plain model of
tests/graph_model.py, and the two layers on top of them: data.union_batch_graphs at 12 and 40 prepared meshes (two and
four launches of 96 copy segments) and the FeaSt kernels on a symmetric multigraph, where the reverse-edge index is no
permutation.  tests/test_graph_model_host.py keeps the model and the cases honest.

Every integer output is compared EXACTLY and every float bit for bit; every output is filled with a poison word before
the call and carries GUARD poisoned words past its end, which must survive.  The only tolerance of the file is the per-row
bar of feast_cases (1e-5 of the fp64 oracle) in the FeaSt test, whose second half is again bit for bit.

Cases per entry point: csr_from_coo 108 (27 inputs x drop_self x bad counter given / NULL), csr_transpose 30 calls
(7 inputs x their paddings x inv_pos given / NULL), csr_reverse_index 10 (6 inputs, flag NULL on the four symmetric
ones), expand_rowptr 5, gather_f32 5, segment_csr 13, concat32 16 (7 segment counts and the 4.2 M-element launch, int32
and float), union_batch_graphs 2, FeaSt 9 (3 shapes x 3 launch geometries), each on both paths to pos_in.
"""
import ctypes

import numpy as np
import pytest
import torch

import feast_cases as F
import graph_model as M

pytestmark = pytest.mark.gpu

COO = M.coo_cases()
TRANSPOSE = M.transpose_cases()
REVERSE = M.reverse_cases()
SEGMENT = M.segment_cases()


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


def _L():
    from geobi_gnn_amd import _lib
    return _lib


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def _i64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


def _out(dev, n):
    """n poisoned int32 words and GUARD more behind them"""
    return torch.full((n + M.GUARD,), M.POISON, dtype=torch.int32, device=dev)


def _read(t, n, what):
    """the first n words of an output; the guard behind them must be untouched"""
    a = t.cpu().numpy()
    assert a.size == n + M.GUARD and np.all(a[n:] == M.POISON), '%s: written past its end' % what
    return a[:n]


# ============================================================================================ geobi_csr_from_coo
@pytest.mark.parametrize('with_bad', [True, False])
@pytest.mark.parametrize('drop_self', [0, 1])
@pytest.mark.parametrize('name', sorted(COO))
def test_csr_from_coo(dev, name, drop_self, with_bad):
    """rowptr, the kept part of col and eid, the -1 tail of col and the whole of eid (a permutation of range(E), dropped
    pairs last in input order) equal the model; bad[0] is the exact count of pairs with an id outside [0, N) -- the ids
    -2^40 and 2^40 + 3 among them, whose low words are valid ids -- and with bad = NULL they are dropped all the same."""
    L = _L()
    c = COO[name]
    seg, nbr, N = c['seg'], c['nbr'], c['N']
    E = seg.size
    rowptr, col, eid, bad = _out(dev, N + 1), _out(dev, E), _out(dev, E), _out(dev, 1)
    s, b = _i64(seg, dev), _i64(nbr, dev)
    ws = L.workspace(L.size_query('geobi_csr_ws_bytes', E, N), dev)
    L.call('geobi_csr_from_coo', L.ptr(s) if E else None, L.ptr(b) if E else None, E, N, drop_self, L.ptr(rowptr),
           L.ptr(col), L.ptr(eid), L.ptr(bad) if with_bad else None, L.ptr(ws), ws.numel(), L.stream())
    m_rowptr, m_col, m_eid, m_bad = M.csr_from_coo_slots(seg, nbr, N, drop_self)
    assert np.array_equal(_read(rowptr, N + 1, 'rowptr'), m_rowptr)
    assert np.array_equal(_read(col, E, 'col'), m_col)
    assert np.array_equal(_read(eid, E, 'eid'), m_eid)
    assert _read(bad, 1, 'bad')[0] == (m_bad if with_bad else M.POISON)


# =========================================================================================== geobi_csr_transpose
@pytest.mark.parametrize('name', sorted(TRANSPOSE))
def test_csr_transpose(dev, name):
    """Ecap = E, E + 1, E + 300 (per case): rowptr_t, col_t and pos_t with their -1 tails equal the model; inv_pos is the
    inverse of pos_t on [0, E) and keeps its poison on [E, Ecap); inv_pos = NULL changes nothing else.  rowptr[N] never
    exceeds Ecap (outside the contract: the kernels would write past the arrays)."""
    L = _L()
    c = TRANSPOSE[name]
    N, E = c['N'], c['E']
    rowptr = _i32(c['rowptr'], dev)
    for pad in c['pads']:
        Ecap = E + pad
        assert int(c['rowptr'][N]) <= Ecap
        col = _i32(np.concatenate([c['col'], -np.ones(pad, dtype=np.int64)]), dev)
        m_rowptr, m_col, m_pos, m_inv = M.csr_transpose(c['rowptr'], c['col'], N, Ecap)
        for with_inv in (True, False):
            rowptr_t, col_t, pos_t, inv = _out(dev, N + 1), _out(dev, Ecap), _out(dev, Ecap), _out(dev, Ecap)
            ws = L.workspace(L.size_query('geobi_csr_ws_bytes', Ecap, N), dev)
            L.call('geobi_csr_transpose', L.ptr(rowptr), L.ptr(col) if Ecap else None, N, Ecap, L.ptr(rowptr_t),
                   L.ptr(col_t), L.ptr(pos_t), L.ptr(inv) if with_inv else None, L.ptr(ws), ws.numel(), L.stream())
            tag = '%s Ecap = E + %d, inv_pos %s' % (name, pad, 'given' if with_inv else 'NULL')
            assert np.array_equal(_read(rowptr_t, N + 1, 'rowptr_t'), m_rowptr), tag
            assert np.array_equal(_read(col_t, Ecap, 'col_t'), m_col), tag
            assert np.array_equal(_read(pos_t, Ecap, 'pos_t'), m_pos), tag
            got = _read(inv, Ecap, 'inv_pos')
            assert np.array_equal(got[:E], m_inv if with_inv else np.full(E, M.POISON)), tag
            assert np.all(got[E:] == M.POISON), tag


# ======================================================================================= geobi_csr_reverse_index
@pytest.mark.parametrize('name', sorted(REVERSE))
def test_csr_reverse_index(dev, name):
    """pos_rev is the FIRST position of the reverse entry (a multigraph: the first of the run) and -1 at exactly the
    entries without one; the poisoned flag comes back 0 or 1, 0 for E = 0; flag = NULL on the symmetric inputs."""
    L = _L()
    c = REVERSE[name]
    N, E = c['N'], c['col'].size
    rowptr, col = _i32(c['rowptr'], dev), _i32(c['col'], dev)
    row = _i32(M.rows_of(c['rowptr']), dev)
    m_pos, m_flag = M.reverse_index(c['rowptr'], c['col'])
    for with_flag in (True, False) if m_flag == 0 else (True,):
        pos, flag = _out(dev, E), _out(dev, 1)
        L.call('geobi_csr_reverse_index', L.ptr(rowptr), L.ptr(row) if E else None, L.ptr(col) if E else None, E,
               L.ptr(pos), L.ptr(flag) if with_flag else None, L.stream())
        assert np.array_equal(_read(pos, E, 'pos_rev'), m_pos), name
        assert _read(flag, 1, 'flag')[0] == (m_flag if with_flag else M.POISON), name
    if c['missing'] is not None:
        assert int((m_pos < 0).sum()) == c['missing']


# ============================================================ geobi_expand_rowptr / geobi_gather_f32 / geobi_segment_csr
@pytest.mark.parametrize('N', M.EXPAND_N)
def test_expand_rowptr(dev, N):
    L = _L()
    rowptr = M.expand_case(N)
    E = int(rowptr[N])
    row, rp = _out(dev, E), _i32(rowptr, dev)
    L.call('geobi_expand_rowptr', L.ptr(rp), N, L.ptr(row), L.stream())
    assert np.array_equal(_read(row, E, 'row'), M.expand_rowptr(rowptr))


@pytest.mark.parametrize('n', M.GATHER_N)
def test_gather_f32(dev, n):
    """a copy of the bits: -0.0, +-inf, NaNs with a payload and a subnormal arrive as they are, index < 0 gives +0.0"""
    L = _L()
    src, idx = M.gather_case(n)
    dst, s, k = _out(dev, n), torch.from_numpy(src).to(dev), _i32(idx, dev)
    L.call('geobi_gather_f32', L.ptr(s), L.ptr(k), n, L.ptr(dst), L.stream())
    got = _read(dst, n, 'dst').view(np.uint32)
    assert np.array_equal(got, M.gather_f32(src, idx).view(np.uint32))
    assert np.all(got[idx < 0] == 0)


@pytest.mark.parametrize('name', sorted(SEGMENT))
def test_segment_csr(dev, name):
    L = _L()
    seg, nseg = SEGMENT[name]
    n = seg.size
    segptr, members, ids = _out(dev, nseg + 1), _out(dev, n), _i32(seg, dev)
    ws = L.workspace(L.size_query('geobi_segment_csr_ws_bytes', n), dev)
    L.call('geobi_segment_csr', L.ptr(ids) if n else None, n, nseg, L.ptr(segptr), L.ptr(members), L.ptr(ws),
           ws.numel(), L.stream())
    m_segptr, m_members = M.segment_csr(seg, nseg)
    assert np.array_equal(_read(segptr, nseg + 1, 'segptr'), m_segptr)
    assert np.array_equal(_read(members, n, 'members'), m_members)


# ================================================================================================= geobi_concat32
def _concat(dev, segs, is_float):
    """One geobi_concat32 call.  The sources are slices of ONE array and the destinations are adjacent in another, so
    one element too many lands in the neighbour's first word (or in the guard).  -> the destination with its guard"""
    from geobi_gnn_amd.data import _CopySeg
    L = _L()
    srcs = [np.ascontiguousarray(s[0]).view(np.int32) for s in segs if s[0] is not None]
    pool = _i32(np.concatenate(srcs + [np.full(M.GUARD, M.POISON, dtype=np.int32)]), dev)
    total = sum(s[1] for s in segs)
    dst = _out(dev, total)
    jobs, so, do = [], 0, 0
    for src, n, add, value in segs:
        jobs.append(_CopySeg(None if src is None else pool.data_ptr() + 4 * so, dst.data_ptr() + 4 * do, n, add, value))
        so += 0 if src is None else n
        do += n
    arr = (_CopySeg * len(jobs))(*jobs)
    L.call('geobi_concat32', ctypes.cast(arr, ctypes.c_void_p), len(jobs), is_float, L.stream())
    return _read(dst, total, 'dst').view(np.uint32)


@pytest.mark.parametrize('is_float', [0, 1])
@pytest.mark.parametrize('count', M.CONCAT_COUNTS)
def test_concat32(dev, count, is_float):
    """1 .. 300 segments (one to four launches of 96) of 0 .. 1025 elements; empty ones first, last and, from 192
    segments on, four in a row across the first launch edge, while the other edges fall between segments that hold
    something; fills, adds of both signs up to +-2^31 (wrapping), float sources with NaN payloads and -0.0."""
    segs = M.concat_case(count, is_float)
    want = np.concatenate(M.concat32(segs, is_float))
    got = _concat(dev, segs, is_float)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, 'first difference at element %d of %d (%d differ)' % (bad[0], want.size, bad.size)


@pytest.mark.parametrize('is_float', [0, 1])
def test_concat32_grid_stride(dev, is_float):
    """4 200 009 elements in one launch: more than 4096 blocks x 1024, so the grid-stride loop runs twice"""
    segs = M.concat_case(len(M.BIG_LENGTHS), is_float, lengths=M.BIG_LENGTHS)
    assert sum(s[1] for s in segs) > 4096 * 1024
    want = np.concatenate(M.concat32(segs, is_float))
    assert np.array_equal(_concat(dev, segs, is_float), want)


# ============================================================================================= union_batch_graphs
UNION_SIZES = (2, 3, 4, 5, 3, 2, 4, 3)                   # icosphere frequencies, cycled


@pytest.fixture(scope='module')
def prepared(dev):
    """40 small prepared meshes of differing sizes: in-CSR, reverse-edge index and vertex -> corner lists built per part"""
    from geobi_gnn_amd import meshgen, meshprep
    from geobi_gnn_amd.network import _fv_index
    parts = []
    for i in range(40):
        noisy, clean, faces = meshgen.noisy_icosphere(UNION_SIZES[i % len(UNION_SIZES)], 0.2, seed=100 + i)
        dv, df = meshprep.build_dual_data(noisy, faces, clean, device=dev)
        dv.graph().ensure_in(); df.graph().ensure_in()
        _fv_index(df, dv.x.shape[0])[1].get()
        parts.append((dv, df))
    return parts


def _host_union(graphs):
    """rowptr, col and pos_in of the disjoint union with torch.cat and offsets on the host"""
    rps, cols, poss, noff, eoff = [], [], [], 0, 0
    for g in graphs:
        rps.append(g.rowptr_out[:g.N].cpu() + eoff)
        cols.append(g.col_out.cpu() + noff)
        poss.append(g.pos_in.cpu() + eoff)
        noff += g.N
        eoff += g.E
    rps.append(torch.tensor([eoff], dtype=torch.int32))
    return torch.cat(rps), torch.cat(cols), torch.cat(poss), noff, eoff


@pytest.mark.parametrize('B', [12, 40])
def test_union_of_many_prepared_meshes(dev, prepared, B):
    """B = 12 is more than 96 int32 copy segments (9 per mesh and 3 closing ones: 111, the second launch), B = 40 is 363
    (four launches).  Every array of the union equals the same union built with torch.cat and offsets on the host;
    pos_in equals geobi_csr_reverse_index run on the union itself; Graph.union gives the same rowptr_out and col_out."""
    from geobi_gnn_amd.data import union_batch_graphs
    from geobi_gnn_amd.graph import Graph
    parts = prepared[:B]
    uv, uf = union_batch_graphs(parts)
    torch.cuda.synchronize()
    nv = [dv.x.shape[0] for dv, _ in parts]
    nf = [df.x.shape[0] for _, df in parts]
    off_v, off_f = np.concatenate([[0], np.cumsum(nv)]), np.concatenate([[0], np.cumsum(nf)])
    assert len(set(nv)) >= 4
    for u, side, n in ((uv, 0, nv), (uf, 1, nf)):
        graphs = [p[side].graph() for p in parts]
        g = u.graph()
        rowptr, col, pos, N, E = _host_union(graphs)
        assert (g.N, g.E) == (N, E) and g.symmetric
        assert torch.equal(g.rowptr_out.cpu(), rowptr) and torch.equal(g.col_out.cpu(), col)
        assert g.rowptr_in is g.rowptr_out and g.col_in is g.col_out and torch.equal(g.pos_in.cpu(), pos)
        own = Graph.from_sorted(N, g.rowptr_out, None, g.col_out, symmetric=True).ensure_in()
        assert torch.equal(own.pos_in, g.pos_in)
        cat = Graph.union(graphs)
        assert torch.equal(cat.rowptr_out, g.rowptr_out) and torch.equal(cat.col_out, g.col_out)
        for key in ('x', 'y', 'depth_direction'):
            vals = [getattr(p[side], key, None) for p in parts]
            if any(v is None for v in vals):
                assert getattr(u, key, None) is None, key
                continue
            want = torch.cat([v.cpu() for v in vals])
            assert torch.equal(getattr(u, key).cpu().view(torch.int32), want.view(torch.int32)), key
        w = torch.cat([gr.weights_sorted(p[side].edge_weight).cpu() for gr, p in zip(graphs, parts)])
        assert torch.equal(u.edge_weight.cpu().view(torch.int32), w.view(torch.int32))
        lw = torch.cat([torch.full((k,), 1.0) / (torch.tensor(float(k)) * B) for k in n])
        assert torch.equal(u._loss_weights.cpu(), lw)
        assert u.mesh_ptr.tolist() == (off_v, off_f)[side].tolist()
    fv = torch.cat([df.fv_indices.cpu() + int(o) for (_, df), o in zip(parts, off_v[:-1])])
    assert torch.equal(uf.fv_indices.cpu(), fv)
    fv32, corner, V = uf.fv_indices._geobi_fv
    assert V == off_v[-1] and torch.equal(fv32.cpu().long(), fv) and corner.index is not None
    idx = [df.fv_indices._geobi_fv[1].index for _, df in parts]
    segptr = torch.cat([ix.segptr[:k].cpu() + 3 * int(o) for ix, k, o in zip(idx, nv, off_f[:-1])] +
                       [torch.tensor([3 * int(off_f[-1])], dtype=torch.int32)])
    members = torch.cat([ix.members.cpu() + 3 * int(o) for ix, o in zip(idx, off_f[:-1])])
    assert torch.equal(corner.index.segptr.cpu(), segptr) and torch.equal(corner.index.members.cpu(), members)
    m_segptr, m_members = M.segment_csr(fv.view(-1).numpy(), int(V))                 # and they ARE the union's own lists
    assert np.array_equal(segptr.numpy(), m_segptr) and np.array_equal(members.numpy(), m_members)


# ============================================================================== FeaSt on a symmetric multigraph
@pytest.mark.parametrize('fused', [True, 32, False])
@pytest.mark.parametrize('Cin,Cout', F.RING_SHAPES)
def test_feast_on_a_symmetric_multigraph(dev, Cin, Cout, fused):
    """multi37: 90 pairs on 37 nodes, 30 of them listed twice, both directions.  The layer takes the reverse-index path,
    where pos_in points every entry of a run at the run's FIRST reverse entry; the backward stays right because equal
    entries carry equal dl.  Within the per-row bar of the fp64 oracle, and bit for bit what the transpose path (a true
    permutation) gives.

    Measured on the MI355X over the nine cases, worst kernel distance (worst fp32 oracle distance):
      out per row 1.17e-06 (2.98e-07), dx per row 1.33e-06 (6.44e-07), both 128 -> 128 on 16-row tiles;
      dlin.weight 2.49e-07 (5.95e-07), du.weight 3.00e-07 (5.55e-07), dc 3.64e-07 (2.61e-07), dbias 1.26e-07 (1.34e-07).
    Every case is inside the bar by a factor of seven or more."""
    name = 'multi37'
    got = F.run_gpu(dev, name, Cin, Cout, 0.2, False, fused=fused)
    ref, f32 = F.run_oracle(name, Cin, Cout, 0.2), F.run_oracle_fp32(name, Cin, Cout, 0.2)
    _, _, info = F.graph_of_name(name)
    d, y = F.distances(got, ref), F.distances(f32, ref)
    print('multi37 fused=%s %d -> %d: kernel (fp32 oracle) %s' % (
        fused, Cin, Cout, ' '.join('%s %.2e (%.2e)' % (k, d[k], y[k]) for k in F.KEYS)))
    for k in F.KEYS:
        assert got[k].shape == ref[k].shape and got[k].dtype == torch.float32, k
        assert bool(torch.isfinite(got[k]).all()), k
    for k in F.ROW_KEYS:
        assert not F.floor_engages(ref[k]), k
        assert d[k] < F.BAR, '%s per row %.2e (fp32 oracle %.2e); worst rows: %s' % (
            k, d[k], y[k], F.worst_rows(got[k], ref[k], info))
    for k in F.KEYS:
        assert d[k] < F.BAR, '%s %.2e (fp32 oracle %.2e)' % (k, d[k], y[k])
    other = F.run_gpu(dev, name, Cin, Cout, 0.2, False, fused=fused, transpose=True)
    for k in F.KEYS:
        assert torch.equal(got[k], other[k]), 'reverse-index and transpose path: %s differs' % k
