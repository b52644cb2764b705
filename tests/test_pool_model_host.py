"""tests/pool_model.py against the oracle's own statements of the same operations, and each constructed input of the
device tests (tests/test_gpu_pool.py) against the property it is named for.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import pool_model as M
from helpers import load_fixture


def _converge(rowptr, col, w, cap=100000):
    cache = M._row_order(rowptr, col, w)
    st, und = M.match_rounds(rowptr, col, w, 1, _cache=cache)
    rounds = 1
    while und:
        st, und = M.match_rounds(rowptr, col, w, rounds, state=st, _cache=cache)
        rounds = min(rounds * 2, cap)
    return st


MATCH = M.match_cases()


@pytest.mark.parametrize('name', sorted(MATCH))
def test_rounds_converge_to_greedy(name):
    rowptr, col, w = MATCH[name]
    st = _converge(rowptr, col, w)
    assert st.min() >= 0
    assert np.array_equal(M.finish(st), M.greedy_sorted(rowptr, col, w))
    # a valid matching: partners are mutual and joined by an edge
    u = np.arange(st.size)
    assert np.array_equal(st[st], u)
    row = M.rows_of(rowptr)
    edges = set((row * st.size + col).tolist())
    assert all(int(a) * st.size + int(b) in edges for a, b in zip(u[st != u], st[st != u]))


@pytest.mark.parametrize('n', M.FORM_SIZES)
def test_rounds_converge_on_form_inputs(n):
    rowptr, col, w = M.form_case(n)
    assert np.array_equal(M.finish(_converge(rowptr, col, w)), M.greedy_sorted(rowptr, col, w))


@pytest.mark.parametrize('name', ['path600', 'row_lengths', 'negative', 'no_weights', 'n257'])
def test_array_rounds_equal_the_loops(name):
    rowptr, col, w = MATCH[name]
    st_a = st_l = None
    for rounds in (1, 2, 3, 5):
        st_a, und_a = M.match_rounds(rowptr, col, w, rounds, state=st_a)
        st_l, und_l = M.match_rounds_loops(rowptr, col, w, rounds, state=st_l)
        assert np.array_equal(st_a, st_l) and und_a == und_l
    fresh, _ = M.match_rounds(rowptr, col, w, 11)
    assert np.array_equal(fresh, st_a)                       # 1 + 2 + 3 + 5 resumed = 11 at once


def test_greedy_equals_oracle_c():
    from oracle import pyg_ops as P
    lib = P._load_graclus_c()
    if not lib:
        pytest.skip('oracle C helper not built')
    for name in sorted(MATCH):
        rowptr, col, w = MATCH[name]
        n = rowptr.size - 1
        row = M.rows_of(rowptr)
        ww = np.ones(col.size) if w is None else w.astype(np.float64)
        order = np.ascontiguousarray(np.lexsort((np.maximum(row, col), np.minimum(row, col), -ww)).astype(np.int64))
        out = np.empty(n, dtype=np.int64)
        r, c = np.ascontiguousarray(row), np.ascontiguousarray(col)
        lib.oracle_greedy_sorted(ctypes.c_int64(n), ctypes.c_int64(col.size), ctypes.c_void_p(order.ctypes.data),
                                 ctypes.c_void_p(r.ctypes.data), ctypes.c_void_p(c.ctypes.data),
                                 ctypes.c_void_p(out.ctypes.data))
        assert np.array_equal(out, M.greedy_sorted(rowptr, col, w)), name


def test_inputs_have_their_properties():
    rowptr, col, w = MATCH['path600']
    st, und = M.match_rounds(rowptr, col, w, 299)
    assert und == 2                                           # the 300th round takes the last pair
    assert M.match_rounds(rowptr, col, w, 300)[1] == 0
    for k in (1, 7, 150):
        assert M.match_rounds(rowptr, col, w, k)[1] == 600 - 2 * k
    rowptr, col, w, named = M.row_length_graph()
    deg = np.diff(rowptr)
    assert sorted(named) == sorted(M.ROW_LENGTHS)
    for d, node in named.items():
        assert deg[node] == d
    assert float(MATCH['negative'][2].max()) < 0 and MATCH['no_weights'][2] is None
    assert float(MATCH['mixed_sign'][2].min()) < 0 < float(MATCH['mixed_sign'][2].max())
    assert len(set(MATCH['all_equal'][2].tolist())) == 1
    for n in (255, 256, 257):
        assert MATCH['n%d' % n][0].size == n + 1
    for name, (rp, cl, ww) in MATCH.items():                  # symmetric, and so are the weights
        row = M.rows_of(rp)
        n = rp.size - 1
        fwd = dict(zip((row * n + cl).tolist(), (np.ones(cl.size) if ww is None else ww).tolist()))
        assert all(fwd.get(int(c) * n + int(r)) == v for r, c, v in
                   zip(row, cl, (np.ones(cl.size) if ww is None else ww).tolist())), name


def test_relabel_and_lists_equal_pyg():
    from oracle import pyg_ops as P
    rowptr, col, w = MATCH['ties']
    for rounds in (1, 3, 50):
        st, _ = M.match_rounds(rowptr, col, w, rounds)
        cl = M.finish(st)
        cnew, nc = M.relabel(cl)
        ref, _ = P.consecutive_cluster(torch.from_numpy(cl))
        assert np.array_equal(cnew, ref.numpy()) and nc == int(ref.max()) + 1
        c2, segptr, members, nc2 = M.pair_lists(st)
        assert nc2 == nc and np.array_equal(c2, cnew)
        sp, mem = M.segment_csr(cnew, nc)                     # the lists of a matching ascend, as the sorted ones do
        assert np.array_equal(sp, segptr) and np.array_equal(mem, members)
    cluster = np.random.RandomState(0).randint(0, 500, 2000)
    ref, _ = P.consecutive_cluster(torch.from_numpy(cluster))
    assert np.array_equal(M.relabel(cluster)[0], ref.numpy())


@pytest.mark.parametrize('C', [1, 3, 64])
def test_segment_functions_equal_scatter(C):
    from oracle import pyg_ops as P
    case = M.segment_case(C)
    x = torch.from_numpy(case['x_finite']).double()
    covered = case['seg1'] >= 0
    for seg, nseg, lists in ((case['seg1'], case['n_mid'], ('segptr1', 'members1')),
                             (case['seg12'], case['n_coarse'], None)):
        idx = torch.from_numpy(seg[covered])
        xs = x[torch.from_numpy(covered)]
        if lists is None:
            sp, mem = M.compose_lists(case['segptr1'], case['members1'], case['segptr2'], case['members2'])
        else:
            sp, mem = case[lists[0]], case[lists[1]]
        assert sorted(mem.tolist()) == sorted(np.nonzero(covered)[0].tolist())
        assert np.allclose(M.segment_sum(x.numpy(), sp, mem), P.scatter(xs, idx, dim_size=nseg, reduce='sum').numpy(),
                           rtol=1e-12, atol=1e-12)
        assert np.allclose(M.segment_mean(x.numpy(), sp, mem), P.scatter(xs, idx, dim_size=nseg, reduce='mean').numpy(),
                           rtol=1e-12, atol=1e-12)
        out, arg = M.segment_max(x.numpy(), sp, mem)
        assert np.array_equal(out, P.scatter(xs, idx, dim_size=nseg, reduce='max').numpy())     # values (args: list order)
        assert np.all((arg >= 0) == (np.diff(sp) > 0)[:, None])
        cols = np.broadcast_to(np.arange(C), arg.shape)
        assert np.array_equal(np.where(arg >= 0, x.numpy()[np.maximum(arg, 0), cols], 0.0), out)
    # max2 = max over the composed lists, value and routed row
    xf = case['x']
    o2, a12 = M.segment_max2(xf, case['segptr1'], case['members1'], case['segptr2'], case['members2'])
    sp, mem = M.compose_lists(case['segptr1'], case['members1'], case['segptr2'], case['members2'])
    o12, a = M.segment_max(xf, sp, mem)
    assert np.array_equal(o2.view(np.uint32), o12.view(np.uint32)) and np.array_equal(a12, a)
    assert np.array_equal(M.segment_sum2(x.numpy(), case['segptr1'], case['members1'], case['segptr2'], case['members2']),
                          M.segment_sum(x.numpy(), sp, mem))
    # backwards: the routed gradient sums to gout where a segment is not empty; the mean's spreads it evenly
    gout = np.random.RandomState(C).randn(case['n_coarse'], C).astype(np.float32)
    gx = M.segment_max_bwd(gout, a12, case['seg12'], case['n_fine'])
    assert np.array_equal(M.segment_sum(gx, sp, mem), np.where(a12 >= 0, gout, 0).astype(np.float64))
    seg = np.where(case['seg12'] >= 0, case['seg12'], 0)
    gm = M.segment_mean_bwd(gout, seg, sp)[case['seg12'] >= 0]
    back = np.zeros((case['n_coarse'], C))
    np.add.at(back, case['seg12'][case['seg12'] >= 0], gm)
    assert np.allclose(back, np.where((np.diff(sp) > 0)[:, None], gout, 0.0), rtol=1e-12, atol=1e-12)


def test_segment_case_has_its_properties():
    case = M.segment_case(4)
    x = case['x']
    sizes1, sizes2 = np.diff(case['segptr1']), np.diff(case['segptr2'])
    assert sizes1.min() >= 1 and sizes1.max() == 1000
    empty = np.nonzero(sizes2 == 0)[0]
    assert any(0 < e < sizes2.size - 1 and sizes2[e - 1] > 0 and sizes2[e + 1] > 0 for e in empty)
    assert sizes2[-1] == 0
    assert np.any(np.diff(case['members2']) < 0)              # step-two members do not ascend
    o1, a1 = M.segment_max(x, case['segptr1'], case['members1'])
    o2, a12 = M.segment_max2(x, case['segptr1'], case['members1'], case['segptr2'], case['members2'])
    assert np.any(np.all(o2 < 0, axis=1) & np.all(np.isfinite(o2), axis=1))          # all negative: 0 must not win
    assert np.any(np.isposinf(o2)) and np.any(np.isneginf(o2))
    zero = (o2 == 0) & (sizes2 > 0)[:, None]
    assert np.any(np.signbit(o2[zero])) and np.any(~np.signbit(o2[zero]))            # -0.0 first and +0.0 first
    # a tie across two step-one segments: the winner's value also tops another mid segment of the same coarse one
    sp, mem = M.compose_lists(case['segptr1'], case['members1'], case['segptr2'], case['members2'])
    straddle = 0
    for c in range(sizes2.size):
        mids = case['members2'][case['segptr2'][c]:case['segptr2'][c + 1]]
        straddle += int(np.sum(o1[mids, 0] == o2[c, 0]) >= 2)
    assert straddle >= 2
    assert np.sum(x[case['members1'][:1000], 0] == o1[0, 0]) == 2                     # and one inside the long segment
    assert np.sum(case['seg1'] < 0) == 2 and np.all(np.isfinite(case['x_finite']))


def test_pool_edge_equals_reference():
    from oracle import ref_model as R
    fx = load_fixture('pure_functions.npz')
    rowptr_c, row_c, col_c, w_c = M.pool_edge(fx['cluster'], fx['edge_index'][0], fx['edge_index'][1], fx['calc_weight'])
    assert np.array_equal(np.stack([row_c, col_c]), fx['pool_edge_index'])
    assert np.allclose(w_c, fx['pool_edge_weight'], rtol=1e-6, atol=0)
    rng = np.random.RandomState(4)
    rowptr, col, w = M.random_graph(2000, 8000, 4)
    row = M.rows_of(rowptr)
    cluster = np.unique(rng.randint(0, 700, 2000), return_inverse=True)[1].reshape(-1)
    ei, ew = R.pool_edge(torch.from_numpy(cluster), torch.from_numpy(np.stack([row, col])), torch.from_numpy(w).double())
    rowptr_c, row_c, col_c, w_c = M.pool_edge(cluster, row, col, w)
    assert np.array_equal(np.stack([row_c, col_c]), ei.numpy())
    assert np.array_equal(w_c, ew.numpy().astype(np.float32))
    assert np.array_equal(np.diff(rowptr_c), np.bincount(row_c, minlength=rowptr_c.size - 1))
    assert M.pool_edge(cluster, row, col, None)[3] is None


@pytest.mark.parametrize('with65', [False, True])
def test_coarsen_case_gathers_what_it_names(with65):
    case = M.coarsen_case(with65)
    assert case['N'] % 4 in (1, 3)
    st, und = M.match_rounds(case['rowptr'], case['col'], case['w'], M.COARSEN_ROUNDS)
    assert und == 0
    assert np.array_equal(M.finish(st), M.greedy_sorted(case['rowptr'], case['col'], case['w']))
    cnew, segptr, members, nc = M.pair_lists(st)
    counts = M.row_gather_counts(case['rowptr'], segptr, members)
    named = {k: int(cnew[v]) for k, v in case['named'].items()}
    want = {'pair%d' % T: T for T in M.COARSEN_PAIRS if T != 65 or with65}
    want.update(hub64=64, single1=1, single0=0)
    assert {k: int(counts[c]) for k, c in named.items()} == want
    assert int(counts.max()) == (65 if with65 else 64)
    sizes = np.diff(segptr)
    assert all(sizes[named[k]] == 2 for k in want if k.startswith('pair'))
    assert all(sizes[named[k]] == 1 for k in ('hub64', 'single1', 'single0'))
    rowptr_c, row_c, col_c, w_c = M.pool_edge(cnew, M.rows_of(case['rowptr']), case['col'], case['w'], nc)
    out_deg = np.diff(rowptr_c)
    assert out_deg[named['pair2']] == 0 and out_deg[named['single0']] == 0 and out_deg[named['hub64']] == 64
    for T in (31, 32, 33, 63, 64):
        assert 0 < out_deg[named['pair%d' % T]] < T - 2           # duplicates were merged
    wq = case['w'].astype(np.float64) * 4096
    assert np.all(wq == np.round(wq)) and wq.min() > 0 and wq.max() <= 4 * 4096


def test_run64_case():
    case = M.run64_case()
    cnew, segptr, members, nc = M.pair_lists(case['state'])
    assert nc == 4 and list(M.row_gather_counts(case['rowptr'], segptr, members)) == [64, 64, 33, 31]
    rowptr_c, row_c, col_c, w_c = M.pool_edge(cnew, M.rows_of(case['rowptr']), case['col'], case['w'], nc)
    assert list(zip(row_c, col_c)) == [(0, 1), (1, 0), (2, 3), (3, 2)]
    row = M.rows_of(case['rowptr'])
    assert np.float32(case['w'][row == 0].astype(np.float64).sum() / 64) == w_c[0]


@pytest.mark.parametrize('C', M.EW_CHANNELS)
def test_edge_weight_case(C):
    case = M.edge_weight_case(C)
    d = M.sq_dist(case['x'], case['row'], case['col'])
    assert d.max() < 160.0 and np.sum(np.abs(d - 80.0) < 0.01) >= 40 and np.sum(case['row'] == case['col']) >= case['n']
    assert np.all(M.edge_weight_t10(case['x'], case['row'], case['col'])[case['row'] == case['col']] == 1.0)
    x64 = case['x_att'].astype(np.float64)
    al, ar = x64 @ case['att_l'].astype(np.float64), x64 @ case['att_r'].astype(np.float64)
    alpha = (al[case['row']] + ar[case['col']]) + (al[case['col']] + ar[case['row']])
    assert alpha.max() > 100.0 and alpha.min() < -100.0
    for w_in in (None, case['w_in']):
        ref = M.edge_weight_att(case['x_att'], case['att_l'], case['att_r'], case['row'], case['col'], w_in)
        f32 = M.edge_weight_att(case['x_att'], case['att_l'], case['att_r'], case['row'], case['col'], w_in, dtype=np.float32)
        assert np.all(np.isfinite(f32)) and ref.min() >= 0.0 and ref.max() <= 1.0
        # what single precision delivers on these inputs: the device test's bar of 1e-6 must be reachable
        print('C = %d: fp32 formula against fp64, max abs %.3e' % (C, np.abs(f32 - ref).max()))


def test_scan_model():
    for n in (1, 16, 1000):
        v = M.scan_case(n)
        assert v.min() >= 0 and v.max() <= 64
        assert np.array_equal(M.exclusive_scan(v), np.concatenate([[0], np.cumsum(v.astype(np.int64))[:-1]]))
