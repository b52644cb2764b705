"""tests/graph_model.py kept honest on a machine without a GPU: the model against a brute-force dense adjacency count,
the algebra its outputs must obey (transposing twice, inverse permutations, the involution of the reverse index), and
every generated case against the property its name claims -- degrees, number of bad ids, runs of duplicates, which
segments are empty.  The symmetric multigraph of the FeaSt tests is checked for what it is, and the fp64 oracle evaluated
in fp32 stays under a quarter of feast_cases.BAR on it.

Measured on multi37 (slope 0.2, seeds of feast_cases.seed_of), fp32 oracle from fp64, worst over out, dx and the four
parameter gradients: 6 -> 32 6.98e-07 (dx), 64 -> 64 6.14e-07 (dx), 128 -> 128 8.78e-07 (du.weight); the quarter is 2.5e-06."""
import numpy as np
import pytest
import torch

import feast_cases as F
import graph_model as M

COO = M.coo_cases()
TRANSPOSE = M.transpose_cases()
REVERSE = M.reverse_cases()
SEGMENT = M.segment_cases()


def _small(N):
    return N <= 300


# ------------------------------------------------------------------------------------- the model, by brute force
@pytest.mark.parametrize('name', sorted(COO))
@pytest.mark.parametrize('drop_self', [0, 1])
def test_csr_from_coo_model(name, drop_self):
    c = COO[name]
    seg, nbr, N = c['seg'], c['nbr'], c['N']
    E = seg.size
    rowptr, col, eid, n_bad = M.csr_from_coo(seg, nbr, N, drop_self)
    ok = np.asarray([0 <= a < N and 0 <= b < N for a, b in zip(seg.tolist(), nbr.tolist())], dtype=bool)
    keep = ok & ~((seg == nbr) & bool(drop_self))
    assert n_bad == int((~ok).sum()) and rowptr[N] == keep.sum() == col.size == eid.size
    assert rowptr[0] == 0 and np.all(np.diff(rowptr) >= 0)
    row = M.rows_of(rowptr)
    assert np.array_equal(seg[eid], row) and np.array_equal(nbr[eid], col)            # eid maps back
    key = row * N + col
    assert np.all(np.diff(key) >= 0)                                                  # sorted by (seg, nbr)
    assert np.all(np.diff(eid)[np.diff(key) == 0] > 0)                                # stable inside a run
    assert np.array_equal(np.sort(eid), np.nonzero(keep)[0])
    if _small(N):
        assert np.array_equal(M.dense_count(row, col, N), M.dense_count(seg[keep], nbr[keep], N))
    rp2, col_s, eid_s, _ = M.csr_from_coo_slots(seg, nbr, N, drop_self)
    E1 = int(rowptr[N])
    assert np.array_equal(rp2, rowptr) and col_s.size == eid_s.size == E
    assert np.array_equal(col_s[:E1], col) and np.all(col_s[E1:] == -1)
    assert np.array_equal(np.sort(eid_s), np.arange(E)) and np.all(np.diff(eid_s[E1:]) > 0)


@pytest.mark.parametrize('name', sorted(TRANSPOSE))
def test_csr_transpose_model(name):
    c = TRANSPOSE[name]
    rowptr, col, N, E = c['rowptr'], c['col'], c['N'], c['E']
    row = M.rows_of(rowptr)
    for pad in c['pads']:
        rowptr_t, col_t, pos_t, inv = M.csr_transpose(rowptr, col, N, E + pad)
        assert col_t.size == pos_t.size == E + pad and np.all(col_t[E:] == -1) and np.all(pos_t[E:] == -1)
        assert rowptr_t[N] == E and inv.size == E
        row_t = M.rows_of(rowptr_t)
        assert np.array_equal(row_t, col[pos_t[:E]]) and np.array_equal(col_t[:E], row[pos_t[:E]])
        key = row_t * N + col_t[:E]
        assert np.all(np.diff(key) >= 0) and np.all(np.diff(pos_t[:E])[np.diff(key) == 0] > 0)
        assert np.array_equal(pos_t[:E][inv], np.arange(E)) and np.array_equal(inv[pos_t[:E]], np.arange(E))
        if _small(N):
            assert np.array_equal(M.dense_count(row_t, col_t[:E], N), M.dense_count(row, col, N).T)
        back_rp, back_col, back_pos, _ = M.csr_transpose(rowptr_t, col_t, N, E + pad)          # twice: the original
        assert np.array_equal(back_rp, rowptr) and np.array_equal(back_col[:E], col)
        assert np.array_equal(pos_t[:E][back_pos[:E]], np.arange(E))


@pytest.mark.parametrize('name', sorted(REVERSE))
def test_reverse_index_model(name):
    c = REVERSE[name]
    rowptr, col, N = c['rowptr'], c['col'], c['N']
    row = M.rows_of(rowptr)
    pos, flag = M.reverse_index(rowptr, col)
    A = M.dense_count(row, col, N) if N <= 400 else None
    for e in range(col.size):                                                         # brute force, entry by entry
        i, j = row[e], col[e]
        where = np.nonzero((row == j) & (col == i))[0]
        assert pos[e] == (where[0] if where.size else -1)
        if A is not None:
            assert (pos[e] >= 0) == (A[j, i] > 0)
    assert flag == int(np.any(pos < 0))
    if c['missing'] is not None:
        assert int((pos < 0).sum()) == c['missing']


def test_expand_gather_concat_models():
    for N in M.EXPAND_N:
        rowptr = M.expand_case(N)
        row = M.expand_rowptr(rowptr)
        assert np.array_equal(row, M.rows_of(rowptr)) and row.size == rowptr[N]
        assert np.array_equal(np.bincount(row, minlength=N), np.diff(rowptr))
    src = np.asarray([1.5, -0.0, np.nan], dtype=np.float32)
    got = M.gather_f32(src, [2, -1, 1, 0, -5]).view(np.uint32)
    assert got.tolist() == [src.view(np.uint32)[2], 0, 0x80000000, src.view(np.uint32)[0], 0]
    segs = [(np.asarray([1, -2, 2 ** 31 - 1], dtype=np.int32), 3, -5, 0.0), (None, 2, -7, 2.5), (np.zeros(0, np.int32), 0, 1, 0.0)]
    i = M.concat32(segs, 0)
    assert [a.view(np.int32).tolist() for a in i] == [[-4, -7, 2 ** 31 - 6], [-7, -7], []]
    i = M.concat32([(np.asarray([7], dtype=np.int32), 1, 2 ** 31 - 1, 0.0)], 0)
    assert i[0].view(np.int32).tolist() == [-2 ** 31 + 6]                             # wraps as the uint32 add does
    f = M.concat32([(np.asarray([-0.0], dtype=np.float32), 1, 9, 1.0), (None, 2, 9, 2.5)], 1)
    assert f[0].tolist() == [0x80000000] and f[1].view(np.float32).tolist() == [2.5, 2.5]


@pytest.mark.parametrize('name', sorted(SEGMENT))
def test_segment_csr_model(name):
    seg, nseg = SEGMENT[name]
    segptr, members = M.segment_csr(seg, nseg)
    assert segptr.size == nseg + 1 and segptr[nseg] == seg.size == members.size
    assert np.array_equal(np.diff(segptr), np.bincount(seg, minlength=nseg))
    owner = M.rows_of(segptr)
    assert np.array_equal(seg[members], owner)
    assert np.all(np.diff(members)[np.diff(owner) == 0] > 0)                          # ascending inside a segment
    assert np.array_equal(np.sort(members), np.arange(seg.size))


# ------------------------------------------------------------------------------ the cases are what they are called
def test_coo_cases_have_their_properties():
    assert M.COO_N == (1, 2, 3, 4, 255, 256, 257, 65535, 65536, 65537, 2 ** 20 + 1) and M.COO_E == (1, 255, 256, 257, 1000)
    for N in M.COO_N:
        c = COO['n%d' % N]
        assert c['N'] == N and c['seg'].size == (7 if N == 2 ** 20 + 1 else 1000)
        pairs = set(zip(c['seg'].tolist(), c['nbr'].tolist()))
        assert {(0, N - 1), (N - 1, 0), (N - 1, N - 1), (0, 0)} <= pairs               # both ends, and the loop on N - 1
    for E in M.COO_E:
        for N in (257, 65536):
            c = COO['e%d_n%d' % (E, N)]
            assert c['N'] == N and c['seg'].size == E
            assert (c['seg'][0], c['nbr'][0]) == (0, N - 1)
            if E >= 256:                                                              # more than one block, with duplicates
                key = c['seg'] * N + c['nbr']
                assert np.unique(key).size < E
    for N in (255, 65535):                                                            # N = 2^k - 1: the largest key of all
        rowptr, col, _, _ = M.csr_from_coo(COO['n%d' % N]['seg'], COO['n%d' % N]['nbr'], N, 0)
        assert col[-1] == N - 1 and rowptr[N] - rowptr[N - 1] >= 1 and M.rows_of(rowptr)[-1] == N - 1
    c = COO['isolated_ends']
    deg = np.diff(M.csr_from_coo(c['seg'], c['nbr'], c['N'], 0)[0])
    assert c['N'] == 300 and np.all(deg[:100] == 0) and np.all(deg[200:] == 0) and deg[100] > 0 and deg[199] > 0
    c = COO['all_invalid']
    rowptr, col, _, n_bad = M.csr_from_coo(c['seg'], c['nbr'], c['N'], 0)
    assert n_bad == c['seg'].size == 280 and col.size == 0 and not rowptr.any()
    c = COO['all_loops']
    assert np.array_equal(c['seg'], c['nbr']) and M.csr_from_coo(c['seg'], c['nbr'], c['N'], 1)[1].size == 0
    assert M.csr_from_coo(c['seg'], c['nbr'], c['N'], 0)[1].size == 300
    seg, nbr, times = M.runs_case()
    assert sorted(times.values()) == [1, 1, 2, 3, 3, 4, 5] and seg.size == sum(times.values())
    for (a, b), t in times.items():
        assert int(((seg == a) & (nbr == b)).sum()) == t
    assert any(np.any(np.diff(np.nonzero((seg == a) & (nbr == b))[0]) > 1) for (a, b), t in times.items() if t > 1)  # shuffled
    c = COO['bad_ids']
    N = c['N']
    for b in (-1, N, -2 ** 40, 2 ** 40 + 3):
        assert int((c['seg'] == b).sum()) == 2 and int((c['nbr'] == b).sum()) == 2
    assert 0 <= (2 ** 40 + 3) % 2 ** 32 < N and 0 <= (-2 ** 40) % 2 ** 32 < N           # the low words look valid
    assert M.csr_from_coo(c['seg'], c['nbr'], N, 0)[3] == 12 and c['seg'].size == 26
    assert COO['empty']['seg'].size == 0 and COO['empty']['N'] == 5


def test_transpose_cases_have_their_properties():
    c = TRANSPOSE['directed']
    deg, row = np.diff(c['rowptr']), M.rows_of(c['rowptr'])
    assert np.all(deg[:40] == 0) and np.all(deg[260:] == 0) and c['pads'] == (0, 1, 300)
    assert np.unique(row * c['N'] + c['col']).size < c['E']                              # duplicates
    A = M.dense_count(row, c['col'], c['N'])
    assert not np.array_equal(A, A.T)                                                  # directed
    c = TRANSPOSE['no_valid_edge']
    assert c['E'] == 0 and min(c['pads']) > 0
    c = TRANSPOSE['one_node']
    assert c['N'] == 1 and c['E'] == 3
    c = TRANSPOSE['hub_row']
    assert np.diff(c['rowptr']).max() == 5000
    for c in TRANSPOSE.values():
        assert c['rowptr'][c['N']] == c['E'] == c['col'].size                          # never above Ecap = E + pad
        assert c['col'].size == 0 or (0 <= c['col'].min() and c['col'].max() < c['N'])


def test_reverse_cases_have_their_properties():
    for name in ('simple', 'multi', 'row_lengths'):
        c = REVERSE[name]
        row = M.rows_of(c['rowptr'])
        pos, flag = M.reverse_index(c['rowptr'], c['col'])
        assert flag == 0 and np.array_equal(row[pos], c['col']) and np.array_equal(c['col'][pos], row)
        key = row * c['N'] + c['col']
        assert np.all(np.diff(key) >= 0) and not np.any(row == c['col'])
        if name == 'multi':
            assert np.unique(key).size < key.size and np.unique(pos).size < pos.size   # no permutation
            runs = np.bincount(np.unique(key, return_inverse=True)[1].reshape(-1))
            assert set(runs.tolist()) == {1, 2, 3}
            first = np.ones(key.size, dtype=bool)
            first[1:] = key[1:] != key[:-1]
            assert np.all(first[pos])                                                  # the first of the run
        else:
            assert np.unique(key).size == key.size
            assert np.array_equal(pos[pos], np.arange(pos.size))                       # an involution
    assert sorted(set(np.diff(REVERSE['row_lengths']['rowptr']).tolist())) == [0, 1, 2, 5000]
    assert REVERSE['one_missing']['missing'] == 1
    pos, flag = M.reverse_index(REVERSE['many_missing']['rowptr'], REVERSE['many_missing']['col'])
    assert flag == 1 and 100 < int((pos < 0).sum()) < pos.size
    assert REVERSE['empty']['col'].size == 0


def test_small_cases_have_their_properties():
    for N in M.EXPAND_N:
        deg = np.diff(M.expand_case(N))
        assert N == 1 or (deg[0] == 0 and deg[-1] == 0 and deg.max() > 1)
        assert N < 256 or np.all(deg[N // 3:N // 3 + 10] == 0)
    for n in M.GATHER_N:
        src, idx = M.gather_case(n)
        assert idx.size == n and idx.max() < src.size and (n < 4 or int((idx < 0).sum()) == n // 4)
        assert src.view(np.uint32)[:7].tolist() == list(M.SPECIAL_BITS)
        assert np.isnan(src[3]) and np.isnan(src[4]) and np.isinf(src[1]) and src[0] == 0 and np.signbit(src[0])
    sizes = sorted((s.size, n) for s, n in SEGMENT.values())
    for k in (8, 16):
        for d in (-1, 0, 1):
            assert (2 ** k + d, 2 ** k + d) in sizes
    for seg, nseg in SEGMENT.values():
        assert seg.size == 0 or (0 <= seg.min() and seg.max() < nseg)
    seg, nseg = SEGMENT['empty_ends']
    cnt = np.bincount(seg, minlength=nseg)
    assert np.all(cnt[:100] == 0) and np.all(cnt[200:] == 0)
    assert np.unique(SEGMENT['one_segment'][0]).size == 1 and SEGMENT['no_member'][0].size == 0
    assert set(SEGMENT['first_segment'][0]) == {0} and set(SEGMENT['last_segment'][0]) == {SEGMENT['last_segment'][1] - 1}


def test_concat_cases_have_their_properties():
    assert M.CONCAT_COUNTS == (1, 95, 96, 97, 192, 193, 300)
    seen = set()
    for count in M.CONCAT_COUNTS:
        n = M.concat_lengths(count)
        assert n.size == count and set(n.tolist()) <= set(M.CONCAT_LENGTHS)
        seen |= set(n.tolist())
        if count == 1:
            continue
        assert n[0] == 0 and n[-1] == 0 and n.sum() > 0
        edges = list(range(M.CONCAT_CHUNK, count, M.CONCAT_CHUNK))
        for edge in edges:                                        # the first launch edge lies in a row of empty segments,
            want_empty = edge == M.CONCAT_CHUNK and count >= 192  # every other one between segments that hold something
            for i in range(edge - 2, min(edge + 2, count - 1)):
                assert (n[i] == 0) == want_empty, (count, i)
        for is_float in (0, 1):
            segs = M.concat_case(count, is_float)
            assert [s[1] for s in segs] == n.tolist()
            assert all(s[0] is None or s[0].size == s[1] for s in segs)
            assert any(s[0] is None and s[1] > 0 for s in segs) or count < 10            # fills
            assert any(s[2] < 0 for s in segs) and any(s[2] > 0 for s in segs)
            if is_float and count >= 95:
                bits = np.concatenate([s[0].view(np.uint32) for s in segs if s[0] is not None])
                assert 0x80000000 in bits and 0x7fc12345 in bits
    assert seen == set(M.CONCAT_LENGTHS)
    assert sum(M.BIG_LENGTHS) > 4096 * 1024 and 0 in M.BIG_LENGTHS


# --------------------------------------------------------------------------- the multigraph of the FeaSt tests
def test_multi_graph_is_a_symmetric_multigraph():
    ei, n, info = F.graph_of_name('multi37')
    assert n == 37 and ei.dtype == torch.long and ei.shape == (2, 240)
    assert int(ei.min()) >= 0 and int(ei.max()) < n and not bool((ei[0] == ei[1]).any())
    key, cnt = torch.unique(ei[0] * n + ei[1], return_counts=True)
    assert key.numel() == 180 and sorted(cnt.tolist()) == [1] * 120 + [2] * 60           # 30 pairs twice, both directions
    rkey, rcnt = torch.unique(ei[1] * n + ei[0], return_counts=True)
    assert torch.equal(key, rkey) and torch.equal(cnt, rcnt)                           # symmetric, run for run
    assert torch.equal(info.indeg, info.outdeg) and int(info.indeg.min()) >= 1
    rowptr, col, _, _ = M.csr_from_coo(ei[0].numpy(), ei[1].numpy(), n, 1)
    pos, flag = M.reverse_index(rowptr, col)
    assert flag == 0 and np.unique(pos).size == 180                                    # pos_in is no permutation
    ei2, _, _ = F.graph_of_name('multi37')
    assert torch.equal(ei, ei2) and ei.data_ptr() != ei2.data_ptr()


@pytest.mark.parametrize('Cin,Cout', F.RING_SHAPES)
def test_fp32_oracle_distance_on_the_multigraph(Cin, Cout):
    ref, f32 = F.run_oracle('multi37', Cin, Cout, 0.2), F.run_oracle_fp32('multi37', Cin, Cout, 0.2)
    for k in F.ROW_KEYS:
        assert not F.floor_engages(ref[k]), (k, F.row_share(ref[k]))
    d = F.distances(f32, ref)
    print('multi37 %d -> %d: fp32 oracle %s' % (Cin, Cout, ' '.join('%s %.2e' % (k, d[k]) for k in F.KEYS)))
    assert max(d.values()) <= F.BAR / 4, d
