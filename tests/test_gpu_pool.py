"""The pooling front end (csrc/match.hip, csrc/segment.hip, csrc/pool.hip) through the C ABI against the plain model of
tests/pool_model.py, at the edges of its paths: every form of the matching tail and of the scans (forced through
geobi_set_match_scanfree / geobi_set_scan_lookback), the state of the matching after every call, the bitonic row merge
at gathered counts of 0 / 1 / 31 / 32 / 33 / 63 / 64 / 65, the segment reductions on negative, signed-zero, infinite,
tied and empty segments, and the edge weights element by element.

Bars: every integer output and every selection (max, arg, routed gradient, merged weight) is compared EXACTLY; sums,
means and the edge weights have the bounds stated at their tests, each derived from fp32 arithmetic."""
import ctypes
import time

import numpy as np
import pytest
import torch

import pool_model as M

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


def _L():
    from geobi_gnn_amd import _lib
    return _lib


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def _f32(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want):
    return np.array_equal(_bits(got), _bits(want))


class _Graph(object):
    def __init__(self, dev, rowptr, col, w):
        self.N, self.E = len(rowptr) - 1, len(col)
        self.rowptr, self.col, self.w = _i32(rowptr, dev), _i32(col, dev), _f32(w, dev)
        self.dev = dev


# ======================================================================================================= matching
def _match(g, rounds, state=None):
    """geobi_match_heavy_edge -> (state, cluster_final, undecided)"""
    L = _L()
    init = state is None
    state = torch.empty(g.N, dtype=torch.int32, device=g.dev) if init else state.clone()
    final = torch.empty(g.N, dtype=torch.int32, device=g.dev)
    status = torch.full((1,), -7, dtype=torch.int32, device=g.dev)
    ws = L.workspace(L.size_query('geobi_match_ws_bytes', g.N), g.dev)
    L.call('geobi_match_heavy_edge', L.ptr(g.rowptr), L.ptr(g.col), L.ptr(g.w), g.N, rounds, 1 if init else 0,
           L.ptr(state), L.ptr(final), L.ptr(status), L.ptr(ws), ws.numel(), L.stream())
    return state, final, int(status.item())


class _Coarse(object):
    pass


def _match_coarsen(g, rounds, state=None, rowinfo=False):
    """geobi_match_coarsen (or its rowinfo twin) -> object with state, final, cnew, segptr, members, und, nc[, rowinfo]"""
    L = _L()
    init = state is None
    o = _Coarse()
    o.state = torch.empty(g.N, dtype=torch.int32, device=g.dev) if init else state.clone()
    o.final = torch.empty(g.N, dtype=torch.int32, device=g.dev)
    o.cnew = torch.empty(g.N, dtype=torch.int32, device=g.dev)
    o.segptr = torch.full((g.N + 1,), -9, dtype=torch.int32, device=g.dev)
    o.members = torch.full((g.N,), -9, dtype=torch.int32, device=g.dev)
    o.counters = torch.full((8,), -7, dtype=torch.int32, device=g.dev)
    ws = L.workspace(L.size_query('geobi_match_coarsen_ws_bytes', g.N), g.dev)
    head = (L.ptr(g.rowptr), L.ptr(g.col), L.ptr(g.w), g.N, rounds, 1 if init else 0, L.ptr(o.state), L.ptr(o.final),
            L.ptr(o.cnew), L.ptr(o.segptr), L.ptr(o.members), L.ptr(o.counters))
    if rowinfo:
        o.rowinfo = torch.full((g.N, 4), -9, dtype=torch.int32, device=g.dev)
        made = ctypes.c_int32(-1)
        L.call('geobi_debug_match_coarsen_rowinfo', *head, L.ptr(o.rowinfo), ctypes.byref(made), L.ptr(ws), ws.numel(),
               L.stream())
        o.made = made.value
    else:
        L.call('geobi_match_coarsen', *head, L.ptr(ws), ws.numel(), L.stream())
    o.und, o.nc = (int(v) for v in _np(o.counters[:2]))
    return o


def _check_coarse(o, st, und, tag):
    """every output of a match_coarsen call against the model's lists of the model's state"""
    cnew, segptr, members, nc = M.pair_lists(st)
    assert (o.und, o.nc) == (und, nc), tag
    assert np.array_equal(_np(o.state), st), tag
    assert np.array_equal(_np(o.final), M.finish(st)), tag
    assert np.array_equal(_np(o.cnew), cnew), tag
    assert np.array_equal(_np(o.segptr)[:nc + 1], segptr), tag
    assert np.array_equal(_np(o.members), members), tag


def _first_difference(got, want):
    bad = np.nonzero(got != want)[0]
    return 'node %d: device %d, model %d (%d nodes differ)' % (bad[0], got[bad[0]], want[bad[0]], bad.size) if bad.size else ''


MATCH = M.match_cases()
_GREEDY = {}


def _greedy(name):
    if name not in _GREEDY:
        _GREEDY[name] = M.greedy_sorted(*MATCH[name])
    return _GREEDY[name]


@pytest.mark.parametrize('name', sorted(MATCH))
def test_matching_state_after_every_call(dev, name):
    """state and status after fresh calls of 1, 2 and 3 rounds, then after every resume (3, 6, 12, ... rounds) of the
    3-round state until nothing is undecided: each equals the model's synchronous rounds, so the state between calls is a
    function of the input alone; at convergence cluster_final is the sorted greedy matching.  The same through
    geobi_match_coarsen, with its lists."""
    rowptr, col, w = MATCH[name]
    g = _Graph(dev, rowptr, col, w)
    for coarsen in (False, True):
        run = (lambda r, s=None: _match_coarsen(g, r, s)) if coarsen else (lambda r, s=None: _match(g, r, s))
        st_m = st_d = None
        for rounds in (1, 2, 3):
            st_m, und_m = M.match_rounds(rowptr, col, w, rounds)
            out = run(rounds)
            st_d = out.state if coarsen else out[0]
            und_d = out.und if coarsen else out[2]
            assert np.array_equal(_np(st_d), st_m), '%s fresh %d rounds: %s' % (name, rounds, _first_difference(_np(st_d), st_m))
            assert und_d == und_m
            if coarsen:
                _check_coarse(out, st_m, und_m, '%s fresh %d' % (name, rounds))
            else:
                assert np.array_equal(_np(out[1]), M.finish(st_m))
        rounds, calls = 3, 0
        while und_m:
            st_m, und_m = M.match_rounds(rowptr, col, w, rounds, state=st_m)
            out = run(rounds, st_d)
            st_d = out.state if coarsen else out[0]
            und_d = out.und if coarsen else out[2]
            assert np.array_equal(_np(st_d), st_m), '%s resume of %d rounds: %s' % (name, rounds,
                                                                                    _first_difference(_np(st_d), st_m))
            assert und_d == und_m
            if coarsen:
                _check_coarse(out, st_m, und_m, '%s resume %d' % (name, rounds))
            rounds *= 2
            calls += 1
            assert calls < 20
        final = out.final if coarsen else out[1]
        assert np.array_equal(_np(final), _greedy(name)), name
    if name == 'path600':
        assert calls == 7                                    # 3 fresh + 3 + 6 + ... + 192 = 384 >= 300 rounds


# =========================================================================================== forms of match_coarsen
_FORM_MODEL = {}


def _form_model(n, rowptr, col, w):
    if n not in _FORM_MODEL:
        cache = M._row_order(rowptr, col, w)
        _FORM_MODEL[n] = {r: M.match_rounds(rowptr, col, w, r, _cache=cache) for r in (2, 8)}
    return _FORM_MODEL[n]


@pytest.mark.parametrize('n', M.FORM_SIZES)
def test_match_coarsen_forms(dev, n):
    """The scan-free kernel pair and commit + scans + lists (forced through geobi_set_match_scanfree) both equal the
    model, hence each other bit for bit, at 2 rounds (undecided nodes left) and 8.  n + 1 = 262 144 / 262 145 is the
    boundary between the one-block dual scan and two rocPRIM scans inside the two-pass form."""
    L = _L()
    rowptr, col, w = M.form_case(n)
    g = _Graph(dev, rowptr, col, w)
    model = _form_model(n, rowptr, col, w)
    try:
        for rounds in (2, 8):
            st, und = model[rounds]
            if rounds == 2:
                assert und > 0
            outs = []
            for form in (1, 0):
                L.call('geobi_set_match_scanfree', form)
                o = _match_coarsen(g, rounds, rowinfo=True)
                assert o.made == form                            # only the scan-free pair writes the row info
                _check_coarse(o, st, und, 'n %d, %d rounds, scanfree %d' % (n, rounds, form))
                outs.append(o)
            a, b = outs
            for f in ('state', 'final', 'cnew', 'members'):
                assert torch.equal(getattr(a, f), getattr(b, f)), f
            assert torch.equal(a.segptr[:a.nc + 1], b.segptr[:b.nc + 1]) and torch.equal(a.counters[:2], b.counters[:2])
    finally:
        L.call('geobi_set_match_scanfree', -1)


def _separate_calls(g, rounds):
    """geobi_match_heavy_edge + geobi_relabel_compact + geobi_segment_csr_pairs"""
    L = _L()
    state, final, und = _match(g, rounds)
    cnew = torch.empty(g.N, dtype=torch.int32, device=g.dev)
    count = torch.zeros(1, dtype=torch.int32, device=g.dev)
    ws = L.workspace(L.size_query('geobi_relabel_ws_bytes', g.N), g.dev)
    L.call('geobi_relabel_compact', L.ptr(final), g.N, 1, L.ptr(cnew), L.ptr(count), L.ptr(ws), ws.numel(), L.stream())
    nc = int(count.item())
    segptr = torch.empty(g.N + 1, dtype=torch.int32, device=g.dev)
    members = torch.empty(g.N, dtype=torch.int32, device=g.dev)
    ws = L.workspace(L.size_query('geobi_segment_pairs_ws_bytes', nc), g.dev)
    L.call('geobi_segment_csr_pairs', L.ptr(cnew), L.ptr(final), g.N, nc, L.ptr(segptr), L.ptr(members), L.ptr(ws),
           ws.numel(), L.stream())
    return state, final, und, cnew, nc, segptr, members


@pytest.mark.parametrize('n', [1048576, 1048577])
def test_match_coarsen_million_nodes(dev, n):
    """256 * 4096 nodes is the last size of the scan-free pair; one node more takes commit + two rocPRIM scans + lists with
    no hook.  Both against the separate calls (model-independent) and against the model (about 5 s on the host)."""
    rowptr, col, w = M.random_graph(n, 1500000, n + 1, ties=True)
    g = _Graph(dev, rowptr, col, w)
    cache = M._row_order(rowptr, col, w)
    for rounds in (2, 8):
        t0 = time.time()
        o = _match_coarsen(g, rounds, rowinfo=True)
        assert o.made == (1 if n <= 1048576 else 0)
        state, final, und, cnew, nc, segptr, members = _separate_calls(g, rounds)
        assert (o.und, o.nc) == (und, nc)
        assert torch.equal(o.state, state) and torch.equal(o.final, final) and torch.equal(o.cnew, cnew)
        assert torch.equal(o.segptr[:nc + 1], segptr[:nc + 1]) and torch.equal(o.members, members)
        t1 = time.time()
        st, und_m = M.match_rounds(rowptr, col, w, rounds, _cache=cache)
        _check_coarse(o, st, und_m, 'n %d, %d rounds' % (n, rounds))
        print('n = %d, %d rounds: device calls %.2f s, model and comparison %.2f s' % (n, rounds, t1 - t0, time.time() - t1))


# ========================================================================================================== scans
@pytest.mark.parametrize('lookback', [0, 1])
@pytest.mark.parametrize('n', M.SCAN_SIZES)
def test_exclusive_scan_forms(dev, n, lookback):
    """the library's int scan with the look-back form forced off (the one-block walk: 1 .. 17 steps of 16 384) and on,
    across 16 384 (one step / look-back) and 262 144 (look-back or one block / rocPRIM); values 0 .. 64 as row counts"""
    L = _L()
    v = M.scan_case(n)
    src = _i32(v, dev)
    out = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ws = L.workspace(L.lib().geobi_debug_scan_ws_bytes(n), dev)
    try:
        L.call('geobi_set_scan_lookback', lookback)
        L.call('geobi_debug_scan_exclusive_i32', L.ptr(src), L.ptr(out), n, L.ptr(ws), ws.numel(), L.stream())
    finally:
        L.call('geobi_set_scan_lookback', -1)
    want = np.cumsum(v.astype(np.int64)) - v
    assert np.array_equal(_np(out), want)


def _scan_buffers(dev, v, in_off, out_off):
    """v in a buffer `in_off` ints behind a 16-byte boundary, an output range of -1 sentinels `out_off` ints behind one
    with a guard element on either side -> (in view, out view, whole output buffer, index of out[0] in it)"""
    n = len(v)
    src = torch.zeros(n + 4, dtype=torch.int32, device=dev)
    buf = torch.full((n + 8,), -1, dtype=torch.int32, device=dev)
    assert src.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
    o0 = 4 + out_off                                     # one whole int4 of guards in front of an aligned range
    a, o = src[in_off:in_off + n], buf[o0:o0 + n]
    a.copy_(torch.from_numpy(v))
    assert a.data_ptr() % 16 == 4 * in_off and o.data_ptr() % 16 == 4 * out_off
    return a, o, buf, o0


def _check_scan(buf, o0, v, what):
    got = _np(buf)
    n = len(v)
    assert np.array_equal(got[o0:o0 + n], np.cumsum(v.astype(np.int64)) - v), what
    assert (got[:o0] == -1).all() and (got[o0 + n:] == -1).all(), what + ': wrote outside out[0 .. n)'


def test_exclusive_scan_unaligned(dev):
    """Pointers 4 bytes behind a 16-byte boundary take the scalar loads and stores of load_chunk / store_chunk, which no
    torch allocation reaches: the single scan in both look-back settings with in and out = buf[1:1 + n] (and once with
    only out so) at one int, either side of a thread's 16, a full step plus one (4097 look-back / 16 385 walk) and
    20 000 (five look-back blocks with a tail); the pair scan (one kernel, vec = all four pointers aligned) aligned and
    with only out_b off.  List b has other values than list a (seed n + 1): a carry or wave sum taken from the wrong
    list shows.  The elements around every output range keep their -1."""
    L = _L()
    try:
        for lookback in (0, 1):
            L.call('geobi_set_scan_lookback', lookback)
            for n, in_off in [(m, 1) for m in (1, 15, 17, 4097, 16385, 20000)] + [(20000, 0)]:
                v = M.scan_case(n)
                a, o, buf, o0 = _scan_buffers(dev, v, in_off, 1)
                ws = L.workspace(L.lib().geobi_debug_scan_ws_bytes(n), dev)
                L.call('geobi_debug_scan_exclusive_i32', L.ptr(a), L.ptr(o), n, L.ptr(ws), ws.numel(), L.stream())
                _check_scan(buf, o0, v, 'n %d, look-back %d, in +%d ints, out +1' % (n, lookback, in_off))
    finally:
        L.call('geobi_set_scan_lookback', -1)
    for n in (1, 16, 16385, 20000):
        va, vb = M.scan_case(n), M.scan_case(n + 1)[:n]
        for off_b in (0, 1):
            a, oa, buf_a, a0 = _scan_buffers(dev, va, 0, 0)
            b, ob, buf_b, b0 = _scan_buffers(dev, vb, 0, off_b)
            L.call('geobi_debug_scan_exclusive_i32_pair', L.ptr(a), L.ptr(b), L.ptr(oa), L.ptr(ob), n, L.stream())
            _check_scan(buf_a, a0, va, 'pair, n %d, list a, out_b +%d ints' % (n, off_b))
            _check_scan(buf_b, b0, vb, 'pair, n %d, list b, out_b +%d ints' % (n, off_b))


# ================================================================================================ edge coarsening
def _rows_form(g, cnew, segptr, members, nc, w, onepass, rowinfo_in=None):
    """geobi_pool_edge_rows (two passes) or geobi_debug_pool_edge_rows_onepass -> (rowptr_c, row_c, col_c, w_c, count, overflow)"""
    L = _L()
    dev = g.dev
    rowptr_c = torch.full((g.N + 1,), -9, dtype=torch.int32, device=dev)
    row_c = torch.full((max(g.E, 1),), -9, dtype=torch.int32, device=dev)
    col_c = torch.full((max(g.E, 1),), -9, dtype=torch.int32, device=dev)
    w_c = torch.full((max(g.E, 1),), float('nan'), device=dev) if w is not None else None
    ctr = torch.zeros(4, dtype=torch.int32, device=dev)
    ctr[0] = nc
    if onepass:
        ws = L.workspace(L.lib().geobi_debug_pool_edge_rows_onepass_ws_bytes(g.N, g.E), dev)
        L.call('geobi_debug_pool_edge_rows_onepass', L.ptr(cnew), L.ptr(segptr), L.ptr(members), L.ptr(g.rowptr),
               L.ptr(g.col), L.ptr(w), L.ptr(ctr[0:1]), g.N, g.E, L.ptr(rowinfo_in), L.ptr(rowptr_c), L.ptr(row_c),
               L.ptr(col_c), L.ptr(w_c), L.ptr(ctr[1:2]), L.ptr(ctr[2:3]), L.ptr(ws), ws.numel(), L.stream())
    else:
        ws = L.workspace(L.size_query('geobi_pool_edge_rows_ws_bytes', g.N), dev)
        L.call('geobi_pool_edge_rows', L.ptr(cnew), L.ptr(segptr), L.ptr(members), L.ptr(g.rowptr), L.ptr(g.col),
               L.ptr(w), L.ptr(ctr[0:1]), g.N, L.ptr(rowptr_c), L.ptr(row_c), L.ptr(col_c), L.ptr(w_c), L.ptr(ctr[1:2]),
               L.ptr(ctr[2:3]), L.ptr(ws), ws.numel(), L.stream())
    count, overflow = (int(x) for x in _np(ctr[1:3]))
    return _np(rowptr_c), _np(row_c), _np(col_c), None if w_c is None else _np(w_c), count, overflow


def _radix_form(g, cnew, w):
    L = _L()
    dev = g.dev
    row = _i32(M.rows_of(_np(g.rowptr)), dev)
    rowptr_c = torch.full((g.N + 1,), -9, dtype=torch.int32, device=dev)
    row_c = torch.full((g.E,), -9, dtype=torch.int32, device=dev)
    col_c = torch.full((g.E,), -9, dtype=torch.int32, device=dev)
    w_c = torch.full((g.E,), float('nan'), device=dev) if w is not None else None
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = L.workspace(L.lib().geobi_pool_edge_ws_bytes(g.E), dev)
    L.call('geobi_pool_edge', L.ptr(cnew), L.ptr(row), L.ptr(g.col), L.ptr(w), g.E, g.N, L.ptr(rowptr_c), L.ptr(row_c),
           L.ptr(col_c), L.ptr(w_c), L.ptr(count), L.ptr(ws), ws.numel(), L.stream())
    return _np(rowptr_c), _np(row_c), _np(col_c), None if w_c is None else _np(w_c), int(count.item()), 0


def _check_edges(got, want, nc, N, weighted, tag):
    rowptr_c, row_c, col_c, w_c, count, overflow = got
    m_rowptr, m_row, m_col, m_w = want
    assert overflow == 0 and count == m_row.size, tag
    assert np.array_equal(rowptr_c[:nc + 1], m_rowptr), tag
    assert np.all(rowptr_c[nc:N + 1] == count), tag              # the row pointers past the coarse count close the list
    assert np.array_equal(row_c[:count], m_row) and np.array_equal(col_c[:count], m_col), tag
    if weighted:
        assert _same_bits(w_c[:count], m_w), tag                  # weights are multiples of 2^-12: the fp64 sums are exact


def _coarsen_forms(g, cnew, segptr, members, nc, rowinfo_sources, case, overflow_expected, tag):
    rows = M.rows_of(case['rowptr'])
    for weighted in (True, False):
        w = g.w if weighted else None
        want = M.pool_edge(_np(cnew), rows, case['col'], case['w'] if weighted else None, nc)
        forms = [('two-pass', _rows_form(g, cnew, segptr, members, nc, w, False))]
        for src_name, ri in rowinfo_sources:
            forms.append(('one-pass, rowinfo %s' % src_name, _rows_form(g, cnew, segptr, members, nc, w, True, ri)))
        for name, got in forms:
            if overflow_expected:
                assert got[5] == 1, '%s %s' % (tag, name)
            else:
                _check_edges(got, want, nc, g.N, weighted, '%s %s' % (tag, name))
        _check_edges(_radix_form(g, cnew, w), want, nc, g.N, weighted, tag + ' radix')


@pytest.mark.parametrize('with65', [False, True])
def test_edge_coarsening_at_the_merge_boundaries(dev, with65):
    """Coarse nodes that gather exactly 0, 1, 2 (an empty row), 31, 32, 33, 63, 64 and -- with65 -- 65 entries
    (tests/test_pool_model_host.py checks that they do), 64 distinct keys in one wave, a node count that leaves the last
    block ragged.  The matching comes from geobi_match_coarsen, whose rowinfo must equal the model's (r0, d0, r1, d1)."""
    case = M.coarsen_case(with65)
    g = _Graph(dev, case['rowptr'], case['col'], case['w'])
    st, und = M.match_rounds(case['rowptr'], case['col'], case['w'], M.COARSEN_ROUNDS)
    o = _match_coarsen(g, M.COARSEN_ROUNDS, rowinfo=True)
    assert o.made == 1
    _check_coarse(o, st, und, 'coarsen_case')
    cnew, segptr, members, nc = M.pair_lists(st)
    assert np.array_equal(_np(o.rowinfo)[:nc], M.row_info(case['rowptr'], segptr, members))
    _coarsen_forms(g, o.cnew, o.segptr, o.members, nc, (('from match_coarsen', o.rowinfo), ('NULL', None)), case, with65,
                   'with65 %d' % with65)


def test_edge_coarsening_one_run_fills_the_wave(dev):
    """64 gathered entries that all relabel to ONE neighbour, and a run of 31 behind two dropped self entries in a
    33-entry gather (a multigraph with a hand-made matching state; lists and row info from the model)."""
    case = M.run64_case()
    g = _Graph(dev, case['rowptr'], case['col'], case['w'])
    cnew, segptr, members, nc = M.pair_lists(case['state'])
    sp = np.full(g.N + 1, -9, dtype=np.int64)
    sp[:nc + 1] = segptr
    ri = np.full((g.N, 4), -9, dtype=np.int64)
    ri[:nc] = M.row_info(case['rowptr'], segptr, members)
    _coarsen_forms(g, _i32(cnew, dev), _i32(sp, dev), _i32(members, dev), nc, (('from the model', _i32(ri, dev)), ('NULL', None)),
                   case, False, 'run64')


# ============================================================================================= segment reductions
def _lists(case, dev):
    comp = M.compose_lists(case['segptr1'], case['members1'], case['segptr2'], case['members2'])
    return dict(sp1=_i32(case['segptr1'], dev), m1=_i32(case['members1'], dev), sp2=_i32(case['segptr2'], dev),
                m2=_i32(case['members2'], dev), comp=comp)


def _seg_max(dev, x, C, segptr, members, nseg):
    L = _L()
    out = torch.full((nseg, C), float('nan'), device=dev)
    arg = torch.full((nseg, C), -9, dtype=torch.int32, device=dev)
    L.call('geobi_segment_max_fwd', L.ptr(x), C, L.ptr(segptr), L.ptr(members), nseg, L.ptr(out), L.ptr(arg), L.stream())
    return out, arg


def _seg_sum(dev, x, C, segptr, members, nseg, mean):
    L = _L()
    out = torch.full((nseg, C), float('nan'), device=dev)
    L.call('geobi_segment_sum', L.ptr(x), C, L.ptr(segptr), L.ptr(members), nseg, mean, L.ptr(out), L.stream())
    return out


@pytest.mark.parametrize('C', M.SEG_CHANNELS)
def test_segment_reductions_on_edge_values(dev, C):
    """geobi_segment_* and the max2 / sum2 forms on segments that are all negative, hold -0.0 / +0.0 in either order,
    +-inf, exact ties inside and across step-one segments, nothing at all, or 1000 members.
    Max, arg and routed gradients: exact.  Sums and means: |error| <= n_members * 2^-24 * sum|x| per element (n - 1
    roundings of at most 2^-24 of the running sum each, one more for the mean's division)."""
    L = _L()
    case = M.segment_case(C)
    d = _lists(case, dev)
    n_fine, n_mid, n_coarse = case['n_fine'], case['n_mid'], case['n_coarse']
    x = _f32(case['x'], dev)
    # ---- the composed lists
    sp12_m, m12_m = d['comp']
    n_cov = int(sp12_m[-1])
    sp12 = torch.full((n_coarse + 1,), -9, dtype=torch.int32, device=dev)
    m12 = torch.full((n_fine,), -9, dtype=torch.int32, device=dev)
    ws = L.workspace(L.size_query('geobi_segment_pairs_ws_bytes', n_coarse), dev)
    L.call('geobi_segment_csr_compose', L.ptr(d['sp1']), L.ptr(d['m1']), L.ptr(d['sp2']), L.ptr(d['m2']), n_coarse, n_cov,
           L.ptr(sp12), L.ptr(m12), L.ptr(ws), ws.numel(), L.stream())
    assert np.array_equal(_np(sp12), sp12_m) and np.array_equal(_np(m12)[:n_cov], m12_m)
    # ---- max: one step, the composed list, and the one-pass form of both steps
    o1_m, a1_m = M.segment_max(case['x'], case['segptr1'], case['members1'])
    o1, a1 = _seg_max(dev, x, C, d['sp1'], d['m1'], n_mid)
    assert _same_bits(_np(o1), o1_m) and np.array_equal(_np(a1), a1_m)
    o2_m, a12_m = M.segment_max2(case['x'], case['segptr1'], case['members1'], case['segptr2'], case['members2'])
    o12, a12 = _seg_max(dev, x, C, sp12, m12, n_coarse)
    assert _same_bits(_np(o12), o2_m) and np.array_equal(_np(a12), a12_m)
    o2 = torch.full((n_coarse, C), float('nan'), device=dev)
    a2 = torch.full((n_coarse, C), -9, dtype=torch.int32, device=dev)
    L.call('geobi_debug_segment_max2_fwd', L.ptr(x), C, L.ptr(d['sp1']), L.ptr(d['m1']), L.ptr(d['sp2']), L.ptr(d['m2']),
           n_coarse, L.ptr(o2), L.ptr(a2), L.stream())
    assert _same_bits(_np(o2), o2_m) and np.array_equal(_np(a2), a12_m)
    # two composed passes on the device itself: max of the step-one maxima, routed through both args
    o_two, a_two = _seg_max(dev, o1, C, d['sp2'], d['m2'], n_coarse)
    cols = torch.arange(C, device=dev).expand(n_coarse, C)
    routed = torch.where(a_two >= 0, a1[a_two.clamp(min=0).long(), cols], torch.full_like(a_two, -1))
    assert torch.equal(o_two.view(torch.int32), o2.view(torch.int32)) and torch.equal(routed, a2)
    # ---- routed gradients
    rng = np.random.RandomState(C)
    gout = rng.randn(n_coarse, C).astype(np.float32)
    gx0 = (rng.randn(n_fine, C).astype(np.float32) + np.float32(3.0))
    seg12 = _i32(case['seg12'], dev)
    gd = _f32(gout, dev)
    gx = torch.full((n_fine, C), float('nan'), device=dev)
    L.call('geobi_segment_max_bwd', L.ptr(gd), L.ptr(a12), L.ptr(seg12), C, n_coarse, n_fine, L.ptr(gx), L.stream())
    want = M.segment_max_bwd(gout, a12_m, case['seg12'], n_fine)
    assert _same_bits(_np(gx), want)
    gx = torch.full((n_fine, C), float('nan'), device=dev)
    L.call('geobi_debug_segment_max2_bwd', L.ptr(gd), L.ptr(a2), L.ptr(seg12), C, n_coarse, n_fine, L.ptr(gx), 0, L.stream())
    assert _same_bits(_np(gx), want)
    gx = _f32(gx0, dev)
    L.call('geobi_debug_segment_max2_bwd', L.ptr(gd), L.ptr(a2), L.ptr(seg12), C, n_coarse, n_fine, L.ptr(gx), 1, L.stream())
    assert _same_bits(_np(gx), M.segment_max_bwd(gout, a12_m, case['seg12'], n_fine, gx=gx0))
    # ---- sums and means (finite values)
    xf = _f32(case['x_finite'], dev)
    for sp_t, m_t, sp_m, m_m, nseg in ((d['sp1'], d['m1'], case['segptr1'], case['members1'], n_mid),
                                       (sp12, m12, sp12_m, m12_m, n_coarse)):
        bound = np.diff(sp_m)[:, None] * U24 * M.segment_abs_sum(case['x_finite'], sp_m, m_m)
        for mean, ref in ((0, M.segment_sum(case['x_finite'], sp_m, m_m)), (1, M.segment_mean(case['x_finite'], sp_m, m_m))):
            got = _np(_seg_sum(dev, xf, C, sp_t, m_t, nseg, mean)).astype(np.float64)
            err = np.abs(got - ref)
            print('C = %d, %d segments, mean %d: max error / bound = %.3f' %
                  (C, nseg, mean, float(np.max(err / np.maximum(bound, 1e-300)))))
            assert np.all(err <= bound)
            assert np.all(got[np.diff(sp_m) == 0] == 0.0)
    s12 = _seg_sum(dev, xf, C, sp12, m12, n_coarse, 0)
    s2 = torch.full((n_coarse, C), float('nan'), device=dev)
    args = (L.ptr(xf), C, L.ptr(d['sp1']), L.ptr(d['m1']), L.ptr(d['sp2']), L.ptr(d['m2']), n_coarse, L.ptr(s2), L.stream())
    if C % 4 == 0:
        L.call('geobi_debug_segment_sum2', *args)
        assert torch.equal(s2.view(torch.int32), s12.view(torch.int32))       # same order of additions: same bits
    else:
        with pytest.raises(L.GeobiError, match='multiple of 4'):
            L.call('geobi_debug_segment_sum2', *args)
    # ---- the other backwards: mean (one correctly rounded division: <= 2^-24 relative) and sum (a gather: exact)
    seg12c = np.where(case['seg12'] >= 0, case['seg12'], 0)
    gm = torch.full((n_fine, C), float('nan'), device=dev)
    L.call('geobi_segment_mean_bwd', L.ptr(gd), L.ptr(_i32(seg12c, dev)), L.ptr(sp12), C, n_fine, L.ptr(gm), L.stream())
    ref = M.segment_mean_bwd(gout, seg12c, sp12_m)
    assert np.all(np.abs(_np(gm).astype(np.float64) - ref) <= U24 * np.abs(ref))
    gr = torch.full((n_fine, C), float('nan'), device=dev)
    L.call('geobi_gather_rows', L.ptr(gd), L.ptr(_i32(seg12c, dev)), C, n_fine, L.ptr(gr), L.stream())
    assert _same_bits(_np(gr), M.segment_sum_bwd(gout, seg12c))


def test_segment_sum2_rejects_six_channels(dev):
    L = _L()
    z = torch.zeros(64, dtype=torch.int32, device=dev)
    x = torch.zeros(64, 6, device=dev)
    with pytest.raises(L.GeobiError, match='multiple of 4'):
        L.call('geobi_debug_segment_sum2', L.ptr(x), 6, L.ptr(z), L.ptr(z), L.ptr(z), L.ptr(z), 4, L.ptr(x), L.stream())


# =================================================================================================== edge weights
# |sigmoid - fp64| of geobi_edge_weight_att.  The values lie in [0, 1]; 1e-6 is the module-level bar tightened to the
# kernel's own arithmetic.
ATT_TOL = 1e-6


@pytest.mark.parametrize('C', M.EW_CHANNELS)
def test_edge_weights_per_element(dev, C):
    """t10 with w_in: 1e-5 of the maximum.  Without: relative error per element <= ((C + 3) d / 2 + 4) 2^-23 with the
    squared distance d from fp64: the fp32 sum of C squares carries about (C + 3) 2^-24 relative into d, the exponent
    -d / 2 turns that into (C + 3) d / 2 * 2^-24 relative in the result (twice that is allowed for), and expf and the
    final rounding take the 4 * 2^-23.  row == col gives exactly w_in + 1; pairs at d ~ 80 sit at e^-40.
    att: within ATT_TOL of fp64, alpha beyond +-100 without a NaN."""
    L = _L()
    case = M.edge_weight_case(C)
    E, n = case['E'], case['n']
    row, col = _i32(case['row'], dev), _i32(case['col'], dev)
    x, w_in = _f32(case['x'], dev), _f32(case['w_in'], dev)
    d = M.sq_dist(case['x'], case['row'], case['col'])
    loops = case['row'] == case['col']
    for wi in (w_in, None):
        out = torch.full((E,), float('nan'), device=dev)
        L.call('geobi_edge_weight_t10', L.ptr(x), C, L.ptr(row), L.ptr(col), L.ptr(wi), E, L.ptr(out), L.stream())
        got = _np(out).astype(np.float64)
        ref = M.edge_weight_t10(case['x'], case['row'], case['col'], None if wi is None else case['w_in'])
        if wi is not None:
            assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()
            assert _same_bits(got[loops], case['w_in'][loops] + np.float32(1.0))
        else:
            rel = np.abs(got - ref) / ref
            bound = ((C + 3) * d / 2 + 4) * 2.0 ** -23
            print('C = %d: t10 max relative error / bound = %.3f; at d ~ 80: %.3e' %
                  (C, float(np.max(rel / bound)), float(rel[np.abs(d - 80) < 0.01].max())))
            assert np.all(rel <= bound)
            assert np.all(got[loops] == 1.0)
    xa, al, ar = _f32(case['x_att'], dev), _f32(case['att_l'], dev), _f32(case['att_r'], dev)
    for wi in (w_in, None):
        out = torch.full((E,), float('nan'), device=dev)
        node_ws = torch.empty(2 * n, device=dev)
        L.call('geobi_edge_weight_att', L.ptr(xa), C, L.ptr(al), L.ptr(ar), L.ptr(row), L.ptr(col), L.ptr(wi), n, E,
               L.ptr(node_ws), L.ptr(out), L.stream())
        got = _np(out).astype(np.float64)
        ref = M.edge_weight_att(case['x_att'], case['att_l'], case['att_r'], case['row'], case['col'],
                                None if wi is None else case['w_in'])
        f32 = M.edge_weight_att(case['x_att'], case['att_l'], case['att_r'], case['row'], case['col'],
                                None if wi is None else case['w_in'], dtype=np.float32)
        assert np.all(np.isfinite(got))
        print('C = %d: att max abs error %.3e (the same formula in numpy fp32: %.3e)' %
              (C, float(np.abs(got - ref).max()), float(np.abs(f32 - ref).max())))
        assert np.abs(got - ref).max() <= ATT_TOL
        if wi is None:
            assert got.min() == 0.0 or got.min() < 1e-30           # saturated at both ends
            assert got.max() == 1.0
