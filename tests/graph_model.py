"""The index builders under every kernel (csrc/graph.hip, with their entry points) stated in plain numpy:
int64, loops and np.lexsort.  One function per entry point, its contract written out from include/geobi_hip.h and the
kernels; the device tests (tests/test_gpu_graph.py) compare with it exactly, tests/test_graph_model_host.py pins the
model itself to a dense adjacency count on a CPU-only machine.  The inputs of the device tests live here too, so that
both files see the same ones.

    csr_from_coo     stable sort of the kept (seg, nbr) pairs by (seg, nbr): eid ascends within a run of equal pairs.  A
                     pair with an id outside [0, N) is counted in bad and dropped, a self loop is dropped when drop_self.
                     Device arrays have E slots: col = -1 beyond rowptr[N], and eid as a whole is a permutation of
                     range(E) whose tail lists the dropped pairs in input order (the sort is stable and they share a key).
    csr_transpose    the kept entries sorted by (col, row), stable; col_t = the row, pos_t = the entry's position in the
                     input; both -1 in [E, Ecap).  inv_pos[pos_t[k]] = k for k < E, nothing else of inv_pos is written.
    reverse_index    pos_rev[e] of entry (i, j) = FIRST position of i in row j, or -1 and the flag set
    expand_rowptr    row[e] = the row that holds e
    gather_f32       dst[i] = src[idx[i]], 0.0 where idx[i] < 0; a copy, bit for bit
    segment_csr      inverse lists of an index, members ascending (pool_model.segment_csr)
    concat32         dst = src + add (int32, wrapping) / src (float, a copy of the bits); src None: add / value
"""
import bisect

import numpy as np

from pool_model import segment_csr, rows_of      # noqa: F401  (segment_csr is part of this model's surface)

I64 = np.int64
POISON = -0x5a5a5a5b            # fills every output before a call
GUARD = 8                       # words past the end of every output that must keep the poison


# ---------------------------------------------------------------------------------------------------------- model
def _rowptr_of(rows, N):
    rowptr = np.zeros(N + 1, dtype=I64)
    for r in np.asarray(rows, dtype=I64).tolist():
        rowptr[r + 1] += 1
    return np.cumsum(rowptr)


def csr_from_coo(seg, nbr, N, drop_self):
    """-> (rowptr [N + 1], col_valid, eid_valid, n_bad)"""
    seg, nbr = np.asarray(seg, dtype=I64), np.asarray(nbr, dtype=I64)
    ok = (seg >= 0) & (seg < N) & (nbr >= 0) & (nbr < N)
    keep = ok & ~((seg == nbr) & bool(drop_self))
    idx = np.nonzero(keep)[0]
    eid = idx[np.lexsort((idx, nbr[idx], seg[idx]))]
    return _rowptr_of(seg[eid], N), nbr[eid], eid, int((~ok).sum())


def csr_from_coo_slots(seg, nbr, N, drop_self):
    """The device arrays with their E slots -> (rowptr, col [E], eid [E], n_bad)"""
    rowptr, col, eid, n_bad = csr_from_coo(seg, nbr, N, drop_self)
    E = len(np.asarray(seg))
    dropped = np.setdiff1d(np.arange(E, dtype=I64), eid)                    # ascending
    return rowptr, np.concatenate([col, -np.ones(dropped.size, dtype=I64)]), np.concatenate([eid, dropped]), n_bad


def csr_transpose(rowptr, col, N, Ecap):
    """-> (rowptr_t [N + 1], col_t [Ecap], pos_t [Ecap], inv_pos [rowptr[N]])"""
    rowptr = np.asarray(rowptr, dtype=I64)
    E = int(rowptr[N])
    assert E <= Ecap, 'rowptr[N] above Ecap is outside the contract'
    col = np.asarray(col, dtype=I64)[:E]
    row = rows_of(rowptr)
    pos = np.lexsort((np.arange(E), row, col))
    pad = -np.ones(Ecap - E, dtype=I64)
    inv = np.empty(E, dtype=I64)
    inv[pos] = np.arange(E)
    return _rowptr_of(col, N), np.concatenate([row[pos], pad]), np.concatenate([pos, pad]), inv


def reverse_index(rowptr, col):
    """-> (pos_rev [E], flag): the lower-bound position of the reverse entry, -1 where there is none"""
    rowptr, col = np.asarray(rowptr, dtype=I64).tolist(), np.asarray(col, dtype=I64).tolist()
    out, flag = [], 0
    for i in range(len(rowptr) - 1):
        for e in range(rowptr[i], rowptr[i + 1]):
            j = col[e]
            p = bisect.bisect_left(col, i, rowptr[j], rowptr[j + 1])
            if p < rowptr[j + 1] and col[p] == i:
                out.append(p)
            else:
                out.append(-1)
                flag = 1
    return np.asarray(out, dtype=I64), flag


def expand_rowptr(rowptr):
    rowptr = np.asarray(rowptr, dtype=I64).tolist()
    row = []
    for n in range(len(rowptr) - 1):
        row += [n] * (rowptr[n + 1] - rowptr[n])
    return np.asarray(row, dtype=I64)


def gather_f32(src, idx):
    """on the bits, so that a NaN keeps its payload and -0.0 its sign"""
    bits = np.ascontiguousarray(src, dtype=np.float32).view(np.uint32)
    idx = np.asarray(idx, dtype=I64)
    return np.where(idx >= 0, bits[np.maximum(idx, 0)], np.uint32(0)).astype(np.uint32).view(np.float32)


def concat32(segments, is_float):
    """segments: (src or None, n, add, value) -> the list of destination arrays (uint32 bit patterns)"""
    out = []
    for src, n, add, value in segments:
        if src is None:
            word = np.asarray([value], dtype=np.float32).view(np.uint32)[0] if is_float else np.uint32(add & 0xffffffff)
            out.append(np.full(n, word, dtype=np.uint32))
        else:
            bits = np.ascontiguousarray(src).view(np.uint32)[:n].astype(I64)
            out.append((bits if is_float else (bits + add) & 0xffffffff).astype(np.uint32))
    return out


def dense_count(rows, cols, N):
    """A[i, j] = number of entries (i, j): the brute-force statement the model is checked against"""
    A = np.zeros((N, N), dtype=I64)
    for r, c in zip(np.asarray(rows, dtype=I64).tolist(), np.asarray(cols, dtype=I64).tolist()):
        A[r, c] += 1
    return A


# ========================================================================================================= inputs
# ---- geobi_csr_from_coo
COO_N = (1, 2, 3, 4, 255, 256, 257, 65535, 65536, 65537, 2 ** 20 + 1)
COO_E = (1, 255, 256, 257, 1000)
BAD_IDS = (-1, None, -2 ** 40, 2 ** 40 + 3)             # None stands for N; the low 32 bits of the last two look valid


def coo_random(N, E, seed):
    """E random pairs; the first four touch node 0 and node N - 1 -- (0, N-1), (N-1, 0), the loops (N-1, N-1) and (0, 0) --
    and the last E / 8 repeat the first ones."""
    rng = np.random.RandomState(seed)
    seg, nbr = rng.randint(0, N, E).astype(I64), rng.randint(0, N, E).astype(I64)
    for k, (a, b) in enumerate(((0, N - 1), (N - 1, 0), (N - 1, N - 1), (0, 0))[:E]):
        seg[k], nbr[k] = a, b
    d = E // 8
    if d:
        seg[E - d:], nbr[E - d:] = seg[:d], nbr[:d]
    return seg, nbr


def runs_case():
    """runs of 2, 3, 4 and 5 equal pairs, a loop listed three times and two single pairs, shuffled
    -> (seg, nbr, {pair: times listed})"""
    rng = np.random.RandomState(21)
    pairs = [(7, 3), (7, 4), (0, 49), (49, 0), (12, 12), (30, 31), (31, 30)]
    times = [2, 3, 4, 5, 3, 1, 1]
    seg = np.repeat([p[0] for p in pairs], times)
    nbr = np.repeat([p[1] for p in pairs], times)
    order = rng.permutation(seg.size)
    return seg[order].astype(I64), nbr[order].astype(I64), dict(zip(pairs, times))


def bad_case(N=100):
    """every bad id once as a segment, once as a neighbour and once as both, between valid pairs"""
    rng = np.random.RandomState(22)
    seg, nbr = [], []
    for b in BAD_IDS:
        b = N if b is None else b
        for a, c in ((b, 5), (6, b), (b, b)):
            seg += [a, int(rng.randint(0, N))]
            nbr += [c, int(rng.randint(0, N))]
    seg += [N - 1, 0]
    nbr += [0, N - 1]
    return np.asarray(seg, dtype=I64), np.asarray(nbr, dtype=I64)


def coo_cases():
    """name -> dict(seg, nbr, N): every case runs with drop_self 0 and 1, with and without the bad counter"""
    cases = {}
    for N in COO_N:
        cases['n%d' % N] = coo_random(N, 7 if N > 2 ** 20 else 1000, N % 1000) + (N,)
    for E in COO_E:
        for N in (257, 65536):
            cases['e%d_n%d' % (E, N)] = coo_random(N, E, E + N % 1000) + (N,)
    seg, nbr = coo_random(100, 400, 23)
    cases['isolated_ends'] = (seg + 100, nbr + 100, 300)               # nodes 0..99 and 200..299 have no entry
    cases['all_invalid'] = (np.asarray([-1, 300, 5, 2 ** 40 + 3] * 70, dtype=I64), np.asarray([4, 2, -7, 1] * 70, dtype=I64), 300)
    cases['all_loops'] = (np.arange(300, dtype=I64) % 37, np.arange(300, dtype=I64) % 37, 37)
    cases['runs'] = runs_case()[:2] + (50,)
    cases['bad_ids'] = bad_case(100) + (100,)
    cases['empty'] = (np.zeros(0, dtype=I64), np.zeros(0, dtype=I64), 5)
    return {k: dict(seg=seg, nbr=nbr, N=N) for k, (seg, nbr, N) in cases.items()}


# ---- geobi_csr_transpose
def _csr(seg, nbr, N, drop_self=1):
    rowptr, col, _, _ = csr_from_coo(seg, nbr, N, drop_self)
    return rowptr, col


def hub_pairs(leaves=5000):
    """node 0 with `leaves` neighbours 1 .. leaves, a path of three behind them, one isolated node at the end:
    -> (u, v, N) undirected pairs; rows of 5000, 1, 2 and 0 entries once symmetrised"""
    u = [0] * leaves + [leaves + 1, leaves + 2]
    v = list(range(1, leaves + 1)) + [leaves + 2, leaves + 3]
    return np.asarray(u, dtype=I64), np.asarray(v, dtype=I64), leaves + 5


def transpose_cases():
    """name -> dict(rowptr, col, N, E, pads): the call runs with Ecap = E + pad for every pad"""
    cases = {}
    rng = np.random.RandomState(31)
    seg, nbr = rng.randint(40, 260, 900).astype(I64), rng.randint(0, 300, 900).astype(I64)
    seg[700:], nbr[700:] = seg[:200], nbr[:200]                          # duplicates; rows 0..39 and 260..299 are empty
    cases['directed'] = _csr(seg, nbr, 300) + (300, (0, 1, 300))
    cases['no_valid_edge'] = (np.zeros(5, dtype=I64), np.zeros(0, dtype=I64), 4, (3,))
    cases['one_node'] = _csr(np.zeros(3, dtype=I64), np.zeros(3, dtype=I64), 1, drop_self=0) + (1, (0, 1))
    u, v, N = hub_pairs()
    cases['hub_row'] = _csr(u, v, N) + (N, (0, 1))                       # directed: one row of 5000 entries
    for N in (255, 256, 257):
        seg, nbr = coo_random(N, 1000, 32 + N)
        cases['n%d' % N] = _csr(seg, nbr, N, drop_self=0) + (N, (0, 300))
    return {k: dict(rowptr=rp, col=cl, N=N, E=int(rp[N]), pads=pads) for k, (rp, cl, N, pads) in cases.items()}


# ---- geobi_csr_reverse_index
def sym_csr(u, v, N):
    """the CSR of the entries (u, v) and (v, u), pair by pair as listed (a pair listed twice gives a run of two)"""
    u, v = np.asarray(u, dtype=I64), np.asarray(v, dtype=I64)
    return _csr(np.concatenate([u, v]), np.concatenate([v, u]), N)


def random_pairs(N, m, seed):
    """m distinct undirected pairs u < v"""
    rng = np.random.RandomState(seed)
    a, b = rng.randint(0, N, 4 * m), rng.randint(0, N, 4 * m)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = lo[lo != hi].astype(I64) * N + hi[lo != hi]
    _, first = np.unique(key, return_index=True)
    key = key[np.sort(first)][:m]
    assert key.size == m
    return key // N, key % N


def _without(rowptr, col, drop):
    """the CSR with the entries at the positions `drop` removed"""
    row = rows_of(rowptr)
    keep = np.ones(col.size, dtype=bool)
    keep[drop] = False
    return _rowptr_of(row[keep], rowptr.size - 1), col[keep]


def reverse_cases():
    """name -> dict(rowptr, col, N, missing = number of entries without a reverse)"""
    cases = {}
    u, v = random_pairs(400, 1500, 41)
    rp, cl = sym_csr(u, v, 400)
    cases['simple'] = (rp, cl, 0)
    cases['multi'] = sym_csr(np.concatenate([u, u[:300], u[:40]]), np.concatenate([v, v[:300], v[:40]]), 400) + (0,)
    cases['one_missing'] = _without(rp, cl, [1234]) + (1,)
    rng = np.random.RandomState(42)
    cases['many_missing'] = _without(rp, cl, rng.permutation(cl.size)[:700]) + (None,)
    hu, hv, hn = hub_pairs()
    cases['row_lengths'] = sym_csr(hu, hv, hn) + (0,)
    cases['empty'] = (np.zeros(4, dtype=I64), np.zeros(0, dtype=I64), 0)
    return {k: dict(rowptr=rp, col=cl, N=rp.size - 1, missing=miss) for k, (rp, cl, miss) in cases.items()}


# ---- geobi_expand_rowptr / geobi_gather_f32 / geobi_segment_csr
EXPAND_N = (1, 255, 256, 257, 600)


def expand_case(N):
    """row lengths 0 .. 4 with a stretch of empty rows in the middle and an empty first and last row"""
    rng = np.random.RandomState(50 + N)
    deg = rng.randint(0, 5, N)
    deg[[0, N - 1]] = 0
    deg[N // 3:N // 3 + 10] = 0
    if N == 1:
        deg[0] = 3
    rowptr = np.zeros(N + 1, dtype=I64)
    rowptr[1:] = np.cumsum(deg)
    return rowptr


GATHER_N = (1, 255, 256, 257, 1000)
SPECIAL_BITS = (0x80000000, 0x7f800000, 0xff800000, 0x7fc12345, 0xffc00001, 0x7f800001, 0x00000001)
# -0.0, +inf, -inf, a quiet NaN with a payload, a negative one, a signalling NaN, the smallest subnormal


def gather_case(n):
    """-> (src fp32 [m], idx [n]): the special values at known places, every fourth index negative"""
    rng = np.random.RandomState(60 + n)
    m = 301
    src = rng.randn(m).astype(np.float32)
    src.view(np.uint32)[:len(SPECIAL_BITS)] = SPECIAL_BITS
    idx = rng.randint(0, m, n).astype(I64)
    idx[:min(n, len(SPECIAL_BITS))] = np.arange(len(SPECIAL_BITS))[:n]
    idx[3::4] = -1 - rng.randint(0, 5, idx[3::4].size)
    return src, idx


def segment_cases():
    """name -> (seg [n], nseg), every id within [0, nseg)"""
    cases = {}
    for k in (8, 16):
        for d in (-1, 0, 1):
            s = 2 ** k + d
            rng = np.random.RandomState(70 + s % 1000)
            seg = rng.randint(0, s, s)
            seg[[0, -1]] = s - 1, 0
            cases['n%d_nseg%d' % (s, s)] = (seg, s)
    rng = np.random.RandomState(71)
    cases['n255_nseg65537'] = (np.concatenate([[65536, 0], rng.randint(0, 65537, 253)]), 65537)
    cases['n65537_nseg255'] = (rng.randint(0, 255, 65537), 255)
    cases['empty_ends'] = (rng.randint(100, 200, 1000), 300)
    cases['one_segment'] = (np.full(1000, 128), 257)
    cases['first_segment'] = (np.zeros(257, dtype=I64), 256)
    cases['last_segment'] = (np.full(257, 255), 256)
    cases['no_member'] = (np.zeros(0, dtype=I64), 5)
    return {k: (np.asarray(s, dtype=I64), n) for k, (s, n) in cases.items()}


# ---- geobi_concat32
CONCAT_COUNTS = (1, 95, 96, 97, 192, 193, 300)
CONCAT_LENGTHS = (0, 1, 3, 4, 5, 1023, 1024, 1025)
CONCAT_CHUNK = 96                                     # kMaxSegs of csrc/graph.hip: segments per launch
BIG_LENGTHS = (2000003, 0, 2200001, 5)                # 4 200 009 > 4096 x 1024 elements in one launch


def concat_lengths(count):
    """segment lengths: the first and the last are empty; from 192 segments on the four around the first launch edge
    (indices 94 .. 97) are empty as well, while the later edges (192, 288) fall between segments that hold something;
    with 97 segments so does the first."""
    rng = np.random.RandomState(80 + count)
    n = np.asarray(CONCAT_LENGTHS)[rng.randint(0, len(CONCAT_LENGTHS), count)]
    if count == 1:
        return np.asarray([5])
    for edge in range(CONCAT_CHUNK, count, CONCAT_CHUNK):
        lo, hi = edge - 2, min(edge + 2, count - 1)
        n[lo:hi] = np.where(n[lo:hi] == 0, 3, n[lo:hi])
    if count >= 2 * CONCAT_CHUNK:
        n[CONCAT_CHUNK - 2:CONCAT_CHUNK + 2] = 0
    n[[0, -1]] = 0
    return n


def concat_case(count, is_float, lengths=None):
    """-> list of (src or None, n, add, value).  Every seventh segment is a fill (src None); adds alternate in sign and
    reach +-2^31; float sources carry the special bit patterns of SPECIAL_BITS."""
    lengths = concat_lengths(count) if lengths is None else np.asarray(lengths)
    rng = np.random.RandomState(90 + len(lengths) + is_float)
    segs = []
    for k, n in enumerate(lengths.tolist()):
        add = int((-1) ** k * (k * 1000003 + 17)) if k % 5 else (-2 ** 31 if k % 2 else 2 ** 31 - 1)
        value = float(np.float32(k * 0.37 - 11.0))
        if k % 7 == 3:
            segs.append((None, n, add, value))
        elif is_float:
            src = rng.randn(n).astype(np.float32)
            m = min(n, len(SPECIAL_BITS))
            src.view(np.uint32)[:m] = SPECIAL_BITS[:m]
            segs.append((src, n, add, value))
        else:
            segs.append((rng.randint(-2 ** 31, 2 ** 31, n).astype(np.int32), n, add, value))
    return segs
