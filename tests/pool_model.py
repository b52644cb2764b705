"""The pooling front end (csrc/match.hip, csrc/segment.hip, csrc/pool.hip) stated in plain numpy: int64 / fp64, loops where
a loop is the clearest statement.  Written from the semantics in the files' headers and in include/geobi_hip.h, not from the kernels; the device
tests (tests/test_gpu_pool.py) compare with it exactly wherever the result is an integer or a selection, and
tests/test_pool_model_host.py pins the model itself to the oracle's sequential rules on a CPU-only machine.  The inputs
of the device tests live here too, so that both files see the same ones.

    matching     node state: -1 undecided, u closed as a singleton, v != u matched with partner v.  One ROUND: every
                 undecided node proposes to its best undecided neighbour -- edge (u, v) beats (u, v') under (weight desc,
                 min(u, v) asc, max(u, v) asc); self entries are no neighbours -- or to nobody; then the round is committed:
                 mutual proposals match, a node that proposed to nobody (no free neighbour left) closes as a singleton.
                 The state after k rounds is a function of the input alone.  Converged, it is the greedy matching in
                 globally descending edge order (greedy_sorted).  graclus ids = min(u, state), undecided nodes as singletons.
    lists        dense ids by rank of the representative (smaller member); segment c = [representative, partner]
    pool_edge    relabel both endpoints, drop loops, sort by (row, col), merge duplicates by their mean (fp64 sum, fp64
                 division, one rounding to fp32)
    segment_max  first maximum in list order by strict '>', empty segment -> 0 and arg -1
"""
import numpy as np

I64 = np.int64


# ------------------------------------------------------------------------------------------------------- matching
def rows_of(rowptr):
    rowptr = np.asarray(rowptr, dtype=I64)
    return np.repeat(np.arange(rowptr.size - 1, dtype=I64), np.diff(rowptr))


def _weights(col, w):
    return np.ones(len(col), dtype=np.float64) if w is None else np.asarray(w, dtype=np.float64)


def match_rounds_loops(rowptr, col, w, rounds, state=None):
    """The rounds, node by node (the clearest statement; match_rounds is the same thing in array form)."""
    rowptr, col = np.asarray(rowptr, dtype=I64).tolist(), np.asarray(col, dtype=I64).tolist()
    n = len(rowptr) - 1
    ww = _weights(col, w).tolist()
    st = [-1] * n if state is None else np.asarray(state, dtype=I64).tolist()
    for _ in range(rounds):
        prop = [-2] * n
        for u in range(n):
            if st[u] >= 0:
                continue
            best, key = -1, None
            for e in range(rowptr[u], rowptr[u + 1]):
                v = col[e]
                if v == u or st[v] >= 0:
                    continue
                k = (-ww[e], min(u, v), max(u, v))
                if key is None or k < key:
                    best, key = v, k
            prop[u] = best
        new = list(st)
        for u in range(n):
            if st[u] >= 0:
                continue
            if prop[u] == -1:
                new[u] = u
            elif prop[prop[u]] == u:
                new[u] = prop[u]
        st = new
    return np.asarray(st, dtype=I64), sum(1 for s in st if s < 0)


def _row_order(rowptr, col, w):
    """edge ids sorted by (row asc, weight desc, min asc, max asc): inside a row, best edge first"""
    row = rows_of(rowptr)
    col = np.asarray(col, dtype=I64)
    return np.lexsort((np.maximum(row, col), np.minimum(row, col), -_weights(col, w), row)), row


def match_rounds(rowptr, col, w, rounds, state=None, _cache=None):
    """-> (state [N] int64, number of undecided nodes) after `rounds` synchronous rounds from `state` (None: scratch).
    w = None: every weight is 1."""
    rowptr = np.asarray(rowptr, dtype=I64)
    col = np.asarray(col, dtype=I64)
    n = rowptr.size - 1
    order, row = _cache if _cache is not None else _row_order(rowptr, col, w)
    srow, scol = row[order], col[order]
    st = -np.ones(n, dtype=I64) if state is None else np.asarray(state, dtype=I64).copy()
    big = I64(len(col))
    pos = np.arange(len(col), dtype=I64)
    has = rowptr[1:] > rowptr[:-1]
    for _ in range(rounds):
        und = st < 0
        if not und.any():
            break
        ok = und[srow] & und[scol] & (srow != scol)
        first = np.full(n, big, dtype=I64)
        if len(col):
            # first eligible edge of each row in best-first order (reduceat over the non-empty rows only)
            red = np.minimum.reduceat(np.where(ok, pos, big), rowptr[:-1][has])
            first[has] = red
        prop = np.where(first < big, scol[np.minimum(first, len(col) - 1)], -1) if len(col) else np.full(n, -1, dtype=I64)
        prop = np.where(und, prop, -2)
        mutual = und & (prop >= 0)
        mutual[mutual] = prop[prop[mutual]] == np.nonzero(mutual)[0]
        st = np.where(und & (prop == -1), np.arange(n, dtype=I64), st)
        st = np.where(mutual, prop, st)
    return st, int((st < 0).sum())


def greedy_sorted(rowptr, col, w):
    """The sequential rule: walk the edges in globally descending order (weight desc, min asc, max asc), take an edge iff
    both ends are free.  -> graclus ids (min member, unmatched nodes their own id)."""
    rowptr = np.asarray(rowptr, dtype=I64)
    col = np.asarray(col, dtype=I64)
    row = rows_of(rowptr)
    n = rowptr.size - 1
    mn, mx = np.minimum(row, col), np.maximum(row, col)
    order = np.lexsort((mx, mn, -_weights(col, w)))
    out = [-1] * n
    for u, v in zip(mn[order].tolist(), mx[order].tolist()):
        if u != v and out[u] < 0 and out[v] < 0:
            out[u] = out[v] = u
    return np.asarray([i if c < 0 else c for i, c in enumerate(out)], dtype=I64)


def finish(state):
    """graclus ids of a state: min(u, partner); undecided nodes closed as singletons"""
    state = np.asarray(state, dtype=I64)
    u = np.arange(state.size, dtype=I64)
    return np.where(state < 0, u, np.minimum(u, state))


def relabel(cluster):
    """consecutive_cluster: dense ids by ascending cluster id -> (cnew, count)"""
    uniq, inv = np.unique(np.asarray(cluster, dtype=I64), return_inverse=True)
    return inv.astype(I64).reshape(-1), int(uniq.size)


def pair_lists(state):
    """-> (cnew [N], segptr [nc + 1], members [N], nc) of a matching state: segment c = [representative, partner]"""
    state = np.asarray(state, dtype=I64)
    u = np.arange(state.size, dtype=I64)
    cnew, nc = relabel(finish(state))
    rep = (state < 0) | (state >= u)                 # undecided, singleton, or the smaller member of a pair
    pair = rep & (state > u)
    segptr = np.zeros(nc + 1, dtype=I64)
    segptr[1:] = np.cumsum(1 + pair[rep])
    members = np.empty(state.size, dtype=I64)
    members[segptr[:-1]] = u[rep]
    members[segptr[:-1][pair[rep]] + 1] = state[pair]
    return cnew, segptr, members, nc


def segment_csr(seg, nseg):
    """inverse lists of an index: members ascending inside a segment; entries outside [0, nseg) belong to none"""
    seg = np.asarray(seg, dtype=I64)
    lists = [[] for _ in range(nseg)]
    for i, s in enumerate(seg.tolist()):
        if 0 <= s < nseg:
            lists[s].append(i)
    return lists_to_csr(lists)


def lists_to_csr(lists):
    segptr = np.zeros(len(lists) + 1, dtype=I64)
    segptr[1:] = np.cumsum([len(l) for l in lists])
    members = np.asarray([m for l in lists for m in l], dtype=I64)
    return segptr, members


def compose_lists(segptr1, members1, segptr2, members2):
    """lists of fine -> mid -> coarse: segment c = the step-one segments of its step-two members, in that order"""
    lists = []
    for c in range(len(segptr2) - 1):
        l = []
        for m in members2[segptr2[c]:segptr2[c + 1]]:
            l += list(members1[segptr1[m]:segptr1[m + 1]])
        lists.append(l)
    return lists_to_csr(lists)


# ------------------------------------------------------------------------------------------------------ pool_edge
def pool_edge(cnew, row, col, w, nc=None):
    """-> (rowptr_c [nc + 1], row_c, col_c, w_c fp32 or None)"""
    cnew = np.asarray(cnew, dtype=I64)
    a, b = cnew[np.asarray(row, dtype=I64)], cnew[np.asarray(col, dtype=I64)]
    nc = int(cnew.max()) + 1 if nc is None else nc
    keep = a != b
    a, b = a[keep], b[keep]
    ww = None if w is None else np.asarray(w, dtype=np.float64)[keep]
    order = np.lexsort((b, a))
    a, b = a[order], b[order]
    head = np.ones(a.size, dtype=bool)
    head[1:] = (a[1:] != a[:-1]) | (b[1:] != b[:-1])
    start = np.nonzero(head)[0]
    row_c, col_c = a[start], b[start]
    w_c = None
    if ww is not None:
        ww = ww[order]
        end = np.append(start[1:], a.size)
        w_c = np.asarray([np.float32(ww[s:e].sum() / np.float64(e - s)) for s, e in zip(start, end)], dtype=np.float32)
    rowptr_c = np.zeros(nc + 1, dtype=I64)
    rowptr_c[1:] = np.cumsum(np.bincount(row_c, minlength=nc))
    return rowptr_c, row_c, col_c, w_c


def row_info(rowptr, segptr, members):
    """(r0, d0, r1, d1) per coarse node: start and length of the fine rows of its (one or two) members"""
    rowptr = np.asarray(rowptr, dtype=I64)
    out = np.zeros((len(segptr) - 1, 4), dtype=I64)
    for c in range(len(segptr) - 1):
        m = members[segptr[c]:segptr[c + 1]]
        assert 1 <= len(m) <= 2, 'a matching has one or two members per cluster'
        out[c, 0], out[c, 1] = rowptr[m[0]], rowptr[m[0] + 1] - rowptr[m[0]]
        if len(m) == 2:
            out[c, 2], out[c, 3] = rowptr[m[1]], rowptr[m[1] + 1] - rowptr[m[1]]
    return out


def row_gather_counts(rowptr, segptr, members):
    """d0 + d1 of each coarse node: the entries its wave gathers before relabelling"""
    ri = row_info(rowptr, segptr, members)
    return ri[:, 1] + ri[:, 3]


# ------------------------------------------------------------------------------------------------- segment reduce
def segment_max(x, segptr, members):
    """-> (out [nseg, C] in x's dtype, arg [nseg, C] int64): first maximum in list order by strict '>'"""
    x = np.asarray(x)
    nseg, C = len(segptr) - 1, x.shape[1]
    out, arg = np.zeros((nseg, C), dtype=x.dtype), -np.ones((nseg, C), dtype=I64)
    for s in range(nseg):
        for m in members[segptr[s]:segptr[s + 1]]:
            take = (arg[s] < 0) | (x[m] > out[s])
            out[s] = np.where(take, x[m], out[s])
            arg[s] = np.where(take, m, arg[s])
    return out, arg


def segment_max_bwd(gout, arg, seg, n_fine, gx=None):
    """row n receives gout of its segment where it was the arg-max; on top of gx if given (else zeros)"""
    gout = np.asarray(gout)
    out = np.zeros((n_fine, gout.shape[1]), dtype=gout.dtype) if gx is None else np.array(gx, dtype=gout.dtype)
    for n in range(n_fine):
        s = int(seg[n])
        if 0 <= s < gout.shape[0]:
            hit = arg[s] == n
            out[n] = np.where(hit, (out[n] + gout[s]).astype(gout.dtype), out[n])
    return out


def segment_max2(x, segptr1, members1, segptr2, members2):
    """Two segment_max steps composed -> (out [nseg2, C], arg12 = FINE row of the maximum).  Every step-one segment
    must be non-empty: an empty one would enter step two with the value 0, which is not what a composed list holds."""
    assert np.all(np.diff(segptr1) > 0), 'segment_max2 requires non-empty step-one segments'
    o1, a1 = segment_max(x, segptr1, members1)
    o2, a2 = segment_max(o1, segptr2, members2)
    cols = np.broadcast_to(np.arange(o2.shape[1]), a2.shape)
    arg12 = np.where(a2 >= 0, a1[np.maximum(a2, 0), cols], -1)
    return o2, arg12


def segment_sum(x, segptr, members):
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros((len(segptr) - 1, x.shape[1]))
    for s in range(len(segptr) - 1):
        for m in members[segptr[s]:segptr[s + 1]]:
            out[s] += x[m]
    return out


def segment_abs_sum(x, segptr, members):
    return segment_sum(np.abs(np.asarray(x, dtype=np.float64)), segptr, members)


def segment_mean(x, segptr, members):
    return segment_sum(x, segptr, members) / np.maximum(np.diff(segptr), 1)[:, None]


def segment_mean_bwd(gout, seg, segptr):
    gout = np.asarray(gout, dtype=np.float64)
    seg = np.asarray(seg, dtype=I64)
    return gout[seg] / np.maximum(np.diff(segptr), 1)[seg][:, None]


def segment_sum_bwd(gout, seg):
    """backward of a segment sum = the unpool gather"""
    return np.asarray(gout)[np.asarray(seg, dtype=I64)]


def segment_sum2(x, segptr1, members1, segptr2, members2):
    sp, mem = compose_lists(segptr1, members1, segptr2, members2)
    return segment_sum(x, sp, mem)


def exclusive_scan(v):
    v = np.asarray(v, dtype=I64)
    out = np.zeros(v.size, dtype=I64)
    out[1:] = np.cumsum(v)[:-1]
    return out


# --------------------------------------------------------------------------------------------------- edge weights
def sq_dist(x, row, col):
    x = np.asarray(x, dtype=np.float64)
    return ((x[row] - x[col]) ** 2).sum(1)


def edge_weight_t10(x, row, col, w_in=None):
    out = np.exp(-0.5 * sq_dist(x, row, col))
    return out if w_in is None else out + np.asarray(w_in, dtype=np.float64)


def edge_weight_att(x, att_l, att_r, row, col, w_in=None, dtype=np.float64):
    """sigmoid((al[r] + ar[c]) + (al[c] + ar[r])), averaged with w_in if given; dtype = np.float32 evaluates the same
    formula in single precision (the yardstick for what fp32 dot products can deliver)"""
    x, att_l, att_r = (np.asarray(a, dtype=dtype) for a in (x, att_l, att_r))
    al, ar = x @ att_l, x @ att_r
    alpha = (al[row] + ar[col]) + (al[col] + ar[row])
    with np.errstate(over='ignore'):
        sg = dtype(1) / (dtype(1) + np.exp(-alpha))
    return sg if w_in is None else (sg + np.asarray(w_in, dtype=dtype)) * dtype(0.5)


# ========================================================================================================= inputs
def csr_from_pairs(n, u, v, w=None):
    """symmetric CSR of the undirected pairs {u, v} (each once, u != v) -> (rowptr, col, w per entry or None)"""
    u, v = np.asarray(u, dtype=I64), np.asarray(v, dtype=I64)
    row, col = np.concatenate([u, v]), np.concatenate([v, u])
    order = np.lexsort((col, row))
    rowptr = np.zeros(n + 1, dtype=I64)
    rowptr[1:] = np.cumsum(np.bincount(row, minlength=n))
    ww = None if w is None else np.concatenate([w, w]).astype(np.float32)[order]
    return rowptr, col[order], ww


def random_graph(n, m, seed, ties=False):
    """m random undirected pairs (duplicates and loops removed); weights symmetric, fp32, optionally in quarters"""
    rng = np.random.RandomState(seed)
    a, b = rng.randint(0, n, m), rng.randint(0, n, m)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = np.unique(lo[lo != hi].astype(I64) * n + hi[lo != hi])
    w = rng.rand(key.size).astype(np.float32)
    if ties:
        w = np.floor(w * 4) / 4
    return csr_from_pairs(n, key // n, key % n, w)


def path_graph(n=600):
    """strictly decreasing weights along a path: one pair per round, n / 2 rounds"""
    u = np.arange(n - 1)
    return csr_from_pairs(n, u, u + 1, (n - u).astype(np.float32))


ROW_LENGTHS = (0, 1, 3, 4, 5, 8, 9, 40)


def row_length_graph(seed=5):
    """rows of exactly 0, 1, 3, 4, 5, 8, 9 and 40 entries: hubs with d leaves each (the MB = 4 batches of the round kernel
    end on a batch, one past it, on two batches and one past two); every third leaf also sits in a ring (rows of 3), so the
    matching is not trivial.  -> (rowptr, col, w, named = {row length: a node with that many entries})"""
    rng = np.random.RandomState(seed)
    u, v, named = [], [], {0: 0}                      # node 0 stays isolated
    n = 1
    for d in ROW_LENGTHS[2:]:
        for _ in range(3):
            hub = n
            named.setdefault(d, hub)
            n += 1
            for _ in range(d):
                u.append(hub); v.append(n); n += 1
    leaves = list(v)
    named[1] = leaves[0]
    ring = leaves[1::3]
    for a, b in zip(ring, ring[1:] + ring[:1]):
        u.append(a); v.append(b)
    w = (rng.randint(1, 64, len(u)) / 64.0).astype(np.float32)
    rowptr, col, ww = csr_from_pairs(n, u, v, w)
    return rowptr, col, ww, named


def match_cases():
    """name -> (rowptr, col, w): the inputs of the matching tests"""
    cases = {'path600': path_graph(600), 'row_lengths': row_length_graph()[:3]}
    rp, cl, w = random_graph(2000, 7000, 11)
    cases['negative'] = (rp, cl, (w - np.float32(0.5)) * np.float32(-3.0) - np.float32(2.0))      # all below zero
    cases['mixed_sign'] = (rp, cl, w - np.float32(0.5))
    cases['all_equal'] = (rp, cl, np.full(cl.size, 0.25, dtype=np.float32))
    cases['no_weights'] = (rp, cl, None)
    cases['ties'] = random_graph(3000, 9000, 12, ties=True)
    for n in (255, 256, 257):
        cases['n%d' % n] = random_graph(n, 3 * n, n)
    return cases


FORM_SIZES = (700, 70001, 262143, 262144, 300000)


def form_case(n):
    return random_graph(n, 3 * n, n + 1, ties=True)


# ---- edge coarsening
def _w12(rng, lo, hi, size):
    """multiples of 2^-12 in (lo, hi]: fp64 sums of a few hundred of them are exact in any order"""
    return (rng.randint(int(lo * 4096) + 1, int(hi * 4096) + 1, size) / 4096.0).astype(np.float32)


COARSEN_PAIRS = {2: (1, 1), 31: (16, 15), 32: (16, 16), 33: (17, 16), 63: (32, 31), 64: (32, 32), 65: (33, 32)}


def coarsen_case(with65, seed=3):
    """A symmetric simple graph whose heavy-edge matching leaves named coarse nodes with exact gather counts d0 + d1:

        pair<T>    a pair (a, b) joined by the heaviest weight (4.0), with T - 2 leaves of their own between them
                   (T = 2: the two rows hold only each other -- an empty coarse row).  The leaves of a gadget form a
                   ring with weights in (2, 3] and pair up among themselves, so several entries of the gathered row
                   relabel to the same coarse node (runs of duplicates, also across the two rows)
        hub64      a singleton with 64 neighbours that are all matched elsewhere (weight 3.5), so it gathers 64 distinct
                   keys: every lane a head, lane 63 included
        single1    a singleton with one entry, single0 an isolated node
    -> dict(rowptr, col, w, named = {name: fine node}, N); node ids are shuffled; N is no multiple of 4."""
    rng = np.random.RandomState(seed)
    u, v, w, named = [], [], [], {}
    n = 0

    def edge(a, b, ww):
        u.append(a); v.append(b); w.append(ww)

    for T, (da, db) in sorted(COARSEN_PAIRS.items()):
        if T == 65 and not with65:
            continue
        a, b = n, n + 1
        n += 2
        named['pair%d' % T] = a
        edge(a, b, 4.0)
        leaves = []
        for hub, d in ((a, da), (b, db)):
            for _ in range(d - 1):
                edge(hub, n, float(_w12(rng, 0, 2, 1)[0]))
                leaves.append(n)
                n += 1
        rng.shuffle(leaves)
        if len(leaves) == 2:
            edge(leaves[0], leaves[1], float(_w12(rng, 2, 3, 1)[0]))
        elif len(leaves) > 2:
            for x, y in zip(leaves, leaves[1:] + leaves[:1]):
                edge(x, y, float(_w12(rng, 2, 3, 1)[0]))
    hub = n
    n += 1
    named['hub64'] = hub
    for i in range(64):
        edge(hub, n, float(_w12(rng, 0, 2, 1)[0]))
        edge(n, n + 1, 3.5)
        if i == 0:
            edge(n, n + 2, float(_w12(rng, 0, 2, 1)[0]))
            named['single1'] = n + 2
            n += 1
        n += 2
    named['single0'] = n
    n += 1
    while n % 4 == 0 or n % 4 == 2:                    # an odd tail: the last block of four waves is ragged
        n += 1
    perm = rng.permutation(n)
    rowptr, col, ww = csr_from_pairs(n, perm[np.asarray(u)], perm[np.asarray(v)], np.asarray(w, dtype=np.float32))
    return dict(rowptr=rowptr, col=col, w=ww, named={k: int(perm[x]) for k, x in named.items()}, N=n)


COARSEN_ROUNDS = 64


def run64_case(seed=4):
    """A symmetric MULTIgraph with a hand-made state (no pair is matched unless stated): node 0 and node 1 are singletons
    joined by 64 parallel entries -- each gathers 64 entries that all relabel to the other: one run of duplicates that
    fills the wave; the pair (2, 3) and the singleton 4: 15 + 16 parallel entries to node 4 (with the two mutual entries
    33 gathered: the 64-wide stage runs, one run of 31 behind two dropped self entries).
    -> dict(rowptr, col, w, state, N)"""
    rng = np.random.RandomState(seed)
    row = [0] * 64 + [1] * 64 + [2] * 16 + [3] * 17 + [4] * 31
    col = [1] * 64 + [0] * 64 + [3] + [4] * 15 + [2] + [4] * 16 + [2] * 15 + [3] * 16
    n = 5
    rowptr = np.zeros(n + 1, dtype=I64)
    rowptr[1:] = np.cumsum(np.bincount(row, minlength=n))
    return dict(rowptr=rowptr, col=np.asarray(col, dtype=I64), w=_w12(rng, 0, 4, len(col)),
                state=np.asarray([0, 1, 3, 2, 4], dtype=I64), N=n)


# ---- segment reductions
SEG_CHANNELS = (1, 3, 4, 64, 128, 130)


def segment_case(C, seed=7):
    """Two-step lists over n_fine rows plus features with the values selections go wrong on.

    step one (fine -> mid): segments of 1..5 members and one of 1000, every one non-empty, members in shuffled order;
    two fine rows belong to no segment.  step two (mid -> coarse): segments of 0..3 members, an EMPTY one between full
    ones, members not ascending.  x: a mid segment whose values are all negative; -0.0 before +0.0 and the reverse; +inf
    and -inf; exact ties inside a step-one segment and ties that straddle two step-one segments of one coarse segment.
    -> dict(x, x_finite, segptr1, members1, segptr2, members2, seg1, seg12, n_fine, n_mid, n_coarse)"""
    rng = np.random.RandomState(seed + C)
    sizes = [1000] + list(rng.randint(1, 6, 160))
    n_mid = len(sizes)
    n_fine = int(np.sum(sizes)) + 2
    perm = rng.permutation(n_fine)
    lists1, o = [], 0
    for s in sizes:
        lists1.append(list(perm[o:o + s]))
        o += s
    loose = perm[o:]                                         # rows of no segment
    segptr1, members1 = lists_to_csr(lists1)
    mids = list(rng.permutation(n_mid))
    lists2 = []
    while mids:
        k = int(rng.randint(0, 4))
        if len(lists2) == 3:
            k = 0                                            # an empty segment between full ones
        lists2.append([mids.pop() for _ in range(min(k, len(mids)))])
    lists2.append([])                                        # and one at the end
    segptr2, members2 = lists_to_csr(lists2)
    x = rng.randn(n_fine, C).astype(np.float32)
    big = lists1[0]
    x[big[10]], x[big[500]] = 7.5, 7.5                       # the same maximum twice in the 1000-member segment
    # coarse segments with two or more mid members: ties / zeros / infinities across step-one segments
    multi = [l for l in lists2 if len(l) >= 2 and 0 not in l]
    for k, l in enumerate(multi[:6]):
        f0, f1 = lists1[l[0]][-1], lists1[l[1]][0]
        if k == 0:
            x[f0], x[f1] = 9.0, 9.0                          # a tie that straddles two step-one segments
        elif k in (1, 2):                                    # zeros only: -0.0 first (k = 1), +0.0 first (k = 2)
            for j, m in enumerate(l):
                x[lists1[m]] = (-0.0 if j == 0 else 0.0) if k == 1 else (0.0 if j == 0 else -0.0)
        elif k == 3:
            x[f0], x[f1] = np.inf, np.inf
        elif k == 4:
            for m in l:
                x[lists1[m]] = -np.inf                       # a coarse segment of -inf only
        else:
            x[f0, ::2], x[f1, 1::2] = -np.inf, np.inf
    for l in multi[6:8] + [l for l in lists2 if len(l) == 1][:2]:      # coarse segments whose values are all negative
        for m in l:
            x[lists1[m]] = -np.abs(x[lists1[m]]) - 1.0
    seg1 = -np.ones(n_fine, dtype=I64)
    for m, l in enumerate(lists1):
        seg1[l] = m
    mid2 = -np.ones(n_mid, dtype=I64)
    for c, l in enumerate(lists2):
        mid2[l] = c
    seg12 = np.where(seg1 >= 0, mid2[np.maximum(seg1, 0)], -1)
    assert len(loose) == 2 and np.all(seg1[loose] < 0)
    x_finite = np.where(np.isfinite(x), x, np.sign(x) * 3.0).astype(np.float32)
    return dict(x=x, x_finite=x_finite, segptr1=segptr1, members1=members1, segptr2=segptr2, members2=members2, seg1=seg1,
                seg12=seg12, n_fine=n_fine, n_mid=n_mid, n_coarse=len(lists2))


# ---- edge weights
EW_CHANNELS = (3, 6, 12, 36, 64, 128)


def edge_weight_case(C, seed=9):
    """n nodes, E edges: random pairs whose squared distance stays below 160 (exp(-80) is still a normal fp32 number),
    every node once with itself (row == col), and pairs built to lie at squared distance ~ 80.  att_l / att_r are scaled
    so that alpha spreads over about +-10, and the last 8 nodes are blown up so that it reaches beyond +-100.
    -> dict(x, row, col, w_in, att_l, att_r, x_att, n, E)"""
    rng = np.random.RandomState(seed + C)
    n = 400
    x = (rng.randn(n, C) * np.sqrt(10.0 / C)).astype(np.float32)
    for k in range(20):                                     # node 2k+1 = node 2k moved by sqrt(80) along a random direction
        d = rng.randn(C)
        x[2 * k + 1] = (x[2 * k].astype(np.float64) + d / np.linalg.norm(d) * np.sqrt(80.0)).astype(np.float32)
    row, col = rng.randint(0, n, 4000), rng.randint(0, n, 4000)
    keep = sq_dist(x, row, col) < 160.0
    far = np.arange(20) * 2
    row = np.concatenate([row[keep], np.arange(n), far, far + 1])
    col = np.concatenate([col[keep], np.arange(n), far + 1, far])
    w_in = rng.rand(row.size).astype(np.float32)
    att_l = (rng.randn(C) * 2.5 / np.sqrt(C)).astype(np.float32)
    att_r = (rng.randn(C) * 2.5 / np.sqrt(C)).astype(np.float32)
    x_att = rng.randn(n, C).astype(np.float32)
    x_att[-8:] *= 25.0
    return dict(x=x, row=row.astype(I64), col=col.astype(I64), w_in=w_in, att_l=att_l, att_r=att_r, x_att=x_att, n=n,
                E=int(row.size))


SCAN_SIZES = (1, 15, 16, 16383, 16384, 16385, 32768, 32769, 100003, 262144, 262145)


def scan_case(n):
    return np.random.RandomState(n).randint(0, 65, n).astype(np.int32)
