"""tests/feast_cases.py kept honest: the ladder graph has the degrees it promises, the fp32 oracle sits a factor of four
below the bar of tests/test_gpu_feast_edges.py on every input used there, the floor of row_err never engages on the
references, and faults planted into the fp64 oracle's inputs or outputs (edges beyond a chunk boundary dropped, one row
off by 1e-4) are flagged at exactly the rows they touch.  No GPU.

Measured with the seeds of feast_cases.seed_of over the ladder (both slopes), the reversed ladder and the rings: the fp32
oracle is 0.9e-7 .. 7.2e-7 per row from fp64 for out, 1.7e-7 .. 1.8e-6 for dx (the largest: 6 -> 128 on the ladder; the
6-channel layers are the only ones above 1.1e-6), and <= 1.2e-6 of the tensor's maximum for the parameter gradients, so
a quarter of the bar, 2.5e-6, holds.  The smallest row of a reference is >= 17 % of the tensor's maximum for out and
>= 0.7 % for dx (32 -> 32 on the ladder), seven times the floor of row_err."""
import pytest
import torch

import feast_cases as F
from helpers import rel_err

QUARTER = F.BAR / 4

LADDER_SHAPES = [(ci, co) for ci in (6, 12, 32, 64, 128) for co in (32, 64, 128)]


# ------------------------------------------------------------------------------- graphs
def test_ladder_graph_properties():
    ei, n, info = F.ladder_graph()
    assert n == 161 and n % 32 == 1 and n % 16 == 1
    assert ei.dtype == torch.long and ei.shape == (2, 1352)
    assert int(ei.min()) >= 0 and int(ei.max()) < n
    assert not bool((ei[0] == ei[1]).any())                                  # no self loops
    assert torch.unique(ei[0] * n + ei[1]).numel() == ei.shape[1]            # no duplicates
    L, D = F.L, torch.tensor(F.D)
    assert torch.equal(info.indeg[:L], D) and torch.equal(info.outdeg[L:2 * L], D)
    assert int(info.outdeg[:L].sum()) == 0 and int(info.indeg[L:2 * L].sum()) == 0
    pool = slice(2 * L, 2 * L + F.POOL)
    assert 5 <= int(info.indeg[pool].min()) and int(info.indeg[pool].max()) <= 9
    assert int(info.indeg[144:160].sum()) == 0 and int(info.outdeg[144:160].sum()) == 0     # the isolated block
    assert int(info.indeg[160]) == 33 and int(info.outdeg[160]) == 17
    assert int(((info.indeg == 0) & (info.outdeg == 0)).sum()) == 18
    # the four nodes a wave works on side by side (ids 4k .. 4k + 3) walk different numbers of 16-edge chunks
    for side in (info.indeg, info.outdeg[L:]):
        for k in range(2, L // 4):
            assert torch.unique((side[4 * k:4 * k + 4] + 15) // 16).numel() > 1
    for quad in ((15, 16, 17, 18), (31, 32, 33, 34)):
        i0 = F.D.index(quad[0])
        assert tuple(F.D[i0:i0 + 4]) == quad
    # built from arithmetic: twice the same graph, and the caller's copy is its own
    ei2, _, _ = F.ladder_graph()
    assert torch.equal(ei, ei2) and ei.data_ptr() != ei2.data_ptr()
    rev, _, rinfo = F.graph_of_name('ladder_rev')
    assert torch.equal(rev, ei.flip(0)) and torch.equal(rinfo.indeg, info.outdeg) and torch.equal(rinfo.outdeg, info.indeg)


def test_ladder_grid_shape():
    """11 tiles of 16 rows padded to 16 workgroups, 6 tiles of 32 rows padded to 8; node 160 alone in the last tile."""
    n = F.N_LADDER
    for rows, tiles, grid in ((16, 11, 16), (32, 6, 8)):
        assert -(-n // rows) == tiles and -(-tiles // 8) * 8 == grid and n - (tiles - 1) * rows == 1


@pytest.mark.parametrize('n', F.RING_SIZES)
def test_ring_graph(n):
    ei = F.ring_graph(n)
    want = {1: 0, 2: 2}.get(n, 2 * n)
    assert ei.dtype == torch.long and ei.shape == (2, want)
    if n > 1:
        key = ei[0] * n + ei[1]
        assert torch.unique(key).numel() == want and not bool((ei[0] == ei[1]).any())
        assert torch.equal(torch.sort(key).values, torch.sort(ei[1] * n + ei[0]).values)        # symmetric
        assert bool((((ei[0] - ei[1]) % n == 1) | ((ei[1] - ei[0]) % n == 1)).all())
        info = F.GraphInfo(ei, n)
        assert int(info.indeg.min()) == int(info.indeg.max()) == (1 if n == 2 else 2)


def test_row_err_is_per_row():
    b = torch.tensor([[100.0, -50.0], [0.0, 1.0], [0.0, 0.0]], dtype=torch.double)
    a = b.clone(); a[1, 1] += 1e-3; a[2, 0] += 1e-3
    e = F.row_errs(a, b)
    assert e[0] == 0 and abs(float(e[1]) - 1e-3) < 1e-12
    assert abs(float(e[2]) - 1e-3 / (F.FLOOR * 100.0)) < 1e-12              # the row of zeros: the floor, not a division by 0
    assert F.row_err(a, b) == float(e.max()) and F.floor_engages(b) and not F.floor_engages(b[:2])
    assert rel_err(a, b) == pytest.approx(1e-5)


# ------------------------------------------------------------------- fp32 oracle distance
def _check_fp32_distance(name, Cin, Cout, slope):
    ref, f32 = F.run_oracle(name, Cin, Cout, slope), F.run_oracle_fp32(name, Cin, Cout, slope)
    assert all(ref[k].dtype == torch.double and f32[k].dtype == torch.float32 for k in F.KEYS)
    for k in F.ROW_KEYS:
        assert not F.floor_engages(ref[k]), (k, F.row_share(ref[k]))
    d = F.distances(f32, ref)
    print('%s %d -> %d slope %.1f: fp32 oracle %s; smallest row out %.3f dx %.3f of the max'
          % (name, Cin, Cout, slope, ' '.join('%s %.2e' % (k, d[k]) for k in F.KEYS), F.row_share(ref['out']),
             F.row_share(ref['dx'])))
    assert max(d.values()) <= QUARTER, d


@pytest.mark.parametrize('Cin,Cout', LADDER_SHAPES)
def test_fp32_oracle_distance_on_the_ladder(Cin, Cout):
    """Both slopes: the device tests alternate them over the (Cin, Cout, split) product."""
    for slope in (0.2, 1.0):
        _check_fp32_distance('ladder', Cin, Cout, slope)


@pytest.mark.parametrize('Cin,Cout', F.REVERSED_SHAPES)
def test_fp32_oracle_distance_on_the_reversed_ladder(Cin, Cout):
    _check_fp32_distance('ladder_rev', Cin, Cout, 0.2)


@pytest.mark.parametrize('n', F.RING_SIZES)
def test_fp32_oracle_distance_on_rings(n):
    for Cin, Cout in F.RING_SHAPES:
        _check_fp32_distance('ring%d' % n, Cin, Cout, 0.2)


def test_runner_draws_fp32_numbers_and_leaves_the_rng_alone():
    torch.manual_seed(123)
    before = torch.get_rng_state()
    params, x, gout = F.draw(12, 32, 161, 999)
    assert torch.equal(torch.get_rng_state(), before)
    assert x.dtype == gout.dtype == torch.float32 and x.shape == (161, 12) and gout.shape == (161, 32)
    assert sorted(params) == ['bias', 'c', 'lin.weight', 'u.weight']
    assert 0.9 < float(x.std()) < 1.1                                        # unit scale


# --------------------------------------------------------------------------- planted faults
def _in_csr_position(ei, n):
    """position of every edge in the row of its target, rows (target, source)-sorted as the in-CSR is"""
    order = torch.argsort(ei[1] * n + ei[0])
    tgt = ei[1][order]
    start = torch.zeros(n + 1, dtype=torch.long)
    start[1:] = torch.cumsum(torch.bincount(tgt, minlength=n), 0)
    pos = torch.empty_like(order)
    pos[order] = torch.arange(ei.shape[1]) - start[tgt]
    return pos


@pytest.mark.parametrize('Cin,Cout', [(12, 32), (64, 64), (128, 128)])
@pytest.mark.parametrize('keep', [16, 32])
def test_dropped_chunks_are_flagged_at_their_rows(Cin, Cout, keep):
    """A walk that stops after `keep` edges of a row: out is wrong at exactly the nodes of in-degree > keep."""
    ei, n, info = F.ladder_graph()
    ref = F.run_oracle('ladder', Cin, Cout, 0.2)
    cut = ei[:, _in_csr_position(ei, n) < keep]
    bad = F.run_oracle_on(cut, n, Cin, Cout, 0.2, F.seed_of(Cin, Cout))
    e = F.row_errs(bad['out'], ref['out'])
    assert F.row_err(bad['out'], ref['out']) > F.BAR
    want = torch.nonzero(info.indeg > keep).flatten()
    assert torch.equal(torch.nonzero(e > F.BAR).flatten(), want), F.worst_rows(bad['out'], ref['out'], info)
    assert set(want.tolist()) == {i for i, d in enumerate(F.D) if d > keep} | {160}
    assert float(e[info.indeg <= keep].max()) == 0.0


@pytest.mark.parametrize('Cin,Cout', [(12, 32), (64, 64), (128, 128)])
def test_one_dropped_edge_is_flagged(Cin, Cout):
    """The 17th edge of the node of in-degree 17 (the only item of its second chunk) goes missing."""
    ei, n, info = F.ladder_graph()
    node = F.D.index(17)
    ref = F.run_oracle('ladder', Cin, Cout, 0.2)
    pos = _in_csr_position(ei, n)
    drop = (ei[1] == node) & (pos == 16)
    assert int(drop.sum()) == 1
    bad = F.run_oracle_on(ei[:, ~drop], n, Cin, Cout, 0.2, F.seed_of(Cin, Cout))
    e = F.row_errs(bad['out'], ref['out'])
    assert torch.equal(torch.nonzero(e > F.BAR).flatten(), torch.tensor([node]))
    report = F.worst_rows(bad['out'], ref['out'], info, k=1)
    assert report.startswith('node %d (in-degree 17, out-degree 0, row %d of 16-row tile 0, row %d of 32-row tile 0)'
                             % (node, node, node)), report


@pytest.mark.parametrize('Cin,Cout', [(12, 32), (64, 64), (128, 128)])
def test_small_row_off_by_1e4_passes_rel_err_but_not_row_err(Cin, Cout):
    """The gap this metric closes: one ordinary pool row of dx off by 1e-4 of itself stays under the tensor metric's
    1e-5 as long as the row is under a tenth of the tensor's maximum."""
    ref = F.run_oracle('ladder', Cin, Cout, 0.2)['dx']
    pool = torch.arange(2 * F.L, 2 * F.L + F.POOL)
    rows = ref.abs().amax(1)
    node = int(pool[torch.argmin(rows[pool])])
    assert float(rows[node]) < 0.1 * float(rows.max())
    bad = ref.clone()
    bad[node] *= 1 + 1e-4
    assert rel_err(bad, ref) < 1e-5
    e = F.row_errs(bad, ref)
    assert F.row_err(bad, ref) > F.BAR and torch.equal(torch.nonzero(e > F.BAR).flatten(), torch.tensor([node]))
    assert float(e[node]) == pytest.approx(1e-4, rel=1e-6)
