"""The FeaSt kernels row by row, on a ladder of degrees and at the edges of their tiles (inputs, metric and runners:
tests/feast_cases.py; what keeps those honest: tests/test_feast_cases_host.py).

Bar: every ROW of out and dx within 1e-5 of the fp64 oracle relative to that row's own largest value (feast_cases.row_err),
the four parameter gradients within 1e-5 of the tensor's largest value, everything finite.  Inputs are unit scale; the
oracle evaluated in fp32 stays below a quarter of the bar on every one of them (asserted on the host).  A failure names the
worst rows by node id, in-degree, out-degree and position in the 16- and the 32-row tile.

Measured on the MI355X over the 217 printed cases of this file, worst kernel distance (worst fp32 oracle distance):
  out, per row           1.74e-06 (6.12e-07)   ladder 128 -> 128, 16-row tiles
  dx, per row            2.18e-06 (1.64e-06)   ring of 128 nodes, 128 -> 128, 16-row tiles; on the ladder 1.79e-06
  dlin.weight            3.95e-07 (1.09e-06)
  du.weight              7.05e-07 (1.42e-06)
  dc                     8.40e-07 (5.19e-07)
  dbias                  3.86e-07 (2.03e-07)
Every case is inside the bar by a factor of four or more.
"""
import pytest
import torch

import feast_cases as F

pytestmark = pytest.mark.gpu

FUSED = [True, 32, False]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


def _check(label, name, Cin, Cout, slope, got):
    """One printed line (kernel and fp32 oracle, each from the fp64 oracle), then the bars."""
    ref, f32 = F.run_oracle(name, Cin, Cout, slope), F.run_oracle_fp32(name, Cin, Cout, slope)
    _, _, info = F.graph_of_name(name)
    d, y = F.distances(got, ref), F.distances(f32, ref)
    print('%s %s %d -> %d slope %.1f: kernel (fp32 oracle) %s' % (
        label, name, Cin, Cout, slope, ' '.join('%s %.2e (%.2e)' % (k, d[k], y[k]) for k in F.KEYS)))
    for k in F.KEYS:
        assert got[k].shape == ref[k].shape and got[k].dtype == torch.float32, k
        assert bool(torch.isfinite(got[k]).all()), '%s %s: %s is not finite' % (label, name, k)
    for k in F.ROW_KEYS:
        assert not F.floor_engages(ref[k]), k
        assert d[k] < F.BAR, '%s %s %d -> %d: %s per row %.2e (fp32 oracle %.2e); worst rows: %s' % (
            label, name, Cin, Cout, k, d[k], y[k], F.worst_rows(got[k], ref[k], info))
    for k in F.KEYS:
        assert d[k] < F.BAR, '%s %s %d -> %d: %s %.2e (fp32 oracle %.2e)' % (label, name, Cin, Cout, k, d[k], y[k])


def _assert_same_bits(a, b, what):
    for k in F.KEYS:
        assert torch.equal(a[k], b[k]), '%s: %s differs' % (what, k)


@pytest.mark.parametrize('fused', FUSED)
@pytest.mark.parametrize('Cin,Cout,slope,split', F.FEAST_PRODUCT)
def test_feast_degree_ladder(dev, Cin, Cout, slope, split, fused):
    """Every (Cin, Cout, split) the C ABI accepts x the three launch geometries on ladder_graph(): in- and out-degrees
    0 .. 80 around every multiple of the 16-edge chunk, an isolated block, a one-node ragged tile, surplus workgroups."""
    got = F.run_gpu(dev, 'ladder', Cin, Cout, slope, split, fused=fused)
    _check('ladder fused=%s split=%d' % (fused, split), 'ladder', Cin, Cout, slope, got)


@pytest.mark.parametrize('Cout,slope,split', [(32, 0.2, False), (32, 1.0, True), (64, 1.0, False), (64, 0.2, True),
                                              (128, 0.2, False), (128, 1.0, True)])
def test_feast_ladder_rowpass_forms(dev, Cout, slope, split):
    """The three forms of the 64-channel backward row pass (geobi_set_rowpass_form: lane-private, staged through LDS,
    channel-chunked on 32-node tiles) on the ladder; lane-private and staged run the same FMAs in the same order."""
    from geobi_gnn_amd import _lib as L
    got = {}
    try:
        for form in ((0, 0), (1, 0), (0, 1)):
            L.call('geobi_set_rowpass_form', *form)
            got[form] = F.run_gpu(dev, 'ladder', 64, Cout, slope, split)
            _check('rowpass form=%s split=%d' % (form, split), 'ladder', 64, Cout, slope, got[form])
    finally:
        L.call('geobi_set_rowpass_form', -1, -1)
    _assert_same_bits(got[(0, 0)], got[(1, 0)], 'lane-private and staged row pass')


@pytest.mark.parametrize('Cin,Cout,split', [(128, 32, False), (128, 64, False), (128, 64, True), (128, 128, False),
                                            (64, 128, False)])
def test_feast_ladder_column_parts(dev, Cin, Cout, split):
    """Layers that read 128 channels with every tile on one workgroup and on two (geobi_set_column_parts): both within the
    bar per row, and bit for bit the same."""
    from geobi_gnn_amd import _lib as L
    got = {}
    try:
        for parts in (1, 2):
            L.call('geobi_set_column_parts', parts)
            got[parts] = F.run_gpu(dev, 'ladder', Cin, Cout, 0.2, split)
            _check('column parts=%d split=%d' % (parts, split), 'ladder', Cin, Cout, 0.2, got[parts])
    finally:
        L.call('geobi_set_column_parts', 0)
    _assert_same_bits(got[1], got[2], 'one and two column parts')


@pytest.mark.parametrize('fused', FUSED)
@pytest.mark.parametrize('Cin,Cout', F.RING_SHAPES)
@pytest.mark.parametrize('n', F.RING_SIZES)
def test_feast_tile_edges(dev, n, Cin, Cout, fused):
    """Rings of N nodes around the tile sizes: N = 1 has no edge at all, 128 is eight full 16-row tiles (a grid without
    surplus workgroups), 129 nine tiles (seven surplus workgroups and a one-node ragged tile)."""
    name = 'ring%d' % n
    got = F.run_gpu(dev, name, Cin, Cout, 0.2, False, fused=fused)
    _check('ring fused=%s' % (fused,), name, Cin, Cout, 0.2, got)


@pytest.mark.parametrize('fused', FUSED)
@pytest.mark.parametrize('Cin,Cout,split', [(ci, co, (ci, co) == (128, 64)) for ci, co in F.REVERSED_SHAPES])
def test_feast_ladder_reversed(dev, Cin, Cout, split, fused):
    """Every edge of the ladder flipped: the forward walk meets the row lengths the dx walk had, at its node positions,
    and the other way round."""
    got = F.run_gpu(dev, 'ladder_rev', Cin, Cout, 0.2, split, fused=fused)
    _check('reversed fused=%s split=%d' % (fused, split), 'ladder_rev', Cin, Cout, 0.2, got)
