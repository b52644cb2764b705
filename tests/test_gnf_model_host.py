"""Anchors of tests/gnf_model.py (the reference of tests/test_gpu_gnf.py) and the host side of `denoise --method gnf`:
no device needed."""
import numpy as np
import pytest
import torch

import bnf_model as B
import gnf_model as M
import geom_model as G
from test_bnf_model_host import _flat_patch


def test_flat_patch_is_a_fixed_point():
    """A flat triangulated square: every difference of normals is exactly 0, so H = 0 everywhere, every selection is the
    lowest index of the row, and the normals come back bit for bit."""
    pts, faces = _flat_patch()
    topo = M.Topology(faces, pts.shape[0])
    for dtype in (torch.float64, torch.float32):
        hist, sel = M.guided_normals(pts.to(dtype), faces, normal_iters=3, history=True, return_selection=True, topo=topo)
        assert float(M.patch_measure(hist[0], topo).abs().max()) == 0.0
        for n in hist[1:]:
            assert torch.equal(n, hist[0])
        lowest = topo.patch[:, 0]
        assert torch.equal(sel, lowest.expand_as(sel))


def test_clean_cube_ties_go_to_the_lowest_index():
    """cube(2), clean: the normals are exact axis vectors, so every difference is 0 or sqrt(2) and congruent patches tie
    EXACTLY (the model adds the terms of R in ascending order).  Every selection is the lowest index among the row's
    minima, and no two H values are close without being equal -- a near-tie would be a tie the arithmetic broke."""
    pts, faces = M.cube(2)
    assert faces.shape[0] == 48 and pts.shape[0] == 26
    topo = M.Topology(faces, pts.shape[0])
    n = B.face_records(pts, faces)[2]
    assert set(n.abs().flatten().tolist()) == {0.0, 1.0}
    H = M.patch_measure(n, topo)
    values = torch.unique(H)
    assert values.numel() >= 2 and values.numel() < H.numel()                 # ties exist, and not everything is tied
    assert float((values[1:] - values[:-1]).min()) > 1e-6                       # distinct values are far apart
    sel = M.select(H, topo)
    tied = 0
    for i in range(topo.F):
        row = topo.patch[i][topo.valid[i]]
        least = H[row].min()
        ties = row[H[row] == least]
        tied += int(ties.numel() > 1)
        assert int(sel[i]) == int(ties.min()) and int(sel[i]) in row.tolist()
    assert tied > 0
    # fp32 gives the same selections on this mesh: its differences are exact too (0 or fl(sqrt 2), sums of <= 2^k terms)
    assert torch.equal(M.select(M.patch_measure(n.float(), topo), topo), sel)


def test_lone_face():
    pts = torch.tensor([[0.1, 0.2, 0.3], [1.3, 0.1, 0.2], [0.4, 1.1, 0.9]], dtype=torch.float64)
    faces = torch.tensor([[0, 1, 2]])
    f = M.Filter(pts, faces)
    start = f.n.clone()
    assert float(f.measure()[0]) == 0.0
    sel = M.select(f.measure(), f.topo)
    assert sel.tolist() == [0]
    g = M.guidance(f.n, f.area, sel, f.topo)
    assert float((g - start).abs().max()) <= 2.3e-16                            # s / |s| of one unit vector
    f.step()
    assert float((f.n - start).abs().max()) <= 2.3e-16
    got = M.guided_normals(pts, faces, normal_iters=3)
    assert float((got - start).abs().max()) <= 1e-15


def _flag_matrix(faces, V):
    topo = M.Topology(faces, V)
    return topo, topo.pairs


def test_edge_pair_flags():
    """Three faces on one edge: all three pairs are edge pairs; the face that touches one vertex is in their patches but in
    no pair.  A duplicate face is an edge pair with its twin (3 common ids) and with the twin's edge neighbours.  [0, 0, 3]
    has the two distinct ids {0, 3}: an edge pair with a face holding both, not with one holding only 0."""
    pts, faces = M.three_on_an_edge()
    topo, pairs = _flag_matrix(faces, pts.shape[0])
    want = torch.zeros((4, 4), dtype=torch.bool)
    for j, m in ((0, 1), (0, 2), (1, 2)):
        want[j, m] = want[m, j] = True
    assert torch.equal(pairs, want)
    assert topo.patch[3][topo.valid[3]].tolist() == [0, 3] and topo.patch[0][topo.valid[0]].tolist() == [0, 1, 2, 3]
    assert topo.csr_flags().tolist() == [1, 1, 0, 1, 1, 1, 1, 0]               # rows 0 | 1 | 2 | 3, loop-free
    # both copies of the face see each other and the neighbour across 1-2; the sliver [0, 0, 3] pairs with [0, 3, 1] only
    faces = torch.tensor([[0, 1, 2], [0, 1, 2], [2, 1, 4], [0, 0, 3], [0, 3, 1], [4, 5, 6]])
    _, pairs = _flag_matrix(faces, 7)
    want = torch.zeros((6, 6), dtype=torch.bool)
    for j, m in ((0, 1), (0, 2), (1, 2), (3, 4), (0, 4), (1, 4)):
        want[j, m] = want[m, j] = True
    assert torch.equal(pairs, want)
    # symmetric, loop-free on a real mesh; every face of a closed manifold has exactly three
    pts, faces = G.sphere(4, 0.3, 1)
    _, pairs = _flag_matrix(faces, pts.shape[0])
    assert torch.equal(pairs, pairs.T) and not bool(pairs.diagonal().any()) and bool((pairs.sum(1) == 3).all())


def test_measure_by_hand():
    """Two faces over an edge: one patch {0, 1}, one edge pair: Phi = |n_0 - n_1| = d, R = d / (1e-9 + d)."""
    pts = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.5, -1.0, 1.0]], dtype=torch.float64)
    faces = torch.tensor([[0, 1, 2], [1, 0, 3]])
    f = M.Filter(pts, faces)
    d = float((f.n[0] - f.n[1]).norm())
    H = f.measure()
    assert np.allclose(H.numpy(), [d * d / (1e-9 + d)] * 2, rtol=1e-15)
    sel = M.select(H, f.topo)
    assert sel.tolist() == [0, 0]                                               # an exact tie: the lowest index
    g = M.guidance(f.n, f.area, sel, f.topo)
    s = f.area[0] * f.n[0] + f.area[1] * f.n[1]
    assert np.allclose(g.numpy(), np.stack([(s / s.norm()).numpy()] * 2), atol=1e-15)
    # g_0 = g_1: the range term is 1, the sweep is the area- and distance-weighted mean
    before = f.n.clone()
    f.step()
    w = float(torch.exp(-f.a * (f.cen[0] - f.cen[1]).pow(2).sum()))
    s0 = f.area[0] * before[0] + f.area[1] * w * before[1]
    assert np.allclose(f.n[0].numpy(), (s0 / s0.norm()).numpy(), atol=1e-15)


def test_guided_beats_bilateral_at_high_noise():
    """cube(8) with gaussian vertex noise of 0.3 x the grid spacing, sigma_r 0.35, sigma_s 1, 20 sweeps, fp64 models: the
    guided filter's mean angle to the clean normals is below the bilateral filter's."""
    noisy, clean, faces = M.noisy_cube(8, 0.3, seed=0)
    assert faces.shape[0] == 768
    nt = B.face_records(clean, faces)[2]
    before = B.mean_angle_deg(B.face_records(noisy, faces)[2], nt)
    hist = M.guided_normals(noisy, faces, normal_iters=20, history=True)
    bhist = B.bilateral_normals(noisy, faces, normal_iters=20, history=True)
    gnf10, gnf20 = B.mean_angle_deg(hist[10], nt), B.mean_angle_deg(hist[20], nt)
    bnf10, bnf20 = B.mean_angle_deg(bhist[10], nt), B.mean_angle_deg(bhist[20], nt)
    print('cube(8), noise 0.3: input %.2f degrees; 10 sweeps GNF %.2f BNF %.2f; 20 sweeps GNF %.2f BNF %.2f'
          % (before, gnf10, bnf10, gnf20, bnf20))
    assert gnf20 < bnf20


def test_fp32_model_stays_near_the_fp64_model():
    """d32 of the GPU test's bars: the fp32 model against the fp64 model, both replaying the fp64 model's selections (a
    selection is discrete: a near-tie that fp32 resolves the other way is another filter, not a rounding)."""
    for name, (pts, faces) in (('sphere4', G.sphere(4, 0.3, 1)), ('sphere8', G.sphere(8, 0.3, 1)),
                               ('cube4', M.noisy_cube(4, 0.3, 1)[::2])):
        topo = M.Topology(faces, pts.shape[0])
        ref, sel = M.guided_normals(pts, faces, normal_iters=5, return_selection=True, topo=topo)
        f32 = M.guided_normals(pts.float(), faces, normal_iters=5, selection=sel, topo=topo)
        d32 = float((f32.double() - ref).abs().max())
        n0 = B.face_records(pts, faces)[2]
        dH = float((M.patch_measure(n0.float(), topo).double() - M.patch_measure(n0, topo)).abs().max())
        print('%s: d32 after 5 sweeps %.3g, of H on the start normals %.3g' % (name, d32, dH))
        assert d32 < 1e-5 and dH < 1e-5


# ------------------------------------------------------------------------------------------------ command line, module
def test_parser_accepts_the_guided_method():
    from geobi_gnn_amd.__main__ import denoise, parse_args
    opt = parse_args(['denoise', '--data_dir', 'D', '--method', 'gnf'])
    assert opt.fn is denoise and opt.method == 'gnf'
    assert (opt.normal_iters, opt.sigma_r, opt.sigma_s) == (20, 0.35, 1.0)
    assert opt.n_iter == 60 and not getattr(opt, 'n_iter_given', False)       # the filter then takes its own 20
    opt = parse_args(['denoise', '--data_dir', 'D', '--method', 'gnf', '--normal_iters', '5', '--sigma_r', '0.2',
                      '--sigma_s', '2', '--n_iter', '7'])
    assert (opt.normal_iters, opt.sigma_r, opt.sigma_s, opt.n_iter, opt.n_iter_given) == (5, 0.2, 2.0, 7, True)


@pytest.mark.parametrize('extra', [['--model', 'net.pt'], ['--sigma_r', '0'], ['--normal_iters', '-1']])
def test_parser_rejects(extra, capsys):
    from geobi_gnn_amd.__main__ import parse_args
    with pytest.raises(SystemExit) as e:
        parse_args(['denoise', '--data_dir', 'D', '--method', 'gnf'] + extra)
    assert e.value.code == 2
    if extra[0] == '--model':
        err = capsys.readouterr().err
        assert '--model' in err and 'gnf' in err


def test_guided_functions_import_without_a_device():
    import inspect
    from geobi_gnn_amd import filters
    assert not torch.cuda.is_initialized()
    sig = inspect.signature(filters.guided_normals).parameters
    assert [(k, sig[k].default) for k in sig] == \
        [('points', inspect.Parameter.empty), ('faces', inspect.Parameter.empty), ('normal_iters', 20), ('sigma_r', 0.35),
         ('sigma_s', 1.0), ('incidence', None), ('return_selection', False)]
    assert inspect.signature(filters.guided_denoise).parameters.keys() == \
        inspect.signature(filters.bilateral_denoise).parameters.keys()
    assert [p.default for p in inspect.signature(filters.guided_denoise).parameters.values()] == \
        [p.default for p in inspect.signature(filters.bilateral_denoise).parameters.values()]
    assert filters.GNF_COST_BUDGET >= 200 ** 3 * 20                             # the 200-fan at the default sweeps
    for bad in (dict(sigma_r=0), dict(sigma_s=0), dict(normal_iters=-1), dict(normal_iters=1.5)):
        with pytest.raises(ValueError):                       # refused before any device is looked for
            filters.guided_normals(np.zeros((3, 3), np.float32), np.array([[0, 1, 2]]), **bad)
