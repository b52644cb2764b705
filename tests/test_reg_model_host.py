"""tests/reg_model.py -- the fp64 statement tests/test_gpu_reg.py compares the kernels with -- against the reference's own
laplacian_loss (oracle.ref_model), a hand-computed edge term, and the CPU paths of the package; the two training flags.
No GPU."""
import argparse

import numpy as np
import pytest
import torch

import reg_model as M
from helpers import load_fixture


def _fixture():
    fx = load_fixture('dualgnn_n4.npz')
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    ei = t(fx['v_edge_index']).long()
    return t(fx['out_verts']).double(), t(fx['v_y']).double(), t(fx['v_x'][:, 3:6]).double(), ei


@pytest.mark.parametrize('projected', [False, True])
def test_laplacian_model_is_the_references_and_the_cpu_path(projected):
    """On the vertex graph of the n = 4 fixture (prediction: the recorded network output) the model, the reference's
    laplacian_loss and network.laplacian_loss on CPU tensors agree to fp64 rounding; the fixture's COO carries one self
    loop per vertex, which all three drop."""
    from geobi_gnn_amd import network
    from oracle import ref_model as R
    vp, v, normal, ei = _fixture()
    assert int((ei[0] == ei[1]).sum()) == vp.shape[0]
    keep = ei[0] != ei[1]
    key = ei[0][keep] * vp.shape[0] + ei[1][keep]
    order = torch.argsort(key)
    row, col = ei[0][keep][order], ei[1][keep][order]
    assert torch.equal(key[order], torch.unique(key))                     # coalesced
    assert set(zip(row.tolist(), col.tolist())) == set(zip(col.tolist(), row.tolist()))          # symmetric
    n = normal if projected else None
    want = float(R.laplacian_loss(vp, v, ei, n))
    got = float(M.laplacian_term(vp, v, row, col, n))
    cpu = float(network.laplacian_loss(vp, v, ei, n))
    assert want > 1e-4
    assert abs(got - want) <= 1e-12 * want and abs(cpu - want) <= 1e-12 * want
    # the weighted form with 1 / V everywhere is the mean
    w = torch.full((vp.shape[0],), 1.0 / vp.shape[0], dtype=torch.float64)
    assert abs(float(M.laplacian_term(vp, v, row, col, n, w)) - want) <= 1e-12 * want


def test_entries_are_the_fixtures_graph():
    """reg_model.entries from the fixture's faces = the fixture's loop-free COO: the tests' graphs are the dataset's."""
    fx = load_fixture('dualgnn_n4.npz')
    ei = torch.from_numpy(fx['v_edge_index']).long()
    keep = ei[0] != ei[1]
    row, col = M.entries(fx['fv_indices'], fx['v_x'].shape[0])
    assert sorted(zip(row.tolist(), col.tolist())) == sorted(zip(ei[0][keep].tolist(), ei[1][keep].tolist()))
    full = M.edge_index(fx['fv_indices'], fx['v_x'].shape[0])
    assert full.shape == ei.shape


def test_edge_term_on_one_triangle_by_hand():
    """Target: the 3-4-5 triangle; prediction: its right-angle corner moved so that the legs are 6 and 4 and the
    hypotenuse sqrt(52).  Six directed entries: mean of (6 - 3)^2, (4 - 4)^2, (sqrt(52) - 5)^2, each twice."""
    from geobi_gnn_amd import network
    v = torch.tensor([[0.0, 0, 0], [3.0, 0, 0], [0.0, 4, 0]], dtype=torch.float64)
    vp = torch.tensor([[0.0, 0, 0], [6.0, 0, 0], [0.0, 4, 0]], dtype=torch.float64)
    faces = np.array([[0, 1, 2]])
    row, col = M.entries(faces, 3)
    assert row.tolist() == [0, 0, 1, 1, 2, 2] and col.tolist() == [1, 2, 0, 2, 0, 1]
    want = (9.0 + 0.0 + (52 ** 0.5 - 5.0) ** 2) / 3.0
    assert abs(float(M.edge_term(vp, v, row, col)) - want) <= 1e-14
    assert abs(float(network.edge_length_loss(vp, v, M.edge_index(faces, 3))) - want) <= 1e-14
    # gradient of corner 1 by hand: entries (1,0), (0,1): 2 * 2 (6 - 3) (1, 0, 0) / 6; (1,2), (2,1): 2 * 2 (l - 5) e / l / 6
    _, _, _, g, _ = M.both(vp, v, row, col)
    ln = 52 ** 0.5
    e = np.array([6.0, -4.0, 0.0]) / ln
    hand = (4 * 3.0 * np.array([1.0, 0, 0]) + 4 * (ln - 5.0) * e) / 6.0
    assert np.abs(g[1].numpy() - hand).max() <= 1e-14
    # no entries: 0, with a gradient of zeros
    none = torch.empty(0, dtype=torch.long)
    assert float(M.edge_term(vp, v, none, none)) == 0.0
    assert float(network.edge_length_loss(vp, v, torch.empty((2, 0), dtype=torch.long))) == 0.0


def test_coincident_predicted_ends_have_a_finite_model_gradient():
    """|vp_i - vp_j| = 0 on one edge: the model's value counts the entry, its gradient is finite (torch's norm has the
    subgradient 0 there) -- what the kernel is held to."""
    vp, v, _, faces = M.sphere_input(2, 0.5)
    row, col = M.entries(faces, vp.shape[0])
    vp = vp.clone()
    vp[int(col[0])] = vp[int(row[0])]
    l_lap, l_edge, g_lap, g_edge, _ = M.both(vp, v, row, col)
    assert np.isfinite(l_edge) and bool(torch.isfinite(g_edge).all()) and bool(torch.isfinite(g_lap).all())
    lg = float((v[int(row[0])].double() - v[int(col[0])].double()).norm())
    # the pair is entries (row0, col0) and its reverse; count both at lg^2
    rev = int(((row == col[0]) & (col == row[0])).nonzero()[0])
    mask = torch.ones(row.numel(), dtype=torch.bool)
    mask[0] = mask[rev] = False
    rest = ((vp[row[mask]].double() - vp[col[mask]].double()).norm(dim=1)
            - (v[row[mask]].double() - v[col[mask]].double()).norm(dim=1)).pow(2).sum()
    assert abs(l_edge - float(rest + 2 * lg * lg) / row.numel()) <= 1e-12 * l_edge


def test_gradient_inputs_leave_out_few_vertices():
    """The inputs of the device test: the share of vertices whose Laplacian gradient is not decided in fp32 (a component
    of d below 1e-5 max |d| at the vertex or a neighbour) stays below the 2 % the device test allows, plain and projected."""
    for n, s in ((2, 0.5), (8, 0.5), (24, 0.3)):
        vp, v, normal, faces = M.sphere_input(n, s)
        row, col = M.entries(faces, vp.shape[0])
        for nrm in (None, normal):
            d = M.lap_difference(vp.double(), v.double(), row, col, None if nrm is None else nrm.double())
            out = int(M.undecided(d, row, col).sum())
            print('n = %d%s: %d of %d vertices left out' % (n, '' if nrm is None else ' projected', out, vp.shape[0]))
            assert out <= 0.02 * vp.shape[0]


def test_batched_regularisers_cpu_branch_equals_the_model_on_a_union():
    """Three meshes of unequal size in one union: the CPU branch of parallel.batched_regularisers = the model with the
    per-mesh weights 1 / (B n_mesh) and 1 / (B E_mesh) = the mean of the three single-mesh terms; a term that is off is None."""
    from geobi_gnn_amd import parallel
    from geobi_gnn_amd.data import Data
    parts = [(p, t, f) for p, t, _, f in (M.sphere_input(n, 0.4, seed=k) for k, n in enumerate((1, 2, 3)))]
    vp, faces, vptr, _ = M.union([(p.double(), torch.from_numpy(f)) for p, _, f in parts])
    v = torch.cat([t.double() for _, t, _ in parts])
    assert vptr.tolist() == [0, 12, 54, 146]
    V = vp.shape[0]
    data = Data(vp.clone(), M.edge_index(faces.numpy(), V), y=v)
    data.mesh_ptr = vptr
    row, col = M.entries(faces.numpy(), V)
    want_lap = float(M.laplacian_term(vp, v, row, col, None, M.mesh_weights(vptr)))
    want_edge = float(M.edge_term(vp, v, row, col, M.edge_weights(row, vptr)))
    singles = []
    for (p, t, f) in parts:
        r, c = M.entries(f, p.shape[0])
        singles.append((float(M.laplacian_term(p.double(), t.double(), r, c)), float(M.edge_term(p.double(), t.double(), r, c))))
    assert abs(want_lap - sum(a for a, _ in singles) / 3) <= 1e-12 * want_lap
    assert abs(want_edge - sum(b for _, b in singles) / 3) <= 1e-12 * want_edge
    p = vp.clone().requires_grad_(True)
    got_lap, got_edge = parallel.batched_regularisers(p, data, True, True)
    assert abs(float(got_lap) - want_lap) <= 1e-12 * want_lap and abs(float(got_edge) - want_edge) <= 1e-12 * want_edge
    (got_lap + got_edge).backward()
    _, _, g_lap, g_edge, _ = M.both(vp, v, row, col, None, M.mesh_weights(vptr), M.edge_weights(row, vptr))
    assert float((p.grad - (g_lap + g_edge)).abs().max()) <= 1e-12 * float((g_lap + g_edge).abs().max())
    only_lap = parallel.batched_regularisers(vp, data, True, False)
    only_edge = parallel.batched_regularisers(vp, data, False, True)
    assert only_lap[1] is None and only_edge[0] is None
    assert float(only_lap[0]) == float(got_lap) and float(only_edge[1]) == float(got_edge)
    assert parallel.batched_regularisers(vp, data, False, False) == (None, None)
    # without mesh_ptr: one mesh, the plain means
    one = Data(vp.clone(), M.edge_index(faces.numpy(), V), y=v)
    a, b = parallel.batched_regularisers(vp, one, True, True)
    assert abs(float(a) - float(M.laplacian_term(vp, v, row, col))) <= 1e-12 * float(a)
    assert abs(float(b) - float(M.edge_term(vp, v, row, col))) <= 1e-12 * float(b)


def test_regulariser_flags_default_to_zero_and_refuse_negatives(capsys):
    from geobi_gnn_amd import train_util, trainer
    parser = train_util.add_training_flags(argparse.ArgumentParser())
    opt = parser.parse_args([])
    assert opt.loss_lap_scale == 0 and opt.loss_edge_scale == 0
    assert trainer.reg_scales(opt) == (0.0, 0.0) and trainer.train_tags(opt) == trainer.TRAIN_TAGS
    assert trainer.reg_scales(argparse.Namespace()) == (0.0, 0.0)                   # options older than the flags
    opt = parser.parse_args(['--loss_lap_scale', '0.5', '--loss_edge_scale', '2'])
    assert (opt.loss_lap_scale, opt.loss_edge_scale) == (0.5, 2.0)
    assert trainer.train_tags(opt) == trainer.TRAIN_TAGS + ('loss_lap', 'loss_edge')
    assert trainer.train_tags(parser.parse_args(['--loss_edge_scale', '1'])) == trainer.TRAIN_TAGS + ('loss_edge',)
    for flag in ('--loss_lap_scale', '--loss_edge_scale'):
        for bad in ('-0.1', 'nan'):
            with pytest.raises(SystemExit):
                parser.parse_args([flag, bad])
            assert flag in capsys.readouterr().err
    full = trainer.add_train_flags(argparse.ArgumentParser()).parse_args(['--data_dir', 'd', '--out_dir', 'o'])
    assert full.loss_lap_scale == 0 and full.loss_edge_scale == 0
