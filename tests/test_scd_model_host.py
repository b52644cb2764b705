"""The sampled surface Chamfer loss without a device: the host model of tests/scd_model.py against torch
fp64 autograd, the folded quad that vertex CD cannot see, and the public surface around the loss -- names, flag, errors,
the header's declarations."""
import argparse
import os
import re
import types

import numpy as np
import pytest
import torch

import sample_model as S
import scd_model as M
from chamfer_model import _cd64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the argument names of DESIGN.md 4m, as the header must declare them
ENTRY_POINTS = {
    'geobi_sample_parts_ws_bytes': ['F', 'P'],
    'geobi_sample_weights_parts': ['points', 'fv', 'fptr', 'P', 'V', 'weight', 'cum', 'exponent', 'ws', 'ws_bytes', 'stream'],
    'geobi_sample_surface_parts': ['points', 'fv', 'cum', 'fptr', 'P', 'V', 'N', 'first', 'seed', 'stream_id', 'draw',
                                   'out_points', 'out_face', 'out_bary', 'stream'],
    'geobi_bary_points': ['points', 'fv', 'face', 'bary', 'V', 'F', 'n', 'out', 'stream'],
    'geobi_bary_keys': ['fv', 'face', 'V', 'F', 'n', 'keys', 'stream'],
    'geobi_bary_points_bwd': ['bary', 'gx', 'segptr', 'members', 'V', 'n', 'gp', 'stream'],
}


# ------------------------------------------------------------------------------------------------ the model
def test_loop_backward_equals_torch_autograd_through_the_gather():
    """A random strip of 40 faces, 500 samples (some with face = -1): the inverse-list loops give the gradient torch fp64
    autograd gives through p[fv[face]], and the forward the same points."""
    p, f = S.strip(40, seed=3)
    rng = np.random.default_rng(1)
    n, V = 500, len(p)
    face = rng.integers(0, len(f), n)
    face[::50] = -1
    bary = rng.dirichlet(np.ones(3), n).astype(np.float32)
    gx = rng.standard_normal((n, 3))
    pt = torch.from_numpy(p.astype(np.float64)).requires_grad_()
    on = torch.from_numpy(face >= 0)
    corners = pt[torch.from_numpy(f.astype(np.int64))[torch.from_numpy(np.where(face >= 0, face, 0))]]
    x = (torch.from_numpy(bary.astype(np.float64))[:, :, None] * corners).sum(1) * on[:, None]
    (x * torch.from_numpy(gx)).sum().backward()
    assert np.abs(M.bary_points64(p, f, face, bary) - x.detach().numpy()).max() <= 1e-15
    got = M.bary_points_bwd_loops(f, face, bary, gx, V)
    err = np.abs(got - pt.grad.numpy()).max() / np.abs(pt.grad.numpy()).max()
    print('loop backward against torch fp64 autograd: rel err %.3g' % err)
    assert err <= 1e-13
    lists = M.inverse_lists(f, face, V)
    assert sum(len(v) for v in lists) == 3 * int((face >= 0).sum()) and all(v == sorted(v) for v in lists)


def test_sample_parts_is_the_single_mesh_sampler_part_by_part():
    """Two strips in one union: every part's rows are sample_model.sample of that mesh alone, the face offset by fptr."""
    (p0, f0), (p1, f1) = S.strip(5, seed=1), S.strip(9, seed=2)
    pts, faces, fptr = np.concatenate([p0, p1]), np.concatenate([f0, f1 + len(p0)]), [0, 5, 14]
    got = M.sample_parts(pts, faces, fptr, 100, seed=3, stream_ids=[7, 2], draw=1)
    for k, (p, f, sid) in enumerate(((p0, f0, 7), (p1, f1, 2))):
        ref = S.sample(p, f, 100, 3, sid, 1)
        r = slice(100 * k, 100 * (k + 1))
        assert np.array_equal(got['face'][r], ref['face'] + fptr[k]) and np.array_equal(got['bary'][r], ref['bary'])
        assert np.array_equal(got['points'][r], ref['points'])
    w, cum, e = M.weights_parts(pts, faces, fptr)
    assert np.array_equal(cum[:5], S.weights(p0, f0)[1]) and np.array_equal(cum[5:], S.weights(p1, f1)[1])
    assert e.tolist() == [S.weights(p0, f0)[2], S.weights(p1, f1)[2]]


def test_folded_quad_is_zero_to_vertex_cd_and_not_to_scd():
    """The folded quad of DESIGN.md 4l (h = 0.3) as prediction and target over one face table: the vertex sets are equal,
    so vertex CD is exactly 0 with a zero gradient; SCD at N = 2 000 is positive and moves all four vertices."""
    p, t, faces = M.folded_pair(0.3)
    cd, g = _cd64(p, t)
    assert cd == 0.0 and not g.any()
    value, gp = M.scd_of_meshes(p, t, faces, [0, 2], 2000, seed=1, stream_ids=[0])
    print('folded quad: CD %g, SCD %.6g, |gradient| per vertex %s' % (cd, value, np.linalg.norm(gp, axis=1)))
    assert value > 1e-3                        # the surfaces are 0.3 apart in the middle
    assert (np.linalg.norm(gp, axis=1) > 0).all()


# ------------------------------------------------------------------------------------------------ the public surface
def test_loss_names_accept_scd_and_the_error_text_keeps_its_order():
    from geobi_gnn_amd import network
    network.check_loss_names('SCD', 'sided')
    assert network.LOSS_V_NAMES[:3] == ('L1', 'L2', 'CD') and network.LOSS_V_NAMES[-1] == 'SCD'
    with pytest.raises(ValueError, match='L1, L2, CD, SCD'):
        network.check_loss_names('nonsense')
    with pytest.raises(ValueError, match='faces'):
        network.loss_v(torch.zeros(4, 3), torch.zeros(4, 3), 'SCD')


def test_loss_samples_flag_parses_and_lands_in_the_params():
    from geobi_gnn_amd import trainer
    parser = trainer.add_train_flags(argparse.ArgumentParser())
    base = ['--data_dir', 'd', '--out_dir', 'o']
    assert parser.parse_args(base).loss_samples == 10000
    opt = parser.parse_args(base + ['--loss_v', 'SCD', '--loss_samples', '500'])
    assert opt.loss_samples == 500 and isinstance(opt.loss_samples, int)
    # what trainer._train writes into the params file: the options of a plain type
    assert {k: v for k, v in vars(opt).items() if isinstance(v, (int, float, str, bool, list, type(None)))}['loss_samples'] == 500
    for bad in ('0', '-1', str(1 << 24), 'many'):
        with pytest.raises(SystemExit):
            parser.parse_args(base + ['--loss_samples', bad])
    assert parser.parse_args(base + ['--loss_samples', str((1 << 24) - 1)]).loss_samples == (1 << 24) - 1
    # the draw of a step: seed, epoch and the dataset indices of the batch; nothing for the other losses
    opt.seed = 31
    assert trainer.loss_sampling(opt, 4, [5, 2]) == dict(n=500, seed=31, draw=4, stream_ids=[5, 2])
    opt.loss_v = 'CD'
    assert trainer.loss_sampling(opt, 4, [5, 2]) is None


def test_batched_losses_refuses_scd_on_cpu_tensors():
    from geobi_gnn_amd.parallel import batched_losses
    p, t, faces = M.folded_pair()
    vp = torch.from_numpy(p).requires_grad_()
    dv = types.SimpleNamespace(y=torch.from_numpy(t))
    df = types.SimpleNamespace(y=torch.zeros(2, 3), fv_indices=torch.from_numpy(faces).long())
    with pytest.raises(ValueError, match='runs on the device only'):
        batched_losses(vp, torch.zeros(2, 3), dv, df, 'SCD', 'L1', sampling=dict(n=10, seed=1, draw=0, stream_ids=[0]))
    lv, _ = batched_losses(vp, torch.zeros(2, 3), dv, df, 'CD', 'L1')          # the CPU branches stay as they are
    assert float(lv.detach()) == 0.0


def test_train_groups_keep_refusing():
    from geobi_gnn_amd.executor import TrainGroups
    with pytest.raises(NotImplementedError, match="'CD' and 'sided'.*not supported by the group path.*'SCD'"):
        TrainGroups(None, None, loss_v='SCD')


def test_header_declares_the_entry_points_with_the_documented_names():
    from geobi_gnn_amd import _lib
    protos = _lib.parse_header()
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    for name, argnames in ENTRY_POINTS.items():
        assert name in protos, name
        assert protos[name][2] == argnames, (name, protos[name][2])
        m = re.search(r'`%s\(([^)]*)\)`' % name, design)
        assert m, 'DESIGN.md 4m does not spell the call of %s' % name
        assert [a.strip() for a in m.group(1).split(',')] == argnames, name
