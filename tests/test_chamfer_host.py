"""The correspondence-free losses without a device: the torch branch of parallel.batched_losses ('CD' / 'sided')
against fp64 statements written in numpy, the errors of the public surface, the header's declarations."""
import types

import numpy as np
import pytest
import torch

from chamfer_model import _argmin64, _cd64, _input, _sided64

TOL = 1e-5                      # the project's bar (tests/test_gpu_kernels.py)


# ------------------------------------------------------------------------------------------------ fp64 statements
def _normals64(pts, faces):
    n = np.cross(pts[faces[:, 1]] - pts[faces[:, 0]], pts[faces[:, 2]] - pts[faces[:, 0]])
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def _bags(parts):
    """[(q, t, faces)] -> prediction tensors and the two Data-like bags of their disjoint union (CPU)."""
    off_v = np.cumsum([0] + [len(q) for q, _, _ in parts])
    off_f = np.cumsum([0] + [len(f) for _, _, f in parts])
    vp = torch.from_numpy(np.concatenate([q for q, _, _ in parts])).requires_grad_()
    y_v = torch.from_numpy(np.concatenate([t for _, t, _ in parts]))
    fv = torch.from_numpy(np.concatenate([f + o for (_, _, f), o in zip(parts, off_v)])).long()
    npred = torch.from_numpy(np.concatenate([_normals64(q.astype(np.float64), f) for q, _, f in parts]).astype(np.float32))
    npred.requires_grad_()
    y_f = torch.from_numpy(np.concatenate([_normals64(t.astype(np.float64), f) for _, t, f in parts]).astype(np.float32))
    dv = types.SimpleNamespace(y=y_v)
    df = types.SimpleNamespace(y=y_f, fv_indices=fv)
    if len(parts) > 1:
        dv.mesh_ptr, df.mesh_ptr = torch.from_numpy(off_v).long(), torch.from_numpy(off_f).long()
    return vp, npred, dv, df


def _statement(parts):
    """fp64: (CD, dCD/dvp, sided, dsided/dnp) of a union batch = the mean over its meshes."""
    B = len(parts)
    cd, sided, g_v, g_n = 0.0, 0.0, [], []
    for q, t, f in parts:
        c, g = _cd64(q, t)
        cd += c / B
        g_v.append(g / B)
        q32, t32 = q.astype(np.float32), t.astype(np.float32)
        fc_p = (q32[f].sum(1) / np.float32(3)).astype(np.float64)
        fc = (t32[f].sum(1) / np.float32(3)).astype(np.float64)
        np_ = _normals64(q.astype(np.float64), f).astype(np.float32)
        n_ = _normals64(t.astype(np.float64), f).astype(np.float32)
        s, g = _sided64(np_, n_, fc_p, fc)
        sided += s / B
        g_n.append(g / B)
    return cd, np.concatenate(g_v), sided, np.concatenate(g_n)


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize('batch', [1, 2])
def test_torch_branch_matches_fp64(batch):
    """parallel.batched_losses on CPU tensors with 'CD' / 'sided': value and gradient against the numpy fp64 statement on
    the n = 8 input, one mesh and a 2-mesh union (the second mesh: the same sphere under another noise scale)."""
    from geobi_gnn_amd.parallel import batched_losses
    parts = [_input(8, 0.5)]
    if batch == 2:
        q, t, f = _input(8, 0.3)
        parts.append((q * np.float32(1.5), t * np.float32(1.5), f))
    vp, npred, dv, df = _bags(parts)
    lv, ln = batched_losses(vp, npred, dv, df, 'CD', 'sided')
    (lv + ln).backward()
    cd, g_v, sided, g_n = _statement(parts)
    print('CD %.9g (fp64 %.9g)  sided %.9g (fp64 %.9g)' % (float(lv.detach()), cd, float(ln.detach()), sided))
    assert abs(float(lv) - cd) <= TOL * abs(cd)
    assert abs(float(ln) - sided) <= TOL * abs(sided)
    assert _rel(vp.grad.numpy(), g_v) <= TOL
    assert _rel(npred.grad.numpy(), g_n) <= TOL


def test_cd_differs_from_l2_on_these_inputs():
    """Only part of the noisy vertices have their own clean vertex as the nearest one: CD is not L2 in disguise."""
    q, t, _ = _input(8, 0.5)
    a, _, _ = _argmin64(q, t)
    own = float((a == np.arange(len(q))).mean())
    print('share of vertices whose nearest target is their own: %.3f' % own)
    assert 0.1 < own < 0.9


def test_unknown_names_are_value_errors_listing_the_valid_ones():
    from geobi_gnn_amd import network
    from geobi_gnn_amd.parallel import batched_losses
    vp, npred, dv, df = _bags([_input(8, 0.5)])
    with pytest.raises(ValueError, match='L1, L2, CD'):
        batched_losses(vp, npred, dv, df, 'nonsense', 'L1')
    with pytest.raises(ValueError, match='L1, L2, sided'):
        batched_losses(vp, npred, dv, df, 'L1', 'nonsense')
    with pytest.raises(ValueError, match='L1, L2, CD'):
        network.loss_v(vp, dv.y, 'nonsense')
    with pytest.raises(ValueError, match='L1, L2, sided'):
        network.loss_n(npred, df.y, 'nonsense')
    with pytest.raises(ValueError, match='centroids'):
        network.loss_n(npred, df.y, 'sided')
    with pytest.raises(NotImplementedError):
        network.loss_v(vp, dv.y, 'EMD')
    with pytest.raises(NotImplementedError):
        network.loss_v(vp, dv.y, 'CD', apply_icp=True)


def test_train_groups_name_the_new_losses_as_unsupported():
    from geobi_gnn_amd.executor import TrainGroups
    for kw in ({'loss_v': 'CD'}, {'loss_n': 'sided'}):
        with pytest.raises(NotImplementedError, match="'CD' and 'sided'"):
            TrainGroups(None, None, **kw)


def test_train_rejects_an_unknown_loss_before_any_work(tmp_path):
    """trainer.train validates the names first: no device, no dataset, no output folder."""
    import argparse
    from geobi_gnn_amd import trainer
    out = tmp_path / 'never'
    opt = trainer.add_train_flags(argparse.ArgumentParser()).parse_args(
        ['--data_dir', str(tmp_path / 'missing'), '--out_dir', str(out), '--loss_v', 'nonsense'])
    with pytest.raises(SystemExit, match='L1, L2, CD'):
        trainer.train(opt, torch.device('cpu'))
    assert not out.exists()


def test_header_declares_the_new_entry_points():
    from geobi_gnn_amd import _lib
    protos = _lib.parse_header()
    for name in ('geobi_nearest_parts_ws_bytes', 'geobi_nearest_parts_slices', 'geobi_nearest_parts',
                 'geobi_chamfer_ws_bytes', 'geobi_chamfer_fwd', 'geobi_chamfer_bwd'):
        assert name in protos, name
    _, argtypes, argnames = protos['geobi_nearest_parts']
    assert argnames == ['q', 't', 'qptr', 'tptr', 'P', 'd2', 'idx', 'ws', 'ws_bytes', 'stream']
