"""CPU: anchors tests/geom_model.py (the fp64 reference of tests/test_gpu_geom.py) to the reference project's own numbers
and proves the conditions the GPU tests rely on: every builder reaches the edge it is meant to reach, and the fp64
reference is finite there.  The fp32 yardsticks are printed, never asserted against: the GPU tests recompute them."""
import numpy as np
import pytest
import torch

import geom_model as M
from helpers import load_fixture, rel_err


def test_model_reproduces_the_reference_fixture():
    """pure_functions.npz holds what the reference project's own functions returned; same bars as test_oracle_golden.py
    (bit-equal in fp32)."""
    fx = load_fixture('pure_functions.npz')
    torch.set_num_threads(1)
    t = lambda k: torch.from_numpy(fx[k])
    a, b = t('a'), t('b')
    an, bn = torch.nn.functional.normalize(a, dim=1), torch.nn.functional.normalize(b, dim=1)
    n = a.shape[0]
    assert M.row_loss(a, b, None, 0, 1.0 / n).item() == pytest.approx(float(fx['loss_v_L1']), rel=1e-6)
    assert M.row_terms(a, b, 0).mean().item() == float(fx['loss_v_L1'])
    assert M.row_terms(a, b, 1).mean().item() == float(fx['loss_v_L2'])
    assert M.row_terms(an, bn, 0).mean().item() == float(fx['loss_n_L1'])
    assert M.row_terms(an, bn, 1).mean().item() == float(fx['loss_n_L2'])
    assert M.row_terms(a, b, 2).mean().item() == float(fx['error_v'])
    assert M.row_terms(an, bn, 3).mean().item() == float(fx['error_n'])
    # the fp64 run of the same expressions agrees with the fp32 fixture to fp32 accuracy
    for kind, key, x, y in ((0, 'loss_v_L1', a, b), (1, 'loss_v_L2', a, b), (2, 'error_v', a, b), (3, 'error_n', an, bn)):
        got = M.row_loss(x.double(), y.double(), None, kind, 1.0 / n).item()
        assert abs(got - float(fx[key])) <= 1e-5 * abs(float(fx[key])), (key, got)
    pts, fv, vf = t('points'), t('faces').long(), t('vf').long()
    xf = torch.randn(fv.shape[0], 9)
    fg = M.face_geom(pts, fv, xf)
    assert torch.equal(fg[:, 9:12], t('face_normal')) and torch.equal(fg[:, :6], xf[:, :6])
    assert torch.equal(fg[:, 6:9], pts[fv].mean(1))
    assert torch.equal(M.update_position2(pts, fv, vf, t('gt_normal'), n_iter=5), t('update2'))
    assert torch.equal(M.update_position2(pts, fv, vf, t('gt_normal'), n_iter=3, depth_direction=t('depth_direction')),
                       t('update2_depth'))


def test_mesh_weights_are_the_trainers():
    from geobi_gnn_amd.data import Data
    from geobi_gnn_amd.parallel import _mesh_weights
    for n, parts in ((1, 3), (2, 3), (31, 32), (50, 3), (1025, 32), (524289, 32), (2500001, 3)):
        ptr = M.unequal_ptr(n, parts)
        sizes = np.diff(ptr)
        assert ptr[0] == 0 and ptr[-1] == n and len(sizes) == min(parts, n) and sizes.min() >= 1
        if n >= 50:
            assert len(set(sizes.tolist())) > 1                    # unequal
        w = M.mesh_weights(ptr)
        assert w.shape[0] == n and abs(float(w.sum()) - 1.0) < 1e-12
        if len(sizes) > 1:
            d = Data(None, None, y=torch.zeros(n, 3))
            d.mesh_ptr = torch.tensor(ptr)
            assert torch.equal(_mesh_weights(d), M.mesh_weights(ptr, torch.float32))
    # the batched loss in torch ops (CPU branch of parallel.batched_losses) is this weighted sum
    a, b = torch.randn(50, 3, dtype=torch.float64), torch.randn(50, 3, dtype=torch.float64)
    want = 0.5 * ((a[:20] - b[:20]).abs().sum(1).mean() + (a[20:] - b[20:]).abs().sum(1).mean())
    assert abs(float(M.row_loss(a, b, M.mesh_weights([0, 20, 50]), 0, 1.0)) - float(want)) < 1e-14


def test_builders_reach_their_edges_and_the_reference_is_finite_there():
    widths = []
    for val in (8, 9, 16, 17, 40, 200):
        pts, faces = M.fan(val, seed=val)
        V = pts.shape[0]
        vf = M.vertex_faces(faces, V)
        widths.append(vf.shape[1])
        cnt = (vf >= 0).sum(1)
        assert int(cnt[0]) == val and int(cnt[-1]) == 0 and bool((cnt[1:-1] == 2).all())   # hub, isolated vertex, rim
        assert int(faces.max()) == V - 2                                                  # no face uses the last vertex
        assert float(M.cross_lengths(pts, faces).min()) > 1e-3
        assert torch.equal(pts, pts.float().double())
        nrm = M.perturbed_normals(pts, faces, seed=val)
        for dd in (None, M.unit_depth(V, seed=val)):
            for it in (0, 1, 2, 5, 60):
                o64 = M.update_position2(pts, faces, vf, nrm, it, dd)
                assert bool(torch.isfinite(o64).all())
                assert torch.equal(o64[-1], pts[-1])                                      # cnt = 0: the vertex stays
                o32 = M.update_position2(pts.float(), faces, vf, nrm.float(), it, None if dd is None else dd.float())
                print('fan %3d  dd %d  n_iter %2d  fp32 oracle vs fp64: %.2e' % (val, dd is not None, it, rel_err(o32, o64)))
    assert widths[:5] == [8, 9, 16, 17, 40] and max(widths) >= 40

    # union: the pointers cut it where the meshes were joined; ids stay inside their mesh
    parts = [M.fan(9, 1), M.sphere(3, 0.2, 2), M.fan(17, 3)]
    pts, faces, vptr, fptr = M.union(parts)
    assert vptr.tolist() == [0, 11, 11 + 92, 11 + 92 + 19] and fptr.tolist() == [0, 9, 9 + 180, 9 + 180 + 17]
    for k in range(3):
        f = faces[fptr[k]:fptr[k + 1]]
        assert int(f.min()) >= int(vptr[k]) and int(f.max()) < int(vptr[k + 1])
        assert torch.equal(pts[vptr[k]:vptr[k + 1]], parts[k][0])

    # degenerate sphere: the cross product is exactly 0 in both precisions, nothing else comes close to it
    pts, faces, deg = M.degenerate_sphere()
    assert deg.numel() == 3 and faces.shape[0] == 180
    f0, f1, f2 = (faces[i].tolist() for i in deg.tolist())
    assert f0[0] == f0[1] != f0[2] and f1[0] == f1[1] == f1[2]
    assert pts[f2].tolist() == [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0]]
    for p in (pts, pts.float()):
        tri = p[faces[deg]]
        cr = torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1)
        assert bool((cr == 0).all())
    ok = torch.ones(faces.shape[0], dtype=torch.bool)
    ok[deg] = False
    assert float(M.cross_lengths(pts, faces)[ok].min()) > 1e-3         # no nearly degenerate face
    touched = torch.zeros(pts.shape[0], dtype=torch.bool)
    touched[faces[deg].reshape(-1)] = True
    g = torch.Generator().manual_seed(0)
    xf = torch.randn(faces.shape[0], 6, generator=g, dtype=torch.float64)
    gout = torch.randn(faces.shape[0], 12, generator=g, dtype=torch.float64)
    grads = {}
    for dt in (torch.float64, torch.float32):
        v = pts.detach().to(dt).clone().requires_grad_(True)
        out = M.face_geom(v, faces, xf.to(dt))
        out.backward(gout.to(dt))
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(v.grad).all())
        assert bool((out[deg, 9:12] == 0).all())                       # zero normals on the degenerate faces
        grads[dt] = v.grad
    g64 = grads[torch.float64]
    assert float(g64[touched].abs().max()) > 1e11 and float(g64[~touched].abs().max()) < 1e3    # g / eps on the touched
    print('degenerate sphere: |grad| max touched %.2e, others %.2e; fp32 model vs fp64: touched %.2e, others %.2e'
          % (float(g64[touched].abs().max()), float(g64[~touched].abs().max()),
             rel_err(grads[torch.float32][touched], g64[touched]), rel_err(grads[torch.float32][~touched], g64[~touched])))
    nrm = M.perturbed_normals(pts, faces, seed=5)
    assert bool(torch.isfinite(nrm).all()) and bool(((nrm.norm(dim=1) - 1).abs() < 1e-6).all())
    vf = M.vertex_faces(faces, pts.shape[0])
    assert bool(torch.isfinite(M.update_position2(pts, faces, vf, nrm, 60)).all())


def test_head_model_is_finite_where_raw_is_exactly_zero():
    """Face head with one node whose raw output is exactly 0 (x row 0, b1 = 0, b2 = 0): output 0 and finite gradients of
    the g / eps scale in the rows that depend on raw."""
    torch.manual_seed(0)
    N, Cin, K = 5, 16, 512
    x = torch.randn(N, Cin, dtype=torch.float64)
    x[2] = 0
    w1 = torch.randn(K, Cin, dtype=torch.float64).requires_grad_(True)
    b1 = torch.zeros(K, dtype=torch.float64, requires_grad=True)
    w2 = torch.randn(3, K, dtype=torch.float64).requires_grad_(True)
    b2 = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    out = M.head(x, w1, b1, w2, b2, 1)
    assert bool((out[2] == 0).all()) and bool(((out.norm(dim=1) - 1).abs()[[0, 1, 3, 4]] < 1e-12).all())
    out.backward(torch.randn(N, 3, dtype=torch.float64))
    for p in (w1, b1, w2, b2):
        assert bool(torch.isfinite(p.grad).all())
    assert float(b2.grad.abs().max()) > 1e10                      # g / eps reaches b2 (and b1 through W2)
    assert float(b1.grad.abs().max()) > 1e10


def test_metric_edge_inputs_and_fp32_yardsticks():
    """Inputs of the kind-3 edges are what they claim to be; prints how far the fp32 run of error_n's expression is from
    fp64 on them (the yardstick the GPU test recomputes)."""
    e = M.exact_unit_rows(1000)
    assert bool(((e * e).sum(1) == 1).all())
    assert float(M.row_terms(e, -e, 3).sub(180).abs().max()) < 1e-3 and float(M.row_terms(e, e, 3).abs().max()) == 0.0
    for name, lo, hi in (('tiny', 1e-4, 1.0), ('ordinary', 0.1, 179.0)):
        n = 100000
        g = torch.Generator().manual_seed(3)
        u = torch.rand(n, generator=g, dtype=torch.float64)
        th = lo * (hi / lo) ** u if name == 'tiny' else lo + (hi - lo) * u
        a, b = M.rows_at_angles(th, seed=4)
        ref = M.row_terms(a.double(), b.double(), 3)
        assert float((ref - th).abs().max()) < 2e-5 * hi + 2e-5            # the rows do sit at these angles (fp32 rows)
        d32 = abs(float(M.row_loss(a, b, None, 3, 1.0 / n)) - float(ref.mean()))
        print('%s angles [%g, %g] deg: mean %.6f deg, fp32 model off by %.2e deg' % (name, lo, hi, float(ref.mean()), d32))
        assert np.isfinite(d32)
