"""The bilateral normal filter on the device (csrc/filter.hip, geobi_gnn_amd/filters.py) against the fp64 model of
tests/bnf_model.py, its determinism and edge rows, filters.bilateral_denoise, and `denoise --method bnf` end to end.

Bar of every comparison with the model, per component: 8 x max(d32, 4 x 2^-24), d32 = max |fp32 model - fp64 model| on the
same input and sweep count, computed here on the CPU -- measured against the model, never against the kernel.  The 8 covers
the device's exp differing from torch's by a few ulp and another summation order in a contractive iteration.
Observed after 5 sweeps, kernel / d32 (every figure is printed by the tests): one face 5.5e-8 / 6.4e-8; icosahedron
3.5e-7 / 5.9e-7; n = 16 sphere 1.2e-7 / 1.6e-7; fans 3-17 0.6-1.9e-7 / 0.8-3.3e-7, fan 33 7.0e-7 / 2.9e-7, fan 64 4.3e-7 /
2.1e-6, fan 65 1.8e-7 / 5.6e-7, fan 200 6.0e-7 / 7.0e-6; degenerate sphere 3.2e-7 / 5.5e-7; translated n = 8 sphere 5.9e-4 /
9.5e-4.  Largest ratio to the bar over all meshes and sweep counts: 0.30 (fan 33).  d32 of the n = 4 and n = 8 spheres
after 20 sweeps: 1.1e-6 and 1.5e-7 (test_bnf_model_host.test_fp32_model_stays_near_the_fp64_model)."""
import os
import re

import numpy as np
import pytest
import torch

import bnf_model as M
import geom_model as G
from filter_cases import (FAN_VALENCES, FANS, SWEEPS, U, _all_degenerate, _angle, _bar, _DeviceMesh, _icosahedron, _one_face,
                          _opposite, _shifted, _sphere8_with_truth)
from train_cases import _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------ meshes and references
MESHES = {'one_face': _one_face, 'icosahedron': _icosahedron, 'sphere16': lambda: G.sphere(16, 0.2, 0),
          'sphere8': lambda: G.sphere(8, 0.3, 1), 'degenerate': lambda: G.degenerate_sphere()[:2],
          'all_degenerate': _all_degenerate, 'opposite': _opposite, 'shifted': _shifted}
MESHES.update(FANS)
_CACHE = {}


def _case(name, sigma_r=0.35):
    """(points f64 with f32 values, faces, fp64 model after 0..5 sweeps, d32 per sweep count): computed once, never changed."""
    key = (name, sigma_r)
    if key not in _CACHE:
        pts, faces = MESHES[name]()
        ref = M.bilateral_normals(pts, faces, normal_iters=max(SWEEPS), sigma_r=sigma_r, history=True)
        f32 = M.bilateral_normals(pts.float(), faces, normal_iters=max(SWEEPS), sigma_r=sigma_r, history=True)
        d32 = [float((a.double() - b).abs().max()) for a, b in zip(f32, ref)]
        _CACHE[key] = (pts, faces, ref, d32)
    return _CACHE[key]


class _Device(_DeviceMesh):
    """The filter's device inputs for one mesh: records, facet graph, the spatial scale."""

    def run(self, n_sweeps, start=None, sigma_r=0.35):
        out = self.filters.filter_records(self.rec_c, self.rec_n if start is None else start, self.graph, self.inv2ss,
                                          sigma_r, n_sweeps)
        torch.cuda.synchronize()
        return out


def _check_mesh(dev, name, sigma_r=0.35):
    from geobi_gnn_amd import filters
    pts, faces, ref, d32 = _case(name, sigma_r)
    d = _Device(pts, faces, dev)
    F = faces.shape[0]
    # the facet graph the kernel walks is the model's, loops aside
    row, col = M.facet_coo(faces.numpy(), pts.shape[0])
    off = row != col
    assert d.graph.E == int(off.sum())
    assert torch.equal(d.graph.col_out.cpu().long(), col[off])
    singles = [d.rec_n]
    for _ in range(max(SWEEPS)):
        singles.append(d.run(1, start=singles[-1], sigma_r=sigma_r))
    worst = 0.0
    for k in SWEEPS:
        got = d.run(k, sigma_r=sigma_r)
        assert tuple(got.shape) == (F, 4) and float(got[:, 3].abs().max()) == 0.0
        assert torch.equal(got, d.run(k, sigma_r=sigma_r)), 'two runs of %d sweeps differ' % k
        assert torch.equal(got, singles[k]), '%d sweeps in one call differ from %d calls of one sweep' % (k, k)
        err = float((got[:, :3].cpu().double() - ref[k]).abs().max())
        worst = max(worst, err / _bar(d32[k]))
        print('%-14s F %5d sweeps %d: |kernel - fp64 model| %.3g, d32 %.3g, bar %.3g' % (name, F, k, err, d32[k], _bar(d32[k])))
        assert err <= _bar(d32[k]), (name, k, err, d32[k])
        if k > 0:
            # every row is a unit vector, or exactly the row it was (kept: cancellation, all-degenerate neighbourhood)
            length = got[:, :3].cpu().double().norm(dim=1)
            kept = (got == singles[k - 1]).all(1).cpu()
            unit = (length - 1).abs() <= 4 * U * np.sqrt(3.0)
            assert bool((unit | kept).all()), (name, k, float((length - 1).abs()[~kept].max()))
    assert torch.equal(d.run(0), d.rec_n)                              # 0 sweeps: the start normals, bit for bit
    # the public function: same bits as the steps above, [F, 3]
    for k in (0, 5):
        pub = filters.bilateral_normals(d.pts, d.fv, normal_iters=k, sigma_r=sigma_r)
        assert tuple(pub.shape) == (F, 3) and pub.is_contiguous() and torch.equal(pub, singles[k][:, :3])
    return worst, d, singles, ref


@pytest.mark.parametrize('name', ['one_face', 'icosahedron', 'sphere16', 'shifted'])
def test_kernel_against_the_fp64_model(dev, name):
    """F = 1 (no edge: a = 0, the face's own normal), the icosahedron, the n = 16 sphere (F = 5120: 320 blocks of 16
    faces, every degree 12 or 13), the n = 8 sphere translated by (1000, -2000, 500) (differences, never the expanded
    form).  0, 1, 2 and 5 sweeps (both ping-pong parities); two runs bit-identical; k sweeps = k single sweeps bit for
    bit; rows unit or kept."""
    worst, d, singles, ref = _check_mesh(dev, name)
    if name == 'one_face':
        assert d.graph.E == 0 and float(d.inv2ss.item()) == 0.0
        assert float((singles[5][:, :3].cpu().double() - ref[0]).abs().max()) <= _bar(0.0)
    if name == 'sphere16':
        # a block holds 16 faces: a face count that is no multiple of it exercises the tail block
        pts, faces, _, _ = _case(name)
        cut = faces[:5120 - 7]
        dc = _Device(pts, cut, dev)
        want = M.bilateral_normals(pts, cut, normal_iters=2)
        d32 = float((M.bilateral_normals(pts.float(), cut, normal_iters=2).double() - want).abs().max())
        got = dc.run(2)
        err = float((got[:, :3].cpu().double() - want).abs().max())
        print('sphere16 without its last 7 faces: %.3g (d32 %.3g)' % (err, d32))
        assert got.shape[0] == 5113 and err <= _bar(d32)


@pytest.mark.parametrize('valence', FAN_VALENCES)
def test_fan_rows(dev, valence):
    """geom_model.fan(v): every face shares the hub, so every row has v - 1 entries (v with the face itself) -- one below,
    at and above the 16-lane group (15, 16, 17 entries), several passes, and a 200-entry hub row."""
    worst, d, _, _ = _check_mesh(dev, 'fan%d' % valence)
    deg = (d.graph.rowptr_out[1:] - d.graph.rowptr_out[:-1]).cpu()
    assert bool((deg == valence - 1).all())


def test_degenerate_faces(dev):
    """Zero-area faces carry weight 0 and a zero start normal and take their neighbours' direction; a mesh of nothing but
    zero-area faces has W = 0 everywhere and keeps its normals."""
    _, d, singles, _ = _check_mesh(dev, 'degenerate')
    bad = G.degenerate_sphere()[2]
    assert float(d.rec_c[bad, 3].abs().max()) == 0.0 and float(d.rec_n[bad].abs().max()) == 0.0
    assert float((singles[1][bad, :3].norm(dim=1) - 1).abs().max()) <= 4 * U * np.sqrt(3.0)
    _, d, singles, _ = _check_mesh(dev, 'all_degenerate')
    assert float(d.rec_c[:, 3].abs().max()) == 0.0
    for s in singles:
        assert float(s.abs().max()) == 0.0


@pytest.mark.parametrize('sigma_r', [1e6, 0.35])
def test_opposite_normals_are_kept(dev, sigma_r):
    _, d, singles, _ = _check_mesh(dev, 'opposite', sigma_r=sigma_r)
    assert torch.equal(d.rec_n[0], -d.rec_n[1])
    for s in singles:
        assert torch.equal(s, d.rec_n)


def test_start_normals_and_records(dev):
    """geobi_bnf_prepare against the model: centroid, area and start normal within 2^-24 of their magnitude."""
    for name in ('sphere8', 'degenerate', 'shifted', 'fan17'):
        pts, faces, _, _ = _case(name)
        d = _Device(pts, faces, dev)
        cen, area, n = M.face_records(pts, faces)
        rc, rn = d.rec_c.cpu().double(), d.rec_n.cpu().double()
        # one rounding of an fp64 value each (half an ulp: at most 2^-24 relative), 1 % for the model's own last digit
        assert float(((rc[:, :3] - cen).abs() / cen.abs().clamp(min=1.0)).max()) <= 1.01 * U
        assert float(((rc[:, 3] - area).abs() / area.clamp(min=1e-30)).max()) <= 1.01 * U
        assert float((rn[:, :3] - n).abs().max()) <= 1.01 * U and float(rn[:, 3].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ bilateral_denoise
def test_bilateral_denoise_against_the_model(dev):
    """n = 8, sigma 0.3, defaults: angle1 and angle2 within 0.01 degrees of the model's normals pushed through the fp64
    vertex update; and the filter denoises (below a quarter of the input's angle, the condition checked on the host)."""
    from geobi_gnn_amd import filters
    noisy, clean, faces = _sphere8_with_truth()
    r = filters.bilateral_denoise(noisy, faces, gt_points=clean, device=dev)
    assert sorted(r) == ['Np', 'V_updated', 'angle1', 'angle2']
    assert tuple(r['Np'].shape) == (faces.shape[0], 3) and tuple(r['V_updated'].shape) == noisy.shape
    p64, f64 = torch.from_numpy(noisy.astype(np.float64)), torch.from_numpy(faces)
    nt = M.face_records(torch.from_numpy(clean.astype(np.float64)), f64)[2]
    np_model = M.bilateral_normals(p64, f64)
    vu = G.update_position2(p64, f64, G.vertex_faces(f64, noisy.shape[0]), np_model, n_iter=20)
    want1, want2 = _angle(np_model, nt), _angle(M.face_records(vu, f64)[2], nt)
    before = _angle(M.face_records(p64, f64)[2], nt)
    print('angle1 %.6f (model %.6f), angle2 %.6f (model %.6f), input %.3f' % (r['angle1'], want1, r['angle2'], want2, before))
    assert abs(r['angle1'] - want1) <= 0.01 and abs(r['angle2'] - want2) <= 0.01
    assert r['angle1'] < before / 4
    assert float((r['V_updated'].cpu().double() - vu).abs().max()) <= 1e-5
    assert torch.equal(r['Np'], filters.bilateral_normals(noisy, faces))
    none = filters.bilateral_denoise(noisy, faces, n_iter=0, device=dev)
    assert none['angle1'] is None and none['angle2'] is None
    assert torch.equal(none['V_updated'], torch.from_numpy(noisy).to(dev))


def test_bilateral_denoise_kinect_moves_along_the_viewing_ray(dev):
    """data_type Kinect_v1: every vertex moves along normalize(points) only.  The part of the displacement d across the
    ray is rounding: each of the 20 sweeps rounds p + step once per coordinate (u |p|, |p| growing by less than a factor
    2) and the fp32 ray is within 2u per coordinate of the exact one: 20 x 2 sqrt(3) u max|p| + 8u |d|.  A displacement
    off the ray would be of the order of |d| itself (1e-2)."""
    from geobi_gnn_amd import filters
    noisy, clean, faces = _sphere8_with_truth()
    r = filters.bilateral_denoise(noisy, faces, data_type='Kinect_v1', gt_points=clean, device=dev)
    free = filters.bilateral_denoise(noisy, faces, gt_points=clean, device=dev)
    assert torch.equal(r['Np'], free['Np'])
    p = torch.from_numpy(noisy.astype(np.float64))
    ray = torch.nn.functional.normalize(p, dim=1)
    d = r['V_updated'].cpu().double() - p
    across = (d - (d * ray).sum(1, keepdim=True) * ray).norm(dim=1)
    bar = 20 * 2 * np.sqrt(3.0) * U * float(p.norm(dim=1).max()) + 8 * U * d.norm(dim=1)
    print('largest displacement %.3g, largest part across the ray %.3g' % (float(d.norm(dim=1).max()), float(across.max())))
    assert float(d.norm(dim=1).max()) > 1e-3 and bool((across <= bar).all())
    assert not torch.equal(r['V_updated'], free['V_updated'])


def test_errors(dev):
    from geobi_gnn_amd import _lib as L
    from geobi_gnn_amd import filters
    noisy, _, faces = _sphere8_with_truth()
    bad = faces.copy()
    bad[3, 1] = noisy.shape[0]
    for fn in (filters.bilateral_normals, filters.bilateral_denoise):
        with pytest.raises(L.GeobiError, match='outside'):
            fn(noisy, bad)
        neg = faces.copy()
        neg[0, 0] = -1
        with pytest.raises(L.GeobiError, match='outside'):
            fn(noisy, neg)
        with pytest.raises(ValueError, match='sigma_r'):
            fn(noisy, faces, sigma_r=0)
        with pytest.raises(ValueError, match='sigma_s'):
            fn(noisy, faces, sigma_s=-1.0)
        with pytest.raises(ValueError, match='normal_iters'):
            fn(noisy, faces, normal_iters=-1)
    with pytest.raises(ValueError, match='n_iter'):
        filters.bilateral_denoise(noisy, faces, n_iter=-1)
    # an int64 id that the conversion to int32 would wrap into range (2^32 + 1 -> 1) is refused as it arrives
    p4 = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], dtype=np.float32)
    wrap = np.array([[0, 1, 2], [1, 2, 2 ** 32 + 1]], dtype=np.int64)
    for fn in (filters.bilateral_normals, filters.bilateral_denoise):
        with pytest.raises(L.GeobiError, match='outside'):
            fn(p4, wrap)
    # the C entry points enforce the size limits and their own arguments
    d = _Device(*_case('icosahedron')[:2], dev)
    out = torch.empty_like(d.rec_n)
    ws = L.workspace(1 << 16, dev)
    args = (L.ptr(d.rec_c), L.ptr(d.rec_n), L.ptr(d.graph.rowptr_out), L.ptr(d.graph.col_out))
    with pytest.raises(L.GeobiError, match='GEOBI_MAX_NODES'):
        L.call('geobi_bnf_filter', *args, 1 << 24, d.graph.E, L.ptr(d.inv2ss), 4.0, 1, L.ptr(out), L.ptr(ws), ws.numel(), L.stream())
    with pytest.raises(L.GeobiError, match='GEOBI_MAX_EDGES'):
        L.call('geobi_bnf_filter', *args, 20, 1 << 28, L.ptr(d.inv2ss), 4.0, 1, L.ptr(out), L.ptr(ws), ws.numel(), L.stream())
    with pytest.raises(L.GeobiError, match='GEOBI_MAX_NODES'):
        L.call('geobi_bnf_prepare', L.ptr(d.pts), L.ptr(d.fv), 1 << 24, 12, L.ptr(d.rec_c), L.ptr(d.rec_n), L.stream())
    with pytest.raises(L.GeobiError, match='n_sweeps'):
        L.call('geobi_bnf_filter', *args, 20, d.graph.E, L.ptr(d.inv2ss), 4.0, -1, L.ptr(out), L.ptr(ws), ws.numel(), L.stream())
    with pytest.raises(L.GeobiError, match='workspace'):
        L.call('geobi_bnf_filter', *args, 20, d.graph.E, L.ptr(d.inv2ss), 4.0, 1, L.ptr(out), L.ptr(ws), 64, L.stream())
    with pytest.raises(L.GeobiError, match='aliases'):
        L.call('geobi_bnf_filter', *args, 20, d.graph.E, L.ptr(d.inv2ss), 4.0, 1, L.ptr(d.rec_n), L.ptr(ws), ws.numel(), L.stream())


# ------------------------------------------------------------------------------------------------ command
def test_denoise_command_with_the_filter(dev, tmp_path):
    from geobi_gnn_amd import filters, meshgen, meshio
    data = str(tmp_path / 'set')
    os.makedirs(os.path.join(data, 'original'))
    os.makedirs(os.path.join(data, 'noisy'))
    for name, seed in (('ball', 1), ('ball2', 2)):
        noisy, clean, faces = meshgen.noisy_icosphere(4, 0.3, seed=seed)
        meshio.write_obj(os.path.join(data, 'original', name + '.obj'), clean, np.asarray(faces, dtype=np.int32))
        meshio.write_obj(os.path.join(data, 'noisy', name + '_n1.obj'), noisy, np.asarray(faces, dtype=np.int32))
    run = _run(['denoise', '--method', 'bnf', '--data_dir', data])
    assert run.returncode == 0, run.stderr[-2000:]
    result = os.path.join(data, 'result')
    assert sorted(os.listdir(result)) == ['ball2_n1-20.obj', 'ball_n1-20.obj']
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith('angle1:')]
    assert len(lines) == 2 and 'angle_mean1' in run.stdout and 'random init' not in run.stdout
    faces_total, weighted = 0, np.zeros(2)
    for name in ('ball', 'ball2'):
        ln, = [x for x in lines if "'%s_n1-20.obj'" % name in x]
        pts, faces = meshio.read_obj(os.path.join(data, 'noisy', name + '_n1.obj'))
        gt, _ = meshio.read_obj(os.path.join(data, 'original', name + '.obj'))
        r = filters.bilateral_denoise(pts, faces, gt_points=gt, device=dev)
        assert ln.startswith('angle1: %9.6f,  angle2: %9.6f,  faces: %6d,' % (r['angle1'], r['angle2'], faces.shape[0])), ln
        got, got_faces = meshio.read_obj(os.path.join(result, name + '_n1-20.obj'))
        assert (got_faces == faces).all()
        assert (got.view(np.uint32) == r['V_updated'].cpu().numpy().view(np.uint32)).all()      # nine digits: bit for bit
        faces_total += faces.shape[0]
        weighted += faces.shape[0] * np.array([r['angle1'], r['angle2']])
    mean = re.search(r'Num_face:\s*(\d+),\s*angle_mean1: ([0-9.]+),\s*angle_mean2: ([0-9.]+)', run.stdout)
    assert mean and int(mean.group(1)) == faces_total
    assert abs(float(mean.group(2)) - weighted[0] / faces_total) <= 2e-6
    assert abs(float(mean.group(3)) - weighted[1] / faces_total) <= 2e-6
    # `eval` pairs the results with their originals as it does for the network's
    run = _run(['eval', '--result_dir', result, '--original_dir', os.path.join(data, 'original')])
    assert run.returncode == 0 and '2 pairs' in run.stdout, run.stderr[-2000:]
    # flags reach the filter: other sweep counts, the file name follows --n_iter
    other = str(tmp_path / 'other')
    run = _run(['denoise', '--method', 'bnf', '--data_dir', data, '--out_dir', other, '--normal_iters', '3', '--sigma_r', '0.5',
                '--sigma_s', '1.5', '--n_iter', '7'])
    assert run.returncode == 0 and sorted(os.listdir(other)) == ['ball2_n1-7.obj', 'ball_n1-7.obj']
    pts, faces = meshio.read_obj(os.path.join(data, 'noisy', 'ball_n1.obj'))
    gt, _ = meshio.read_obj(os.path.join(data, 'original', 'ball.obj'))
    r = filters.bilateral_denoise(pts, faces, normal_iters=3, sigma_r=0.5, sigma_s=1.5, n_iter=7, gt_points=gt, device=dev)
    assert ('angle1: %9.6f,  angle2: %9.6f,' % (r['angle1'], r['angle2'])) in run.stdout
    # --model with the filter is an argument error, before anything runs
    run = _run(['denoise', '--method', 'bnf', '--model', 'net.pt', '--data_dir', data])
    assert run.returncode == 2 and '--model' in run.stderr
    # without --method the command is what it was: the network (random init), NAME-60.obj
    plain = str(tmp_path / 'plain')
    run = _run(['denoise', '--data_dir', data, '--out_dir', plain])
    assert run.returncode == 0, run.stderr[-2000:]
    assert sorted(os.listdir(plain)) == ['ball2_n1-60.obj', 'ball_n1-60.obj'] and 'random init' in run.stdout
