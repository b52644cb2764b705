"""Synthetic mesh noise on the device: geobi_mesh_noise against the fp64 model of tests/noise_model.py, its determinism
and statistics, meshnoise.add_noise, the `noise` command, DualDataset(noise=...) against a file-mode dataset over files
written from the same draws, meshprep.refresh_dual_data, and `train --noise_levels` end to end."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import noise_model as M
from train_cases import _assert_same_sample, _run

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                  # unit roundoff of fp32
# ulp bounds taken for the HIP math API's precise functions: its tables give logf 1, sincosf 1 (sine and cosine each) and
# sqrtf 1; 2 is taken for the two transcendentals so that the bar does not hang on the last digit of a table
K_LOG, K_SINCOS, K_SQRT, K_DIV = 2, 2, 1, 1
BIG_SEED = (0x9e3779b9 << 32) | 0x7f4a7c15          # non-zero high word


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


def _kernel(points, vnormal, sigma, kind, direction, fraction, seed, stream_id, draw, out=None):
    from geobi_gnn_amd import _lib as L
    out = torch.empty_like(points) if out is None else out
    L.call('geobi_mesh_noise', L.ptr(points), L.ptr(vnormal), points.shape[0], float(sigma), kind, direction,
           float(fraction), seed, stream_id, draw, L.ptr(out), L.stream())
    torch.cuda.synchronize()
    return out


def _inputs(V, seed, dev):
    rng = np.random.default_rng(seed)
    pts = (rng.standard_normal((V, 3)) * 2.0).astype(np.float32)
    n = rng.standard_normal((V, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    return pts, n, torch.from_numpy(pts).to(dev), torch.from_numpy(n).to(dev)


def _bars(points, vnormal, sigma, direction, n4, disp):
    """Per-coordinate bound on |(out - points) - model| for a moved vertex, u = 2^-24, every factor below (1 + O(u)) folded
    into a closing 1.01.

    One normal g = r c with r = sqrt(-2 ln u0), c = cos or sin of t = 2 pi u1:
      t      fl(2 pi) is within u of 2 pi relatively, the product rounds once: |dt| <= 2 pi 2u
      c      |dc| <= |dt| + K_SINCOS ulp, an ulp of a value of magnitude <= 1 being <= 2u: dc = 4 pi u + 2 K_SINCOS u
      r      logf: K_LOG ulp = 2 K_LOG u relative; -2 x is exact; the square root halves that and adds K_SQRT ulp:
             rho_r = (K_LOG + 2 K_SQRT) u relative
      g      one more rounding: |dg| <= r (|c| (rho_r + u) + dc)
    direction 0:  d_c = fl(fl(sigma g0) n_c), two roundings: |dd_c| <= sigma |n_c| (dg0 + 2u |g0|)
    direction 1:  len = sqrtf(g1^2 + g2^2 + g3^2): the inputs move it by at most |dg|_2, five roundings under the root
                  count half, the root K_SQRT ulp: rho_len = |dg|_2 / len + (2.5 + 2 K_SQRT) u relative;
                  q = fl(fl(sigma g0) / len): |dq| <= sigma (dg0 + u |g0|) / len + |q| (rho_len + 2 K_DIV u);
                  d_c = fl(q g_c): |dd_c| <= |dq| |g_c| + |q| dg_c + u |d_c|
    both:         out_c = fl(p_c + d_c) rounds once more: u (|p_c| + |d_c|)."""
    g, r, cs = n4['g'], n4['r'], n4['cs']
    dc = (4 * np.pi + 2 * K_SINCOS) * U
    rho_r = (K_LOG + 2 * K_SQRT) * U
    rr = np.stack([r[:, 0], r[:, 0], r[:, 1], r[:, 1]], 1)
    dg = rr * (np.abs(cs) * (rho_r + U) + dc)
    p = np.abs(points.astype(np.float64))
    if direction == 0:
        bar = sigma * np.abs(vnormal.astype(np.float64)) * (dg[:, :1] + 2 * U * np.abs(g[:, :1]))
    else:
        length = np.sqrt((g[:, 1:] ** 2).sum(1, keepdims=True))
        q = sigma * np.abs(g[:, :1]) / length
        rho_len = np.sqrt((dg[:, 1:] ** 2).sum(1, keepdims=True)) / length + (2.5 + 2 * K_SQRT) * U
        dq = sigma * (dg[:, :1] + U * np.abs(g[:, :1])) / length + q * (rho_len + 2 * K_DIV * U)
        bar = dq * np.abs(g[:, 1:]) + q * dg[:, 1:] + U * np.abs(disp)
    return 1.01 * (bar + U * (p + np.abs(disp)))


def _check_against_model(dev, V, kind, direction, seed, stream_id, draw, alias, fraction=0.3, sigma=0.05):
    pts, n, pts_d, n_d = _inputs(V, 100 + V, dev)
    rows = np.arange(V)
    want, moved, n4 = M.displacement(rows, n, sigma, kind, direction, fraction, seed, stream_id, draw)
    if kind == 1:     # the comparison u < fraction must not hang on a rounding of the test's own
        assert np.abs(M.coin(rows, seed, stream_id, draw) - float(np.float32(fraction))).min() > 2.0 ** -20
    before = pts_d.clone()
    out = _kernel(pts_d, n_d if direction == 0 else None, sigma, kind, direction, fraction, seed, stream_id, draw,
                  out=pts_d if alias else None)
    if alias:
        assert out.data_ptr() == pts_d.data_ptr()
    else:
        assert torch.equal(pts_d, before)
    got = out.cpu().numpy().astype(np.float64) - pts.astype(np.float64)
    got_moved = (out.cpu().numpy() != pts).any(1)
    # a moved vertex whose displacement rounds away entirely would read as unmoved: none at these sizes
    assert (got_moved == moved).all(), (int(got_moved.sum()), int(moved.sum()))
    assert (got[~moved] == 0).all()
    bar = _bars(pts, n, float(np.float32(sigma)), direction, n4, want)
    err = np.abs(got - want)[moved]
    ratio = float((err / bar[moved]).max()) if moved.any() else 0.0
    print('V %6d kind %d direction %d seed %x stream %d draw %d alias %d: worst error / bar = %.3f (%d moved)'
          % (V, kind, direction, seed, stream_id, draw, alias, ratio, int(moved.sum())))
    assert (err <= bar[moved]).all(), ratio


@pytest.mark.parametrize('direction', [0, 1])
@pytest.mark.parametrize('kind', [0, 1])
@pytest.mark.parametrize('V', [1, 63, 10242])
def test_kernel_against_the_fp64_model(dev, V, kind, direction):
    """Every coordinate of out - points against the fp64 model fed the same Philox words, bar as derived in `_bars` from
    the rounding steps and the ulp bounds of logf, sincosf and sqrtf.  A wrong word moves a vertex by O(sigma), five
    orders above the bar, so this pins the integer path as well; for the impulsive kind the moved set is the model's.
    Two (stream_id, draw) pairs, a 64-bit seed with a non-zero high word, out aliasing points."""
    # V = 1 with fraction 0.3 may leave the one vertex unmoved: fraction 0.9 there so that the kind is exercised too
    fraction = 0.9 if V == 1 else 0.3
    _check_against_model(dev, V, kind, direction, 1, 0, 0, alias=False, fraction=fraction)
    _check_against_model(dev, V, kind, direction, BIG_SEED, 0xdeadbeef, 7, alias=True, fraction=fraction)


def test_impulsive_margin_of_the_model():
    """fraction = 0.3, seeds 1-3, V = 10 242: no vertex's coin is within 2^-20 of the fraction (on the model alone)."""
    from geobi_gnn_amd import meshnoise
    for seed in (1, 2, 3):
        u = M.coin(np.arange(10242), seed, meshnoise.stream_of('ball'), 1)
        assert np.abs(u - float(np.float32(0.3))).min() > 2.0 ** -20
        assert abs((u < 0.3).mean() - 0.3) <= 5 * np.sqrt(0.21 / 10242)


def test_determinism_and_what_the_counter_is(dev):
    V = 10242
    pts, n, pts_d, n_d = _inputs(V, 9, dev)
    args = (0.05, 0, 0, 0.3)
    a = _kernel(pts_d, n_d, *args, 5, 11, 2)
    assert torch.equal(a, _kernel(pts_d, n_d, *args, 5, 11, 2))
    # the counter is the ROW INDEX OF THE CALL: the first half agrees with the whole (same indices), the second half
    # called on its own starts again at row 0 and differs
    h = V // 2
    first = _kernel(pts_d[:h].contiguous(), n_d[:h].contiguous(), *args, 5, 11, 2)
    second = _kernel(pts_d[h:].contiguous(), n_d[h:].contiguous(), *args, 5, 11, 2)
    assert torch.equal(first, a[:h])
    assert not torch.equal(second, a[h:])
    want, _, n4 = M.displacement(np.arange(V - h), n[h:], 0.05, 0, 0, 0.3, 5, 11, 2)
    got = second.cpu().numpy().astype(np.float64) - pts[h:].astype(np.float64)
    assert (np.abs(got - want) <= _bars(pts[h:], n[h:], float(np.float32(0.05)), 0, n4, want)).all()      # rows 0 .. V - h
    for other in ((5, 11, 3), (5, 12, 2), (6, 11, 2), (5 | (1 << 32), 11, 2)):
        b = _kernel(pts_d, n_d, *args, *other)
        changed = float((b != a).any(1).float().mean())
        print('seed, stream, draw', other, 'changes %.4f of the vertices' % changed)
        assert changed > 0.99


def _sphere(freq):
    from geobi_gnn_amd import meshgen
    pts, faces = meshgen.icosphere(freq)
    return np.asarray(pts, dtype=np.float32), np.asarray(faces, dtype=np.int32)


def test_statistics(dev):
    """Frequency-32 icosphere (V = 10 242), seeds 1-3, level 0.2.  Normal direction: g = (out - points).n / sigma has
    |mean| <= 5 / sqrt(V) and |var - 1| <= 5 sqrt(2 / V) (five standard errors of the mean and of the variance of V
    standard normals); the tangential part is rounding: |n.n - 1| <= 8u for a normalised fp32 vector and u(|p| + |d|)
    per coordinate from the closing sum give 16u |d| + 4u (|p| + |d|).  Random direction: a coordinate of the displacement is
    sigma g e_c with e uniform on the sphere, E = sigma^2 / 3 and var of its square (3 / 5 - 1 / 9) sigma^4, so the
    coordinate variance over sigma^2 / 3 is within 5 sqrt(4.4 / V) of 1.  The model is checked first on the same seeds."""
    from geobi_gnn_amd import meshnoise
    pts, faces = _sphere(32)
    V = pts.shape[0]
    assert V == 10242
    geom = meshnoise.MeshGeometry(pts, faces, dev)
    sigma = geom.sigma(0.2)
    n = geom.vnormal.cpu().numpy().astype(np.float64)
    p = pts.astype(np.float64)
    bar_mean, bar_var, bar_coord = 5 / np.sqrt(V), 5 * np.sqrt(2.0 / V), 5 * np.sqrt(4.4 / V)
    for seed in (1, 2, 3):
        g_model = M.normals4(np.arange(V), seed, 3, 1)['g']
        assert abs(g_model[:, 0].mean()) <= bar_mean and abs(g_model[:, 0].var() - 1) <= bar_var
        d = geom.draw(0.2, seed=seed, stream_id=3, draw=1).cpu().numpy().astype(np.float64) - p
        g = (d * n).sum(1) / sigma
        print('seed %d normal: |mean| %.4f (bar %.4f), |var - 1| %.4f (bar %.4f)'
              % (seed, abs(g.mean()), bar_mean, abs(g.var() - 1), bar_var))
        assert abs(g.mean()) <= bar_mean and abs(g.var() - 1) <= bar_var
        tangent = np.linalg.norm(d - (d * n).sum(1, keepdims=True) * n, axis=1)
        dn, pn = np.linalg.norm(d, axis=1), np.linalg.norm(p, axis=1)
        assert (tangent <= 16 * U * dn + 4 * U * (pn + dn)).all()

        want, _, _ = M.displacement(np.arange(V), None, sigma, 0, 1, 0.3, seed, 3, 1)
        assert (np.abs(want.var(0) / (sigma ** 2 / 3) - 1) <= bar_coord).all()
        d = geom.draw(0.2, direction='random', seed=seed, stream_id=3, draw=1).cpu().numpy().astype(np.float64) - p
        rel = np.abs(d.var(0) / (sigma ** 2 / 3) - 1)
        print('seed %d random: coordinate variances off by %s (bar %.4f)' % (seed, np.round(rel, 4), bar_coord))
        assert (rel <= bar_coord).all()


def test_add_noise(dev):
    from geobi_gnn_amd import _lib as L
    from geobi_gnn_amd import meshnoise, meshprep
    pts, faces = _sphere(8)
    pts[pts == 0] = -0.0                             # a sum with +0.0 would flip these
    assert np.signbit(pts[pts == 0]).sum() > 0
    V = pts.shape[0]
    fv = torch.from_numpy(faces).to(dev)
    pts_d = torch.from_numpy(pts).to(dev)
    rowptr, lst = meshprep.vertex_faces(fv, V)
    g_v = meshprep.ring_graph(0, fv, rowptr, lst, V)
    mean_edge = np.float32(meshprep.mean_edge_length(pts_d, g_v).tolist()[0])
    vn = meshprep.mesh_normals(pts_d, fv, rowptr, lst)[2]
    geom = meshnoise.MeshGeometry(pts, faces, dev)
    assert np.float32(geom.mean_edge) == mean_edge
    sigma = np.float32(np.float32(0.25) * mean_edge)
    assert np.float32(geom.sigma(0.25)) == sigma
    got = meshnoise.add_noise(pts, faces, 0.25, seed=4, stream_id=8, draw=2)
    assert got.is_cuda and tuple(got.shape) == (V, 3) and got.dtype == torch.float32
    assert torch.equal(got, _kernel(pts_d, vn, float(sigma), 0, 0, 0.3, 4, 8, 2))
    want, _, n4 = M.displacement(np.arange(V), vn.cpu().numpy(), sigma, 0, 0, 0.3, 4, 8, 2)
    err = np.abs(got.cpu().numpy().astype(np.float64) - pts.astype(np.float64) - want)
    assert (err <= _bars(pts, vn.cpu().numpy(), float(sigma), 0, n4, want)).all()
    for kw in ({}, {'direction': 'random'}, {'kind': 'impulsive'}):
        assert torch.equal(meshnoise.add_noise(pts, faces, 0.0, seed=4, **kw), pts_d), kw      # bit-unchanged, -0.0 included
    assert np.signbit(meshnoise.add_noise(pts, faces, 0.0, seed=4).cpu().numpy()).sum() == np.signbit(pts).sum()
    for kw in ({'level': -0.1}, {'fraction': 1.1}, {'fraction': -0.1}, {'kind': 'salt'}, {'direction': 'up'}):
        args = dict(level=0.1, seed=1)
        args.update(kw)
        with pytest.raises(ValueError):
            meshnoise.add_noise(pts, faces, **args)
    bad = faces.copy()
    bad[0, 0] = V
    with pytest.raises(L.GeobiError):
        meshnoise.add_noise(pts, bad, 0.1, seed=1)
    # an int64 id that the conversion to int32 would wrap into range (2^32 + 1 -> 1) is refused as it arrives
    p4 = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], dtype=np.float32)
    wrap = np.array([[0, 1, 2], [1, 2, 2 ** 32 + 1]], dtype=np.int64)
    with pytest.raises(L.GeobiError, match='outside'):
        meshnoise.add_noise(p4, wrap, 0.1, seed=1)


# ------------------------------------------------------------------------------------------------ command
def _write_originals(folder, spheres):
    from geobi_gnn_amd import meshio
    os.makedirs(folder, exist_ok=True)
    for name, freq in spheres:
        pts, faces = _sphere(freq)
        meshio.write_obj(os.path.join(folder, name + '.obj'), pts, faces)


def test_noise_command_end_to_end(dev, tmp_path):
    from geobi_gnn_amd import meshio, meshnoise
    data = str(tmp_path / 'set')
    _write_originals(os.path.join(data, 'original'), (('ball', 12), ('ball2', 16)))
    run = _run(['noise', '--data_dir', data, '--levels', '0.1,0.3', '--seed', '5'])
    assert run.returncode == 0, run.stderr[-2000:]
    names = ['ball2_n1.obj', 'ball2_n2.obj', 'ball_n1.obj', 'ball_n2.obj']
    assert sorted(os.listdir(os.path.join(data, 'noisy'))) == names
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith('V:')]
    assert len(lines) == 4 and all('L:' in ln and 'sigma:' in ln and 'F:' in ln for ln in lines)
    for name in ('ball', 'ball2'):
        pts, faces = meshio.read_obj(os.path.join(data, 'original', name + '.obj'))
        geom = meshnoise.MeshGeometry(pts, faces, dev)
        for k, level in ((1, 0.1), (2, 0.3)):
            got, got_faces = meshio.read_obj(os.path.join(data, 'noisy', '%s_n%d.obj' % (name, k)))
            assert (got_faces == faces).all()
            want = meshnoise.add_noise(pts, faces, level, seed=5, stream_id=meshnoise.stream_of(name), draw=k)
            assert (got.view(np.uint32) == want.cpu().numpy().view(np.uint32)).all()          # bit for bit
            # RMS displacement over L against the level: the mean of V squared standard normals has standard error
            # sqrt(2 / V); the root halves it, five of them and the float32 rounding of sigma (1e-6) give the bar
            V = pts.shape[0]
            rms = np.sqrt(((got.astype(np.float64) - pts.astype(np.float64)) ** 2).sum(1).mean()) / geom.mean_edge
            print('%s level %.1f: RMS displacement / L = %.4f' % (name, level, rms))
            assert abs(rms / level - 1) <= 2.5 * np.sqrt(2.0 / V) + 1e-6
    first = {f: open(os.path.join(data, 'noisy', f), 'rb').read() for f in names}
    again = str(tmp_path / 'again')
    run = _run(['noise', '--data_dir', data, '--levels', '0.1,0.3', '--seed', '5', '--out_dir', again])
    assert run.returncode == 0, run.stderr[-2000:]
    assert {f: open(os.path.join(again, f), 'rb').read() for f in names} == first
    # a file without faces is reported and skipped, the status says so; nothing found is status 1 too
    with open(os.path.join(data, 'original', 'cloud.obj'), 'w') as fh:
        fh.write('v 0 0 0\nv 1 0 0\nv 0 1 0\n')
    run = _run(['noise', '--data_dir', data, '--out_dir', str(tmp_path / 'third')])
    assert run.returncode == 1 and 'skipped:' in run.stderr and 'cloud.obj' in run.stderr
    assert len(os.listdir(str(tmp_path / 'third'))) == 6
    os.makedirs(str(tmp_path / 'empty' / 'original'))
    assert _run(['noise', '--data_dir', str(tmp_path / 'empty')]).returncode == 1


# ------------------------------------------------------------------------------------------------ dataset
def _file_mode_twin(synthetic, root, tmp, tag, **kw):
    """A file-mode DualDataset(cache=False) over the files `synthetic` writes from its current draw."""
    from geobi_gnn_amd.dataset import DualDataset
    twin = os.path.join(tmp, tag)
    shutil.copytree(os.path.join(root, 'train', 'original'), os.path.join(twin, 'train', 'original'))
    synthetic.write_noisy(os.path.join(twin, 'train', 'noisy'))
    return DualDataset(twin, 'train', cache=False, **kw)


@pytest.mark.parametrize('data_type', ['Synthetic', 'Kinect_v1'])
def test_dataset_unsplit_equals_file_mode(dev, tmp_path, data_type):
    from geobi_gnn_amd import meshnoise
    from geobi_gnn_amd.dataset import DualDataset
    root = str(tmp_path / 'clean')
    _write_originals(os.path.join(root, 'train', 'original'), (('ball', 6), ('ball2', 8)))
    noise = {'levels': (0.1, 0.3), 'seed': 7}
    kw = dict(data_type=data_type, device=dev)
    ds = DualDataset(root, 'train', noise=noise, **kw)
    assert ds.names == ['ball_n1', 'ball_n2', 'ball2_n1', 'ball2_n2'] and ds.skipped == 0 and len(ds.pairs) == 4
    assert not os.path.exists(os.path.join(root, 'train', 'processed_data'))
    twin = _file_mode_twin(ds, root, str(tmp_path), 'draw0', **kw)
    assert twin.names == ds.names
    for i in range(len(ds)):
        _assert_same_sample(ds[i], twin[i])
    # draw 0 of (NAME, k) is add_noise(..., stream_of(NAME), draw = k)
    pts, faces = _sphere(6)
    want = meshnoise.add_noise(pts, faces, 0.3, seed=7, stream_id=meshnoise.stream_of('ball'), draw=2)
    assert torch.equal(ds.noisy_points(ds._entries[1]), want)

    kept = [(s[0], s[1], s[0].graph(), s[1].graph(), s[0].graph().pos_in, s[1].fv_indices, s[1].fv_indices._geobi_fv)
            for s in ds.samples]
    x_before = [s[0].x.clone() for s in ds.samples]
    ds.resample(2)
    for i, (dv, df, gv, gf, pos_in, fv, mark) in enumerate(kept):
        assert ds[i][0] is dv and ds[i][1] is df
        assert ds[i][0].graph() is gv and ds[i][1].graph() is gf and gv.pos_in is pos_in          # nothing rebuilt
        assert ds[i][1].fv_indices is fv and fv._geobi_fv is mark
        assert not torch.equal(ds[i][0].x, x_before[i])
    want = meshnoise.add_noise(pts, faces, 0.3, seed=7, stream_id=meshnoise.stream_of('ball'), draw=2 + 2 * 2)
    assert torch.equal(ds.noisy_points(ds._entries[1]), want)
    twin2 = _file_mode_twin(ds, root, str(tmp_path), 'draw2', **kw)
    assert twin2.names == ds.names
    for i in range(len(ds)):
        _assert_same_sample(ds[i], twin2[i])
    ds.resample(0)
    for i in range(len(ds)):
        _assert_same_sample(ds[i], twin[i])
    with pytest.raises(ValueError):
        twin.resample(1)


def test_refresh_equals_a_fresh_build(dev):
    """Every field of both Data objects after meshprep.refresh_dual_data equals a fresh build_dual_data on the new points,
    meta (centroid, scale, vf table, incidence) included, and the graphs are the objects they were."""
    from geobi_gnn_amd import meshnoise, meshprep
    pts, faces = _sphere(10)
    for data_type in ('Synthetic', 'Kinect_v2'):
        first = meshnoise.add_noise(pts, faces, 0.2, seed=1, draw=1)
        second = meshnoise.add_noise(pts, faces, 0.3, seed=1, draw=2)
        dv, df = meshprep.build_dual_data(first, faces, points_gt=pts, data_type=data_type, device=dev)
        gv, gf = dv.graph(), df.graph()
        meshprep.refresh_dual_data(dv, df, second, pts, data_type)
        wv, wf = meshprep.build_dual_data(second, faces, points_gt=pts, data_type=data_type, device=dev)
        assert dv.graph() is gv and df.graph() is gf
        _assert_same_sample((dv, df), (wv, wf))
        assert torch.equal(df.y, wf.y)
        assert torch.equal(dv.meta['centroid'], wv.meta['centroid']) and dv.meta['scale'] == wv.meta['scale']
        assert torch.equal(dv.meta['vf_indices'], wv.meta['vf_indices'])
        assert sorted(dv.keys()) == sorted(wv.keys()) and sorted(df.keys()) == sorted(wf.keys())
        # without meta (as the dataset keeps its samples) the scale never leaves the device: same bits
        dv.meta = None
        meshprep.refresh_dual_data(dv, df, first, pts, data_type)
        _assert_same_sample((dv, df), meshprep.build_dual_data(first, faces, points_gt=pts, data_type=data_type, device=dev))


def _two_component_clean():
    """The two-component mesh of the split test of tests/test_gpu_train.py, clean: a frequency-16 icosphere and, far away,
    a frequency-1 icosphere scaled by 0.2 at x = 3."""
    from geobi_gnn_amd import meshgen
    big, faces = meshgen.icosphere(16)
    small, small_faces = meshgen.icosphere(1)
    small = (np.asarray(small, dtype=np.float64) * 0.2 + np.array([3.0, 0.0, 0.0])).astype(np.float32)
    big = np.asarray(big, dtype=np.float32)
    all_faces = np.concatenate([np.asarray(faces), np.asarray(small_faces) + big.shape[0]]).astype(np.int32)
    return np.concatenate([big, small]).astype(np.float32), all_faces


def test_dataset_split_equals_file_mode(dev, tmp_path):
    from geobi_gnn_amd import meshio
    from geobi_gnn_amd.dataset import DualDataset
    root = str(tmp_path / 'clean')
    os.makedirs(os.path.join(root, 'train', 'original'))
    pts, faces = _two_component_clean()
    meshio.write_obj(os.path.join(root, 'train', 'original', 'pair.obj'), pts, faces)
    kw = dict(submesh_size=2000, filter_patch_count=100, device=dev)
    ds = DualDataset(root, 'train', noise={'levels': (0.2,), 'seed': 3}, **kw)
    assert len(ds) >= 3 and all(n.startswith('pair_n1-sub2000-') for n in ds.names)
    twin = _file_mode_twin(ds, root, str(tmp_path), 'draw0', **kw)
    assert twin.names == ds.names
    for i in range(len(ds)):
        _assert_same_sample(ds[i], twin[i])
    ds.resample(2)
    twin2 = _file_mode_twin(ds, root, str(tmp_path), 'draw2', **kw)
    assert twin2.names == ds.names and len(ds) >= 3
    for i in range(len(ds)):
        _assert_same_sample(ds[i], twin2[i])
    assert ds.names != twin.names or not torch.equal(ds[0][0].x, twin[0][0].x)          # it is another draw


# ------------------------------------------------------------------------------------------------ training
def _train(data, out, extra):
    return _run(['train', '--data_dir', data, '--out_dir', out, '--max_epoch', '2', '--batch_size', '2', '--seed', '31']
                + list(extra))


def _model_bytes(out):
    with open(os.path.join(out, 'GeoBi-GNN_Synthetic_model.pth'), 'rb') as fh:
        return fh.read()


def _epoch_seconds(out):
    log = open(os.path.join(out, 'training_info.txt')).read()
    return [json.loads(ln)['epoch_s'] for ln in log.splitlines() if ln.startswith('{"epoch"') and 'epoch_s' in ln]


def test_train_from_clean_meshes(dev, tmp_path):
    """train/ and test/ hold original/ only.  Child processes one after the other, each only after the one before it
    returned 0."""
    data = str(tmp_path / 'Clean')
    _write_originals(os.path.join(data, 'train', 'original'), (('s1', 8), ('s2', 6), ('s3', 7)))
    _write_originals(os.path.join(data, 'test', 'original'), (('t1', 8),))
    renoise = ['--noise_levels', '0.1,0.2', '--renoise_every', '1']
    out1 = str(tmp_path / 'run1')
    run = _train(data, out1, renoise)
    assert run.returncode == 0, run.stderr[-2000:]
    assert sorted(os.listdir(os.path.join(out1, 'test_noisy'))) == ['t1_n1.obj', 't1_n2.obj']
    assert sorted(f for f in os.listdir(os.path.join(out1, 'result')) if f.endswith('.obj')) == ['t1_n1-60.obj', 't1_n2-60.obj']
    assert 'angle1' in run.stdout                                  # the result meshes were scored against test/original
    with open(os.path.join(out1, 'GeoBi-GNN_Synthetic_params.json')) as fh:
        params = json.load(fh)
    assert params['noise_levels'] == [0.1, 0.2] and params['renoise_every'] == 1 and params['noise_kind'] == 'gaussian'
    assert params['noise_direction'] == 'normal' and params['noise_fraction'] == 0.3
    assert not os.path.exists(os.path.join(data, 'train', 'noisy')) and not os.path.exists(os.path.join(data, 'test', 'noisy'))
    assert not os.path.exists(os.path.join(data, 'train', 'processed_data'))

    out2 = str(tmp_path / 'run2')
    run = _train(data, out2, renoise + ['--no_predict'])
    assert run.returncode == 0, run.stderr[-2000:]
    assert _model_bytes(out2) == _model_bytes(out1)

    out3 = str(tmp_path / 'run3')
    run = _train(data, out3, ['--noise_levels', '0.1,0.2', '--renoise_every', '0', '--no_predict'])
    assert run.returncode == 0, run.stderr[-2000:]
    assert _model_bytes(out3) != _model_bytes(out1)

    # the file-mode loop over files the `noise` command writes with the same seed: the model of --renoise_every 0
    files = str(tmp_path / 'Files')
    shutil.copytree(data, files)
    for split in ('train', 'test'):
        run = _run(['noise', '--data_dir', os.path.join(files, split), '--levels', '0.1,0.2', '--seed', '31'])
        assert run.returncode == 0, run.stderr[-2000:]
    out4 = str(tmp_path / 'run4')
    run = _train(files, out4, ['--no_predict'])
    assert run.returncode == 0, run.stderr[-2000:]
    assert _model_bytes(out4) == _model_bytes(out3)
    print('epoch seconds: renoise_every 1 %s, renoise_every 0 %s, file mode %s'
          % (_epoch_seconds(out1), _epoch_seconds(out3), _epoch_seconds(out4)))
    # --renoise_every without --noise_levels is refused
    run = _train(files, str(tmp_path / 'run5'), ['--renoise_every', '1', '--no_predict'])
    assert run.returncode != 0
