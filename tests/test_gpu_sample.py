"""The surface sampler on the device (csrc/sample.hip, meshsample.py) against its host model (tests/sample_model.py),
and its three consumers: eval_sampled, align(samples=) and the commands.  The model is fed the DEVICE's cum wherever a
selection is compared, so the integer part stands on its own and a weight difference cannot hide a search bug."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import icp_model as M
import sample_model as S

pytestmark = pytest.mark.gpu

TOL = 1e-5                      # the project's bar (tests/test_gpu_kernels.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


def _t(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


def _table():
    from geobi_gnn_amd import meshsample
    return meshsample.table_entries()


def _degenerate(F):
    """Degenerate faces first, last and in a run in the middle (none below 8 faces)."""
    return (0, F // 2, F // 2 + 1, F // 2 + 2, F - 1) if F >= 8 else ()


_MESHES = {}


def _mesh(F, grid=False, offset=0.0, heavy=None, degenerate=None):
    """One strip per key, built once and never changed -> points float32, faces int32, the model's (weight, cum, e)."""
    key = (F, grid, offset, heavy, degenerate)
    if key not in _MESHES:
        p, f = S.strip(F, seed=F % 97, grid=grid, offset=offset, heavy=heavy,
                       degenerate=_degenerate(F) if degenerate is None else degenerate)
        _MESHES[key] = (p, f, S.weights(p, f))
    return _MESHES[key]


def _device_weights(p, f, dev):
    from geobi_gnn_amd import meshsample
    weight, cum, e = meshsample.surface_weights(_t(p, dev), _t(f, dev, torch.int32))
    assert weight.dtype == torch.int64 and cum.dtype == torch.int64 and isinstance(e, int)
    return weight.cpu().numpy(), cum.cpu().numpy(), e


WEIGHT_F = (1, 2, 255, 256, 257, 300001)        # the last crosses the scan's tiles and the grid-stride walk


# ------------------------------------------------------------------------------------------------ 1. weights
@pytest.mark.parametrize('F', WEIGHT_F)
def test_weights_equal_the_model_on_a_grid_mesh(dev, F):
    """Coordinates on the 1/8 grid below 64: every product, difference and sum of the weights is exact in fp64, so weight,
    cum and exponent equal the model bit for bit."""
    p, f, (w_ref, cum_ref, e_ref) = _mesh(F, grid=True)
    assert np.array_equal(p * 8, np.round(p * 8)) and p.max() < 64 and p.min() >= 0
    w, cum, e = _device_weights(p, f, dev)
    assert e == e_ref and np.array_equal(w, w_ref) and np.array_equal(cum, cum_ref)
    assert (w[list(_degenerate(F))] == 0).all() and w.max() >= 2 ** 31 and w.max() < 2 ** 32


@pytest.mark.parametrize('F', WEIGHT_F)
def test_weights_are_within_one_unit_of_the_model_on_a_float_mesh(dev, F):
    """A general float mesh: only the rounding of the device's fp64 sqrt stands between the device and the model, which is
    one unit of the floor at most.  cum is the exact integer scan of the DEVICE's weights."""
    p, f, (w_ref, _, e_ref) = _mesh(F)
    w, cum, e = _device_weights(p, f, dev)
    diff = np.abs(w - w_ref)
    print('F = %d: %d of %d weights differ from the model (largest difference %d)' % (F, (diff > 0).sum(), F, diff.max()))
    assert e == e_ref and diff.max() <= 1
    assert np.array_equal(cum, np.cumsum(w, dtype=np.int64)) and cum[-1] < 2 ** 56
    assert (w[list(_degenerate(F))] == 0).all() and (w >= 0).all() and w.max() >= 2 ** 31 and w.max() < 2 ** 32


# ------------------------------------------------------------------------------------------------ 2. / 3. selection, points
def _check_draw(dev, p, f, n, seed=11, stream_id=5, draw=1, first=0):
    """One device draw against the model fed the device's cum -> the device's arrays on the host."""
    from geobi_gnn_amd import meshsample
    pd, fd = _t(p, dev), _t(f, dev, torch.int32)
    weights = meshsample.surface_weights(pd, fd)
    got = meshsample.sample_surface(pd, fd, n, seed=seed, stream_id=stream_id, draw=draw, first=first, weights=weights)
    assert got.points.shape == (n, 3) and got.face.shape == (n,) and got.bary.shape == (n, 3)
    assert got.points.dtype == torch.float32 and got.face.dtype == torch.int32 and got.bary.dtype == torch.float32
    w, cum = weights[0].cpu().numpy(), weights[1].cpu().numpy()
    face, pts, bary = got.face.cpu().numpy(), got.points.cpu().numpy(), got.bary.cpu().numpy()
    ref = S.sample(p, f, n, seed, stream_id, draw, first, cum=cum)
    assert np.array_equal(face, ref['face'])                               # every sample
    assert (w[face] > 0).all()                                             # never a zero-weight face
    assert np.array_equal(bary.view(np.uint32), ref['bary'].view(np.uint32))
    assert bary[:, 0].min() >= 0
    bound = 4 * 2.0 ** -24 * np.abs(p[f[face]].astype(np.float64)).max(axis=(1, 2))
    err = np.abs(pts.astype(np.float64) - ref['points'])
    print('F = %d, n = %d: largest point error %.3g of its bound' % (len(f), n, (err / bound[:, None]).max()))
    assert (err <= bound[:, None]).all()
    return face, pts, bary, w


# F in terms of T, the LDS table size the binding reports (read in the test: the lists here are made at collection)
_F_OF_T = {'1': lambda T: 1, '2': lambda T: 2, '3': lambda T: 3, 'T-1': lambda T: T - 1, 'T': lambda T: T,
           'T+1': lambda T: T + 1, '2T+1': lambda T: 2 * T + 1, '300001': lambda T: 300001}
_DRAW_PAIRS = (('1', 257), ('2', 1), ('3', 255), ('T-1', 256), ('T', 100003), ('T+1', 100003), ('2T+1', 257),
               ('300001', 100003), ('300001', 255))


@pytest.mark.parametrize('F_of_T,n', _DRAW_PAIRS)
def test_selection_and_points_equal_the_model(dev, F_of_T, n):
    """F around the LDS table (T - 1, T: all of cum in LDS; T + 1, 2 T + 1, 300 001: a bucket finished from global memory),
    n around one block and beyond the grid: face equal for every sample, barycentrics bit for bit, points within three
    float32 roundings of terms bounded by the face's largest coordinate."""
    T = _table()
    assert 8 <= T < 100000 and {k for k, _ in _DRAW_PAIRS} == set(_F_OF_T)
    F = _F_OF_T[F_of_T](T)
    p, f, _ = _mesh(F)
    face, _, _, w = _check_draw(dev, p, f, n)
    if n >= 100000 and F > 8:
        drawn = np.bincount(face, minlength=F) > 0
        print('F = %d: %d of %d faces with weight drawn at least once' % (F, drawn.sum(), (w > 0).sum()))
        assert not drawn[list(_degenerate(F))].any() and drawn.sum() > min((w > 0).sum(), n) // 4


@pytest.mark.parametrize('heavy', ('last', 'first'))
def test_a_face_with_ninety_percent_of_the_area(dev, heavy):
    F = 3000
    p, f, (w_ref, cum_ref, _) = _mesh(F, heavy=F - 1 if heavy == 'last' else 0, degenerate=())
    k = F - 1 if heavy == 'last' else 0
    share = w_ref[k] / cum_ref[-1]
    assert 0.9 <= share <= 0.91
    n = 20000
    face, _, _, _ = _check_draw(dev, p, f, n)
    got = (face == k).mean()
    print('heavy %s face: %.4f of the samples (area share %.4f)' % (heavy, got, share))
    assert abs(got - share) <= 5 * math.sqrt(share * (1 - share) / n)


def test_a_mesh_that_ends_in_ten_degenerate_faces(dev):
    F = 500
    p, f, (w_ref, _, _) = _mesh(F, degenerate=tuple(range(F - 10, F)))
    assert (w_ref[-10:] == 0).all() and (w_ref[:-10] > 0).all()
    face, _, _, _ = _check_draw(dev, p, f, 50000)
    assert face.max() == F - 11                                            # the last face with area is reached, none beyond


def test_points_of_a_mesh_offset_by_a_thousand(dev):
    p, f, _ = _mesh(300, offset=1000.0)
    assert p.min() > 990
    _, pts, _, _ = _check_draw(dev, p, f, 5000)
    assert pts.min() > 990


# ------------------------------------------------------------------------------------------------ 4. determinism
def test_same_bits_twice_in_chunks_and_with_weights_handed_in(dev):
    from geobi_gnn_amd import meshsample
    p, f, _ = _mesh(2 * _table() + 1)
    pd, fd = _t(p, dev), _t(f, dev, torch.int32)
    n, kw = 3001, {'seed': 2 ** 40 + 3, 'stream_id': 77, 'draw': 4}
    one = meshsample.sample_surface(pd, fd, n, **kw)
    two = meshsample.sample_surface(pd, fd, n, **kw)
    weights = meshsample.surface_weights(pd, fd)
    handed = meshsample.sample_surface(pd, fd, n, weights=weights, **kw)
    cuts = (0, 1000, 1257, n)
    chunks = [meshsample.sample_surface(pd, fd, b - a, first=a, weights=weights, **kw) for a, b in zip(cuts, cuts[1:])]
    for k in range(3):
        assert torch.equal(one[k], two[k]) and torch.equal(one[k], handed[k])
        assert torch.equal(one[k], torch.cat([c[k] for c in chunks]))
    other = meshsample.sample_surface(pd, fd, n, seed=kw['seed'], stream_id=77, draw=5)
    assert not torch.equal(other.face, one.face)
    empty = meshsample.sample_surface(pd, fd, 0, **kw)
    assert empty.points.shape == (0, 3) and empty.face.shape == (0,)
    normals = meshsample.sample_normals(pd, fd, one).cpu().numpy().astype(np.float64)
    fc = f[one.face.cpu().numpy()]
    nn = np.cross(p[fc[:, 1]].astype(np.float64) - p[fc[:, 0]], p[fc[:, 2]].astype(np.float64) - p[fc[:, 0]])
    assert np.abs(normals - nn / np.linalg.norm(nn, axis=1, keepdims=True)).max() <= 1e-4


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_come_in_words_before_any_launch(dev):
    from geobi_gnn_amd import meshsample
    from geobi_gnn_amd._lib import GeobiError
    p, f, _ = _mesh(300)
    pd, fd = _t(p, dev), _t(f, dev, torch.int32)
    flat = fd.clone()
    flat[:, 2] = flat[:, 0]                                                # every face degenerate
    with pytest.raises(GeobiError, match='without area'):
        meshsample.sample_surface(pd, flat, 10, seed=1)
    weight, cum, e = meshsample.surface_weights(pd, flat)                  # the weights themselves are an answer: all 0
    assert int(weight.abs().sum()) == 0 and int(cum[-1]) == 0 and e == 0
    with pytest.raises(GeobiError, match='without area'):
        meshsample.sample_surface(pd, fd[:0].contiguous(), 10, seed=1)
    for value in (p.shape[0], -1):
        bad = fd.clone()
        bad[7, 1] = value
        with pytest.raises(GeobiError, match='outside'):
            meshsample.sample_surface(pd, bad, 10, seed=1)
        with pytest.raises(GeobiError, match='outside'):
            meshsample.surface_weights(pd, bad)
    with pytest.raises(GeobiError, match='no CPU fallback'):
        meshsample.sample_surface(torch.from_numpy(p), fd, 10, seed=1)
    with pytest.raises(GeobiError, match='no CPU fallback'):
        meshsample.sample_surface(pd, torch.from_numpy(f), 10, seed=1)
    with pytest.raises(ValueError, match='negative'):
        meshsample.sample_surface(pd, fd, -1, seed=1)
    with pytest.raises(ValueError, match='negative'):
        meshsample.sample_surface(pd, fd, 10, seed=1, first=-1)
    with pytest.raises(ValueError, match='exceeds'):
        meshsample.sample_surface(pd, fd, 10, seed=1, first=2 ** 24 - 10)
    with pytest.raises(ValueError, match='64 bits'):
        meshsample.sample_surface(pd, fd, 10, seed=-1)
    with pytest.raises(ValueError, match='another mesh'):
        meshsample.sample_surface(pd, fd, 10, seed=1, weights=meshsample.surface_weights(pd, fd[:100].contiguous()))
    # the C ABI says the same for what the Python layer would have stopped
    from geobi_gnn_amd import _lib as L
    out = meshsample.sample_surface(pd, fd, 10, seed=1)
    cum = meshsample.surface_weights(pd, fd)[1]
    with pytest.raises(GeobiError, match='first'):
        L.call('geobi_sample_surface', L.ptr(pd), L.ptr(fd), L.ptr(cum), fd.shape[0], pd.shape[0], 10, 2 ** 24 - 5, 1, 0, 0,
               L.ptr(out.points), L.ptr(out.face), L.ptr(out.bary), L.stream())


# ------------------------------------------------------------------------------------------------ 6. eval_sampled
def test_eval_sampled_sees_what_no_vertex_can(dev):
    """The folded quad cut along one diagonal and along the other (h = 0.3): all four vertices are shared, so eval_free
    measures exactly 0; the sampled distances are those of the fp64 statement on the device's own sample points."""
    from geobi_gnn_amd import mesheval, meshsample
    from test_gpu_mesheval import _rel, _surface_fp64
    p, fa, fb = S.folded_quad(0.3)
    free = mesheval.eval_free(p, fa, p, fb, device=dev)
    assert free['surf'] == 0.0 and free['surf_back'] == 0.0 and free['hausdorff'] == 0.0
    n = 20000
    got = mesheval.eval_sampled(p, fa, p, fb, n, seed=1, device=dev)
    pd = _t(p, dev)
    sr = meshsample.sample_surface(pd, _t(fa, dev, torch.int32), n, seed=1, draw=1).points.cpu().numpy()
    so = meshsample.sample_surface(pd, _t(fb, dev, torch.int32), n, seed=1, draw=0).points.cpu().numpy()
    d_ro, d_or = _surface_fp64(sr, p, fb), _surface_fp64(so, p, fa)
    ref = {'surf_s': d_ro.mean(), 'surf_back_s': d_or.mean(), 'hausdorff_s': max(d_ro.max(), d_or.max())}
    e = got['scale']
    assert got['num_s'] == n and abs(e - (4 * math.sqrt(1.09) + math.sqrt(2)) / 5) <= TOL * e
    for key in ('surf_s', 'surf_back_s', 'hausdorff_s'):
        print('%s: %.9g (fp64 %.9g)' % (key, got[key], ref[key]))
        assert ref[key] > 0.01 and _rel(got[key], ref[key], e) <= TOL, key
    assert abs(got['surf_s_norm'] - got['surf_s'] / e) <= 1e-12 and abs(got['surf_back_s_norm'] - got['surf_back_s'] / e) <= 1e-12
    assert set(got) == {'num_s', 'surf_s', 'surf_back_s', 'hausdorff_s', 'angle_s', 'scale', 'surf_s_norm', 'surf_back_s_norm'}


def test_eval_sampled_against_the_numpy_statement(dev):
    """The frequency-8 bumpy sphere against the frequency-6 one.  Distances to TOL in the _rel form; the ground-truth
    triangle the device chose for a sample is as near as the nearest within TOL, and angle_s is the fp64 angle recomputed
    from the device's indices (test_eval_free_against_the_numpy_statement's way)."""
    from geobi_gnn_amd import mesheval, meshsample
    from test_gpu_mesheval import _rel, _surface_fp64, _tri_dist_fp64
    (pr, fr), (po, fo) = M.bumpy(8), M.bumpy(6)
    n = 4000
    got = mesheval.eval_sampled(pr, fr, po, fo, n, seed=3, stream_id=9, device=dev)
    prd, frd, pod, fod = _t(pr, dev), _t(fr, dev, torch.int32), _t(po, dev), _t(fo, dev, torch.int32)
    sr = meshsample.sample_surface(prd, frd, n, seed=3, stream_id=9, draw=1)
    so = meshsample.sample_surface(pod, fod, n, seed=3, stream_id=9, draw=0)
    q, back = sr.points.cpu().numpy(), so.points.cpu().numpy()
    d_ro, d_or = _surface_fp64(q, po, fo), _surface_fp64(back, pr, fr)
    e = got['scale']
    ref = {'surf_s': d_ro.mean(), 'surf_back_s': d_or.mean(), 'hausdorff_s': max(d_ro.max(), d_or.max())}
    for key in ref:
        print('%s: %.9g (fp64 %.9g)' % (key, got[key], ref[key]))
        assert _rel(got[key], ref[key], e) <= TOL, key
    _, near = mesheval.point_to_mesh(sr.points, pod, fod)
    near = near.cpu().numpy()
    p64, o64 = pr.astype(np.float64), po.astype(np.float64)
    t = fo[near]
    d_at = _tri_dist_fp64(q, o64[t[:, 0]], o64[t[:, 1]], o64[t[:, 2]])
    assert _rel(d_at, d_ro, e) <= TOL

    def normals(p, t):
        c = np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
        return c / np.linalg.norm(c, axis=1, keepdims=True)
    err = ((normals(p64, fr)[sr.face.cpu().numpy()] - normals(o64, fo)[near]) ** 2).sum(1)
    angle = (np.arccos(np.clip(1 - err / 2, -1, 1)) * 180 / np.pi).mean()
    print('angle_s: %.9g (fp64 from the device indices %.9g)' % (got['angle_s'], angle))
    assert abs(got['angle_s'] - angle) <= TOL * angle
    with pytest.raises(ValueError):
        mesheval.eval_sampled(pr, fr, po, fo, 0, device=dev)


# ------------------------------------------------------------------------------------------------ 7. align(samples=)
def test_align_with_samples_on_the_box(dev):
    """The 12-triangle box as the target, the finely meshed box turned by 5 degrees as the source.  R, T, s and rmse against
    icp_model.icp on the device's own target set, at the bars of tests/test_gpu_icp.py; those bars presuppose what that file
    checks of its inputs -- no nearest-neighbour gap below 1e-5 and no relative rmse change near the 1e-6 threshold -- and
    seed 4 is the first seed for which the model run has both (seed 1: a gap of 3e-6).  The residual angle to the true pose
    is at least 5 times smaller than without samples."""
    from geobi_gnn_amd import mesheval
    src, _, tp, tf, R_true = S.box_case(5.0)
    res = mesheval.align(src, tp, device=dev, target_faces=tf, samples=2000, seed=4)
    target = mesheval.align_target(tp, tf, 2000, seed=4, device=dev).cpu().numpy()
    assert target.shape == (2008, 3) and np.array_equal(target[:8], tp)
    ref = M.icp(src, target)
    assert min(float(t['nn_gap'].min()) for t in ref['trace']) >= 1e-5
    assert all(t['rel'] >= 2e-6 or (t['same_idx'] and t['rel'] == 0.0) for t in ref['trace'][1:])
    R, T = res.R[0].numpy().astype(np.float64), res.T[0].numpy().astype(np.float64)
    st = res.state.cpu().numpy()[0]
    ymax = float(np.abs(target).max())
    print('%d iterations (model %d), rmse %.9g (model %.9g), errors R %.2e, T %.2e'
          % (int(res.iterations[0]), ref['iterations'], st[13], ref['rmse'], np.abs(st[:9].reshape(3, 3) - ref['R']).max(),
             np.abs(st[9:12] - ref['T']).max()))
    assert int(res.iterations[0]) == ref['iterations'] and bool(res.converged[0]) == ref['converged']
    assert np.abs(st[:9].reshape(3, 3) - ref['R']).max() <= 1e-9 and np.abs(st[9:12] - ref['T']).max() <= 1e-9 * ymax
    assert abs(st[12] - ref['s']) <= 1e-9 * ref['s'] and abs(st[13] - ref['rmse']) <= 1e-9 * ymax
    assert np.abs(R - ref['R']).max() <= 1e-6 and np.abs(T - ref['T']).max() <= 1e-6
    plain = mesheval.align(src, tp, device=dev)
    a_plain = S.residual_angle(plain.state.cpu().numpy()[0][:9].reshape(3, 3), R_true)
    a_sampled = S.residual_angle(st[:9].reshape(3, 3), R_true)
    message = 'residual angle to the true pose: %.3f degrees onto the vertices, %.3f onto vertices and samples' % (a_plain, a_sampled)
    print(message)
    assert a_plain >= 5 * a_sampled, message
    with pytest.raises(ValueError, match='target_faces'):
        mesheval.align(src, tp, device=dev, samples=10)


# ------------------------------------------------------------------------------------------------ 8. commands
def _run(args):
    run = subprocess.run([sys.executable, '-m', 'geobi_gnn_amd'] + args, cwd=ROOT, timeout=300, capture_output=True, text=True)
    print(run.stdout)
    print(run.stderr)
    return run


def test_sample_command(dev, tmp_path):
    """`sample --normals` on two small files, one with a degenerate face: the written points are sample_surface's bit for
    bit and lie on their faces; a file without area is skipped and counted.  One child process."""
    from geobi_gnn_amd import meshio, meshnoise, meshsample
    p, f, _ = _mesh(37)
    p2, f2, _ = _mesh(12, degenerate=(3,))
    meshio.write_obj(str(tmp_path / 'strip.obj'), p, f)
    meshio.write_obj(str(tmp_path / 'dent.obj'), p2, f2)
    (tmp_path / 'flat.obj').write_text('v 0 0 0\nv 1 0 0\nv 2 0 0\nf 1 2 3\n')
    out = tmp_path / 'cloud'
    run = _run(['sample', '--data_dir', str(tmp_path), '--out_dir', str(out), '--n', '1000', '--seed', '6', '--normals'])
    assert run.returncode == 1 and 'without area' in run.stderr and '1 of 3 files skipped' in run.stderr
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith('V:')]
    assert len(lines) == 2 and "'dent.obj'" in lines[0] and "'strip.obj'" in lines[1]
    assert 'zero_faces: 1,' in lines[0] and ('zero_faces: %d,' % len(_degenerate(37))) in lines[1]     # the strip carries its own
    assert not (out / 'flat.obj').exists()
    for name, pts, faces in (('strip', p, f), ('dent', p2, f2)):
        got, none = meshio.read_obj(str(out / (name + '.obj')))
        assert none.shape == (0, 3)
        text = (out / (name + '.obj')).read_text().splitlines()
        assert len(text) == 2000 and all(ln.startswith('v ') for ln in text[:1000]) and all(ln.startswith('vn ') for ln in text[1000:])
        pd, fd = _t(pts, dev), _t(faces, dev, torch.int32)
        want = meshsample.sample_surface(pd, fd, 1000, seed=6, stream_id=meshnoise.stream_of(name))
        assert np.array_equal(got.view(np.uint32), want.points.cpu().numpy().view(np.uint32))
        vn = np.array([[float(x) for x in ln.split()[1:]] for ln in text[1000:]], np.float64).astype(np.float32)
        assert np.array_equal(vn.view(np.uint32), meshsample.sample_normals(pd, fd, want).cpu().numpy().view(np.uint32))
        area = 0.5 * S.face_norms(pts, faces).sum()
        line = lines[0 if name == 'dent' else 1]
        assert abs(float(line.split('area:')[1].split(',')[0]) - area) <= 1e-5 * area
        # on their faces: the fp64 distance to the face each sample was drawn from
        from test_gpu_mesheval import _tri_dist_fp64
        t = faces[want.face.cpu().numpy()]
        p64 = pts.astype(np.float64)
        d = _tri_dist_fp64(got, p64[t[:, 0]], p64[t[:, 1]], p64[t[:, 2]])
        assert d.max() <= 4 * 2.0 ** -24 * np.abs(pts).max() * math.sqrt(3)


def test_eval_command_with_samples(dev, tmp_path):
    """`eval --free --samples 2000` writes ErrorInfo_sampled.txt with eval_sampled's numbers, and ErrorInfo_free.txt is
    byte-equal to a run without the flag.  Two child processes, the second only after the first returned 0."""
    from geobi_gnn_amd import mesheval, meshio, meshnoise
    res, orig = tmp_path / 'res', tmp_path / 'orig'
    res.mkdir()
    orig.mkdir()
    (p8, f8), (p6, f6) = M.bumpy(8), M.bumpy(6)
    p, fa, fb = S.folded_quad(0.3)
    meshio.write_obj(str(orig / 'a.obj'), p6, f6)
    meshio.write_obj(str(res / 'a_1.obj'), p8, f8)
    meshio.write_obj(str(orig / 'q.obj'), p, fb)
    meshio.write_obj(str(res / 'q_1.obj'), p, fa)
    run = _run(['eval', '--result_dir', str(res), '--original_dir', str(orig), '--free'])
    assert run.returncode == 0, run.stderr[-2000:]
    before = (res / 'ErrorInfo_free.txt').read_bytes()
    assert not (res / 'ErrorInfo_sampled.txt').exists()
    run = _run(['eval', '--result_dir', str(res), '--original_dir', str(orig), '--free', '--samples', '2000', '--seed', '5'])
    assert run.returncode == 0, run.stderr[-2000:]
    assert (res / 'ErrorInfo_free.txt').read_bytes() == before
    rows = [ln.split() for ln in (res / 'ErrorInfo_sampled.txt').read_text().splitlines() if ln.strip()]
    assert rows[0][0] == 'Error_sampled:' and len(rows) == 4 and [r[0] for r in rows[2:]] == ['a_1.obj', 'q_1.obj']
    cols = ('num_s', 'angle_s', 'surf_s', 'surf_s_norm', 'surf_back_s', 'surf_back_s_norm', 'hausdorff_s')
    want = [mesheval.eval_sampled(p8, f8, p6, f6, 2000, seed=5, stream_id=meshnoise.stream_of('a'), device=dev),
            mesheval.eval_sampled(p, fa, p, fb, 2000, seed=5, stream_id=meshnoise.stream_of('q'), device=dev)]
    for row, w in zip(rows[2:], want):
        assert len(row) == 8
        for key, tok in zip(cols, row[1:]):
            assert abs(float(tok) - w[key]) <= 0.51e-6, (key, tok, w[key])
    tot = mesheval.sampled_totals(want)
    assert len(rows[1]) == 7 and int(rows[1][0]) == 4000
    for key, tok in zip(cols, rows[1]):
        assert abs(float(tok) - tot[key]) <= 0.51e-6, (key, tok, tot[key])
    assert float(rows[3][3]) > 0.01                                        # the folded quad: what ErrorInfo_free.txt calls 0
    free_rows = [ln.split() for ln in before.decode().splitlines() if ln.strip()]
    assert free_rows[3][0] == 'q_1.obj' and float(free_rows[3][6]) == 0.0 and float(free_rows[3][8]) == 0.0


def test_align_command_with_samples(dev, tmp_path):
    """`align --samples 2000` on the box: the aligned mesh is written with its own faces and mesheval.align's bits, the
    stream is the target's name.  One child process."""
    from geobi_gnn_amd import mesheval, meshio, meshnoise
    src_dir, dst_dir, out = tmp_path / 'src', tmp_path / 'dst', tmp_path / 'out'
    src_dir.mkdir()
    dst_dir.mkdir()
    src, sf, tp, tf, R_true = S.box_case(5.0)
    meshio.write_obj(str(src_dir / 'box_1.obj'), src, sf)
    meshio.write_obj(str(dst_dir / 'box.obj'), tp, tf)
    run = _run(['align', '--data_dir', str(src_dir), '--target_dir', str(dst_dir), '--out_dir', str(out), '--samples', '2000',
                '--seed', '4'])
    assert run.returncode == 0, run.stderr[-2000:]
    pts, fv = meshio.read_obj(str(out / 'box_1.obj'))
    assert np.array_equal(fv, sf.astype(np.int32))
    want = mesheval.align(src, tp, device=dev, target_faces=tf, samples=2000, seed=4, stream_id=meshnoise.stream_of('box'))
    assert np.array_equal(pts.view(np.uint32), want.xt.cpu().numpy().view(np.uint32))
    angle = S.residual_angle(want.state.cpu().numpy()[0][:9].reshape(3, 3), R_true)
    print('residual angle %.3f degrees' % angle)
    assert angle < 1.0 and 'converged: yes' in run.stdout
