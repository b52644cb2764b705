"""The surface sampler's host model (tests/sample_model.py) against its own specification, the box experiment that
motivates sampled alignment, write_obj(normals=) and the new command-line flags.  No GPU."""
import math

import numpy as np
import pytest

import icp_model as M
import noise_model as NM
import sample_model as S


def test_barycentrics_are_exact_in_float32_and_not_negative():
    """200 000 draws: the fold and 1 - u1 - u2 in float32 equal the fp64 evaluation exactly; b0 >= 0, the rows sum to 1."""
    w = NM.words_of(np.arange(200000, dtype=np.uint64), 7, 3, 1, S.BLOCK)
    b32, b64 = S.bary32(w[2], w[3]), S.bary64(w[2], w[3])
    assert b32.dtype == np.float32
    assert np.array_equal(b32.astype(np.float64), b64)
    assert b32[:, 0].min() >= 0 and b32.min() >= 0 and b32.max() < 1
    assert np.array_equal(b64.sum(1), np.ones(len(b64)))
    assert (NM.uniform(w[2]) + NM.uniform(w[3]) > 1).mean() > 0.4          # the fold is exercised


def _five_faces():
    """Areas 1 : 9 and three degenerate faces (first, between the two, last)."""
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [3, 0, 1], [0, 3, 1], [0, 0, 1]], np.float32)
    f = np.array([[0, 0, 1], [0, 1, 2], [1, 2, 1], [5, 3, 4], [3, 3, 3]], np.int32)
    return p, f


def test_counts_follow_the_areas_and_degenerate_faces_are_never_drawn():
    p, f = _five_faces()
    w, cum, e = S.weights(p, f)
    assert w.tolist() == [0, 2 ** 28, 0, 9 * 2 ** 28, 0] and e == 4 and cum[-1] == 10 * 2 ** 28
    assert math.ldexp(int(cum[-1]), e - 33) == 5.0                       # the area: 0.5 + 4.5
    n = 200000
    face = S.sample(p, f, n, seed=1)['face']
    counts = np.bincount(face, minlength=5)
    sigma = math.sqrt(n * 0.1 * 0.9)
    print('counts %s: the small face %d of %d (%.2f sigma from 0.1)' % (counts.tolist(), counts[1], n, (counts[1] - 0.1 * n) / sigma))
    assert counts[0] == counts[2] == counts[4] == 0
    assert abs(counts[1] - 0.1 * n) <= 5 * sigma, counts


def test_samples_lie_on_their_faces():
    p, f = S.strip(37, seed=2)
    got = S.sample(p, f, 5000, seed=3)
    assert got['face'].min() >= 0 and got['face'].max() < 37 and len(np.unique(got['face'])) == 37
    a, b, c = (p[f[got['face'], k]].astype(np.float64) for k in range(3))
    n = np.cross(b - a, c - a)
    off = np.abs(((got['points'] - a) * n).sum(1)) / np.linalg.norm(n, axis=1)
    assert off.max() <= 1e-12


def test_a_sample_depends_on_its_row_only():
    """The first n rows of an N-draw are the n-draw; first = k gives rows k..; another draw or stream differs."""
    p, f = S.strip(50, seed=1)
    whole = S.sample(p, f, 1000, seed=5, stream_id=9, draw=2)
    head = S.sample(p, f, 300, seed=5, stream_id=9, draw=2)
    tail = S.sample(p, f, 700, seed=5, stream_id=9, draw=2, first=300)
    for key in ('points', 'face', 'bary'):
        assert np.array_equal(whole[key][:300], head[key]) and np.array_equal(whole[key][300:], tail[key])
    for other in (S.sample(p, f, 1000, seed=5, stream_id=9, draw=3), S.sample(p, f, 1000, seed=5, stream_id=8, draw=2),
                  S.sample(p, f, 1000, seed=6, stream_id=9, draw=2)):
        assert (other['face'] != whole['face']).mean() > 0.5 and not np.array_equal(other['bary'], whole['bary'])


def test_a_mesh_without_area_selects_no_face():
    p, f = _five_faces()
    w, cum, e = S.weights(p, f[[0, 2, 4]])
    assert w.tolist() == [0, 0, 0] and e == 0 and S.select(cum, 10, 1)[0].tolist() == [-1] * 10


def test_box_alignment_improves_with_samples():
    """A 12-triangle box as the target, the finely meshed box turned by 5 degrees as the source: ICP onto the 8 target
    vertices ends further from the true pose than it began; onto the vertices plus 2 000 samples of the surface it ends at
    least 5 times nearer (DESIGN.md 4l quotes both angles)."""
    src, _, tp, tf, R_true = S.box_case(5.0)
    assert src.shape == (866, 3) and tp.shape == (8, 3) and tf.shape == (12, 3)
    drawn = S.sample(tp, tf, 2000, seed=1)['points'].astype(np.float32)
    plain = S.residual_angle(M.icp(src, tp)['R'], R_true)
    sampled = S.residual_angle(M.icp(src, np.concatenate([tp, drawn]))['R'], R_true)
    message = 'residual angle to the true pose: %.2f degrees onto the vertices, %.2f onto vertices and samples' % (plain, sampled)
    print(message)
    assert plain >= 5 * sampled, message
    assert sampled < 1.0 < plain, message


def test_folded_quad_shares_its_vertices_and_differs_inside():
    p, fa, fb = S.folded_quad(0.3)
    assert sorted(np.unique(fa)) == sorted(np.unique(fb)) == [0, 1, 2, 3]
    mid_a = 0.5 * (p[0] + p[2]).astype(np.float64)                       # on A's diagonal
    mid_b = 0.5 * (p[1] + p[3]).astype(np.float64)                       # on B's
    assert abs(abs(mid_a[2] - mid_b[2]) - 0.3) <= 1e-7 and np.array_equal(mid_a[:2], mid_b[:2])


def test_write_obj_with_normals_round_trips(tmp_path):
    from geobi_gnn_amd import meshio
    rng = np.random.default_rng(0)
    pts = rng.standard_normal((50, 3)).astype(np.float32)
    vn = rng.standard_normal((50, 3)).astype(np.float32)
    path = str(tmp_path / 'cloud.obj')
    meshio.write_obj(path, pts, np.zeros((0, 3), np.int32), normals=vn)
    got, faces = meshio.read_obj(path)
    assert np.array_equal(got.view(np.uint32), pts.view(np.uint32)) and faces.shape == (0, 3)
    lines = open(path).read().splitlines()
    assert len(lines) == 100 and all(ln.startswith('v ') for ln in lines[:50]) and all(ln.startswith('vn ') for ln in lines[50:])
    back = np.array([[float(x) for x in ln.split()[1:]] for ln in lines[50:]], np.float64).astype(np.float32)
    assert np.array_equal(back.view(np.uint32), vn.view(np.uint32))
    # a mesh keeps its faces beside the normals, and without normals the file is what it was
    fv = np.array([[0, 1, 2], [2, 3, 4]], np.int32)
    meshio.write_obj(path, pts, fv, normals=vn)
    got, faces = meshio.read_obj(path)
    assert np.array_equal(got.view(np.uint32), pts.view(np.uint32)) and np.array_equal(faces, fv)
    meshio.write_obj(path, pts, fv)
    assert 'vn' not in open(path).read()
    with pytest.raises(ValueError):
        meshio.write_obj(path, pts, fv, normals=vn[:-1])


def test_parser_takes_the_sampling_flags(capsys):
    from geobi_gnn_amd.__main__ import parse_args
    opt = parse_args(['sample', '--data_dir', 'd', '--n', '1000'])
    assert opt.command == 'sample' and opt.n == 1000 and opt.seed == 1 and opt.normals is False and opt.out_dir == '' and opt.gpu == -1
    opt = parse_args(['sample', '--data_dir', 'd', '--n', '5', '--seed', '7', '--normals', '--out_dir', 'o'])
    assert opt.seed == 7 and opt.normals is True and opt.out_dir == 'o'
    opt = parse_args(['eval', '--result_dir', 'r', '--original_dir', 'o', '--free', '--samples', '2000', '--seed', '3'])
    assert opt.samples == 2000 and opt.seed == 3 and opt.free
    opt = parse_args(['eval', '--result_dir', 'r', '--original_dir', 'o', '--free'])
    assert opt.samples == 0 and opt.seed == 1
    opt = parse_args(['align', '--data_dir', 'd', '--target_dir', 't', '--samples', '2000'])
    assert opt.samples == 2000 and opt.seed == 1
    assert parse_args(['align', '--data_dir', 'd', '--target_dir', 't']).samples == 0
    for bad in (['eval', '--result_dir', 'r', '--original_dir', 'o', '--samples', '2000'],
                ['eval', '--result_dir', 'r', '--original_dir', 'o', '--free', '--samples', '-1'],
                ['align', '--data_dir', 'd', '--target_dir', 't', '--samples', '-5'],
                ['sample', '--data_dir', 'd'],
                ['sample', '--data_dir', 'd', '--n', '-1']):
        with pytest.raises(SystemExit):
            parse_args(bad)
    assert '--samples needs --free' in capsys.readouterr().err
