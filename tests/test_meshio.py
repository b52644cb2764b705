"""OBJ reader / writer, the host side of the evaluation (pairing, unreferenced vertices) and the size checks of the
nearest-distance entry points: everything of the mesh-file path that runs without a GPU."""
import ctypes

import numpy as np
import pytest


def test_write_then_read_is_bit_exact(tmp_path):
    from geobi_gnn_amd import meshgen, meshio
    noisy, _, faces = meshgen.noisy_icosphere(6)
    path = str(tmp_path / 'ico.obj')
    meshio.write_obj(path, noisy, faces)
    pts, fv = meshio.read_obj(path)
    assert pts.dtype == np.float32 and fv.dtype == np.int32
    assert pts.shape == noisy.shape and fv.shape == faces.shape
    assert np.array_equal(pts.view(np.uint32), np.ascontiguousarray(noisy).view(np.uint32))
    assert np.array_equal(fv, faces.astype(np.int32))


_OBJ_TEXT = '\r\n'.join([
    '# a comment',
    'mtllib scene.mtl',
    'o thing',
    'v 0 0 0',
    'v 1 0 0 1.0',                   # w ignored
    'v 1 1 0 0.5 0.25 0.125',        # r g b ignored
    'v 0 1 0',
    'vn 0 0 1',
    'vt 0.5 0.5',
    '',
    'g group1',
    'usemtl red',
    's off',
    'f 1 2 3 4',                     # quad -> (0,1,2) (0,2,3)
    'v 0.5 1.5 0',
    'v -0.5 0.5 1e-1',
    'f 1/1/1 2/1/1 3/1/1 5/1/1 4/1/1',   # pentagon -> (0,1,2) (0,2,4) (0,4,3)
    'f -1//1 -2//1 -6//1',           # relative: 6 vertices so far -> (5, 4, 0)
    'f 6/1 1/1 -3/1',                # i/t and a mix -> (5, 0, 3)
    'l 1 2',
    '# the end', ''])


def test_hand_written_obj_parses(tmp_path):
    from geobi_gnn_amd import meshio
    path = tmp_path / 'mix.obj'
    path.write_bytes(_OBJ_TEXT.encode())
    pts, fv = meshio.read_obj(str(path))
    want_p = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 1.5, 0], [-0.5, 0.5, 0.1]], dtype=np.float32)
    want_f = np.array([[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 4], [0, 4, 3], [5, 4, 0], [5, 0, 3]], dtype=np.int32)
    assert np.array_equal(pts, want_p)
    assert np.array_equal(fv, want_f)


@pytest.mark.parametrize('bad_line,what', [
    ('f 0 1 2', 'index'), ('f 1 2 5', 'index'), ('f 1 2', 'corners'), ('v nan 0 0', 'non-finite'), ('f 1 2 -5', 'index')])
def test_bad_records_raise_with_the_line_number(tmp_path, bad_line, what):
    from geobi_gnn_amd import meshio
    lines = ['v 0 0 0', 'v 1 0 0', 'v 0 1 0', 'v 0 0 1', 'f 1 2 3', bad_line, 'f 2 3 4']
    path = tmp_path / 'bad.obj'
    path.write_text('\n'.join(lines) + '\n')
    with pytest.raises(ValueError) as e:
        meshio.read_obj(str(path))
    assert 'bad.obj:6:' in str(e.value) and what in str(e.value)


def test_unreferenced_vertex_check(tmp_path):
    from geobi_gnn_amd import meshgen, meshio
    noisy, _, faces = meshgen.noisy_icosphere(6)
    assert meshio.unreferenced_vertices(noisy.shape[0], faces) == 0
    path = str(tmp_path / 'loose.obj')
    meshio.write_obj(path, noisy, faces)
    with open(path, 'a') as fh:
        fh.write('v 9 9 9\n')
    pts, fv = meshio.read_obj(path)
    assert pts.shape[0] == noisy.shape[0] + 1
    assert meshio.unreferenced_vertices(pts.shape[0], fv) == 1


def test_eval_pairing(tmp_path):
    from geobi_gnn_amd import mesheval
    res, ori = tmp_path / 'result', tmp_path / 'original'
    res.mkdir()
    ori.mkdir()
    for name in ('b.obj', 'a.obj', 'ab.obj'):
        (ori / name).write_text('')
    for name in ('a_n2-60.obj', 'ab_n1-60.obj', 'a_n1-60.obj', 'b_n1-60.obj', 'a.obj', 'ErrorInfo_h.txt'):
        (res / name).write_text('')
    pairs = [(r[len(str(res)) + 1:], o[len(str(ori)) + 1:]) for r, o in mesheval.pair_files(str(res), str(ori))]
    assert pairs == [('a_n1-60.obj', 'a.obj'), ('a_n2-60.obj', 'a.obj'), ('ab_n1-60.obj', 'ab.obj'), ('b_n1-60.obj', 'b.obj')]


def test_denoise_job_list(tmp_path):
    """original/NAME.obj pairs with noisy/NAME_n*.obj (test_dual.py:104-110); without the two folders every *.obj."""
    from geobi_gnn_amd.__main__ import _denoise_list
    (tmp_path / 'original').mkdir()
    (tmp_path / 'noisy').mkdir()
    for name in ('a.obj', 'ab.obj'):
        (tmp_path / 'original' / name).write_text('')
    for name in ('a_n2.obj', 'a_n1.obj', 'ab_n1.obj', 'a_x.obj'):
        (tmp_path / 'noisy' / name).write_text('')
    jobs = [(os_base(n), os_base(g)) for n, g in _denoise_list(str(tmp_path))]
    assert jobs == [('a_n1.obj', 'a.obj'), ('a_n2.obj', 'a.obj'), ('ab_n1.obj', 'ab.obj')]
    flat = tmp_path / 'flat'
    flat.mkdir()
    for name in ('y.obj', 'x.obj', 'z.txt'):
        (flat / name).write_text('')
    assert [(os_base(n), g) for n, g in _denoise_list(str(flat))] == [('x.obj', None), ('y.obj', None)]


def os_base(p):
    import os
    return os.path.basename(p)


def test_totals_are_count_weighted():
    from geobi_gnn_amd import mesheval
    rows = [dict(num_f=10, err_face=1.0, angle=2.0, num_v=4, err_v=1.0, err_v_norm=2.0, surf=0.5, surf_norm=1.0, hausdorff=3.0),
            dict(num_f=30, err_face=3.0, angle=6.0, num_v=12, err_v=3.0, err_v_norm=6.0, surf=1.5, surf_norm=3.0, hausdorff=2.0)]
    t = mesheval.totals(rows)
    assert t['num_f'] == 40 and t['num_v'] == 16
    assert t['err_face'] == 2.5 and t['angle'] == 5.0 and t['err_v'] == 2.5 and t['err_v_norm'] == 5.0
    assert t['surf'] == 1.25 and t['surf_norm'] == 2.5 and t['hausdorff'] == 3.0


def test_nearest_sizes_are_checked_before_any_launch():
    """geobi_nearest_ws_bytes answers without a GPU; Q or T above GEOBI_MAX_NODES is an error naming the limit, returned
    before anything touches the device (the pointers are never dereferenced)."""
    from geobi_gnn_amd import _lib as L
    lib = L.lib()
    max_nodes = (1 << 24) - 1
    assert lib.geobi_nearest_ws_bytes(10242, 20480) > 0
    assert lib.geobi_nearest_ws_bytes(1, 1) > 0
    assert lib.geobi_dist_summary_ws_bytes(10242) > 0
    one = ctypes.c_void_p(256)
    for Q, T in ((max_nodes + 1, 10), (10, max_nodes + 1)):
        rc = lib.geobi_nearest_point(one, one, Q, T, one, one, one, 1 << 20, None)
        assert rc != 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
        rc = lib.geobi_nearest_triangle(one, one, one, Q, 10, T, one, one, one, 1 << 20, None)
        assert rc != 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
    rc = lib.geobi_nearest_triangle(one, one, one, 10, max_nodes + 1, 10, one, one, one, 1 << 20, None)
    assert rc != 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
    rc = lib.geobi_dist_summary(one, max_nodes + 1, one, one, 1 << 20, None)
    assert rc != 0 and b'GEOBI_MAX_NODES' in lib.geobi_last_error()
    # an empty target set and a workspace that is too small are errors as well, again before a launch
    rc = lib.geobi_nearest_point(one, one, 10, 0, one, one, one, 1 << 20, None)
    assert rc != 0 and b'empty' in lib.geobi_last_error()
    rc = lib.geobi_nearest_point(one, one, 10242, 20480, one, one, one, 16, None)
    assert rc != 0 and b'workspace' in lib.geobi_last_error()


def test_slice_count_follows_the_sizes():
    """Small query sets are cut into more target slices than large ones (the chip is filled either way), never more
    than there are target tiles."""
    from geobi_gnn_amd import _lib as L
    lib = L.lib()
    for tri in (0, 1):
        s_small, s_big = lib.geobi_nearest_slices(1000, 151380, tri), lib.geobi_nearest_slices(75692, 151380, tri)
        assert s_small > s_big >= 1
        assert lib.geobi_nearest_slices(1000, 1, tri) == 1
