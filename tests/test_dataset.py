"""Host side of training from OBJ folders: file pairing (dataset.file_pairs), the rotation draws
(RandomRotate.matrices), the argument checks of geobi_rotate_parts and the `train` sub-command's parser.  No GPU."""
import ctypes
import os

import numpy as np
import pytest


def _base(pairs):
    return [(os.path.basename(n), os.path.basename(o)) for n, o in pairs]


def _tree(tmp_path, originals, noisy, split='train'):
    for sub, names in (('original', originals), ('noisy', noisy)):
        (tmp_path / split / sub).mkdir(parents=True, exist_ok=True)
        for name in names:
            (tmp_path / split / sub / name).write_text('')


def test_file_pairs_sorted_fallback_matches_the_denoise_list(tmp_path):
    """Without a list: sorted original/*.obj, each with its sorted noisy/NAME_n*.obj -- `ab` beside `a` is not picked
    up by `a`, a noisy file without the `_n` infix is ignored; the pairs are those `denoise` would make of the folder."""
    from geobi_gnn_amd.dataset import file_pairs
    from geobi_gnn_amd.__main__ import _denoise_list
    _tree(tmp_path, ('b.obj', 'a.obj', 'ab.obj', 'w[1].obj'),
          ('a_n2.obj', 'a_n1.obj', 'ab_n1.obj', 'a_x.obj', 'b_n3.obj', 'w[1]_n1.obj', 'w1_n1.obj'))
    pairs = file_pairs(str(tmp_path), 'train')
    assert _base(pairs) == [('a_n1.obj', 'a.obj'), ('a_n2.obj', 'a.obj'), ('ab_n1.obj', 'ab.obj'), ('b_n3.obj', 'b.obj'),
                            ('w[1]_n1.obj', 'w[1].obj')]
    assert pairs == _denoise_list(str(tmp_path / 'train'))


def test_file_pairs_list_order_and_missing_names(tmp_path, capsys):
    """With a list: its order, blank lines dropped; a name without an original or without a noisy file is reported on
    stderr and skipped."""
    from geobi_gnn_amd.dataset import file_pairs
    _tree(tmp_path, ('a.obj', 'b.obj', 'c.obj', 'lonely.obj'), ('a_n1.obj', 'b_n1.obj', 'b_n2.obj', 'c_n1.obj', 'ghost_n1.obj'))
    (tmp_path / 'train_list.txt').write_text('c\n\nghost\n  b  \nlonely\n\na\n')
    pairs = file_pairs(str(tmp_path), 'train', 'train_list.txt')
    assert _base(pairs) == [('c_n1.obj', 'c.obj'), ('b_n1.obj', 'b.obj'), ('b_n2.obj', 'b.obj'), ('a_n1.obj', 'a.obj')]
    err = capsys.readouterr().err
    assert 'ghost' in err and 'lonely' in err and 'skipped' in err


def test_file_pairs_refuses_an_empty_result(tmp_path):
    from geobi_gnn_amd.dataset import file_pairs
    _tree(tmp_path, ('a.obj',), ('b_n1.obj',))
    with pytest.raises(ValueError):
        file_pairs(str(tmp_path), 'train')
    (tmp_path / 'l.txt').write_text('\n\n')
    with pytest.raises(ValueError):
        file_pairs(str(tmp_path), 'train', 'l.txt')
    with pytest.raises(ValueError):
        file_pairs(str(tmp_path), 'test')


@pytest.mark.parametrize('z_rotated', [False, True])
def test_rotation_matrices_are_sequential_draws(z_rotated):
    """matrices(k) = k matrix() calls of an equally seeded generator, bit for bit; each is a rotation."""
    from geobi_gnn_amd.data import RandomRotate
    a = RandomRotate(z_rotated=z_rotated, rng=np.random.default_rng(123))
    b = RandomRotate(z_rotated=z_rotated, rng=np.random.default_rng(123))
    got = a.matrices(5)
    want = np.stack([b.matrix() for _ in range(5)])
    assert got.shape == (5, 3, 3) and got.dtype == np.float64
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(a.matrices(2), np.stack([b.matrix(), b.matrix()]))      # the generator moved on alike
    for m in got:
        assert np.abs(m @ m.T - np.eye(3)).max() < 1e-14
        assert abs(np.linalg.det(m) - 1.0) < 1e-14
    assert not np.array_equal(got[0], got[1])
    assert a.matrices(0).shape == (0, 3, 3)


def test_rotate_parts_arguments_are_checked_before_any_launch():
    """geobi_rotate_parts: every bad call returns non-zero with a message naming the argument, before anything touches
    the device (the device pointers are never dereferenced: this runs without a GPU); n = 0 is a no-op."""
    from geobi_gnn_amd import _lib as L
    lib = L.lib()
    one = ctypes.c_void_p(256)
    R = (ctypes.c_float * 18)(*([1, 0, 0, 0, 1, 0, 0, 0, 1] * 2))

    def call(ptr, P, x=one, ldx=6, triples=2, n=None, part_ptr=True, mats=R):
        arr = (ctypes.c_int64 * len(ptr))(*ptr)
        rc = lib.geobi_rotate_parts(ctypes.cast(arr, ctypes.c_void_p) if part_ptr else None, P,
                                    ctypes.cast(mats, ctypes.c_void_p) if mats is not None else None, x, ldx, triples, None,
                                    None, ptr[-1] if n is None else n, None)
        return rc, lib.geobi_last_error() or b''

    rc, msg = call([0, 10], 0)
    assert rc != 0 and b'P = 0' in msg
    rc, msg = call([0, 10], -3)
    assert rc != 0 and b'P = -3' in msg
    rc, msg = call([0, 10], 1, part_ptr=False)
    assert rc != 0 and b'part_ptr' in msg
    rc, msg = call([0, 10], 1, mats=None)
    assert rc != 0 and b'R is NULL' in msg
    rc, msg = call([0, 7, 5, 10], 3)                       # decreasing
    assert rc != 0 and b'part_ptr' in msg
    rc, msg = call([1, 5, 10], 2)                          # does not start at 0
    assert rc != 0 and b'part_ptr' in msg
    rc, msg = call([0, 5, 10], 2, n=12)                    # does not end at n
    assert rc != 0 and b'part_ptr' in msg
    rc, msg = call([0, 5, 1 << 24], 2)
    assert rc != 0 and b'GEOBI_MAX_NODES' in msg
    rc, msg = call([0, 5, 10], 2, n=-1)
    assert rc != 0 and b'negative' in msg
    rc, msg = call([0, 5, 10], 2, ldx=5)
    assert rc != 0 and b'ldx' in msg
    rc, msg = call([0, 5, 10], 2, ldx=3, triples=-1)
    assert rc != 0 and b'x_triples' in msg
    rc, msg = call([0, 5, 10], 2, x=None)
    assert rc != 0 and b'x is NULL' in msg
    rc, _ = call([0, 0, 0], 2, x=None)                     # n == 0: nothing to do, nothing is launched
    assert rc == 0


def test_train_parser_defaults_are_the_references():
    """code/train_dual.py:39-82: --sub_size 20000, --filter_patch_count 100 and the flags of add_training_flags."""
    import argparse
    from geobi_gnn_amd import train_util
    from geobi_gnn_amd.__main__ import build_parser, train
    opt = build_parser().parse_args(['train', '--data_dir', 'd', '--out_dir', 'o'])
    assert opt.fn is train
    assert opt.sub_size == 20000 and opt.filter_patch_count == 100
    assert opt.rotate == 'full' and opt.seed is None and opt.gpu == -1 and opt.data_type == 'Synthetic'
    assert opt.no_cache is False and opt.no_predict is False and opt.model_path == ''
    ref = train_util.add_training_flags(argparse.ArgumentParser()).parse_args([])
    assert vars(ref) and all(getattr(opt, k) == v for k, v in vars(ref).items())
    assert (opt.max_epoch, opt.batch_size, opt.lr, opt.lr_sch, opt.lr_step, opt.optimizer) == (1000, 1, 0.001, 'lmd', [10], 'adam')
    with pytest.raises(SystemExit):
        build_parser().parse_args(['train', '--data_dir', 'd', '--out_dir', 'o', '--rotate', 'sideways'])
    # the two earlier commands parse as before
    d = build_parser().parse_args(['denoise', '--data_dir', 'd'])
    assert d.sub_size == 20000 and d.n_iter == 60 and d.model == ''


def test_train_refuses_more_than_one_process(tmp_path, monkeypatch):
    """WORLD_SIZE > 1: the command stops with a message that names the data-parallel tool, before any device call (there is
    no GPU here, and the message is not the missing-GPU one) and before anything is written."""
    from geobi_gnn_amd.__main__ import main
    monkeypatch.setenv('WORLD_SIZE', '2')
    out = tmp_path / 'out'
    with pytest.raises(SystemExit) as e:
        main(['train', '--data_dir', str(tmp_path), '--out_dir', str(out)])
    assert 'tools/train_synthetic.py' in str(e.value) and 'WORLD_SIZE' in str(e.value)
    assert not out.exists()
