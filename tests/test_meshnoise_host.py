"""Host side of the synthetic mesh noise: the numpy Philox4x32-10 model against its known answers, the argument checks
of the entry point (they come before anything touches the device), the parsers of the `noise` command and of the new
`train` flags, stream ids and file names."""
import ctypes
import re

import numpy as np
import pytest

import noise_model as M


# counter, key -> output: the Random123 known-answer vectors of philox4x32-10
KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_numpy_philox_reproduces_the_known_answers():
    for counter, key, want in KNOWN:
        got = tuple(int(w[0]) for w in M.philox4x32_10(counter, key))
        assert got == want, (['%08x' % g for g in got], ['%08x' % w for w in want])
    # vectorised over the first counter word: row i of a batch equals the single call
    batch = M.philox4x32_10((np.arange(5), 7, 9, 1), (3, 4))
    for i in range(5):
        assert [int(w[i]) for w in batch] == [int(w[0]) for w in M.philox4x32_10((i, 7, 9, 1), (3, 4))]


def test_word_to_uniform_is_exact_in_fp32_and_open():
    w = np.array([0, 1, 511, 512, 0xffffffff, 0x80000000], dtype=np.uint64)
    u = M.uniform(w)
    assert (u > 0).all() and (u < 1).all()
    assert (u.astype(np.float32).astype(np.float64) == u).all()          # 24 significant bits at most
    assert u[0] == 2.0 ** -24 and u[4] == 1.0 - 2.0 ** -24
    assert -2.0 * np.log(u.min()) <= 33.3


def test_model_key_counter_layout():
    """key = (seed & 0xffffffff, seed >> 32), counter = (v, stream_id, draw, block)."""
    seed = (0x299f31d0 << 32) | 0xa4093822
    words = M.words_of([0x243f6a88], seed, 0x85a308d3, 0x13198a2e, 0x03707344)
    assert tuple(int(w[0]) for w in words) == KNOWN[2][2]


def test_header_declares_the_entry_point():
    from geobi_gnn_amd import _lib
    protos = _lib.parse_header()
    assert 'geobi_mesh_noise' in protos
    restype, argtypes, argnames = protos['geobi_mesh_noise']
    assert argnames == ['points', 'vnormal', 'V', 'sigma', 'kind', 'direction', 'fraction', 'seed', 'stream_id', 'draw',
                        'out', 'stream']
    assert argtypes[7] is ctypes.c_uint64 and argtypes[8] is ctypes.c_uint32 and argtypes[9] is ctypes.c_uint32
    src = open(_lib.HEADER).read()
    block = src[src.index('synthetic mesh noise'):src.index('int geobi_mesh_noise')]
    assert 'README.md:7' in block and re.search(r'no call site', block, flags=re.I)


def test_entry_point_checks_its_arguments_before_the_device():
    from geobi_gnn_amd import _lib as L
    lib = L.lib()
    one = ctypes.c_void_p(256)                     # never dereferenced: the checks come first
    call = lambda *a: lib.geobi_mesh_noise(*a)
    assert call(one, one, 0, 0.1, 0, 0, 0.3, 1, 0, 0, one, None) == 0             # V == 0: a no-op
    assert call(one, one, (1 << 24), 0.1, 0, 0, 0.3, 1, 0, 0, one, None) != 0
    assert b'GEOBI_MAX_NODES' in lib.geobi_last_error()
    assert call(one, one, -1, 0.1, 0, 0, 0.3, 1, 0, 0, one, None) != 0
    assert call(one, None, 10, 0.1, 0, 0, 0.3, 1, 0, 0, one, None) != 0
    assert b'vnormal' in lib.geobi_last_error()
    assert call(one, one, 10, 0.1, 2, 0, 0.3, 1, 0, 0, one, None) != 0 and b'kind' in lib.geobi_last_error()
    assert call(one, one, 10, 0.1, 0, 2, 0.3, 1, 0, 0, one, None) != 0 and b'direction' in lib.geobi_last_error()
    assert call(one, one, 10, 0.1, 1, 0, 1.5, 1, 0, 0, one, None) != 0 and b'fraction' in lib.geobi_last_error()
    assert call(one, one, 10, -0.1, 0, 0, 0.3, 1, 0, 0, one, None) != 0 and b'sigma' in lib.geobi_last_error()
    assert call(None, one, 10, 0.1, 0, 0, 0.3, 1, 0, 0, one, None) != 0
    assert call(one, one, 10, 0.1, 0, 0, 0.3, 1, 0, 0, None, None) != 0


def test_noise_parser_defaults_and_rejections():
    from geobi_gnn_amd.__main__ import build_parser, noise
    ap = build_parser()
    opt = ap.parse_args(['noise', '--data_dir', 'D'])
    assert opt.fn is noise
    assert opt.levels == [0.1, 0.2, 0.3] and opt.kind == 'gaussian' and opt.direction == 'normal'
    assert opt.fraction == 0.3 and opt.seed == 1 and opt.out_dir == '' and opt.gpu == -1
    opt = ap.parse_args(['noise', '--data_dir', 'D', '--levels', '0.05, 0.4', '--kind', 'impulsive', '--direction', 'random',
                         '--fraction', '0.5', '--seed', '9', '--out_dir', 'O'])
    assert opt.levels == [0.05, 0.4] and (opt.kind, opt.direction, opt.fraction, opt.seed, opt.out_dir) == \
        ('impulsive', 'random', 0.5, 9, 'O')
    for bad in ('', '0.1,,0.2', 'a', '0.1;0.2', '-0.1', '0.1,nan', 'inf'):
        with pytest.raises(SystemExit):
            ap.parse_args(['noise', '--data_dir', 'D', '--levels', bad])
    for flag, bad in (('--kind', 'salt'), ('--direction', 'tangent')):
        with pytest.raises(SystemExit):
            ap.parse_args(['noise', '--data_dir', 'D', flag, bad])
    with pytest.raises(SystemExit):
        ap.parse_args(['noise'])                                   # --data_dir is required


def test_train_noise_flags():
    from geobi_gnn_amd.__main__ import build_parser
    ap = build_parser()
    opt = ap.parse_args(['train', '--data_dir', 'D', '--out_dir', 'O'])
    assert opt.noise_levels is None and opt.renoise_every == 0
    assert (opt.noise_kind, opt.noise_direction, opt.noise_fraction) == ('gaussian', 'normal', 0.3)
    opt = ap.parse_args(['train', '--data_dir', 'D', '--out_dir', 'O', '--noise_levels', '0.1,0.2', '--renoise_every', '3',
                         '--noise_kind', 'impulsive', '--noise_direction', 'random', '--noise_fraction', '0.25'])
    assert opt.noise_levels == [0.1, 0.2] and opt.renoise_every == 3
    assert (opt.noise_kind, opt.noise_direction, opt.noise_fraction) == ('impulsive', 'random', 0.25)
    assert isinstance(opt.noise_levels, list)                      # lists go into the params file, tuples would not
    with pytest.raises(SystemExit):
        ap.parse_args(['train', '--data_dir', 'D', '--out_dir', 'O', '--noise_levels', '0.1,x'])


def test_stream_ids_file_names_and_options():
    import zlib
    from geobi_gnn_amd import meshnoise
    assert meshnoise.stream_of('ball') == zlib.crc32(b'ball')
    assert meshnoise.stream_of('ball') != meshnoise.stream_of('ball2')
    assert 0 <= meshnoise.stream_of('ball') < 2 ** 32
    assert [meshnoise.noisy_name('ball', k) + '.obj' for k in (1, 2, 3)] == ['ball_n1.obj', 'ball_n2.obj', 'ball_n3.obj']
    nz = meshnoise.NoiseOptions.of({'levels': (0.1, 0.2), 'seed': 5})
    assert nz.levels == (0.1, 0.2) and nz.kind == 'gaussian' and nz.direction == 'normal' and nz.fraction == 0.3
    # round d of level k: draws of different rounds never collide
    assert [nz.draw_index(k, d) for d in (0, 1, 2) for k in (1, 2)] == [1, 2, 3, 4, 5, 6]
    assert meshnoise.NoiseOptions.of(None) is None and meshnoise.NoiseOptions.of(nz) is nz
    for kw in ({'levels': ()}, {'levels': (-0.1,)}, {'kind': 'salt'}, {'direction': 'up'}, {'fraction': 1.5},
               {'fraction': -0.1}):
        with pytest.raises(ValueError):
            meshnoise.NoiseOptions(**kw)
    for text in ('', '0.1,,0.2', 'a', '-1'):
        with pytest.raises(ValueError):
            meshnoise.parse_levels(text)
    assert meshnoise.parse_levels('0.1, 0.2') == (0.1, 0.2)
