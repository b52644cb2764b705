"""The command line of the winding-number tools (meshwind.py) without a GPU: the parser takes --outward,
--solid and --signed, and without them the options of clean, info and eval hand on exactly what they handed on before."""
import pytest

from geobi_gnn_amd import __main__ as main

TODAY = {'orient': False, 'min_component': 0, 'drop_intersecting': False}


def test_the_flags_parse():
    opt = main.parse_args(['clean', '--data_dir', 'd', '--outward'])
    assert opt.outward is True and main._topo_args(opt) == dict(TODAY, outward=True)
    opt = main.parse_args(['clean', '--data_dir', 'd', '--outward', '--orient', '--min_component', '3'])
    assert main._topo_args(opt) == {'orient': True, 'min_component': 3, 'drop_intersecting': False, 'outward': True}
    opt = main.parse_args(['denoise', '--data_dir', 'd', '--clean', '--outward'])
    assert main._topo_args(opt) == dict(TODAY, outward=True)
    assert main.parse_args(['info', '--data_dir', 'd', '--solid']).solid is True
    opt = main.parse_args(['eval', '--result_dir', 'r', '--original_dir', 'o', '--free', '--signed'])
    assert opt.signed is True and opt.free is True


def test_without_the_flags_nothing_new_is_handed_on():
    for argv in (['clean', '--data_dir', 'd'], ['denoise', '--data_dir', 'd', '--clean'], ['denoise', '--data_dir', 'd']):
        opt = main.parse_args(argv)
        assert not hasattr(opt, 'outward') and main._topo_args(opt) == TODAY
    opt = main.parse_args(['clean', '--data_dir', 'd', '--orient'])
    assert main._topo_args(opt) == dict(TODAY, orient=True)
    for argv in (['info', '--data_dir', 'd'], ['eval', '--result_dir', 'r', '--original_dir', 'o']):
        opt = main.parse_args(argv)
        assert not hasattr(opt, 'outward') and main._topo_args(opt) == TODAY
    assert main.parse_args(['info', '--data_dir', 'd']).solid is False
    assert main.parse_args(['eval', '--result_dir', 'r', '--original_dir', 'o', '--free']).signed is False


def test_the_flags_need_what_they_build_on():
    with pytest.raises(SystemExit):
        main.parse_args(['denoise', '--data_dir', 'd', '--outward'])                    # as the other clean flags: with --clean
    with pytest.raises(SystemExit):
        main.parse_args(['eval', '--result_dir', 'r', '--original_dir', 'o', '--signed'])   # with --free
