"""The geobi_set_* switches (include/geobi_hip.h) from the host: what each accepts, what it rejects and in which words.
Nothing here touches the device.  Every switch is left at its reset value."""
import os

import pytest


@pytest.fixture(scope='module')
def lib():
    from geobi_gnn_amd import _lib
    return _lib.lib()


def _rejected(lib, rc, text):
    assert rc != 0
    assert lib.geobi_last_error().decode() == text


def test_tile_rows_values_and_error(lib):
    for rows in (16, 32, 0):                       # 0: back to GEOBI_TILE16
        assert lib.geobi_set_tile_rows(rows) == 0
    for bad in (-16, 1, 8, 17, 64):
        _rejected(lib, lib.geobi_set_tile_rows(bad), 'tile rows: 16, 32 or 0 (environment default), got %d' % bad)
    assert lib.geobi_set_tile_rows(0) == 0


def test_rowpass_form_values_and_error(lib):
    for staged in (1, 0, -1):
        for chunked in (1, 0, -1):
            assert lib.geobi_set_rowpass_form(staged, chunked) == 0
    for staged, chunked in ((2, 0), (0, 2), (-2, -1), (-1, -2), (5, 7)):
        _rejected(lib, lib.geobi_set_rowpass_form(staged, chunked),
                  'row-pass form: staged and chunked64 are 1, 0 or -1 (default), got %d, %d' % (staged, chunked))
    assert lib.geobi_set_rowpass_form(-1, -1) == 0


def test_column_parts_values_and_error(lib):
    for parts in (1, 2, 0):                        # 0: chosen per launch
        assert lib.geobi_set_column_parts(parts) == 0
    for bad in (-1, 3, 16):
        _rejected(lib, lib.geobi_set_column_parts(bad), 'fused kernel column parts: 1, 2 or 0 (per launch), got %d' % bad)
    assert lib.geobi_set_column_parts(0) == 0


def test_head_precision_values_and_error(lib):
    env = os.environ.get('GEOBI_HEAD_BF16X3')
    start = 1 if env is not None and env.strip().lstrip('+-').isdigit() and int(env) != 0 else 0
    try:
        for mode in (1, 0):
            assert lib.geobi_set_head_precision(mode) == 0
        for bad in (-1, 2, 3):
            _rejected(lib, lib.geobi_set_head_precision(bad), 'head precision: 0 (fp32) or 1 (3 x bf16 split, six products)')
    finally:
        assert lib.geobi_set_head_precision(start) == 0


def test_hooks_without_a_range_return_ok(lib):
    assert lib.geobi_set_match_round_cap(3) == 0
    assert lib.geobi_set_match_round_cap(-3) == 0          # negatives clamp to 0: no cap
    for on in (1, 0, -1):                                  # -1: back to the environment
        assert lib.geobi_set_match_scanfree(on) == 0
        assert lib.geobi_set_scan_lookback(on) == 0
    assert lib.geobi_set_overlap(0) == 0
    assert lib.geobi_set_overlap(1) == 0
