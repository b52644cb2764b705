"""What the network path's entry points refuse when handed nothing: a table that pins their first checks.

Each of the 65 entry points below is defined in the unit that implements it, its argument checks ahead of
the launch.  No kernel result depends on those checks, so they are pinned here: each entry point is called three times
with every pointer NULL and every float 0 --

    one     every integer 1
    minus   every integer -1
    big     every int64_t count 2^24 (one above GEOBI_MAX_NODES), the other integers 1

-- and the outcome is compared with tests/entry_refusals.json: the returned value of a size_t function (and of
geobi_feast_ldz, an int that is a stride); (rc, text of geobi_last_error()) where an int function refuses its
arguments; null where it does not (it returned 0, or it passed its checks and then failed in a HIP call, which its
message shows by naming a `.hip:` source line); {"signal": n} where the call killed its process (three size queries
divide by a channel count of -1), which is why the calls run in forked children.  With every pointer NULL a function
stops at its first size or NULL check: what stands behind that one (empty-input, workspace and alignment refusals) is
not reached from here.  The table was recorded from the library of commit e35f94c, where capi.hip still forwarded these
65 to launchers in other units, by running this file as a script with GEOBI_LIB naming that library.

Skipped when torch.cuda.is_available(): without a device a call that passes its checks ends in HIP's "no ROCm-capable
device" error, with one it would launch kernels on NULL pointers.  The test never touches the GPU.
"""
import ctypes
import faulthandler
import json
import os

import pytest
import torch

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'entry_refusals.json')
MODES = ('one', 'minus', 'big')

MOVED = {
    'graph': ['geobi_expand_rowptr', 'geobi_concat32', 'geobi_gather_f32'],
    'feast': ['geobi_debug_exp_le0', 'geobi_feast_wpack_floats', 'geobi_feast_ldz', 'geobi_feast_fwd_ws_bytes',
              'geobi_feast_fwd', 'geobi_feast_bwd_ws_bytes', 'geobi_feast_bwd'],
    'feast_fused': ['geobi_set_tile_rows', 'geobi_set_rowpass_form', 'geobi_set_column_parts'],
    'head_fused': ['geobi_set_head_precision'],
    'gemm': ['geobi_gemm_nn', 'geobi_gemm_tn_ws_bytes', 'geobi_gemm_tn', 'geobi_debug_gemm_nn', 'geobi_debug_gemm_tn'],
    'geom': ['geobi_face_geom_fwd', 'geobi_face_geom_bwd', 'geobi_head_fwd', 'geobi_head_bwd_ws_bytes', 'geobi_head_bwd',
             'geobi_row_loss_ws_bytes', 'geobi_row_loss_fwd', 'geobi_row_loss_bwd', 'geobi_adam_step',
             'geobi_rotate_parts', 'geobi_update_position_ws_bytes', 'geobi_update_position2'],
    'scan': ['geobi_set_scan_lookback', 'geobi_debug_scan_ws_bytes', 'geobi_debug_scan_exclusive_i32',
             'geobi_debug_scan_exclusive_i32_pair'],
    'match': ['geobi_edge_weight_t10', 'geobi_edge_weight_att', 'geobi_match_ws_bytes', 'geobi_match_heavy_edge',
              'geobi_set_match_round_cap', 'geobi_set_match_scanfree', 'geobi_match_coarsen_ws_bytes',
              'geobi_match_coarsen', 'geobi_debug_match_coarsen_rowinfo', 'geobi_relabel_ws_bytes',
              'geobi_relabel_compact'],
    'segment': ['geobi_segment_csr_ws_bytes', 'geobi_segment_csr', 'geobi_segment_pairs_ws_bytes',
                'geobi_segment_csr_pairs', 'geobi_segment_csr_compose', 'geobi_segment_max_fwd', 'geobi_segment_max_bwd',
                'geobi_debug_segment_max2_fwd', 'geobi_debug_segment_max2_bwd', 'geobi_debug_segment_sum2',
                'geobi_segment_sum', 'geobi_segment_mean_bwd', 'geobi_gather_rows'],
    'pool': ['geobi_pool_edge_rows_ws_bytes', 'geobi_pool_edge_rows', 'geobi_debug_pool_edge_rows_onepass_ws_bytes',
             'geobi_debug_pool_edge_rows_onepass', 'geobi_pool_edge_ws_bytes', 'geobi_pool_edge'],
}
NAMES = [n for unit in MOVED.values() for n in unit]


def _args(argtypes, mode):
    out = []
    for t in argtypes:
        if t is ctypes.c_void_p or not issubclass(t, ctypes._SimpleCData):
            out.append(None)                                   # every pointer NULL (host out-parameters included)
        elif t in (ctypes.c_float, ctypes.c_double):
            out.append(0.0)
        elif mode == 'minus':
            out.append(-1)
        else:
            out.append(1 << 24 if mode == 'big' and t is ctypes.c_int64 else 1)
    return out


def _outcome(lib, name, restype, args):
    # the error text is per thread and survives a call that sets none: plant a known one first, so that a non-zero int
    # that left it alone (geobi_feast_ldz returns a row stride) reads as the value it is, not as a refusal
    lib.geobi_read_i32(None, 1, None, None)
    planted = lib.geobi_last_error()
    ret = getattr(lib, name)(*args)
    text = lib.geobi_last_error()
    if restype is ctypes.c_size_t or (ret != 0 and text == planted):
        return int(ret)                                        # a value
    if ret == 0 or b'.hip:' in text:
        return None                                            # no refusal by an argument check
    return [int(ret), text.decode()]


def observe():
    """{name: {mode: value | [rc, text] | None | {'signal': n}}} of the loaded library.  The calls of an entry point run in
    a forked child: a size query takes its nonsense arguments as they are (geobi_feast_bwd_ws_bytes, geobi_gemm_tn_ws_bytes
    and geobi_head_bwd_ws_bytes die of SIGFPE on -1 channels; a fresh child then takes the modes behind the fatal
    one), and a hook that is set stays set in the child only."""
    from geobi_gnn_amd import _lib
    lib, protos = _lib.lib(), _lib.parse_header()
    table = {}
    for name in NAMES:
        restype, argtypes, _ = protos[name]
        row = table[name] = {}
        todo = list(MODES)
        while todo:
            r, w = os.pipe()
            pid = os.fork()
            if pid == 0:
                code = 1                                       # an exception in the child: the parent fails on it
                try:
                    faulthandler.disable()
                    for mode in todo:
                        os.write(w, (json.dumps(_outcome(lib, name, restype, _args(argtypes, mode))) + '\n').encode())
                    code = 0
                finally:
                    os._exit(code)
            os.close(w)
            with os.fdopen(r, 'rb') as f:
                done = [json.loads(line) for line in f.read().splitlines()]
            status = os.waitpid(pid, 0)[1]
            if os.WIFSIGNALED(status):
                done.append({'signal': os.WTERMSIG(status)})
            assert done and (os.WIFSIGNALED(status) or os.WEXITSTATUS(status) == 0), (name, todo, status)
            row.update(zip(todo, done))
            todo = todo[len(done):]
    return table


def test_moved_list_is_the_65():
    assert len(NAMES) == 65 and len(set(NAMES)) == 65
    from geobi_gnn_amd import _lib
    assert set(NAMES) <= set(_lib.parse_header())


@pytest.mark.skipif(torch.cuda.is_available(), reason='with a device the calls that pass their checks would launch on NULL')
def test_refusals_match_the_recorded_table():
    want = json.load(open(TABLE))
    assert sorted(want) == sorted(NAMES)
    got = observe()
    for name in NAMES:
        for mode in MODES:
            assert got[name][mode] == want[name][mode], (name, mode, got[name][mode], want[name][mode])


if __name__ == '__main__':       # GEOBI_LIB=<library to record> python tests/test_entry_refusals_host.py
    assert not torch.cuda.is_available()
    with open(TABLE, 'w') as f:
        json.dump(observe(), f, indent=1, sort_keys=True)
        f.write('\n')
