"""The folder rules of the mesh commands (geobi_gnn_amd/folders.py) on the host: the two walks driven by a tool made of
numpy callables -- ``plan`` appends the centroid as a vertex and one face, ``apply`` does the same to the paired array -- on
meshes of four to six vertices.  What is pinned: the files written, the order of the printed lines, both trailers and the
return values, with and without failures; and the one definition of the library's row limit."""
import os
import re
import types

import numpy as np
import pytest

from geobi_gnn_amd import folders, meshio
from geobi_gnn_amd._lib import GeobiError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TETRA = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32),
         np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int32))
PYRAMID = (np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1]], dtype=np.float32),
           np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], dtype=np.int32))


def _with_centroid(points):
    return np.concatenate([points, points.mean(axis=0, keepdims=True)]).astype(np.float32)


def _plan(points, faces, path):
    return {'points': _with_centroid(points), 'faces': np.concatenate([faces, [[0, 1, points.shape[0]]]]).astype(np.int32)}


def _mesh_of(result):
    return result['points'], result['faces']


def _apply(result, noisy_points):
    return _with_centroid(noisy_points)


def _line(result, V, F, out_file):
    return "V: %d -> %d,  F: %d -> %d,  '%s'" % (V, result['points'].shape[0], F, result['faces'].shape[0],
                                                  os.path.basename(out_file))


def _write(path, mesh, shift=0.0):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    meshio.write_obj(path, (mesh[0] + np.float32(shift)).astype(np.float32), mesh[1])


def _junk(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write('v 0 0 nothing\n')


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root).replace(os.sep, '/') for d, _, fs in os.walk(root) for f in fs)


def _dirs(root):
    return sorted(os.path.relpath(os.path.join(d, s), root).replace(os.sep, '/') for d, ss, _ in os.walk(root) for s in ss)


def _paired(data, out, plan=_plan, apply=_apply):
    return folders.paired_walk(str(data), str(out), 'Tool, mode 1', plan, _mesh_of, _line, apply)


def _names(stdout):
    """the file names of the printed lines, in order, after the header and before the end line"""
    lines = stdout.split('\n')
    assert lines[0] == '' and lines[1].startswith('Tool, mode 1, ') and lines[2] == ''
    assert lines[-3:] == ['', '--- end ---', '']
    return [re.search(r"'([^']*)'$", l).group(1) for l in lines[3:-3]]


# ------------------------------------------------------------------------------------------- nothing goes wrong
def test_paired_walk_on_a_flat_folder(tmp_path, capsys):
    data, out = tmp_path / 'data', tmp_path / 'out'
    _write(str(data / 'b.obj'), PYRAMID)
    _write(str(data / 'a.obj'), TETRA)
    assert _paired(data, out) == 0
    io = capsys.readouterr()
    assert io.out == ("\nTool, mode 1, 2 files ...\n\nV: 4 -> 5,  F: 4 -> 5,  'a.obj'\nV: 5 -> 6,  F: 4 -> 5,  'b.obj'\n"
                      "\n--- end ---\n") and io.err == ''
    assert _tree(str(out)) == ['a.obj', 'b.obj'] and _dirs(str(out)) == []
    points, faces = meshio.read_obj(str(out / 'a.obj'))
    assert np.array_equal(points, _with_centroid(TETRA[0])) and np.array_equal(faces[-1], [0, 1, 4])


def test_paired_walk_carries_the_noisy_files_of_equal_size(tmp_path, capsys):
    data, out = tmp_path / 'data', tmp_path / 'out'
    _write(str(data / 'original' / 'b.obj'), PYRAMID)
    _write(str(data / 'original' / 'a.obj'), TETRA)
    _write(str(data / 'noisy' / 'a_n1.obj'), TETRA, 0.25)
    _write(str(data / 'noisy' / 'a_n2.obj'), PYRAMID)                  # another size: skipped, and the walk goes on
    _write(str(data / 'noisy' / 'a_n3.obj'), TETRA, 0.5)
    _write(str(data / 'a.obj'), PYRAMID)                               # beside original/: not listed
    assert _paired(data, out) == 1
    io = capsys.readouterr()
    assert _names(io.out) == ['a.obj', 'a_n1.obj', 'a_n3.obj', 'b.obj'] and '4 -> 5' in io.out.split('\n')[4]
    assert io.out.startswith('\nTool, mode 1, 2 files ...\n')
    noisy, original = str(data / 'noisy' / 'a_n2.obj'), str(data / 'original' / 'a.obj')
    assert io.err == ('skipped: %s (V = 5, F = 4) and its original %s (V = 4, F = 4) differ in size\n1 files skipped\n'
                      % (noisy, original))
    assert _tree(str(out)) == ['noisy/a_n1.obj', 'noisy/a_n3.obj', 'original/a.obj', 'original/b.obj']
    points, faces = meshio.read_obj(str(out / 'noisy' / 'a_n3.obj'))
    assert np.array_equal(points, _with_centroid(TETRA[0] + np.float32(0.5)))
    assert np.array_equal(faces, meshio.read_obj(str(out / 'original' / 'a.obj'))[1])


def test_paired_walk_without_a_noisy_folder_still_makes_one(tmp_path, capsys):
    data, out = tmp_path / 'data', tmp_path / 'out'
    _write(str(data / 'original' / 'a.obj'), TETRA)
    assert _paired(data, out) == 0
    io = capsys.readouterr()
    assert _names(io.out) == ['a.obj'] and io.err == ''
    assert _tree(str(out)) == ['original/a.obj'] and _dirs(str(out)) == ['noisy', 'original']


def test_names_are_taken_literally(tmp_path, capsys):
    data, out = tmp_path / 'd[1]', tmp_path / 'out'
    _write(str(data / 'original' / 'p[x].obj'), TETRA)
    _write(str(data / 'noisy' / 'p[x]_n1.obj'), TETRA, 0.25)
    _write(str(data / 'noisy' / 'px_n1.obj'), TETRA)                   # what the character class [x] would match
    _write(str(tmp_path / 'd1' / 'original' / 'q.obj'), TETRA)         # what the character class [1] would match
    assert _paired(data, out) == 0
    assert _names(capsys.readouterr().out) == ['p[x].obj', 'p[x]_n1.obj']
    assert _tree(str(out)) == ['noisy/p[x]_n1.obj', 'original/p[x].obj']


def test_listings(tmp_path):
    d = tmp_path / 'd'
    for name in ('box.obj', 'box_n2.obj', 'box_n1.obj', 'box_new_n1.obj', 'box_r.obj', 'boxy_n1.obj', 'box_n1.txt'):
        _write(str(d / name), TETRA)
    full = lambda *names: [str(d / n) for n in names]
    assert folders.obj_files(str(d)) == full('box.obj', 'box_n1.obj', 'box_n2.obj', 'box_new_n1.obj', 'box_r.obj', 'boxy_n1.obj')
    assert folders.obj_files(str(d), 'box_n?') == full('box_n1.obj', 'box_n2.obj')
    # a stem that continues another with _n is matched too: known, and kept
    assert folders.noisy_of(str(d), 'box') == full('box_n1.obj', 'box_n2.obj', 'box_new_n1.obj')
    assert folders.variants_of(str(d), 'box') == full('box_n1.obj', 'box_n2.obj', 'box_new_n1.obj', 'box_r.obj')
    assert folders.stem_of(str(d / 'box_n1.obj')) == 'box_n1'
    assert folders.obj_files(str(tmp_path / 'none')) == []
    # DIR/original if it exists, else DIR
    assert folders.originals(str(d)) == (folders.obj_files(str(d)), False)
    _write(str(d / 'original' / 'one.obj'), TETRA)
    assert folders.originals(str(d)) == ([str(d / 'original' / 'one.obj')], True)


# ---------------------------------------------------------------------------------------------------- failures
def test_an_unreadable_original_between_two_good_ones(tmp_path, capsys):
    data, out = tmp_path / 'data', tmp_path / 'out'
    _write(str(data / 'original' / 'a.obj'), TETRA)
    _junk(str(data / 'original' / 'b.obj'))
    _write(str(data / 'original' / 'c.obj'), PYRAMID)
    _write(str(data / 'noisy' / 'b_n1.obj'), TETRA)                    # its original fails: never read
    _write(str(data / 'noisy' / 'c_n1.obj'), PYRAMID)
    assert _paired(data, out) == 1
    io = capsys.readouterr()
    assert _names(io.out) == ['a.obj', 'c.obj', 'c_n1.obj']
    err = io.err.split('\n')
    assert len(err) == 3 and err[0].startswith('skipped: ') and 'b.obj' in err[0] and err[1:] == ['1 files skipped', '']
    assert _tree(str(out)) == ['noisy/c_n1.obj', 'original/a.obj', 'original/c.obj']


@pytest.mark.parametrize('paired', [False, True])
def test_an_empty_folder_returns_1(tmp_path, capsys, paired):
    data, out = tmp_path / 'data', tmp_path / 'out'
    os.makedirs(str(data / 'original') if paired else str(data))
    assert _paired(data, out) == 1
    io = capsys.readouterr()
    assert io.out == '\nTool, mode 1, 0 files ...\n\n\n--- end ---\n' and io.err == ''
    assert _tree(str(out)) == [] and _dirs(str(out)) == (['noisy', 'original'] if paired else [])
    assert folders.walk([], None) == 1 and folders.walk([], None, of_total=False) == 1


def test_a_plan_that_raises_a_device_error_or_refuses(tmp_path, capsys):
    data, out = tmp_path / 'data', tmp_path / 'out'
    for name in ('a', 'b', 'c'):
        _write(str(data / 'original' / (name + '.obj')), TETRA)
        _write(str(data / 'noisy' / (name + '_n1.obj')), TETRA)

    def plan(points, faces, path):
        if path.endswith('a.obj'):
            raise GeobiError('the device said no')
        if path.endswith('b.obj'):          # the refusal of `clean`
            raise ValueError('%s: no faces left after cleaning' % path)
        return _plan(points, faces, path)

    assert _paired(data, out, plan=plan) == 1
    io = capsys.readouterr()
    assert _names(io.out) == ['c.obj', 'c_n1.obj']
    assert io.err == ('skipped: the device said no\nskipped: %s: no faces left after cleaning\n2 files skipped\n'
                      % str(data / 'original' / 'b.obj'))
    assert _tree(str(out)) == ['noisy/c_n1.obj', 'original/c.obj']


def test_a_device_error_on_a_paired_file_ends_its_stem_and_counts_once(tmp_path, capsys):
    data, out = tmp_path / 'data', tmp_path / 'out'
    _write(str(data / 'original' / 'a.obj'), TETRA)
    _write(str(data / 'noisy' / 'a_n1.obj'), TETRA, 0.25)
    _write(str(data / 'noisy' / 'a_n2.obj'), TETRA, 0.5)
    _write(str(data / 'original' / 'b.obj'), PYRAMID)
    _write(str(data / 'noisy' / 'b_n1.obj'), PYRAMID, 0.25)
    calls = []

    def apply(result, noisy_points):
        calls.append(noisy_points.shape[0])
        if len(calls) == 1:
            raise GeobiError('the device said no')
        return _apply(result, noisy_points)

    assert _paired(data, out, apply=apply) == 1
    io = capsys.readouterr()
    assert _names(io.out) == ['a.obj', 'b.obj', 'b_n1.obj'] and calls == [4, 5]          # a_n2 was never tried
    assert io.err == 'skipped: the device said no\n1 files skipped\n'
    assert _tree(str(out)) == ['noisy/b_n1.obj', 'original/a.obj', 'original/b.obj']


def test_an_inner_skip_stays_counted_when_the_stem_ends_later(tmp_path, capsys):
    data, out = tmp_path / 'data', tmp_path / 'out'
    _write(str(data / 'original' / 'a.obj'), TETRA)
    _write(str(data / 'noisy' / 'a_n1.obj'), PYRAMID)                  # another size: the inner handler
    _write(str(data / 'noisy' / 'a_n2.obj'), TETRA)                    # the device error: the outer handler
    _write(str(data / 'noisy' / 'a_n3.obj'), TETRA)

    def apply(result, noisy_points):
        raise GeobiError('the device said no')

    assert _paired(data, out, apply=apply) == 1
    io = capsys.readouterr()
    err = io.err.split('\n')
    assert 'differ in size' in err[0] and err[1:] == ['skipped: the device said no', '2 files skipped', '']
    assert _names(io.out) == ['a.obj'] and _tree(str(out)) == ['original/a.obj']


def test_a_paired_file_that_cannot_be_read_or_an_apply_that_refuses_is_an_inner_skip(tmp_path, capsys):
    data, out = tmp_path / 'data', tmp_path / 'out'
    _write(str(data / 'original' / 'a.obj'), TETRA)
    _junk(str(data / 'noisy' / 'a_n1.obj'))
    _write(str(data / 'noisy' / 'a_n2.obj'), TETRA, 0.25)
    _write(str(data / 'noisy' / 'a_n3.obj'), TETRA, 0.5)

    def apply(result, noisy_points):
        if noisy_points[0, 0] == 0.25:
            raise ValueError('apply: not this one')
        return _apply(result, noisy_points)

    assert _paired(data, out, apply=apply) == 1
    io = capsys.readouterr()
    assert _names(io.out) == ['a.obj', 'a_n3.obj']
    err = io.err.split('\n')
    assert 'a_n1.obj' in err[0] and err[1:] == ['skipped: apply: not this one', '2 files skipped', '']


@pytest.mark.parametrize('of_total, trailer', [(True, '2 of 4 files skipped\n'), (False, '2 files skipped\n')])
def test_flat_walk_counts_a_file_once_and_has_two_trailers(tmp_path, capsys, of_total, trailer):
    """a callable that writes several files (`noise`: one per level) and fails part-way counts as one file"""
    jobs = ['a', 'b', 'c', 'd']

    def one(job, skip):
        for k in (1, 2, 3):
            if (job, k) == ('b', 2):
                raise OSError('disk full at %s level %d' % (job, k))
            if (job, k) == ('c', 1):
                raise GeobiError('no device')
            meshio.write_obj(str(tmp_path / ('%s_n%d.obj' % (job, k))), *TETRA)
            print("'%s_n%d.obj'" % (job, k), flush=True)

    assert folders.walk(jobs, one, of_total=of_total) == 1
    io = capsys.readouterr()
    assert io.out == ''.join("'%s_n%d.obj'\n" % (j, k) for j, k in
                             [('a', 1), ('a', 2), ('a', 3), ('b', 1), ('d', 1), ('d', 2), ('d', 3)]) + '\n--- end ---\n'
    assert io.err == 'skipped: disk full at b level 2\nskipped: no device\n' + trailer
    assert _tree(str(tmp_path)) == ['a_n1.obj', 'a_n2.obj', 'a_n3.obj', 'b_n1.obj', 'd_n1.obj', 'd_n2.obj', 'd_n3.obj']
    assert folders.walk(jobs[:1], one, of_total=of_total) == 0
    io = capsys.readouterr()
    assert io.err == '' and io.out.endswith("'a_n3.obj'\n\n--- end ---\n")


def test_an_error_of_another_kind_is_not_swallowed(tmp_path):
    def one(job, skip):
        raise KeyError(job)

    with pytest.raises(KeyError):
        folders.walk(['a'], one)


# ------------------------------------------------------------------------------- what the commands hand to the walks
def test_clean_replays_its_maps_on_a_numpy_array_on_the_host():
    import torch
    from geobi_gnn_amd import meshclean
    cleaned = types.SimpleNamespace(vertex_map=torch.tensor([0, 0, 1, -1], dtype=torch.int32),
                                    vertex_src=torch.tensor([0, 2], dtype=torch.int32))
    noisy = np.arange(12, dtype=np.float32).reshape(4, 3)
    got = meshclean.apply(cleaned, noisy)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got, noisy[[0, 2]])
    with pytest.raises(ValueError, match='3 rows for a cleaning of 4'):
        meshclean.apply(cleaned, noisy[:3])


def test_fill_line_keeps_its_hint():
    from geobi_gnn_amd.__main__ import _fill_line
    counts = {'boundary_edges': 9, 'loops': 2, 'filled_loops': 1, 'skipped_loops': 1, 'blocked_vertices': 0, 'chain_edges': 0}
    filled = types.SimpleNamespace(points=np.zeros((9, 3)), faces=np.zeros((14, 3)), counts=counts)
    plain = _fill_line(filled, 8, 7, os.path.join('out', 'cup.obj'))
    assert plain == ("V:       8 ->       9,  F:       7 ->      14,  boundary: 9,  loops: 2,  filled: 1,  skipped: 1,  "
                     "blocked: 0,  chain: 0,  'cup.obj'")
    filled.counts = dict(counts, blocked_vertices=1, chain_edges=6)
    assert _fill_line(filled, 8, 7, 'tie.obj').endswith("blocked: 1,  chain: 6,  'tie.obj',  run clean --orient first")


# --------------------------------------------------------------------------------------------- one row limit
def test_max_nodes_is_the_headers():
    from geobi_gnn_amd import meshfill, meshin, meshremesh, meshsubdiv
    with open(os.path.join(ROOT, 'include', 'geobi_hip.h')) as fh:
        found = re.findall(r'^#define\s+GEOBI_MAX_NODES\s+\(\(1\s*<<\s*(\d+)\)\s*-\s*1\)', fh.read(), flags=re.M)
    assert len(found) == 1
    assert meshin.MAX_NODES == (1 << int(found[0])) - 1
    assert meshremesh.MAX_NODES == meshsubdiv.MAX_NODES == meshfill.MAX_NODES == meshin.MAX_NODES


def test_folders_names_no_device_module():
    with open(os.path.join(ROOT, 'geobi_gnn_amd', 'folders.py')) as fh:
        imports = [l for l in fh.read().split('\n') if re.match(r'\s*(import|from)\s', l)]
    assert imports == ['import glob', 'import os', 'import sys', 'from . import meshio', 'from ._lib import GeobiError']
