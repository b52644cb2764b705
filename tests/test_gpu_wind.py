"""Winding numbers on the device (csrc/winding.hip: geobi_winding_number, geobi_part_solids, geobi_flip_faces), the Python
layer (meshwind) and its callers (meshclean.clean_mesh(outward=True), meshtopo.mesh_report(solid=True),
mesheval.eval_signed and the three commands) against tests/wind_model.py.

Tolerance of w: F * 2^-40 absolute.  A device term and a model term are the same fp64 expression in the same order up to
atan2, whose rounding moves a term by at most one quantum (2^-40) where the quotient lies across a rounding boundary; the
float error itself is five orders below (tests/test_wind_model_host.py).  Everything else is exact: integer depths, flags,
counts, the bits of a repeated query, the bits of |sd|.

Shapes: the octahedron spheres of 128 and 2 048 faces; F = 1, 255, 256, 257, 513, 2 048 (T = 256 faces per tile) and Q = 1,
255, 256, 257 (one query block is 256); Q = 1 against F = 1 283 (six slices, a last tile of 3); 5 000 queries for the slicing.

Seen on an MI355X: the largest |device - model| of w was 0 quanta in every test here (bound: F quanta); volume6 was
bit-equal to the model on the four shells of nested() (the order of the sum is stated, and the model follows it).  The
assertions stay the bounds, F * 2^-40 absolute and F * 2^-50 relative; the figures are printed."""
import os
import re

import numpy as np
import pytest
import torch

import test_gpu_workspace as W
import wind_model as M

pytestmark = pytest.mark.gpu

QUANTUM = 2.0 ** -40
F_EDGES = (1, 255, 256, 257, 513, 2048)
Q_EDGES = (1, M.QUERY_BLOCK - 1, M.QUERY_BLOCK, M.QUERY_BLOCK + 1)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda:0')


_CACHE = {}


def _big():
    """the 2 048-face sphere, its mean edge, 257 + 4 queries (radius 1 +- h/4 and 1 +- h/1024 in turn, then four at distance
    10) and the model's terms [261, 2048], computed once"""
    if 'big' not in _CACHE:
        verts, faces = M.sphere(4)
        h = M.mean_edge(verts, faces)
        d = M.directions(257, 41)
        offs = np.array([h / 4, -h / 4, h / 1024, -h / 1024])[np.arange(257) % 4]
        q = np.concatenate([d * (1.0 + offs[:, None]), 10.0 * M.directions(4, 42)]).astype(np.float32)
        _CACHE['big'] = (verts, faces, h, q, M.terms(q, verts, faces))
    return _CACHE['big']


def _w(dev, q, verts, faces, state=None):
    from geobi_gnn_amd import meshwind
    return meshwind.winding_number(q, verts, faces, state=state, device=dev).cpu().numpy()


def _model_w(terms):
    return terms.sum(axis=1).astype(np.float64) * QUANTUM


# ------------------------------------------------------------------------------------------------ the kernel
def test_tolerance_against_the_model(dev):
    verts, faces, h, q, terms = _big()
    got = _w(dev, q, verts, faces)
    assert got.dtype == np.float64 and got.shape == (q.shape[0],)
    worst = np.abs(got - _model_w(terms)).max()
    print('largest |device - model| = %.3g = %.1f quanta (bound %d quanta)' % (worst, worst / QUANTUM, faces.shape[0]))
    assert worst <= faces.shape[0] * QUANTUM
    # every value is a whole number of quanta
    assert np.array_equal(np.rint(got / QUANTUM) * QUANTUM, got)


def test_tile_block_and_slice_edges(dev):
    from geobi_gnn_amd import _lib as L
    verts, faces, h, q, terms = _big()
    worst = 0.0
    for F in F_EDGES:
        state = (np.arange(faces.shape[0]) < F).astype(np.int32)
        for Q in Q_EDGES:
            want = _model_w(terms[:Q, :F])
            by_state, by_table = _w(dev, q[:Q], verts, faces, state), _w(dev, q[:Q], verts, faces[:F])
            assert np.array_equal(by_state, by_table), (F, Q)
            worst = max(worst, np.abs(by_state - want).max())
            assert np.abs(by_state - want).max() <= F * QUANTUM, (F, Q)
    print('largest |device - model| over the edges = %.1f quanta' % (worst / QUANTUM))
    # one query, several slices and a ragged last tile
    assert L.lib().geobi_winding_number_slices(1, 1283) == 6 and L.lib().geobi_winding_number_slices(5000, 2048) > 1
    assert L.lib().geobi_winding_number_slices(1, 256) == 1 and L.lib().geobi_winding_number_slices(0, 5) == 0
    assert abs(_w(dev, q[:1], verts, faces[:1283])[0] - _model_w(terms[:1, :1283])[0]) <= 1283 * QUANTUM
    # nothing to do
    assert _w(dev, q[:0], verts, faces).shape == (0,)
    assert np.array_equal(_w(dev, q[:3], verts, faces[:0]), np.zeros(3))
    assert np.array_equal(_w(dev, q[:3], verts, faces, np.zeros(faces.shape[0], dtype=np.int32)), np.zeros(3))
    # the raw entry point with Q == 0 and with F == 0: no launch, no error
    w = torch.full((4,), 7.0, dtype=torch.float64, device=dev)
    some = torch.zeros((4, 3), dtype=torch.float32, device=dev)
    L.call('geobi_winding_number', L.ptr(some), L.ptr(some), None, None, None, None, 0, 4, 0, L.ptr(w), None, 0, L.stream())
    assert (w == 7.0).all()
    L.call('geobi_winding_number', L.ptr(some), L.ptr(some), None, None, None, None, 4, 4, 0, L.ptr(w), None, 0, L.stream())
    assert (w == 0.0).all()


def test_the_face_limit_is_refused_by_name(dev):
    from geobi_gnn_amd import _lib as L
    assert L.lib().geobi_winding_number_ws_bytes(1, (1 << 23) + 1) == 0 and L.lib().geobi_winding_number_ws_bytes(1, 1 << 23) > 0
    some = torch.zeros((4, 3), dtype=torch.float32, device=dev)
    w = torch.zeros(4, dtype=torch.float64, device=dev)
    with pytest.raises(L.GeobiError, match=r'geobi_winding_number: F = 8388609 faces \(at most 2\^23'):
        L.call('geobi_winding_number', L.ptr(some), L.ptr(some), L.ptr(some), None, None, None, 4, 4, (1 << 23) + 1, L.ptr(w),
               None, 0, L.stream())


def test_slicing_independence_bit_for_bit(dev):
    from geobi_gnn_amd import _lib as L
    verts, faces, h, q, _ = _big()
    rng = np.random.RandomState(3)
    batch = (M.directions(5000, 4) * rng.uniform(0.5, 1.5, (5000, 1))).astype(np.float32)
    batch[0] = batch[-1] = q[2]                                # h/1024 off the surface
    lib = L.lib()
    # 40 000 queries are cut into fewer slices than one query: another slicing, the same bits
    assert lib.geobi_winding_number_slices(1, 2048) == 8 and lib.geobi_winding_number_slices(40000, 2048) == 4
    alone = _w(dev, q[2:3], verts, faces)
    whole = _w(dev, batch, verts, faces)
    halves = np.concatenate([_w(dev, batch[:2500], verts, faces), _w(dev, batch[2500:], verts, faces)])
    assert alone.view(np.int64)[0] == whole.view(np.int64)[0] == whole.view(np.int64)[-1]
    assert np.array_equal(whole.view(np.int64), halves.view(np.int64))
    assert np.array_equal(whole.view(np.int64), _w(dev, batch, verts, faces).view(np.int64))
    many = _w(dev, np.tile(batch, (8, 1)), verts, faces)
    assert np.array_equal(many.view(np.int64), np.tile(whole, 8).view(np.int64))


def test_closed_surfaces_give_whole_depths(dev):
    from geobi_gnn_amd import meshwind
    verts, faces, h, q, terms = _big()
    r = np.linalg.norm(q.astype(np.float64), axis=1)
    got = _w(dev, q, verts, faces)
    off = np.abs(r - 1.0) >= 0.25 * h * (1 - 1e-6)
    assert off.sum() >= 128
    assert np.array_equal(np.rint(got[off]), (r[off] < 1.0).astype(np.float64))
    assert np.array_equal(np.rint(got[off]), np.rint(_model_w(terms)[off]))
    assert np.array_equal(meshwind.inside(q[off], verts, faces, device=dev).cpu().numpy(), r[off] < 1.0)
    # nested(): the depth is the number of shells a query is in
    nv, nf = M.nested()
    hn = min(M.mean_edge(*M.sphere(2, rad, c)) for rad, c in M.NESTED)
    rng = np.random.RandomState(8)
    p = np.concatenate([rng.uniform(-1.2, 1.2, (300, 3)), rng.uniform(-0.7, 0.7, (100, 3)) + [3, 0, 0],
                        [[0, 0, 0], [0.05, 0.02, -0.03], [0.1, 0, 0], [0.3, 0.1, 0.1]]]).astype(np.float32)
    dist = np.stack([np.linalg.norm(p.astype(np.float64) - np.array(c, dtype=np.float64), axis=1) - rad for rad, c in M.NESTED], 1)
    # a shell of 128 faces lies up to 0.08 of its radius inside its sphere: keep the queries well off that band
    clear = ((dist > 0.25 * hn) | (dist < -0.25 * hn - 0.08)).all(axis=1)
    assert clear.sum() >= 200
    depth = (dist[clear] < 0).sum(axis=1)
    assert set(depth.tolist()) == {0, 1, 2, 3}
    got = _w(dev, p[clear], nv, nf)
    assert np.array_equal(np.rint(got), depth) and np.array_equal(np.rint(M.winding(p[clear], nv, nf)), depth)
    assert np.array_equal(meshwind.inside(p[clear], nv, nf, device=dev).cpu().numpy(), depth > 0)


def test_the_det_zero_rule_on_the_integer_cube(dev):
    verts, faces = M.cube()
    q = np.array([[0.5, 0.5, 0.0], [0.5, 0.0, 0.0], [0.0, 0.0, 0.0], [0.5, 0.5, 0.5], [1.0, 1.0, 1.0], [0.25, 1.0, 0.5]],
                 dtype=np.float32)
    got, want = _w(dev, q, verts, faces), M.winding(q, verts, faces)
    assert np.abs(got - want).max() <= 12 * QUANTUM, (got, want)
    assert abs(got[0] - 0.5) <= 12 * QUANTUM                     # a face centre
    # reversed faces: the negated values, exactly
    back = _w(dev, q, verts, faces[:, [0, 2, 1]])
    assert np.array_equal(back, -got)


def test_parts_skip_the_own_component(dev):
    from geobi_gnn_amd import meshwind
    nv, nf = M.nested()
    label = np.repeat(np.arange(4) * 128, 128).astype(np.int32)
    roots = np.arange(4, dtype=np.int32) * 128
    q = nv[nf[roots, 0]]
    v, fv = torch.from_numpy(nv).to(dev), torch.from_numpy(nf).to(dev)
    w = meshwind.winding_device(torch.from_numpy(q).to(dev), v, fv, None, torch.from_numpy(label).to(dev),
                                torch.from_numpy(roots).to(dev)).cpu().numpy()
    want = M.winding(q, nv, nf, face_part=label, query_part=roots)
    assert np.abs(w - want).max() <= 384 * QUANTUM
    assert np.array_equal(np.rint(w), [0, 1, 2, 0]) and np.array_equal(np.rint(want), [0, 1, 2, 0])
    # without the parts the own shell adds about half a turn: the query is one of its corners
    assert (np.abs(_w(dev, q, nv, nf) - w) > 0.25).all()
    # one part array alone skips nothing
    lone = meshwind.winding_device(torch.from_numpy(q).to(dev), v, fv, None, torch.from_numpy(label).to(dev), None).cpu().numpy()
    assert np.array_equal(lone, _w(dev, q, nv, nf))


# ------------------------------------------------------------------------------------------------ the helpers
def test_part_solids(dev):
    from geobi_gnn_amd import meshwind
    nv, nf = M.nested()
    label = np.repeat(np.arange(4) * 128, 128).astype(np.int32)
    volume6, closed, consistent = (t.cpu().numpy() for t in meshwind.part_solids(nv, nf, label, device=dev))
    want = M.part_solids(nv, nf, label)
    roots = np.arange(4) * 128
    print('volume6 bit-equal to the model: %s' % np.array_equal(volume6.view(np.int64), want[0].view(np.int64)))
    assert (np.abs(volume6[roots] - want[0][roots]) <= 128 * 2.0 ** -50 * np.abs(want[0][roots])).all()
    assert (volume6[roots] > 0).all() and not np.delete(volume6, roots).any()
    assert np.array_equal(closed, want[1]) and np.array_equal(consistent, want[2]) and closed[roots].all()
    # reversed shells: the negated volumes, bit for bit
    back = meshwind.part_solids(nv, nf[:, [0, 2, 1]], label, device=dev)[0].cpu().numpy()
    assert np.array_equal(back[roots], -volume6[roots])
    # one face of the second shell removed by its state, and once from the table
    state = np.ones(512, dtype=np.int32)
    state[200] = 0
    lab = np.where(state == 1, label, -1).astype(np.int32)
    got = [t.cpu().numpy() for t in meshwind.part_solids(nv, nf, lab, state=state, device=dev)]
    want = M.part_solids(nv, nf, lab, state)
    assert [int(got[1][x]) for x in roots] == [1, 0, 1, 1] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert (np.abs(got[0][roots] - want[0][roots]) <= 128 * 2.0 ** -50 * np.abs(want[0][roots])).all()
    cut_f = np.delete(nf, 200, axis=0)
    cut_label = M.orient_labels(cut_f, V=nv.shape[0])[0]
    cut = [t.cpu().numpy() for t in meshwind.part_solids(nv, cut_f, cut_label, device=dev)]
    assert [int(cut[1][x]) for x in (0, 128, 255, 383)] == [1, 0, 1, 1]
    # one face of the first shell reversed: closed, not consistent
    odd = nf.copy()
    odd[5] = odd[5, [0, 2, 1]]
    got = [t.cpu().numpy() for t in meshwind.part_solids(nv, odd, label, device=dev)]
    assert [int(got[1][x]) for x in roots] == [1, 1, 1, 1] and [int(got[2][x]) for x in roots] == [0, 1, 1, 1]


def _scrambled(seed):
    """nested() with every shell reversed by coin and 20 % of all faces reversed on top"""
    nv, nf = M.nested()
    rng = np.random.RandomState(seed)
    shells = np.repeat(rng.rand(4) < 0.5, 128)
    return nv, M.flipped(M.flipped(nf, shells), rng.rand(512) < 0.2)


def _volume_signs(verts, faces, starts=(0, 128, 256, 384), n=128):
    return tuple(int(np.sign(M.signed_volume6(verts, faces[s:s + n]))) for s in starts)


@pytest.mark.parametrize('seed', [11, 12])
def test_orient_outward(dev, seed):
    from geobi_gnn_amd import meshtopo, meshwind
    nv, table = _scrambled(seed)
    want_f, want_flip, want_label, want_counts = M.orient_outward(nv, table)
    got = meshwind.orient_outward(nv, table, nv.shape[0], device=dev)
    faces = got.faces.cpu().numpy()
    assert meshtopo.mesh_report(nv, faces, weld_tol=None, device=dev)['inconsistent_edges'] == 0
    assert _volume_signs(nv, faces) == M.NESTED_SIGNS
    assert np.array_equal(faces, want_f) and np.array_equal(got.flip.cpu().numpy(), want_flip)
    assert np.array_equal(got.label.cpu().numpy(), want_label)
    assert {k: got.counts[k] for k in want_counts} == want_counts, (got.counts, want_counts)
    assert got.counts['closed_components'] == 4 and got.counts['open_components'] == 0 and got.counts['ambiguous'] == 0
    # the flips are the difference between the input and the output
    assert np.array_equal(got.flip.cpu().numpy() == 1, (faces != table).any(axis=1))
    # again: nothing turns, nothing flips
    again = meshwind.orient_outward(nv, faces, device=dev)
    assert again.counts['turned'] == 0 and again.counts['flipped'] == 0 and np.array_equal(again.faces.cpu().numpy(), faces)


def test_orient_outward_leaves_an_open_shell_alone(dev):
    from geobi_gnn_amd import meshtopo, meshwind
    nv, table = _scrambled(13)
    cut = np.delete(table, 130, axis=0)                           # the second shell loses a face
    got = meshwind.orient_outward(nv, cut, device=dev)
    want = M.orient_outward(nv, cut)
    plain = meshtopo.orient_faces(cut, nv.shape[0], device=dev)
    faces = got.faces.cpu().numpy()
    assert got.counts['closed_components'] == 3 and got.counts['open_components'] == 1
    assert {k: got.counts[k] for k in want[3]} == want[3]
    assert np.array_equal(faces, want[0])
    assert np.array_equal(faces[128:255], plain.faces.cpu().numpy()[128:255])        # as orient_device left it
    # the open shell hides nothing: the shell inside it is at depth 1 now and points into the void
    assert _volume_signs(nv, faces, (0, 255, 383)) == (1, -1, 1)
    # a state instead of a shorter table
    state = np.ones(512, dtype=np.int32)
    state[130] = 0
    by_state = meshwind.orient_outward(nv, table, state=state, device=dev)
    assert {k: by_state.counts[k] for k in want[3]} == want[3]
    assert np.array_equal(np.delete(by_state.faces.cpu().numpy(), 130, axis=0), faces)
    # nothing at all
    empty = meshwind.orient_outward(nv, np.zeros((0, 3), dtype=np.int32), device=dev)
    assert empty.faces.shape == (0, 3) and empty.counts['closed_components'] == 0


# ------------------------------------------------------------------------------------------------ the callers
@pytest.mark.parametrize('index', [None, 'grid'])
def test_signed_distance(dev, index):
    from geobi_gnn_amd import meshproject, meshwind
    verts, faces, h, q, terms = _big()
    sd, w = meshwind.signed_distance(q, verts, faces, index=index, device=dev)
    c = meshproject.closest(q, verts, faces, device=dev, index=index)
    sd, w, dist = sd.cpu().numpy(), w.cpu().numpy(), c.dist.cpu().numpy()
    assert sd.dtype == np.float32 and np.array_equal(np.abs(sd).view(np.int32), dist.view(np.int32))
    assert np.array_equal(sd < 0, _model_w(terms) > 0.5) and np.array_equal(w, _w(dev, q, verts, faces))
    r = np.linalg.norm(q.astype(np.float64), axis=1)
    off = np.abs(r - 1.0) >= 0.25 * h * (1 - 1e-6)
    assert np.array_equal(np.sign(sd[off]), np.sign(r[off] - 1.0))


def test_eval_signed(dev):
    from geobi_gnn_amd import mesheval
    verts, faces = _big()[:2]
    small = (verts.astype(np.float64) * 0.97).astype(np.float32)
    row = mesheval.eval_signed(small, faces, verts, faces, device=dev)
    assert row['signed'] < 0 and row['inside'] == 1.0 and row['num_v'] == verts.shape[0]
    assert -0.031 < row['signed'] < -0.025 and abs(row['signed_norm'] - row['signed'] / row['scale']) < 1e-12
    # float32 rounding of the scaled corners moves a coordinate by 2^-24 relative: 3 * 2^-24 = 1.8e-7 of the volume
    assert abs(row['volume_ratio'] - 0.97 ** 3) <= 1e-6, row['volume_ratio'] - 0.97 ** 3
    assert abs(row['volume_gt'] - M.signed_volume6(verts, faces) / 6.0) <= 1e-12
    grid = mesheval.eval_signed(small, faces, verts, faces, device=dev, index='grid')
    assert grid == row
    # the other way round: outside, positive
    out = mesheval.eval_signed(verts, faces, small, faces, device=dev)
    assert out['signed'] > 0 and out['inside'] == 0.0
    # a ground truth with an open component: its distances, no ratio
    assert mesheval.eval_signed(small, faces, verts, faces[1:], device=dev)['volume_ratio'] is None
    assert mesheval.eval_signed(small, faces, verts, faces[1:], device=dev)['signed'] < 0


def test_clean_mesh_outward(dev):
    from geobi_gnn_amd import meshclean
    nv, table = _scrambled(14)
    today = meshclean.clean_mesh(nv, table, device=dev, orient=True)
    flagless = meshclean.clean_mesh(nv, table, device=dev, orient=True, outward=False)
    assert W._flat(today, []) == W._flat(flagless, []) and set(today.topology) == {'orient_rounds', 'orient_components',
                                                                                'nonorientable', 'flipped'}
    assert W._flat(meshclean.clean_mesh(nv, table, device=dev), []) == W._flat(meshclean.clean_mesh(nv, table, device=dev, outward=False), [])
    got = meshclean.clean_mesh(nv, table, device=dev, outward=True)
    want_f, want_flip, _, want_counts = M.orient_outward(nv, table)
    assert got.faces.shape[0] == 512 and np.array_equal(got.faces.cpu().numpy(), want_f)
    assert _volume_signs(nv, got.faces.cpu().numpy()) == M.NESTED_SIGNS
    # the xor of the two stages: orient's flips, then the turned components
    turned_faces = (want_f != today.faces.cpu().numpy()).any(axis=1)
    flip = got.face_flip.cpu().numpy()
    assert np.array_equal(flip, today.face_flip.cpu().numpy() ^ turned_faces.astype(np.int32)) and np.array_equal(flip, want_flip)
    assert got.topology['turned'] == want_counts['turned'] and got.topology['open_components'] == 0
    assert got.topology['flipped'] == int(flip.sum()) and got.topology['orient_components'] == 4
    assert {k: got.counts[k] for k in got.counts if k != 'rounds'} == {k: today.counts[k] for k in today.counts if k != 'rounds'}


def test_mesh_report_solid(dev):
    from geobi_gnn_amd import meshtopo
    nv, nf = M.nested()
    today = meshtopo.mesh_report(nv, nf, device=dev)
    assert meshtopo.mesh_report(nv, nf, device=dev, solid=False) == today
    r = meshtopo.mesh_report(nv, nf, device=dev, solid=True)
    assert {k: r[k] for k in today} == today and set(r) - set(today) == {'volume', 'closed_components', 'inward_components'}
    # all four wound outward: the file counts the cavity as volume, and --outward would turn it
    total = sum(M.signed_volume6(nv, nf[s:s + 128]) for s in (0, 128, 256, 384)) / 6.0
    assert abs(r['volume'] - total) <= 1e-12 * total and r['closed_components'] == 4 and r['inward_components'] == 1
    turned = M.flipped(nf, np.repeat([False, True, False, False], 128))
    r = meshtopo.mesh_report(nv, turned, device=dev, solid=True)
    assert r['inward_components'] == 0 and abs(r['volume'] - (total - 2 * M.signed_volume6(nv, nf[128:256]) / 6.0)) <= 1e-12 * total


# ------------------------------------------------------------------------------------------------ the workspaces
def test_workspace_guard_band_and_a_short_one(dev, monkeypatch):
    from geobi_gnn_amd import _lib as L
    from geobi_gnn_amd import meshwind
    verts, faces, h, q, terms = _big()
    nv, nf = M.nested()
    label = np.repeat(np.arange(4) * 128, 128).astype(np.int32)
    calls = {'geobi_winding_number': lambda: [meshwind.winding_number(q[:257], verts, faces, device=dev)],
             'geobi_part_solids': lambda: list(meshwind.part_solids(nv, nf, label, device=dev))}
    for entry, run in calls.items():
        want = W._flat(run(), [])
        guard = W._Guarded().install(monkeypatch)
        got = W._flat(run(), [])
        assert guard.sentinels_whole() and list(guard.entries.values()) == [entry]
        assert got == want and guard.requests[0][2] > W.SHORT_BY
        monkeypatch.undo()
        guard = W._Guarded(short_at=0).install(monkeypatch)
        with pytest.raises(L.GeobiError) as e:
            run()
        monkeypatch.undo()
        assert guard.sentinels_whole()
        give, nbytes = guard.requests[0][1:]
        m = re.search(r'%s failed: %s: workspace too small \((\d+) bytes given, (\d+) needed\)' % (entry, entry[6:]), str(e.value))
        assert m and int(m.group(1)) == give and give < int(m.group(2)) <= nbytes, str(e.value)


# ------------------------------------------------------------------------------------------------ the commands
def test_commands(dev, tmp_path, capsys):
    from geobi_gnn_amd import __main__ as main
    from geobi_gnn_amd import meshio
    data = str(tmp_path / 'scan')
    os.makedirs(data)
    nv, table = _scrambled(11)
    meshio.write_obj(os.path.join(data, 'shells.obj'), nv, table)
    assert main.main(['info', '--data_dir', data, '--solid']) == 0
    out = capsys.readouterr().out
    m = re.search(r"closed: yes,  'shells\.obj',  volume: (-?[0-9.e+-]+),  closed_components: 4,  inward_components: (\d)$", out, re.M)
    assert m, out
    assert main.main(['info', '--data_dir', data]) == 0
    assert 'volume' not in capsys.readouterr().out
    assert main.main(['clean', '--data_dir', data, '--outward']) == 0
    out = capsys.readouterr().out
    assert re.search(r'turned: %d,  open_components: 0$' % M.orient_outward(nv, table)[3]['turned'], out, re.M), out
    cleaned = meshio.read_obj(os.path.join(data, 'clean', 'shells.obj'))
    assert _volume_signs(cleaned[0], cleaned[1]) == M.NESTED_SIGNS
    assert main.main(['clean', '--data_dir', data, '--orient']) == 0
    assert 'turned' not in capsys.readouterr().out
    # eval --free --signed: a shrunk copy against the shells
    res, orig = str(tmp_path / 'result'), str(tmp_path / 'original')
    os.makedirs(res)
    os.makedirs(orig)
    meshio.write_obj(os.path.join(orig, 'shells.obj'), *cleaned)
    centre = np.where(cleaned[0][:, :1] > 2.0, [[3.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]])
    meshio.write_obj(os.path.join(res, 'shells_d.obj'), ((cleaned[0] - centre) * 0.98 + centre).astype(np.float32), cleaned[1])
    assert main.main(['eval', '--result_dir', res, '--original_dir', orig, '--free']) == 0
    free_bytes = open(os.path.join(res, 'ErrorInfo_free.txt'), 'rb').read()
    assert not os.path.exists(os.path.join(res, 'ErrorInfo_signed.txt'))
    assert main.main(['eval', '--result_dir', res, '--original_dir', orig, '--free', '--signed']) == 0
    assert open(os.path.join(res, 'ErrorInfo_free.txt'), 'rb').read() == free_bytes
    lines = open(os.path.join(res, 'ErrorInfo_signed.txt')).read().splitlines()
    assert lines[0].startswith('Error_signed:') and len(lines) == 4
    fields = lines[3].split()
    assert fields[0] == 'shells_d.obj' and int(fields[1]) == cleaned[0].shape[0] and abs(float(fields[5]) - 0.98 ** 3) < 1e-5
    # three shells shrink into their solids; the cavity's copy shrinks into the void, which is outside: 66 of 264 vertices
    assert float(fields[4]) == 0.75 and float(fields[2]) < 0
