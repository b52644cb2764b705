"""tests/wind_model.py held to account without a GPU: the fp64 term against a 60-digit evaluation (where the tolerance of
tests/test_gpu_wind.py, F * 2^-40, comes from), the det == 0 rule on an integer cube, exact negation under a reversal, and
the outward rule on nested shells."""
import numpy as np
import pytest

import wind_model as M

QUANTUM = 2.0 ** -40


def _mp_winding(queries, verts, faces, subsets):
    """60-digit winding numbers of float32 inputs (exact as mpf), the same formula with the det == 0 rule; one pass over the
    pairs serves every subset of the faces -> {name: [mpf per query]}"""
    import mpmath as mp
    mp.mp.dps = 60
    tri = [[[mp.mpf(float(x)) for x in verts[i]] for i in face] for face in faces]
    out = {name: [] for name in subsets}
    for q in queries:
        p = [mp.mpf(float(x)) for x in q]
        theta = []
        for t in tri:
            a, b, c = ([t[k][i] - p[i] for i in range(3)] for k in range(3))
            det = (a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2])) + a[2] * (b[0] * c[1] - b[1] * c[0])
            if det == 0:
                theta.append(mp.mpf(0))
                continue
            dot = lambda u, w: u[0] * w[0] + u[1] * w[1] + u[2] * w[2]
            la, lb, lc = mp.sqrt(dot(a, a)), mp.sqrt(dot(b, b)), mp.sqrt(dot(c, c))
            theta.append(2 * mp.atan2(det, la * lb * lc + dot(a, b) * lc + dot(b, c) * la + dot(c, a) * lb))
        for name, keep in subsets.items():
            out[name].append(mp.fsum(theta[f] for f in keep) / (4 * mp.pi))
    return out


@pytest.mark.parametrize('k, F', [(2, 128), (3, 512)])
def test_the_model_against_sixty_digits(k, F):
    """Inputs: the sphere of F faces, closed and with the cap z > 0.6 removed; 40 queries at each of 1, 1/4, 1/64 and 1/1024
    of the mean edge off the sphere, alternately inside and outside.  Asserted: the plain fp64 sum is within one quantum
    (2^-40) of the 60-digit value -- measured: at most 1.6e-15 in the stated order, 2.0e-15 with the faces reversed in
    order, five orders below F * 2^-40 -- and the quantised model within F / 2 quanta (half a quantum of rounding per
    term) plus that."""
    import mpmath as mp
    verts, faces = M.sphere(k)
    assert faces.shape[0] == F
    h = M.mean_edge(verts, faces)
    centroid_z = verts[faces].astype(np.float64).mean(axis=1)[:, 2]
    subsets = {'closed': list(range(F)), 'capped': [int(f) for f in np.flatnonzero(centroid_z <= 0.6)]}
    assert 0 < len(subsets['capped']) < F
    queries = []
    for j, frac in enumerate((1.0, 0.25, 1.0 / 64, 1.0 / 1024)):
        d = M.directions(40, 10 * k + j)
        sign = np.where(np.arange(40) % 2 == 0, 1.0, -1.0)[:, None]
        queries.append(d * (1.0 + sign * frac * h))
    queries = np.concatenate(queries).astype(np.float32)
    want = _mp_winding(queries, verts, faces, subsets)
    worst_plain = worst_reordered = worst_quantised = 0.0
    for name, keep in subsets.items():
        sub = faces[keep]
        plain, reordered = M.winding_plain(queries, verts, sub), M.winding_plain(queries, verts, sub[::-1])
        quantised = M.winding(queries, verts, sub)
        for i, ref in enumerate(want[name]):
            worst_plain = max(worst_plain, float(abs(mp.mpf(float(plain[i])) - ref)))
            worst_reordered = max(worst_reordered, float(abs(mp.mpf(float(reordered[i])) - ref)))
            worst_quantised = max(worst_quantised, float(abs(mp.mpf(float(quantised[i])) - ref)))
        if name == 'closed':      # the radius of a query says which side it is on
            r = np.linalg.norm(queries.astype(np.float64), axis=1)
            far = np.abs(r - 1.0) >= 0.25 * h
            assert np.array_equal(np.rint(quantised[far]), (r[far] < 1.0).astype(np.float64))
    print('F = %d: plain %.3g, reordered %.3g, quantised %.3g (bound %.3g)' % (F, worst_plain, worst_reordered, worst_quantised,
                                                                           F * QUANTUM))
    assert worst_plain <= QUANTUM and worst_reordered <= QUANTUM
    assert worst_quantised <= 0.5 * F * QUANTUM + QUANTUM


def test_the_integer_cube():
    verts, faces = M.cube()
    q = np.array([[0.5, 0.5, 0.0], [0.5, 0.5, 0.5], [0.5, 0.5, -1.0], [3.0, 0.5, 0.5], [0.5, 0.0, 0.0], [0.0, 0.0, 0.0]],
                 dtype=np.float32)
    w = M.winding(q, verts, faces)
    theta, det = M.thetas(q, verts[faces])
    # a face centre: the two faces of its square have det == 0 and count 0, the other ten give half a turn
    assert (det[0] == 0.0).sum() == 2 and abs(w[0] - 0.5) <= 12 * QUANTUM
    # the body centre: twelve equal terms of 1/12; the distance from 1 is what the quantisation leaves
    assert abs(w[1] - 1.0) <= 12 * 0.5 * QUANTUM, w[1] - 1.0
    print('cube centre: w - 1 = %g' % (w[1] - 1.0))
    # outside
    assert abs(w[2]) <= 12 * QUANTUM and abs(w[3]) <= 12 * QUANTUM
    # an edge midpoint and a corner: a quarter and an eighth, with every face through the point counting 0
    assert (det[4] == 0.0).sum() == 4 and abs(w[4] - 0.25) <= 12 * QUANTUM
    assert (det[5] == 0.0).sum() >= 6 and abs(w[5] - 0.125) <= 12 * QUANTUM


def test_a_reversal_negates_every_bit():
    verts, faces = M.sphere(2)
    cube_v, cube_f = M.cube()
    for v, f, q in ((verts, faces, (M.directions(64, 5) * np.linspace(0.2, 2.0, 64)[:, None]).astype(np.float32)),
                    (cube_v, cube_f, np.array([[0.5, 0.5, 0.0], [0.25, 0.5, 0.75], [2, 2, 2]], dtype=np.float32))):
        t, back = M.terms(q, v, f), M.terms(q, v, f[:, [0, 2, 1]])
        assert np.array_equal(back, -t)
        w, w_back = M.winding(q, v, f), M.winding(q, v, f[:, [0, 2, 1]])
        nonzero = w != 0.0                                     # an integer sum of 0 is +0.0 either way
        assert np.array_equal(w_back[nonzero].view(np.int64), (-w[nonzero]).view(np.int64)) and not w_back[~nonzero].any()


def test_parts_exclude_the_queries_own_component():
    verts, faces = M.nested()
    part = np.repeat(np.arange(4), 128)
    q = np.array([[0, 0, 0], [0.4, 0, 0], [0.8, 0, 0], [3, 0, 0], [5, 0, 0]], dtype=np.float32)
    for p in range(4):
        with_parts = M.winding(q, verts, faces, face_part=part, query_part=np.full(5, p))
        state = (part != p).astype(np.int32)
        assert np.array_equal(with_parts, M.winding(q, verts, faces, state=state))
    assert np.array_equal(np.rint(M.winding(q, verts, faces)), [3, 2, 1, 1, 0])


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_nested_shells_come_out_plus_minus_plus_plus(seed):
    verts, faces = M.nested()
    rng = np.random.RandomState(seed)
    reversed_parts = rng.rand(4) < 0.5
    if seed == 0:
        reversed_parts[:] = [True, False, True, True]          # every shell starts on the wrong side of the rule
    table = M.flipped(faces, np.repeat(reversed_parts, 128))
    out, flip, label, counts = M.orient_outward(verts, table)
    signs = [np.sign(M.signed_volume6(verts, out[128 * p:128 * p + 128])) for p in range(4)]
    assert tuple(signs) == M.NESTED_SIGNS
    want_flip = np.repeat(reversed_parts ^ (np.array(M.NESTED_SIGNS) < 0), 128)
    assert np.array_equal(flip == 1, want_flip)
    assert np.array_equal(label, np.repeat(np.arange(4) * 128, 128))
    assert counts['closed_components'] == 4 and counts['open_components'] == 0 and counts['ambiguous'] == 0
    assert counts['turned'] == int((reversed_parts ^ (np.array(M.NESTED_SIGNS) < 0)).sum())
    # again: nothing turns
    again = M.orient_outward(verts, out)
    assert again[3]['turned'] == 0 and np.array_equal(again[0], out)


def test_part_solids_of_the_model():
    verts, faces = M.nested()
    label = np.repeat(np.arange(4) * 128, 128).astype(np.int32)
    volume6, closed, consistent = M.part_solids(verts, faces, label)
    for p, (r, _) in enumerate(M.NESTED):
        x = 128 * p
        assert closed[x] == 1 and consistent[x] == 1
        # the inscribed polyhedron of 128 faces holds 0.86 .. 1 of the ball
        assert 0.8 * 8 * np.pi * r ** 3 < volume6[x] < 8 * np.pi * r ** 3
        assert abs(volume6[x] - M.signed_volume6(verts, faces[x:x + 128])) <= 128 * 2.0 ** -50 * volume6[x]
    state = np.ones(512, dtype=np.int32)
    state[200] = 0                                              # one face of the second shell removed
    _, closed, _ = M.part_solids(verts, faces, np.where(state == 1, label, -1), state)
    assert [closed[128 * p] for p in range(4)] == [1, 0, 1, 1]
