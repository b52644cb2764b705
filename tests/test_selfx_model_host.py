"""tests/selfx_model.py on the host: the exact statement of the definition (integers and fractions, point sets) and the
order statement of the kernel's procedure (numpy fp64) agree pair by pair wherever the arithmetic is exact -- the hand
cases, random integer soups, the same soups at coordinates up to 2^14 -- and the exact statement catches mistakes planted
in the other one.  No GPU."""
import numpy as np
import pytest

import selfx_model as X

HAND = X.hand_cases()


@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_cases_both_statements_and_the_pairs_written_down(name):
    verts, faces, state, pairs = HAND[name]
    assert X.exact_pairs(verts, faces, state) == pairs
    found = X.search(verts, faces, state)
    assert X.pair_set(found) == pairs
    assert found.counts['pairs'] == len(pairs) and found.counts['pairs_k2'] == sum(1 for p in pairs if p[2] == 2)
    assert found.hits.sum() == 2 * len(pairs)


def test_hand_cases_count_what_they_leave_out():
    c = {name: X.search(*HAND[name][:3]).counts for name in HAND}
    assert (c['k3_duplicates']['included'], c['k3_duplicates']['degenerate'], c['k3_duplicates']['box_candidates']) == (4, 0, 3)
    assert (c['repeated_index']['included'], c['repeated_index']['degenerate']) == (2, 1)
    assert (c['zero_area']['included'], c['zero_area']['degenerate']) == (2, 1)
    assert (c['excluded_by_state']['included'], c['excluded_by_state']['degenerate']) == (1, 0)
    assert c['k0_boxes_overlap_triangles_apart']['box_candidates'] == 1 and c['k0_parallel_planes']['box_candidates'] == 0
    assert c['k2_folded_flat']['pairs_k2'] == 1 and c['k2_dihedral']['box_candidates'] == 1


@pytest.fixture(scope='module')
def soups():
    out = {}
    for seed in X.SOUP_SEEDS:
        verts, faces = X.soup(seed)
        out[seed] = (verts, faces, X.exact_pairs(verts, faces))
    return out


@pytest.mark.parametrize('seed', X.SOUP_SEEDS)
def test_integer_soups_agree_pair_by_pair(soups, seed):
    verts, faces, exact = soups[seed]
    found = X.search(verts, faces)
    assert X.pair_set(found) == exact and len(exact) > 0
    assert found.counts['box_candidates'] >= found.counts['pairs'] == len(exact)
    # scaled by 2^10 and shifted: differences below 2^15, every product exact, the same pairs
    big = X.scaled(verts)
    assert X.pair_set(X.search(big, faces)) == exact
    assert X.exact_pairs(big, faces) == exact


def test_the_soups_hold_every_class_both_ways():
    seen = {}
    for seed in X.SOUP_SEEDS:
        for key, n in X.exact_classes(*X.soup(seed)).items():
            seen[key] = seen.get(key, 0) + n
    for k in (0, 1, 2):
        assert seen.get((k, True), 0) > 0 and seen.get((k, False), 0) > 0, (k, seen)


@pytest.mark.parametrize('fault, cases', [
    ('touching_apart', ('k0_vertex_in_the_face', 'k0_vertex_on_an_edge', 'k0_edges_cross_in_one_point')),
    ('no_coplanar', ('k0_coplanar_overlap', 'k0_one_inside_the_other', 'k1_coplanar_wedges_overlap', 'k2_folded_flat')),
    ('no_k1', ('k1_opposite_edge_through_the_face', 'k1_coplanar_wedges_overlap'))])
def test_planted_faults_are_caught(soups, fault, cases):
    for name in cases:
        verts, faces, state, pairs = HAND[name]
        assert X.pair_set(X.search(verts, faces, state, fault=fault)) != X.exact_pairs(verts, faces, state) == pairs, name
    for seed in X.SOUP_SEEDS:
        verts, faces, exact = soups[seed]
        assert X.pair_set(X.search(verts, faces, fault=fault)) != exact, seed


def test_sizes_and_the_stated_bound():
    # the exactness bound of the header: 2^14 coordinates give dot products below 2^48 < 2^53
    m = 1 << 14
    diff, cross = 2 * m, 2 * (2 * m) ** 2
    assert 3 * cross * diff < 1 << 48 <= 1 << 53
    assert X.TILE == 256 and X.QUERY_BLOCK == 512
    for empty in (X.search(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32)),
                  X.search(np.zeros((3, 3)), np.zeros((0, 3), dtype=np.int32))):
        assert empty.pairs.shape == (0, 2) and empty.counts == dict.fromkeys(X.COUNT_KEYS, 0)
