"""The NumPy oracle of minimum-distance subsampling (tests/thin_oracle.py) checked against itself and against first
principles, without the library: the parallel round rule run to completion is sequential greedy selection on uniform,
slab and line scenes in both priority modes; kept points are pairwise at least the bound apart, every dropped eligible
point has a kept one inside the bound, the owner is the (DistSq, id) minimum; the cell-grid lists are the brute-force
lists; and a line at spacing 2^-7 gives the sets the contract's strict bound says."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thin_oracle as TO  # noqa: E402

f32 = np.float32
nan, inf = np.nan, np.inf


def _uniform(n, seed, box=(1.0, 1.0, 1.0)):
    return (np.random.default_rng(seed).random((n, 3)) * np.array(box)).astype(f32)


def line_scene(n=600, seed=3):
    """n points at spacing 2^-7 along x, ids permuted -> (points, position of every id)"""
    pos = np.random.default_rng(seed).permutation(n)
    pts = np.zeros((n, 3), f32)
    pts[:, 0] = pos.astype(f32) * f32(2.0 ** -7)
    return pts, pos


SCENES = {
    "uniform": lambda: (_uniform(1500, 1), 0.12),
    "slab": lambda: (_uniform(1500, 2, (2.0, 2.0, 0.02)), 0.1),
    "line": lambda: (line_scene(300, 4)[0], 3.5 * 2.0 ** -7),
}


def _scores(pts, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "coordinate":
        s = pts[:, 0].copy()
    else:  # heavy ties, NaN, -1, +-0, +-inf
        s = rng.integers(0, 4, len(pts)).astype(f32)
        pick = rng.permutation(len(pts))
        s[pick[:15]] = nan
        s[pick[15:30]] = -1.0
        s[pick[30:40]] = -0.0
        s[pick[40:43]] = inf
        s[pick[43:46]] = -inf
    return s


def _check_first_principles(pts, r, lists, e, kept, own):
    bound = f32(r) * f32(r)
    k = np.nonzero(kept)[0]
    assert not kept[~e].any() and np.all(own[~e] == -1)
    for i in k:  # pairwise >= bound, by every pair
        d = TO.dist_sq(pts[k], pts[i])
        assert np.all((d >= bound) | (k == i)) and own[i] == i
    for i in np.nonzero(e & ~kept)[0]:
        d = TO.dist_sq(pts[k], pts[i])
        inside = d < bound
        assert inside.any()
        best = min(zip(d[inside].tolist(), k[inside].tolist()))
        assert own[i] == best[1]


@pytest.mark.parametrize("scene", sorted(SCENES))
@pytest.mark.parametrize("mode", ["hash 0", "hash 77", "ties", "coordinate"])
def test_rounds_to_completion_are_greedy(scene, mode):
    pts, r = SCENES[scene]()
    lists = TO.site_lists(pts, r)
    score = None if mode.startswith("hash") else _scores(pts, mode, 9)
    seed = int(mode.split()[1]) if score is None else 0
    e = TO.eligible(lists, score)
    order = TO.priority_order(e, seed, score)
    kept = TO.greedy(lists, order)
    states, history = TO.rounds(lists, TO.rank_of(order, len(pts)))
    assert history[-1] == 0 and all(x >= y for x, y in zip(history, history[1:]))
    assert np.array_equal(states[-1] == TO.KEPT, kept)
    assert np.array_equal(states[-1] == TO.DROPPED, e & ~kept) and np.array_equal(states[-1] == TO.INELIGIBLE, ~e)
    for s in states:  # what a round keeps stays kept: every prefix is a subset of K
        assert not (s == TO.KEPT)[~kept].any()
    # a given number of rounds stops where the run to completion passed
    some, h = TO.rounds(lists, TO.rank_of(order, len(pts)), R=2)
    assert h == history[:2] and np.array_equal(some[-1], states[min(1, len(states) - 1)])
    _check_first_principles(pts, r, lists, e, kept, TO.owner(pts, lists, kept, e))


def test_cell_lists_are_the_brute_force_lists():
    pts = np.concatenate([_uniform(700, 5), np.tile(f32([0.5, 0.5, 0.5]), (40, 1)),
                          f32([[nan, 0, 0], [0.1, inf, 0.2], [0.5, 0.5, 0.5 + 2.0 ** -4]])])
    gone = np.array([3, 77, 705])
    for r in (0.15, 2.0 ** -4, np.nextafter(f32(2.0 ** -4), f32(1))):
        for deleted in (None, gone):
            a, b = TO.site_lists(pts, r, deleted), TO.brute_lists(pts, r, deleted)
            for i in range(len(pts)):
                assert np.array_equal(np.sort(a.of(i)), b.of(i)), (r, i)
            assert np.array_equal(TO.eligible(a), TO.eligible(b))
    assert not TO.eligible(a)[[740, 741, 3, 77, 705]].any()


def test_exact_spacing_on_a_line():
    """600 points at spacing 2^-7, score = -x: greedy walks the line from x = 0.  At r = 4 spacings a point at exactly r
    is no neighbour, so every 4th position is kept; one ulp more and it is every 5th."""
    pts, pos = line_scene()
    score = -pts[:, 0]
    for r, step in ((f32(4 * 2.0 ** -7), 4), (np.nextafter(f32(4 * 2.0 ** -7), f32(1)), 5)):
        ids, own, lists = TO.thin(pts, r, score=score)
        assert np.array_equal(np.sort(pos[ids]), np.arange(0, 600, step))
        id_at = np.argsort(pos)  # the id at every position
        for i in range(600):  # the nearest kept position within reach (exactly 4 away: only with the wider radius)
            c = [k for k in range(0, 600, step) if abs(k - pos[i]) < step]
            assert own[i] == min(((k - pos[i]) ** 2, id_at[k]) for k in c)[1]
        e = TO.eligible(lists, score)
        states, history = TO.rounds(lists, TO.rank_of(TO.priority_order(e, 0, score), 600))
        assert len(history) == 2 * len(ids) - (0 if (599 % step) else 1)  # a kept wave, then the drops it causes


def test_hash_mode_depends_on_the_seed_and_on_nothing_else():
    pts = _uniform(800, 6)
    a = TO.thin(pts, 0.1, seed=1)[0]
    assert np.array_equal(a, TO.thin(pts, 0.1, seed=1, lists=TO.brute_lists(pts, 0.1))[0])
    assert not np.array_equal(a, TO.thin(pts, 0.1, seed=2)[0])
    assert int(TO.shape_mix(1, [0])[0]) == 0x514E28B7 and int(TO.shape_mix(0, [0])[0]) == 0  # fmix32, as shape_terms pins it
