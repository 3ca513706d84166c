"""The matching oracle (tests/match_oracle.py) itself, on the CPU: rows worked by hand, and the CONDITION the GPU tests
(tests/test_gpu_match.py) rest on -- on scene R no query has a tie between its best and its runner-up, and a fused, a
widened and a reordered evaluation of the distance each give other bits in at least one query in ten, so comparing
bits catches such a kernel."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_oracle as MO  # noqa: E402

f32 = np.float32
INF = np.inf


def row(*v):
    r = np.zeros(MO.LEN, f32)
    r[:len(v)] = v
    return r


def last(x):
    r = np.zeros(MO.LEN, f32)
    r[-1] = x
    return r


# candidates: two equal rows at ids 0 and 2, one apart, and four unusable ones
B_HAND = np.stack([row(1, 2, 3), row(4, 6, 3), row(1, 2, 3), row(), -row(), last(np.nan), last(np.inf)])
#   q0 = (1, 2, 4):  D = 0 + 0 + 1 = 1 to ids 0 and 2 (a tie: id 0, runner-up 1), 9 + 16 + 1 = 26 to id 1
#   q1 = (4, 6, 5):  D = 9 + 16 + 4 = 29 to ids 0 and 2, 0 + 0 + 4 = 4 to id 1
#   q2 = 0, q3 = -0.0, q4 has a NaN, q5 an inf: unusable, nothing found
#   q6 = (1e20, 0, ...): (1e20 - 1)^2 overflows: D = +inf to every candidate, unmatched
A_HAND = np.stack([row(1, 2, 4), row(4, 6, 5), row(), -row(), last(np.nan), last(-np.inf), row(1e20)])
WANT_HAND = ([0, 1, -1, -1, -1, -1, -1], [1, 4, INF, INF, INF, INF, INF], [1, 29, INF, INF, INF, INF, INF])


def hand_cases():
    """-> [(name, A, B, ids, d1, d2)]"""
    q = A_HAND[:2]
    return [
        ("hand", A_HAND, B_HAND, *WANT_HAND),
        ("one candidate", q, B_HAND[1:2], [0, 0], [26, 4], [INF, INF]),
        ("one usable candidate", q, B_HAND[[3, 1, 5]], [1, 1], [26, 4], [INF, INF]),
        ("no candidate", q, B_HAND[3:], [-1, -1], [INF, INF], [INF, INF]),
        ("empty B", q, B_HAND[:0], [-1, -1], [INF, INF], [INF, INF]),
        # a row of 1e20 is usable but at D = +inf of everything else: no match, never a runner-up -- yet at D = 0 of itself
        ("1e20 candidate", q, np.stack([row(1, 2, 3), row(1e20), row(-1e20)]), [0, 0], [1, 29], [INF, INF]),
        ("1e20 both", np.stack([row(1e20)]), np.stack([row(1, 2, 3), row(1e20)]), [1], [0], [INF]),
    ]


def hand_pairs():
    """-> a (m, 33), b (m, 33), D (m,) float32: usable pairs with distances worked by hand"""
    a = [row(1, 2, 4), row(1, 2, 4), row(4, 6, 5), row(1e20), row(1e20), last(3), row(0.5, 0, -0.25)]
    b = [row(1, 2, 3), row(4, 6, 3), row(1, 2, 3), row(1, 2, 3), row(1e20), last(-1), row(0, 0, 0, 2)]
    D = [1, 26, 29, INF, 0, 16, 0.25 + 0.0625 + 4]
    return np.stack(a), np.stack(b), np.array(D, f32)


def test_usable_rows():
    assert MO.usable(B_HAND).tolist() == [True, True, True, False, False, False, False]
    assert MO.usable(A_HAND).tolist() == [True, True, False, False, False, False, True]
    assert np.signbit(-row()).all()  # (the -0.0 row is what it says)


def test_hand_distances():
    a, b, D = hand_pairs()
    for k in range(len(a)):
        got = MO.dist_matrix(a[k:k + 1], b[k:k + 1])[0, 0]
        assert got.dtype == f32 and got == D[k], (k, got, D[k])
        assert MO.dist_matrix(b[k:k + 1], a[k:k + 1])[0, 0] == D[k]
    # rounding happens where the contract says: 2^24 + 1 is not a float32, so (2^12)^2 + 1^2 = 2^24 in float32
    assert MO.dist_matrix(row(4096, 1)[None], row()[None])[0, 0] == f32(16777216.0)
    assert MO.dist_matrix_f64(row(4096, 1, 1)[None], row()[None])[0, 0] == f32(16777218.0)
    assert MO.dist_matrix(row(4096, 1, 1)[None], row()[None])[0, 0] == f32(16777216.0)


def test_hand_matches():
    for name, A, B, ids, d1, d2 in hand_cases():
        g_ids, g1, g2 = MO.match(A, B)
        assert g_ids.dtype == np.int64 and g1.dtype == f32 and g2.dtype == f32
        assert g_ids.tolist() == list(ids), name
        assert np.array_equal(g1, np.array(d1, f32)) and np.array_equal(g2, np.array(d2, f32)), name


def test_hand_correspondences():
    A, B = A_HAND, B_HAND
    # back: B0 -> q0 (1 against 29), B1 -> q1 (4 against 26), B2 -> q0
    assert MO.match(B, A)[0].tolist() == [0, 1, 0, -1, -1, -1, -1]
    assert MO.correspondences(A, B, 1.0, True).tolist() == [[0, 0], [1, 1]]
    assert MO.correspondences(A, B, 1.0, False).tolist() == [[0, 0], [1, 1]]
    # q0: 1 <= 0.5 * 1 fails; q1: 4 <= 0.5 * 29 holds
    assert MO.correspondences(A, B, 0.5, True).tolist() == [[1, 1]]
    # the rule is <=: 4 <= (4 / 32) * 32 with candidates at 4 and 32
    ids, d1, d2 = MO.match(A[1:2], np.stack([row(4, 6, 3), row(0, 2, 5)]))
    assert (ids[0], d1[0], d2[0]) == (0, 4, 32)
    assert MO.correspondences(A[1:2], np.stack([row(4, 6, 3), row(0, 2, 5)]), 0.125, False).tolist() == [[0, 0]]
    assert MO.correspondences(A[1:2], np.stack([row(4, 6, 3), row(0, 2, 5)]), 0.12, False).tolist() == []
    # not mutual: two queries share a candidate, the nearer one keeps it
    A2 = np.stack([row(1, 2, 5), row(1, 2, 4)])
    assert MO.match(A2, B)[0].tolist() == [0, 0]
    assert MO.correspondences(A2, B, 1.0, True).tolist() == [[1, 0]]
    assert MO.correspondences(A2, B, 1.0, False).tolist() == [[0, 0], [1, 0]]
    assert MO.correspondences(A[:0], B).shape == (0, 2) and MO.correspondences(A, B[:0]).shape == (0, 2)


_R = {}


def scene_r_reference():
    """scene R with its distance matrix and match, computed once per process: A, B, D, ids, d1, d2"""
    if not _R:
        A, B = MO.scene_r()
        D = MO.dist_matrix(A, B)
        ids, d1, d2 = MO.match_from(D, MO.usable(A), MO.usable(B))
        _R.update(A=A, B=B, D=D, ids=ids, d1=d1, d2=d2)
    return _R


def test_scene_r_is_decisive():
    R = scene_r_reference()
    A, B, D, ids, d1, d2 = (R[k] for k in ("A", "B", "D", "ids", "d1", "d2"))
    assert A.shape == (3000, 33) and B.shape == (2999, 33) and len(A) % 64 == 56 and len(B) % 2 == 1
    assert MO.usable(A).all() and MO.usable(B).all() and np.all(ids >= 0)
    assert np.array_equal(D.view(np.uint32), MO.dist_matrix(B, A).T.view(np.uint32))  # D(a, b) and D(b, a): the same bits
    assert not np.any(d1 == d2)
    gap = ((d2.astype(np.float64) - d1) / d2).min()
    print("smallest relative gap between best and runner-up: %.3g" % gap)
    assert gap > 0
    for f in (MO.dist_matrix_fma, MO.dist_matrix_f64, MO.dist_matrix_reversed):
        e1 = MO.match_from(f(A, B), MO.usable(A), MO.usable(B))[1]
        share = np.mean(e1.view(np.uint32) != d1.view(np.uint32))
        print("%s: other bits of the best distance in %.1f %% of the queries" % (f.__name__, 100 * share))
        assert share >= 0.1, f.__name__
