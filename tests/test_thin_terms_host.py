"""csrc/thin_terms.h compiled for the host with g++ -ffp-contract=off under -fsanitize=address,undefined, as a program of
its own (tests/cpp/thin_terms_host.cpp over the shim tests/cpp/host_shim): the two priority comparisons, the score and
eligibility tests, the round's three-way decision and the owner comparison give the NumPy oracle's answers
(tests/thin_oracle.py) over a table of ids, seeds and scores that holds NaN, +-0, +-inf and equal scores.  That the
program runs to its end with nothing on stderr is the first assertion."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thin_oracle as TO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32
nan, inf = np.nan, np.inf


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("thin_terms") / "thin_terms_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "thin_terms_host.cpp")])
    return exe


def _table():
    rng = np.random.default_rng(5)
    special = [nan, 0.0, -0.0, inf, -inf, 1.0, 1.0, -1.0, 3.0, 3.0, np.float32(1e-45), -np.float32(1e-45), 3.4e38]
    score = np.concatenate([np.array(special, f32), rng.integers(0, 4, 300).astype(f32), rng.normal(size=100).astype(f32)])
    ids = np.concatenate([[0, 1, 2, 3, 0x7fffffff, 0x7ffffffe], rng.integers(0, 2 ** 31 - 1, len(score) - 6)]).astype(np.int64)
    ids[20:40] = ids[0:20]  # the same id on both sides of a pair comes up too
    m = len(score)
    a, b = rng.integers(0, m, 6000), rng.integers(0, m, 6000)
    a[:len(special) ** 2] = np.repeat(np.arange(len(special)), len(special))  # every pair of the special scores
    b[:len(special) ** 2] = np.tile(np.arange(len(special)), len(special))
    a[-200:] = b[-200:]  # a point against itself
    seed = rng.choice(np.array([0, 1, 12345, 0xffffffff, 0x9E3779B1], np.int64), len(a))
    return ids, score, seed, a, b


@pytest.fixture(scope="module")
def output(program):
    ids, score, seed, a, b = _table()
    lines = ["%d %d" % (len(ids), len(a))]
    lines += ["%d %08x" % (i, w) for i, w in zip(ids, score.view(u32))]
    lines += ["%d %d %d" % (s, x, y) for s, x, y in zip(seed, a, b)]
    p = subprocess.run([program], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, "the sanitizer (or the program) stopped: %s" % p.stderr[-2000:]
    assert p.stderr == ""
    out = p.stdout.split("\n")
    assert out[-1] == "" and len(out) == len(a) + 8 + 3 + 1
    return out


def test_the_comparisons_match_the_numpy_restatement(output):
    ids, score, seed, a, b = _table()
    rows = [r.split() for r in output[:len(a)]]
    got = np.array([[int(w) for w in r[:4]] + [int(r[5])] for r in rows], np.int64)
    keys = np.array([int(r[4], 16) for r in rows], np.uint64)
    ia, ib, sa, sb = ids[a], ids[b], score[a], score[b]
    ka = np.array([TO.hash_key(s, [i])[0] for s, i in zip(seed, ia)], np.uint64)
    kb = np.array([TO.hash_key(s, [i])[0] for s, i in zip(seed, ib)], np.uint64)
    assert np.array_equal(keys, ka)
    assert np.array_equal(got[:, 0], (ka < kb).astype(np.int64))
    with np.errstate(invalid="ignore"):
        before = (sa > sb) | ((sa == sb) & (ia < ib))
        owner = (sa < sb) | ((sa == sb) & (ia < ib))
    assert np.array_equal(got[:, 1], before.astype(np.int64))
    assert np.array_equal(got[:, 2], (~np.isnan(sa)).astype(np.int64))
    assert np.array_equal(got[:, 3], (~np.isnan(sa)).astype(np.int64))
    assert np.array_equal(got[:, 4], owner.astype(np.int64))
    # what the table was made to hold: -0 == +0 ties go to the id, NaN is before nobody and nobody before it, a point
    # is never before itself, and the order by score is the oracle's priority_order
    assert got[a == b, 0].sum() == 0 and got[a == b, 1].sum() == 0
    assert got[np.isnan(sa) | np.isnan(sb), 1].sum() == 0
    zero = (sa == 0) & (sb == 0) & (np.signbit(sa) != np.signbit(sb))
    assert zero.any() and np.array_equal(got[zero, 1], (ia[zero] < ib[zero]).astype(np.int64))
    assert (np.isinf(sa) & np.isinf(sb) & (sa != sb)).any()
    first = np.unique(ids, return_index=True)[1]  # one row per distinct id
    order = first[np.lexsort((ids[first], -(score[first] + f32(0.0)).astype(np.float64)))]
    order = order[~np.isnan(score[order])]
    rank = {int(r): k for k, r in enumerate(order)}
    for x, y, w in zip(a[:2000], b[:2000], got[:2000, 1]):
        if x in rank and y in rank and ids[x] != ids[y]:
            assert bool(w) == (rank[int(x)] < rank[int(y)]), (x, y)


def test_the_decision_table_and_the_constants(output):
    ids, score, seed, a, b = _table()
    tail = output[len(a):-1]
    want = {}
    for e in (0, 1):
        for kb in (0, 1):
            for ub in (0, 1):
                want[(e, kb, ub)] = TO.INELIGIBLE if not e else TO.DROPPED if kb else TO.UNDECIDED if ub else TO.KEPT
    got = {tuple(int(w) for w in r.split()[1:4]): int(r.split()[4]) for r in tail[:8]}
    assert got == want
    assert tail[8] == "states %d %d %d %d" % (TO.UNDECIDED, TO.KEPT, TO.DROPPED, TO.INELIGIBLE)
    assert tail[9] == "owner -1 -2"
    assert tail[10] == "hash_mode 1 1 0"  # no score: a NaN in its place means nothing; a point that never met itself is out
