"""csrc/orient_terms.h compiled for the host with g++ -ffp-contract=off under -fsanitize=address,undefined, as a program
of its own (tests/cpp/orient_terms_host.cpp over the shim tests/cpp/host_shim): the agreement c is symmetric bit for bit
and the NumPy oracle's (tests/orient_oracle.py); the edge comparison is a strict total order over a table that holds
equal |c|, c = +-0 and the same pair with its ends swapped, and sorting by it is the oracle's sort; node and pair words
pack and unpack at id 2^31 - 2; hooks and parity jumps over random forests of 1 000 nodes, in random orders, leave every
node with the XOR of the signs along its path.  That the program runs to its end with nothing on stderr is the first
assertion."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orient_oracle as OO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32, u64 = np.float32, np.uint32, np.uint64


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("orient_terms") / "orient_terms_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "pcgol_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "orient_terms_host.cpp")])
    return exe


def _table():
    """(i, j, n_i, n_j) per row: random unit normals, then rows made to tie: the same normals for several pairs (equal
    |c|), opposite normals (c and -c), orthogonal ones (c = +0 and -0), and every pair again with its ends swapped"""
    rng = np.random.default_rng(17)
    v = rng.normal(size=(40, 3))
    nrm = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)
    ids = np.concatenate([[0, 1, 2, 3, 0x7ffffffe, 0x7ffffffd], rng.integers(4, 2 ** 31 - 3, 34)]).astype(np.int64)
    rows = []
    for _ in range(30):
        a, b = rng.choice(40, 2, replace=False)
        rows.append((ids[a], ids[b], nrm[a], nrm[b]))
    x, y, z = f32([1, 0, 0]), f32([0, 1, 0]), f32([0, 0, 1])
    for a, b in ((0, 1), (2, 3), (0, 3), (4, 5), (1, 2)):  # |c| = 1 five times over, the signs mixed
        rows.append((ids[a], ids[b], x, -x if a % 2 else x))
    for a, b in ((6, 7), (8, 9), (0, 2)):  # c = +0 and c = -0
        rows.append((ids[a], ids[b], x, y if a != 8 else -y))
    rows.append((ids[10], ids[11], z * f32(0.5), z))
    rows.append((ids[12], ids[13], z, -z * f32(0.5)))  # |c| = 0.5 twice
    rows += [(j, i, nj, ni) for i, j, ni, nj in rows]
    return rows


@pytest.fixture(scope="module")
def output(program):
    rows = _table()
    lines = ["%d" % len(rows)]
    for i, j, ni, nj in rows:
        lines.append("%d %d " % (i, j) + " ".join("%08x" % w for w in np.concatenate([ni, nj]).astype(f32).view(u32)))
    p = subprocess.run([program], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, "the sanitizer (or the program) stopped: %s" % p.stderr[-2000:]
    assert p.stderr == ""
    out = p.stdout.split("\n")
    assert out[-1] == "" and len(out) == 2 * len(rows) + 13 + 1
    return out


def test_c_is_symmetric_and_the_oracles(output):
    rows = _table()
    for (i, j, ni, nj), line in zip(rows, output):
        c0, c1, s, w, pij, pji = line.split()
        want = OO.agreement(ni, nj)[0]
        assert c0 == c1 == "%016x" % np.float64(want).view(u64)
        assert int(s) == (1 if want < 0 else 0)
        assert int(w, 16) == int(np.abs(np.float64(want)).view(u64)) + 1
        lo, hi = int(min(i, j)), int(max(i, j))
        assert int(pij, 16) == (lo << 33) | (hi << 1) | (1 if int(i) == hi else 0)
        assert int(pji, 16) == int(pij, 16) ^ 1
    assert any(OO.agreement(ni, nj)[0] == 0 and np.signbit(OO.agreement(ni, nj)[0]) for _, _, ni, nj in rows)


def test_the_edge_comparison_is_a_strict_total_order_and_the_oracles_sort(output):
    rows = _table()
    k = len(rows)
    before = np.array([[ch == "1" for ch in line] for line in output[k:2 * k]])
    assert before.shape == (k, k)
    c = np.array([OO.agreement(ni, nj)[0] for _, _, ni, nj in rows])
    lo = np.array([min(i, j) for i, j, _, _ in rows])
    hi = np.array([max(i, j) for i, j, _, _ in rows])
    same = (np.abs(c)[:, None] == np.abs(c)[None, :]) & (lo[:, None] == lo[None, :]) & (hi[:, None] == hi[None, :])
    assert same.sum() >= 2 * k  # (every row and its swapped twin)
    assert not before[same].any()  # irreflexive, and an edge is the same edge from either end
    assert np.array_equal(before | before.T, ~same)  # total ...
    assert not (before & before.T).any()  # ... and antisymmetric
    for a in range(k):  # transitive
        assert not (before[a][:, None] & before & ~before[a][None, :]).any()
    want = np.array([[OO.edge_before(c[a], lo[a], hi[a], c[b], lo[b], hi[b]) for b in range(k)] for a in range(k)])
    assert np.array_equal(before, want)
    order = OO.edge_order(lo, hi, c)
    for a, b in zip(order[:-1], order[1:]):
        assert before[a, b] or same[a, b]
    assert output[2 * k] == "none 1 0 0"  # "no edge" comes after every edge and not before itself


def test_words_keys_and_forests(output):
    tail = output[2 * len(_table()) + 1:-1]
    assert tail[0] == "words %d 1" % (2 ** 31 - 2)
    heights = f32([-np.inf, -1.0, -0.0, 0.0, 1e-45, 1.0, np.inf])
    keys = [int(line.split()[1], 16) for line in tail[1:8]]
    assert all(line.split()[2] == "7" for line in tail[1:8])
    assert keys == [int(v) for v in OO.anchor_key(heights, np.full(7, 7))]
    assert keys[2] == keys[3] and keys == sorted(keys)  # -0 ties with +0; the order of the heights
    assert tail[8] == "flip bf800000 ffc00001 80000000"
    assert tail[9] == "votes 1 -1 0 1 0"
    assert tail[10] == "rounds 1 1 2 12 13"
    assert tail[11] == "forests 0"
