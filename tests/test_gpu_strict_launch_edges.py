"""The strict sums' device pipeline on both sides of the launch decisions csrc/strict_plan.h owns (plan_strict_launches),
through pcgx_debug_strict_sum_dev: the one-GPU form, a Fit's first step, nine rows.

* the repair pass runs from kRepairMinTiles = 1024 tiles: 1023 tiles (off) and 1024 (on);
* the chain kernel's walk-ahead instantiation runs once some walker has spec_depth = 4 walks in front of it: 4 chunks of
  512 tiles (the plain kernel) and 5 (strict_chain_kernel<false, true>);
* the 5-chunk case without a single slot and with the in-kernel self-check (strict_chain_kernel<true, false>).

Rows as in test_gpu_strict_rows.py's three-chunk case: drifting, hovering, and one with +inf and -inf late in the row.
Checker: the plain sequential float32 accumulation, bit for bit; the eight finite rows are accumulated once at the
longest length and read off at every case's.

Counters.  stats[62]: walkers that gave up waiting for the chunk before them and walked alone (the tests require 0).
stats[58]: tiles the repair pass made jobs, written by strict_repair_kernel alone: 0 at 1023 tiles, 246 at 1024 on this
input.  stats[10]: without PCGX_STRICT_CLOCKS it is written only by the walk-ahead code of strict_chain_kernel<., true>
("walks ahead of a wait, carried through"; resolve_stats adds its tick column there, which is 0 without that variable),
so it is 0 wherever the plain kernel ran.  At 5 chunks it is printed and must be > 0: measured 8 on this input (the
walker of chunk 4 in eight of the nine rows; every one found its start state among its candidates, stats[11] = 8) at
commit b14be59 and at the commit that introduced this file, on an MI355X."""
import numpy as np
import pytest

from test_gpu_strict_rows import device_sums
from test_strict_model import same_bits, sequential_f32

pytestmark = pytest.mark.gpu

TILE, CHUNK_TILES = 2048, 512
REPAIR_EDGE = (1023 * TILE, 1023 * TILE + 1)                       # 1023 and 1024 tiles
CHAIN_EDGE = (4 * CHUNK_TILES * TILE, 4 * CHUNK_TILES * TILE + 1)  # 4 and 5 chunks
N_MAX = CHAIN_EDGE[1]


@pytest.fixture(scope="module")
def rows8():
    """-> (the eight finite rows at N_MAX, {n: their eight sequential sums over the first n terms})"""
    rng = np.random.Generator(np.random.PCG64(321))
    rows = [(rng.standard_normal(N_MAX) * 10.0 ** (k - 4) + (k % 3 - 1) * 10.0 ** (k - 6)).astype(np.float32) for k in range(8)]
    want = {n: [] for n in REPAIR_EDGE + CHAIN_EDGE}
    for t in rows:
        acc = np.add.accumulate(t, dtype=np.float32)  # (0.0f + t0 = t0 exactly, -0.0f aside: no such term here)
        for n in want:
            want[n].append(acc[n - 1])
    for k, t in enumerate(rows):
        assert same_bits(want[REPAIR_EDGE[0]][k], sequential_f32(t[:REPAIR_EDGE[0]])), k  # the reading-off is the checker's sum
    return rows, want


def run_case(rows8, n):
    rows, want = rows8
    last = (np.random.Generator(np.random.PCG64(n)).standard_normal(n) * 0.01).astype(np.float32)
    last[n - 100_000] = np.float32(np.inf)
    last[n - 50_000] = np.float32(-np.inf)
    got, stats = device_sums([t[:n] for t in rows] + [last])
    print("n = %d: stats[10] = %d, stats[58] = %d, stats[62] = %d" % (n, stats[10], stats[58], stats[62]))
    for k in range(8):
        assert same_bits(got[k], want[n][k]), (n, k, got[k], want[n][k], stats[:8])
    assert same_bits(got[8], sequential_f32(last)) and np.isnan(got[8]), (n, got[8], stats[:8])
    return stats


@pytest.mark.parametrize("n", REPAIR_EDGE)
def test_the_repair_pass_off_and_on(rows8, n):
    stats = run_case(rows8, n)
    assert stats[62] == 0 and stats[10] == 0, stats  # (two chunks: nobody walks ahead)
    assert (stats[58] > 0) == (n == REPAIR_EDGE[1]), stats


@pytest.mark.parametrize("n", CHAIN_EDGE)
def test_the_plain_chain_kernel_and_the_one_that_walks_ahead(rows8, n):
    stats = run_case(rows8, n)
    assert stats[62] == 0, stats
    assert (stats[10] > 0) == (n == CHAIN_EDGE[1]), stats


def test_five_chunks_without_a_slot_under_the_selfcheck(rows8, monkeypatch):
    monkeypatch.setenv("PCGX_STRICT_SLOTS_PER_SHARD", "0")
    monkeypatch.setenv("PCGX_STRICT_SELFCHECK", "1")
    stats = run_case(rows8, CHAIN_EDGE[1])
    assert not stats[12:16].any() and stats[6] == 0 and stats[7] == 0, stats[:24]
    assert stats[62] == 0, stats
