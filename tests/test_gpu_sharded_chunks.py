"""Sharded Fits with the reference's sums where a rank holds MORE than one chunk of the chain kernel (512 tiles of 2048
targets = 1 048 576 targets, csrc/strict.hip kChainTiles), and sessions that share one communicator.

Three hand-overs meet in such a Fit: the ring's from rank to rank (strict_enqueue_ring), the chain kernel's from
chunk to chunk inside a rank (chunk_state), and the walk ahead of that wait (strict_chain_kernel<., kSpec>, with
walks_before = rank * nchunks + chunk).  Every test compares with the CPU oracle's Fit of the concatenated target
(oracle/, sums_mode 0) bit for bit: transform, Value, Gradient, NumIteration.

* A: one ~4.5M-point target (synth.chunked_icp) cut three ways -- 3 slots (3 chunks ending on a single target, one
  full chunk, the rest), 2 slots (a cut on a tile boundary inside the fourth chunk), 8 slots (empty slots at both ends
  and in the middle, a single target, ranks with different chunk counts) -- through pcgx_icp_fit_multi (ring and
  collectives), through sessions stepped per slot (ring, with the walk ahead's guess forced to miss as well), and
  through two processes (IPC inboxes).  One oracle Fit serves all of them.
* B: two reference-sum sessions with different targets on every slot, stepped alternately on one communicator:
  each is its own oracle Fit (a ring word's tag must name the step on the communicator, not the session's step).
* C: config C5 as worded -- eight device slots, each with a replica of the 64M-point tree and its octant of the target,
  three steps in the collective form (why not the ring on one GPU: the test's docstring) -- against
  tests/golden/c5_octants_digest.json (the oracle's Fit of the eight octants in rank order; tests/golden/make_c5_digest.py
  octants).

All slots share the box's one GPU, as in tests/test_gpu_multi.py."""
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np
import pytest

import oracle as O
from pcgol_amd import _lib as L
from pcgol_amd import icp, kdtree, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 512 * 2048   # targets per chunk of the chain kernel (kChainTiles tiles of kTile)
NT = 4_500_000
CUTS = {   # the same target cut three ways
    3: [0, 2 * CHUNK + 1, 3 * CHUNK + 1, NT],                          # 3 chunks (the last: one target), 1 full, 2
    2: [0, 3 * CHUNK + 100 * 2048, NT],                                 # 4 chunks (a tile boundary inside the 4th), 2
    8: [0, 0, 1, 1, 2_200_000, 2_200_000, 3_300_000, NT, NT],           # -, 1 target, -, 3 chunks, -, 2, 2, -
}
MAX_SLOTS = 8


def nchunks(n):
    tiles = -(-n // 2048)
    return -(-tiles // 512)


def _bits(a):
    return np.asarray(a, np.float32).ravel().view(np.uint32).tolist()


def _same_as_oracle(trans, num_iteration, value, gradient, o):
    assert num_iteration == o["num_iteration"]
    assert _bits(trans) == _bits(o["trans"])
    assert _bits([value]) == _bits([o["value"]])
    assert _bits(gradient) == _bits(o["gradient"])


@pytest.fixture(scope="module")
def case():
    return synth.chunked_icp(n_target=NT)


@pytest.fixture(scope="module")
def oracle_a(case):
    """The oracle's Fit of the whole target: ~40 s of one CPU core."""
    c = case
    return O.icp_fit(O.KDTree(c["base"]), c["target"], c["max_dist"], c["min_pairs"], c["weight"], c["threshold"],
                     c["max_iteration"], sums_mode=0)


@pytest.fixture(scope="module")
def slots():
    L.check(L.lib().pcgx_init_devices(MAX_SLOTS, L.ptr(np.zeros(MAX_SLOTS, np.int32))))
    yield MAX_SLOTS
    L.check(L.lib().pcgx_set_device(0))


@pytest.fixture(scope="module")
def trees(case, slots):
    out = []
    for r in range(MAX_SLOTS):
        L.check(L.lib().pcgx_set_device(r))
        out.append(kdtree.New(case["base"]))   # the replica of slot r
    L.check(L.lib().pcgx_set_device(0))
    yield out
    del out


def _tiles(target, cuts):
    return [np.ascontiguousarray(target[cuts[r]:cuts[r + 1]]) for r in range(len(cuts) - 1)]


def test_cuts_hold_the_shapes_they_claim():
    assert [nchunks(CUTS[3][r + 1] - CUTS[3][r]) for r in range(3)] == [3, 1, 2]
    assert CUTS[3][1] % 2048 == 1 and CUTS[3][2] - CUTS[3][1] == CHUNK
    assert [nchunks(CUTS[2][r + 1] - CUTS[2][r]) for r in range(2)] == [4, 2]
    assert CUTS[2][1] % 2048 == 0 and 3 * CHUNK < CUTS[2][1] < 4 * CHUNK
    n8 = [CUTS[8][r + 1] - CUTS[8][r] for r in range(8)]
    assert n8[0] == n8[-1] == 0 and 0 in n8[1:-1] and 1 in n8
    assert sum(nchunks(n) >= 2 for n in n8) >= 2 and len({nchunks(n) for n in n8 if n > 1}) >= 2


# ------------------------------------------------------------------------------------ A.3: two processes (first: the
# oracle of the module is computed in this process while the ranks run)

def _process_worker(rank, world, port, q, cut):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pcgol_amd.distributed import Comm
        c = synth.chunked_icp(n_target=NT)
        lo, hi = (0, cut) if rank == 0 else (cut, NT)
        tile = np.ascontiguousarray(c["target"][lo:hi])
        tree = kdtree.New(c["base"])
        comm = Comm.gloo()
        params = icp._params(c["max_dist"], 0.0, c["min_pairs"], c["weight"], c["threshold"], c["max_iteration"])
        trans = np.empty(16, np.float32)
        st = L.IcpStat()
        L.check(L.lib().pcgx_icp_fit_sharded(tree._h, L.ptr(tile), len(tile), C.byref(params), comm._h, L.ptr(trans),
                                             C.byref(st)))
        comm.close()
        stats = np.zeros(4, np.int64)
        L.check(L.lib().pcgx_debug_shard_stats(L.ptr(stats), 0))
        kinds = np.zeros(2, np.int64)
        L.check(L.lib().pcgx_debug_ring_kinds(L.ptr(kinds), 0))
        q.put((rank, trans, int(st.num_iteration), float(st.evaluated.value), np.array(st.evaluated.gradient, np.float32),
               stats.tolist(), kinds.tolist()))
    finally:
        dist.destroy_process_group()


def test_two_processes_with_multi_chunk_shards_equal_the_oracle(request, monkeypatch):
    """Two processes, a callback (gloo) communicator, the ring with every inbox in its rank's GPU memory (IPC): rank 0
    holds 3.2M targets (4 chunks), rank 1 1.3M (2 chunks)."""
    import socket
    import torch.multiprocessing as mp
    monkeypatch.setenv("PCGX_SHARD_RING", "1")
    cut = 3_200_000
    assert (nchunks(cut), nchunks(NT - cut)) == (4, 2)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_process_worker, args=(r, 2, port, q, cut)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        t0 = time.time()
        o = request.getfixturevalue("oracle_a")
        print("oracle Fit of %d targets: %.1f s" % (NT, time.time() - t0))
        res = sorted(q.get(timeout=600) for _ in range(2))
    finally:
        for p in procs:
            p.join(timeout=120)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert o["num_iteration"] == 4
    for r in res:
        _same_as_oracle(r[1], r[2], r[3], r[4], o)
        assert r[5] == [4, 0, 1, 0], r[5]   # four ring steps, no collective step, no fallback
    assert res[0][6] == [1, 0], res[0][6]   # device inboxes, mapped through IPC


# ------------------------------------------------------------------------------------ A.1: pcgx_icp_fit_multi

def _fit_multi(c, trees, tiles, sums_mode=0):
    n = len(tiles)
    params = icp._params(c["max_dist"], 0.0, c["min_pairs"], c["weight"], c["threshold"], c["max_iteration"],
                         sums_mode=sums_mode)
    bases = (C.c_void_p * n)(*[t._h for t in trees[:n]])
    tps = (C.c_void_p * n)(*[t.ctypes.data for t in tiles])
    nts = (C.c_int64 * n)(*[len(t) for t in tiles])
    trans = np.empty(16, np.float32)
    st = L.IcpStat()
    rc = L.lib().pcgx_icp_fit_multi(n, bases, tps, nts, C.byref(params), L.ptr(trans), C.byref(st))
    return rc, trans, st


@pytest.mark.parametrize("ring", ["1", "0"], ids=["ring", "collectives"])
@pytest.mark.parametrize("ns", [3, 2, 8])
def test_fit_multi_with_multi_chunk_shards_equals_the_oracle(case, oracle_a, trees, ns, ring, monkeypatch):
    monkeypatch.setenv("PCGX_SHARD_RING", ring)
    tiles = _tiles(case["target"], CUTS[ns])
    stats = np.zeros(4, np.int64)
    kinds = np.zeros(2, np.int64)
    L.check(L.lib().pcgx_debug_shard_stats(L.ptr(stats), 1))
    L.check(L.lib().pcgx_debug_ring_kinds(L.ptr(kinds), 1))
    rc, trans, st = _fit_multi(case, trees, tiles)
    L.check(rc)
    L.check(L.lib().pcgx_debug_shard_stats(L.ptr(stats), 1))
    L.check(L.lib().pcgx_debug_ring_kinds(L.ptr(kinds), 1))
    assert kinds.tolist() == ([1, 0] if ring == "1" else [0, 0]), kinds
    assert (stats[0], stats[1], stats[2]) == ((4 * ns, 0, 1) if ring == "1" else (0, 4 * ns, 0)), stats
    _same_as_oracle(trans, st.num_iteration, st.evaluated.value, st.evaluated.gradient, oracle_a)
    assert 6 <= st.evaluated.num_pairs < NT


def test_fit_multi_float64_sums_with_multi_chunk_shards(case, trees, monkeypatch):
    """The float64 mode over the 3-slot cut: the one-GPU float64 Fit to rounding."""
    monkeypatch.setenv("PCGX_SHARD_RING", "1")
    c = case
    rc, t64, st64 = _fit_multi(c, trees, _tiles(c["target"], CUTS[3]), sums_mode=icp.SumsF64Tree)
    L.check(rc)
    reg = icp.PointToPointICPGradient(
        icp.PointToPointEvaluator(icp.NearestPointCorresponder(MaxDist=c["max_dist"]), MinPairs=c["min_pairs"],
                                  SumsMode=icp.SumsF64Tree),
        icp.GradientDescentUpdaterFactory(Weight=c["weight"], Threshold=c["threshold"], MaxIteration=c["max_iteration"]))
    t1, s1 = reg.Fit(trees[0], c["target"])
    assert st64.num_iteration == s1.NumIteration == 4
    assert np.max(np.abs(t64.ravel() - np.asarray(t1).ravel())) <= 1e-6


# ------------------------------------------------------------------------------------ slots in threads

def _run_slots(ns, body, timeout=600):
    """body(r, comm) in a thread per slot, slot r current, with a callback communicator each (the callback sums over
    the threads in rank order).  Returns the bodies' results; re-raises the first error."""
    from pcgol_amd.distributed import Comm
    barrier = threading.Barrier(ns)
    parts = [None] * ns

    def make_fn(r):
        def fn(a):
            parts[r] = a.copy()
            barrier.wait(timeout=120)
            tot = np.zeros_like(a)
            for k in range(ns):
                tot += parts[k]
            barrier.wait(timeout=120)
            a[:] = tot
        return fn
    out = [None] * ns
    errs = []

    def main(r):
        comm = None
        try:
            L.check(L.lib().pcgx_set_device(r))
            comm = Comm.callback(r, ns, make_fn(r))
            out[r] = body(r, comm)
        except Exception as e:  # noqa: BLE001
            errs.append((r, repr(e)))
            barrier.abort()
        finally:
            if comm is not None:
                comm.close()
    th = [threading.Thread(target=main, args=(r,)) for r in range(ns)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=timeout)
    assert not any(t.is_alive() for t in th), "a slot's thread did not finish"
    assert not errs, errs
    return out


def _session(c, tree, tile):
    return icp.IcpSession(tree, tile, c["max_dist"], c["min_pairs"], c["weight"], c["threshold"], c["max_iteration"],
                          SumsMode=icp.SumsReference)


def _step(sess, comm):
    L.check(L.lib().pcgx_icp_session_step_sharded(sess._h, comm._h, None))


# ------------------------------------------------------------------------------------ A.2: sessions per slot

@pytest.mark.parametrize("miss", [False, True], ids=["plain", "spec-miss"])
def test_sessions_per_slot_with_multi_chunk_shards_equal_the_oracle(case, oracle_a, trees, miss, monkeypatch):
    """The 3-slot cut, a session per slot stepped through pcgx_icp_session_step_sharded over the ring: the oracle's
    bits, no chunk walker that gave up its wait and walked alone ([62]), and walks ahead of the chunks' waits carried
    through ([10]) -- with the guess pushed off (PCGX_TEST_SPEC_MISS) none of them hits ([11]).
    (Not asserted: [63], summary workgroups that gave up their exchange.  Here the three slots' summary kernels share
    one GPU, and with 512 to 1025 tiles each they do not all fit on it at once: one launch's waiting workgroups can
    hold the places another launch's next tiles need, until the 2 ms bound frees them -- csrc/strict.hip,
    kExchangeTicks.  That costs time, not bits; a rank alone on its GPU has no such neighbour.)"""
    monkeypatch.setenv("PCGX_SHARD_RING", "1")
    if miss:
        monkeypatch.setenv("PCGX_TEST_SPEC_MISS", "1")
    c = case
    tiles = _tiles(c["target"], CUTS[3])
    assert max(nchunks(len(t)) for t in tiles) >= 3

    def body(r, comm):
        s = _session(c, trees[r], tiles[r])
        try:
            s.strict_stats()
            for _ in range(c["max_iteration"]):
                _step(s, comm)
            tr, st, _ = s.result()
            return tr, st, s.strict_stats()
        finally:
            s.close()
    out = _run_slots(3, body)
    walked = sum(int(o[2][10]) for o in out)
    hit = sum(int(o[2][11]) for o in out)
    print("walks ahead carried through %d, hit %d (miss forced: %s); summary workgroups that gave up, per slot: %s" %
          (walked, hit, miss, [int(o[2][63]) for o in out]))
    for tr, st, sst in out:
        _same_as_oracle(tr, st.NumIteration, st.Evaluated.Value, st.Evaluated.Gradient, oracle_a)
        assert sst[62] == 0, sst[60:64]
    assert walked > 0
    if miss:
        assert hit == 0


# ------------------------------------------------------------------------------------ B: two sessions, one communicator

@pytest.fixture(scope="module")
def two_cases():
    n = 200_000
    w = 10.0 * (n / 1e6) ** (1 / 3)
    ca, cb = synth.c4_icp(n=n, width=w, perm_seed=5), synth.c4_icp(n=n, width=w, perm_seed=11)
    tree = O.KDTree(ca["base"])
    fits = [O.icp_fit(tree, x["target"], x["max_dist"], x["min_pairs"], x["weight"], x["threshold"], x["max_iteration"],
                      sums_mode=0) for x in (ca, cb)]
    return ca, cb, fits


@pytest.mark.parametrize("pattern", ["alternate", "blocks"])
@pytest.mark.parametrize("ns", [2, 3])
def test_two_sessions_stepped_in_turn_on_one_communicator(two_cases, slots, ns, pattern, monkeypatch):
    """Two reference-sum sessions A and B with different targets on every slot, one communicator per slot.
    alternate: both reset, then A's step k and B's step k in turn; blocks: A 0-5, B 0-5, A 6-19, B 6-19.  Slot 0's
    thread sleeps 20 ms before it enqueues each of B's steps, so the slots behind it reach B's words first.  Each
    session's Fit is its own oracle Fit, bit for bit."""
    monkeypatch.setenv("PCGX_SHARD_RING", "1")
    ca, cb, fits = two_cases
    nt = len(ca["target"])
    cuts = [nt * r // ns for r in range(ns + 1)]
    n_it = ca["max_iteration"]
    if pattern == "alternate":
        order = [(x, k) for k in range(n_it) for x in (0, 1)]
    else:
        order = [(0, k) for k in range(6)] + [(1, k) for k in range(6)] + [(0, k) for k in range(6, n_it)] + \
                [(1, k) for k in range(6, n_it)]

    def body(r, comm):
        tree = kdtree.New(ca["base"])
        ss = [_session(x, tree, np.ascontiguousarray(x["target"][cuts[r]:cuts[r + 1]])) for x in (ca, cb)]
        try:
            for s in ss:
                s.reset()
                s.strict_stats()
            for x, k in order:
                if x == 1 and r == 0:
                    time.sleep(0.02)
                _step(ss[x], comm)
            return [(*s.result()[:2], s.strict_stats()) for s in ss]
        finally:
            for s in ss:
                s.close()
    out = _run_slots(ns, body)
    for r in range(ns):
        for x in (0, 1):
            tr, st, sst = out[r][x]
            assert sst[62] == 0 and sst[63] == 0, (r, x, sst[60:64])
            _same_as_oracle(tr, st.NumIteration, st.Evaluated.Value, st.Evaluated.Gradient, fits[x])


# ------------------------------------------------------------------------------------ C: C5, eight octants

def test_c5_eight_octants_sharded_equal_the_oracle_digest(monkeypatch):
    """Eight device slots, each with its replica of the 64M-point tree and its octant (8M targets: eight chunks per
    rank, 64 chunk hand-overs per sum), sessions stepped three times over callback communicators: the digest's bits
    (tests/golden/c5_octants_digest.json).
    The collective form (PCGX_SHARD_RING=0): the ring form needs every rank's chain kernel resident at once, and a
    chain workgroup holds 154 KB of LDS, one CU (tests/test_kernel_resources.py).  Eight ranks of eight chunks and nine
    rows are 576 workgroups; on the one GPU the slots share here (256 CUs) the waiting walkers of ranks 1-7 take every
    CU, rank 0's walkers never start, and the walks' 10 s bound ends the Fit (PCGX_E_RCCL) -- what a ring-form run of
    this test did.  On eight GPUs each holds its own 72.  The ring with several chunks per rank: the tests above.
    [62] (a later chunk's walker that gave up its 50 ms wait for the chunk before and walked alone, csrc/strict.hip
    kChunkWaitTicks) is not required to be 0: the wait is bounded by wall-clock time, and here eight ranks' 8M-target
    launches contend for one GPU (runs saw 1 and 25 of the 1512 waits give up, 12 at most on one slot; the bits were
    the digest's every time).  A broken hand-over would make all 189 waits of a slot give up."""
    monkeypatch.setenv("PCGX_SHARD_RING", "0")
    with open(os.path.join(os.path.dirname(__file__), "golden", "c5_octants_digest.json")) as f:
        g = json.load(f)
    L.check(L.lib().pcgx_init_devices(8, L.ptr(np.zeros(8, np.int32))))
    stats = np.zeros(4, np.int64)
    L.check(L.lib().pcgx_debug_shard_stats(L.ptr(stats), 1))
    try:
        base = synth.uniform_cloud_chunked(g["n_base"], g["width"], 2)
        tiles = synth.c5_tiles(base, 8, g["width"])
        assert [len(t) for t in tiles] == g["octant_sizes"]
        assert all(nchunks(len(t)) == 8 for t in tiles)
        w, th = np.full(6, g["weight"], np.float32), np.full(6, g["threshold"], np.float32)

        def body(r, comm):
            tree = kdtree.New(base)
            s = icp.IcpSession(tree, tiles[r], g["max_dist"], g["min_pairs"], w, th, g["max_iteration"],
                               SumsMode=icp.SumsReference)
            try:
                s.strict_stats()
                for _ in range(g["max_iteration"]):
                    _step(s, comm)
                tr, st, _ = s.result()
                return tr, st, s.strict_stats()
            finally:
                s.close()
                del tree
        out = _run_slots(8, body)
    finally:
        L.check(L.lib().pcgx_set_device(0))
    L.check(L.lib().pcgx_debug_shard_stats(L.ptr(stats), 1))
    assert (stats[0], stats[1]) == (0, 3 * 8), stats   # every slot's three steps in the collective form
    alone = [int(o[2][62]) for o in out]
    print("chunk walkers that walked alone, per slot:", alone)
    for tr, st, sst in out:
        assert st.NumIteration == g["fit3_num_iteration"] == 3
        assert _bits(tr) == g["fit3_trans_bits"]
        assert _bits([st.Evaluated.Value]) == [g["fit3_value_bits"]]
        assert _bits(st.Evaluated.Gradient) == g["fit3_gradient_bits"]
        assert _bits([st.Evaluated.DistRMS]) == [g["fit3_dist_rms_bits"]]
    assert max(alone) < 189 // 2, alone   # of 9 rows x 7 later chunks x 3 steps = 189 waits per slot
