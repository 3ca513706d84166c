"""What the strict sums allocate and launch (csrc/strict_plan.h) is what the host side of strict.hip did at b14be59.

The header is compiled for the host with g++ (tests/cpp/strict_plan_host.cpp; it needs neither HIP nor the library) and
its three plans are compared, field by field, with restatements in numpy of pcgol_amd/csrc/strict.hip at commit b14be59,
where strict_create carved its block by hand, three enqueue functions each said which kernels run, and two of them
managed the shard block.  The line numbers beside the expressions are that file's.  Both sides are total functions:
combinations no entry point produces (a certified step of the ring form, rank 7 of a world of 2) are compared like the
others.  A kernel that does not run has grid 0; what a failed rank launches nothing with is not compared (`exchange`)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pcgol_amd", "csrc")

REGIONS = ("tile_sum", "tile_err", "tile_pub", "tile_arrived", "tile_pairs", "recs", "aux", "aux_terms", "jobs", "cand",
           "xyz_caller", "counters", "dbg", "stamps", "chunk_state")  # strict.hip 2753-2772: the order of the `p +=`
R = {name: i for i, name in enumerate(REGIONS)}
LAYOUT_OUT = (("ntiles", "ntiles_pad", "nchunks", "naux", "total") + tuple("off_" + r for r in REGIONS) +
              tuple("bytes_" + r for r in REGIONS) + tuple("create%d" % i for i in range(6)) + tuple("reset%d" % i for i in range(4)))
LAUNCH_IN = ("form", "exchange", "have_tile_sums", "first_iter", "certify", "pos_of", "naux", "ntiles", "nchunks", "nrows",
             "rank", "world", "spec_depth", "selfcheck", "spec_on", "repair_on", "local_failed", "fuse_update")
LAUNCH_OUT = ("live", "tilesum", "summary", "exchange", "bases_behind_summary", "ring_err_grid", "repair_grid", "jobs_grid",
              "chain", "chain_grid", "fuse_update")
ONE_GPU, COLLECTIVE, RING = 0, 1, 2
SUM_NONE, SUM_PLAIN, SUM_EXCHANGE, SUM_RING, SUM_CERTIFIED, SUM_ERROR = range(6)  # <false>, <true>, <true,true>, <true,false,true>
CHAIN_NONE, CHAIN_CHECK, CHAIN_SPEC, CHAIN_PLAIN = range(4)                         # <true,false>, <false,true>, <false,false>
# strict.hip / strict_terms.h / strict_sum.h at b14be59
K_ROWS, K_TILE, K_LANES, K_CHAIN_TILES, K_AUX_SHARDS, K_CAND, K_REPAIR_BLOCK, K_REPAIR_MIN, K_JOB_ROLES = 9, 2048, 64, 512, 64, 768, 512, 1024, 3
SIZEOF_TILEREC, SIZEOF_LEAFAUX, SIZEOF_JOBDESC = 64, 96, 16


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("strict_plan") / "libstrict_plan_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + CSRC, "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "strict_plan_host.cpp")])
    lib = ctypes.CDLL(so)
    rows = (ctypes.c_int32 * 6)()
    assert lib.strict_plan_rows(rows) == len(REGIONS)
    assert list(rows) == [2, len(LAYOUT_OUT), len(LAUNCH_IN), len(LAUNCH_OUT), 5, 4]
    return lib


def run(lib, fn, in_rows, n_out):
    rows = np.ascontiguousarray(np.stack([np.asarray(r, np.int64) for r in in_rows]))
    n = rows.shape[1]
    out = np.empty((n_out, n), np.int64)
    getattr(lib, fn)(rows.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(n), out.ctypes.data_as(ctypes.c_void_p))
    return out


def product(axes):
    grids = np.meshgrid(*[np.asarray(v, np.int64) for v in axes.values()], indexing="ij")
    return {k: g.ravel() for k, g in zip(axes, grids)}


def compare(got, want, cases, only=None):
    assert set(got) == set(want)
    for k in got:
        differ = np.asarray(got[k]) != np.asarray(want[k]).astype(np.int64)
        if only is not None and k in only:
            differ &= only[k]
        at = np.flatnonzero(differ)
        first = {name: int(v[at[0]]) for name, v in cases.items()} if len(at) else None
        assert len(at) == 0, "%s differs in %d of %d cases, first at %r" % (k, len(at), len(differ), first)


def test_the_facts_are_the_parents_constants(host):
    out = (ctypes.c_int64 * 12)()
    host.strict_plan_facts(out)
    assert list(out) == [K_ROWS, K_TILE, K_LANES, K_CHAIN_TILES, K_AUX_SHARDS, K_CAND, K_REPAIR_BLOCK, K_REPAIR_MIN, K_JOB_ROLES,
                         SIZEOF_TILEREC, SIZEOF_LEAFAUX, SIZEOF_JOBDESC]


# ---- the block -------------------------------------------------------------------------------------------------------

def parent_layout(c):
    """strict.hip at b14be59, strict_create (2712-2776), strict_reset (3128-3129), on arrays; slots -1: the variable is absent"""
    nt, slots = np.asarray(c["nt"], np.int64), np.asarray(c["slots_per_shard"], np.int64)
    up = lambda v: (v + 255) & ~np.int64(255)  # noqa: E731  (2718)
    ntiles = np.where(nt > 0, (nt + K_TILE - 1) // K_TILE, 1)                      # 2712
    sz = {}
    sz["tile_sum"] = sz["tile_err"] = up(K_ROWS * ntiles * 8)                      # 2719 (twice)
    sz["tile_pairs"] = up(ntiles * 4)                                              # 2720
    ntiles_pad = (ntiles + 127) & ~np.int64(127)                                   # 2721
    sz["tile_pub"] = up(ntiles_pad * 16 * 8)                                       # 2722
    n_groups = (ntiles + 31) // 32                                                 # 2723
    sz["tile_arrived"] = up((n_groups + (n_groups + 31) // 32) * 128)              # 2724
    sz["recs"] = up(K_ROWS * ntiles * SIZEOF_TILEREC)                              # 2727
    naux = K_AUX_SHARDS * ((K_ROWS * ntiles // 4 + K_AUX_SHARDS - 1) // K_AUX_SHARDS + 4)  # 2731
    naux = np.where((slots >= 0) & (slots * K_AUX_SHARDS < naux), slots * K_AUX_SHARDS, naux)  # 2732-2735
    sz["aux"] = up(naux * K_LANES * SIZEOF_LEAFAUX)                                # 2736
    sz["aux_terms"] = up(naux * K_TILE * 4)                                        # 2737
    sz["jobs"] = up(naux * SIZEOF_JOBDESC)                                         # 2738
    sz["cand"] = up(naux * K_CAND * 4)                                             # 2739
    sz["xyz_caller"] = up(np.where(nt != 0, nt, 1) * 12 + 64)                      # 2740
    sz["stamps"] = up(ntiles * 16 * 8)                                             # 2741
    sz["counters"] = 256 + K_AUX_SHARDS * 128 + 0 * nt                             # 2742
    nchunks = (ntiles + K_CHAIN_TILES - 1) // K_CHAIN_TILES                        # 2743
    sz["chunk_state"] = up(K_ROWS * nchunks * 16 * 8)                              # 2745
    sz["dbg"] = 512 + 0 * nt                                                       # 2746, 2770
    total = (2 * sz["tile_sum"] + sz["tile_pub"] + sz["tile_arrived"] + sz["tile_pairs"] + sz["recs"] + sz["aux"] + sz["aux_terms"] +
             sz["jobs"] + sz["cand"] + sz["xyz_caller"] + sz["counters"] + 512 + sz["stamps"] + sz["chunk_state"])  # 2746
    w = {"ntiles": ntiles, "ntiles_pad": ntiles_pad, "nchunks": nchunks, "naux": naux, "total": total}
    p = np.zeros_like(nt)
    for r in REGIONS:                                                              # 2752-2772
        w["off_" + r], w["bytes_" + r] = p, sz[r]
        p = p + sz[r]
    # 2774: counters, sz_ctr + 512 = counters and dbg; 2775: tile_arrived; 2776: chunk_state
    for i, r in enumerate(("counters", "dbg", "tile_arrived", "tile_arrived", "chunk_state", "chunk_state")):
        w["create%d" % i] = R[r] + 0 * nt
    for i, r in enumerate(("counters", "counters", "tile_arrived", "tile_arrived")):  # 3128, 3129 (2766, 2767)
        w["reset%d" % i] = R[r] + 0 * nt
    return w


LAYOUT_AXES = dict(nt=(0, 1, 2047, 2048, 2049, 65 * 2048, 2 ** 20, 2 ** 20 + 1, 8_000_000, 2 ** 31 - 1),
                   slots_per_shard=(-1, 0, 1, 10 ** 6))


def test_the_block_is_carved_as_the_parent_carved_it(host):
    c = product(LAYOUT_AXES)
    out = run(host, "strict_layout_cases", [c["nt"], c["slots_per_shard"]], len(LAYOUT_OUT))
    got = {k: out[i] for i, k in enumerate(LAYOUT_OUT)}
    compare(got, parent_layout(c), c)
    # regions are disjoint, ascending and 256-aligned, and the last ends at the total
    end = np.zeros_like(c["nt"])
    for r in REGIONS:
        assert np.all(got["off_" + r] == end) and np.all(got["off_" + r] % 256 == 0) and np.all(got["bytes_" + r] % 256 == 0), r
        assert np.all(got["bytes_" + r] > 0) or r in ("aux", "aux_terms", "jobs", "cand"), r
        end = end + got["bytes_" + r]
    assert np.all(end == got["total"])
    # the enumeration reaches the edges: one tile and two, one chunk and two, no slot at all, the cap not reached
    assert {1, 2, 65, 512, 513, 3907, 2 ** 20} <= set(got["ntiles"].tolist()) and {1, 2, 8, 2048} <= set(got["nchunks"].tolist())
    assert np.count_nonzero(got["naux"] == 0) == 10 and np.count_nonzero(got["naux"] == 64) == 10
    assert np.all(got["naux"][c["slots_per_shard"] == 10 ** 6] == got["naux"][c["slots_per_shard"] == -1])


def test_rows_of_the_block_a_reader_can_check_by_eye(host):
    out = run(host, "strict_layout_cases", [[1_000_000], [-1]], len(LAYOUT_OUT))
    g = {k: int(out[i, 0]) for i, k in enumerate(LAYOUT_OUT)}
    assert (g["ntiles"], g["ntiles_pad"], g["nchunks"], g["naux"]) == (489, 512, 1, 64 * (18 + 4))
    assert g["bytes_tile_sum"] == 35328 and g["bytes_recs"] == 9 * 489 * 64 + 192 and g["bytes_counters"] == 256 + 64 * 128
    assert g["off_dbg"] == g["off_counters"] + g["bytes_counters"] and g["bytes_dbg"] == 512
    assert [g["create%d" % i] for i in range(6)] == [11, 12, 3, 3, 14, 14] and [g["reset%d" % i] for i in range(4)] == [11, 11, 3, 3]


# ---- a step's launches -------------------------------------------------------------------------------------------------

def parent_launches(c):
    """strict.hip at b14be59: launch_chain (2823-2833), strict_enqueue (2835-2874), strict_enqueue_sharded (2943-3016),
    strict_enqueue_ring (3062-3123), on arrays"""
    b = {k: np.asarray(c[k]) != 0 for k in ("exchange", "have_tile_sums", "first_iter", "certify", "pos_of", "spec_on",
                                            "repair_on", "local_failed", "fuse_update")}
    form, naux, ntiles, nchunks, nrows, rank, world, depth = (np.asarray(c[k], np.int64) for k in (
        "form", "naux", "ntiles", "nchunks", "nrows", "rank", "world", "spec_depth"))
    one, coll, ring = form == ONE_GPU, form == COLLECTIVE, form == RING
    zero = np.zeros_like(form)
    # 2962-2964, 2975, 2983, 2991, 2996, 3005: a failed rank of the collective form launches none of these kernels;
    # 3077-3083: one of the ring form returns in front of all of them
    live = one | ~b["local_failed"]
    # strict_enqueue: 2847 the certified instantiation, 2850 the error, 2852 <true>, 2855 <false>
    summary_one = np.where(b["certify"] & b["exchange"] & ~b["pos_of"], SUM_CERTIFIED,
                           np.where(b["certify"], SUM_ERROR, np.where(b["exchange"], SUM_EXCHANGE, SUM_PLAIN)))
    summary = np.where(one, summary_one, np.where(coll, SUM_PLAIN, SUM_RING))      # 2986: <false>; 3100: <true, true>
    summary = np.where(live, summary, SUM_NONE)
    after = live & ~(one & (summary == SUM_ERROR))                                 # 2851: return fail(...)
    tilesum = np.where(one, ~b["have_tile_sums"] & ~b["exchange"], coll & live)    # 2840; 2977 (always); the ring form: none
    exchange = np.where(ring, 1, b["exchange"])                                    # 3097: W.exchange = 1; 2956: W as it is
    repair = b["first_iter"] & (naux > 0) & (ntiles >= K_REPAIR_MIN) & b["repair_on"] & ~coll & after  # 2862 = 3111; 2996-3000: none
    repair_grid = np.where(repair, nrows * ((ntiles + K_REPAIR_BLOCK - 1) // K_REPAIR_BLOCK), 0)       # 2863 = 3112
    jobs_grid = np.where((naux > 0) & after, K_JOB_ROLES * naux, 0)                # 2865-2866 = 2998-2999 = 3114-3115
    waits = np.where(ring, True, nchunks > 1)                                      # 2870, 3007: W.nchunks > 1; 3119: true
    w_rank = np.where(ring, rank, 0)                                               # 2828: W.ring ? W.rank : 0 (3086, 3091)
    spec = waits & b["spec_on"] & (w_rank * nchunks + nchunks - 1 >= depth)        # 2828
    chain = np.where((np.asarray(c["selfcheck"]) & 1) != 0, CHAIN_CHECK, np.where(spec, CHAIN_SPEC, CHAIN_PLAIN))  # 2826-2832
    return {
        "live": live, "tilesum": tilesum, "summary": summary, "exchange": exchange,
        "bases_behind_summary": ring & live & (rank > 0),                          # 3105-3108
        "ring_err_grid": np.where(ring & live & (world > 1), K_ROWS + (rank > 0), zero),  # 3103-3104
        "repair_grid": repair_grid, "jobs_grid": jobs_grid,
        "chain": np.where(after, chain, CHAIN_NONE),
        "chain_grid": np.where(after, nrows * nchunks, 0),                         # 2825
        "fuse_update": np.where(after, np.where(one, b["fuse_update"], ring), 0),  # 2870: the caller's; 3007: 0; 3119: 1
    }


LAUNCH_AXES = dict(exchange=(0, 1), have_tile_sums=(0, 1), first_iter=(0, 1), certify=(0, 1), pos_of=(0, 1), naux=(0, 64),
                   ntiles=(1, 512, 513, 1023, 1024, 2048, 2049, 3907), nrows=(8, 9), rank=(0, 1, 7), world=(1, 2, 8),
                   spec_depth=(0, 4, 100), selfcheck=(0, 1), spec_on=(0, 1), repair_on=(0, 1), local_failed=(0, 1))


def launches(lib, c):
    out = run(lib, "strict_launch_cases", [c[k] for k in LAUNCH_IN], len(LAUNCH_OUT))
    return {k: out[i] for i, k in enumerate(LAUNCH_OUT)}


@pytest.mark.parametrize("form", [ONE_GPU, COLLECTIVE, RING])
def test_every_step_launches_what_the_parent_launched(host, form):
    seen = 0
    for fuse in (0, 1):  # (the product in slices: a third of a million cases at a time)
        c = product(dict(LAUNCH_AXES, form=(form,), fuse_update=(fuse,)))
        c["nchunks"] = (c["ntiles"] + K_CHAIN_TILES - 1) // K_CHAIN_TILES  # as the layout has it (2743)
        got, want = launches(host, c), parent_launches(c)
        compare(got, want, c, only={"exchange": got["live"] != 0})
        seen += len(c["form"])
        count = lambda m: int(np.count_nonzero(m))  # noqa: E731
        # the enumeration reaches both sides of every decision (conditions on the cases, not measurements)
        assert count(got["chain"] == CHAIN_CHECK) > 0 and count(got["chain"] == CHAIN_SPEC) > 0 and count(got["chain"] == CHAIN_PLAIN) > 0
        assert count(got["jobs_grid"] == 192) > 0 and count((got["jobs_grid"] == 0) & (got["live"] != 0)) > 0
        if form == ONE_GPU:
            assert sorted(set(got["summary"].tolist())) == [SUM_PLAIN, SUM_EXCHANGE, SUM_CERTIFIED, SUM_ERROR]
            assert count(got["live"] == 0) == 0 and count((got["summary"] == SUM_ERROR) & (got["chain"] != CHAIN_NONE)) == 0
            assert count(got["fuse_update"] == fuse) == count(got["summary"] != SUM_ERROR) if fuse else count(got["fuse_update"]) == 0
        if form != COLLECTIVE:
            for ntiles in (1023, 1024):  # kRepairMinTiles
                assert (count((c["ntiles"] == ntiles) & (got["repair_grid"] > 0)) > 0) == (ntiles == 1024)
            assert count(got["repair_grid"] == 9 * 8) > 0 and count(got["repair_grid"] == 8 * 5) > 0   # 3907 and 2049 tiles
        else:
            assert count(got["repair_grid"]) == 0 and count(got["tilesum"] != got["live"]) == 0
            assert sorted(set(got["summary"].tolist())) == [SUM_NONE, SUM_PLAIN] and count(got["fuse_update"]) == 0
            assert count((got["exchange"] == 0) & (got["live"] != 0)) > 0  # handed on unchanged
        if form == RING:
            assert count(got["tilesum"]) == 0 and count((got["exchange"] != 1) & (got["live"] != 0)) == 0
            assert sorted(set(got["ring_err_grid"].tolist())) == [0, 9, 10]
            assert count((got["chain"] == CHAIN_SPEC) & (c["nchunks"] == 1) & (c["rank"] > 0)) > 0  # a rank behind another waits
            assert count((got["live"] == 0) & ((got["summary"] != SUM_NONE) | (got["chain"] != CHAIN_NONE) | (got["jobs_grid"] > 0))) == 0
        else:
            assert count((got["chain"] == CHAIN_SPEC) & (c["nchunks"] == 1)) == 0
    assert seen == 2 * 2 ** 5 * 2 * 8 * 2 * 3 ** 3 * 2 ** 4 == 442_368 * 2


def test_steps_a_reader_can_check_by_eye(host):
    def one(**facts):
        c = dict(form=ONE_GPU, exchange=1, have_tile_sums=0, first_iter=0, certify=0, pos_of=1, naux=1408, ntiles=489, nchunks=1,
                 nrows=8, rank=0, world=1, spec_depth=4, selfcheck=0, spec_on=1, repair_on=1, local_failed=0, fuse_update=1)
        c.update(facts)
        return {k: int(v[0]) for k, v in launches(host, {k: [v] for k, v in c.items()}).items()}

    # the C4 step: the summaries with their own exchange, the jobs, one chunk of the plain chain kernel with the update
    assert one() == dict(live=1, tilesum=0, summary=SUM_EXCHANGE, exchange=1, bases_behind_summary=0, ring_err_grid=0,
                         repair_grid=0, jobs_grid=3 * 1408, chain=CHAIN_PLAIN, chain_grid=8, fuse_update=1)
    assert one(certify=1, pos_of=0)["summary"] == SUM_CERTIFIED and one(certify=1)["summary"] == SUM_ERROR
    assert one(exchange=0)["tilesum"] == 1 and one(exchange=0, have_tile_sums=1)["tilesum"] == 0
    # C5's 3907 tiles: eight chunks, the walk-ahead instantiation, the repair pass in a Fit's first step
    c5 = one(ntiles=3907, nchunks=8, nrows=9, first_iter=1)
    assert (c5["chain"], c5["chain_grid"], c5["repair_grid"]) == (CHAIN_SPEC, 72, 72)
    assert [one(ntiles=512 * k, nchunks=k)["chain"] for k in (4, 5)] == [CHAIN_PLAIN, CHAIN_SPEC]  # spec_depth 4
    assert one(ntiles=3907, nchunks=8, spec_on=0)["chain"] == CHAIN_PLAIN and one(selfcheck=1)["chain"] == CHAIN_CHECK
    ring = one(form=RING, rank=1, world=2, exchange=0, first_iter=1, ntiles=1024, nchunks=2)
    assert ring == dict(live=1, tilesum=0, summary=SUM_RING, exchange=1, bases_behind_summary=1, ring_err_grid=10,
                        repair_grid=16, jobs_grid=3 * 1408, chain=CHAIN_PLAIN, chain_grid=16, fuse_update=1)
    assert one(form=RING, rank=1, world=2, ntiles=1024, nchunks=2, spec_depth=3)["chain"] == CHAIN_SPEC  # 1 * 2 + 1 walks in front
    assert one(form=COLLECTIVE, rank=1, world=2, first_iter=1, ntiles=1024, nchunks=2) == dict(
        live=1, tilesum=1, summary=SUM_PLAIN, exchange=1, bases_behind_summary=0, ring_err_grid=0, repair_grid=0,
        jobs_grid=3 * 1408, chain=CHAIN_PLAIN, chain_grid=16, fuse_update=0)


# ---- the block a sharded step exchanges through ---------------------------------------------------------------------

def test_the_shard_block_over_its_whole_input_space(host):
    c = product(dict(have_block=(0, 1), block_world=(1, 2, 3, 8), block_ring=(0, 1), world=(1, 2, 3, 8), want_ring=(0, 1)))
    out = run(host, "strict_shard_cases", [c[k] for k in ("have_block", "block_world", "block_ring", "world", "want_ring")], 4)
    got = dict(zip(("allocate", "zero", "bytes", "ring"), out))
    have, ring, want_ring = c["have_block"] != 0, c["block_ring"] != 0, c["want_ring"] != 0
    nbytes = (c["world"] + 4) * 16 * 8                # 2948 = 3070
    fresh = ~have | (c["block_world"] != c["world"])  # 2945 = 3067: !b->shard || b->shard_world != world
    # strict_enqueue_sharded (2945-2952): free and allocate, never zero, shard_ring = false
    collective = {"allocate": fresh, "zero": np.zeros_like(fresh), "bytes": nbytes, "ring": np.zeros_like(fresh)}
    # strict_enqueue_ring (3066-3076): behind `... || !b->shard_ring` maybe allocate (3067-3073), zero (3074), shard_ring = true
    # (3075); else the block is left as it is, shard_ring is true already
    ring_form = {"allocate": fresh, "zero": fresh | ~ring, "bytes": nbytes, "ring": np.ones_like(fresh)}
    want = {k: np.where(want_ring, ring_form[k], collective[k]) for k in collective}
    compare(got, want, c)
    assert len(c["world"]) == 128 and np.count_nonzero(got["zero"] & ~got["allocate"]) == 4  # a collective block of this world taken over
