"""Level 2 of the ICP loop's certificates (csrc/knn_grid.hip, grid_cert_kernel; csrc/strict.hip, certified_level2): a
pair that fails its partner's certificate is kept, or flipped to the partner's nearest other point n1, on the partner's
runner-up record {n1, cert2} -- without a search -- where its DistSq is below cert2; the rest is searched as before.

The cloud is built for the edges: uniform points, close pairs (a companion at 1 to 5 mm), triples (two companions
within 5 mm: cert2 fails too, a search remains), exact twins and a lattice patch (exact ties for n1 and for rho2).  The
Fit starts 27 mm off (synth.icp_pose), so targets cross the bisectors between a point and its companion on the way in:
flips.  tools/cert2_probe.py --cloud edges shows the same on the CPU (keeps, flips and searches all above zero, seed 11).
Twins and lattice points are in the base, not among the targets: a target that ties exactly is left to the tree walk by
the grid and takes the session off the certified steps altogether (tests/test_gpu_icp_certified_terms.py, `twins`).

Every Fit is the oracle's bit for bit: level 2 on (PCGX_ICP_CERT2=1, the default), off (0), certificates off (PCGX_ICP_CERT=0), searches
forced inside the summary kernel, a forced GRID_WALK there, every pair with a record (PCGX_GRID_RUNNER_BELOW=inf) and
a threshold that leaves half the close pairs without one.  The knobs are read once per process: a process per
configuration.

Counters: pcgx_debug_icp_strict_stats [59] = targets searched in certified steps; pcgx_debug_icp_runner_pairs counts =
{kept on level 2, flipped, all that failed level 1 while level 2 was on}."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import oracle as O
from pcgol_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11
NT = 6001        # three tiles of 2048, the last one ragged, not a multiple of 4
N_PAIRS = 400
N_TRIPLES = 120
N_TWINS = 50
HALF_BELOW = 0.031  # PCGX_GRID_RUNNER_BELOW that splits the close pairs: 0.031 cell edges of ~97 mm = 3 mm, companions at 1 to 5 mm


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def case(seed=SEED):
    rng = np.random.default_rng(seed)
    f32 = np.float32
    uni = synth.uniform_cloud(12_000, 2.0, seed)
    a = uni[:N_PAIRS]
    comp = (a + _unit(rng, N_PAIRS) * rng.uniform(1e-3, 5e-3, (N_PAIRS, 1))).astype(f32)
    b = uni[N_PAIRS:N_PAIRS + N_TRIPLES]
    tri1 = (b + _unit(rng, N_TRIPLES) * rng.uniform(1e-3, 5e-3, (N_TRIPLES, 1))).astype(f32)
    tri2 = (b + _unit(rng, N_TRIPLES) * rng.uniform(1e-3, 5e-3, (N_TRIPLES, 1))).astype(f32)
    twins = uni[1000:1000 + N_TWINS]
    lattice = (np.stack(np.meshgrid(*[np.arange(6, dtype=f32) * f32(0.03125) + f32(0.5)] * 3), -1).reshape(-1, 3)).astype(f32)
    base = np.ascontiguousarray(np.concatenate([uni, comp, tri1, tri2, twins, lattice]), dtype=f32)
    # targets: the points with companions, the companions, and uniform points (no twin, no lattice point)
    special = np.concatenate([np.arange(N_PAIRS + N_TRIPLES), 12_000 + np.arange(N_PAIRS + 2 * N_TRIPLES)])
    rest = 2000 + rng.permutation(10_000)[:NT - len(special)]
    sel = rng.permutation(np.concatenate([special, rest]))
    target = synth.transform_points(synth.icp_pose(), base[sel])
    return dict(base=base, target=np.ascontiguousarray(target), max_dist=0.5, min_pairs=6,
                weight=np.full(6, 0.3, f32), threshold=np.full(6, -1.0, f32), max_iteration=20,
                pairs_ids=np.arange(N_PAIRS), n_uniform=12_000)


_oracle = {}


def oracle():
    """The reference's Fit, Evaluate by Evaluate (the Stat's DistRMS and NumPairs are the last Evaluate's)."""
    if not _oracle:
        c = case()
        tree = O.KDTree(c["base"])
        trans, it, tt, ev = O.translate(0, 0, 0), 0, c["target"], None
        for _ in range(c["max_iteration"]):
            ev = O.icp_evaluate(tree, tt, c["max_dist"], c["min_pairs"])
            trans, _conv, it = O.icp_update(trans, ev["gradient"], it, c["weight"], c["threshold"], c["max_iteration"])
            tt = synth.transform_points(trans, c["target"])
        fit = O.icp_fit(tree, c["target"], c["max_dist"], c["min_pairs"], c["weight"], c["threshold"], c["max_iteration"])
        assert np.array_equal(np.asarray(trans, np.float32).ravel(), np.asarray(fit["trans"], np.float32).ravel())
        assert np.float32(ev["value"]) == np.float32(fit["value"])
        _oracle.update(trans=np.asarray(trans, np.float32).ravel(), value=np.float32(ev["value"]),
                       gradient=np.asarray(ev["gradient"], np.float32), dist_rms=np.float32(ev["dist_rms"]),
                       npairs=int(ev["npairs"]), n=int(fit["num_iteration"]))
    return _oracle


_SCRIPT = textwrap.dedent("""
    import json, sys
    import numpy as np
    from pcgol_amd import icp, kdtree, _lib as L
    sys.path.insert(0, %(tests)r)
    import test_gpu_icp_cert2 as T

    def out(s):
        tr, st, _ = s.result()
        e = st.Evaluated
        return dict(trans=np.asarray(tr, np.float32).ravel().tobytes().hex(), n=int(st.NumIteration),
                    value=np.float32(e.Value).tobytes().hex(), grad=np.asarray(e.Gradient, np.float32).tobytes().hex(),
                    dist_rms=np.float32(e.DistRMS).tobytes().hex(), npairs=int(e.NumPairs))

    def counters(s):
        st = np.asarray(s.strict_stats(), np.int64)
        l2 = np.zeros(3, np.int64)   # (a session without runner words, level 2 off: PCGX_E_INVALID, and nothing counted)
        L.lib().pcgx_debug_icp_runner_pairs(s._h, None, None, None, None, 0, L.ptr(l2))
        return dict(fused=int(st[47]) & 0xffffffff, replayed=int(st[47]) >> 32, searched=int(st[59]), gave_up=int(st[63]),
                    keeps=int(l2[0]), flips=int(l2[1]), fails=int(l2[2]))

    c = T.case()
    base, n, nt = c["base"], len(c["base"]), len(c["target"])
    t = kdtree.New(base)
    cert, runner, runner_id, below = np.empty(n, np.float32), np.empty((n, 4), np.float32), np.empty(n, np.uint32), np.zeros(1, np.float32)
    L.check(L.lib().pcgx_debug_grid_cert(t._h, L.ptr(cert), n))
    L.check(L.lib().pcgx_debug_grid_runner(t._h, L.ptr(runner), L.ptr(runner_id), L.ptr(below), n))
    s = icp.IcpSession(t, c["target"], c["max_dist"], c["min_pairs"], c["weight"], c["threshold"], c["max_iteration"])
    s.set_strict(True)
    r = dict(below=float(below[0]), pairs_below=int(np.sum(cert[c["pairs_ids"]] < below[0])))
    for name in ("first", "second"):
        for _ in range(c["max_iteration"]):
            s.step()
        r[name] = out(s)
        r[name + "_counters"] = counters(s)
        s.reset()                                # (the second Fit: Evaluates 0 and 1 through the grid pass again)
    # the invariant: every pair under the threshold carries its partner's runner words (the partner: by brute force)
    for _ in range(c["max_iteration"]):
        s.step()
    mc, rc, ric = np.empty((nt, 4), np.float32), np.empty((nt, 4), np.float32), np.empty(nt, np.uint32)
    have = L.lib().pcgx_debug_icp_runner_pairs(s._h, None, L.ptr(mc), L.ptr(rc), L.ptr(ric), nt, None) == 0
    checked, bad = 0, []
    for i in np.nonzero((mc[:, 3] >= 0) & (mc[:, 3] < below[0]))[0] if have else []:
        ids = np.nonzero(np.all(base == mc[i, :3], axis=1))[0]      # (more than one: twins)
        ok = any(mc[i, 3] == cert[j] and rc[i].tobytes() == runner[j].tobytes() and ric[i] == runner_id[j] for j in ids)
        checked += 1
        if not ok:
            bad.append(int(i))
    r["invariant"] = dict(pairs=int(np.sum(mc[:, 3] >= 0)), checked=checked, bad=bad[:8])
    s.close()
    print("RESULT " + json.dumps(r))
""")


def run(**knobs):
    knobs.setdefault("PCGX_ICP_CERT2", 1)
    env = dict(os.environ, **{k: str(v) for k, v in knobs.items()})
    code = _SCRIPT % dict(tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r)\n" % ROOT + code], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def assert_oracle(got):
    o = oracle()
    assert got["n"] == o["n"], (got["n"], o["n"])
    assert np.array_equal(np.frombuffer(bytes.fromhex(got["trans"]), np.float32), o["trans"])
    assert np.frombuffer(bytes.fromhex(got["value"]), np.float32)[0] == o["value"]
    assert np.array_equal(np.frombuffer(bytes.fromhex(got["grad"]), np.float32), o["gradient"])
    assert np.frombuffer(bytes.fromhex(got["dist_rms"]), np.float32)[0] == o["dist_rms"]
    assert got["npairs"] == o["npairs"], (got["npairs"], o["npairs"])


def assert_invariant(r):
    inv = r["invariant"]
    assert inv["checked"] > 0 and inv["bad"] == [], inv


@pytest.fixture(scope="module")
def default_run():
    return run()


@pytest.mark.gpu
def test_level2_keeps_flips_and_searches_and_the_fit_is_the_oracles(default_run):
    r = default_run
    for name in ("first", "second"):
        assert_oracle(r[name])
        ctr = r[name + "_counters"]
        print(name, ctr)
        assert ctr["fused"] == case()["max_iteration"] - 2 and ctr["replayed"] == 0 and ctr["gave_up"] == 0, ctr
        assert ctr["keeps"] + ctr["flips"] + ctr["searched"] == ctr["fails"], ctr
        assert ctr["keeps"] > 0 and ctr["flips"] > 0 and ctr["searched"] > 0, ctr
    assert r["first"] == r["second"] and r["first_counters"] == r["second_counters"]
    assert_invariant(r)


@pytest.mark.gpu
def test_level2_off_and_certificates_off_give_the_same_bits(default_run):
    off = run(PCGX_ICP_CERT2=0)
    none = run(PCGX_ICP_CERT=0)
    for r in (off, none):
        assert r["first"] == default_run["first"] and r["second"] == default_run["second"]
    ctr, on = off["first_counters"], default_run["first_counters"]
    print(ctr, none["first_counters"])
    # level 2 off: what it kept and flipped is searched (the counts of the library before level 2)
    assert ctr["keeps"] == 0 and ctr["flips"] == 0 and ctr["fails"] == 0 and ctr["searched"] == on["fails"], (ctr, on)
    assert ctr["fused"] == on["fused"]
    assert none["first_counters"]["fused"] == 0 and none["first_counters"]["keeps"] == 0 and none["first_counters"]["flips"] == 0


@pytest.mark.gpu
def test_level2_beside_forced_searches_and_a_forced_grid_walk(default_run):
    forced = run(PCGX_TEST_ICP_FUSED_SEARCH=7)
    assert forced["first"] == default_run["first"] and forced["second"] == default_run["second"]
    ctr = forced["first_counters"]
    print(ctr)
    assert ctr["fused"] > 0 and ctr["replayed"] == 0 and ctr["gave_up"] == 0, ctr
    assert ctr["searched"] >= ctr["fused"] * (NT // 7) and ctr["keeps"] > 0 and ctr["flips"] > 0, ctr  # (a forced target is searched)
    assert ctr["keeps"] + ctr["flips"] + ctr["searched"] == ctr["fails"], ctr
    assert_invariant(forced)
    # a GRID_WALK inside the summary kernel: the step is enqueued again with the grid pass and the walk (settle()), which
    # find the runner words in place and leave them in place
    walk = run(PCGX_TEST_ICP_FUSED_GRID_WALK=1009)
    assert walk["first"] == default_run["first"] and walk["second"] == default_run["second"]
    assert walk["first_counters"]["replayed"] == 1 and walk["first_counters"]["gave_up"] == 0, walk["first_counters"]


@pytest.mark.gpu
def test_level2_with_every_pair_and_with_half_the_close_pairs_under_the_threshold(default_run):
    every = run(PCGX_GRID_RUNNER_BELOW="inf")
    half = run(PCGX_GRID_RUNNER_BELOW=HALF_BELOW)
    assert every["below"] == float("inf")
    assert N_PAIRS // 4 < half["pairs_below"] < 3 * N_PAIRS // 4, half["pairs_below"]   # (half the close pairs, roughly)
    assert default_run["pairs_below"] == N_PAIRS
    for r in (every, half):
        assert r["first"] == default_run["first"] and r["second"] == default_run["second"]
        ctr = r["first_counters"]
        print(r["below"], ctr)
        assert ctr["keeps"] + ctr["flips"] + ctr["searched"] == ctr["fails"] == default_run["first_counters"]["fails"], ctr
        assert ctr["keeps"] > 0 and ctr["searched"] > 0, ctr
        assert_invariant(r)
    # a lower threshold leaves more to the searches, a higher one no more than the default's
    assert half["first_counters"]["searched"] > default_run["first_counters"]["searched"]
    assert every["first_counters"]["searched"] <= default_run["first_counters"]["searched"]
    assert every["invariant"]["checked"] == every["invariant"]["pairs"]


@pytest.mark.gpu
def test_runner_records_against_brute_force():
    """runner, runner_id and cert2 on the edge cloud, in float32 as the kernel computes them: n1 at the smallest computed
    DistSq to another point, cert2 no larger than 0.24 times the second-smallest one (twins and lattice ties included)."""
    from pcgol_amd import _lib as L, kdtree
    c = case()
    base, n = c["base"], len(c["base"])
    t = kdtree.New(base)
    cert, runner, runner_id, below = np.empty(n, np.float32), np.empty((n, 4), np.float32), np.empty(n, np.uint32), np.zeros(1, np.float32)
    L.check(L.lib().pcgx_debug_grid_cert(t._h, L.ptr(cert), n))
    L.check(L.lib().pcgx_debug_grid_runner(t._h, L.ptr(runner), L.ptr(runner_id), L.ptr(below), n))
    geom, dims = np.zeros(5, np.float32), np.zeros(3, np.int32)
    L.check(L.lib().pcgx_debug_grid_geometry(t._h, L.ptr(geom), L.ptr(dims)))
    h = float(geom[3])
    assert below[0] == np.float32(0.24) * (np.float32(0.22) * geom[3]) * (np.float32(0.22) * geom[3])
    d1, d2 = np.empty(n, np.float32), np.empty(n, np.float32)
    for i0 in range(0, n, 1024):   # the kernel's expression, (dx dx + dy dy) + dz dz in float32, o - p
        p = base[i0:i0 + 1024]
        d = base[None, :, :] - p[:, None, :]
        dsq = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        dsq[np.arange(len(p)), i0 + np.arange(len(p))] = np.inf
        two = np.partition(dsq, 1, axis=1)[:, :2]
        d1[i0:i0 + 1024], d2[i0:i0 + 1024] = two[:, 0], two[:, 1]
    assert np.all(runner_id < n)
    n1 = base[runner_id]
    has = runner[:, 3] > 0
    # n1: the record's point is the id's, and it lies at the smallest computed DistSq (any of the ties)
    assert np.array_equal(runner[has, :3], n1[has])
    dd = n1 - base
    dn1 = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
    near = d1 < np.float32((0.99 * h) ** 2)          # (the nearest other point is inside the 27 cells for certain)
    assert np.all(runner_id[near] != np.arange(n)[near]) and np.array_equal(dn1[near], d1[near])
    # cert2 <= 0.24 rho2^2, cert2 >= cert, and exactly the kernel's value where the second-nearest is inside the 27 cells
    assert np.all(runner[:, 3] <= np.float32(0.24) * d2) and np.all(runner[:, 3] >= 0) and np.all(runner[near, 3] >= cert[near])
    near2 = d2 < np.float32((0.99 * h) ** 2) * np.float32(0.9)
    want = np.float32(0.24) * (d2 - np.float32(2.0e-6) * d2)
    assert np.array_equal(runner[near2, 3], want[near2]) and np.sum(near2) > n // 2
    # twins: cert 0 (never certified), a record all the same: n1 is the twin, cert2 from the next point
    tw = np.concatenate([1000 + np.arange(N_TWINS), n - 216 - N_TWINS + np.arange(N_TWINS)])
    assert np.all(cert[tw] == 0) and np.all(d1[tw] == 0) and np.array_equal(runner[tw, :3], base[tw]) and np.all(runner[tw, 3] > 0)
    # the lattice's inner points: six neighbours at one distance -- a tie for n1 is the second-smallest too: cert2 == cert
    lat = n - 216 + np.arange(216)
    tie = lat[d1[lat] == d2[lat]]
    assert len(tie) >= 64 and np.array_equal(runner[tie, 3], cert[tie])
    # triples: the second companion is within 5 mm as well
    tri = N_PAIRS + np.arange(N_TRIPLES)
    assert np.all(runner[tri, 3] <= np.float32(0.24 * 5.1e-3 ** 2))
