"""The certified-terms step (csrc/icp.hip, enqueue_corr; csrc/strict.hip, strict_sum_kernel<., ., true>): from a Fit's
K-th Evaluate on a strict session launches no grid pass -- the summary kernel tests every pair against its partner's
certificate and searches the rest itself.  Every Fit here is the oracle's bit for bit, with the path on, off
(PCGX_ICP_FUSED_FROM=0), with searches forced inside the summary kernel (PCGX_TEST_ICP_FUSED_SEARCH) and with a forced
GRID_WALK there (PCGX_TEST_ICP_FUSED_GRID_WALK: the step is enqueued again with the grid pass and the walk).  The knobs
are read once per process: every configuration runs in a process of its own.

Debug counters (pcgx_debug_icp_strict_stats): [47] low word = certified steps, high word = those of them that met a
target the grid could not answer; [59] = targets searched inside certified steps."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import oracle as O
from pcgol_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = 123_457  # (not a multiple of 4, nor of a tile's 2048 targets)

_SCRIPT = textwrap.dedent("""
    import json, sys
    import numpy as np
    from pcgol_amd import icp, kdtree
    sys.path.insert(0, %(tests)r)
    import test_gpu_icp_certified_terms as T

    def out(s):
        tr, st, _ = s.result()
        return dict(trans=np.asarray(tr, np.float32).ravel().tobytes().hex(), n=int(st.NumIteration),
                    value=float(np.float32(st.Evaluated.Value)),
                    grad=np.asarray(st.Evaluated.Gradient, np.float32).tobytes().hex())

    def counters(s):
        st = np.asarray(s.strict_stats(), np.int64)
        return dict(fused=int(st[47]) & 0xffffffff, replayed=int(st[47]) >> 32, searched=int(st[59]), gave_up=int(st[63]))

    res = {}
    for name in %(cases)r:
        c = T.case(name)
        t = kdtree.New(c["base"])
        s = icp.IcpSession(t, c["target"], c["max_dist"], c["min_pairs"], c["weight"], c["threshold"], c["max_iteration"])
        s.set_strict(True)
        r = {}
        if name == "sequence":
            for _ in range(7):
                s.step()
            s.read_sums()
            for _ in range(c["max_iteration"] - 7):
                s.step()
            r["first"] = out(s)
            s.reset()                           # a second Fit: iterations 0 and 1 through the grid pass again
            for _ in range(5):
                s.step()
            r["five"] = out(s)
            for _ in range(c["max_iteration"] - 5):
                s.step()
            r["second"] = out(s)
            s.set_pose(np.frombuffer(bytes.fromhex(r["five"]["trans"]), np.float32).reshape(4, 4), 5)
            for _ in range(c["max_iteration"] - 5):
                s.step()
            r["resumed"] = out(s)
        else:
            for _ in range(c["max_iteration"]):
                s.step()
            r["fit"] = out(s)
        r["counters"] = counters(s)
        r["grid_stats"] = [int(v) for v in s.grid_stats()]
        s.close()
        res[name] = r
    print("RESULT " + json.dumps(res))
""")


def case(name):
    if name == "c4":
        return synth.c4_icp()
    if name in ("ragged", "sequence"):
        return synth.c4_icp(n=RAGGED, width=10.0 * (RAGGED / 1e6) ** (1 / 3))
    if name == "far":  # MaxDist below the points' spacing: a share of the targets has no partner within it
        c = synth.c4_icp(n=RAGGED, width=10.0 * (RAGGED / 1e6) ** (1 / 3))
        c["max_dist"] = 0.05
        return c
    if name == "twins":  # twins and a lattice patch: exact ties, which the grid leaves to the tree walk
        rng = np.random.default_rng(3)
        base = np.concatenate([
            synth.uniform_cloud(60_000, 4.0, 21),
            np.stack(np.meshgrid(*[np.arange(10, dtype=np.float32) * np.float32(0.0625) + np.float32(1.0)] * 3), -1).reshape(-1, 3),
        ]).astype(np.float32)
        base = np.ascontiguousarray(np.concatenate([base, base[:200]]))
        target = synth.transform_points(synth.icp_pose(), base[rng.permutation(len(base))[:50_001]])
        return dict(base=base, target=np.ascontiguousarray(target), max_dist=0.5, min_pairs=6,
                    weight=np.full(6, 0.3, np.float32), threshold=np.full(6, -1.0, np.float32), max_iteration=12)
    raise KeyError(name)


_oracle_cache = {}


def oracle(name, iters=None):
    key = (name, iters)
    if key not in _oracle_cache:
        c = case(name)
        o = O.icp_fit(O.KDTree(c["base"]), c["target"], c["max_dist"], c["min_pairs"], c["weight"], c["threshold"],
                      iters or c["max_iteration"], sums_mode=0)
        _oracle_cache[key] = o
    return _oracle_cache[key]


def run(cases, **knobs):
    env = dict(os.environ, **{k: str(v) for k, v in knobs.items()})
    code = _SCRIPT % dict(tests=os.path.join(ROOT, "tests"), cases=list(cases))
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r)\n" % ROOT + code], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):]), r.stderr


def assert_oracle(got, o):
    assert got["n"] == o["num_iteration"], (got["n"], o["num_iteration"])
    assert np.array_equal(np.frombuffer(bytes.fromhex(got["trans"]), np.float32), np.asarray(o["trans"], np.float32).ravel())
    assert np.float32(got["value"]) == np.float32(o["value"])
    assert np.array_equal(np.frombuffer(bytes.fromhex(got["grad"]), np.float32), np.asarray(o["gradient"], np.float32))


def assert_sequence(r):
    assert_oracle(r["first"], oracle("sequence"))
    assert_oracle(r["second"], oracle("sequence"))
    assert r["five"]["n"] == 5  # (its pose: the session that never certified has the same, the caller compares)
    # (set_pose starts the device's count at 0: the fifteen steps after it are the oracle's last fifteen)
    assert r["resumed"]["trans"] == r["first"]["trans"] and r["resumed"]["n"] == 15


CASES = ["c4", "ragged", "far", "twins", "sequence"]


@pytest.fixture(scope="module")
def unfused():
    return run(CASES, PCGX_ICP_FUSED_FROM=0)[0]


def test_certified_steps_equal_the_oracle_and_the_grid_pass(unfused):
    on, _ = run(CASES)
    for name in CASES:
        a, b = on[name], unfused[name]
        if name == "sequence":
            assert_sequence(a)
            assert_sequence(b)
            assert all(a[k] == b[k] for k in ("first", "five", "second", "resumed"))
        else:
            assert_oracle(a["fit"], oracle(name))
            assert a["fit"] == b["fit"], name
        assert b["counters"]["fused"] == 0, (name, b["counters"])
        # every Evaluate from the third on was a certified one (K = 2), none was enqueued again
        iters = case(name)["max_iteration"]
        # (sequence: the first Fit, the second -- reset, five steps, result(), fifteen more -- and fifteen behind set_pose)
        # (twins: the grid pass of iteration 1 already leaves the tied targets to the walk -- settle() puts the session on
        # the grid pass and the walk before any certified step)
        want = {"sequence": (iters - 2) + (iters - 2) + (iters - 5 - 2), "twins": 0}.get(name, iters - 2)
        assert a["counters"]["fused"] == want and a["counters"]["replayed"] == 0, (name, a["counters"])
        assert a["counters"]["gave_up"] == 0 and b["counters"]["gave_up"] == 0
        assert (a["counters"]["searched"] > 0) == (want > 0), (name, a["counters"])
        # the session-order records the certified steps kept are the grid pass's: the same trace
        assert a["grid_stats"] == b["grid_stats"], (name, a["grid_stats"], b["grid_stats"])


def test_searches_forced_inside_the_summary_kernel(unfused):
    cases = ["ragged", "sequence"]
    got, _ = run(cases, PCGX_TEST_ICP_FUSED_SEARCH=97)
    assert_oracle(got["ragged"]["fit"], oracle("ragged"))
    assert_sequence(got["sequence"])
    for name in cases:
        ctr = got[name]["counters"]
        assert ctr["fused"] > 0 and ctr["replayed"] == 0 and ctr["gave_up"] == 0, ctr
        assert ctr["searched"] >= ctr["fused"] * (RAGGED // 97), ctr
        assert got[name]["grid_stats"] == unfused[name]["grid_stats"], name


def test_a_grid_walk_inside_the_summary_kernel_enqueues_the_step_again():
    cases = ["ragged", "twins", "sequence"]
    got, err = run(cases, PCGX_TEST_ICP_FUSED_GRID_WALK=100_003, PCGX_ICP_SPEC_TRACE=1)
    assert_oracle(got["ragged"]["fit"], oracle("ragged"))
    assert_oracle(got["twins"]["fit"], oracle("twins"))
    assert_sequence(got["sequence"])
    for name in cases:
        # the first certified step (target 0 is forced) is enqueued again, and the session leaves the path (the steps
        # enqueued behind it return at once: `done`)
        want = 0 if name == "twins" else 1  # (twins: the grid pass met the ties first)
        assert got[name]["counters"]["fused"] <= want and got[name]["counters"]["replayed"] == want, (name, got[name]["counters"])
        assert got[name]["counters"]["gave_up"] == 0
    assert err.count("enqueued again") == len(cases), err[-3000:]
