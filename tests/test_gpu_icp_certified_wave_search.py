"""The certified step's searches, wave by wave (csrc/strict.hip, certified_wave_search): a wave of the summary kernel
numbers its own targets whose certificate did not hold -- a ballot per slot of the lanes' quads -- and searches them in
rounds of 64, an item a lane, with the operands taken from the owner lanes by shuffles and the answers handed back the
same way.  The knobs of tests/test_gpu_icp_certified_terms.py drive every shape of that: all four slots of every lane
(four full rounds a wave), partial rounds, items spread over slots and lanes, waves with one item next to waves with none,
searches that find nothing and a forced GRID_WALK.  Every Fit is the oracle's bit for bit (trans, Value, Gradient,
NumIteration) and equal to a run that never certifies (PCGX_ICP_FUSED_FROM=0).

Not covered: a GRID_WALK that the wave search meets by itself.  The "twins" case has exact ties, but the grid pass of
iteration 1 meets them first and settle() puts the session on the grid pass and the walk before any certified step
(fused == 0, asserted below): that Fit checks the way OUT of the path with the search knob set, not the wave search.

The clouds are small: 6151 targets are three full tiles of 2048 and a ragged one of 7 (not a multiple of 4 either).
The knobs are read once per process: every configuration runs in a process of its own.

The binding has no call that reads the session-order pairs; what a later grid pass would read of them is compared
through grid_stats() (the NEXT grid pass's trace over the session-order records and certificates)."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from pcgol_amd import synth
import test_gpu_icp_certified_terms as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = 6151  # 3 x 2048 + 7

_SCRIPT = textwrap.dedent("""
    import json, sys
    import numpy as np
    from pcgol_amd import icp, kdtree
    sys.path.insert(0, %(tests)r)
    import test_gpu_icp_certified_wave_search as W

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
        c = W.case(name)
        t = kdtree.New(c["base"])
        s = icp.IcpSession(t, c["target"], c["max_dist"], c["min_pairs"], c["weight"], c["threshold"], c["max_iteration"])
        s.set_strict(True)
        r = {}
        if name == "refit":
            for _ in range(c["max_iteration"]):
                s.step()
            s.reset()                           # nothing has looked at the first Fit: its speculated steps are pending
            for _ in range(c["max_iteration"]):
                s.step()
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
    if name in ("small", "refit"):
        return synth.c4_icp(n=SMALL, width=10.0 * (SMALL / 1e6) ** (1 / 3))
    if name == "far":  # MaxDist below the points' spacing: many searches find nothing
        c = synth.c4_icp(n=SMALL, width=10.0 * (SMALL / 1e6) ** (1 / 3))
        c["max_dist"] = 0.05
        return c
    if name == "twins":  # exact ties, which the grid leaves to the tree walk (the existing file's case and size)
        return T.case("twins")
    raise KeyError(name)


_oracle_cache = {}


def oracle(name):
    if name == "twins":
        return T.oracle("twins")
    key = "small" if name == "refit" else name
    if key not in _oracle_cache:
        import oracle as O
        c = case(key)
        _oracle_cache[key] = O.icp_fit(O.KDTree(c["base"]), c["target"], c["max_dist"], c["min_pairs"], c["weight"],
                                       c["threshold"], c["max_iteration"], sums_mode=0)
    return _oracle_cache[key]


def run(cases, **knobs):
    env = dict(os.environ, **{k: str(v) for k, v in knobs.items()})
    code = _SCRIPT % dict(tests=os.path.join(ROOT, "tests"), cases=list(cases))
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r)\n" % ROOT + code], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.fixture(scope="module")
def unfused():
    got = run(["small", "far", "twins"], PCGX_ICP_FUSED_FROM=0)
    for name, r in got.items():
        T.assert_oracle(r["fit"], oracle(name))
        assert r["counters"]["fused"] == 0 and r["counters"]["gave_up"] == 0, (name, r["counters"])
    return got


def test_every_target_searched_four_full_rounds_a_wave(unfused):
    got = run(["small", "far"], PCGX_TEST_ICP_FUSED_SEARCH=1)
    for name in ("small", "far"):  # (far: the no-pair path -- w = -1, terms -0.0f, the pair count)
        r = got[name]
        T.assert_oracle(r["fit"], oracle(name))
        assert r["fit"] == unfused[name]["fit"], name
        ctr = r["counters"]
        assert ctr["fused"] == case(name)["max_iteration"] - 2, ctr
        assert ctr["searched"] == ctr["fused"] * SMALL and ctr["replayed"] == 0 and ctr["gave_up"] == 0, ctr
        assert r["grid_stats"] == unfused[name]["grid_stats"], name


@pytest.mark.parametrize("every", [3, 7, 64, 257])
def test_partial_rounds_and_items_spread_over_slots_and_lanes(unfused, every):
    r = run(["small"], PCGX_TEST_ICP_FUSED_SEARCH=every)["small"]
    T.assert_oracle(r["fit"], oracle("small"))
    assert r["fit"] == unfused["small"]["fit"]
    ctr = r["counters"]
    assert ctr["fused"] == case("small")["max_iteration"] - 2 and ctr["replayed"] == 0 and ctr["gave_up"] == 0, ctr
    assert ctr["searched"] >= ctr["fused"] * ((SMALL + every - 1) // every), ctr  # (the forced ones, index 0 included)
    assert r["grid_stats"] == unfused["small"]["grid_stats"]


def test_twins_with_every_second_target_searched(unfused):
    r = run(["twins"], PCGX_TEST_ICP_FUSED_SEARCH=2)["twins"]
    T.assert_oracle(r["fit"], oracle("twins"))
    assert r["fit"] == unfused["twins"]["fit"]
    # (no certified step ran: the ties ended the speculation in iteration 1 -- see the module's docstring)
    assert r["counters"]["fused"] == 0 and r["counters"]["searched"] == 0 and r["counters"]["gave_up"] == 0, r["counters"]


def test_a_forced_grid_walk_enqueues_the_first_certified_step_again(unfused):
    r = run(["small"], PCGX_TEST_ICP_FUSED_GRID_WALK=5)["small"]
    T.assert_oracle(r["fit"], oracle("small"))
    assert r["fit"] == unfused["small"]["fit"]
    assert r["counters"]["replayed"] == 1 and r["counters"]["gave_up"] == 0, r["counters"]
    assert r["grid_stats"] == unfused["small"]["grid_stats"]


def test_a_second_fit_behind_reset_without_result(unfused):
    # (the one-launch reset, csrc/icp.hip reset_state: walk counts, strict counters and arrival bits zeroed by the
    # reset kernel itself)
    got = run(["small", "refit"])
    T.assert_oracle(got["small"]["fit"], oracle("small"))
    assert got["refit"]["fit"] == got["small"]["fit"] == unfused["small"]["fit"]
    assert got["refit"]["counters"]["gave_up"] == 0 and got["refit"]["counters"]["replayed"] == 0, got["refit"]["counters"]
    assert got["refit"]["counters"]["fused"] == 2 * (case("small")["max_iteration"] - 2), got["refit"]["counters"]
    assert got["refit"]["grid_stats"] == unfused["small"]["grid_stats"]
