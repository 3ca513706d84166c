"""The edges of an ICP session's set-up (csrc/icp.hip, session_create; csrc/icp_session_plan.h): empty and tiny targets,
host inputs against device-resident ones, the one-launch session beside the general one, and many sessions made and
freed in a row through the block cache.  Everything is compared for equality: with the same session made another way,
with the first session of its kind, or with the oracle's Fit.

The block cache itself exposes no figures (pcgx_debug_call_stats counts pooled calls), so that it does not grow over
the 50 sessions is not asserted here."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
from pcgol_amd import _lib as L
from pcgol_amd import icp, kdtree, synth

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = np.full(6, -1, f32)  # Threshold -1: every iteration runs
KINDS = ("point", "plane", "gicp")


def _spd6(n, seed):
    """n symmetric positive definite 3x3 matrices as xx, xy, xz, yy, yz, zz"""
    m = np.random.Generator(np.random.PCG64(seed)).standard_normal((n, 3, 3))
    c = 0.01 * m @ m.transpose(0, 2, 1) + 1e-3 * np.eye(3)
    return np.ascontiguousarray(np.stack([c[:, 0, 0], c[:, 0, 1], c[:, 0, 2], c[:, 1, 1], c[:, 1, 2], c[:, 2, 2]], 1), f32)


def _scene(n):
    c = synth.c4_plane(n)
    c["tree"] = kdtree.New(c["base"])
    c["bc"], c["tc"] = _spd6(n, 11), _spd6(n, 12)
    return c


@pytest.fixture(scope="module")
def scene500():
    return _scene(500)


@pytest.fixture(scope="module")
def scene5k():
    return _scene(5000)


def _session(c, kind, nt, min_pairs=1, device=False, max_iteration=8):
    """-> (session, what must stay alive beside it)"""
    target, normals, bc, tc = c["target"][:nt], c["normals"], c["bc"], c["tc"][:nt]
    keep = None
    kw = {}
    if device:
        import torch
        keep = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in (target, normals, bc, tc)]
        torch.cuda.synchronize()
        target, normals, bc, tc = keep
        kw = dict(target_on_device=True, nt=nt)
        target = target.data_ptr()
    if kind == "plane":
        kw["BaseNormals"] = normals
    elif kind == "gicp":
        kw["BaseCov"], kw["TargetCov"] = bc, tc
    return icp.IcpSession(c["tree"], target, c["max_dist"], min_pairs, None, ALL, max_iteration, **kw), keep


def _outcome(s, kind):
    """everything a session lets its caller read, errors as values"""
    out = {"sums": s.read_sums()}
    try:
        trans, st, conv = s.result()
        out["result"] = (trans, st.NumIteration, f32(st.Evaluated.Value), np.asarray(st.Evaluated.Gradient, f32),
                         st.Evaluated.NumPairs, conv)
    except L.PcgxError as e:
        out["result"] = (type(e).__name__, str(e))
    if kind != "point":
        out["hessian"] = s.hessian()
    if kind == "gicp":
        out["dropped"] = s.dropped()
    return out


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        va, vb = (a[k], b[k]) if isinstance(a[k], tuple) else ((a[k],), (b[k],))
        assert len(va) == len(vb), k
        for x, y in zip(va, vb):
            if isinstance(x, str) or isinstance(y, str):
                assert x == y, (k, x, y)
            else:
                assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), (k, x, y)


def _stepped(c, kind, nt, steps, **kw):
    s, keep = _session(c, kind, nt, **kw)
    try:
        for _ in range(steps):
            s.step()
        return _outcome(s, kind)
    finally:
        s.close()
        del keep


# ---- empty and tiny targets ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_an_empty_target_is_not_enough_pairs(scene500, kind):
    """nt = 0: no arena, no upload, no gather; the step runs and the result says why there is none"""
    for device in (False, True):
        s, keep = _session(scene500, kind, 0, min_pairs=6, device=device)
        try:
            s.step()
            with pytest.raises(icp.ErrNotEnoughPairs) as e:
                s.result()
            stat = e.value.stat
            assert stat.Evaluated.NumPairs == 0
            assert str(e.value).endswith(": not enough correspondence pairs (0 < 6) at iteration %d" % stat.NumIteration)
        finally:
            s.close()


@pytest.mark.parametrize("nt", [1, 2])  # 1: no Morton order (perm is null); 2: the first ordered gather
@pytest.mark.parametrize("kind", KINDS)
def test_tiny_targets_from_the_host_and_from_the_device(scene500, kind, nt):
    host = _stepped(scene500, kind, nt, 1)
    dev = _stepped(scene500, kind, nt, 1, device=True)
    assert host["sums"][-1] == nt  # (every target has a partner within MaxDist: the sums are of something)
    assert np.array_equal(host["sums"], dev["sums"])
    _same(host, dev)


# ---- host inputs equal device inputs ---------------------------------------------------------------------------------

@pytest.mark.parametrize("nt", [255, 256, 257, 5000])  # the GICP grid's and the partial rows' rounding; a few blocks
@pytest.mark.parametrize("kind", ["plane", "gicp"])
def test_host_inputs_equal_device_inputs(scene5k, kind, nt):
    host = _stepped(scene5k, kind, nt, 5, min_pairs=6)
    dev = _stepped(scene5k, kind, nt, 5, min_pairs=6, device=True)
    assert host["sums"][-1] > 0.9 * nt  # (pairs: the comparison below is of Fits that found their partners)
    _same(host, dev)


# ---- the one-launch session beside the general one -------------------------------------------------------------------

def _small_shapes():
    """(name, base, target, MaxDist): 63, 64, 65 targets on a 256-point base (the edge of nt_pad), and the first shape
    test_which_clouds_get_the_one_launch_by_default finds past eligibility"""
    c = synth.c4_icp(n=256, width=1.0)
    shapes = [("nt%d" % nt, c["base"], np.ascontiguousarray(c["target"][:nt]), 0.5) for nt in (63, 64, 65)]
    big = synth.c4_icp(n=16000, width=4.0)
    return shapes + [("past", big["base"], big["target"], 0.5)]


def _fit_all(shapes):
    """-> name -> (trans, NumIteration, Value, Gradient, one-launch launches)"""
    import ctypes as C
    out = {}
    for name, base, target, max_dist in shapes:
        launches = (C.c_int64 * 3)()
        L.check(L.lib().pcgx_debug_icp_one_launch(launches, 1))
        reg = icp.PointToPointICPGradient(icp.PointToPointEvaluator(icp.NearestPointCorresponder(MaxDist=max_dist), MinPairs=3),
                                          icp.GradientDescentUpdaterFactory(Threshold=ALL, MaxIteration=4))
        trans, st = reg.Fit(kdtree.New(base), target)
        L.check(L.lib().pcgx_debug_icp_one_launch(launches, 0))
        out[name] = (np.asarray(trans, f32).ravel(), st.NumIteration, f32(st.Evaluated.Value),
                     np.asarray(st.Evaluated.Gradient, f32), int(launches[0]))
    return out


CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import test_gpu_icp_session_setup as T
fits = T._fit_all(T._small_shapes())
np.savez(sys.argv[1], **{"%%s_%%d" %% (k, i): np.asarray(x) for k, v in fits.items() for i, x in enumerate(v)})
"""


@pytest.fixture(scope="module")
def general_path_fits(tmp_path_factory):
    """The same Fits with PCGX_ICP_SMALL=0.  The knob is read once per process: a fresh child, before this process
    starts anything for these tests; if it ends on a signal or runs out of time nothing more is started."""
    out = str(tmp_path_factory.mktemp("small_off") / "fits.npz")
    env = dict(os.environ, PCGX_ICP_SMALL="0")
    for k in ("PCGX_ICP_SMALL_BASE", "PCGX_ICP_SMALL_TARGET", "PCGX_ICP_STRICT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), out], capture_output=True,
                       text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, "the child ended with %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    z = np.load(out)
    return {name: tuple(z["%s_%d" % (name, i)] for i in range(5)) for name, _, _, _ in _small_shapes()}


@pytest.fixture(scope="module")
def default_fits(general_path_fits):
    return _fit_all(_small_shapes())


@pytest.mark.parametrize("name", ["nt63", "nt64", "nt65", "past"])
def test_one_launch_and_general_path_fit_like_the_oracle(general_path_fits, default_fits, name):
    _, base, target, max_dist = next(s for s in _small_shapes() if s[0] == name)
    o = O.icp_fit(O.KDTree(base), target, max_dist, 3, None, ALL, 4, sums_mode=0)
    for what, fits in (("default", default_fits), ("PCGX_ICP_SMALL=0", general_path_fits)):
        trans, num_iteration, value, gradient, launches = fits[name]
        assert int(num_iteration) == o["num_iteration"], what
        assert np.array_equal(np.asarray(trans, f32).ravel(), np.asarray(o["trans"], f32).ravel()), what
        assert f32(value) == o["value"] and np.array_equal(np.asarray(gradient, f32), o["gradient"]), what
    # ... and each leg went the way it is named for
    assert int(default_fits[name][4]) == (0 if name == "past" else 1)
    assert int(general_path_fits[name][4]) == 0


# ---- buffer reuse through the block cache ----------------------------------------------------------------------------

def test_fifty_sessions_in_a_row_reuse_their_buffers(scene5k):
    """create, step, free -- the three kinds and three sizes in turn: a session that gets another session's blocks back
    from the cache computes what the first of its kind and size did"""
    first = {}
    for i in range(50):
        kind, nt = KINDS[i % 3], (1, 257, 5000)[(i // 3) % 3]
        got = _stepped(scene5k, kind, nt, 1)
        if (kind, nt) not in first:
            first[(kind, nt)] = got
            assert got["sums"][-1] == nt
        _same(got, first[(kind, nt)])
    assert len(first) == 9
