"""NDT registration on the GPU (pcgx_ndt_map_*, pcgx_ndt_evaluate / _dev, pcgx_ndt_fit; csrc/ndt.hip) against the
float64 oracle (tests/ndt_oracle.py) on the scenes of tests/test_ndt_oracle.py.

Map: addresses, counts and validity exact, the mean within one float32 ulp, cov6 / icov6 within
2^-23 |oracle| + delta max|entry| with delta = max(4 x the measured order sensitivity, 64 / min_eigen_ratio 2^-53)
(test_ndt_oracle.map_delta: 7.1e-13 on every scene, the sensitivity being 1.5e-15).
Sums: the oracle is fed the LIBRARY's float32 map; per component |got - oracle| <= (pairs + kNdtChain) 2^-53 A_k, A_k the
oracle's sum of absolute terms with the weight's share taken as omega (1 + k2 m / 2); the pair count is exact.
Fit: bit for bit the host-driven loop; within 1e-5 of the oracle's pose after every iteration count 1 ... 30 (the
tolerance BASELINE.json states for ICP poses); the final translation error within 1.5 x the oracle's pinned one.

PCGX_E_SINGULAR: the issue that asked for NDT named "every voxel coplanar with one shared normal" as the singular
case.  By the map's own contract it is not: the eigenvalue floor keeps every voxel's icov6 positive definite
(cond <= 1 / min_eigen_ratio), so sum H is positive definite for any target that is not degenerate itself, and that
Fit runs (test_coplanar_map_is_usable).  The singular case tested here is a target whose moved points all sit on the
origin: the rotation rows of J = e_k x p vanish exactly and sum H has three zero pivots."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from pcgol_amd import _lib as L
from pcgol_amd import icp, ndt, segmentation

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ndt_oracle as NO  # noqa: E402
from test_ndt_oracle import (ALL_RUN, PROTO_ERR_30, check_map, map_delta, map_scenes, prototype,  # noqa: E402
                             prototype_trace, scene_params)

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
_CACHE = {}


def _grid(g, cloud):
    vg = segmentation.StorageVoxelGrid(float(g.resolution), g.size, g.origin)
    vg.AddAll(cloud)
    return vg


def _lib_map(name):
    """(NDTMap of the library over the scene, its Cells())"""
    if name not in _CACHE:
        sc = map_scenes()[name]
        mp, ratio = scene_params(name)
        m = ndt.NDTMap(_grid(sc["grid"], sc["base"]), sc["base"], MinPoints=mp, MinEigenRatio=ratio)
        _CACHE[name] = (m, m.Cells())
    return _CACHE[name]


def _as_oracle_map(grid, cells):
    """The library's float32 map in the oracle's shape"""
    return dict(grid=grid, addr=cells["addr"], valid=cells["valid"], mean=cells["mean"], icov6=cells["icov6"])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if np.asarray(a).dtype == f32 else np.uint64)


def check_sums(got, ref, what):
    assert got[NO.P_PAIRS] == ref["pairs"], (what, got[NO.P_PAIRS], ref["pairs"])
    bound = (ref["pairs"] + NO.CHAIN) * 2.0 ** -53 * ref["A"]
    err = np.abs(got - ref["sums"])
    assert np.all(err <= bound), (what, int(np.argmax(err - bound)), float(np.max(err - bound)))


# ---- the map

@pytest.mark.parametrize("name", ["prototype", "hand", "fat", "single"])
def test_map_against_oracle(name):
    sc = map_scenes()[name]
    m, cells = _lib_map(name)
    ref = sc["map"]
    assert m.Counts() == (len(ref["addr"]), int(ref["valid"].sum()))
    check_map(cells, ref, map_delta(name), name)


def test_empty_grid_and_empty_cloud():
    g = map_scenes()["single"]["grid"]
    none = np.zeros((0, 3), f32)
    m = ndt.NDTMap(_grid(g, none), none)
    assert m.Counts() == (0, 0) and len(m.Cells()["addr"]) == 0
    s = m.Evaluate(map_scenes()["single"]["target"])
    assert np.all(s == 0)
    far = f32([[100, 100, 100], [np.nan, 0, 0]])   # points, but none inside the grid
    m = ndt.NDTMap(_grid(g, far), far)
    assert m.Counts() == (0, 0)


# ---- the sums

POSES = {"null": None, "identity": NO.IDENTITY, "general": NO.truth_pose()}


@pytest.mark.parametrize("neighbors", [1, 7, 27])
@pytest.mark.parametrize("pose", sorted(POSES))
def test_sums_against_oracle(neighbors, pose):
    sc = prototype()
    m, cells = _lib_map("prototype")
    om = _as_oracle_map(sc["grid"], cells)
    # 3000: three workgroups, every lane of which takes several targets, the last round partly filled
    for nt in (0, 1, 63, 64, 65, 257, 3000):
        t = sc["target"][:nt]
        got = m.Evaluate(t, POSES[pose], neighbors)
        check_sums(got, NO.sums(om, t, POSES[pose], neighbors), (neighbors, pose, nt))
    if pose == "general":   # the truth pose lines the clouds up: more pairs carry weight than at the identity
        assert got[NO.P_WEIGHT] > 100.0


@pytest.mark.parametrize("neighbors", [1, 7, 27])
def test_sums_nan_inf_off_grid_and_row_wrap(neighbors):
    """The hand scene's targets: NaN, +Inf, off-grid points, and targets in voxel (3,0,0) / (0,1,0), whose addresses 3 and
    4 follow each other although the voxels are no neighbours: +-1 on the flat address would pair them."""
    sc = map_scenes()["hand"]
    m, cells = _lib_map("hand")
    om = _as_oracle_map(sc["grid"], cells)
    got = m.Evaluate(sc["target"], None, neighbors)
    ref = NO.sums(om, sc["target"], None, neighbors)
    check_sums(got, ref, neighbors)
    assert np.all(np.isfinite(got))
    for i in (1, 2):   # each border target alone
        t = sc["target"][i:i + 1]
        ref = NO.sums(om, t, None, neighbors)
        got = m.Evaluate(t, None, neighbors)
        check_sums(got, ref, (neighbors, i))
        if neighbors == 7:
            assert ref["pairs"] == (2 if i == 1 else 1)
    bad = sc["target"][8:]   # outside, NaN, Inf: nothing
    assert np.all(m.Evaluate(bad, None, neighbors) == 0)


def test_sums_fat_and_single_voxel():
    for name in ("fat", "single"):
        sc = map_scenes()[name]
        m, cells = _lib_map(name)
        om = _as_oracle_map(sc["grid"], cells)
        for nb in (1, 27):
            check_sums(m.Evaluate(sc["target"], None, nb), NO.sums(om, sc["target"], None, nb), (name, nb))


# ---- the Fit

def _host_loop(m, target, neighbors=7, outlier=0.55, min_pairs=0, threshold=None, damping=0.0, max_iter=0, init=None):
    """pcgx_ndt_evaluate -> pcgx_icp_plane_finish_evaluate -> pcgx_icp_gauss_newton_update, driven from here.
    -> (trans, number of evaluations, last Evaluated, poses after every iteration)"""
    u = icp.GaussNewtonUpdaterFactory(Threshold=threshold, MaxIteration=max_iter, Damping=damping).New()
    trans = NO.IDENTITY.copy() if init is None else np.asarray(init, f32).copy()
    num, ev, poses = 0, None, []
    for _ in range(max_iter or 20):
        num += 1
        ev = icp.FinishEvaluatePlane(m.Evaluate(target, trans, neighbors, outlier), min_pairs)
        trans, conv = u.Update(trans, ev)
        poses.append(trans.copy())
        if conv:
            break
    return trans, num, ev, poses


def _same_fit(fit, loop):
    trans, stat = fit
    ltrans, num, ev, _ = loop
    assert np.array_equal(_bits(trans), _bits(ltrans))
    assert stat.NumIteration == num
    assert stat.Evaluated.NumPairs == ev.NumPairs and stat.Evaluated.DistRMS == 0.0
    assert np.array_equal(_bits(f32([stat.Evaluated.Value])), _bits(f32([ev.Value])))
    assert np.array_equal(_bits(stat.Evaluated.Gradient), _bits(ev.Gradient))
    assert np.array_equal(_bits(stat.Evaluated.Hessian), _bits(ev.Hessian))


def test_fit_equals_host_loop_bit_for_bit():
    sc = prototype()
    m, _ = _lib_map("prototype")
    # default threshold: the flat test ends the Fit; threshold -1: the iteration cap does; damping; another neighbourhood
    for kw in (dict(max_iter=30), dict(threshold=ALL_RUN, max_iter=5), dict(threshold=ALL_RUN, max_iter=3, damping=0.1),
               dict(neighbors=27, max_iter=30), dict(neighbors=1, threshold=ALL_RUN, max_iter=4, init=sc["truth"])):
        reg = ndt.NDT(m, Neighbors=kw.get("neighbors", 7), Threshold=kw.get("threshold"),
                      MaxIteration=kw.get("max_iter", 0), Damping=kw.get("damping", 0.0))
        loop = _host_loop(m, sc["target"], **kw)
        _same_fit(reg.Fit(sc["target"], kw.get("init")), loop)
    assert loop[1] == 4


def test_fit_follows_the_oracle_iteration_by_iteration():
    sc = prototype()
    m, _ = _lib_map("prototype")
    ref = prototype_trace(7, 30)["poses"]
    _, num, _, poses = _host_loop(m, sc["target"], threshold=ALL_RUN, max_iter=30)
    assert num == 30
    for k in range(30):
        d = float(np.max(np.abs(poses[k].astype(f64) - ref[k].astype(f64))))
        assert d <= 1e-5, (k + 1, d)
    for k in (1, 2, 7, 30):   # the Fit itself stopped after k iterations is the loop's k-th pose
        trans, stat = ndt.NDT(m, Threshold=ALL_RUN, MaxIteration=k).Fit(sc["target"])
        assert stat.NumIteration == k and np.array_equal(_bits(trans), _bits(poses[k - 1]))
    err = NO.translation_error(trans, sc["truth"])
    print("translation error after 30 iterations: %.3e (oracle %.3e)" % (err, PROTO_ERR_30))
    assert err <= 1.5 * PROTO_ERR_30


def test_fit_from_the_truth_pose_converges_in_one_flat_test():
    """At the truth pose the omega-weighted mean gradient is O(1) on this scene (largest component 2.0; 4.5e2 at the
    identity: tests/test_ndt_oracle.py), so the flat test is given 10."""
    sc = prototype()
    m, _ = _lib_map("prototype")
    reg = ndt.NDT(m, Threshold=np.full(6, 10, f32))
    trans, stat = reg.Fit(sc["target"], sc["truth"])
    assert stat.NumIteration == 1 and np.array_equal(_bits(trans), _bits(sc["truth"]))
    assert 1.0 < np.max(np.abs(stat.Evaluated.Gradient)) < 3.0
    trans, stat = reg.Fit(sc["target"])   # ... and does not hold at the identity
    assert stat.NumIteration > 1


def test_fit_on_device_target_equals_host_target():
    import torch
    sc = prototype()
    m, _ = _lib_map("prototype")
    reg = ndt.NDT(m, MaxIteration=6, Threshold=ALL_RUN)
    a = reg.Fit(sc["target"])
    b = reg.Fit(torch.from_numpy(sc["target"]).cuda())
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and a[1].NumIteration == b[1].NumIteration == 6
    assert np.array_equal(_bits(a[1].Evaluated.Hessian), _bits(b[1].Evaluated.Hessian))


def test_not_enough_pairs():
    sc = prototype()
    m, _ = _lib_map("prototype")
    far = sc["target"] + f32(100.0)   # outside the grid: no pairs at all
    with pytest.raises(icp.ErrNotEnoughPairs) as e:
        ndt.NDT(m).Fit(far, sc["truth"])
    assert e.value.stat.NumIteration == 1 and e.value.stat.Evaluated.NumPairs == 0
    assert np.array_equal(_bits(e.value.trans), _bits(sc["truth"]))   # the pose the failing iteration started from
    with pytest.raises(icp.ErrNotEnoughPairs):
        ndt.NDT(m).Fit(np.zeros((0, 3), f32))
    pairs = int(m.Evaluate(sc["target"])[NO.P_PAIRS])
    with pytest.raises(icp.ErrNotEnoughPairs) as e:
        ndt.NDT(m, MinPairs=pairs + 1).Fit(sc["target"])
    assert e.value.stat.Evaluated.NumPairs == pairs
    trans, stat = ndt.NDT(m, MinPairs=pairs, MaxIteration=1).Fit(sc["target"])
    assert stat.NumIteration == 1


def test_singular_when_every_moved_point_is_the_origin():
    sc = map_scenes()["hand"]
    m, _ = _lib_map("hand")
    t = np.zeros((8, 3), f32)   # voxel (0,0,0) is invalid, its neighbours (1,0,0), (0,1,0), (0,0,1) are valid
    s = m.Evaluate(t)
    assert s[NO.P_PAIRS] == 24 and s[NO.P_WEIGHT] > 0
    assert np.all(s[NO.P_G0 + 3:NO.P_G0 + 6] == 0)   # J_{3+k} = e_k x 0
    with pytest.raises(L.ErrSingular):
        ndt.NDT(m).Fit(t)
    with pytest.raises(NO.Singular):
        NO.fit(_as_oracle_map(sc["grid"], m.Cells()), t)


def _plane_scene():
    """Every voxel coplanar with one shared normal: a jittered lattice in the plane z = 0.25, 3 x 3 voxels of edge 1"""
    if "plane" not in _CACHE:
        rng = np.random.default_rng(12)
        xy = rng.uniform(-0.45, 2.45, (900, 2))
        base = np.column_stack([xy, np.full(len(xy), 0.25)]).astype(f32)
        grid = NO.Grid(1.0, (3, 3, 2), (0.0, 0.0, 0.0))
        tgt = np.column_stack([rng.uniform(0.0, 2.0, (300, 2)), np.full(300, 0.25)]).astype(f32)
        move = NO.GO._mat4_mul(NO.GO._translate(0.03, -0.02, 0.01), NO.GO._rodrigues(f32([0.01, -0.01, 0.02])))
        _CACHE["plane"] = dict(grid=grid, base=base, target=NO.synth.transform_points(NO.inverse_pose(move), tgt),
                               move=move)
    return _CACHE["plane"]


def test_coplanar_map_is_usable():
    """(see the head of the file) the eigenvalue floor makes a map of coplanar voxels positive definite: no
    PCGX_E_SINGULAR; the Fit equals the oracle's and pulls the target back into the plane"""
    sc = _plane_scene()
    m = ndt.NDTMap(_grid(sc["grid"], sc["base"]), sc["base"])
    cells = m.Cells()
    assert m.Counts() == (9, 9)
    ev = np.linalg.eigvalsh(NO.sym6(cells["cov6"]))
    assert np.all(np.abs(ev[:, 0] / ev[:, 2] - 0.01) <= 1e-5)   # the normal direction sits on the floor
    trans, stat = ndt.NDT(m, Threshold=ALL_RUN, MaxIteration=10).Fit(sc["target"])
    ref = NO.fit(_as_oracle_map(sc["grid"], cells), sc["target"], threshold=ALL_RUN, max_iter=10)
    assert stat.NumIteration == 10 and np.max(np.abs(trans.astype(f64) - ref["trans"].astype(f64))) <= 1e-5
    moved = NO.synth.transform_points(trans, sc["target"])
    assert np.max(np.abs(moved[:, 2] - 0.25)) < 2e-3 < np.max(np.abs(sc["target"][:, 2] - 0.25))


def test_no_voxel_in_reach_returns_the_input_pose():
    """Pairs, but every omega underflows to 0: a plate 0.1 wide whose normal variance sits on the floor (1 / l' ~ 1e5),
    and targets 0.4 off it.  The gradient is 0, the flat test holds, the input pose comes back; sum omega tells."""
    rng = np.random.default_rng(13)
    base = np.column_stack([rng.uniform(-0.05, 0.05, (60, 2)), np.zeros(60)]).astype(f32)
    grid = NO.Grid(1.0, (1, 1, 1), (0.0, 0.0, 0.0))
    m = ndt.NDTMap(_grid(grid, base), base)
    assert m.Counts() == (1, 1)
    t = np.column_stack([rng.uniform(-0.05, 0.05, (10, 2)), np.full(10, 0.4)]).astype(f32)
    s = m.Evaluate(t)
    ref = NO.sums(_as_oracle_map(grid, m.Cells()), t)
    assert s[NO.P_PAIRS] == 10 == ref["pairs"] and s[NO.P_WEIGHT] == 0.0 == ref["sums"][NO.P_WEIGHT]
    init = NO.GO._translate(0.001, 0.0, 0.0)
    trans, stat = ndt.NDT(m).Fit(t, init)
    assert stat.NumIteration == 1 and np.array_equal(_bits(trans), _bits(init))
    assert np.all(stat.Evaluated.Gradient == 0) and stat.Evaluated.NumPairs == 10


# ---- bits

def test_same_call_same_bits():
    sc = prototype()
    m, cells = _lib_map("prototype")
    mp, ratio = scene_params("prototype")
    again = ndt.NDTMap(_grid(sc["grid"], sc["base"]), sc["base"], MinPoints=mp, MinEigenRatio=ratio).Cells()
    for k in cells:
        assert np.array_equal(cells[k].view(np.uint8), again[k].view(np.uint8)), k
    for nb in (1, 7, 27):
        a, b = m.Evaluate(sc["target"], sc["truth"], nb), m.Evaluate(sc["target"], sc["truth"], nb)
        assert np.array_equal(_bits(a), _bits(b))
    reg = ndt.NDT(m, MaxIteration=8)
    a, b = reg.Fit(sc["target"]), reg.Fit(sc["target"])
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and a[1].NumIteration == b[1].NumIteration


def test_host_form_equals_dev_form_on_a_stream():
    import torch
    sc = prototype()
    m, _ = _lib_map("prototype")
    t = torch.from_numpy(sc["target"]).cuda()
    out = torch.full((3, 30), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for i, nb in enumerate((1, 7, 27)):
            m.EvaluateDev(t, out[i], sc["truth"], nb, stream=stream.cuda_stream)
    stream.synchronize()   # the one synchronise
    got = out.cpu().numpy()
    for i, nb in enumerate((1, 7, 27)):
        assert np.array_equal(_bits(got[i]), _bits(m.Evaluate(sc["target"], sc["truth"], nb)))
    # nt == 0 on the device form: thirty zeros
    m.EvaluateDev(t[:0], out[0])
    torch.cuda.synchronize()
    assert np.all(out[0].cpu().numpy() == 0)


def test_on_device_creation_equals_host_creation():
    import torch
    sc = prototype()
    _, cells = _lib_map("prototype")
    mp, ratio = scene_params("prototype")
    vg = _grid(sc["grid"], sc["base"])
    dev = ndt.NDTMap(vg, torch.from_numpy(sc["base"]).cuda(), MinPoints=mp, MinEigenRatio=ratio)
    wide = torch.zeros((len(sc["base"]), 5), dtype=torch.float32, device="cuda")   # stride 20: xyz + two more fields
    wide[:, :3] = torch.from_numpy(sc["base"]).cuda()
    dev_wide = ndt.NDTMap(vg, wide, MinPoints=mp, MinEigenRatio=ratio)
    del vg   # the map owns what it needs
    for other in (dev.Cells(), dev_wide.Cells()):
        for k in cells:
            assert np.array_equal(cells[k].view(np.uint8), other[k].view(np.uint8)), k
    a, b = _lib_map("prototype")[0].Evaluate(sc["target"]), dev.Evaluate(sc["target"])
    assert np.array_equal(_bits(a), _bits(b))


def test_nullable_outputs():
    sc = prototype()
    m, cells = _lib_map("prototype")
    lib = L.lib()
    k = len(cells["addr"])
    names = ("addr", "count", "valid", "mean", "cov6", "icov6")
    for keep in range(6):   # each output alone, the others NULL
        out = np.zeros_like(cells[names[keep]])
        args = [L.ptr(out) if i == keep else None for i in range(6)]
        L.check(lib.pcgx_ndt_map_cells(m._h, *args))
        assert np.array_equal(out.view(np.uint8), cells[names[keep]].view(np.uint8)) and len(out) == k
    L.check(lib.pcgx_ndt_map_cells(m._h, None, None, None, None, None, None))
    a, b = C.c_int64(-1), C.c_int64(-1)
    L.check(lib.pcgx_ndt_map_counts(m._h, C.byref(a), None))
    L.check(lib.pcgx_ndt_map_counts(m._h, None, C.byref(b)))
    L.check(lib.pcgx_ndt_map_counts(m._h, None, None))
    assert (a.value, b.value) == m.Counts()
    # the Fit with and without stat / hessian / init
    p = icp._params(0.0, 0.0, 0, np.zeros(6, f32), np.zeros(6, f32), 4)
    t = sc["target"]
    full, bare = np.zeros(16, f32), np.zeros(16, f32)
    st, h = L.IcpStat(), np.zeros(36, f32)
    L.check(lib.pcgx_ndt_fit(m._h, L.ptr(t), len(t), 0, C.byref(p), 0.0, 7, 0.55, L.ptr(NO.IDENTITY), L.ptr(full),
                             C.byref(st), L.ptr(h)))
    L.check(lib.pcgx_ndt_fit(m._h, L.ptr(t), len(t), 0, C.byref(p), 0.0, 7, 0.55, None, L.ptr(bare), None, None))
    assert np.array_equal(_bits(full), _bits(bare)) and st.num_iteration == 4 and np.any(h != 0)


# ---- arguments

def test_bad_arguments():
    sc = prototype()
    m, _ = _lib_map("prototype")
    lib = L.lib()
    vg = _grid(sc["grid"], sc["base"])
    base, n = sc["base"], len(sc["base"])
    h = C.c_void_p()
    inv = L.PCGX_E_INVALID
    create = lib.pcgx_ndt_map_create
    assert create(None, L.ptr(base), n, 12, 0, 0, 6, 0.01, C.byref(h)) == inv
    assert create(vg._h, L.ptr(base), n, 12, 0, 0, 6, 0.01, None) == inv
    assert create(vg._h, L.ptr(base), n - 1, 12, 0, 0, 6, 0.01, C.byref(h)) == inv      # not the grid's cloud
    assert create(vg._h, None, n, 12, 0, 0, 6, 0.01, C.byref(h)) == inv
    for ratio in (0.0, -0.1, 1.5, float("nan")):
        assert create(vg._h, L.ptr(base), n, 12, 0, 0, 6, ratio, C.byref(h)) == inv
    assert create(vg._h, L.ptr(base), n, 12, 0, 0, 6, 1.0, C.byref(h)) == L.PCGX_OK      # 1 is inside (0, 1]
    L.check(lib.pcgx_ndt_map_free(h))
    assert lib.pcgx_ndt_map_counts(None, None, None) == inv
    assert lib.pcgx_ndt_map_cells(None, None, None, None, None, None, None) == inv
    t, nt = sc["target"], len(sc["target"])
    s = np.zeros(30)
    ev = lib.pcgx_ndt_evaluate
    assert ev(None, L.ptr(t), nt, None, 7, 0.55, L.ptr(s)) == inv
    assert ev(m._h, None, nt, None, 7, 0.55, L.ptr(s)) == inv
    assert ev(m._h, L.ptr(t), -1, None, 7, 0.55, L.ptr(s)) == inv
    assert ev(m._h, L.ptr(t), nt, None, 7, 0.55, None) == inv
    for nb in (0, 6, 8, 26, -1):
        assert ev(m._h, L.ptr(t), nt, None, nb, 0.55, L.ptr(s)) == inv
    for o in (0.0, 1.0, -0.2, 1.2, float("nan")):
        assert ev(m._h, L.ptr(t), nt, None, 7, o, L.ptr(s)) == inv
    evd = lib.pcgx_ndt_evaluate_dev   # (the checks come before any pointer is used)
    assert evd(None, L.ptr(t), nt, None, 7, 0.55, L.ptr(s), None) == inv
    assert evd(m._h, None, nt, None, 7, 0.55, L.ptr(s), None) == inv
    assert evd(m._h, L.ptr(t), nt, None, 5, 0.55, L.ptr(s), None) == inv
    assert evd(m._h, L.ptr(t), nt, None, 7, 1.0, L.ptr(s), None) == inv
    assert evd(m._h, L.ptr(t), nt, None, 7, 0.55, None, None) == inv
    p = icp._params(0.0, 0.0, 0, np.zeros(6, f32), np.zeros(6, f32), 0)
    tr = np.zeros(16, f32)
    fit = lib.pcgx_ndt_fit
    assert fit(None, L.ptr(t), nt, 0, C.byref(p), 0.0, 7, 0.55, None, L.ptr(tr), None, None) == inv
    assert fit(m._h, None, nt, 0, C.byref(p), 0.0, 7, 0.55, None, L.ptr(tr), None, None) == inv
    assert fit(m._h, L.ptr(t), -1, 0, C.byref(p), 0.0, 7, 0.55, None, L.ptr(tr), None, None) == inv
    assert fit(m._h, L.ptr(t), nt, 0, None, 0.0, 7, 0.55, None, L.ptr(tr), None, None) == inv
    assert fit(m._h, L.ptr(t), nt, 0, C.byref(p), 0.0, 7, 0.55, None, None, None, None) == inv
    assert fit(m._h, L.ptr(t), nt, 0, C.byref(p), 0.0, 9, 0.55, None, L.ptr(tr), None, None) == inv
    assert fit(m._h, L.ptr(t), nt, 0, C.byref(p), 0.0, 7, 0.0, None, L.ptr(tr), None, None) == inv
    # a resolution at which k2 is not finite and > 0 (c2 overflows): PCGX_E_INVALID, as the oracle says
    tiny = NO.Grid(1e-30, (1, 1, 1), (0.0, 0.0, 0.0))
    assert NO.k2_of(0.55, tiny.resolution) is None
    pts = np.zeros((8, 3), f32)
    mt = ndt.NDTMap(_grid(tiny, pts), pts)
    assert ev(mt._h, L.ptr(pts), 8, None, 7, 0.55, L.ptr(s)) == inv
