"""K poses scored on the whole clouds (pcgx_kdtree_score_poses[_dev]) and the selection of the hypotheses worth scoring
(pcgx_pose_select[_dev]): include/pcgx.h, "score poses".

The reference is the library's own NearestBatch (pinned to the Go oracle by tests/test_gpu_kdtree.py, test_gpu_grid.py,
test_gpu_delete.py), fed pose_oracle.transform's points pose by pose: counts equal, sums within n 2^-52 S of math.fsum
(S that sum: the worst case of a float64 sum of n non-negative terms in any order, doubled), best and pose equal.  The
brute-force oracle (tests/score_oracle.py) is checked on the main scene as well."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_oracle as PO  # noqa: E402
import score_oracle as SO  # noqa: E402
from test_pose_oracle import scene_m_reference  # noqa: E402
from test_score_oracle import decoy_reference, main_reference  # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64, u32 = np.float32, np.float64, np.uint32
EYE = np.eye(4, dtype=f32).reshape(-1)


def per_pair_reference(tree, P, poses, max_dist):
    """-> found (K, n) bool, d (K, n) float32: what NearestBatch answers for every moved point (a dead pose and a point
    that is not finite after the move: never a pair)"""
    poses = np.asarray(poses, f32).reshape(-1, 16)
    P = np.asarray(P, f32).reshape(-1, 3)
    found = np.zeros((len(poses), len(P)), bool)
    d = np.zeros((len(poses), len(P)), f32)
    for k, m in enumerate(poses):
        if not SO.pose_live(m) or len(P) == 0:
            continue
        X = np.stack(PO.transform(m, P), axis=1)
        fin = np.isfinite(X).all(axis=1)
        if fin.any():
            ids, dsq = tree.NearestBatch(np.ascontiguousarray(X[fin]), max_dist)
            found[k, fin] = ids >= 0
            d[k, fin] = dsq
    return found, d


def fold(found, d, poses, n=None):
    """the reference's per-pair answers -> counts, fsums, best, pose over the first n points"""
    n = found.shape[1] if n is None else n
    K = len(poses)
    counts = np.array([int(found[k, :n].sum()) for k in range(K)], np.int64)
    sums = np.array([math.fsum(float(v) for v in d[k, :n][found[k, :n]]) for k in range(K)], f64)
    best = -1
    for k in range(K):
        if SO.pose_live(poses[k]) and (best < 0 or counts[k] > counts[best]):
            best = k
    return counts, sums, best, (np.asarray(poses[best], f32).copy() if best >= 0 else np.zeros(16, f32))


def check(got, want, n, what=""):
    counts, sums, best, pose = got
    wc, ws, wb, wp = want
    print("%s counts %s sums %s best %d | reference sums %s" % (what, counts.tolist(), sums.tolist(), best, ws.tolist()))
    assert counts.tolist() == wc.tolist(), what
    for k in range(len(wc)):
        assert abs(sums[k] - ws[k]) <= SO.sum_bound(n, ws[k]), (what, k, sums[k], ws[k])
    assert best == wb, what
    assert np.array_equal(np.asarray(pose, f32).view(u32), wp.view(u32)), what


def score_dev(tree, P, poses, max_dist, with_outputs=True):
    """the device form over torch buffers -> (counts, sums, record dict, raw words)"""
    import torch
    from pcgol_amd import alignment
    dev = torch.device("cuda", 0)
    P = np.ascontiguousarray(P, f32).reshape(-1, 3)
    poses = np.ascontiguousarray(poses, f32).reshape(-1, 16)
    n, K = len(P), len(poses)
    dP = torch.from_numpy(P).to(dev) if n else None
    dM = torch.from_numpy(poses).to(dev) if K else None
    dc = torch.full((max(K, 1),), -7, dtype=torch.int32, device=dev)
    ds = torch.full((max(K, 1),), -7.0, dtype=torch.float64, device=dev)
    res = torch.full((alignment.RESULT_WORDS,), 0x55555555, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    alignment.ScorePosesDev(tree, dP.data_ptr() if n else 0, n, dM.data_ptr() if K else 0, K, max_dist, res.data_ptr(),
                            d_counts=dc.data_ptr() if with_outputs else 0, d_sums=ds.data_ptr() if with_outputs else 0,
                            stream=st)
    torch.cuda.synchronize()
    words = res.cpu().numpy()
    return dc.cpu().numpy()[:K].astype(np.int64), ds.cpu().numpy()[:K], alignment.ReadScore(words), words


def check_record(rec, words, want, n, n_live):
    wc, ws, wb, wp = want
    assert rec["best"] == wb and rec["n"] == n and rec["live"] == n_live
    assert rec["best_count"] == (int(wc[wb]) if wb >= 0 else 0)
    assert abs(rec["sum"] - (ws[wb] if wb >= 0 else 0.0)) <= SO.sum_bound(n, ws[wb] if wb >= 0 else 0.0)
    assert words[6] == 0 and words[7] == 0
    assert np.array_equal(rec["pose"].view(u32), wp.view(u32))


@pytest.fixture(scope="module")
def main():
    """the main scene: the tree over the decoy scene's Q, the six poses, the reference's per-pair answers (read-only)"""
    from pcgol_amd import kdtree
    s = SO.decoy_scene()
    tree = kdtree.New(s["Q"])
    poses = SO.main_poses()
    ref = {}
    for md in (0.02, 10.0):
        found, d = per_pair_reference(tree, s["P"], poses, md)
        found.setflags(write=False)
        d.setflags(write=False)
        ref[md] = (found, d)
    poses.setflags(write=False)
    return dict(s=s, tree=tree, poses=poses, ref=ref)


@pytest.mark.parametrize("max_dist", [0.02, 10.0])
def test_main_scene(main, max_dist):
    from pcgol_amd import alignment
    s, tree, poses = main["s"], main["tree"], main["poses"]
    found, d = main["ref"][max_dist]
    want = fold(found, d, poses)
    n = len(s["P"])
    got = alignment.ScorePoses(tree, s["P"], poses, max_dist)
    check(got, want, n, "host form, max_dist %g:" % max_dist)
    # the brute-force oracle says the same
    o = main_reference(max_dist)
    assert not o["fragile"].any()
    check(got, (o["counts"], o["sums"], o["best"], o["pose"]), n, "against the oracle:")
    if max_dist == 0.02:
        assert got[0].tolist()[:3] == [3000, 105, 0] and got[0][3] == 3000 and got[1][3] > 0
    # the device form: the same counts, the same sum bits (a fixed summation order), the record
    for with_outputs in (True, False):
        dc, dsum, rec, words = score_dev(tree, s["P"], poses, max_dist, with_outputs)
        if with_outputs:
            assert dc.tolist() == got[0].tolist() and dsum.view(np.uint64).tolist() == got[1].view(np.uint64).tolist()
        check_record(rec, words, want, n, 5)
    # the same call twice
    again = alignment.ScorePoses(tree, s["P"], poses, max_dist)
    assert again[0].tolist() == got[0].tolist() and again[1].view(np.uint64).tolist() == got[1].view(np.uint64).tolist()


def test_prefixes_of_points_and_poses(main):
    """n across the tile, K from 0: every combination against the reference's prefix"""
    from pcgol_amd import alignment
    s, tree, poses = main["s"], main["tree"], main["poses"]
    found, d = main["ref"][0.02]
    tile = alignment.ScoreTile()
    assert tile == 256
    for n in (0, 1, tile - 1, tile, tile + 1, 3 * tile + 5):
        for K in (0, 1, 2, 6):
            want = fold(found[:K], d[:K], poses[:K], n)
            got = alignment.ScorePoses(tree, s["P"][:n], poses[:K], 0.02)
            check(got, want, n, "n %d K %d:" % (n, K))
            _, _, rec, words = score_dev(tree, s["P"][:n], poses[:K], 0.02)
            check_record(rec, words, want, n, sum(SO.pose_live(m) for m in poses[:K]))
    # dead poses first: the best is the first live one
    order = [4, 1, 0, 3]
    want = fold(found[order], d[order], poses[order])
    check(alignment.ScorePoses(tree, s["P"], poses[order], 0.02), want, 3000, "dead pose first:")
    assert want[2] == 2
    # no live pose at all
    c, sm, best, pose = alignment.ScorePoses(tree, s["P"], np.zeros((3, 16), f32), 0.02)
    assert c.tolist() == [0, 0, 0] and sm.tolist() == [0, 0, 0] and best == -1 and not pose.any()


@pytest.mark.parametrize("chunk", [None, "1", "4"])
def test_forced_chunk(main, chunk, monkeypatch):
    from pcgol_amd import alignment
    if chunk is None:
        monkeypatch.delenv("PCGX_SCORE_CHUNK", raising=False)
    else:
        monkeypatch.setenv("PCGX_SCORE_CHUNK", chunk)
    s, tree, poses = main["s"], main["tree"], main["poses"]
    for md in (0.02, 10.0):
        found, d = main["ref"][md]
        check(alignment.ScorePoses(tree, s["P"], poses, md), fold(found, d, poses), 3000, "chunk %s, max_dist %g:" % (chunk, md))


@pytest.mark.parametrize("grid", [None, "0", "2"])
def test_grid_modes(main, grid, monkeypatch):
    """a handle built and asked with PCGX_GRID unset, 0 (walk only) and 2 (grid whatever the cells look like)"""
    from pcgol_amd import alignment, kdtree
    if grid is None:
        monkeypatch.delenv("PCGX_GRID", raising=False)
    else:
        monkeypatch.setenv("PCGX_GRID", grid)
    s, poses = main["s"], main["poses"]
    tree = kdtree.New(s["Q"])
    n = 3 * alignment.ScoreTile() + 5
    for md in (0.02, 10.0):
        found, d = per_pair_reference(tree, s["P"][:n], poses, md)
        mf, mdd = main["ref"][md]
        assert np.array_equal(found, mf[:, :n]) and np.array_equal(d[found], mdd[:, :n][found])  # (the reference agrees with itself)
        check(alignment.ScorePoses(tree, s["P"][:n], poses, md), fold(found, d, poses), n, "PCGX_GRID %s, max_dist %g:" % (grid, md))


def test_after_delete_point(main):
    """every tenth id deleted: the reference's patched tree answers; then every point deleted: an empty tree"""
    from pcgol_amd import alignment, kdtree
    s, poses = main["s"], main["poses"]
    tree = kdtree.New(s["Q"])
    tree.DeletePoints(np.arange(0, len(s["Q"]), 10))
    n = 3 * alignment.ScoreTile() + 5
    for md in (0.02, 10.0):
        found, d = per_pair_reference(tree, s["P"][:n], poses, md)
        want = fold(found, d, poses)
        check(alignment.ScorePoses(tree, s["P"][:n], poses, md), want, n, "after DeletePoint, max_dist %g:" % md)
        if md == 0.02:
            assert 0 < want[0][0] < n  # (the deletions are felt)
    small = kdtree.New(s["Q"][:100])
    small.DeletePoints(np.arange(100))
    found, d = per_pair_reference(small, s["P"][:n], poses, 10.0)
    assert not found.any()
    got = alignment.ScorePoses(small, s["P"][:n], poses, 10.0)
    check(got, fold(found, d, poses), n, "empty tree:")
    assert got[2] == 0 and not got[0].any()
    _, _, rec, words = score_dev(small, s["P"][:n], poses, 10.0)
    check_record(rec, words, fold(found, d, poses), n, 5)


def test_points_that_are_not_finite(main):
    from pcgol_amd import alignment
    s, tree, poses = main["s"], main["tree"], main["poses"]
    n = alignment.ScoreTile() + 1
    P = s["P"][:n].copy()
    P[3, 1] = np.nan
    P[n - 1, 0] = np.inf
    for md in (0.02, 10.0):
        found, d = per_pair_reference(tree, P, poses, md)
        assert not found[:, 3].any() and not found[:, n - 1].any()
        want = fold(found, d, poses)
        check(alignment.ScorePoses(tree, P, poses, md), want, n, "NaN and +Inf points, max_dist %g:" % md)
        assert want[0][0] == n - 2


def test_every_pair_tied(monkeypatch):
    """the tree over P2 with every point stored twice: every nearest is tied, every pair leaves the grid uncertified --
    the worst case the temporaries are sized for; five poses in chunks of two"""
    from pcgol_amd import alignment, kdtree
    monkeypatch.setenv("PCGX_SCORE_CHUNK", "2")
    s = SO.decoy_scene()
    tree = kdtree.New(np.concatenate([s["P2"], s["P2"]]))
    moved = PO.TRUE_POSE.copy()
    moved[13] -= f32(0.005)
    far = PO.TRUE_POSE.copy()
    far[14] += f32(0.019)
    poses = np.stack([PO.TRUE_POSE, s["W"], moved, EYE, far])
    n = 2 * alignment.ScoreTile() + 9
    found, d = per_pair_reference(tree, s["P"][:n], poses, 0.02)
    want = fold(found, d, poses)
    got = alignment.ScorePoses(tree, s["P"][:n], poses, 0.02)
    check(got, want, n, "every pair tied:")
    assert want[0][0] == n and want[0][2] == n and want[0][3] == 0 and 0 < want[0][4] <= n
    again = alignment.ScorePoses(tree, s["P"][:n], poses, 0.02)
    assert again[0].tolist() == got[0].tolist() and again[1].view(np.uint64).tolist() == got[1].view(np.uint64).tolist()


@pytest.mark.parametrize("grid", [None, "0"])
def test_dist_sq_equal_to_max_dist_sq(grid, monkeypatch):
    """DistSq == max_dist^2 exactly (3-4-5): whatever NearestBatch answers there -- on four points, and on a lattice
    large enough to carry a grid (PCGX_GRID=2 where the grid is asked for)"""
    from pcgol_amd import alignment, kdtree
    if grid is None:
        monkeypatch.delenv("PCGX_GRID", raising=False)
    else:
        monkeypatch.setenv("PCGX_GRID", grid)
    T = np.array([[0, 0, 0], [100, 0, 0], [0, 100, 0], [0, 0, 100]], f32)
    P = np.array([[3, 4, 0], [0, 3, 4]], f32)
    tree = kdtree.New(T)
    found, d = per_pair_reference(tree, P, EYE[None], 5.0)
    assert d.tolist() == [[25.0, 25.0]]
    check(alignment.ScorePoses(tree, P, EYE[None], 5.0), fold(found, d, EYE[None]), 2, "four points, PCGX_GRID %s:" % grid)
    if grid is None:
        monkeypatch.setenv("PCGX_GRID", "2")
    g = np.arange(8, dtype=f32) * 8
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    P = np.array([[19, 20, 16], [16, 19, 20], [20, 16, 19], [16, 16, 21], [16.5, 16, 16]], f32)
    tree = kdtree.New(lattice)
    found, d = per_pair_reference(tree, P, EYE[None], 5.0)
    print("lattice: found %s DistSq %s" % (found.tolist(), d.tolist()))
    assert found[0, 4] and d[0, 4] == 0.25
    check(alignment.ScorePoses(tree, P, EYE[None], 5.0), fold(found, d, EYE[None]), len(P), "lattice, PCGX_GRID %s:" % grid)


def select_dev(status, counts, poses, K):
    import torch
    from pcgol_amd import alignment
    dev = torch.device("cuda", 0)
    nh = len(status)
    ds = torch.from_numpy(np.ascontiguousarray(status, np.int32)).to(dev) if nh else None
    dc = torch.from_numpy(np.ascontiguousarray(counts, np.int32)).to(dev) if nh else None
    dp = torch.from_numpy(np.ascontiguousarray(poses, f32)).to(dev) if nh else None
    ids = torch.full((max(K, 1),), -9, dtype=torch.int32, device=dev)       # sentinels
    out = torch.full((max(K, 1), 16), 7.5, dtype=torch.float32, device=dev)
    nsel = torch.full((1,), -9, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    alignment.SelectPosesDev(ds.data_ptr() if nh else 0, dc.data_ptr() if nh else 0, dp.data_ptr() if nh else 0, nh, K,
                             ids.data_ptr() if K else 0, out.data_ptr() if K else 0, nsel.data_ptr(),
                             stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return ids.cpu().numpy()[:K].astype(np.int64), out.cpu().numpy()[:K], int(nsel.cpu().numpy()[0])


def test_selection():
    from pcgol_amd import alignment
    s, est, _ = decoy_reference()
    found, pose, inl, info = alignment.EstimatePose(s["P"], s["Q"], s["pairs"], 0, s["max_dist"], EdgeSimilarity=s["es"],
                                                    samples=s["samples"], per_hypothesis=True)
    assert info["counts"].tolist() == [14, 10, 14, 10] and info["best"] == 0 and found
    sm, _ = scene_m_reference()
    _, _, _, big = alignment.EstimatePose(sm["P"], sm["Q"], np.stack([sm["src"], sm["dst"]], axis=1), 0, sm["max_dist"],
                                          samples=sm["samples"], per_hypothesis=True)
    hand = dict(status=np.array([0, 0, 1, 0, 0, 0, 0], np.int32), counts=np.array([5, 9, 50, 9, 2, 3, 9], np.int64),
                poses=np.arange(112, dtype=f32).reshape(7, 16) + 1)
    for name, h in (("decoy", info), ("scene M", big), ("hand", hand)):
        qualify = int(((h["status"] == 0) & (h["counts"] >= 3)).sum())
        assert qualify < 5000
        for K in (1, 8, 64, 5000):
            wi, wp, wn = SO.select(h["status"], h["counts"], h["poses"], K)
            assert wn == min(K, qualify)
            for form, got in (("host", alignment.SelectPoses(h["status"], h["counts"], h["poses"], K)),
                              ("device", select_dev(h["status"], h["counts"], h["poses"], K))):
                gi, gp, gn = got
                assert gn == wn and gi.tolist() == wi.tolist(), (name, K, form)
                assert np.array_equal(gp.view(u32), wp.view(u32)), (name, K, form)
                assert (gi[wn:] == -1).all() and not gp[wn:].any()  # the padding over the sentinels
        # ties in count go to the smaller h
        wi, _, wn = SO.select(h["status"], h["counts"], h["poses"], 5000)
        c = h["counts"][wi[:wn]]
        assert np.all((c[:-1] > c[1:]) | ((c[:-1] == c[1:]) & (wi[:wn][:-1] < wi[:wn][1:])))
    assert SO.select(hand["status"], hand["counts"], hand["poses"], 4)[0].tolist() == [1, 3, 6, 0]
    assert SO.select(info["status"], info["counts"], info["poses"], 8)[0].tolist() == [0, 2, 1, 3, -1, -1, -1, -1]
    # no hypothesis, no slot
    for form in (alignment.SelectPoses, select_dev):
        gi, gp, gn = form(hand["status"][:0], hand["counts"][:0], hand["poses"][:0], 3)
        assert gi.tolist() == [-1, -1, -1] and not gp.any() and gn == 0
        gi, gp, gn = form(hand["status"], hand["counts"], hand["poses"], 0)
        assert len(gi) == 0 and gn == 0


def test_device_chain_prefers_the_true_pose():
    """EstimatePoseDev -> SelectPosesDev -> ScorePosesDev on one stream, one synchronise at the end: the estimator's
    best is the decoy (hypothesis 0, 14 of the 24 pairs), the whole clouds pick hypothesis 1 (slot 2, all 3000 points)"""
    import torch
    from pcgol_amd import alignment, kdtree
    s, est, _ = decoy_reference()
    P, Q = s["P"], s["Q"]
    tree = kdtree.New(Q)
    dev = torch.device("cuda", 0)
    n_hyp, K, m = len(s["samples"]), 8, len(s["pairs"])
    dP, dQ = torch.from_numpy(P.copy()).to(dev), torch.from_numpy(Q.copy()).to(dev)
    dsrc = torch.from_numpy(s["src"].astype(np.int32)).to(dev)
    ddst = torch.from_numpy(s["dst"].astype(np.int32)).to(dev)
    du = torch.from_numpy(s["samples"].view(np.int32).copy()).to(dev)
    res = torch.zeros(alignment.RESULT_WORDS, dtype=torch.int32, device=dev)
    status, counts = (torch.zeros(n_hyp, dtype=torch.int32, device=dev) for _ in range(2))
    poses = torch.zeros((n_hyp, 16), dtype=torch.float32, device=dev)
    ids = torch.full((K,), -9, dtype=torch.int32, device=dev)
    sel = torch.full((K, 16), 7.5, dtype=torch.float32, device=dev)
    nsel = torch.full((1,), -9, dtype=torch.int32, device=dev)
    sc = torch.full((K,), -9, dtype=torch.int32, device=dev)
    ss = torch.full((K,), -9.0, dtype=torch.float64, device=dev)
    score = torch.full((alignment.RESULT_WORDS,), 0x55555555, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    alignment.EstimatePoseDev(dP.data_ptr(), len(P), dQ.data_ptr(), len(Q), dsrc.data_ptr(), ddst.data_ptr(), m,
                              du.data_ptr(), n_hyp, res.data_ptr(), s["max_dist"], EdgeSimilarity=s["es"],
                              d_status=status.data_ptr(), d_counts=counts.data_ptr(), d_poses=poses.data_ptr(), stream=st)
    alignment.SelectPosesDev(status.data_ptr(), counts.data_ptr(), poses.data_ptr(), n_hyp, K, ids.data_ptr(),
                             sel.data_ptr(), nsel.data_ptr(), stream=st)
    alignment.ScorePosesDev(tree, dP.data_ptr(), len(P), sel.data_ptr(), K, s["max_dist"], score.data_ptr(),
                            d_counts=sc.data_ptr(), d_sums=ss.data_ptr(), stream=st)
    torch.cuda.synchronize()
    got = alignment.ReadResult(res.cpu().numpy())
    assert got["found"] and got["best"] == 0 and got["best_count"] == 14
    assert counts.cpu().numpy().tolist() == [14, 10, 14, 10]
    assert ids.cpu().numpy().tolist() == [0, 2, 1, 3, -1, -1, -1, -1] and int(nsel.cpu().numpy()[0]) == 4
    words = score.cpu().numpy()
    rec = alignment.ReadScore(words)
    hposes = poses.cpu().numpy()
    assert rec["best"] == 2 and rec["best_count"] == 3000 and rec["live"] == 4 and rec["n"] == 3000
    assert np.array_equal(rec["pose"].view(u32), hposes[1].view(u32))
    hsc = sc.cpu().numpy()
    assert hsc[0] < 300 and hsc[1] < 300 and hsc[2] == 3000 and hsc[3] == 3000
    assert not sc.cpu().numpy()[4:].any()
    # the host forms' composition: every word of the record
    found, pose, inl, info = alignment.EstimatePose(P, Q, s["pairs"], 0, s["max_dist"], EdgeSimilarity=s["es"],
                                                    samples=s["samples"], per_hypothesis=True)
    assert np.array_equal(info["poses"].view(u32), hposes.view(u32))
    hi, hp, hn = alignment.SelectPoses(info["status"], info["counts"], info["poses"], K)
    hc, hs, hbest, hpose = alignment.ScorePoses(tree, P, hp, s["max_dist"])
    want = np.zeros(alignment.RESULT_WORDS, np.int32)
    want[0:4] = [hbest, hc[hbest], hn, len(P)]
    want[4:6] = np.array([hs[hbest]], f64).view(np.int32)
    want[8:24] = hpose.view(np.int32)
    assert words.tolist() == want.tolist()
    assert sc.cpu().numpy().tolist() == hc.tolist() and ss.cpu().numpy().view(np.uint64).tolist() == hs.view(np.uint64).tolist()
    vfound, vpose, vinfo = alignment.EstimatePoseVerified(tree, P, Q, s["pairs"], 0, s["max_dist"], K=K,
                                                          EdgeSimilarity=s["es"], samples=s["samples"])
    assert vfound and np.array_equal(vpose.view(u32), rec["pose"].view(u32))
    assert vinfo["best"] == 1 and vinfo["best_slot"] == 2 and not vinfo["agree"] and vinfo["estimate"]["best"] == 0
    assert vinfo["counts"].tolist() == hc.tolist() and vinfo["ids"].tolist() == hi.tolist()
    # the pose the whole clouds pick maps P onto P2; the estimator's own does not
    x = np.stack(PO.transform(vpose, P), axis=1).astype(f64)
    assert np.max(np.linalg.norm(x - s["P2"], axis=1)) < s["max_dist"]
    x0 = np.stack(PO.transform(pose, P), axis=1).astype(f64)
    assert np.max(np.linalg.norm(x0 - s["P2"], axis=1)) > 1.0


def test_bad_arguments(main):
    import ctypes as C
    from pcgol_amd import _lib as L
    lib = L.lib()
    s, tree, poses = main["s"], main["tree"], main["poses"]
    P = np.ascontiguousarray(s["P"][:10])
    M = np.ascontiguousarray(poses[:2])
    counts, sums, pose = np.zeros(2, np.int64), np.zeros(2, f64), np.zeros(16, f32)
    best = C.c_int64(0)
    INV = L.PCGX_E_INVALID

    def host(t=tree._h, p=L.ptr(P), n=10, m=L.ptr(M), K=2, d=0.02, c=L.ptr(counts), sm=L.ptr(sums), b=C.byref(best),
             o=L.ptr(pose)):
        return lib.pcgx_kdtree_score_poses(t, p, n, m, K, d, c, sm, b, o)

    assert host() == L.PCGX_OK
    assert host(sm=None) == L.PCGX_OK
    for bad in (dict(t=None), dict(p=None), dict(m=None), dict(c=None), dict(b=None), dict(o=None), dict(n=-1), dict(K=-1),
                dict(n=2 ** 31), dict(K=2 ** 31), dict(d=0.0), dict(d=-1.0), dict(d=float("inf")), dict(d=float("nan"))):
        assert host(**bad) == INV, bad
    assert host(p=None, n=0) == L.PCGX_OK and best.value == 0 and counts.tolist() == [0, 0]
    assert host(m=None, K=0, c=None, sm=None) == L.PCGX_OK and best.value == -1 and not pose.any()

    import torch
    dev = torch.device("cuda", 0)
    dP, dM = torch.from_numpy(P).to(dev), torch.from_numpy(M).to(dev)
    res = torch.full((24,), 0x55555555, dtype=torch.int32, device=dev)

    def devf(t=tree._h, p=dP.data_ptr(), n=10, m=dM.data_ptr(), K=2, d=0.02, r=res.data_ptr()):
        return lib.pcgx_kdtree_score_poses_dev(t, p, n, m, K, d, None, None, r, None)

    assert devf() == L.PCGX_OK
    for bad in (dict(t=None), dict(p=None), dict(m=None), dict(r=None), dict(n=-1), dict(K=-1), dict(n=2 ** 31),
                dict(K=2 ** 31), dict(d=0.0), dict(d=float("inf")), dict(d=float("nan"))):
        assert devf(**bad) == INV, bad
    for kw, want_best, live in ((dict(p=None, n=0), 0, 2), (dict(m=None, K=0), -1, 0)):
        res.fill_(0x55555555)
        assert devf(**kw) == L.PCGX_OK
        torch.cuda.synchronize()
        w = res.cpu().numpy()
        assert w[:4].tolist() == [want_best, 0, live, kw.get("n", 10)] and not w[4:8].any()
        assert np.array_equal(w[8:].view(f32), M[0] if want_best == 0 else np.zeros(16, f32))

    st = np.array([0, 0, 0], np.int32)
    ct = np.array([3, 4, 5], np.int64)
    ps = np.ones((3, 16), f32)
    ids, out = np.zeros(2, np.int64), np.zeros((2, 16), f32)
    nsel = C.c_int64(0)

    def sel(s_=L.ptr(st), c=L.ptr(ct), p=L.ptr(ps), n=3, K=2, i=L.ptr(ids), o=L.ptr(out), ns=C.byref(nsel)):
        return lib.pcgx_pose_select(s_, c, p, n, K, i, o, ns)

    assert sel() == L.PCGX_OK and ids.tolist() == [2, 1] and nsel.value == 2
    for bad in (dict(s_=None), dict(c=None), dict(p=None), dict(i=None), dict(o=None), dict(ns=None), dict(n=-1), dict(K=-1),
                dict(n=2 ** 31), dict(K=2 ** 31)):
        assert sel(**bad) == INV, bad
    d_st, d_ct = torch.from_numpy(st).to(dev), torch.from_numpy(ct.astype(np.int32)).to(dev)
    d_ps = torch.from_numpy(ps).to(dev)
    d_ids = torch.zeros(2, dtype=torch.int32, device=dev)
    d_out = torch.zeros((2, 16), dtype=torch.float32, device=dev)
    d_ns = torch.zeros(1, dtype=torch.int32, device=dev)

    def seld(s_=d_st.data_ptr(), c=d_ct.data_ptr(), p=d_ps.data_ptr(), n=3, K=2, i=d_ids.data_ptr(), o=d_out.data_ptr(),
             ns=d_ns.data_ptr()):
        return lib.pcgx_pose_select_dev(s_, c, p, n, K, i, o, ns, None)

    assert seld() == L.PCGX_OK
    torch.cuda.synchronize()
    assert d_ids.cpu().numpy().tolist() == [2, 1] and int(d_ns.cpu().numpy()[0]) == 2
    for bad in (dict(s_=None), dict(c=None), dict(p=None), dict(i=None), dict(o=None), dict(ns=None), dict(n=-1), dict(K=-1),
                dict(n=2 ** 31), dict(K=2 ** 31)):
        assert seld(**bad) == INV, bad
