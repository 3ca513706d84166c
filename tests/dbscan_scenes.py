"""The scenes the density clustering tests share (tests/test_dbscan_oracle.py pins what each is for, the GPU tests run
them): built once per process, never modified."""
import numpy as np

from pcgol_amd import synth

f32 = np.float32
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def uniform():
    """the clusters tests' cloud"""
    return cached("uniform", lambda: synth.uniform_cloud(20_000, 1.0, 71))


def seven_points(swap=False):
    """ids 0 .. 6 on the x axis; r = 1, min_pts = 4: the points at +-0.9 are core, the point at 0 is at equal DistSq from
    both.  swap: ids 0 and 5 change places"""
    x = f32([0.9, 1.3, 1.7, 0.0, -1.7, -0.9, -1.3])
    if swap:
        x[[0, 5]] = x[[5, 0]]
    pts = np.zeros((7, 3), f32)
    pts[:, 0] = x
    return pts


def chain(cut=False, n=50_000):
    """n points 0.25 apart on the x axis (exact in float32), ids shuffled -> (pts, pos): pos[id] = the point's place
    along the line.  cut: the points at places 999, 1999, ... are NaN (deleted): 50 pieces of 999"""
    def make():
        perm = np.random.default_rng(60).permutation(n)  # the k-th point along the line has id perm[k]
        pts = np.zeros((n, 3), f32)
        pts[perm, 0] = f32(0.25) * np.arange(n, dtype=f32)
        pos = np.empty(n, np.int64)
        pos[perm] = np.arange(n)
        if cut:
            pts[pos % 1000 == 999] = np.nan
        return pts, pos
    return cached(("chain", cut, n), make)


def lattice():
    """a 48 x 48 lattice of spacing 1/16 in the plane z = 0 with holes (a random 45 % kept), ids shuffled"""
    def make():
        rng = np.random.default_rng(5)
        keep = rng.random(48 * 48) < 0.45
        ij = np.stack(np.divmod(np.nonzero(keep)[0], 48), axis=1)
        pts = np.zeros((len(ij), 3), f32)
        pts[:, :2] = ij.astype(f32) / f32(16)
        return np.ascontiguousarray(pts[rng.permutation(len(pts))])
    return cached("lattice", make)
