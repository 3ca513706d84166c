"""Scenes of the boundary tests (tests/test_boundary_oracle.py on the CPU, tests/test_gpu_boundary.py on the GPU).

lattice()  a 7 x 7 unit lattice in z = 0: at radius 1.5 an interior point sees its eight neighbours on the multiples of
           45 degrees (gap 7), an edge point five of them over a half turn (gap 31), a corner three over a quarter turn
           (gap 47).
plate()    a jittered 83 x 75 unit grid lifted onto a gentle height field, with two discs cut out: an outer rim and two
           holes, about 5 950 points, not a multiple of 64.  rim_distance() is the distance in the xy plane to the
           nearest of the three rims."""
import numpy as np

f32 = np.float32

LATTICE_RADIUS = 1.5
LATTICE_GAPS = {"interior": 7, "edge": 31, "corner": 47}

PLATE_NX, PLATE_NY = 83, 75
PLATE_JITTER = 0.25
PLATE_HOLES = (((27.3, 40.2), 8.0), ((61.8, 22.4), 5.0))  # (centre, radius)
PLATE_RADIUS = 3.0  # of the normals and of the boundary
PLATE_MIN_GAP = 16


def lattice():
    """-> (points (49, 3) float32, kind (49,): 0 interior, 1 edge, 2 corner)"""
    i, j = np.meshgrid(np.arange(7), np.arange(7), indexing="ij")
    pts = np.stack([i.ravel(), j.ravel(), np.zeros(49)], axis=1).astype(f32)
    on_i, on_j = (i.ravel() % 6) == 0, (j.ravel() % 6) == 0
    return pts, on_i.astype(int) + on_j.astype(int)


def plate_height(x, y):
    return 1.5 * np.sin(x / 13.0) * np.cos(y / 17.0)


def plate():
    """-> points (n, 3) float32, n about 5 950 and no multiple of 64"""
    rng = np.random.default_rng(20261)
    i, j = np.meshgrid(np.arange(PLATE_NX), np.arange(PLATE_NY), indexing="ij")
    xy = np.stack([i.ravel(), j.ravel()], axis=1) + rng.uniform(-PLATE_JITTER, PLATE_JITTER, (PLATE_NX * PLATE_NY, 2))
    keep = np.ones(len(xy), bool)
    for c, r in PLATE_HOLES:
        keep &= np.linalg.norm(xy - np.array(c), axis=1) >= r
    xy = xy[keep]
    pts = np.concatenate([xy, plate_height(xy[:, 0], xy[:, 1])[:, None]], axis=1).astype(f32)
    pts = np.ascontiguousarray(pts[rng.permutation(len(pts))])
    assert 5900 < len(pts) < 6000 and len(pts) % 64 != 0, len(pts)
    return pts


def rim_distance(pts):
    """the distance in the xy plane of every point to the nearest rim: the rectangle of the unjittered grid or a hole's
    circle (a jittered point may lie up to PLATE_JITTER beyond either: still a small distance)"""
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    d = np.minimum(np.minimum(np.abs(x), np.abs(PLATE_NX - 1 - x)), np.minimum(np.abs(y), np.abs(PLATE_NY - 1 - y)))
    for c, r in PLATE_HOLES:
        d = np.minimum(d, np.abs(np.hypot(x - c[0], y - c[1]) - r))
    return d
