"""Scenes of the ray tests whose answers are known by construction (tests/test_rays_oracle.py pins the oracle on them,
tests/test_gpu_rays.py the library)."""
import numpy as np

f32, f64 = np.float32, np.float64

LATTICE_RHO = 0.5


def lattice_id(x, y, z):
    return (x * 8 + y) * 8 + z


def lattice():
    """The 8 x 8 x 8 unit lattice, id = (x 8 + y) 8 + z."""
    g = np.arange(8, dtype=f32)
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3))


def lattice_rays():
    """Axis-parallel and diagonal rays through the lattice with rho = 0.5 -> (o, d, s_min, s_max, ids, along, off_sq,
    counts), the last four written down from the geometry: (o, d, s_min, s_max, members, first, along, off_sq)."""
    R = range(8)
    inf = np.inf
    rows = []
    for j, k in ((0, 0), (3, 4), (7, 7)):  # along x from outside: the whole row, the first at a = 1
        rows.append(((-1, j, k), (1, 0, 0), 0, inf, [(x, j, k) for x in R], (0, j, k), 1.0, 0.0))
    rows += [
        ((-1, 3, 4), (2, 0, 0), 0, inf, [(x, 3, 4) for x in R], (0, 3, 4), 2.0, 0.0),  # d is not normalised: a = 2
        ((-1, -1, -1), (1, 1, 1), 0, inf, [(i, i, i) for i in R], (0, 0, 0), 3.0, 0.0),  # the space diagonal
        ((-1, -1, 5), (1, 1, 0), 0, inf, [(i, i, 5) for i in R], (0, 0, 5), 2.0, 0.0),  # a face diagonal
        ((-1, 2, 2), (1, 0, 0), 3.5, 5, [(3, 2, 2), (4, 2, 2)], (3, 2, 2), 4.0, 0.0),  # a range inside the row
        ((-1, 2, 2), (-1, 0, 0), 0, inf, [], None, 0.0, 0.0),  # pointing away
        ((-1, 2, 2), (-1, 0, 0), -3, 0, [(0, 2, 2), (1, 2, 2), (2, 2, 2)], (2, 2, 2), -3.0, 0.0),  # ... a negative s_min
        # between two rows, both at exactly rho: 16 members, the first a tie at a = 1 that the smaller id wins
        ((-1, 0.5, 6), (1, 0, 0), 0, inf, [(x, y, 6) for x in R for y in (0, 1)], (0, 0, 6), 1.0, 0.25),
        ((3.5, 3.5, -2), (0, 0, 1), 0, inf, [], None, 0.0, 0.0),  # between four columns, sqrt(0.5) from each
        ((3, 3, 3), (0, 0, 1), 0, inf, [(3, 3, z) for z in range(3, 8)], (3, 3, 3), 0.0, 0.0),  # starts on a point
        ((5, 9, 1), (0, -1, 0), 0, inf, [(5, y, 1) for y in R], (5, 7, 1), 2.0, 0.0),  # along -y
        ((20, 20, 20), (1, 0, 0), 0, inf, [], None, 0.0, 0.0),  # misses the box
    ]
    o = np.array([r[0] for r in rows], f32)
    d = np.array([r[1] for r in rows], f32)
    s_min = np.array([r[2] for r in rows], f32)
    s_max = np.array([r[3] for r in rows], f32)
    ids = np.array([-1 if r[5] is None else lattice_id(*r[5]) for r in rows], np.int64)
    along = np.array([r[6] for r in rows], f64)
    off = np.array([r[7] for r in rows], f64)
    counts = np.zeros(512, np.int32)
    for r in rows:
        for m in r[4]:
            counts[lattice_id(*m)] += 1
    return o, d, s_min, s_max, ids, along, off, counts


DYADIC_RHO = 0.5
DYADIC_D = (2.0, 0.0, 0.0)  # not unit: dd = 4, a = 2 p.x, cc = 4 (p.y^2 + p.z^2): every product exact


def dyadic():
    """Points on and just off the tube's surface and the range's ends, the ray from the origin along DYADIC_D with
    rho = 0.5 -> (points, s_min, s_max, member): row i is its own (point, range) pair."""
    up, dn = np.nextafter(f32(0.5), f32(1)), np.nextafter(f32(0.5), f32(0))
    rows = [  # (p, s_min, s_max, member)
        ([3, 0.5, 0], 0, 4, 1), ([3, up, 0], 0, 4, 0), ([3, 0, -0.5], 0, 4, 1), ([3, 0, -up], 0, 4, 0),
        ([3, 0.5, 0.5], 0, 4, 0), ([3, dn, 0], 0, 4, 1),
        ([1, 0, 0], 0.5, 4, 1), ([np.nextafter(f32(1), f32(0)), 0, 0], 0.5, 4, 0),  # at s_min, and just before it
        ([8, 0.25, 0], 0, 4, 1), ([np.nextafter(f32(8), f32(9)), 0.25, 0], 0, 4, 0),  # at s_max, and just beyond it
        ([-2, 0, 0.5], -1, 4, 1), ([np.nextafter(f32(-2), f32(-3)), 0, 0.5], -1, 4, 0),  # a negative s_min
    ]
    return (np.array([r[0] for r in rows], f32), np.array([r[1] for r in rows], f32), np.array([r[2] for r in rows], f32),
            np.array([r[3] for r in rows], bool))


def sphere(n=5000, radius=1.0, seed=4):
    """n points on a sphere about the origin (a Fibonacci spiral, jittered a little)."""
    rng = np.random.default_rng(seed)
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    s = np.sqrt(1.0 - z * z)
    p = np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1) * radius
    return np.ascontiguousarray(p + rng.normal(scale=1e-4, size=p.shape), f32)


SPHERE_VIEW = (0.0, 0.0, 6.0)
SPHERE_RADIUS = 0.05  # the points' spacing (sqrt(4 pi / 5000)): no ray slips between them (at 0.03 some do)
SPHERE_SLACK = 0.02   # the rays stop 2 % short: 0.1 at the distance of 5 .. 6, beyond the point's own patch
