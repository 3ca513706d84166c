"""Scenes of the cylinder tests whose answers are known by construction (tests/test_m3c2_oracle.py pins the oracle on
them, tests/test_gpu_m3c2.py the library).  The lattice is tests/rays_scenes.py's."""
import numpy as np

f32, f64 = np.float32, np.float64

LATTICE_RHO = 0.5


def lattice_cylinders():
    """Cylinders through the 8 x 8 x 8 unit lattice with rho = 0.5, grouped by half length -> [(L, cores, axes, counts,
    sums)], counts and sums written down from the geometry.  Every a is a small dyadic number: any order sums exactly."""
    groups = {
        2.0: [
            ((3, 3, 3), (1, 0, 0), 5, 0.0, 10.0),      # x = 1 .. 5, a = -2 .. 2: both caps hold a point
            ((3, 3, 3), (2, 0, 0), 5, 0.0, 40.0),      # the axis is not normalised: the same points, a doubled
            ((3, 3, 3), (-0.25, 0, 0), 5, 0.0, 0.625),  # ... reversed and shortened
            ((4, 1, 6), (0, 0, 1), 4, -2.0, 6.0),      # z = 4 .. 7 of 8: a = -2 .. 1, the far cap is outside the lattice
            ((20, 20, 20), (1, 0, 0), 0, 0.0, 0.0),    # misses the box
            ((3, 3, 3), (0, 0, 0), 0, 0.0, 0.0),       # dd == 0: unusable
            ((0, 0, 0), (1, 1, 1), 2, 3.0, 9.0),       # the space diagonal from a corner: a = 0, 3 (6 6 > 4 3)
        ],
        1.5: [
            ((3.5, 3, 3), (0, 0, 1), 6, 0.0, 4.0),     # between two columns, both at exactly rho: z = 2, 3, 4 of each
            ((3.5, 3.5, 3), (0, 0, 1), 0, 0.0, 0.0),   # between four columns, sqrt(0.5) from each
            ((2, 5, 1.5), (0, -2, 0), 6, 0.0, 16.0),   # ... along -y with |d| = 2: y = 4, 5, 6 of each, a = 2, 0, -2
        ],
        3.0: [
            ((0, 0, 0), (1, 1, 0), 3, 6.0, 20.0),      # a face diagonal: dd = 2, a = 0, 2, 4 (4 4 <= 9 2 < 6 6)
            ((7, 7, 7), (-1, -1, 0), 3, 6.0, 20.0),
        ],
        0.25: [
            ((2.25, 5, 1), (1, 0, 0), 1, -0.25, 0.0625),  # one point, exactly on the cap
            ((2.5, 5, 1), (1, 0, 0), 0, 0.0, 0.0),        # halfway between two points, 0.5 from each
        ],
    }
    out = []
    for half, rows in groups.items():
        out.append((half, np.array([r[0] for r in rows], f32), np.array([r[1] for r in rows], f32),
                    np.array([r[2] for r in rows], np.int32), np.array([[r[3], r[4]] for r in rows], f64)))
    return out


DYADIC_RHO = 0.5
DYADIC_HALF = 2.0
DYADIC_AXES = ((2.0, 0.0, 0.0), (-0.5, 0.0, 0.0), (2.0 ** -10, 0.0, 0.0))  # dd = 4, 1/4, 2^-20: every product exact


def dyadic():
    """Points on and one ulp off the side surface and the caps of the cylinder about the origin along x with rho = 0.5,
    L = 2 -> (points, member).  Along DYADIC_AXES[0] = (2, 0, 0): a = 2 p.x, cc = 4 (p.y^2 + p.z^2)."""
    up = np.nextafter(f32(0.5), f32(1))
    cap = np.nextafter(f32(2), f32(3))
    rows = [  # (p, member)
        ([1, 0.5, 0], 1), ([1, up, 0], 0), ([-1, 0, -0.5], 1), ([-1, 0, -up], 0), ([1, 0.5, 0.5], 0),
        ([2, 0, 0], 1), ([cap, 0, 0], 0), ([-2, 0.25, 0], 1), ([-cap, 0.25, 0], 0),
        ([2, 0.5, 0], 1), ([-2, 0, 0.5], 1), ([cap, 0.5, 0], 0), ([2, up, 0], 0),
    ]
    return np.array([r[0] for r in rows], f32), np.array([r[1] for r in rows], bool)


PLANE_RHO = 0.1875  # the rim band 2 rho wide round a 4 x 4 patch is 9.4 % of the 8 x 8 plane


def plane_epochs(n=20_000, side=8.0, patch=(2.0, 6.0), lift=0.5, noise=0.0, seeds=(1, 2)):
    """Two samplings of the plane z = 0 over [0, side)^2; in epoch 2 the square patch[0] <= x, y < patch[1] is raised by
    `lift`.  Coordinates are multiples of 2^-10 (and lift is dyadic): noise-free, every a along (0, 0, 1) is 0 or lift
    exactly.  noise: a normal deviate in z, both epochs."""
    out = []
    for k, seed in enumerate(seeds):
        rng = np.random.default_rng(seed)
        p = np.zeros((n, 3), f64)
        p[:, :2] = rng.integers(0, int(side * 1024), (n, 2)) / 1024.0
        if noise:
            p[:, 2] = rng.normal(scale=noise, size=n)
        if k == 1:
            inside = ((p[:, :2] >= patch[0]) & (p[:, :2] < patch[1])).all(1)
            p[inside, 2] += lift
        out.append(np.ascontiguousarray(p, f32))
    return out
