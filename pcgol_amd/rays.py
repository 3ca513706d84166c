"""Small tasks on top of the ray queries (KDTree.RayCast / RayPierce, include/pcgx.h "ray queries"; extension: no
reference parity): which points a viewpoint sees, which points a scan's beams passed through, a range image of a map.
The ray arithmetic is the library's; what is derived here (s = along / |d|^2, depths) is float64 NumPy."""
import ctypes as C

import numpy as np

from . import _lib as L


def tree_points(tree):
    """The tree's points (n,3) float32 in id order, deleted ones included."""
    n = tree.Len()
    ids = np.arange(n, dtype=np.int64)
    out = np.empty((n, 3), np.float32)
    if n:
        L.check(L.lib().pcgx_kdtree_points(tree._h, L.ptr(ids), C.c_int64(n), L.ptr(out)))
    return out


def Visible(tree, viewpoint, radius, slack):
    """The ids (int64 ascending) of the tree's points seen from `viewpoint`: one ray per point i with d = p_i -
    viewpoint and s in [0, 1 - slack]; point i is visible iff its ray has no hit, i.e. no point of the tree lies within
    `radius` of the segment from the viewpoint to where it stops short of p_i.  `slack` (a fraction of the distance)
    keeps p_i and its own surface patch out of its ray: of the order of radius / distance, larger for grazing views.
    A deleted point is reported as seen or not like any other position; filter with the ids you deleted."""
    pts = tree_points(tree)
    vp = np.asarray(viewpoint, np.float32).reshape(1, 3)
    d = pts - vp  # float32, as the caller of the ABI would form it
    o = np.broadcast_to(vp, pts.shape)
    ids, _, _ = tree.RayCast(o, d, radius, 0.0, np.float32(1.0) - np.float32(slack))
    return np.nonzero(ids < 0)[0].astype(np.int64)


def SeeThrough(tree, origins, endpoints, radius, margin):
    """Pierced counts (int32 (Len(),)) of a scan's beams: beam j runs from origins[j] to endpoints[j] and is stopped
    `margin` (a fraction of its length) short of its return, so the surface it ended on is not counted.  A map point
    that later beams passed through was not solid -- free-space carving:

        counts = rays.SeeThrough(tree, origins, endpoints, radius, margin)
        tree.DeletePoints(np.nonzero(counts >= k)[0])
    """
    o = L.f32c(origins).reshape(-1, 3)
    e = L.f32c(endpoints).reshape(-1, 3)
    if len(o) == 1 and len(e) != 1:
        o = np.ascontiguousarray(np.broadcast_to(o, e.shape))
    return tree.RayPierce(o, e - o, radius, 0.0, np.float32(1.0) - np.float32(margin))


def spherical_rays(origin, azimuths, elevations):
    """The rays of a spinning sensor at `origin`: (origins, directions) float32 (len(elevations) * len(azimuths), 3),
    row-major over (elevation, azimuth), directions of unit length up to float32 rounding:
    (cos el cos az, cos el sin az, sin el), angles in radians."""
    az = np.asarray(azimuths, np.float64).reshape(1, -1)
    el = np.asarray(elevations, np.float64).reshape(-1, 1)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az)], axis=-1)
    d = np.ascontiguousarray(d.reshape(-1, 3), np.float32)
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(origin, np.float32).reshape(1, 3), d.shape))
    return o, d


def RangeImage(tree, origin, azimuths, elevations, radius):
    """A range image of the tree seen from `origin` -> (depth float64 (len(elevations), len(azimuths)), ids int64, same
    shape).  depth is the metric distance along the ray to its first hit, along / |d|, +inf where the ray misses;
    ids is -1 there."""
    o, d = spherical_rays(origin, azimuths, elevations)
    ids, along, _ = tree.RayCast(o, d, radius)
    d64 = d.astype(np.float64)
    dd = (d64[:, 0] * d64[:, 0] + d64[:, 1] * d64[:, 1]) + d64[:, 2] * d64[:, 2]
    depth = np.where(ids >= 0, along / np.sqrt(dd), np.inf)
    shape = (len(np.atleast_1d(elevations)), len(np.atleast_1d(azimuths)))
    return depth.reshape(shape), ids.reshape(shape)
