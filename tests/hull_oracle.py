"""The group footprints contract (include/pcgx.h, "group footprints") restated in exact arithmetic: no test inside.

Every float32 coordinate is an integer multiple of 2^-149, so a point becomes a pair of Python integers and every
orientation, area and rectangle below is exact: the monotone chain (lower, then upper) over the places of a group
sorted lexicographically, a place by its smallest id, strict turns only; the polygon's area as a Fraction; the area of
the enclosing rectangle along every hull edge as a Fraction, and the smallest of them."""
import collections
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_oracle as GO  # noqa: E402

SCALE = 1 << 149
UNIT = Fraction(1, SCALE)
Footprints = collections.namedtuple("Footprints", "hull_sizes hull_ids area rect_area")


def integers(v):
    """float32 values -> exact Python integers in units of 2^-149 (-0 and +0 are both 0; 0 for a value that is not
    finite: its point is no live member)"""
    return [int(Fraction(float(x)) * SCALE) if np.isfinite(x) else 0 for x in np.asarray(v, np.float32).ravel()]


def orient(a, b, c):
    """the exact sign of (a - c) x (b - c): +1 when c is left of the line from a to b"""
    d = (a[0] - c[0]) * (b[1] - c[1]) - (a[1] - c[1]) * (b[0] - c[0])
    return (d > 0) - (d < 0)


def hull(places):
    """places: [(x, y, id)] exact integers, one entry per place, sorted by (x, y) -> the strict vertices counter-clockwise
    from the least place: Andrew's monotone chain, a point that does not turn strictly left is popped"""
    if len(places) <= 2:
        return list(places)
    lower, upper = [], []
    for p in places:
        while len(lower) >= 2 and orient(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(places):
        while len(upper) >= 2 and orient(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]  # (all on one line: [least, greatest])


def places_of(X, Y, ids):
    """the live ids of one group -> one (x, y, smallest id) per place, sorted lexicographically"""
    best = {}
    for i in ids:
        k = (X[i], Y[i])
        if k not in best or i < best[k]:
            best[k] = i
    return sorted((x, y, i) for (x, y), i in best.items())


def polygon_area(v):
    """exact area of the polygon v (Fraction, in squared units of the input)"""
    if len(v) < 3:
        return Fraction(0)
    s = sum((v[k][0] - v[0][0]) * (v[k + 1][1] - v[0][1]) - (v[k][1] - v[0][1]) * (v[k + 1][0] - v[0][0])
            for k in range(1, len(v) - 1))
    return Fraction(s, 2) * UNIT * UNIT


def edge_rect_areas(v):
    """exact area of the enclosing rectangle along every edge of the hull v (h >= 3), in edge order"""
    out = []
    nz = [abs(c) for p in v for c in p[:2] if c]
    sh = min((c & -c).bit_length() - 1 for c in nz)  # the power of two every coordinate shares
    if max(nz) >> sh < 1 << 29:  # the same integers in int64: |s|, |t| < 2^61, only the last product is wide
        V = np.array([[p[0] >> sh, p[1] >> sh] for p in v], np.int64)
        for k in range(len(V)):
            d = V[(k + 1) % len(V)] - V[k]
            R = V - V[k]
            s, t = R @ d, R[:, 1] * d[0] - R[:, 0] * d[1]
            out.append(Fraction(int(s.max() - s.min()) * int(t.max() - t.min()), int(d @ d)) * (UNIT * UNIT * (1 << 2 * sh)))
        return out
    for k in range(len(v)):
        a, b = v[k], v[(k + 1) % len(v)]
        dx, dy = b[0] - a[0], b[1] - a[1]
        s = [(p[0] - a[0]) * dx + (p[1] - a[1]) * dy for p in v]
        t = [(p[1] - a[1]) * dx - (p[0] - a[0]) * dy for p in v]
        out.append(Fraction((max(s) - min(s)) * (max(t) - min(t)), dx * dx + dy * dy) * UNIT * UNIT)
    return out


def group_hulls(points, ids, sizes, n_groups=None, cap_ids=None):
    """points (n, 3) float32 (the tree's); ids any ints; sizes (cap_groups,) -> (Footprints over cap_groups rows:
    hull_sizes int64, hull_ids int64 (cap_ids,) with -1 behind the hulls, area float64 (the exact area rounded once),
    rect_area float64 (the exact minimum over the edges rounded once; 0 for h < 3),
    dict(D: the diagonal of each group's xy box, members: the live points per group, hulls: the vertices as float64 (h, 2)))"""
    P = np.asarray(points, np.float32).reshape(-1, 3)
    ids = np.asarray(ids, np.int64).reshape(-1)
    sizes = np.asarray(sizes, np.int64).reshape(-1)
    cap_groups = len(sizes)
    cap_ids = len(ids) if cap_ids is None else cap_ids
    G = cap_groups if n_groups is None else min(max(int(n_groups), 0), cap_groups)
    X, Y = integers(P[:, 0]), integers(P[:, 1])
    hs = np.zeros(cap_groups, np.int64)
    hid = np.full(cap_ids, -1, np.int64)
    area, rect_area, D = np.zeros(cap_groups), np.zeros(cap_groups), np.zeros(cap_groups)
    members, hulls, at = [], [], 0
    for g, (b, e) in enumerate(GO.slices(sizes, G, cap_ids)):
        part = ids[b:e]
        part = part[GO.live(P, part)]
        members.append(P[part])
        v = hull(places_of(X, Y, [int(i) for i in part]))
        hs[g] = len(v)
        hid[at:at + len(v)] = [p[2] for p in v]
        at += len(v)
        hulls.append(P[[p[2] for p in v], :2].astype(np.float64).reshape(-1, 2))
        if len(part):
            xy = P[part, :2].astype(np.float64)
            D[g] = float(np.linalg.norm(xy.max(axis=0) - xy.min(axis=0)))
        area[g] = float(polygon_area(v))
        if len(v) >= 3:
            rect_area[g] = float(min(edge_rect_areas(v)))
    return Footprints(hs, hid, area, rect_area), dict(D=D, members=members, hulls=hulls)
