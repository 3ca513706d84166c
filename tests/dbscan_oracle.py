"""NumPy oracle of density clustering and radius outlier removal: the contracts of include/pcgx.h ("density clusters",
pcgx_ror_filter), restated.  NumPy only, on cluster_oracle's pairs, components and ranking.

Neighbourhood  N(i) = the points p with DistSq(p, point i) < radius^2, DistSq the float32 expression of cluster_oracle.
               A deleted point is given as NaN coordinates: nobody's neighbour.
Usable point   i in N(i).
Core point     usable and |N(i)| >= min_pts (the point counts itself; every member counts, core or not).
Core edge      both core, j in N(i).
Border point   usable, not core, a core point in N(i): it goes with the core neighbour of the smallest (DistSq, id).
Noise          every other point.
Clusters       the components of the core points plus their border points; size and smallest id over both; the size
               range, the numbering and the outputs are cluster_oracle.rank_and_group's.
kind           0 noise, 1 border, 2 core, whatever the size range.

Coincident points are one site (they have one neighbourhood, one count and one kind), so a heap of thousands of copies
stays cheap: a site's count is the sum of the multiplicities of the sites in reach, its own included."""
import numpy as np

import cluster_oracle as CO

f32 = CO.f32
NOISE, BORDER, CORE = 0, 1, 2


def beats(d, i, best_d, best_i):
    """does the core candidate (d, i) beat (best_d, best_i)?  float32 distances; a NaN beats nobody"""
    d, best_d = f32(d), f32(best_d)
    return bool(d < best_d or (d == best_d and int(i) < int(best_i)))


def is_core(own, count, min_pts):
    return bool(own) and int(count) >= int(min_pts)


def analyse(pts, radius, min_pts):
    """-> dict(name [n] (the smallest id of the point's cluster, -1 noise), kind [n] uint8, count [n] (|N(i)|, 0 for an
    unusable point), multi [n] bool (a border point with core neighbours in two or more components), tied [n] bool (...
    and its two nearest core neighbours, of different components, at equal DistSq))"""
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    n = len(pts)
    name = np.full(n, -1, np.int64)
    kind = np.zeros(n, np.uint8)
    count = np.zeros(n, np.int64)
    multi = np.zeros(n, bool)
    tied = np.zeros(n, bool)
    out = dict(name=name, kind=kind, count=count, multi=multi, tied=tied)
    idx = np.nonzero(CO.usable(pts, radius))[0]
    if len(idx) == 0:
        return out
    key = pts[idx].view(np.uint32).astype(np.int64)
    _, first, site, mult = np.unique(key, axis=0, return_index=True, return_inverse=True, return_counts=True)
    site = site.reshape(-1)
    sp = pts[idx][first]
    ns = len(sp)
    a, b = CO.site_pairs(sp, radius)
    cnt = mult.astype(np.int64)
    np.add.at(cnt, a, mult[b])
    count[idx] = cnt[site]
    core_s = cnt >= int(min_pts)
    low_s = np.full(ns, n, np.int64)  # a site's smallest id
    np.minimum.at(low_s, site, idx)
    cc = core_s[a] & core_s[b]
    root = CO.components(ns, a[cc], b[cc])  # (of a site that is not core: itself, unused)
    # border sites: the candidate pairs (border site a, core site b), the best (DistSq, smallest id of b) first
    bc = ~core_s[a] & core_s[b]
    ba, bb = a[bc], b[bc]
    comp_s = np.where(core_s, root, -1)
    multi_s = np.zeros(ns, bool)
    tied_s = np.zeros(ns, bool)
    if len(ba):
        d = CO.dist_sq(sp[bb], sp[ba])
        order = np.lexsort((low_s[bb], d, ba))
        ba, bb, d = ba[order], bb[order], d[order]
        head = np.ones(len(ba), bool)
        head[1:] = ba[1:] != ba[:-1]
        comp_s[ba[head]] = root[bb[head]]
        best_root = comp_s[ba]  # the chosen component, per pair
        other = root[bb] != best_root
        np.logical_or.at(multi_s, ba, other)
        best_d = np.zeros(ns, f32)
        best_d[ba[head]] = d[head]
        np.logical_or.at(tied_s, ba, other & (d == best_d[ba]))
    member_s = comp_s >= 0
    kind[idx] = np.where(core_s, CORE, np.where(member_s, BORDER, NOISE))[site].astype(np.uint8)
    multi[idx] = multi_s[site]
    tied[idx] = tied_s[site]
    low_c = np.full(ns, n, np.int64)  # per component (its root site): the smallest id over core and border points
    np.minimum.at(low_c, comp_s[member_s], low_s[member_s])
    nm = np.full(ns, -1, np.int64)
    nm[member_s] = low_c[comp_s[member_s]]
    name[idx] = nm[site]
    return out


def dbscan(pts, radius, min_pts, min_size=1, max_size=0):
    """-> (labels [n] int64, C, sizes [n] int64 zero padded, ids [n] int64 -1 padded, kind [n] uint8)"""
    r = analyse(pts, radius, min_pts)
    labels, c, sizes, ids = CO.rank_and_group(len(r["name"]), r["name"], min_size, max_size)
    return labels, c, sizes, ids, r["kind"]


def ror_keep(xyz, radius, min_neighbors, negative=False):
    """xyz (n, 3) float32 -> bool [n]: the records pcgx_ror_filter keeps"""
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    finite = np.all(np.isfinite(xyz), axis=1)
    keep = np.zeros(len(xyz), bool)
    if finite.any():
        core = analyse(xyz[finite], radius, min_neighbors)["kind"] == CORE
        keep[np.nonzero(finite)[0]] = ~core if negative else core
    return keep
