"""NumPy restatement of ground segmentation's contract (include/pcgx.h, "ground"): the progressive morphological filter
on the caller's grid, on integer keys.  Independent of csrc/ground_terms.h: written from the comment, not from the code.

Everything is float32 with one rounding an operation, or an unsigned min / max over order-preserving keys, so the
library is compared with array_equal, the surface's bits included."""
import numpy as np

f32 = np.float32
EMPTY = np.uint32(0xFFFFFFFF)
HAG_NONE = np.array([0x7FC00000], np.uint32).view(f32)[0]


def key(z):
    """a < b => key(a) < key(b) as unsigned integers; -0.0 below +0.0"""
    b = np.ascontiguousarray(z, f32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(f32)


def cells(pts, origin, dims, cell, deleted=None):
    """the cell of every point, -1 where it is not live"""
    p = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    nx, ny = int(dims[0]), int(dims[1])
    with np.errstate(all="ignore"):
        fx = np.floor((p[:, 0] - f32(origin[0])) / f32(cell))
        fy = np.floor((p[:, 1] - f32(origin[1])) / f32(cell))
        live = np.isfinite(p).all(axis=1) & (fx >= 0) & (fx < f32(nx)) & (fy >= 0) & (fy < f32(ny))
    if deleted is not None:
        live &= ~np.asarray(deleted, bool)
    c = np.full(len(p), -1, np.int64)
    c[live] = fy[live].astype(np.int64) * nx + fx[live].astype(np.int64)
    return c


def raster(pts, c, dims):
    """S_0 as keys, (ny, nx), EMPTY where a cell has no live point"""
    S = np.full(int(dims[0]) * int(dims[1]), EMPTY, np.uint32)
    live = c >= 0
    np.minimum.at(S, c[live], key(np.ascontiguousarray(pts, f32).reshape(-1, 3)[live, 2]))
    return S.reshape(int(dims[1]), int(dims[0]))


def _square(a, h, op):
    """op over the (2 h + 1)^2 square clipped to the grid, by shift-and-combine along x, then along y"""
    for axis in (1, 0):
        a = np.moveaxis(a, axis, 1)
        out = a.copy()
        for d in range(1, min(h, a.shape[1] - 1) + 1):
            out[:, :-d] = op(out[:, :-d], a[:, d:])
            out[:, d:] = op(out[:, d:], a[:, :-d])
        a = np.moveaxis(out, 1, axis)
    return np.ascontiguousarray(a)


def opening(S, h):
    """S_k -> S_{k+1}: empty cells take no part in the erosion (they are above every key) nor in the dilation (below)"""
    E = _square(S, h, np.minimum)
    D = _square(np.where(E == EMPTY, np.uint32(0), E), h, np.maximum)
    return np.where(D == 0, EMPTY, D).astype(np.uint32)


def surfaces(pts, origin, dims, cell, half, deleted=None):
    """-> (c, [S_0, S_1, ..., S_n_win])"""
    c = cells(pts, origin, dims, cell, deleted)
    S = [raster(pts, c, dims)]
    for h in half:
        S.append(opening(S[-1], int(h)))
    return c, S


def ground(pts, origin, dims, cell, half, height, deleted=None):
    """-> dict(labels, sizes, ids (padded with -1 to n), n_groups, window, surface (ny, nx), hag)"""
    p = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    n = len(p)
    c, S = surfaces(p, origin, dims, cell, half, deleted)
    live = c >= 0
    z = p[live, 2]
    window = np.full(n, -1, np.int32)
    w = np.full(len(z), -1, np.int32)
    for k, ht in enumerate(height):
        with np.errstate(all="ignore"):
            ok = (z - unkey(S[k + 1].reshape(-1)[c[live]])) < f32(ht)
        w[(w < 0) & ~ok] = k
    window[live] = w
    labels = np.full(n, -1, np.int64)
    labels[live] = (w >= 0).astype(np.int64)
    g, o = np.flatnonzero(labels == 0), np.flatnonzero(labels == 1)
    ids = np.concatenate([g, o, np.full(n - len(g) - len(o), -1, np.int64)])
    last = S[-1]
    surface = np.where(last == EMPTY, f32(np.inf), unkey(last)).astype(f32)
    hag = np.full(n, HAG_NONE, f32)
    with np.errstate(all="ignore"):
        hag[live] = z - unkey(last.reshape(-1)[c[live]])
    return dict(labels=labels, sizes=np.array([len(g), len(o)], np.int64), ids=ids, n_groups=2, window=window,
                surface=surface, hag=hag)
