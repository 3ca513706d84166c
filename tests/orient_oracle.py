"""NumPy oracle of consistent normal orientation (include/pcgx.h, "consistent normal orientation"; csrc/orient.hip,
csrc/orient_terms.h), restated.  NumPy only.

  neighbours   N(i) = {j : (dx dx + dy dy) + dz dz < f32(r) f32(r)}, all float32, strict, over the live points; a deleted
               point or one with a NaN / infinite coordinate is in no list, not its own either.
  usable       i in N(i), and the normal's three components are finite and not all zero.
  edge         {i, j}, i != j, both usable, j in N(i).  c = (nx_i nx_j + ny_i ny_j) + nz_i nz_j in float64 from the float32
               components; s = (c < 0).
  edge order   |c| descending, then min(i, j), then max(i, j): strict and total.
  rounds       every component with a leaving edge takes its first leaving edge; all are added at once.
  parity       pi_i = XOR of s along the forest path from i to the smallest member id of its component.
  sigma        mode 0: 0.  mode 1: the member with the largest float32 h = (px ux + py uy) + pz uz (after h + 0; ties to
               the smallest id) is the anchor; sigma = (its normal after pi, dotted with u as c is formed) < 0.  mode 2:
               t_i = (n'x ex + n'y ey) + n'z ez in float64, e = f64(v) - f64(p_i); sigma = #(t < 0) > #(t > 0).
  NaN handles  a tree holding a NaN coordinate is out of order: N is the handle's own Range lists (graph_lists), need not
               be symmetric, and a component takes the first of the leaving edges its own members see and the edges
               other components took into it in that round (boruvka's `seen`).
  outputs      flipped = pi ^ sigma (0 where unusable); normals_out = the sign bits inverted where flipped; component =
               the smallest member id (-1 where unusable); n_components; n_open = components with a leaving edge left.
"""
import numpy as np

f32, f64, u32, u64 = np.float32, np.float64, np.uint32, np.uint64


def live_points(points, deleted=None):
    p = np.array(points, f32).reshape(-1, 3)
    if deleted is not None and len(deleted):
        p[np.asarray(deleted, np.int64)] = np.nan  # never DistSq < bound: nobody's neighbour, not its own either
    return p


def normal_ok(normals):
    m = np.asarray(normals, f32).reshape(-1, 3)
    return np.isfinite(m).all(axis=1) & ~(m == 0).all(axis=1)


def agreement(ni, nj):
    """c of the rows of two float32 (k, 3) arrays, float64, the two additions in the contract's order"""
    a, b = np.asarray(ni, f32).astype(f64).reshape(-1, 3), np.asarray(nj, f32).astype(f64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def graph(points, normals, radius, deleted=None):
    """-> (usable bool (n,), lo, hi int64 (m,), c float64 (m,)): every edge once, lo < hi, by looking at every pair"""
    p = live_points(points, deleted)
    m = np.asarray(normals, f32).reshape(-1, 3)
    n = len(p)
    bound = f32(radius) * f32(radius)
    nok = normal_ok(m)
    usable = np.zeros(n, bool)
    los, his = [], []
    step = max(1, (1 << 24) // max(n, 1))
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, n, step):
            q = p[a:a + step]
            dx, dy, dz = q[:, None, 0] - p[None, :, 0], q[:, None, 1] - p[None, :, 1], q[:, None, 2] - p[None, :, 2]
            inside = ((dx * dx + dy * dy) + dz * dz) < bound
            rows = np.arange(a, a + len(q))
            usable[rows] = inside[np.arange(len(q)), rows] & nok[rows]
            inside &= nok[None, :] & nok[rows][:, None]
            i, j = np.nonzero(inside)
            i = i + a
            keep = i < j
            los.append(i[keep])
            his.append(j[keep])
    lo = np.concatenate(los) if los else np.zeros(0, np.int64)
    hi = np.concatenate(his) if his else np.zeros(0, np.int64)
    both = usable[lo] & usable[hi]  # (a usable neighbour is always in its own list; this is for the form's sake)
    lo, hi = lo[both].astype(np.int64), hi[both].astype(np.int64)
    return usable, lo, hi, agreement(m[lo], m[hi])


def graph_lists(normals, offs, ids):
    """the graph over a handle's own Range lists (CSR: offs [n + 1], ids), for a tree a NaN coordinate has put out of
    order, where no brute force says what the neighbourhoods are and j in N(i) need not mean i in N(j) ->
    (usable, lo, hi, c, from_lo, from_hi): from_lo: hi is in N(lo); from_hi: lo is in N(hi)"""
    m = np.asarray(normals, f32).reshape(-1, 3)
    offs, ids = np.asarray(offs, np.int64), np.asarray(ids, np.int64)
    n = len(offs) - 1
    src = np.repeat(np.arange(n), np.diff(offs))
    usable = np.zeros(n, bool)
    usable[src[src == ids]] = True
    usable &= normal_ok(m)
    arc = (src != ids) & usable[src] & usable[ids]
    src, dst = src[arc], ids[arc]
    a, b = np.minimum(src, dst), np.maximum(src, dst)
    key, inv = np.unique(a * n + b, return_inverse=True)
    lo, hi = key // max(n, 1), key % max(n, 1)
    from_lo, from_hi = np.zeros(len(key), bool), np.zeros(len(key), bool)
    from_lo[inv[src < dst]] = True
    from_hi[inv[src > dst]] = True
    return usable, lo, hi, agreement(m[lo], m[hi]), from_lo, from_hi


def edge_order(lo, hi, c):
    """the edges' indices, first edge first"""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    key = lo * (int(hi.max()) + 1 if len(hi) else 1) + hi
    if np.all(key[1:] >= key[:-1]):  # (graph() lists them by (lo, hi): a stable sort by |c| alone is the order)
        return np.argsort(-np.abs(c), kind="stable")
    return np.lexsort((hi, lo, -np.abs(c)))


def edge_before(ce, ie, je, cf, i_f, jf):
    """one comparison of the edge order, as csrc/orient_terms.h's orient_before"""
    e = (-abs(ce), min(ie, je), max(ie, je))
    f = (-abs(cf), min(i_f, jf), max(i_f, jf))
    return e < f


class _UF:
    def __init__(self, n):
        self.p = np.arange(n)

    def find(self, x):
        p = self.p
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x


def kruskal(n, lo, hi, c):
    """the minimum spanning forest under the edge order -> indices of its edges"""
    uf = _UF(n)
    out = []
    for e in edge_order(lo, hi, c):
        a, b = uf.find(lo[e]), uf.find(hi[e])
        if a != b:
            uf.p[a] = b
            out.append(e)
    return np.array(sorted(out), np.int64)


def boruvka(n, lo, hi, c, rounds=None, seen=None):
    """a literal simulation of the rounds -> (indices of the forest's edges, rounds that added an edge, components that
    still have a leaving edge).  rounds None: until no component has one.  seen = (from_lo, from_hi) (graph_lists): a
    component takes the first leaving edge that one of ITS members sees, or that another component took into it."""
    leaving = edge_order(lo, hi, c)  # the edges between two components, first edge first
    one_sided = seen is not None and not (np.all(seen[0]) and np.all(seen[1]))
    label = np.arange(n)
    chosen_all = []
    done = 0
    while True:
        la, lb = label[lo[leaving]], label[hi[leaving]]
        out = la != lb
        leaving, la, lb = leaving[out], la[out], lb[out]  # (an edge inside a component stays inside)
        present = np.zeros(n, bool)
        present[la] = True
        present[lb] = True
        k = int(present.sum())
        if len(leaving) > 4 * n and k * k <= 1 << 26 and not one_sided:
            # of the edges between one pair of components only the first can ever be taken: drop the others (thousands
            # of coincident points make millions of them); the first place per pair by the trick explained below
            number = np.cumsum(present) - 1
            a, b = number[la], number[lb]
            pair = np.minimum(a, b) * k + np.maximum(a, b)
            table = np.full(k * k, -1, np.int64)
            table[pair[::-1]] = np.arange(len(pair))[::-1]
            keep = np.sort(table[table >= 0])
            leaving, la, lb = leaving[keep], la[keep], lb[keep]
        # per component the place of its first leaving edge: of the writes to one slot the last one stays, so written
        # back to front the first place does
        place = np.arange(len(leaving))
        fa, fb = np.full(n, len(leaving), np.int64), np.full(n, len(leaving), np.int64)
        if one_sided:
            va, vb = seen[0][leaving], seen[1][leaving]
            fa[la[va][::-1]] = place[va][::-1]
            fb[lb[vb][::-1]] = place[vb][::-1]
            own = np.minimum(fa, fb)
            taker = np.nonzero(own < len(leaving))[0]
            into = np.where(la[own[taker]] == taker, lb[own[taker]], la[own[taker]])
            first = own.copy()
            np.minimum.at(first, into, own[taker])
        else:
            fa[la[::-1]] = place[::-1]
            fb[lb[::-1]] = place[::-1]
            first = np.minimum(fa, fb)
        open_comps = int((first < len(leaving)).sum())
        if open_comps == 0 or (rounds is not None and done >= rounds):
            break
        chosen = leaving[np.unique(first[first < len(leaving)])]
        uf = _UF(n)
        uf.p = label.copy()  # (labels are roots of themselves)
        for e in chosen:
            a, b = uf.find(lo[e]), uf.find(hi[e])
            assert a != b, "a strict order cannot close a cycle"
            uf.p[a] = b
        label = np.array([uf.find(x) for x in range(n)])
        chosen_all.append(chosen)
        done += 1
    forest = np.sort(np.concatenate(chosen_all)) if chosen_all else np.zeros(0, np.int64)
    return forest, done, open_comps


def anchor_key(h, ids):
    """csrc/orient_terms.h's orient_anchor_key -> uint64"""
    with np.errstate(invalid="ignore"):
        z = (np.asarray(h, f32) + f32(0.0)).astype(f32)
    b = z.view(u32).astype(u64)
    b = np.where(b & u64(0x80000000), (~b) & u64(0xffffffff), b | u64(0x80000000))
    return (b << u64(32)) | ((~np.asarray(ids).astype(u32)).astype(u64))


def flip_bits(normals, flipped):
    out = np.array(normals, f32).reshape(-1, 3).copy()
    w = out.view(u32)
    w[np.asarray(flipped, bool)] ^= u32(0x80000000)
    return out


def orient(points, normals, radius, mode=0, ref=None, rounds=None, deleted=None, lists=None):
    """the contract -> dict(flipped uint8 (n,), normals_out float32 (n, 3), component int64 (n,), n_components, n_open,
    rounds: the rounds that added an edge)"""
    p = live_points(points, deleted)
    m = np.array(normals, f32).reshape(-1, 3)
    n = len(p)
    seen = None
    if lists is None:
        usable, lo, hi, c = graph(points, m, radius, deleted)
    else:  # (the handle's own Range lists)
        usable, lo, hi, c, from_lo, from_hi = graph_lists(m, *lists)
        seen = (from_lo, from_hi)
    forest, done, n_open = boruvka(n, lo, hi, c, rounds, seen)
    s = (c[forest] < 0).astype(np.int64)
    adj = [[] for _ in range(n)]
    for e, se in zip(forest, s):
        adj[lo[e]].append((int(hi[e]), int(se)))
        adj[hi[e]].append((int(lo[e]), int(se)))
    comp = np.full(n, -1, np.int64)
    pi = np.zeros(n, np.int64)
    for r in range(n):  # ascending: the first unvisited member of a component is its smallest id
        if not usable[r] or comp[r] >= 0:
            continue
        comp[r] = r
        stack = [r]
        while stack:
            x = stack.pop()
            for y, se in adj[x]:
                if comp[y] < 0:
                    comp[y] = r
                    pi[y] = pi[x] ^ se
                    stack.append(y)
    sigma = np.zeros(n, np.int64)  # by component id
    roots = np.unique(comp[comp >= 0])
    if mode in (1, 2):
        ref = np.asarray(ref, f32)
        after = flip_bits(m, pi)
        ids = np.arange(n)
        if mode == 1:
            with np.errstate(invalid="ignore", over="ignore"):
                h = (p[:, 0] * ref[0] + p[:, 1] * ref[1]) + p[:, 2] * ref[2]
            key = anchor_key(h, ids)
            for r in roots:
                mem = ids[comp == r]
                a = mem[np.argmax(key[mem])]
                sigma[r] = 1 if agreement(after[a], ref)[0] < 0 else 0
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                e = ref.astype(f64)[None, :] - p.astype(f64)
                a64 = after.astype(f64)
                t = (a64[:, 0] * e[:, 0] + a64[:, 1] * e[:, 1]) + a64[:, 2] * e[:, 2]
                wrong, right = (t < 0) & usable, (t > 0) & usable
            for r in roots:
                mem = comp == r
                sigma[r] = 1 if wrong[mem].sum() > right[mem].sum() else 0
    flipped = np.where(usable, pi ^ sigma[np.maximum(comp, 0)], 0).astype(np.uint8)
    return dict(flipped=flipped, normals_out=flip_bits(m, flipped), component=comp, n_components=len(roots),
                n_open=int(n_open), rounds=done, usable=usable, forest=(lo[forest], hi[forest]))
