"""float64 NumPy restatement of the FPFH descriptors (include/pcgx.h, pcgx_kdtree_fpfh; csrc/fpfh.hip,
csrc/fpfh_terms.h) over neighbour lists.

No reference counterpart exists: the header's comment is the contract, restated here.  For query s (point ps, normal
ns) and neighbour t (pt, nt), in float64 from the float32 inputs:
  d = pt - ps, f4 = |d|, a1 = ns . d / f4, a2 = nt . d / f4;
  |a1| < |a2|: (n1, n2, d, f3) = (nt, ns, -d, -a2), else (ns, nt, d, a1);
  v = d x n1, v /= |v|; w = n1 x v; f2 = v . n2; f1 = atan2(w . n2, n1 . n2);
  b1 = clamp(floor(11 (f1 + pi) / 2 pi), 0, 10), b2 = clamp(floor(11 (f2 + 1) / 2), 0, 10), b3 likewise from f3.
  Invalid (contributes nothing): float32 DistSq == 0, a normal that is zero or not finite, |v| == 0.
SPFH: c_q[f][b] = valid pairs of q with feature f in bin b, m_q = valid pairs, S_q = 100 c_q / m_q (0 where m_q == 0).
FPFH: w_i = 1 / DistSq(i, q) (float32 DistSq widened), W_f[b] = sum over the neighbours with DistSq > 0 of
  w_i S_i[f][b], T_f = sum_b W_f[b], F_q[f][b] = S_q[f][b] + (T_f > 0 ? 100 W_f[b] / T_f : 0).

A histogram is a discontinuous function of its inputs, so nothing here is compared "to a tolerance".  Every pair gets
an ADMISSIBLE SET of bins per feature -- one bin, unless the pair is FRAGILE:
  near an edge       a scaled value 11 (f + ..) / .. within EDGE = 1e-9 of an integer admits both neighbouring bins;
  near a swap tie    ||a1| - |a2|| < TIE = 1e-9: the bins of the swapped and of the unswapped triple are all admissible
                     (on symmetric shapes they coincide, and the pair is then not fragile);
  near-parallel      |d x n1| < PAR = 1e-6 |d| |n1| under either role assignment: every bin of f1 and f2 is admissible;
  validity           |v| below VEDGE = 1e-12 |d| |n1| (zero included: which cross product rounds to exactly 0 depends
                     on contraction), or a DistSq that underflows float32: the pair may count or not.
Per query, feature and bin: lo[b] = the pairs that certainly count and admit only b, hi[b] = the pairs that may count
and admit b; likewise m_lo, m_hi.  check() asserts lo <= c <= hi, sum_b c == m per feature, m_lo <= m <= m_hi, and --
on queries with no fragile pair of their own or of any neighbour -- |F - F_oracle| <= 2^-22 F_oracle with zeros
exact; and the CONDITION that keeps these checks decisive: at most 1 fragile pair in 1e5 valid ones, at most 1 % of
the queries left out of the float check.

Neighbour lists come from normals_oracle.brute_force_lists / range_lists (pinned elsewhere).  A list may leave out
neighbours at float32 DistSq == 0 (the point itself, coincident heaps): they contribute to nothing."""
import numpy as np

f32, f64 = np.float32, np.float64
BINS, LEN = 11, 33
EDGE, TIE, PAR, VEDGE = 1e-9, 1e-9, 1e-6, 1e-12
FLOAT_TOL = 2.0 ** -22
MAX_FRAGILE_SHARE = 1e-5
MAX_LEFT_OUT = 0.01


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _dot(a, b):
    return np.sum(a * b, axis=1)


def _role(n1, n2, d, f3):
    """scaled features x (m,3) of one role assignment, |v|, near-parallel, |v| at the edge of zero"""
    v = _cross(d, n1)
    vn = np.sqrt(_dot(v, v))
    scale = np.sqrt(_dot(d, d)) * np.sqrt(_dot(n1, n1))
    vu = v / vn[:, None]
    w = _cross(n1, vu)
    f2 = _dot(vu, n2)
    f1 = np.arctan2(_dot(w, n2), _dot(n1, n2))
    x = np.stack([BINS * (f1 + np.pi) / (2.0 * np.pi), BINS * (f2 + 1.0) / 2.0, BINS * (f3 + 1.0) / 2.0], axis=1)
    return x, vn, ~(vn >= PAR * scale), ~(vn >= VEDGE * scale)


def _onehot(b):
    return b[..., None] == np.arange(BINS)


def _bins(x):
    return np.clip(np.floor(np.nan_to_num(x, nan=0.0, posinf=1e9, neginf=-1e9)), 0, BINS - 1).astype(np.int64)


def _admit(x):
    """(m,3) scaled values -> (m,3,11) admissible bins: floor's, and both neighbours of an integer within EDGE"""
    x = np.nan_to_num(x, nan=0.0, posinf=1e9, neginf=-1e9)
    adm = _onehot(_bins(x))
    r = np.rint(x)
    near = np.abs(x - r) < EDGE
    both = _onehot(np.clip(r - 1, 0, BINS - 1).astype(np.int64)) | _onehot(np.clip(r, 0, BINS - 1).astype(np.int64))
    return adm | (near[..., None] & both)


def pair_bins(ps, ns, pt, nt):
    """Pairs (m,3) float32 each -> dict:
    bins (m,3) int64   the bins of this float64 evaluation (meaningful where `counted`);
    counted (m,) bool  valid by this evaluation;
    sure (m,) bool     certainly valid;  maybe (m,) bool  may count or not (validity within a rounding);
    adm (m,3,11) bool  admissible bins (all False where certainly invalid);
    fragile (m,) bool  maybe, or sure with more than one admissible bin in some feature."""
    ps, ns, pt, nt = (np.asarray(a, f32).reshape(-1, 3) for a in (ps, ns, pt, nt))
    m = len(ps)
    e = pt - ps
    dsq32 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    d = pt.astype(f64) - ps.astype(f64)
    ns64, nt64 = ns.astype(f64), nt.astype(f64)
    okn = np.all(np.isfinite(ns), axis=1) & np.all(np.isfinite(nt), axis=1) & np.any(ns != 0, axis=1) & np.any(nt != 0, axis=1)
    with np.errstate(all="ignore"):
        dd = _dot(d, d)
        f4 = np.sqrt(dd)
        a1 = _dot(ns64, d) / f4
        a2 = _dot(nt64, d) / f4
        xu, vnu, paru, vedu = _role(ns64, nt64, d, a1)
        xs, vns, pars, veds = _role(nt64, ns64, -d, -a2)
    with np.errstate(all="ignore"):  # (a1 or a2 is inf or NaN where a normal is: such a pair is invalid whatever follows)
        swap = np.abs(a1) < np.abs(a2)
        tie = ~(np.abs(np.abs(a1) - np.abs(a2)) >= TIE)
    x = np.where(swap[:, None], xs, xu)
    vn = np.where(swap, vns, vnu)
    adm = _admit(x) | (tie[:, None, None] & _admit(np.where(swap[:, None], xu, xs)))
    par = paru | pars
    adm[par, 0, :] = True
    adm[par, 1, :] = True
    vedge = np.where(swap, veds, vedu) | (tie & np.where(swap, vedu, veds))
    dsq_edge = (dd > 0) & (dd < 1e-37)  # float32 DistSq underflows: zero or not by a rounding
    adm[dsq_edge] = True
    counted = okn & (dsq32 > 0) & (vn > 0)
    maybe = okn & (dsq_edge | (vedge & (dsq32 > 0)))
    sure = okn & (dsq32 > 0) & ~dsq_edge & ~vedge
    adm[~(sure | maybe)] = False
    fragile = maybe | (sure & np.any(adm.sum(axis=2) > 1, axis=1))
    assert m == 0 or np.all(adm[sure].sum(axis=2) >= 1)
    return dict(bins=_bins(x), counted=counted, sure=sure, maybe=maybe, adm=adm, fragile=fragile)


def spfh(points, normals, qids, offs, ids, mult=None, chunk=1 << 19):
    """The rows `qids` (ids of the queries, each a point of the cloud) with neighbour lists (offs, ids) -> dict (mult:
    how many times each list entry stands in the neighbourhood -- a heap of coincident points with one normal is
    one entry taken `mult` times; None: once):
    counts (nq,3,11) int64, pairs (nq,)   by this float64 evaluation;
    lo, hi (nq,3,11), m_lo, m_hi (nq,)    the bounds described in the module's head;
    fragile (nq,) int64                   fragile pairs of each query;  n_valid, n_fragile: totals."""
    P = np.asarray(points, f32).reshape(-1, 3)
    N = np.asarray(normals, f32).reshape(-1, 3)
    qids = np.asarray(qids, np.int64)
    offs = np.asarray(offs, np.int64)
    ids = np.asarray(ids, np.int64)
    nq = len(qids)
    row = np.repeat(np.arange(nq), np.diff(offs))
    mult = np.ones(len(ids), np.int64) if mult is None else np.asarray(mult, np.int64)

    def count(at, sel, size):  # how many entries (with their multiplicity) fall at each index: exact integers
        return np.rint(np.bincount(at, weights=mult[a:a + chunk][sel], minlength=size)).astype(np.int64)
    counts = np.zeros((nq, 3, BINS), np.int64)
    lo = np.zeros_like(counts)
    hi = np.zeros_like(counts)
    pairs, m_lo, m_hi, frag = (np.zeros(nq, np.int64) for _ in range(4))
    for a in range(0, len(ids), chunk):
        r = row[a:a + chunk]
        s, t = qids[r], ids[a:a + chunk]
        pb = pair_bins(P[s], N[s], P[t], N[t])
        c, sure, maybe, adm = pb["counted"], pb["sure"], pb["maybe"], pb["adm"]
        pairs += count(r[c], c, nq)
        m_lo += count(r[sure], sure, nq)
        m_hi += count(r[sure | maybe], sure | maybe, nq)
        frag += count(r[pb["fragile"]], pb["fragile"], nq)
        for f in range(3):
            counts[:, f, :] += count(r[c] * BINS + pb["bins"][c, f], c, nq * BINS).reshape(nq, BINS)
            single = sure & (adm[:, f, :].sum(axis=1) == 1)
            one = count(r[single] * BINS + np.argmax(adm[single, f, :], axis=1), single, nq * BINS).reshape(nq, BINS)
            lo[:, f, :] += one
            hi[:, f, :] += one
            rest = (sure | maybe) & ~single
            np.add.at(hi[:, f, :], r[rest], adm[rest, f, :] * mult[a:a + chunk][rest][:, None])
    return dict(counts=counts, pairs=pairs, lo=lo, hi=hi, m_lo=m_lo, m_hi=m_hi, fragile=frag,
                n_valid=int(m_lo.sum()), n_fragile=int(frag.sum()))


def spfh_values(counts, pairs):
    """S = 100 c / m, 0 where m == 0 -> (n, 33) float64"""
    c = np.asarray(counts, f64).reshape(len(pairs), LEN)
    m = np.asarray(pairs, f64)
    return np.where(m[:, None] > 0, 100.0 * c / np.where(m > 0, m, 1.0)[:, None], 0.0)


def fpfh_values(points, qids, offs, ids, S_rows, row_of=None, mult=None):
    """F (nq,33) float64 of the rows `qids` from the SPFH S_rows (one row per entry of row_of's range): the SPFH of
    point i is S_rows[row_of[i]] (row_of None: S_rows has one row per query and qids == arange(n)).  known (nq,) bool:
    every neighbour with DistSq > 0 has its SPFH (row_of >= 0)."""
    P = np.asarray(points, f32).reshape(-1, 3)
    qids = np.asarray(qids, np.int64)
    offs = np.asarray(offs, np.int64)
    ids = np.asarray(ids, np.int64)
    nq = len(qids)
    if row_of is None:
        assert np.array_equal(qids, np.arange(len(P)))
        row_of = np.arange(len(P))
    row = np.repeat(np.arange(nq), np.diff(offs))
    e = P[ids] - P[qids[row]]
    dsq32 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    keep = dsq32 > 0
    row, nb, w = row[keep], row_of[ids[keep]], 1.0 / dsq32[keep].astype(f64)
    if mult is not None:
        w = w * np.asarray(mult, f64)[keep]
    known = np.bincount(row[nb < 0], minlength=nq) == 0
    w = np.where(nb >= 0, w, 0.0)
    W = np.stack([np.bincount(row, weights=w * S_rows[nb, k], minlength=nq) for k in range(LEN)], axis=1)
    W = W.reshape(nq, 3, BINS)
    T = W.sum(axis=2, keepdims=True)
    F = S_rows[row_of[qids]].reshape(nq, 3, BINS) + np.where(T > 0, 100.0 * W / np.where(T > 0, T, 1.0), 0.0)
    return F.reshape(nq, LEN), known


def fpfh(points, normals, qids, offs, ids, row_of=None, mult=None):
    """spfh() of the rows and their FPFH -> spfh()'s dict plus fpfh (nq,33) float64 and float_ok (nq,) bool: no fragile
    pair of the query's own nor of any of its neighbours, and every neighbour's SPFH known."""
    res = spfh(points, normals, qids, offs, ids, mult)
    qids = np.asarray(qids, np.int64)
    n = len(np.asarray(points).reshape(-1, 3))
    if row_of is None:
        assert np.array_equal(qids, np.arange(n))
        row_of = np.arange(n)
    S = spfh_values(res["counts"], res["pairs"])
    F, known = fpfh_values(points, qids, offs, ids, S, row_of, mult)
    nq = len(qids)
    row = np.repeat(np.arange(nq), np.diff(np.asarray(offs, np.int64)))
    nb = row_of[np.asarray(ids, np.int64)]
    nb_fragile = np.bincount(row, weights=(res["fragile"][np.maximum(nb, 0)] > 0) & (nb >= 0), minlength=nq) > 0
    res["fpfh"] = F
    res["float_ok"] = known & (res["fragile"] == 0) & ~nb_fragile
    return res


def check(res, got_fpfh, got_counts, got_pairs, what=""):
    """The count check, the float check and the condition (module's head) of the library's rows against res = fpfh()
    of the same rows.  Prints the figures before it asserts."""
    c = np.asarray(got_counts, np.int64).reshape(-1, 3, BINS)
    m = np.asarray(got_pairs, np.int64)
    F = np.asarray(got_fpfh, f32).reshape(-1, LEN)
    nq = len(res["pairs"])
    assert len(c) == len(m) == len(F) == nq, what
    ok = res["float_ok"]
    want = res["fpfh"][ok]
    err = np.abs(F[ok].astype(f64) - want)
    rel = np.max(np.where(want > 0, err / np.where(want > 0, want, 1.0), 0.0), initial=0.0)
    print("%s: %d rows, %d valid pairs, %d fragile, %d rows out of the float check, worst relative error %.3g (bound %.3g)"
          % (what, nq, res["n_valid"], res["n_fragile"], int((~ok).sum()), rel, FLOAT_TOL))
    assert res["n_valid"] > 0, what
    assert res["n_fragile"] <= MAX_FRAGILE_SHARE * res["n_valid"], (what, res["n_fragile"], res["n_valid"])
    assert (~ok).sum() <= MAX_LEFT_OUT * nq, (what, int((~ok).sum()), nq)
    assert np.all(c >= res["lo"]) and np.all(c <= res["hi"]), (what, np.argwhere((c < res["lo"]) | (c > res["hi"]))[:5])
    assert np.all(c.sum(axis=2) == m[:, None]), what
    assert np.all(m >= res["m_lo"]) and np.all(m <= res["m_hi"]), what
    assert np.all(err <= FLOAT_TOL * want), (what, rel)
    assert np.all(F[ok][want == 0] == 0), what
    assert np.all(np.isfinite(F)) and np.all(F >= 0), what
