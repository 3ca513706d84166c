"""Which targets of a Fit fail their partner's certificate, and what a second-level test would do with them (CPU only:
scipy's cKDTree and the oracle's Fit; DESIGN 3.1, "Level 2").

    python tools/cert2_probe.py [--cloud c4|edges] [--n N]

Per Evaluate, against last Evaluate's partner p of every target q (certificates in float64: cert = 0.24 rho1(p)^2,
cert2 = 0.24 rho2(p)^2, rho1 / rho2 the distances from p to its nearest / second-nearest other point, n1 the nearest):
fail1 = targets with |q - p|^2 >= cert; of them keep2 = below cert2 and nearer to p than to n1, flip = below cert2 and
nearer to n1, tie; search = the rest -- and the tiles of 2048 targets that hold a flip / a search.  The last column counts
the level-1 failures whose partner has rho1 at or above 12 / 20 / 30 mm: what a threshold on the records would lose.
--cloud edges: the cloud of tests/test_gpu_icp_cert2.py (close pairs, triples, twins, a lattice patch)."""
import argparse
import os
import sys

import numpy as np
from scipy.spatial import cKDTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle as O  # noqa: E402
from pcgol_amd import synth  # noqa: E402


def probe(c, out=print):
    base, target = c["base"], c["target"]
    b64 = base.astype(np.float64)
    kt = cKDTree(b64)
    d, idx = kt.query(b64, k=3)
    rho1, rho2, n1 = d[:, 1], d[:, 2], idx[:, 1]
    cert1, cert2 = 0.24 * rho1 ** 2, 0.24 * rho2 ** 2
    tree = O.KDTree(base)
    trans, it, tt, p_old = O.translate(0, 0, 0), 0, target.copy(), None
    rows = []
    for k in range(c["max_iteration"]):
        q = tt.astype(np.float64)
        if p_old is not None:
            dm = np.sum((q - b64[p_old]) ** 2, axis=1)
            keep1 = dm < cert1[p_old]
            dn1 = np.sum((q - b64[n1[p_old]]) ** 2, axis=1)
            in2 = ~keep1 & (dm < cert2[p_old])
            keep2, flip, tie = in2 & (dm < dn1), in2 & (dn1 < dm), in2 & (dn1 == dm)
            search = ~keep1 & ~keep2 & ~flip
            tiles = lambda m: len(np.unique(np.nonzero(m)[0] // 2048))
            thr = [int((~keep1 & (rho1[p_old] >= mm * 1e-3)).sum()) for mm in (12, 20, 30)]
            rows.append(dict(evaluate=k, fail1=int((~keep1).sum()), fail1_tiles=tiles(~keep1), keep2=int(keep2.sum()),
                             flip=int(flip.sum()), flip_tiles=tiles(flip), tie=int(tie.sum()), search=int(search.sum()),
                             search_tiles=tiles(search), above=thr))
            out("eval %2d: fail1 %7d (tiles %3d) keep2 %7d flip %6d (tiles %3d) tie %d search %6d (tiles %3d) | fail1 with rho1 >= 12/20/30 mm: %s" % (
                k, rows[-1]["fail1"], rows[-1]["fail1_tiles"], rows[-1]["keep2"], rows[-1]["flip"], rows[-1]["flip_tiles"],
                rows[-1]["tie"], rows[-1]["search"], rows[-1]["search_tiles"], thr))
        _, p_old = kt.query(q, k=1)
        ev = O.icp_evaluate(tree, tt, c["max_dist"], c["min_pairs"])
        trans, _conv, it = O.icp_update(trans, ev["gradient"], it, c["weight"], c["threshold"], c["max_iteration"])
        tt = synth.transform_points(trans, target)
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cloud", default="c4", choices=("c4", "edges"))
    ap.add_argument("--n", type=int, default=1_000_000)
    a = ap.parse_args()
    if a.cloud == "edges":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import test_gpu_icp_cert2 as T
        case = T.case()
    else:
        case = synth.c4_icp(n=a.n, width=10.0 * (a.n / 1e6) ** (1 / 3))
    rows = probe(case)
    late = [r for r in rows if r["evaluate"] >= 2]   # (the certified steps: from a Fit's third Evaluate on)
    print("Evaluates 2..: keeps %d flips %d searches %d" % (sum(r["keep2"] for r in late), sum(r["flip"] for r in late),
                                                         sum(r["search"] for r in late)))
