"""Per K2 op of one scorer call at the bench shape, from the K ranges the call published (Context.k_ranges): output tiles,
all-zero tiles (no 16-row block of the tile has a range), K tiles per tile and the live share of (block, k-step) inside the
K tiles that run; and how many panel rows the narrowed hulls keep of the structural ones.  Tiles of `mi` 16-row blocks
(default 5) and `kb`-deep K tiles (default 12), as the bench runs them.  Usage: dead_tiles.py [mi [kb [families]]]
(CAFE_NO_NARROW=1 / CAFE_NO_MAGSKIP=1 in the environment give the rows to compare with)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from cafexp_amd import capi, problem as P, synth
from cafexp_amd.gamma_rates import discrete_gamma
mi = int(sys.argv[1]) if len(sys.argv) > 1 else 5
kb = int(sys.argv[2]) if len(sys.argv) > 2 else 12
pb, _ = synth.make_problem(n_families=int(sys.argv[3]) if len(sys.argv) > 3 else 50000)
K = 8
probs, mult = discrete_gamma(K, 2.0)
pr = P.Params(lambdas=np.array([0.002]), prior=P.prior_uniform(750), multipliers=mult, cat_probs=probs)
ctx = capi.Context(pb, max_categories=K)
ctx.score(pr, alpha=2.0)
nodes = [v for v in range(len(pb.parent)) if pb.leaf_taxon[v] < 0 and pb.parent[v] >= 0]
tot = np.zeros(5)
print("node  col tiles  output tiles  all-zero  K tiles/tile  live share  hull rows kept")
for v in nodes:
    row = np.zeros(5)     # tiles, dead, K tiles, live (block, k-step), (block, k-step) of the K tiles that run
    kept = np.zeros(2)
    for k in range(K):
        r = ctx.k_ranges(v, k).astype(np.int64)                  # [tiles][blocks][2]
        nb = r.shape[1]
        pad = (-nb) % mi
        lo = np.pad(r[..., 0], ((0, 0), (0, pad)), constant_values=1).reshape(r.shape[0], -1, mi)
        hi = np.pad(r[..., 1], ((0, 0), (0, pad)), constant_values=0).reshape(r.shape[0], -1, mi)
        some = hi >= lo
        live = np.where(some, hi - lo + 1, 0).sum(axis=2)
        tlo = np.where(some, lo, 1 << 30).min(axis=2) * 4 // kb
        thi = np.where(some, hi, -1).max(axis=2) * 4 // kb
        dead = ~some.any(axis=2)
        kt = np.where(dead, 1, thi - tlo + 1)
        row += [dead.size, dead.sum(), kt.sum(), live.sum(), (np.where(dead, 0, kt) * (kb // 4) * mi).sum()]
        s, n = ctx.extents(v, k)[1].astype(np.int64), ctx.narrowed_extents(v, k).astype(np.int64)
        kept += [np.where(n[:, 1] >= n[:, 0], n[:, 1] - n[:, 0] + 1, 0).sum(), np.where(s[:, 1] >= s[:, 0], s[:, 1] - s[:, 0] + 1, 0).sum()]
    print("%4d %8d %12d %10.3f %12.2f %10.3f %10.3f" % (v, r.shape[0], row[0], row[1] / row[0], row[2] / row[0], row[3] / max(1, row[4]), kept[0] / max(1, kept[1])))
    tot += row
print("all ops: %d output tiles, all-zero %.3f, K tiles per tile %.2f, live (block, k-step) per tile %.1f, live share inside run K tiles %.3f"
      % (tot[0], tot[1] / tot[0], tot[2] / tot[0], tot[3] / tot[0], tot[3] / max(1, tot[4])))
print("issued flops %.6e" % ctx.issued_flops())
