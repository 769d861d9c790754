"""Plain numpy statement of cafe_gain_posterior (a helper, not a test), on the matrices of tests/gain_ref.py.

down_pass() is the sum-product both ways: the up pass leaves factor_v[s] = sum_c P_v[s][c] L_v[c] of every branch, the down
pass outside_u[c] = sum_s w[s] P_u[s][c] with w[s] = outside_parent[s] * prod_{siblings} factor[s], outside_root = the root
mass (root_absent at size 0, (1 - root_absent) (double)(float)prior[j-1] at size j).  posterior_u = outside_u L_u / Z,
p_gain = w[0] sum_{c>=1} P[0][c] L_u[c] / Z, p_loss = L_u[0] sum_{s>=1} w[s] P[s][0] / Z.  A missing leaf has factor exactly
1.0 (the untruncated row sum), so its p_gain is w[0] (1 - P[0][0]) / Z and its posterior over 0..M does not sum to 1.

enumerate_all() owes nothing to the down pass: it walks every assignment of sizes to the interior nodes, weighs it with the
root mass, the matrix entries of the interior branches and the leaf terms, and adds the weight to whatever event it belongs to.

down_pass takes a `wrong` switch that gets the down pass wrong on purpose (tests/test_gain_posterior_model.py shows that the
tables of the GPU test tell each from the right one)."""
import itertools

import numpy as np

import gain_ref as G
import marginal_ref as MR

WRONG = ("siblings_forgotten", "own_factor_included", "no_transpose", "row0_unit_in_down", "root_mass_forgotten")
KEYS = ("p_absent", "mean", "p_gain", "p_loss", "posterior")


def root_mass(prior, root_absent, Rr):
    return np.concatenate([[root_absent], (1.0 - root_absent) * np.asarray(prior, dtype=np.float32).astype(np.float64)[:Rr]])


def _rows(pb, root, v):
    return (pb.max_root_family_size if pb.parent[v] == root else pb.max_family_size) + 1


def down_pass(pb, counts, mats, prior, root_absent, error_model=None, wrong=None):
    """{lnl, p_absent [n_nodes], mean, p_gain, p_loss, posterior [n_nodes][matrix_size]} of one family"""
    M, Rr, N, nn = pb.max_family_size, pb.max_root_family_size, pb.matrix_size, pb.n_nodes
    ch, root = MR.children_of(pb), MR.root_of(pb)
    order, stack = [], [root]
    while stack:
        v = stack.pop()
        order.append(v)
        stack.extend(ch[v])
    L, factor, missing = {}, {}, set()
    for v in reversed(order):
        if pb.leaf_taxon[v] >= 0:
            L[v] = G.leaf_vector(pb, error_model, counts, v)
            if int(counts[pb.leaf_taxon[v]]) < 0:
                missing.add(v)
        else:
            sizes = (Rr if v == root else M) + 1
            L[v] = np.prod([factor[u][:sizes] for u in ch[v]], axis=0)
        if v != root:
            rows = _rows(pb, root, v)
            factor[v] = np.ones(rows) if v in missing else mats[v][:rows, :M + 1] @ L[v]
    mass = root_mass(prior, root_absent, Rr)
    Z = float(np.sum(mass * L[root]))
    out = {"lnl": np.log(Z), "p_absent": np.zeros(nn), "mean": np.zeros(nn), "p_gain": np.full(nn, np.nan), "p_loss": np.full(nn, np.nan),
           "posterior": np.zeros((nn, N))}
    outside = {root: np.ones(Rr + 1) if wrong == "root_mass_forgotten" else mass}
    for u in order:
        if u != root:
            p, rows = int(pb.parent[u]), _rows(pb, root, u)
            w = outside[p][:rows].copy()
            for v in ch[p]:
                if wrong != "siblings_forgotten" and (v != u or wrong == "own_factor_included"):
                    w = w * factor[v][:rows]
            Pm = mats[u].copy()
            if wrong == "row0_unit_in_down":
                Pm[0] = 0.0
                Pm[0, 0] = 1.0
            if wrong == "no_transpose":
                outside[u] = Pm[:M + 1, :rows] @ w
            else:
                outside[u] = w @ Pm[:rows, :M + 1]
            gain_mass = 1.0 - Pm[0, 0] if u in missing else float(Pm[0, 1:M + 1] @ L[u][1:])
            out["p_gain"][u] = w[0] * gain_mass / Z
            out["p_loss"][u] = L[u][0] * float(w[1:] @ Pm[1:rows, 0]) / Z
        post = outside[u] * L[u] / Z
        out["posterior"][u, :len(post)] = post
        out["p_absent"][u] = post[0]
        out["mean"][u] = float(np.arange(len(post)) @ post)
    return out


def enumerate_all(pb, counts, mats, prior, root_absent, error_model=None):
    """The same outputs from the sum over every assignment of sizes to the interior nodes"""
    M, Rr, N, nn = pb.max_family_size, pb.max_root_family_size, pb.matrix_size, pb.n_nodes
    ch, root = MR.children_of(pb), MR.root_of(pb)
    interior = [v for v in range(nn) if ch[v]]
    leaves = [v for v in range(nn) if not ch[v]]
    mass = root_mass(prior, root_absent, Rr)
    seen = {v: G.leaf_vector(pb, error_model, counts, v) for v in leaves}
    missing = {v for v in leaves if int(counts[pb.leaf_taxon[v]]) < 0}
    post, gain, loss, Z = np.zeros((nn, N)), np.zeros(nn), np.zeros(nn), 0.0
    for sizes in itertools.product(*[range((Rr if v == root else M) + 1) for v in interior]):
        size = dict(zip(interior, sizes))
        wt = mass[size[root]]
        for v in interior:
            if v != root:
                wt *= mats[v][size[int(pb.parent[v])], size[v]]
        term = {v: mats[v][size[int(pb.parent[v])], :M + 1] * seen[v] for v in leaves}
        total = {v: 1.0 if v in missing else term[v].sum() for v in leaves}
        full = wt * np.prod([total[v] for v in leaves])
        Z += full
        for v in interior:
            post[v, size[v]] += full
            if v != root:
                sp = size[int(pb.parent[v])]
                gain[v] += full if sp == 0 and size[v] >= 1 else 0.0
                loss[v] += full if sp >= 1 and size[v] == 0 else 0.0
        for v in leaves:
            others = wt * np.prod([total[k] for k in leaves if k != v])
            sp = size[int(pb.parent[v])]
            post[v, :M + 1] += others * term[v]
            if sp == 0:
                gain[v] += others * ((1.0 - mats[v][0, 0]) if v in missing else term[v][1:].sum())
            else:
                loss[v] += others * term[v][0]
    gain[root] = loss[root] = np.nan
    post /= Z
    return {"lnl": np.log(Z), "p_absent": post[:, 0].copy(), "mean": post @ np.arange(N), "p_gain": gain / Z, "p_loss": loss / Z, "posterior": post}


def table(pb, families, lambdas, mus, nus, prior, root_absent, error_model=None, wrong=None, cache=None):
    """down_pass of every listed family (an index, or -1 for the all-zero profile) under row i of lambdas / mus / nus, stacked.
    cache: a dict that keeps pb's matrices from one call to the next."""
    families = np.asarray(families)
    lam, mu, nu = (np.asarray(x, dtype=np.float64).reshape(len(families), -1) for x in (lambdas, mus, nus))
    cache, rows = {} if cache is None else cache, []
    for i, f in enumerate(families):
        key = (tuple(lam[i]), tuple(mu[i]), tuple(nu[i]))
        if key not in cache:
            cache[key] = G.matrices(pb, lam[i], mu[i], nu[i])
        counts = np.zeros(pb.n_taxa, dtype=np.int64) if f < 0 else pb.counts[f]
        rows.append(down_pass(pb, counts, cache[key], prior, root_absent, error_model, wrong))
    return {k: np.array([r[k] for r in rows]) for k in ("lnl",) + KEYS}


# What tests/test_gain_posterior_gpu.py runs on the three-taxon tree: patchy profiles (a family absent in part of the tree is what
# the posterior is asked about; families with ordinary counts have gain posteriors of 1e-14 and below) and one family with counts
# near n / 4, so that the high lanes carry weight.
def patchy_families(n, M):
    q = n // 4
    rows = [(0, 1, 1), (2, 0, 0), (0, 0, 2), (1, 3, 0), (0, 2, 0), (q, q - q // 12, q + q // 16)]
    return [{s: min(c, M) for s, c in zip("ABC", r)} for r in rows]
