"""cafe_pvalues (csrc/pvalues.hip) replayed stage by stage; its sort and bound kernels exact.

tests/pvalues_ref.py restates the call in numpy: simulate_kernel draw for draw (family s * n_sim + i has root size s, the order-N
matrix pool cut at M columns, no draw below an extinct parent), the sort, the upper-bound rule.  cafe_debug_pvalues_stages is
one cafe_pvalues call that also returns what its stages left on the device, and every EXACT comparison below is made on values
the device itself returned -- a simulated root maximum that equals an observed one up to the last bits flips a p-value by k / n
between two correct implementations, so no exact check may cross from one implementation's doubles to the other's:
  1. sizes and counts            == the replay over capi's matrices, family by family (families with an AMBIGUOUS draw left out,
                                    at most LEFT_OUT of them: test_simulate_replay's rule), counts == sizes at the leaves;
  2. root maxima before the sort  within 1e-11 (test_root_max_matches_oracle's bound) of oracle.root_max of the distinct replayed
                                    profiles, zeros matched exactly;
  3. after the sort               == np.sort of (2)'s device values, by bits;
  4. the p-values                 == the numpy rule applied to the device's observed maxima and sorted rows, by bits, ties included;
  5. ... and                      == a plain ctx.pvalues() call with the same arguments;
  6. the observed maxima          == ctx.root_max();
  7. independent of every device intermediate: each p-value lies in [p_lo, p_hi] of replay + oracle (pvalues_ref.pvalue_interval).
Under death rates the oracle has no model: the reference root maxima there are pvalues_ref.prune_root_max, a plain numpy prune,
over the matrices of capi.build_matrices_lm (themselves pinned to numpy by tests/test_bd_lm_gpu.py), at the same bounds.

The CPU tests run the same replay over the oracle's matrices (tests/bd_lm_ref.py's under death rates) and assert what the GPU
comparison needs of every case and seed: ambiguous families <= LEFT_OUT (0 in every case), at least half of the observed
families with p_lo == p_hi, at least three observed p-values strictly inside (1/n, (n-2)/n) -- a table of saturated p-values
tests nothing -- and the numpy rule == oracle.tree_pvalues.  The third condition cannot hold where no k/n lies strictly inside
that interval (n_sim < 5: the cases that reach the sort's and the family tiles' smallest sizes), and not on the two trees with an
all-zero-row branch, where every profile but the extinct one has likelihood exactly 0: those cases say interior=0 and why.

No small case makes the child context take more than one column chunk: its chunk is cut from 80 % of the free device memory
(create_child_for_device_counts passes no workspace limit) or from the 4 GB reach of a panel descriptor, hundreds of thousands
of families at any order; the family-count cases therefore stop at the 128-family tile and the 256-thread block.

On the MI355X (this file's GPU tests, as printed; every line in profiles/pvalues_replay_gpu.txt): no family left out in any of
the 25 cases; root maxima before the sort within 6.5e-13 of the reference (families257; 2.4e-13 to 3.2e-13 at order129, families127 and order300, less elsewhere),
the 1483 and 1464 zeros of the two all-zero-row trees matched exactly; every p-value inside its interval, which is a point
but for the families whose simulated twin ties them (sort256 .. sort2048, the table's copied row: [0.1, 0.12], device 0.12, its
observed maximum bit-equal to its twin's) and the likelihood-0 rows of the all-zero-row trees ([0, 0.99]).  cafe_pvalues
returned the parent commit's bits at test_pvalues.py's arguments (1500 values).  Four mutants of a scratch copy -- '>' for
'>=' in draw_child_size, n_sim - 1 as the divisor of the root size, no n -> n - 1 rule, the sort without its last pass -- each
failed here: the all-zero-row trees, the sort cases at check 1, test_tree_pvalue_kernel and check 4, test_sort_rows_kernel
and check 3."""
import dataclasses

import numpy as np
import pytest

import bd_lm_ref as BR
import pvalues_ref as PR
from helpers import _explicit_problem
from test_per_family_shapes import sizes
from test_simulate_replay import LEFT_OUT, SHAPES, SHAPE_LAMBDAS

TREE3 = "((A:7.25,B:23.904):61.337,C:9.75);"
EQUAL_BRANCHES = "((A:10,B:10):20,C:10);"                    # A and B: equal length and lambda index -> one matrix slot
ROOT_MAX_TOL = 1e-11                                         # test_pvalues.test_root_max_matches_oracle


# ---------------------------------------------------------------------------------------------------- the cases
def _rows(profiles, M=1 << 30):
    """One {species: count} per profile over (A, B, C[, D, E]), counts cut to M"""
    return [dict(zip("ABCDE", (min(c, M) for c in r))) for r in profiles]


# Eight observed families per case.  Most profiles sit at p = 0 or (n - 1) / n; these were picked, on the CPU over the oracle's
# matrices, from the profiles whose p-value lies inside the simulated distributions (what the CPU test asserts of them).
SORT_ROWS = [(2, 9, 4), (12, 3, 15), (5, 6, 11), (3, 5, 2), (1, 1, 1), (4, 2, 7), (6, 6, 6), (0, 3, 1)]
ROWS = {
    "families128": [(0, 1, 0), (9, 6, 4), (5, 8, 3), (6, 4, 3), (2, 0, 2), (3, 3, 4), (1, 1, 1), (2, 9, 4)],
    "families129": [(0, 0, 5), (4, 7, 2), (6, 7, 2), (5, 2, 3), (3, 4, 1), (3, 3, 2), (1, 1, 1), (2, 9, 4)],
    "families255": [(0, 2, 5), (4, 0, 4), (11, 9, 3), (10, 8, 6), (9, 7, 4), (3, 3, 2), (1, 1, 1), (2, 9, 4)],
    "families256": [(11, 12, 4), (7, 7, 6), (4, 7, 5), (3, 1, 5), (5, 7, 4), (1, 2, 2), (1, 1, 1), (2, 9, 4)],
    "order32": [(14, 14, 8), (8, 10, 13), (3, 6, 3), (6, 4, 3), (9, 12, 12), (3, 1, 2), (1, 1, 1), (3, 5, 2)],
    "order33": [(14, 14, 8), (9, 13, 11), (2, 5, 3), (8, 5, 9), (13, 11, 9), (4, 3, 7), (1, 1, 1), (3, 5, 2)],
    "order129": [(14, 9, 2), (8, 6, 0), (1, 6, 7), (7, 1, 4), (6, 5, 0), (11, 5, 13), (1, 1, 1), (40, 44, 39)],
    "order300": [(14, 7, 3), (11, 3, 8), (2, 0, 13), (1, 1, 13), (6, 14, 9), (1, 6, 5), (1, 1, 1), (40, 44, 39)],
    "two_lambdas": [(14, 9, 13), (10, 7, 4), (9, 8, 3), (14, 14, 8), (12, 10, 9), (8, 7, 9), (1, 1, 1), (2, 9, 4)],
    "two_lambdas_death_rates": [(14, 13, 5), (4, 9, 6), (3, 3, 9), (12, 10, 6), (11, 14, 14), (11, 11, 14), (1, 1, 1), (2, 9, 4)],
    "polytomy": [(2, 1, 5, 1, 4), (1, 7, 6, 5, 4), (6, 1, 1, 1, 0), (7, 2, 5, 7, 5), (3, 3, 1, 6, 4), (5, 6, 5, 8, 3), (1, 1, 1, 1, 1), (2, 9, 4, 3, 1)],
    # A's branch has all-zero rows: only A = B = 0 (their parent extinct) has a likelihood above 0; the last two rows have 0.0
    "leaf_under_root_tq0": [(0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 0, 3), (0, 0, 5), (0, 0, 8), (0, 2, 1), (3, 5, 2)],
    "saturated": [(0, 0, 0, 0, 0), (0, 0, 1, 1, 1), (0, 0, 2, 1, 3), (0, 0, 3, 3, 3), (0, 0, 0, 4, 2), (0, 0, 5, 0, 0), (0, 2, 1, 1, 1), (3, 5, 2, 1, 6)],
    # a family listed three times (spread_unique), a profile so unlikely that its root maximum underflows to exactly 0.0, and
    # row 5, which the case replaces by a profile of the simulated set
    "table": [(12, 12, 7), (9, 12, 14), (8, 6, 12), (8, 5, 6), (12, 12, 7), (9, 7, 12), (299, 0, 0), (12, 12, 7)],
}


def _case(name, M, R, n_sim, lambdas, seed, newick=TREE3, lambda_index=None, mus=None, interior=3, copy=None):
    """copy: (row, simulated family): that observed row is replaced by the replayed profile of that simulated family.
    interior: how many observed p-values must lie strictly inside (1/n, (n-2)/n) on the CPU."""
    pb = _explicit_problem(newick, _rows(ROWS.get(name, SORT_ROWS), M), M, R)
    if lambda_index is not None:
        pb = dataclasses.replace(pb, lambda_index=np.asarray(lambda_index(pb), dtype=np.int32), n_lambdas=len(lambdas), single_lambda=False)
    assert pb.matrix_size == max(M, R) + 1 and len(np.atleast_1d(lambdas)) == pb.n_lambdas
    return dict(name=name, pb=pb, n_sim=n_sim, lambdas=np.asarray(lambdas, dtype=np.float64), mus=None if mus is None else np.asarray(mus, dtype=np.float64),
                seed=seed, interior=interior if n_sim >= 5 else 0, copy=copy)


def _alternate(pb):
    return np.arange(pb.n_nodes) % 2


def _a_and_b_share(pb):
    """A, B -> index 0 (equal length too: one slot); C and the interior branch -> index 1 (C: A's length, another lambda)."""
    return np.array([0 if pb.leaf_taxon[v] in (0, 1) else 1 for v in range(pb.n_nodes)])


def _cases():
    out = []
    # the sort kernel: its padding and its passes below, at and above 256 threads
    for n_sim in (1, 2, 3, 255, 256, 257, 1000, 2047, 2048):
        out.append(_case("sort%d" % n_sim, 12, 5, n_sim, [0.01], 7000 + n_sim))
    # R * n_sim either side of the 128-family tile and of simulate_kernel's 256-thread block (127 and 257 are prime: one draw per root size)
    for M, R, n_sim in ((130, 127, 1), (12, 4, 32), (12, 3, 43), (12, 5, 51), (12, 4, 64), (260, 257, 1)):
        out.append(_case("families%d" % (R * n_sim), M, R, n_sim, [0.01], 8000 + R * n_sim))
    # R > M (root sizes >= M draw from a row cut short of its mass) and M > R
    for n, n_sim in ((32, 64), (33, 64), (129, 24), (300, 12)):
        M, R = sizes(n)
        out.append(_case("order%d" % n, M, R, n_sim, [0.002 if n <= 33 else 0.01], 9000 + n))
    # two lambda indices through a lambda tree, two branches in one slot; the same under death rates
    out.append(_case("two_lambdas", 31, 16, 200, [0.004, 0.011], 10001, newick=EQUAL_BRANCHES, lambda_index=_a_and_b_share))
    out.append(_case("two_lambdas_death_rates", 31, 16, 200, [0.004, 0.011], 10002, newick=EQUAL_BRANCHES, lambda_index=_a_and_b_share, mus=[0.007, 0.006]))
    # test_simulate_replay's tree shapes.  A's branch of the second quantizes to t = 0 and A's branch of the third saturates
    # (0.026 * 40 > 1): all-zero rows, A is drawn 0 in every family, and every profile but the all-zero one has likelihood 0
    out.append(_case("polytomy", 31, 16, 200, SHAPE_LAMBDAS, 11001, newick=SHAPES["polytomy"], lambda_index=_alternate))
    out.append(_case("leaf_under_root_tq0", 31, 16, 100, SHAPE_LAMBDAS, 11002, newick=SHAPES["leaf_under_root_tq0"], lambda_index=_alternate, interior=0))
    out.append(_case("saturated", 31, 16, 100, [2.6 * v for v in SHAPE_LAMBDAS], 11003, newick=SHAPES["saturated_for_one_multiplier"],
                     lambda_index=_alternate, interior=0))
    # the observed table
    out.append(_case("table", 299, 20, 50, [0.002], 12001, copy=(5, 10 * 50 + 10)))       # root size 10, drawn (14, 12, 10)
    return out


CASES = _cases()
IDS = [c["name"] for c in CASES]
ZERO_LEAF = {"leaf_under_root_tq0": 0, "saturated": 0}        # the taxon whose branch has all-zero rows


def _numpy_lm_matrices(N, lams, mus, ts):
    return np.stack([BR.matrix(N, float(l), float(m), float(t)) for l, m, t in zip(lams, mus, ts)])


def _observed_problem(case, counts):
    """The case's problem with its observed table final: the copied row (if any) taken from the replayed counts [n_taxa][Fs]"""
    pb = case["pb"]
    if case["copy"] is None:
        return pb
    row, f = case["copy"]
    table = pb.counts.copy()
    table[row] = counts[:, f]
    return dataclasses.replace(pb, counts=table)


def _branch_matrices(pb, lambdas, mus, matrices):
    """mats[v] for prune_root_max: the order-N matrix of the branch above every non-root node"""
    br = [v for v in range(pb.n_nodes) if pb.parent[v] >= 0]
    idx = pb.lambda_index[br]
    got = matrices(pb.matrix_size, lambdas[idx], None if mus is None else mus[idx], pb.branch_length[br])
    mats = [None] * pb.n_nodes
    for v, m in zip(br, got):
        mats[v] = m
    return mats


def _reference(case, matrices, oracle):
    """Replay + reference root maxima of one case over `matrices`: everything the checks compare with, computed once.
    The root maxima are the oracle's; under death rates, where it has no model, a numpy prune over the same matrices."""
    sizes_, counts, ambiguous = PR.replay(case["pb"], case["lambdas"], case["n_sim"], case["seed"], matrices, mus=case["mus"])
    pb = _observed_problem(case, counts)
    sub, inverse = PR.distinct_profiles(pb, counts)
    if case["mus"] is None:
        rm = lambda q: oracle.root_max(q, case["lambdas"])
    else:
        mats = _branch_matrices(pb, case["lambdas"], case["mus"], matrices)
        rm = lambda q: PR.prune_root_max(q, mats)
    cond = rm(sub)[inverse].reshape(pb.max_root_family_size, case["n_sim"])
    return dict(pb=pb, sizes=sizes_, counts=counts, ambiguous=ambiguous, cond=cond, observed=rm(pb), n_profiles=sub.counts.shape[0])


def _line(a):
    return np.array2string(np.asarray(a), max_line_width=10000, precision=6)


def _interval(ref):
    """[p_lo, p_hi] of the observed families; a simulated family with an ambiguous draw counts against p_lo and for p_hi"""
    R, n = ref["cond"].shape
    amb = ref["ambiguous"].reshape(R, n)
    lo, _ = PR.pvalue_interval(ref["observed"], np.where(amb, np.inf, ref["cond"]))
    _, hi = PR.pvalue_interval(ref["observed"], np.where(amb, -np.inf, ref["cond"]))
    return lo, hi


# ---------------------------------------------------------------------------------------------------- CPU
def test_the_cases_reach_every_edge():
    by = {c["name"]: c for c in CASES}
    assert {c["n_sim"] for c in CASES if c["name"].startswith("sort")} == {1, 2, 3, 255, 256, 257, 1000, 2047, 2048}
    assert {c["pb"].max_root_family_size * c["n_sim"] for c in CASES if c["name"].startswith("families")} == {127, 128, 129, 255, 256, 257}
    orders = [by["order%d" % n]["pb"] for n in (32, 33, 129, 300)]
    assert [pb.matrix_size for pb in orders] == [32, 33, 129, 300]
    assert {pb.max_root_family_size > pb.max_family_size for pb in orders} == {True, False}
    for name in ("two_lambdas", "two_lambdas_death_rates"):
        pb = by[name]["pb"]
        a, b, c = (int(np.where(pb.leaf_taxon == t)[0][0]) for t in range(3))
        assert pb.n_lambdas == 2 and pb.lambda_index[a] == pb.lambda_index[b] != pb.lambda_index[c]
        assert pb.branch_length[a] == pb.branch_length[b] == pb.branch_length[c]
    assert by["two_lambdas_death_rates"]["mus"] is not None and by["two_lambdas"]["mus"] is None
    table = by["table"]["pb"].counts
    assert sum(np.array_equal(r, table[0]) for r in table) == 3 and by["table"]["copy"] is not None
    assert all(c["interior"] == 3 for c in CASES if c["n_sim"] >= 5 and c["name"] not in ZERO_LEAF)


def test_the_numpy_rule_on_crafted_rows(oracle):
    """pvalues_ref.pvalues against the oracle's restatement of the reference (probability.cpp:379-407), ties and ends included."""
    rng = np.random.default_rng(5)
    for R, n in ((1, 1), (1, 2), (3, 7), (7, 1000)):
        cond = np.sort(rng.choice(rng.random(max(2, n // 3)), size=(R, n)), axis=1)
        cond[0, : n // 2] = 0.0
        obs = np.concatenate([[0.0, -1.0, 2.0, cond[0, 0], cond[-1, -1], cond[0, n // 2]], cond[rng.integers(0, R, 20), rng.integers(0, n, 20)], rng.random(20)])
        got = PR.pvalues(obs, cond)
        assert np.array_equal(got, oracle.tree_pvalues(obs, cond))
        lo, hi = PR.pvalue_interval(obs, cond)
        assert np.all(lo <= got) and np.all(got <= hi) and got.max() == (n - 1) / n
    assert np.array_equal(PR.pvalues([0.05, 0.0001, 0.099, 5.0], np.cumsum(np.full((1, 10), 0.01), axis=1)), [0.5, 0.0, 0.9, 0.9])      # test.cpp:1175-1183


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_seeds_meet_the_conditions_of_the_gpu_comparison(oracle, case):
    ref = _reference(case, _numpy_lm_matrices if case["mus"] is not None else PR.oracle_matrices(oracle), oracle)
    pb, n, R = ref["pb"], case["n_sim"], case["pb"].max_root_family_size
    Fs = R * n
    assert ref["sizes"].shape == (pb.n_nodes, Fs) and ref["counts"].shape == (pb.n_taxa, Fs)
    root = int(np.where(pb.parent < 0)[0][0])
    assert np.array_equal(ref["sizes"][root], np.arange(Fs) // n) and ref["sizes"][:root].max() <= pb.max_family_size - 1
    assert not ref["sizes"][:, :n].any()                     # root size 0: extinct everywhere
    p = PR.pvalues(ref["observed"], ref["cond"])
    lo, hi = _interval(ref)
    point = int((lo == hi).sum())
    interior = int(((p > 1 / n) & (p < (n - 2) / n)).sum())
    print("%s: %d of %d families ambiguous, %d distinct profiles, %d of %d point intervals, %d interior p-values, p = %s"
          % (case["name"], ref["ambiguous"].sum(), Fs, ref["n_profiles"], point, len(p), interior, _line(p)))
    assert ref["ambiguous"].sum() <= LEFT_OUT * Fs
    assert np.all(lo <= p) and np.all(p <= hi)
    assert 2 * point >= len(p)
    assert interior >= case["interior"]
    assert np.array_equal(p, oracle.tree_pvalues(ref["observed"], np.sort(ref["cond"], axis=1)))
    if case["name"] in ZERO_LEAF:
        assert not ref["counts"][ZERO_LEAF[case["name"]]].any() and ref["counts"].any()
    if case["name"] == "table":
        row, f = case["copy"]
        assert ref["observed"][6] == 0.0 and ref["observed"][row] == ref["cond"].reshape(-1)[f] > 0
        assert p[0] == p[4] == p[7] and 1 / n < p[0] < (n - 2) / n
        assert 1 / n < lo[row] < hi[row] == p[row] < (n - 2) / n          # the tie with its simulated twin decides this p-value


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_stage_of_a_call(capi, oracle, case):
    ref = _reference(case, PR.device_matrices(capi), oracle)
    pb, n, name = ref["pb"], case["n_sim"], case["name"]
    R, Fs = pb.max_root_family_size, pb.max_root_family_size * case["n_sim"]
    ctx = capi.Context(pb)
    try:
        if case["mus"] is not None:
            ctx.set_death_rates(case["mus"])
        st = ctx.pvalues_stages(case["lambdas"], n_simulations=n, seed=case["seed"])
        plain = ctx.pvalues(case["lambdas"], n_simulations=n, seed=case["seed"])
        root_max = ctx.root_max(case["lambdas"])
    finally:
        ctx.close()
    keep = ~ref["ambiguous"]
    print("%s: %d families compared, %d left out" % (name, keep.sum(), Fs - keep.sum()))
    assert Fs - keep.sum() <= LEFT_OUT * Fs
    # 1. the simulation, draw for draw
    bad = np.where(keep & (st["sizes"] != ref["sizes"]).any(axis=0))[0]
    assert len(bad) == 0, "%s: %d families differ, first %d: device %s replay %s" % (name, len(bad), bad[0], st["sizes"][:, bad[0]], ref["sizes"][:, bad[0]])
    assert np.array_equal(st["counts"][:, keep], ref["counts"][:, keep])
    leaves = np.where(pb.leaf_taxon >= 0)[0]
    assert np.array_equal(st["counts"], st["sizes"][leaves[np.argsort(pb.leaf_taxon[leaves])]])
    if name in ZERO_LEAF:
        assert not st["counts"][ZERO_LEAF[name]].any() and st["counts"].any()
    # 2. the root maxima of the simulated families
    got, want = st["cond_unsorted"].reshape(-1)[keep], ref["cond"].reshape(-1)[keep]
    assert np.array_equal(got == 0, want == 0)
    nz = want != 0
    worst = np.abs(got[nz] / want[nz] - 1).max(initial=0.0)
    print("%s: root maxima of %d simulated families (%d exact zeros), worst relative error %.3g" % (name, keep.sum(), (~nz).sum(), worst))
    assert worst <= ROOT_MAX_TOL
    # 3. the sort
    assert np.array_equal(_bits(st["cond_sorted"]), _bits(np.sort(st["cond_unsorted"], axis=1)))
    # 4. the p-value rule on the device's own values: no tie is excused
    assert np.array_equal(_bits(st["pvalues"]), _bits(PR.pvalues(st["observed"], st["cond_sorted"])))
    if case["copy"] is not None:
        row, f = case["copy"]
        print("%s: the copied profile's observed maximum %s the bits of its simulated twin" % (name, "has" if st["observed"][row] == st["cond_unsorted"].reshape(-1)[f] else "has NOT"))
        assert st["observed"][6] == 0.0 and st["pvalues"][0] == st["pvalues"][4] == st["pvalues"][7]
    # 5., 6. the capture changes nothing
    assert np.array_equal(_bits(st["pvalues"]), _bits(plain))
    assert np.array_equal(_bits(st["observed"]), _bits(root_max))
    # 7. against replay + reference alone
    lo, hi = _interval(ref)
    print("%s: p %s in [%s, %s]" % (name, _line(st["pvalues"]), _line(lo), _line(hi)))
    assert np.all(lo <= st["pvalues"]) and np.all(st["pvalues"] <= hi)


SORT_N = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1025, 2047, 2048]


def _sort_rows(n, rng):
    few = rng.random(3)
    special = np.array([0.0, 5e-324, 2.5e-310, np.inf, 1.0, np.inf, 0.0, 1e-320])
    rows = [
        2.0 ** rng.uniform(-300, 300, n),                    # 600 binades
        np.full(n, 0.37),                                    # all equal
        np.sort(rng.random(n)), np.sort(rng.random(n))[::-1],
        rng.choice(few, n),                                  # many duplicates
        rng.permutation(np.resize(special, n)),              # zeros, denormals and +inf: the padding is +inf too
        np.where(rng.random(n) < 0.3, np.inf, rng.random(n)),
        2.0 ** rng.uniform(-300, 300, n),                    # (a last ordinary row behind the special ones: the row stride)
    ]
    return np.array(rows)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SORT_N)
def test_sort_rows_kernel(capi, n):
    v = _sort_rows(n, np.random.default_rng(n))
    got = capi.debug_sort_rows(v)
    assert np.array_equal(_bits(got), _bits(np.sort(v, axis=1)))
    assert np.isinf(got).sum() == np.isinf(v).sum()


def _bound_inputs(R, n, F, rng):
    pool = np.sort(rng.random(max(2, n // 4)))               # few distinct values: runs of equal entries
    cond = np.sort(rng.choice(pool, size=(R, n)), axis=1)
    cond[0, : (n + 1) // 2] = 0.0                            # zeros in the first row
    if R > 1:
        cond[1] = np.sort(2.0 ** rng.uniform(-300, 300, n))
    last = cond[R - 1]
    crafted = np.array([0.0, -1.0, pool[0] / 2, last[0], last[n // 2], last[-1], cond.max(), 2 * cond.max() + 1, np.inf, cond[0, n // 2], 5e-324])
    obs = np.concatenate([crafted, cond[rng.integers(0, R, F), rng.integers(0, n, F)] * rng.choice([1.0, 1 - 2.0 ** -53, 1 + 2.0 ** -52], F)])
    return rng.permutation(obs[:F]) if F >= len(crafted) else obs[:F], cond


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 1000, 2048])
@pytest.mark.parametrize("R", [1, 7])
def test_tree_pvalue_kernel(capi, R, n):
    for F in (1, 255, 256, 257):
        obs, cond = _bound_inputs(R, n, F, np.random.default_rng(1000 * R + n + F))
        got = capi.debug_tree_pvalue(obs, cond)
        want = PR.pvalues(obs, cond)
        assert np.array_equal(_bits(got), _bits(want)), (R, n, F)
        if F >= 255:
            assert want.max() == (n - 1) / n and (want.min() == 0.0 or n == 1)      # above every entry; below every entry
            if R == 1 and n >= 1000:
                assert len(np.unique(want)) > 20
