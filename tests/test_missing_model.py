"""Missing cells, without a GPU: the tables of tests/missing_ref.py can tell the rule from its likely mistakes, they place the
missing cells where the GPU tests say they do, and the Python loaders read and size such a table.

The rule: a missing leaf's factor is exactly 1.0 (include/cafe_mi355x.h).  The mistakes (missing_ref.up's variants), each on the
numpy prune alone with numpy matrices (tests/bd_lm_ref.py):
    zero     at the tests' own rates;
    rowsum   at a rate where the truncation at M matters.  With lambda = mu the matrices saturate before it does (alpha < 1/2
             keeps a lineage's tail ratio below 1/2, and 2^-40 is already below the bound), so this variant is scored with
             death rates: a birth rate far above the death rate, tail ratio beta close to 1;
    taps     under the 3-tap error model at the same rates.  "The taps applied to a missing cell" has no single meaning -- the
             taps of row x need an x -- so the variant is the one a reader could compute: the error model summed over every
             count the cell might hold.  (The taps of the clamped index 0 weigh a factor of 1 by err[0][.] summed over the taps
             that stay inside [0, M]: exactly 1, since row 0 of an error model has no mass below 0.  That reader is right by
             accident and no table can tell it from the rule.)
"""
import numpy as np
import pytest

import bd_lm_ref as R
import missing_ref as MS
from cafexp_amd import problem as P

# (birth, death) per order.  beta = 1 - exp(-lambda t) nearly: beta^M is 1e-4 / 4e-3 on the shortest leaf branch (t = 2).  The death
# rate is tiny because the library marks a branch zero unless alpha + beta < 1, that is exp((lambda - mu) t) < lambda / mu, which
# the longest branch (t = 9) must still satisfy; it is not 0, so that a family whose counts fall along a branch stays possible.
TRUNCATION_RATES = {41: (0.8, 1e-4), 300: (2.0, 1e-9)}


def _lnl(pb, pr, mus, variant):
    lam = pr.lambdas
    mats = R.reference_matrices(pb, lam, lam if mus is None else mus, [1.0])
    return MS.family_lnl(pb, pr, mats, variant)


@pytest.mark.parametrize("order", [41, 300])
def test_the_missing_cells_sit_where_the_gpu_tests_say(order):
    counts = MS.table(order)
    col = {s: j for j, s in enumerate(MS.SPECIES)}
    cols = MS.root_columns(counts)
    n = MS.N_DISTINCT + 1
    assert np.array_equal(cols[:n], np.arange(n))            # family f is column f: 0 the all-missing family, then the 300
    assert (counts[0] == MS.MISSING).all() and counts[1:n, col["D"]].min() >= 0
    assert len(set(cols)) >= 257 + 2                         # at least 257 distinct columns, and the two twins have their own
    h, g = counts[:, col["H"]] < 0, counts[:, col["G"]] < 0
    for leaf in (h, g):                                      # first and last column of a 128-column tile
        assert leaf[0] and leaf[127] and leaf[128] and leaf[255] and leaf[256]
        assert leaf[10] and not leaf[11] and not leaf[12] and leaf[13] and leaf[20] and leaf[21]     # even, odd, both of a pair
    a, b = counts[:, col["A"]] < 0, counts[:, col["B"]] < 0
    assert (a & ~b)[1:n].any() and (b & ~a)[1:n].any() and (a & b)[1:n].any()      # one leaf of the cherry, the other, both
    c, e = counts[:, col["C"]] < 0, counts[:, col["E"]] < 0
    assert (c & ~e)[1:n].any() and (c & e)[1:n].any()        # the polytomy: one leaf, two leaves
    assert (g & ~h & ~a & ~b)[1:n].any()                     # the leaf whose sibling is interior, alone
    # the twins differ from their source by the missing pattern only, and own a column; the duplicates share one
    for i, src in enumerate(MS.SOURCE_OF_PATTERN_TWINS):
        twin = counts[n + i]
        seen = twin >= 0
        assert np.array_equal(twin[seen], counts[src][seen]) and (counts[src][~seen] >= 0).all() and cols[n + i] == n + i
    for i, src in enumerate(MS.SOURCE_OF_DUPLICATES):
        assert np.array_equal(counts[n + 2 + i], counts[src]) and cols[n + 2 + i] == cols[src]
    full = MS.table(order, blank=False)
    assert full.shape == counts.shape and full.min() >= 0 and np.array_equal(full[counts >= 0], counts[counts >= 0])


@pytest.mark.parametrize("order", [41, 300])
def test_the_inputs_tell_the_rule_from_its_likely_mistakes(order):
    missing = (MS.table(order) < 0).any(axis=1)
    assert missing.sum() >= 60
    # zero: the tests' own rates
    pb = MS.problem(order, "two_lambdas")
    pr = MS.params(pb, "two_lambdas")
    right, wrong = _lnl(pb, pr, None, None), _lnl(pb, pr, None, "zero")
    assert np.isfinite(right).all()
    moved = np.abs(wrong - right) / np.abs(right)             # (-inf where a zero is impossible: moved = inf)
    print("order %d, missing scored as 0: smallest relative move %.3g" % (order, moved[missing].min()))
    assert np.all(moved[missing] > 1e-6) and np.all(moved[~missing] == 0.0)
    # rowsum and taps: a rate where the truncation matters
    lam, mu = TRUNCATION_RATES[order]
    for variant, model in (("rowsum", "base"), ("taps", "error3")):
        pb = MS.problem(order, model)
        pr = MS.params(pb, model)
        pr.lambdas = np.array([lam])
        right, wrong = _lnl(pb, pr, np.array([mu]), None), _lnl(pb, pr, np.array([mu]), variant)
        fin = np.isfinite(right)
        assert fin[missing].sum() >= 60 and fin[0]            # (the family with every cell missing among them)
        moved = np.abs(wrong[fin] - right[fin]) / np.abs(right[fin])
        print("order %d, %s: smallest relative move %.3g" % (order, variant, moved[missing[fin]].min()))
        assert np.all(moved[missing[fin]] > 1e-6) and np.all(moved[~missing[fin]] == 0.0), variant


def test_a_missing_leaf_is_the_tree_without_it_in_numpy():
    """the reference itself: E missing in every family = the tree without E (same matrices, one factor fewer)"""
    counts = MS.table(41, blank=False)[1:60]
    blanked = counts.copy()
    blanked[:, MS.SPECIES.index("E")] = MS.MISSING
    pb = MS.problem(41, "base", counts=blanked)
    small = MS.problem(41, "base", counts=np.delete(counts, MS.SPECIES.index("E"), axis=1), newick=MS.NEWICK.replace(",E:3", ""),
                       species=[s for s in MS.SPECIES if s != "E"])
    pr = MS.params(pb, "base")
    a = _lnl(pb, pr, None, None)
    b = _lnl(small, pr, None, None)
    assert np.array_equal(a, b)


TABLE = "Desc\tFamily ID\tA\tB\tC\n(null)\tf1\t3\tNA\t1\n(null)\tf2\t0\t?\t2\n(null)\tf3\t-\t70\t0\n(null)\tf4\t4\t4\t4\n"


def test_the_loaders_read_size_and_filter_a_table_with_missing_cells():
    species, ids, plain = P.read_family_table(TABLE)
    assert plain.tolist() == [[3, 0, 1], [0, 0, 2], [0, 70, 0], [4, 4, 4]]           # as today: atoi makes 0 of every such cell
    _, _, counts = P.read_family_table(TABLE, missing_tokens=("NA", "?", "-"))
    assert counts.tolist() == [[3, -1, 1], [0, -1, 2], [-1, 70, 0], [4, 4, 4]] and counts.dtype == np.int32
    _, _, some = P.read_family_table(TABLE, missing_tokens=["NA"])
    assert some.tolist() == [[3, -1, 1], [0, 0, 2], [0, 70, 0], [4, 4, 4]]
    assert P.max_sizes(counts) == P.max_sizes(plain) == (70 + 50, 88)                # from the observed cells
    assert P.max_sizes(np.full((2, 3), -1, dtype=np.int32)) == P.max_sizes(np.zeros((2, 3), dtype=np.int32))
    tree = P.parse_newick("((A:1,B:1):1,C:2);")
    pb = P.build_problem(tree, species, ids, counts, missing_tokens=("NA", "?", "-"))
    # the root filter: a missing cell counts as absent -- f2 has no gene under (A, B), f3 none under C
    assert pb.family_ids == ["f1", "f4"] and pb.counts.tolist() == [[3, -1, 1], [4, 4, 4]] and pb.missing_counts
    assert (pb.max_family_size, pb.max_root_family_size) == (120, 88)
    same = P.build_problem(tree, None, None, TABLE, missing_tokens=("NA", "?", "-"))
    assert same.counts.tolist() == pb.counts.tolist() and same.family_ids == pb.family_ids and same.missing_counts
    plain_pb = P.build_problem(tree, species, ids, plain)
    assert not plain_pb.missing_counts and plain_pb.counts.min() >= 0
    assert not P.build_problem(tree, species, ids, plain, missing_tokens=("NA",)).missing_counts     # the flag follows the cells


def test_the_binding_sets_the_flag_from_the_problem():
    from cafexp_amd import capi
    tree = P.parse_newick("((A:1,B:1):1,C:2);")
    pb = P.build_problem(tree, None, None, TABLE, missing_tokens=("NA", "?", "-"))
    keep = []
    assert capi._c_problem(pb, keep, flags=capi.CAFE_FLAG_NO_DEDUP).flags == capi.CAFE_FLAG_NO_DEDUP | capi.CAFE_FLAG_MISSING_COUNTS == 5
    assert capi._c_problem(MS.with_flag(pb, False), keep).flags == 0
    assert capi.CAFE_COUNT_MISSING == P.COUNT_MISSING == -1
