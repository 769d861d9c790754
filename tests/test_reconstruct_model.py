"""What tests/test_reconstruct_shapes.py can see, shown on the CPU: the numpy statement of the joint reconstruction
(tests/joint_ref.py) against the oracle, the (M, R) pairs against the index arithmetic of csrc/reconstruct.hip, the inputs
against the guards, and eight deliberately wrong statements each told from the right one.

Inputs are test_marginal_shapes' sweep: SWEEP_TREE, sweep_rows scaled to M (with the all-zero-clade and the one-leaf family),
sweep_prior (not uniform: symmetric ties are broken), plus one duplicated row.  Lambda is the sweep's 0.1 where R >= M.  Where
the root is held below M, 0.1 spreads the climb from R to leaves at M over the whole tree and no interior node reaches M --
at M = 16 g + 1 the last row group, a single row, would go unvisited -- so those pairs take 0.01, which puts the climb on the
root's own branches (pair_lambda; test_the_inputs_see_the_guards).  The variant cases, all at 0.1: at (33, 20) a saturated
interior branch above ((A,B),(C,D)), two lambdas and three gamma categories; at (255, 256) -- cafe_create publishes K1's
extents from matrix order 256 on, so the kernels' extent paths exist only there -- the saturated branch again (an empty
extent) and pure birth (death rate 0).

Pure birth is there for one mutant.  backtrack_kernel scans a matrix row only inside K1's non-zero extent [lo, hi] and starts
from (0, j = 0) when lo > 0.  That start matters only on an all-zero product row under a parent state i >= 1 whose block of
rows has P[.][0] = 0.  A parent picks i >= 1 with value 0 only at the root (its scan starts at 1), so i = 1; and under equal
rates P[1][0] = alpha > 0 unless the whole matrix is zero below row 0 (saturated, t_q = 0: an empty extent, nothing is
scanned).  So no equal-rates input can see that guard; with death rate 0, P[i][0] = 0 for every i >= 1 and the family whose
deep clade is all zeros puts an all-zero panel under a root at 1.
"""
import dataclasses
import functools

import numpy as np
import pytest

import bd_lm_ref
import joint_ref as JR
import marginal_ref as MR
from cafexp_amd import problem as P
from helpers import _explicit_problem
from oracle import oracle as O
from test_marginal_shapes import SWEEP_LAMBDA, SWEEP_TREE, sweep_prior, sweep_rows
from test_reconstruct import _check_bp, _joint_likelihood

kTI, kRowsPerBlock = 16, 64                                  # reconstruct.hip: parent sizes per K5 wave and per block

PAIRS = [(2, 2), (3, 5), (15, 14), (16, 16), (17, 9), (31, 40), (32, 32), (33, 20), (63, 64), (64, 63), (65, 129), (127, 100),
         (128, 128), (129, 130), (255, 256), (1023, 1000), (1024, 1024), (1025, 1100), (2047, 1983), (1920, 2047)]
CPU_PAIRS = [p for p in PAIRS if max(p) + 1 <= 513]
VARIANT_PAIR = (33, 20)
EXTENT_PAIR = (255, 256)                                     # the smallest pair whose context has K1's extents (order >= 256)
DUPLICATED_ROW = 3                                           # the family added once more, as the last row

SATURATED_TREE = "(((A:3,B:5):4,(C:2,D:6):3):15,(E:4,(F:1,G:2):2):3,H:7);"      # lambda t = 1.5 above ((A,B),(C,D))
LAMBDA_TREE = "(((A:1,B:1):1,(C:1,D:1):1):1,(E:2,(F:2,G:2):2):2,H:1);"
TWO_LAMBDAS = np.array([SWEEP_LAMBDA, 0.04])
VARIANTS = ("saturated", "two_lambdas", "gamma", "saturated_with_extents", "pure_birth")
SATURATED = ("saturated", "saturated_with_extents")


def pair_lambda(M, R):
    return SWEEP_LAMBDA if R >= M else 0.01


def flags_path(M):
    """reconstruct_impl: the row-group flags steer K5 while a panel has at most 64 row groups"""
    return (M + 15) // 16 <= 64


def root_prior(M, R):
    """rp[j] = compute(j): 0 at j = 0, the sweep's prior from 1 on, min(M, R) + 1 entries"""
    return np.concatenate(([0.0], sweep_prior(R)))[:min(M, R) + 1].astype(np.float32)


def sweep_problem(M, R, tree=SWEEP_TREE):
    rows = sweep_rows(M)
    pb = _explicit_problem(tree, rows + [rows[DUPLICATED_ROW]], M, R)
    assert pb.matrix_size == max(M, R) + 1 and pb.n_families == 8
    return pb


@dataclasses.dataclass
class Case:
    pb: object
    lambdas: np.ndarray
    rp: np.ndarray
    multipliers: object = None
    mus: object = None

    @property
    def K(self):
        return 1 if self.multipliers is None else len(self.multipliers)

    def params(self):
        pr = P.Params(lambdas=self.lambdas, prior=sweep_prior(self.pb.max_root_family_size))
        if self.multipliers is not None:
            pr.multipliers, pr.cat_probs = self.multipliers, np.full(self.K, 1.0 / self.K)
        return pr


def sweep_case(M, R, mus=None):
    return Case(sweep_problem(M, R), np.array([pair_lambda(M, R)]), root_prior(M, R), mus=mus)


def variant_case(name):
    M, R = EXTENT_PAIR if name in ("saturated_with_extents", "pure_birth") else VARIANT_PAIR
    if name in SATURATED:
        return Case(sweep_problem(M, R, SATURATED_TREE), np.array([SWEEP_LAMBDA]), root_prior(M, R))
    if name == "two_lambdas":
        pb = sweep_problem(M, R)
        index = {nd.key(): nd.lambda_index - 1 for nd in P.parse_newick(LAMBDA_TREE, lambda_tree=True).postorder()}
        pb = dataclasses.replace(pb, lambda_index=np.array([index[k] for k in pb.node_names], dtype=np.int32), n_lambdas=2, single_lambda=False)
        assert set(pb.lambda_index) == {0, 1}
        return Case(pb, TWO_LAMBDAS.copy(), root_prior(M, R))
    if name == "gamma":
        _, mult = O.discrete_gamma(3, 0.7)
        return Case(sweep_problem(M, R), np.array([SWEEP_LAMBDA]), root_prior(M, R), multipliers=mult)
    assert name == "pure_birth"
    return Case(sweep_problem(M, R), np.array([SWEEP_LAMBDA]), root_prior(M, R), mus=np.array([0.0]))


def cpu_matrices(case):
    """mats[k][v] without a device: the oracle's, or under death rates tests/bd_lm_ref.py's"""
    mults = [1.0] if case.multipliers is None else list(case.multipliers)
    if case.mus is not None:
        return bd_lm_ref.reference_matrices(case.pb, case.lambdas, case.mus, mults)
    return MR.oracle_matrices(case.pb, case.params(), O)


def interior(pb):
    return [v for v in range(pb.n_nodes) if pb.leaf_taxon[v] < 0]


def node(pb, *leaves):
    """the smallest clade that holds the named leaves"""
    def up(v):
        out = [v]
        while pb.parent[out[-1]] >= 0:
            out.append(int(pb.parent[out[-1]]))
        return out
    paths = [up(int(np.where(pb.leaf_taxon == pb.taxa.index(s))[0][0])) for s in leaves]
    return next(v for v in paths[0] if all(v in p for p in paths[1:]))


@functools.lru_cache(maxsize=None)
def _cpu_sweep(M, R):
    case = sweep_case(M, R)
    mats = cpu_matrices(case)
    return case, mats, JR.joint_reconstruct(case.pb, case.rp, mats[0])


@functools.lru_cache(maxsize=None)
def _cpu_variant(name):
    case = variant_case(name)
    mats = cpu_matrices(case)
    return case, mats, [JR.joint_reconstruct(case.pb, case.rp, m) for m in mats]


def viterbi_sizes(pb, states, seed):
    """Size rows for cafe_branch_probabilities: the reconstructed states, then as many seeded rows uniform in 0..M, edited so
    that on a leaf branch (A under (A,B)) and on an interior branch ((A,B) under ((A,B),(C,D))) there is a parent at 0, a child
    at M, a parent at M and a parent equal to its child.  The table has 2 F rows: `double_families` gives the problem for it."""
    M, F = pb.max_family_size, len(states)
    assert F >= 8
    extra = np.random.default_rng(seed).integers(0, M + 1, size=(F, pb.n_nodes)).astype(np.int32)
    a, ab, abcd = node(pb, "A"), node(pb, "A", "B"), node(pb, "A", "B", "C", "D")
    for r, (child, par) in enumerate(((a, ab), (ab, abcd))):
        lower = max(0, M - 1)
        extra[4 * r + 0, [par, child]] = 0, M                # parent at 0, child at M
        extra[4 * r + 1, [par, child]] = M, lower            # parent at M
        extra[4 * r + 2, [par, child]] = lower, M            # child at M under a parent above 0
        extra[4 * r + 3, [par, child]] = M // 2, M // 2      # parent equal to child
    return np.concatenate([np.asarray(states, dtype=np.int32), extra])


def double_families(pb):
    return dataclasses.replace(pb, counts=np.ascontiguousarray(np.concatenate([pb.counts, pb.counts])),
                               family_ids=pb.family_ids + ["again_" + s for s in pb.family_ids])


# ---------------------------------------------------------------------------------------------------- the pairs
def test_the_pairs_reach_every_edge():
    assert len(PAIRS) == 20 and len(set(PAIRS)) == 20
    Ms = [M for M, R in PAIRS]
    assert {0, 1, 15} <= {M % kTI for M in Ms}                           # the last wave's rows, the extent and flag blocks
    assert {0, 1, 2, 3} == {(M + 1) % 4 for M in Ms}                     # K5's groups of four and the look-ahead clamp
    assert {0, 1, 63} <= {M % kRowsPerBlock for M in Ms}                 # row groups per column tile in the grid decoding
    assert any(M <= 16 for M in Ms) and any(16 < M < 64 for M in Ms)     # one row group; several in one block
    assert any(R < M for M, R in PAIRS) and any(R > M for M, R in PAIRS) and any(R == M for M, R in PAIRS)
    assert {64, 65} <= {(M + 15) // 16 for M in Ms}                      # the flags switch
    assert {0, 1, 15} <= {M % kTI for M, R in PAIRS if max(M, R) + 1 >= 256}      # ... where the context has K1's extents at all
    assert any(flags_path(M) for M in Ms) and any(not flags_path(M) for M in Ms)
    assert [flags_path(M) for M in (1023, 1024, 1025)] == [True, True, False]
    at_limit = [(M, R) for M, R in PAIRS if max(M, R) + 1 == 2048]
    assert any(M > R for M, R in at_limit) and any(R > M for M, R in at_limit)
    assert max(max(p) + 1 for p in PAIRS) == 2048
    assert len(CPU_PAIRS) == 15 and VARIANT_PAIR in CPU_PAIRS
    for M, R in PAIRS:
        assert all(0 <= c <= M for r in sweep_rows(M) for c in r.values())


@pytest.mark.parametrize("name", SATURATED)
def test_the_saturated_cases_are_what_they_say(name):
    case, mats, res = _cpu_variant(name)
    pb = case.pb
    abcd, ab, cd = node(pb, "A", "B", "C", "D"), node(pb, "A", "B"), node(pb, "C", "D")
    assert pb.matrix_size == (257 if name == "saturated_with_extents" else 34)
    assert O.is_saturated(float(pb.branch_length[abcd]), SWEEP_LAMBDA) and pb.parent[ab] == abcd and pb.parent[cd] == abcd
    assert sum(O.is_saturated(float(t), SWEEP_LAMBDA) for v, t in enumerate(pb.branch_length) if pb.parent[v] >= 0) == 1
    assert not mats[0][abcd][1:].any() and mats[0][abcd][0, 0] == 1.0
    states, info = res[0]
    # the node under the saturated branch reconstructs to 0 (its whole row is zero), its interior children go through row 0
    assert np.all(states[:, abcd] == 0) and np.all(info["zero_row"][:, abcd])
    assert np.all(info["via_row0"][:, [ab, cd]]) and not info["via_row0"][:, abcd].any()
    assert np.all(states[:, [ab, cd]] == 0)                  # B[0] = 0 under leaves: row 0 leaves an all-zero row again
    assert np.all(info["root_value"] == 0.0) and np.all(states[:, MR.root_of(pb)] == 1)
    assert JR.block_extent(mats[0][abcd], 1, pb.max_family_size) == (1, 0)


def test_the_other_variant_cases_are_what_they_say():
    case, mats, res = _cpu_variant("two_lambdas")
    pb = case.pb
    abcd, ab = node(pb, "A", "B", "C", "D"), node(pb, "A", "B")
    assert case.pb.n_lambdas == 2 and {int(i) for i in case.pb.lambda_index[[ab, node(case.pb, "F", "G")]]} == {0, 1}
    case, mats, res = _cpu_variant("gamma")
    assert case.K == 3 and len(mats) == 3 and len({r[0].tobytes() for r in res}) >= 2        # the categories reconstruct differently

    case, mats, res = _cpu_variant("pure_birth")
    pb = case.pb
    states, info = res[0]
    P1 = mats[0][abcd]
    assert not P1[1:, 0].any() and JR.block_extent(P1, 1, pb.max_family_size)[0] == 1        # K1's extent of rows 1..16 starts at 1
    f = 5                                                    # the deep clade all zeros
    assert not pb.counts[f, [pb.taxa.index(s) for s in "ABCD"]].any()
    assert states[f, MR.root_of(pb)] == 1 and info["zero_row"][f, abcd] and not info["via_row0"][f, abcd] and states[f, abcd] == 0


# ---------------------------------------------------------------------------------------------------- against the oracle
def test_the_reference_equals_the_oracle():
    """joint_reconstruct on the oracle's matrices against the oracle's own reconstruction, every CPU pair: a family may differ
    only as a near-tie by test_reconstruct._near_tie_only's measure (1e-9), and at most 1 % of all the families may."""
    total = differing = 0
    for M, R in CPU_PAIRS:
        case, mats, (states, _) = _cpu_sweep(M, R)
        pb, pr = case.pb, case.params()
        want = O.reconstruct(pb, case.lambdas, case.rp)[0]
        bad = np.nonzero((states != want).any(axis=1))[0]
        for f in bad:
            la, lb = (_joint_likelihood(pb, pr, case.rp, s[f], 1.0) for s in (states, want))
            assert abs(la - lb) <= 1e-9 * max(la, lb), (M, R, f, la, lb)
        total += len(states)
        differing += len(bad)
        sizes = viterbi_sizes(pb, states, seed=M)
        pb2 = double_families(pb)
        got = JR.branch_probabilities(pb2, sizes, mats[0])
        want = O.branch_probabilities(pb2, case.lambdas, sizes)
        _check_bp(got, want, 1e-12)
        assert np.isfinite(got).sum() >= len(states)
    print("joint_ref against the oracle: %d of %d families differ (near-ties)" % (differing, total))
    assert differing <= 0.01 * total


def test_the_variant_references_equal_the_oracle():
    for name in ("saturated", "two_lambdas", "gamma", "saturated_with_extents"):
        case, mats, res = _cpu_variant(name)
        want = O.reconstruct(case.pb, case.lambdas, case.rp, multipliers=case.multipliers)
        for k in range(case.K):
            assert np.array_equal(res[k][0], want[k]), (name, k)


# ---------------------------------------------------------------------------------------------------- the guards
@pytest.mark.parametrize("M,R", CPU_PAIRS)
def test_the_inputs_see_the_guards(M, R):
    case, mats, (states, info) = _cpu_sweep(M, R)
    pb = case.pb
    inner = interior(pb)
    counts = pb.counts
    assert not counts[5, [pb.taxa.index(s) for s in "ABCD"]].any() and counts[5].any()           # the all-zero clade
    assert (counts[6] > 0).sum() == 1                                                            # the one-leaf family
    assert np.array_equal(counts[7], counts[DUPLICATED_ROW]) and np.array_equal(states[7], states[DUPLICATED_ROW])
    leaves = np.where(pb.leaf_taxon >= 0)[0]
    assert np.array_equal(states[:, leaves], counts[:, pb.leaf_taxon[leaves]])
    if M > 16:
        assert (states[:, inner] > 16 * ((M - 1) // 16)).any()                                   # the last row group
    assert (states == M).any()
    if R >= M or M % 16 == 1:
        assert (states[:, inner] == M).any()                                                     # ... by an interior node
    # B_v[0] = 0 at every interior node (joint_ref's docstring): without an all-zero row only leaves are at 0
    assert (states == 0).any() and not (states[:, inner] == 0).any() and not info["zero_row"].any()
    assert np.all(info["root_value"] > 0)


# ---------------------------------------------------------------------------------------------------- the mutants
def test_every_mutant_is_told_apart():
    """Each wrong statement differs from the right one in at least one family or cell of some input; the table says where."""
    inputs = [("M %d R %d" % p, _cpu_sweep(*p)) for p in CPU_PAIRS]
    inputs += [(name, (lambda c, m, r: (c, m, r[0]))(*_cpu_variant(name))) for name in ("saturated", "saturated_with_extents", "pure_birth")]
    told = {m: [] for m in JR.MUTANTS + JR.VITERBI_MUTANTS}
    for label, (case, mats, (states, _)) in inputs:
        pb = case.pb
        for m in JR.MUTANTS:
            if not np.array_equal(JR.joint_reconstruct(pb, case.rp, mats[0], mutant=m)[0], states):
                told[m].append(label)
        sizes = viterbi_sizes(pb, states, seed=pb.max_family_size)
        pb2 = double_families(pb)
        right = JR.branch_probabilities(pb2, sizes, mats[0])
        for m in JR.VITERBI_MUTANTS:
            if not np.array_equal(JR.branch_probabilities(pb2, sizes, mats[0], mutant=m), right, equal_nan=True):
                told[m].append(label)
    for m, where in told.items():
        print("%-30s told apart at %d of %d inputs: %s" % (m, len(where), len(inputs), ", ".join(where) or "-"))
    assert all(told.values()), [m for m, w in told.items() if not w]
    assert told["zero_row_takes_first_scanned"] == ["pure_birth"]        # the module docstring's argument
