// cafexp_hip: thin driver around the host adapter -- the part of `cafexp -t -i [-l|-m -y] [-k] [-a]
// [-e] [-p] [-f] [-z]` (src/cafexp.cpp:175, src/execute.cpp:42-150) that ends in scorer calls.
// With a fixed lambda it evaluates one infer_family_likelihoods call; without, it runs the
// Nelder-Mead search on the GPU scorer.  Output: one JSON object on stdout.
// The command line is read and refused in driver_options.cpp; the modes main() dispatches to are in driver.cpp.
#include <cstdio>

#include "cafe_host.h"

using namespace cafe;

static void usage() {
    std::fprintf(stderr,
        "usage: cafexp_hip -t TREE -i FAMILIES [-l LAMBDA | -m L1,L2,.. -y LAMBDA_TREE | -y LAMBDA_TREE] [-k K] [-a ALPHA]\n"
        "                  [--mu M1[,M2,..] | --estimate-mu]   separate death rates, one per lambda: fixed, or searched together with lambda\n"
        "                  (start mu = lambda); every call after the search runs under the pair, <Model>_results.txt gains a Mu: line\n"
        "                  [-e [ERRMODEL]] [-p [POISSON_LAMBDA]] [-f ROOTDIST] [-z] [-s SEED] [-I MAXITER] [-d DEVICE | --gpus N] [--reps N] [--family-out FILE] [-o OUTDIR] [--limit N]\n"
        "                  [--pvalues NSIM [--pvalues-device] [--pvalues-out FILE] [--pvalues-cond FILE:K]] [--sizes M,R]\n"
        "                  [--reconstruct [-P PVALUE]]   (with -o: the reports of reconstruction::write_results)\n"
        "                  [--reconstruct-marginal [LEVEL]]   posterior size of every node under the fitted model: mean, mode, equal-tailed\n"
        "                  interval at LEVEL (default 0.95), probability that each branch contracted / expanded; with -o:\n"
        "                  <Model>_posterior_sizes.tab (mean:mode:lo-hi) and <Model>_posterior_change.tab (p_decrease:p_increase); one GPU\n"
        "                  [--sample-histories N [--sample-seed S]]   N whole ancestral histories per family drawn from the posterior of the\n"
        "                  fitted model (seed S, else -s, else 1); with -o: <Model>_sampled_change.tab, per node the mean and the equal-tailed\n"
        "                  interval (LEVEL of --reconstruct-marginal, default 0.95) across the draws of how many families expanded /\n"
        "                  contracted on its branch and of the net change in genes; one GPU\n"
        "                  [--expected-events]   after the search: the expected number of gene gains (births) and losses (deaths) on every\n"
        "                  branch of every family given its counts, under the fitted model; with -o: <Model>_expected_events.tab (gains:losses\n"
        "                  per family and node) and <Model>_branch_events.tab (per branch: gains, losses, net, turnover over the table); one GPU\n"
        "                  [--branch-change [D] [-P PVALUE]]   after the search: for every family and branch the posterior of the change\n"
        "                  size(node) - size(parent) under the fitted model, exact in a band of +-D (default 10) with the mass beyond it in two\n"
        "                  tails -> in -o OUTDIR (default results) <Model>_branch_change.tab (mean:mode:[lo,hi]:p_below_band:p_above_band, the\n"
        "                  equal-tailed interval at level 1 - PVALUE, default 0.95; lo = -D-1 / hi = D+1: beyond the band) and\n"
        "                  <Model>_branch_change_summary.tab (per branch: summed mean change, families whose interval lies wholly above / wholly\n"
        "                  below 0, families whose interval is clipped by the band: raise D); one GPU, not with -b, --simulate or missing cells\n"
        "                  [--standard-errors]   after the search: the per-family scores at the optimum, the standard error of every\n"
        "                  estimated lambda, mu (--estimate-mu) and alpha from their outer product, Wald 95 %% intervals, correlations and the\n"
        "                  total score -> <Model>_standard_errors.txt in -o OUTDIR (default results); one GPU, not with -b or --simulate\n"
        "                  [--rate-shift-scan [-P PVALUE]]   after the search: one pass at the optimum keeps the score of every branch's rate\n"
        "                  and their information; Rao score tests of a rate shift on every branch and in every clade (and, under death\n"
        "                  rates, of birth and death jointly), Holm-adjusted -> <Model>_rate_shift_scan.tab in -o OUTDIR (default results), and\n"
        "                  <Model>_rate_shift_lambda_tree.txt (-y format) when a clade passes PVALUE (default 0.05); one GPU, not with -b or --simulate\n"
        "                  [--missing TOKENS] [--mask-cells FILE]   cells whose count is unknown: spelled like one of the comma list TOKENS\n"
        "                  (e.g. NA,?,-), or named by a line family<TAB>species of FILE (the first two columns of <Model>_leaf_outliers.tab\n"
        "                  are such a file).  They are summed out of the likelihood (the family on the tree without that species); M and R\n"
        "                  come from the observed cells; with --leaf-predictive also <Model>_imputed_counts.tab (family, species, mean,\n"
        "                  sd, 95 %% interval of the predicted count).  Works with -b and --gpus; not with --pvalues, --reconstruct[-marginal],\n"
        "                  --sample-histories, --standard-errors, --expected-events, --rate-shift-scan, --branch-change\n"
        "                  [--leaf-predictive [-P PVALUE]]   after the search: for every family and species the distribution of the species'\n"
        "                  count predicted from the counts of all the other species under the fitted model -> in -o OUTDIR (default results)\n"
        "                  <Model>_leaf_predictive.tab (mean:sd:p_low:p_high, the two one-sided tails of the observed count),\n"
        "                  <Model>_leaf_outliers.tab (the cells whose two-sided p, Holm-adjusted over the table, is <= PVALUE, default 0.05) and\n"
        "                  <Model>_species_fit.tab (per species: mean standardised residual, outliers low / high, sum log p_obs); one GPU, not\n"
        "                  with -b or --simulate\n"
        "                  [--root-sum]   every search and every scorer call under the marginal likelihood sum_s L_s prior_s of a family instead\n"
        "                  of the reference's max_s (cafe_set_root_rule): the objective the posterior reports condition on.  <Model>_results.txt\n"
        "                  names the rule; --standard-errors and --rate-shift-scan then differentiate the sum; the gamma model also writes\n"
        "                  Gamma_category_posterior.tab (per family the posterior probability of every rate category) in -o OUTDIR (default results)\n"
        "                  [--estimate-rootdist [ROUNDS]]   implies --root-sum: the root size distribution estimated by EM, at most ROUNDS\n"
        "                  (default 10) rounds behind the usual search under the starting prior (uniform, -p or -f).  A round sets\n"
        "                  prior[s] = mean over the families of P(root = s | data) at the current optimum, rounded to float, and searches again\n"
        "                  from that optimum; it stops when a round lowers -lnL by less than 1e-3 relative.  No smoothing: a size that no family\n"
        "                  supports keeps probability 0.  Writes <Model>_root_distribution.txt (size<TAB>probability) and one line per round in\n"
        "                  <Model>_results.txt to -o OUTDIR (default results); one GPU, not with -b\n"
        "                  [--rootdist-probs FILE]   the root prior from such a file of probabilities (instead of -p / -f)\n"
        "  --search-batch G: look-ahead Nelder-Mead -- a point whose score is not known goes to the device with the points the search may ask\n"
        "                  for next, G in one call (cafe_score_batch); same trajectory, files and result, fewer dependent calls.  2 <= G,\n"
        "                  G x K <= 32; one GPU, not with -b or --simulate.  Pays at small matrix orders only (a batch of 4 costs 1.1 to 1.5\n"
        "                  calls at order 141, 3.5 at order 751)\n"
        "  --gpus N: the scorer calls shard the families over devices 0..N-1 (one host thread per GPU, one RCCL all-reduce per call)\n"
        "lambda per family (the reference's -b): cafexp_hip -t TREE -i FAMILIES -b [-y LAMBDA_TREE] [-e ERRMODEL] [-p [L]] [-z] [-s SEED] [-I MAXITER]\n"
        "                  [--workspace BYTES] [-o OUTDIR]   writes OUTDIR (default results)/Base_lambda_per_family.txt, one line per family\n"
        "                  [--family-mu M1[,M2,..] | --family-mu estimate]   separate death rates per family (only with -b): fixed at the given\n"
        "                  rates, one per lambda, or searched with each family's lambdas (start mu = lambda); also writes Base_mu_per_family.txt\n"
        "gene gain rate: cafexp_hip -t TREE -i FAMILIES (--gain NU | --estimate-gain) [--root-absent P0] [--gain-unconditional] [--gain-posterior] [--gain-dense [--gain-scaled]] [-l LAMBDA | -m L1,L2,..]\n"
        "                  [-y LAMBDA_TREE] [--mu M1,.. | --estimate-mu] [-e ERRMODEL] [-p [L]] [-f ROOTDIST] [--missing TOKENS] [--mask-cells FILE] [-z] [-o OUTDIR]\n"
        "                  birth-death with immigration (n -> n+1 at rate n lambda + NU): a family absent in an ancestor can appear below it.  One set\n"
        "                  of rates for the table, fitted under the sum rule to the likelihood conditional on a family being seen in at least one\n"
        "                  species (--gain-unconditional: without that correction); the root is absent with probability P0 (default 0).  First the fit\n"
        "                  without NU, then with it from that optimum.  Writes OUTDIR/Gain_results.txt and Gain_family_likelihoods.txt.  -z keeps the\n"
        "                  families of one clade only, which this model is about.  Base model, one GPU; not with -k / -a, -b, --gpus, --simulate,\n"
        "                  --pvalues, a reconstruction or posterior report (but --leaf-predictive and --reconstruct-marginal with --gain-dense, below), or --search-batch\n"
        "                  [--gain-dense]   score every point of the search, and the final table, by cafe_score_gain: each branch's matrix built\n"
        "                  once per point and all distinct families pruned together by fp64 MFMA GEMMs; values agree with the default path to rounding;\n"
        "                  with --gain-posterior the posterior runs on the same prune, by cafe_gain_posterior_dense\n"
        "                  [--leaf-predictive [-P PVALUE]]   only with --gain-dense (also with --gain-scaled and missing cells): after the fit, at the\n"
        "                  fitted rates, the leave-one-out distribution of every species' count under the gain model, by cafe_gain_leaf_predictive ->\n"
        "                  OUTDIR/Gain_leaf_predictive.tab, Gain_leaf_outliers.tab, Gain_species_fit.tab (the reports of --leaf-predictive above; its\n"
        "                  sum log p_obs is comparable with the fit without NU) and, when cells are missing, Gain_imputed_counts.tab\n"
        "                  [--reconstruct-marginal [LEVEL]]   only with --gain-dense (also with --gain-scaled; not with missing cells): after the fit,\n"
        "                  at the fitted rates, posterior size of every node (mean, mode, equal-tailed interval) and the probability that the family\n"
        "                  shrank or grew on every branch under the gain model, by cafe_gain_marginal_dense -> OUTDIR/Gain_posterior_sizes.tab,\n"
        "                  Gain_posterior_change.tab (the formats of --reconstruct-marginal above)\n"
        "                  [--standard-errors]   only with --gain-dense: standard errors of the searched lambda, mu and nu from the per-family scores\n"
        "                  of the (conditional) likelihood at the fitted rates, by cafe_gain_score_gradient -> OUTDIR/Gain_standard_errors.txt\n"
        "                  [--gain-scaled]   only with --gain-dense: the dense prune holds its panels as mantissas and one binary exponent per\n"
        "                  (node, family), so families whose likelihood lies below fp64's range (trees of a few dozen taxa with counts that disagree\n"
        "                  across clades) keep a finite -lnL and their posteriors; applies to the search and to --gain-posterior\n"
        "                  [--gain-posterior]   after the fit, at the fitted rates: for every family and node the posterior probability that the\n"
        "                  family is absent there and its mean size, and for every branch that it originated (parent absent, node present) or was\n"
        "                  lost (parent present, node absent) on it: OUTDIR/Gain_origins.tab (p_absent:mean per node, p_gain:p_loss per branch) and\n"
        "                  Gain_branch_origins.tab (per branch: the expected numbers of families that originated, were lost, are present, and the\n"
        "                  families with p_gain > 0.5)\n"
        "simulation (the reference's -s; -s here is the SEED): cafexp_hip -t TREE (-l LAMBDA | -m L1,L2,.. -y LAMBDA_TREE) --simulate [N]\n"
        "                  [-k K] [-a ALPHA] [-e ERRMODEL] [-f ROOTDIST] [-s SEED] [-o OUTDIR] [--simulate-device [--workspace BYTES]] [-d DEVICE]\n"
        "  writes OUTDIR (default results)/simulation.txt and simulation_truth.txt; N families (root sizes 0..99), or the\n"
        "  -f distribution pared to N.  --simulate-device: the draws on the GPU (same distribution, another sample).\n"
        "  --mu M1[,M2,..]: simulate under separate death rates, one per lambda (a gamma multiplier scales both rates).\n"
        "  The gamma model (-k > 1 or -a > 0) needs -a > 0: the reference would draw from Gamma(-1, -1) instead.\n");
}

int main(int argc, char** argv) {
    driver_options o;
    if (!parse_options(argc, argv, o)) { usage(); return 2; }
    if (const char* why = driver_refusal(o)) {                   // before anything is read or written
        if (why == driver_usage_exit) { usage(); return 2; }
        std::fprintf(stderr, "cafexp_hip: %s\n", why);
        return 1;
    }
    normalise_options(o);
    if (o.simulate_n >= 0) return run_simulation(o);
    try {
        user_data d;
        driver_model m;
        load_inputs(o, true, d);
        build_model(o, d, m);
        if (o.gain_run()) run_gain_model(o, d, m);
        else if (o.per_family) run_lambda_per_family(o, d, m);
        else run_fitted_model(o, d, m);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "cafexp_hip: %s\n", e.what());
        return 1;
    }
    return 0;
}

