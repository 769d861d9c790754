// cafexp_hip: thin driver around the host adapter -- the part of `cafexp -t -i [-l|-m -y] [-k] [-a]
// [-e] [-p] [-f] [-z]` (src/cafexp.cpp:175, src/execute.cpp:42-150) that ends in scorer calls.
// With a fixed lambda it evaluates one infer_family_likelihoods call; without, it runs the
// Nelder-Mead search on the GPU scorer.  Output: one JSON object on stdout.
#include <sys/stat.h>

#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

#include "cafe_host.h"

#include <iomanip>
#include "../../include/cafe_mi355x.h"

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
        "gene gain rate: cafexp_hip -t TREE -i FAMILIES (--gain NU | --estimate-gain) [--root-absent P0] [--gain-unconditional] [--gain-posterior] [-l LAMBDA | -m L1,L2,..]\n"
        "                  [-y LAMBDA_TREE] [--mu M1,.. | --estimate-mu] [-e ERRMODEL] [-p [L]] [-f ROOTDIST] [--missing TOKENS] [--mask-cells FILE] [-z] [-o OUTDIR]\n"
        "                  birth-death with immigration (n -> n+1 at rate n lambda + NU): a family absent in an ancestor can appear below it.  One set\n"
        "                  of rates for the table, fitted under the sum rule to the likelihood conditional on a family being seen in at least one\n"
        "                  species (--gain-unconditional: without that correction); the root is absent with probability P0 (default 0).  First the fit\n"
        "                  without NU, then with it from that optimum.  Writes OUTDIR/Gain_results.txt and Gain_family_likelihoods.txt.  -z keeps the\n"
        "                  families of one clade only, which this model is about.  Base model, one GPU; not with -k / -a, -b, --gpus, --simulate,\n"
        "                  --pvalues, a reconstruction or posterior report, or --search-batch\n"
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

static std::string slurp_first_line(const std::string& path) {
    std::ifstream f(path);
    if (!f.is_open()) throw std::runtime_error("Failed to open " + path);
    std::string line;
    std::getline(f, line);
    return line;
}

static void print_num(const char* key, double v, bool comma = true) {
    if (std::isinf(v)) std::printf("\"%s\": \"%sinf\"%s", key, v < 0 ? "-" : "", comma ? ", " : "");
    else if (std::isnan(v)) std::printf("\"%s\": \"nan\"%s", key, comma ? ", " : "");
    else std::printf("\"%s\": %.17g%s", key, v, comma ? ", " : "");
}

// "V1,V2,.." -> rates
static std::vector<double> parse_rates(const std::string& list) {
    std::vector<double> v;
    std::stringstream ss(list);
    std::string tok;
    while (std::getline(ss, tok, ',')) v.push_back(std::stod(tok));
    return v;
}

// simulator::simulate (simulator.cpp:113-147) with the checks of input_parameters::check_input (io.cpp:55-98)
static int simulate_main(const std::string& tree_path, const std::string& fam_path, const std::string& rootdist_path,
                         const std::string& lambda_tree_path, const std::string& multi, const std::string& err_path, bool use_err,
                         double fixed_lambda, double fixed_alpha, int k, int nsims, bool on_device, uint64_t seed, int device,
                         size_t workspace, std::string out_dir, const std::string& mu_list) {
    try {
        if (!multi.empty() && lambda_tree_path.empty()) throw std::runtime_error("Multiple lambda values (-m) specified with no lambda tree (-y)");
        if (!fam_path.empty() && !rootdist_path.empty()) throw std::runtime_error("Options -i and -f are mutually exclusive.");
        if (fixed_lambda <= 0.0 && multi.empty()) throw std::runtime_error("Cannot simulate without initial lambda values");
        const bool gamma = fixed_alpha > 0 || k > 1;                 // build_models (core.cpp:26)
        if (gamma && !(fixed_alpha > 0)) throw std::runtime_error("Cannot simulate gamma clusters without an alpha value");
        if (use_err && err_path.empty()) throw std::runtime_error("Simulation needs an error model file (-e FILE)");
        user_data d;
        d.p_tree.reset(parse_newick(slurp_first_line(tree_path), false));
        if (!err_path.empty()) {
            std::ifstream f(err_path);
            if (!f.is_open()) throw std::runtime_error("Failed to open " + err_path + ". Exiting...");
            d.p_error_model.reset(new error_model);
            read_error_model_file(f, d.p_error_model.get());
        }
        if (!lambda_tree_path.empty()) {
            d.p_lambda_tree.reset(parse_newick(slurp_first_line(lambda_tree_path), true));
            d.p_tree->validate_lambda_tree(d.p_lambda_tree.get());
        }
        if (fixed_lambda > 0) d.p_lambda.reset(new single_lambda(fixed_lambda));
        if (!multi.empty()) {
            std::vector<double> v;
            std::stringstream ss(multi);
            std::string tok;
            while (std::getline(ss, tok, ',')) v.push_back(std::stod(tok));
            d.p_lambda.reset(new multiple_lambda(d.p_lambda_tree->get_lambda_index_map(), v));
        }
        if (!rootdist_path.empty()) {
            std::ifstream f(rootdist_path);
            if (!f.is_open()) throw std::runtime_error("Failed to open file '" + rootdist_path + "'");
            read_rootdist(f, d.rootdist);
        }
        const double alpha = gamma ? fixed_alpha : 0.0;
        const std::vector<double> mus = parse_rates(mu_list);       // one per lambda (checked by the simulator); empty: lambda = mu
        auto t0 = std::chrono::steady_clock::now();
        simulation sim = on_device
            ? simulate_families_device(d.p_tree.get(), d.p_lambda.get(), d.p_error_model.get(), d.rootdist, nsims, alpha, device, seed, workspace, &mus)
            : simulate_families(d.p_tree.get(), d.p_lambda.get(), d.p_error_model.get(), d.rootdist, nsims, alpha, device, &mus);
        const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (out_dir.empty()) out_dir = "results";                   // filename() (core.h:196)
        if (::mkdir(out_dir.c_str(), 0777) != 0 && errno != EEXIST) throw std::runtime_error("Failed to create directory " + out_dir);
        auto t1 = std::chrono::steady_clock::now();
        {
            std::ofstream leaves(out_dir + "/simulation.txt");
            print_simulations(leaves, false, sim);
            std::ofstream truth(out_dir + "/simulation_truth.txt");
            print_simulations(truth, true, sim);
            if (!leaves || !truth) throw std::runtime_error("Failed to write the simulations to " + out_dir);
        }
        const double write_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
        const double avg = average_multiplier(sim);
        if (fixed_lambda > 0) std::cout << "Average multiplier for simulated values: " << avg << std::endl;     // simulator.cpp:141-144
        std::printf("{\"model\": \"%s\", \"mode\": \"%s\", \"n_families\": %zu, \"max_family_size\": %d, \"seconds\": %.6f, \"write_seconds\": %.6f, ",
                    gamma ? "Gamma" : "Base", on_device ? "device" : "host", sim.n_families, sim.max_family_size, seconds, write_s);
        print_num("average_multiplier", avg, false);
        if (!mus.empty()) {
            std::printf(", \"mu\": [");
            for (size_t i = 0; i < mus.size(); ++i) std::printf("%s%.17g", i ? ", " : "", mus[i]);
            std::printf("]");
        }
        if (!sim.multipliers.empty() && sim.multipliers.size() <= 1000) {     // one per chunk of 50 families
            std::printf(", \"multipliers\": [");
            for (size_t i = 0; i < sim.multipliers.size(); ++i) std::printf("%s%.17g", i ? ", " : "", sim.multipliers[i]);
            std::printf("]");
        }
        std::printf("}\n");
    } catch (const std::exception& e) {
        std::fflush(stdout);
        std::fprintf(stderr, "cafexp_hip: %s\n", e.what());
        return 1;
    }
    return 0;
}

int main(int argc, char** argv) {
    std::string tree_path, fam_path, lambda_tree_path, multi, err_path, rootdist_path, family_out, out_dir;
    std::string pvalues_out, pvalues_cond;
    int simulate_n = -1;                                         // -1: estimation; >= 0: simulation (0 = no count given)
    bool simulate_on_device = false;
    size_t sim_workspace = 0;
    int pvalue_sims = 0, force_m = -1, force_r = -1;
    bool do_reconstruct = false, pvalues_on_device = false;
    bool do_marginal = false;                                    // --reconstruct-marginal [LEVEL]
    double marginal_level = 0.95;
    int history_draws = 0;                                       // --sample-histories N
    bool do_histories = false, have_history_seed = false;
    uint64_t history_seed = 1;                                   // --sample-seed S; else -s; else this
    double test_pvalue = 0.05;                                   // input_parameters::pvalue default (io.h)
    long limit = -1;
    double fixed_lambda = 0, fixed_alpha = -1, poisson = 0;
    int k = 1, device = 0, max_iter = 300, reps = 1, n_gpus = 1;
    bool use_err = false, use_poisson = false, keep_all = false;
    bool per_family = false, gpus_given = false, alpha_given = false;      // -b: one lambda (vector) per family
    std::string mu_list;                                         // --mu: fixed death rates, one per lambda
    bool estimate_mu = false;                                    // --estimate-mu: death rates searched with the lambdas
    std::string family_mu;                                       // --family-mu (with -b): rates, or "estimate"
    bool do_standard_errors = false;                             // --standard-errors
    bool do_events = false;                                      // --expected-events
    bool do_rate_shift = false;                                  // --rate-shift-scan
    bool do_leaf_predictive = false;                             // --leaf-predictive
    bool do_branch_change = false;                               // --branch-change [D]
    int branch_change_band = 10;
    std::string missing_list, mask_path;                         // --missing TOKENS, --mask-cells FILE: cells whose count is unknown
    bool root_sum = false;                                       // --root-sum: score under CAFE_ROOT_SUM
    bool estimate_rootdist = false;                              // --estimate-rootdist [ROUNDS]
    int rootdist_rounds = 10;
    std::string rootdist_probs;                                  // --rootdist-probs FILE
    unsigned seed = 0;
    bool have_seed = false;
    gain_request gain;                                           // --gain NU, --estimate-gain, --root-absent P0, --gain-unconditional
    int search_batch = 1;                                        // --search-batch G: look-ahead search, G points per device call
    bool search_batch_given = false;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> std::string { if (i + 1 >= argc) { usage(); std::exit(2); } return argv[++i]; };
        auto optional = [&]() -> std::string { if (i + 1 < argc && argv[i + 1][0] != '-') return argv[++i]; return ""; };
        if (a == "-t") tree_path = next();
        else if (a == "-i") fam_path = next();
        else if (a == "-l") fixed_lambda = std::stod(next());
        else if (a == "-m") multi = next();
        else if (a == "-y") lambda_tree_path = next();
        else if (a == "-k") k = std::stoi(next());
        else if (a == "-a") { fixed_alpha = std::stod(next()); alpha_given = true; }
        else if (a == "-b") per_family = true;
        else if (a == "--mu") mu_list = next();
        else if (a == "--estimate-mu") estimate_mu = true;
        else if (a == "--family-mu") family_mu = next();
        else if (a == "--standard-errors") do_standard_errors = true;
        else if (a == "--expected-events") do_events = true;
        else if (a == "--rate-shift-scan") do_rate_shift = true;
        else if (a == "--leaf-predictive") do_leaf_predictive = true;
        else if (a == "--branch-change") { do_branch_change = true; std::string v = optional(); if (!v.empty()) branch_change_band = std::stoi(v); }
        else if (a == "--missing") missing_list = next();
        else if (a == "--mask-cells") mask_path = next();
        else if (a == "--root-sum") root_sum = true;
        else if (a == "--estimate-rootdist") { estimate_rootdist = root_sum = true; std::string v = optional(); if (!v.empty()) rootdist_rounds = std::stoi(v); }
        else if (a == "--rootdist-probs") rootdist_probs = next();
        else if (a == "-e") { use_err = true; err_path = optional(); }
        else if (a == "-p") { use_poisson = true; std::string v = optional(); poisson = v.empty() ? 0 : std::stod(v); }
        else if (a == "-f") rootdist_path = next();
        else if (a == "-z") keep_all = true;
        else if (a == "-s") { seed = (unsigned)std::stoul(next()); have_seed = true; }
        else if (a == "-I") max_iter = std::stoi(next());
        else if (a == "-d") device = std::stoi(next());
        else if (a == "--gpus") { n_gpus = std::stoi(next()); gpus_given = true; }
        else if (a == "--reps") reps = std::stoi(next());
        else if (a == "--family-out") family_out = next();
        else if (a == "-o") out_dir = next();
        else if (a == "--limit") limit = std::stol(next());
        else if (a == "--sizes") {                               // M,R instead of the data-derived maxima (tests)
            std::string v = next();
            const size_t comma = v.find(',');
            force_m = std::stoi(v.substr(0, comma)); force_r = std::stoi(v.substr(comma + 1));
        }
        else if (a == "--reconstruct") do_reconstruct = true;
        else if (a == "--reconstruct-marginal") { do_marginal = true; std::string v = optional(); if (!v.empty()) marginal_level = std::stod(v); }
        else if (a == "--sample-histories") { do_histories = true; history_draws = std::stoi(next()); }
        else if (a == "--sample-seed") { history_seed = std::stoull(next()); have_history_seed = true; }
        else if (a == "-P") test_pvalue = std::stod(next());
        else if (a == "--pvalues-device") pvalues_on_device = true;
        else if (a == "--pvalues") pvalue_sims = std::stoi(next());
        else if (a == "--pvalues-out") pvalues_out = next();
        else if (a == "--pvalues-cond") pvalues_cond = next();
        else if (a == "--simulate") { std::string v = optional(); simulate_n = v.empty() ? 0 : std::stoi(v); }
        else if (a == "--simulate-device") simulate_on_device = true;
        else if (a == "--workspace") sim_workspace = std::stoull(next());
        else if (a == "--search-batch") { search_batch = std::stoi(next()); search_batch_given = true; }
        else if (a == "--gain") { gain.gain = true; gain.nu = std::stod(next()); }
        else if (a == "--estimate-gain") gain.estimate_gain = true;
        else if (a == "--root-absent") { gain.root_absent_given = true; gain.root_absent = std::stod(next()); }
        else if (a == "--gain-unconditional") gain.unconditional = true;
        else if (a == "--gain-posterior") gain.posterior = true;
        else { usage(); return 2; }
    }
    {                                                            // the gain model: refused before anything is read or written
        gain.gamma = k > 1 || alpha_given; gain.per_family = per_family; gain.gpus = gpus_given; gain.simulate = simulate_n >= 0;
        gain.pvalues = pvalue_sims > 0; gain.reconstruct = do_reconstruct; gain.marginal = do_marginal; gain.histories = do_histories;
        gain.standard_errors = do_standard_errors; gain.events = do_events; gain.rate_shift = do_rate_shift; gain.leaf_predictive = do_leaf_predictive;
        gain.branch_change = do_branch_change; gain.rootdist_em = estimate_rootdist; gain.search_batch = search_batch_given;
        gain.estimate_error = use_err && err_path.empty();
        if (const char* why = gain_refusal(gain)) { std::fprintf(stderr, "cafexp_hip: %s\n", why); return 1; }
    }
    const bool gain_run = gain.gain || gain.estimate_gain;
    if (search_batch_given) {                                    // refused before anything is read or written
        const char* why = nullptr;
        const int K = (fixed_alpha > 0 || k > 1) ? std::max(1, k) : 1;
        if (search_batch < 2) why = "--search-batch: G must be at least 2";
        else if ((long)search_batch * K > 32) why = "--search-batch: G x K (the -k categories) must not exceed 32";
        else if (n_gpus > 1) why = "--search-batch scores its points in one call on one GPU: --gpus N > 1 is not supported with it";
        else if (per_family) why = "--search-batch drives the search of one fitted model: -b is not supported with it";
        else if (simulate_n >= 0) why = "--search-batch drives a search: --simulate is not supported with it";
        if (why) { std::fprintf(stderr, "cafexp_hip: %s\n", why); return 1; }
    }
    if (simulate_n >= 0) {
        if (tree_path.empty()) { usage(); return 2; }
        if (estimate_mu) { std::fprintf(stderr, "cafexp_hip: --simulate draws under given rates: --estimate-mu is not supported with it (give --mu)\n"); return 1; }
        if (!family_mu.empty()) { std::fprintf(stderr, "cafexp_hip: --family-mu sets the death rates of -b: it is not supported without -b\n"); return 1; }
        if (do_standard_errors) { std::fprintf(stderr, "cafexp_hip: --standard-errors belongs to a fitted model: --simulate is not supported with it\n"); return 1; }
        if (do_events) { std::fprintf(stderr, "cafexp_hip: --expected-events belongs to a fitted model: --simulate is not supported with it\n"); return 1; }
        if (do_rate_shift) { std::fprintf(stderr, "cafexp_hip: --rate-shift-scan belongs to a fitted model: --simulate is not supported with it\n"); return 1; }
        if (do_leaf_predictive) { std::fprintf(stderr, "cafexp_hip: --leaf-predictive belongs to a fitted model: --simulate is not supported with it\n"); return 1; }
        if (do_branch_change) { std::fprintf(stderr, "cafexp_hip: --branch-change belongs to a fitted model: --simulate is not supported with it\n"); return 1; }
        if (have_seed) randomizer_engine.seed(seed);
        return simulate_main(tree_path, fam_path, rootdist_path, lambda_tree_path, multi, err_path, use_err, fixed_lambda, fixed_alpha, k,
                             simulate_n, simulate_on_device, have_seed ? seed : randomizer_engine(), device, sim_workspace, out_dir, mu_list);
    }
    if (tree_path.empty() || fam_path.empty()) { usage(); return 2; }
    if (!missing_list.empty() || !mask_path.empty()) {           // unknown cells are summed out by the scorer, -b and --leaf-predictive only
        const char* why = nullptr;
        if (!missing_list.empty() && parse_missing_tokens(missing_list).empty()) why = "--missing: TOKENS must name at least one spelling, e.g. NA,?,-";
        else if (pvalue_sims > 0) why = "--pvalues simulates complete families: it is not supported on a table with missing cells (--missing / --mask-cells)";
        else if (do_reconstruct) why = "--reconstruct reads every leaf count: it is not supported on a table with missing cells (--missing / --mask-cells)";
        else if (do_marginal) why = "--reconstruct-marginal is not ported to missing cells: it is not supported with --missing / --mask-cells";
        else if (do_histories) why = "--sample-histories is not ported to missing cells: it is not supported with --missing / --mask-cells";
        else if (do_standard_errors) why = "--standard-errors is not ported to missing cells: it is not supported with --missing / --mask-cells";
        else if (do_events) why = "--expected-events is not ported to missing cells: it is not supported with --missing / --mask-cells";
        else if (do_rate_shift) why = "--rate-shift-scan is not ported to missing cells: it is not supported with --missing / --mask-cells";
        else if (do_branch_change) why = "--branch-change is not ported to missing cells: it is not supported with --missing / --mask-cells";
        if (why) { std::fprintf(stderr, "cafexp_hip: %s\n", why); return 1; }
    }
    if (estimate_mu || !mu_list.empty()) {
        const char* why = nullptr;
        if (estimate_mu && !mu_list.empty()) why = "--mu fixes the death rates and --estimate-mu searches them: give one of the two";
        else if (per_family) why = "-b runs the lambda = mu kernel: --mu / --estimate-mu are not supported with it";
        else if (estimate_mu && (fixed_lambda > 0 || !multi.empty())) why = "--estimate-mu searches lambda and mu together: -l / -m are not supported with it";
        if (why) { std::fprintf(stderr, "cafexp_hip: %s\n", why); return 1; }
    }
    if (!family_mu.empty() && !per_family) {
        std::fprintf(stderr, "cafexp_hip: --family-mu sets the death rates of -b: it is not supported without -b\n");
        return 1;
    }
    if (do_standard_errors) {
        const char* why = nullptr;
        if (gpus_given) why = "--standard-errors runs on one GPU: --gpus is not supported with it";
        else if (per_family) why = "--standard-errors needs one fitted model: -b is not supported with it";
        if (why) { std::fprintf(stderr, "cafexp_hip: %s\n", why); return 1; }
    }
    if (do_rate_shift) {
        const char* why = nullptr;
        if (gpus_given) why = "--rate-shift-scan runs on one GPU: --gpus is not supported with it";
        else if (per_family) why = "--rate-shift-scan needs one fitted model: -b is not supported with it";
        if (why) { std::fprintf(stderr, "cafexp_hip: %s\n", why); return 1; }
    }
    if (do_marginal) {
        const char* why = nullptr;
        if (gpus_given) why = "--reconstruct-marginal runs on one GPU: --gpus is not supported with it";
        else if (per_family) why = "--reconstruct-marginal needs one fitted model: -b is not supported with it";
        else if (!(marginal_level > 0 && marginal_level < 1)) why = "--reconstruct-marginal: LEVEL must lie in (0, 1)";
        if (why) { std::fprintf(stderr, "cafexp_hip: %s\n", why); return 1; }
    }
    if (do_events) {
        const char* why = nullptr;
        if (gpus_given) why = "--expected-events runs on one GPU: --gpus is not supported with it";
        else if (per_family) why = "--expected-events needs one fitted model: -b is not supported with it";
        if (why) { std::fprintf(stderr, "cafexp_hip: %s\n", why); return 1; }
    }
    if (do_leaf_predictive) {
        const char* why = nullptr;
        if (gpus_given) why = "--leaf-predictive runs on one GPU: --gpus is not supported with it";
        else if (per_family) why = "--leaf-predictive needs one fitted model: -b is not supported with it";
        if (why) { std::fprintf(stderr, "cafexp_hip: %s\n", why); return 1; }
    }
    if (do_branch_change) {
        const char* why = nullptr;
        if (gpus_given) why = "--branch-change runs on one GPU: --gpus is not supported with it";
        else if (per_family) why = "--branch-change needs one fitted model: -b is not supported with it";
        else if (branch_change_band < 0) why = "--branch-change: D must not be negative";
        else if (!(test_pvalue > 0 && test_pvalue < 1)) why = "--branch-change: PVALUE (-P) must lie in (0, 1)";
        if (why) { std::fprintf(stderr, "cafexp_hip: %s\n", why); return 1; }
    }
    if (estimate_rootdist) {
        const char* why = nullptr;
        if (gpus_given) why = "--estimate-rootdist runs on one GPU: --gpus is not supported with it";
        else if (per_family) why = "--estimate-rootdist needs one fitted model: -b is not supported with it";
        else if (rootdist_rounds < 0) why = "--estimate-rootdist: ROUNDS must not be negative";
        if (why) { std::fprintf(stderr, "cafexp_hip: %s\n", why); return 1; }
    }
    if (do_histories) {
        const char* why = nullptr;
        if (gpus_given) why = "--sample-histories runs on one GPU: --gpus is not supported with it";
        else if (per_family) why = "--sample-histories needs one fitted model: -b is not supported with it";
        else if (history_draws < 1 || history_draws > 65536) why = "--sample-histories: N must lie in 1..65536";
        else if (!(marginal_level > 0 && marginal_level < 1)) why = "--sample-histories: LEVEL must lie in (0, 1)";
        if (why) { std::fprintf(stderr, "cafexp_hip: %s\n", why); return 1; }
        if (!have_history_seed && have_seed) history_seed = seed;
    }
    if (per_family) {                                            // what -b cannot be combined with: refused before anything is read or written
        const char* why = nullptr;
        if (k > 1 || alpha_given) why = "-b estimates one lambda per family under the base model; -k > 1 and -a are not supported with it";
        else if (use_err && err_path.empty()) why = "-b with -e needs an error model file: estimating epsilon per family is not supported";
        else if (gpus_given) why = "-b runs on one GPU: --gpus is not supported with it";
        if (why) { std::fprintf(stderr, "cafexp_hip: %s\n", why); return 1; }
        if (fixed_lambda > 0 || !multi.empty()) {                // execute.cpp:116 clears the lambda before every family's search
            std::fprintf(stderr, "cafexp_hip: -b estimates every lambda; -l / -m are ignored\n");
            fixed_lambda = 0; multi.clear();
        }
    }
    if (have_seed) randomizer_engine.seed(seed);
    try {
        user_data d;
        d.p_tree.reset(parse_newick(slurp_first_line(tree_path), false));
        {
            std::ifstream f(fam_path);
            if (!f.is_open()) throw std::runtime_error(fam_path + ": Failed to open. Exiting...");
            const std::set<std::string> tokens = parse_missing_tokens(missing_list);
            read_gene_families(f, d.p_tree.get(), d.gene_families, missing_list.empty() ? nullptr : &tokens);
        }
        if (!mask_path.empty()) {
            std::ifstream f(mask_path);
            if (!f.is_open()) throw std::runtime_error("Failed to open " + mask_path + ". Exiting...");
            mask_cells(f, d.gene_families);
        }
        compute_max_sizes(d.gene_families, d.max_family_size, d.max_root_family_size);
        if (force_m > 0) { d.max_family_size = force_m; d.max_root_family_size = force_r; }
        if (!err_path.empty()) {
            std::ifstream f(err_path);
            if (!f.is_open()) throw std::runtime_error("Failed to open " + err_path + ". Exiting...");
            d.p_error_model.reset(new error_model);
            read_error_model_file(f, d.p_error_model.get());
        }
        if (!lambda_tree_path.empty()) {
            d.p_lambda_tree.reset(parse_newick(slurp_first_line(lambda_tree_path), true));
            d.p_tree->validate_lambda_tree(d.p_lambda_tree.get());
        }
        if (fixed_lambda > 0) d.p_lambda.reset(new single_lambda(fixed_lambda));
        if (!multi.empty()) {
            std::vector<double> v;
            std::stringstream ss(multi);
            std::string tok;
            while (std::getline(ss, tok, ',')) v.push_back(std::stod(tok));
            d.p_lambda.reset(new multiple_lambda(d.p_lambda_tree->get_lambda_index_map(), v));
        }
        if (!rootdist_path.empty()) {
            std::ifstream f(rootdist_path);
            if (!f.is_open()) throw std::runtime_error("Failed to open file '" + rootdist_path + "'");
            read_rootdist(f, d.rootdist);
        }
        if (!keep_all) {                                          // cafexp.cpp:189-199
            auto rem = std::remove_if(d.gene_families.begin(), d.gene_families.end(), [&](const gene_family& f) { return !f.exists_at_root(d.p_tree.get()); });
            d.gene_families.erase(rem, d.gene_families.end());
        }
        if (limit >= 0 && (size_t)limit < d.gene_families.size()) d.gene_families.resize(limit);
        if (!rootdist_probs.empty()) {
            std::ifstream f(rootdist_probs);
            if (!f.is_open()) throw std::runtime_error("Failed to open file '" + rootdist_probs + "'");
            d.p_prior.reset(new file_probability_distribution(read_rootdist_probabilities(f)));
        }
        else if (use_poisson && poisson > 0) d.p_prior.reset(new poisson_distribution(poisson));
        else if (use_poisson) d.p_prior.reset(new poisson_distribution(&d.gene_families));     // fitted to the leaf sizes (root_equilibrium_distribution.cpp:34)
        else d.p_prior.reset(new uniform_distribution());

        // build_models (core.cpp:16-50): gamma iff fixed_alpha > 0 or K > 1; default error model for -e without a file
        std::unique_ptr<error_model> default_em;
        error_model* em = d.p_error_model.get();
        std::unique_ptr<hip_model_base> mdl;
        lambda* start_lambda = d.p_lambda.get();
        if (fixed_alpha > 0 || k > 1) {
            auto g = new hip_gamma_model(start_lambda, d.p_tree.get(), &d.gene_families, d.max_family_size, d.max_root_family_size, k, fixed_alpha, em);
            mdl.reset(g);
        } else {
            if (use_err && !em) {
                default_em.reset(new error_model());
                default_em->set_probabilities(0, {0, .95, 0.05});
                default_em->set_probabilities(d.max_family_size, {0.05, .9, 0.05});
                em = default_em.get();
            }
            mdl.reset(new hip_base_model(start_lambda, d.p_tree.get(), &d.gene_families, d.max_family_size, d.max_root_family_size, em));
        }
        mdl->set_device(device);
        mdl->set_search_batch(search_batch);                     // contexts with room for G x K categories
        mdl->set_root_rule(root_sum ? CAFE_ROOT_SUM : CAFE_ROOT_MAX);
        file_probability_distribution* em_prior = nullptr;
        if (estimate_rootdist) {                                 // the starting prior as the floats a call reads, held where the rounds can replace it
            root_distribution rd;
            if (!d.rootdist.empty()) rd.vectorize(d.rootdist);
            else rd.vectorize_uniform(d.max_root_family_size);
            d.p_prior->initialize(&rd);
            std::vector<double> p((size_t)d.max_root_family_size);
            for (size_t j = 0; j < p.size(); ++j) p[j] = d.p_prior->compute(j);
            em_prior = new file_probability_distribution(p);
            d.p_prior.reset(em_prior);
        }
        if (!mu_list.empty()) {                                  // fixed death rates: one per lambda of the -y tree (one without)
            const std::vector<double> mus = parse_rates(mu_list);
            size_t n_lambdas = 1;
            if (d.p_lambda_tree) {
                std::set<int> uniq;
                d.p_lambda_tree->apply_prefix_order([&](const clade* c) { uniq.insert(c->get_lambda_index()); });
                n_lambdas = uniq.size();
            }
            if (mus.size() != n_lambdas) throw std::runtime_error("--mu needs one death rate per lambda (" + std::to_string(n_lambdas) + ")");
            mdl->set_death_rates(mus);
        }
        if (gain_run) {                                          // gain_model.cpp: the table's rates under a gene gain rate
            hip_base_model* base = static_cast<hip_base_model*>(mdl.get());      // -k / -a were refused above
            base->set_workspace_limit(sim_workspace);
            base->set_root_rule(CAFE_ROOT_SUM);                  // the absent profile's value is a probability under the sum rule only
            base->initialize_lambda(d.p_lambda_tree.get());
            std::unique_ptr<lambda> shape(base->get_lambda());
            const int L = shape->count();
            gain_options go;
            go.estimate_nu = gain.estimate_gain; go.fixed_nu = gain.nu; go.root_absent = gain.root_absent; go.conditional = !gain.unconditional;
            go.estimate_mu = estimate_mu; go.max_iterations = max_iter;
            if (fixed_lambda > 0) go.fixed_lambdas.assign(1, fixed_lambda);
            if (!multi.empty()) go.fixed_lambdas = parse_rates(multi);
            if (!mu_list.empty()) go.fixed_mus = parse_rates(mu_list);
            const gain_table table = gain_distinct_families(d.gene_families);
            const std::set<double> lengths = d.p_tree->get_branch_lengths();
            lambda_optimizer starts(shape.get(), base, d.p_prior.get(), *std::max_element(lengths.begin(), lengths.end()), d.rootdist);
            const gain_scorer score = [&](const std::vector<double>& lambdas, const std::vector<double>& mus, double nu) {
                const size_t n = table.family.size();
                std::vector<double> lam, mu, nus(n * L, nu);
                for (size_t i = 0; i < n; ++i) { lam.insert(lam.end(), lambdas.begin(), lambdas.end()); mu.insert(mu.end(), mus.begin(), mus.end()); }
                return base->per_family_gain_lnl(d.p_prior.get(), d.rootdist, table.family, lam, mu, nus, go.root_absent);
            };
            const auto t0 = std::chrono::steady_clock::now();
            const gain_result res = fit_gain_model(score, table, L, go, [&] { return starts.initial_guesses(); });
            const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (out_dir.empty()) out_dir = "results";
            if (::mkdir(out_dir.c_str(), 0777) != 0 && errno != EEXIST) throw std::runtime_error("Failed to create directory " + out_dir);
            {
                std::ofstream f(out_dir + "/Gain_results.txt");
                write_gain_results(f, res, go, table);
                if (!f) throw std::runtime_error("Failed to write " + out_dir + "/Gain_results.txt");
                std::map<std::string, size_t> entry_of;          // the table's distinct entry of every family, by its counts
                std::ofstream g(out_dir + "/Gain_family_likelihoods.txt");
                g << "#FamilyID\tLikelihood of Family (lnL)\n" << std::setprecision(17);
                for (size_t i = 0, e = 0; i < d.gene_families.size(); ++i) {
                    std::string key;
                    for (const std::string& sp : d.gene_families[i].get_species()) key += sp + ':' + std::to_string(d.gene_families[i].get_species_size(sp)) + ',';
                    const auto it = entry_of.emplace(key, e);
                    if (it.second) ++e;
                    g << d.gene_families[i].id() << '\t' << res.with.lnl[it.first->second] << "\n";
                }
                g << "(absent)\t" << res.with.lnl.back() << "\n";
                if (!g) throw std::runtime_error("Failed to write " + out_dir + "/Gain_family_likelihoods.txt");
            }
            double posterior_s = 0;
            gain_branch_origins origins;
            if (gain.posterior) {                                // gain_origins.cpp: one call at the fitted rates over every distinct family
                const auto p0 = std::chrono::steady_clock::now();
                cladevector order;
                d.p_tree->apply_reverse_level_order([&order](const clade* c) { order.push_back(c); });
                const size_t n = table.family.size();
                std::vector<double> lam, mu, nus(n * L, res.with.nu);
                for (size_t i = 0; i < n; ++i) { lam.insert(lam.end(), res.with.lambdas.begin(), res.with.lambdas.end()); mu.insert(mu.end(), res.with.mus.begin(), res.with.mus.end()); }
                const gain_origins go_res = base->gain_posterior(d.p_prior.get(), d.rootdist, table.family, lam, mu, nus, go.root_absent, order);
                std::vector<std::string> names, ids;
                size_t root = 0;
                for (size_t v = 0; v < order.size(); ++v) { names.push_back(clade_index_or_name(order[v], order)); if (order[v]->is_root()) root = v; }
                std::map<std::string, size_t> entry_by_counts;
                std::vector<size_t> entry_of;
                for (size_t i = 0, e = 0; i < d.gene_families.size(); ++i) {
                    std::string key;
                    for (const std::string& sp : d.gene_families[i].get_species()) key += sp + ':' + std::to_string(d.gene_families[i].get_species_size(sp)) + ',';
                    const auto it = entry_by_counts.emplace(key, e);
                    if (it.second) ++e;
                    entry_of.push_back(it.first->second);
                    ids.push_back(d.gene_families[i].id());
                }
                origins = gain_origin_totals(go_res, table.weight, root);
                std::ofstream cells(out_dir + "/Gain_origins.tab"), totals(out_dir + "/Gain_branch_origins.tab");
                write_gain_origins(cells, go_res, names, root, ids, entry_of);
                write_gain_branch_origins(totals, origins, names, root);
                if (!cells || !totals) throw std::runtime_error("Failed to write " + out_dir + "/Gain_origins.tab or Gain_branch_origins.tab");
                posterior_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - p0).count();
            }
            base->set_lambda(nullptr);                           // `shape` goes with this scope
            auto list = [](const char* name, const std::vector<double>& v) {
                std::printf("\"%s\": [", name);
                for (size_t i = 0; i < v.size(); ++i) std::printf("%s%.17g", i ? ", " : "", v[i]);
                std::printf("], ");
            };
            std::printf("{\"model\": \"Gain\", \"root_rule\": \"sum\", \"conditional\": %s, \"families\": %zu, \"distinct_families\": %zu, ",
                        go.conditional ? "true" : "false", d.gene_families.size(), table.family.size() - 1);
            std::printf("\"neg_lnl\": %.17g, ", res.with.neg_lnl);
            list("lambda", res.with.lambdas); list("mu", res.with.mus);
            std::printf("\"nu\": %.17g, \"root_absent\": %.17g, \"p_absent\": %.17g, \"neg_lnl_without_gain\": %.17g, ", res.with.nu, go.root_absent, res.with.p_absent,
                        res.without.neg_lnl);
            list("lambda_without_gain", res.without.lambdas); list("mu_without_gain", res.without.mus);
            list("start_without_gain", res.without.start); list("start", res.with.start);
            if (gain.posterior) {
                double originated = 0, lost = 0;
                for (double v : origins.originated) originated += v;
                for (double v : origins.lost) lost += v;
                std::printf("\"gain_posterior_seconds\": %.3f, \"expected_origins\": %.12g, \"expected_losses\": %.12g, \"absent_at_root\": %.12g, "
                            "\"families_with_a_likely_origin\": %.12g, ", posterior_s, originated, lost, origins.absent_at_root, origins.origin_somewhere);
            }
            std::printf("\"lr_statistic\": %.17g, \"calls\": %d, \"max_family_size\": %d, \"max_root_family_size\": %d, \"seconds\": %.3f}\n", res.lr_statistic,
                        res.without.calls + res.with.calls, d.max_family_size, d.max_root_family_size, seconds);
            return 0;
        }
        if (per_family) {                                        // estimator::estimate_lambda_per_family (execute.cpp:104-128, :136-141)
            hip_base_model* base = static_cast<hip_base_model*>(mdl.get());      // -k / -a were refused above
            base->set_workspace_limit(sim_workspace);
            const auto t0 = std::chrono::steady_clock::now();
            per_family_mu fmu;
            if (family_mu == "estimate") fmu.mode = per_family_mu::ESTIMATE;
            else if (!family_mu.empty()) { fmu.mode = per_family_mu::FIXED; fmu.fixed = parse_rates(family_mu); }
            const per_family_result res = estimate_lambda_per_family(*base, d, max_iter, fmu);
            const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (out_dir.empty()) out_dir = "results";
            if (::mkdir(out_dir.c_str(), 0777) != 0 && errno != EEXIST) throw std::runtime_error("Failed to create directory " + out_dir);
            {
                std::ofstream f(out_dir + "/" + mdl->name() + "_lambda_per_family.txt");
                std::unique_ptr<lambda> shape(d.p_lambda_tree ? (lambda*)new multiple_lambda(d.p_lambda_tree->get_lambda_index_map(), res.lambdas.empty() ? std::vector<double>() : res.lambdas[0])
                                                              : (lambda*)new single_lambda(0.0));
                for (size_t i = 0; i < d.gene_families.size(); ++i) {
                    shape->update(res.lambdas[i].data());
                    f << d.gene_families[i].id() << '\t' << shape->to_string() << "\n";
                }
                if (!f) throw std::runtime_error("Failed to write " + out_dir + "/" + mdl->name() + "_lambda_per_family.txt");
                if (fmu.mode != per_family_mu::NONE) {           // the death rates, in the same shape and format
                    std::ofstream g(out_dir + "/" + mdl->name() + "_mu_per_family.txt");
                    for (size_t i = 0; i < d.gene_families.size(); ++i) {
                        shape->update(res.mus[i].data());
                        g << d.gene_families[i].id() << '\t' << shape->to_string() << "\n";
                    }
                    if (!g) throw std::runtime_error("Failed to write " + out_dir + "/" + mdl->name() + "_mu_per_family.txt");
                }
            }
            std::printf("{\"model\": \"%s\", \"mode\": \"lambda_per_family\", \"families\": %zu, \"distinct_families\": %zu, \"rounds\": %d, \"evaluations\": %ld, \"restarts\": %ld, "
                        "\"max_family_size\": %d, \"max_root_family_size\": %d, ", mdl->name().c_str(), d.gene_families.size(), res.distinct_families, res.rounds,
                        res.evaluations, res.restarts, d.max_family_size, d.max_root_family_size);
            if (auto pd = dynamic_cast<poisson_distribution*>(d.p_prior.get())) print_num("poisson_lambda", pd->poisson_lambda());
            if (fmu.mode != per_family_mu::NONE) std::printf("\"family_mu\": \"%s\", ", fmu.mode == per_family_mu::FIXED ? "fixed" : "estimate");
            std::printf("\"seconds\": %.3f}\n", seconds);
            return 0;
        }
        if (n_gpus > 1) {
            std::vector<int> devs(n_gpus);
            for (int g = 0; g < n_gpus; ++g) devs[g] = g;
            mdl->set_devices(devs);
        }

        std::unique_ptr<inference_optimizer_scorer> scorer(mdl->get_lambda_optimizer(d));
        if (estimate_mu)                                         // lambda is searched (-l / -m were refused), so the scorer leads with the lambdas
            scorer.reset(new lambda_mu_optimizer(scorer.release(), mdl->get_lambda(), mdl.get(), d.p_prior.get(), d.rootdist));
        std::unique_ptr<lambda> owned_lambda;
        optimizer_result opt;
        double search_s = 0;
        if (scorer) {                                            // estimate_missing_variables (execute.cpp:78)
            if (!d.p_lambda) owned_lambda.reset(mdl->get_lambda());
            if (search_batch > 1 && !scorer->batchable())
                std::cout << "--search-batch: the error model is estimated (one error table per point): the look-ahead points are scored one call each" << std::endl;
            optimizer o(scorer.get());
            o.max_iterations = max_iter;
            o.batch = search_batch;
            auto t0 = std::chrono::steady_clock::now();
            opt = o.optimize();
            search_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            scorer->finalize(opt.values.data());
        }
        // EM rounds on the root distribution: the E step is one cafe_root_posterior call at the optimum, the M step total / n_used
        struct em_round { double neg_lnl; std::string rates; };
        std::vector<em_round> em_rounds;
        if (estimate_rootdist) {
            auto rates_now = [&] {
                std::string r = "Lambda: " + mdl->get_lambda()->to_string();
                if (!mdl->death_rates().empty()) r += " Mu: " + mdl->death_rates_to_string();
                if (auto gm = dynamic_cast<hip_gamma_model*>(mdl.get())) { std::ostringstream o; o.precision(14); o << " Alpha: " << gm->get_alpha(); r += o.str(); }
                return r;
            };
            double prev = scorer ? opt.score : mdl->infer_family_likelihoods(d.p_prior.get(), d.rootdist, mdl->get_lambda());
            em_rounds.push_back({prev, rates_now()});
            for (int round = 1; round <= rootdist_rounds; ++round) {
                const root_posterior_result rp = mdl->root_posterior(d.p_prior.get(), d.rootdist);
                if (rp.n_used < 1) throw std::runtime_error("--estimate-rootdist: every family failed (zero likelihood) at the current optimum");
                std::vector<double> p(rp.total.size());
                for (size_t j = 0; j < p.size(); ++j) p[j] = (double)(float)(rp.total[j] / (double)rp.n_used);      // the float the ABI takes
                em_prior->set(p);
                double cur;
                if (scorer) {
                    optimizer o(scorer.get());
                    o.max_iterations = max_iter;
                    o.batch = search_batch;
                    o.start = opt.values;
                    auto t0 = std::chrono::steady_clock::now();
                    optimizer_result again = o.optimize();
                    search_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                    scorer->finalize(again.values.data());
                    opt.values = again.values; opt.score = again.score;
                    opt.num_iterations += again.num_iterations; opt.num_scorer_calls += again.num_scorer_calls;
                    opt.num_batches += again.num_batches; opt.num_points_scored += again.num_points_scored;
                    cur = again.score;
                } else {
                    cur = mdl->infer_family_likelihoods(d.p_prior.get(), d.rootdist, mdl->get_lambda());
                }
                em_rounds.push_back({cur, rates_now()});
                const bool settled = prev - cur < optimizer(nullptr).similarity_precision * std::fabs(prev);
                prev = cur;
                if (settled) break;
            }
        }
        double score = 0, best = 1e300;
        for (int r = 0; r < reps; ++r) {                         // compute (execute.cpp:42)
            auto t0 = std::chrono::steady_clock::now();
            score = mdl->infer_family_likelihoods(d.p_prior.get(), d.rootdist, mdl->get_lambda());
            best = std::min(best, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        }
        if (!family_out.empty()) {
            std::ofstream f(family_out);
            f.precision(17);
            mdl->write_family_likelihoods(f);
        }
        if (estimate_rootdist) {                                 // its files, the results file's rounds among them, default to results/
            if (out_dir.empty()) out_dir = "results";
            if (::mkdir(out_dir.c_str(), 0777) != 0 && errno != EEXIST) throw std::runtime_error("Failed to create directory " + out_dir);
        }
        if (!out_dir.empty()) {                                  // the two files of estimator::compute (execute.cpp:49-54)
            std::ofstream rf(out_dir + "/" + mdl->name() + "_results.txt");
            mdl->write_vital_statistics(rf, score);
            const missing_summary ms = count_missing(d.gene_families);
            if (ms.cells > 0) rf << "Missing cells: " << ms.cells << " in " << ms.families << " families (summed out)" << std::endl;
            rf.precision(17);
            for (size_t r = 0; r < em_rounds.size(); ++r)
                rf << "Root distribution round " << r << ": -lnL " << em_rounds[r].neg_lnl << " " << em_rounds[r].rates << std::endl;
            std::ofstream lf(out_dir + "/" + mdl->name() + "_family_likelihoods.txt");
            mdl->write_family_likelihoods(lf);
            if (use_err) {                                       // write_error_model_if_specified (execute.cpp:24-40)
                std::ofstream ef(out_dir + "/" + mdl->name() + "_error_model.txt");
                if (em) write_error_model_file(ef, *em);
                else {                                           // model::write_error_model's stand-in (core.cpp:118-127)
                    error_model none;
                    none.set_probabilities(d.max_family_size, {0, 1, 0});
                    write_error_model_file(ef, none);
                }
            }
        }
        if (estimate_rootdist) {
            std::ofstream f(out_dir + "/" + mdl->name() + "_root_distribution.txt");
            write_rootdist_probabilities(f, em_prior->probabilities());
            if (!f) throw std::runtime_error("Failed to write " + out_dir + "/" + mdl->name() + "_root_distribution.txt");
        }
        // the posterior probability of every rate category per family, under the rule that was searched
        if (root_sum && dynamic_cast<hip_gamma_model*>(mdl.get())) {
            const root_posterior_result rp = mdl->root_posterior(d.p_prior.get(), d.rootdist);
            const std::string dir = out_dir.empty() ? "results" : out_dir;
            if (::mkdir(dir.c_str(), 0777) != 0 && errno != EEXIST) throw std::runtime_error("Failed to create directory " + dir);
            std::ofstream f(dir + "/" + mdl->name() + "_category_posterior.tab");
            f.precision(17);
            f << "#FamilyID";
            for (double m : dynamic_cast<hip_gamma_model*>(mdl.get())->get_lambda_multipliers()) f << '\t' << m;
            f << '\n';
            for (size_t i = 0; i < d.gene_families.size(); ++i) {
                f << d.gene_families[i].id();
                for (size_t c = 0; c < rp.n_categories; ++c) f << '\t' << rp.category_posterior[i * rp.n_categories + c];
                f << '\n';
            }
            if (!f) throw std::runtime_error("Failed to write " + dir + "/" + mdl->name() + "_category_posterior.tab");
        }
        // compute_pvalues with the model's plain lambda (execute.cpp:153-161); 1000 simulations in the reference
        std::vector<double> pvalues;
        double pvalue_s = 0;
        if (pvalue_sims > 0) {
            pvalue_work work;
            auto t0 = std::chrono::steady_clock::now();
            if (pvalues_on_device)      // simulation on the GPU too: same distribution, another random sample (cafe_pvalues)
                pvalues = mdl->device_pvalues(pvalue_sims, have_seed ? seed : 1u);
            else
                pvalues = compute_pvalues(d.p_tree.get(), d.gene_families, mdl->get_lambda(), pvalue_sims, d.max_family_size, d.max_root_family_size,
                                          device, &work, &mdl->death_rates());
            pvalue_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (!pvalues_out.empty()) {
                std::ofstream f(pvalues_out);
                f.precision(17);
                f << "#FamilyID\tpvalue\tobserved max likelihood\n";
                for (size_t i = 0; i < pvalues.size(); ++i)
                    f << d.gene_families[i].id() << '\t' << pvalues[i] << '\t'
                      << (work.observed_max_likelihood.empty() ? 0.0 : work.observed_max_likelihood[i]) << '\n';
            }
            if (!pvalues_cond.empty()) {                         // FILE:K -> the first K sorted conditional distributions, one per line
                const size_t colon = pvalues_cond.rfind(':');
                const size_t kdump = std::min<size_t>(work.conditional_distribution.size(), std::stoul(pvalues_cond.substr(colon + 1)));
                std::ofstream f(pvalues_cond.substr(0, colon));
                f.precision(17);
                for (size_t i = 0; i < kdump; ++i) {
                    for (size_t j = 0; j < work.conditional_distribution[i].size(); ++j) f << (j ? "\t" : "") << work.conditional_distribution[i][j];
                    f << '\n';
                }
            }
        }
        // reconstruct_ancestral_states, Viterbi branch probabilities of the significant families, reports (execute.cpp:163-180)
        double reconstruct_s = 0;
        size_t n_with_probs = 0;
        if (do_reconstruct) {
            if (pvalues.empty()) pvalues.assign(d.gene_families.size(), 1.0);
            auto t0 = std::chrono::steady_clock::now();
            std::unique_ptr<reconstruction> rec(mdl->reconstruct_ancestral_states(d.gene_families, d.p_prior.get()));
            cladevector order;
            d.p_tree->apply_reverse_level_order([&order](const clade* c) { order.push_back(c); });
            branch_probabilities probs = compute_branch_probabilities(*mdl, *rec, d.gene_families, pvalues, test_pvalue, order);
            reconstruct_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            for (const auto& gf : d.gene_families) n_with_probs += probs.contains(gf);
            if (!out_dir.empty()) rec->write_results(mdl->name(), out_dir, d.p_tree.get(), d.gene_families, pvalues, test_pvalue, probs);
        }
        // marginal reconstruction with the model's final parameters and prior: independent of --reconstruct
        double marginal_s = 0;
        size_t marginal_failed = 0;
        if (do_marginal) {
            auto t0 = std::chrono::steady_clock::now();
            cladevector order;
            d.p_tree->apply_reverse_level_order([&order](const clade* c) { order.push_back(c); });
            const marginal_result mr = mdl->marginal_reconstruction(d.p_prior.get(), d.rootdist, marginal_level, order);
            marginal_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            marginal_failed = mr.failed_count();
            if (!out_dir.empty()) write_marginal_reports(mr, mdl->name(), out_dir, order, d.gene_families);
        }
        // histories drawn from the same posterior, counted per draw: independent of the two reconstructions
        double history_s = 0;
        size_t history_failed = 0;
        if (do_histories) {
            auto t0 = std::chrono::steady_clock::now();
            cladevector order;
            d.p_tree->apply_reverse_level_order([&order](const clade* c) { order.push_back(c); });
            const history_result hr = mdl->sample_histories(d.p_prior.get(), d.rootdist, history_draws, history_seed, order);
            history_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            history_failed = hr.failed_count();
            if (!out_dir.empty()) write_history_reports(hr, marginal_level, mdl->name(), out_dir, order);
        }
        // expected gains and losses per branch under the same model: what the node sizes of the reconstructions do not show
        double events_s = 0;
        size_t events_failed = 0;
        if (do_events) {
            auto t0 = std::chrono::steady_clock::now();
            cladevector order;
            d.p_tree->apply_reverse_level_order([&order](const clade* c) { order.push_back(c); });
            const events_result er = mdl->expected_events(d.p_prior.get(), d.rootdist, order);
            events_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            events_failed = er.failed_count();
            if (!out_dir.empty()) write_events_reports(er, mdl->name(), out_dir, order, d.gene_families);
        }
        // the leave-one-out predictive check of every leaf count under the same model: which cells of the table are surprising
        double predictive_s = 0;
        leaf_predictive_summary predictive;
        if (do_leaf_predictive) {
            auto t0 = std::chrono::steady_clock::now();
            const leaf_predictive_result lp = mdl->leaf_predictive(d.p_prior.get(), d.rootdist);
            const std::string dir = out_dir.empty() ? "results" : out_dir;
            if (::mkdir(dir.c_str(), 0777) != 0 && errno != EEXIST) throw std::runtime_error("Failed to create directory " + dir);
            predictive = write_leaf_predictive_reports(lp, test_pvalue, mdl->name(), dir, d.gene_families);
            if (count_missing(d.gene_families).cells > 0) write_imputed_counts(lp, mdl->name(), dir, d.gene_families);
            predictive_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        // the posterior of every branch's size change under the same model: by how much, and how sure
        double change_s = 0;
        size_t change_failed = 0, change_clipped = 0;
        if (do_branch_change) {
            auto t0 = std::chrono::steady_clock::now();
            cladevector order;
            d.p_tree->apply_reverse_level_order([&order](const clade* c) { order.push_back(c); });
            const int band = std::min(branch_change_band, std::max(d.max_family_size, d.max_root_family_size));      // no change is larger
            const branch_change_result bc = mdl->branch_change(d.p_prior.get(), d.rootdist, band, 1.0 - test_pvalue, order);
            const std::string dir = out_dir.empty() ? "results" : out_dir;
            if (::mkdir(dir.c_str(), 0777) != 0 && errno != EEXIST) throw std::runtime_error("Failed to create directory " + dir);
            std::vector<std::string> ids;
            for (const auto& gf : d.gene_families) ids.push_back(gf.id());
            change_clipped = write_branch_change_reports(bc, mdl->name(), dir, ids);
            change_failed = bc.failed_count();
            change_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        // standard errors of what the search estimated, from the per-family scores of the searched objective at the optimum
        standard_errors se;
        std::vector<double> slopes;
        // what the search estimated (both --standard-errors and --rate-shift-scan condition on the rest)
        auto g = dynamic_cast<hip_gamma_model*>(mdl.get());
        const bool lambda_searched = scorer && !d.p_lambda, alpha_searched = scorer && g && !(fixed_alpha > 0);
        if ((do_standard_errors || do_rate_shift) && alpha_searched) slopes = multiplier_slopes(g->get_lambda_multipliers().size(), g->get_alpha());
        if (do_standard_errors) {
            const gradient_result gr = mdl->score_gradient(d.p_prior.get(), d.rootdist, root_sum ? CAFE_ROOT_SUM : CAFE_ROOT_MAX);
            const std::vector<double> lv = mdl->get_lambda()->values();
            const size_t nl = gr.n_lambdas, F = d.gene_families.size();
            std::vector<std::string> names;
            std::vector<double> est;
            auto rate_name = [&](const char* what, size_t i) { return nl == 1 ? std::string(what) : what + std::to_string(i + 1); };
            if (lambda_searched) for (size_t i = 0; i < nl; ++i) { names.push_back(rate_name("Lambda", i)); est.push_back(lv[i]); }
            if (estimate_mu) for (size_t i = 0; i < nl; ++i) { names.push_back(rate_name("Mu", i)); est.push_back(mdl->death_rates()[i]); }
            if (alpha_searched) { names.push_back("Alpha"); est.push_back(g->get_alpha()); }
            if (names.empty()) throw std::runtime_error("--standard-errors: no parameter was estimated (lambda, mu and alpha are all fixed)");
            const size_t P = names.size();
            std::vector<double> scores(F * P);
            for (size_t f = 0; f < F; ++f) {
                size_t at = f * P;
                if (lambda_searched) for (size_t i = 0; i < nl; ++i) scores[at++] = gr.d_lambda[f * nl + i];
                if (estimate_mu) for (size_t i = 0; i < nl; ++i) scores[at++] = gr.d_mu[f * nl + i];
                if (alpha_searched) {
                    double s = 0;
                    for (size_t c = 0; c < gr.n_categories; ++c) s += gr.d_multiplier[f * gr.n_categories + c] * slopes[c];
                    scores[at++] = s;
                }
            }
            se = compute_standard_errors(names, est, scores, F);
            if (!se.ok) std::fprintf(stderr, "cafexp_hip: warning: the information matrix of the scores is singular or ill-conditioned: no standard errors\n");
            std::string cond = em ? "the error model (epsilon is not differentiated)" : "the model as fitted";
            if (!lambda_searched) cond += ", the fixed lambda";
            if (!mdl->death_rates().empty() && !estimate_mu) cond += ", the fixed mu";
            if (g && !alpha_searched) cond += ", the fixed alpha";
            const std::string dir = out_dir.empty() ? "results" : out_dir;
            if (::mkdir(dir.c_str(), 0777) != 0 && errno != EEXIST) throw std::runtime_error("Failed to create directory " + dir);
            write_standard_errors(se, mdl->name(), dir, cond);
        }
        // score tests of a rate shift on every branch and clade, from the branch scores and their information at the optimum
        rate_shift_scan scan;
        double scan_s = 0;
        bool scan_tree = false;
        if (do_rate_shift) {
            auto t0 = std::chrono::steady_clock::now();
            cladevector order;
            d.p_tree->apply_reverse_level_order([&order](const clade* c) { order.push_back(c); });
            const branch_scores_result bs = mdl->branch_scores(d.p_prior.get(), d.rootdist, root_sum ? CAFE_ROOT_SUM : CAFE_ROOT_MAX, order);
            std::vector<std::vector<double>> theta;
            std::vector<std::string> names;
            auto rate_name = [&](const char* what, size_t i) { return bs.n_lambdas == 1 ? std::string(what) : what + std::to_string(i + 1); };
            auto unit = [&](size_t at) { std::vector<double> v(bs.P, 0.0); v[at] = 1.0; return v; };
            if (lambda_searched) for (size_t i = 0; i < bs.n_lambdas; ++i) { names.push_back(rate_name("Lambda", i)); theta.push_back(unit(bs.global(i))); }
            if (estimate_mu) for (size_t i = 0; i < bs.n_lambdas; ++i) { names.push_back(rate_name("Mu", i)); theta.push_back(unit(bs.global(bs.n_lambdas + i))); }
            if (alpha_searched) {
                std::vector<double> v(bs.P, 0.0);
                for (size_t c = 0; c < bs.n_categories; ++c) v[bs.global(bs.n_lambdas * bs.n_par + c)] = slopes[c];
                names.push_back("Alpha"); theta.push_back(v);
            }
            scan = compute_rate_shift_scan(bs, order, theta, names);
            const std::string dir = out_dir.empty() ? "results" : out_dir;
            if (::mkdir(dir.c_str(), 0777) != 0 && errno != EEXIST) throw std::runtime_error("Failed to create directory " + dir);
            write_rate_shift_scan(scan, mdl->name(), dir, order);
            scan_tree = scan.best >= 0 && scan.rows[(size_t)scan.best].subtree.holm < test_pvalue;
            if (scan_tree) write_rate_shift_lambda_tree(scan, d.p_tree.get(), mdl->name(), dir);
            else std::fprintf(stderr, "cafexp_hip: --rate-shift-scan: no rate shift passed the threshold %g (Holm-adjusted clade p)\n", test_pvalue);
            scan_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        std::printf("{\"model\": \"%s\", ", mdl->name().c_str());
        print_num("neg_lnl", score);
        if (root_sum) std::printf("\"root_rule\": \"sum\", ");
        std::printf("\"n_families\": %zu, \"max_family_size\": %d, \"max_root_family_size\": %d, \"seconds_per_call\": %.6f, ",
                    d.gene_families.size(), d.max_family_size, d.max_root_family_size, best);
        std::printf("\"lambda\": [");
        auto lv = mdl->get_lambda()->values();
        for (size_t i = 0; i < lv.size(); ++i) std::printf("%s%.17g", i ? ", " : "", lv[i]);
        std::printf("]");
        if (!mdl->death_rates().empty()) {
            std::printf(", \"mu\": [");
            for (size_t i = 0; i < mdl->death_rates().size(); ++i) std::printf("%s%.17g", i ? ", " : "", mdl->death_rates()[i]);
            std::printf("]");
        }
        if (auto g = dynamic_cast<hip_gamma_model*>(mdl.get())) {
            std::printf(", "); print_num("alpha", g->get_alpha(), false);
            std::printf(", \"multipliers\": [");
            auto mv = g->get_lambda_multipliers();
            for (size_t i = 0; i < mv.size(); ++i) std::printf("%s%.17g", i ? ", " : "", mv[i]);
            std::printf("]");
        }
        if (em) { std::printf(", "); print_num("epsilon", em->get_epsilons().back(), false); }
        if (scorer) {
            std::printf(", \"search\": {\"iterations\": %d, \"scorer_calls\": %d, \"seconds\": %.3f, ", opt.num_iterations, opt.num_scorer_calls, search_s);
            if (search_batch > 1) std::printf("\"batches\": %d, \"points_scored\": %d, ", opt.num_batches, opt.num_points_scored);
            print_num("score", opt.score, false);
            std::printf("}");
        }
        if (estimate_rootdist) {
            std::printf(", \"rootdist\": {\"rounds\": [");
            for (size_t r = 0; r < em_rounds.size(); ++r) {
                if (std::isfinite(em_rounds[r].neg_lnl)) std::printf("%s%.17g", r ? ", " : "", em_rounds[r].neg_lnl);
                else std::printf("%s\"inf\"", r ? ", " : "");
            }
            std::printf("], \"max_rounds\": %d}", rootdist_rounds);
        }
        if (pvalue_sims > 0) {
            size_t sig = 0;
            for (double p : pvalues) if (p < 0.05) ++sig;
            std::printf(", \"pvalues\": {\"simulations\": %d, \"seconds\": %.3f, \"significant_at_0.05\": %zu}", pvalue_sims, pvalue_s, sig);
        }
        if (do_reconstruct)
            std::printf(", \"reconstruct\": {\"seconds\": %.3f, \"families_with_branch_probabilities\": %zu}", reconstruct_s, n_with_probs);
        if (do_marginal)
            std::printf(", \"marginal\": {\"seconds\": %.3f, \"level\": %.17g, \"failed\": %zu}", marginal_s, marginal_level, marginal_failed);
        if (do_histories)
            std::printf(", \"histories\": {\"seconds\": %.3f, \"draws\": %d, \"failed\": %zu}", history_s, history_draws, history_failed);
        if (do_events)
            std::printf(", \"expected_events\": {\"seconds\": %.3f, \"failed\": %zu}", events_s, events_failed);
        if (do_branch_change)
            std::printf(", \"branch_change\": {\"seconds\": %.3f, \"max_change\": %d, \"level\": %.17g, \"failed\": %zu, \"clipped\": %zu}", change_s,
                        std::min(branch_change_band, std::max(d.max_family_size, d.max_root_family_size)), 1.0 - test_pvalue, change_failed, change_clipped);
        if (do_leaf_predictive) {
            std::printf(", \"leaf_predictive\": {\"seconds\": %.3f, \"failed_cells\": %zu, \"outliers\": %zu, ", predictive_s, predictive.failed_cells, predictive.outliers);
            print_num("log_pseudo_likelihood", predictive.log_pseudo_likelihood, false);
            std::printf("}");
        }
        if (do_standard_errors) {
            auto list = [](const char* key, const std::vector<double>& v) {
                std::printf("\"%s\": [", key);
                for (size_t i = 0; i < v.size(); ++i) {
                    if (std::isfinite(v[i])) std::printf("%s%.17g", i ? ", " : "", v[i]);
                    else std::printf("%s\"nan\"", i ? ", " : "");
                }
                std::printf("]");
            };
            std::printf(", \"standard_errors\": {\"parameters\": [");
            for (size_t i = 0; i < se.names.size(); ++i) std::printf("%s\"%s\"", i ? ", " : "", se.names[i].c_str());
            std::printf("], ");
            list("estimate", se.estimate); std::printf(", ");
            list("se", se.se); std::printf(", ");
            list("total_score", se.total_score); std::printf(", ");
            if (!slopes.empty()) { list("dmultiplier_dalpha", slopes); std::printf(", "); }
            std::printf("\"families\": %zu, \"left_out\": %zu}", se.families_used, se.families_left_out);
        }
        if (do_rate_shift) {
            std::printf(", \"rate_shift_scan\": {\"seconds\": %.3f, \"families\": %zu, \"left_out\": %zu, \"profiled\": [", scan_s, scan.families_used, scan.families_failed);
            for (size_t i = 0; i < scan.profiled.size(); ++i) std::printf("%s\"%s\"", i ? ", " : "", scan.profiled[i].c_str());
            std::printf("], \"dmultiplier_dalpha\": [");
            for (size_t i = 0; i < slopes.size(); ++i) std::printf("%s%.17g", i ? ", " : "", slopes[i]);
            std::printf("], \"threshold\": %.17g, \"lambda_tree_written\": %s, ", test_pvalue, scan_tree ? "true" : "false");
            print_num("smallest_clade_holm_p", scan.best >= 0 ? scan.rows[(size_t)scan.best].subtree.holm : NAN, false);
            std::printf("}");
        }
        std::printf("}\n");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "cafexp_hip: %s\n", e.what());
        return 1;
    }
    return 0;
}
