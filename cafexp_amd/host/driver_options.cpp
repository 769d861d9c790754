// The driver's command line: the options record, its parser, and the one function that says why a combination of options is
// refused.  Nothing here reads a file or touches the device, so host_tests checks every text and their order without a GPU.
#include <cstdio>
#include <sstream>

#include "cafe_host.h"

namespace cafe {

std::vector<double> parse_rates(const std::string& list) {
    std::vector<double> v;
    std::stringstream ss(list);
    std::string tok;
    while (std::getline(ss, tok, ',')) v.push_back(std::stod(tok));
    return v;
}

bool parse_options(int argc, char** argv, driver_options& o) {
    bool missing_value = false;
    for (int i = 1; i < argc && !missing_value; ++i) {
        const std::string a = argv[i];
        auto next = [&]() -> std::string { if (i + 1 >= argc) { missing_value = true; return "0"; } return argv[++i]; };
        auto optional = [&]() -> std::string { if (i + 1 < argc && argv[i + 1][0] != '-') return argv[++i]; return ""; };
        if (a == "-t") o.tree_path = next();
        else if (a == "-i") o.fam_path = next();
        else if (a == "-l") o.fixed_lambda = std::stod(next());
        else if (a == "-m") o.multi = next();
        else if (a == "-y") o.lambda_tree_path = next();
        else if (a == "-k") o.k = std::stoi(next());
        else if (a == "-a") { o.fixed_alpha = std::stod(next()); o.alpha_given = true; }
        else if (a == "-b") o.per_family = true;
        else if (a == "--mu") o.mu_list = next();
        else if (a == "--estimate-mu") o.estimate_mu = true;
        else if (a == "--family-mu") o.family_mu = next();
        else if (a == "--standard-errors") o.do_standard_errors = true;
        else if (a == "--expected-events") o.do_events = true;
        else if (a == "--rate-shift-scan") o.do_rate_shift = true;
        else if (a == "--leaf-predictive") o.do_leaf_predictive = true;
        else if (a == "--branch-change") { o.do_branch_change = true; std::string v = optional(); if (!v.empty()) o.branch_change_band = std::stoi(v); }
        else if (a == "--missing") o.missing_list = next();
        else if (a == "--mask-cells") o.mask_path = next();
        else if (a == "--root-sum") o.root_sum = true;
        else if (a == "--estimate-rootdist") { o.estimate_rootdist = o.root_sum = true; std::string v = optional(); if (!v.empty()) o.rootdist_rounds = std::stoi(v); }
        else if (a == "--rootdist-probs") o.rootdist_probs = next();
        else if (a == "-e") { o.use_err = true; o.err_path = optional(); }
        else if (a == "-p") { o.use_poisson = true; std::string v = optional(); o.poisson = v.empty() ? 0 : std::stod(v); }
        else if (a == "-f") o.rootdist_path = next();
        else if (a == "-z") o.keep_all = true;
        else if (a == "-s") { o.seed = (unsigned)std::stoul(next()); o.have_seed = true; }
        else if (a == "-I") o.max_iter = std::stoi(next());
        else if (a == "-d") o.device = std::stoi(next());
        else if (a == "--gpus") { o.n_gpus = std::stoi(next()); o.gpus_given = true; }
        else if (a == "--reps") o.reps = std::stoi(next());
        else if (a == "--family-out") o.family_out = next();
        else if (a == "-o") o.out_dir = next();
        else if (a == "--limit") o.limit = std::stol(next());
        else if (a == "--sizes") {                               // M,R instead of the data-derived maxima (tests)
            const std::string v = next();
            const size_t comma = v.find(',');
            if (!missing_value) { o.force_m = std::stoi(v.substr(0, comma)); o.force_r = std::stoi(v.substr(comma + 1)); }
        }
        else if (a == "--reconstruct") o.do_reconstruct = true;
        else if (a == "--reconstruct-marginal") { o.do_marginal = true; std::string v = optional(); if (!v.empty()) o.marginal_level = std::stod(v); }
        else if (a == "--sample-histories") { o.do_histories = true; o.history_draws = std::stoi(next()); }
        else if (a == "--sample-seed") { o.history_seed = std::stoull(next()); o.have_history_seed = true; }
        else if (a == "-P") o.test_pvalue = std::stod(next());
        else if (a == "--pvalues-device") o.pvalues_on_device = true;
        else if (a == "--pvalues") o.pvalue_sims = std::stoi(next());
        else if (a == "--pvalues-out") o.pvalues_out = next();
        else if (a == "--pvalues-cond") o.pvalues_cond = next();
        else if (a == "--simulate") { std::string v = optional(); o.simulate_n = v.empty() ? 0 : std::stoi(v); }
        else if (a == "--simulate-device") o.simulate_on_device = true;
        else if (a == "--workspace") o.sim_workspace = std::stoull(next());
        else if (a == "--search-batch") { o.search_batch = std::stoi(next()); o.search_batch_given = true; }
        else if (a == "--gain") { o.gain = true; o.gain_nu = std::stod(next()); }
        else if (a == "--estimate-gain") o.estimate_gain = true;
        else if (a == "--root-absent") { o.root_absent_given = true; o.root_absent = std::stod(next()); }
        else if (a == "--gain-unconditional") o.gain_unconditional = true;
        else if (a == "--gain-posterior") o.gain_posterior = true;
        else if (a == "--gain-dense") o.gain_dense = true;
        else if (a == "--gain-scaled") o.gain_scaled = true;
        else return false;
    }
    return !missing_value;
}

gain_request gain_request_of(const driver_options& o) {
    gain_request r;
    r.gain = o.gain; r.estimate_gain = o.estimate_gain; r.root_absent_given = o.root_absent_given; r.unconditional = o.gain_unconditional;
    r.posterior = o.gain_posterior; r.dense = o.gain_dense; r.scaled = o.gain_scaled; r.nu = o.gain_nu; r.root_absent = o.root_absent;
    r.gamma = o.k > 1 || o.alpha_given; r.per_family = o.per_family; r.gpus = o.gpus_given; r.simulate = o.simulate_n >= 0;
    r.pvalues = o.pvalue_sims > 0; r.reconstruct = o.do_reconstruct; r.marginal = o.do_marginal; r.histories = o.do_histories;
    r.standard_errors = o.do_standard_errors; r.events = o.do_events; r.rate_shift = o.do_rate_shift; r.leaf_predictive = o.do_leaf_predictive;
    r.branch_change = o.do_branch_change; r.rootdist_em = o.estimate_rootdist; r.search_batch = o.search_batch_given;
    r.estimate_error = o.use_err && o.err_path.empty();
    return r;
}

namespace {

const char* level_in_range(const driver_options& o, const char* why) { return o.marginal_level > 0 && o.marginal_level < 1 ? nullptr : why; }
const char* marginal_range(const driver_options& o) { return level_in_range(o, "--reconstruct-marginal: LEVEL must lie in (0, 1)"); }
const char* branch_change_range(const driver_options& o) {
    if (o.branch_change_band < 0) return "--branch-change: D must not be negative";
    if (!(o.test_pvalue > 0 && o.test_pvalue < 1)) return "--branch-change: PVALUE (-P) must lie in (0, 1)";
    return nullptr;
}
const char* rootdist_range(const driver_options& o) { return o.rootdist_rounds < 0 ? "--estimate-rootdist: ROUNDS must not be negative" : nullptr; }
const char* histories_range(const driver_options& o) {
    if (o.history_draws < 1 || o.history_draws > 65536) return "--sample-histories: N must lie in 1..65536";
    return level_in_range(o, "--sample-histories: LEVEL must lie in (0, 1)");
}

// The reports of one fitted model, in the order their refusals are tried.  simulate_rank: the report's place among the
// refusals of --simulate (which tries them in another order), 0 where --simulate ignores the flag.
struct report_row {
    bool driver_options::*flag;
    const char *not_with_gpus, *not_with_b, *not_with_simulate;
    int simulate_rank;
    const char* (*range)(const driver_options&);
};
#define REPORT_ROW(flag, spelling, simulate_rank, range)                                                                          \
    { &driver_options::flag, spelling " runs on one GPU: --gpus is not supported with it",                                       \
      spelling " needs one fitted model: -b is not supported with it",                                                           \
      spelling " belongs to a fitted model: --simulate is not supported with it", simulate_rank, range }
const report_row report_table[] = {
    REPORT_ROW(do_standard_errors, "--standard-errors", 1, nullptr),
    REPORT_ROW(do_rate_shift, "--rate-shift-scan", 3, nullptr),
    REPORT_ROW(do_marginal, "--reconstruct-marginal", 0, marginal_range),
    REPORT_ROW(do_events, "--expected-events", 2, nullptr),
    REPORT_ROW(do_leaf_predictive, "--leaf-predictive", 4, nullptr),
    REPORT_ROW(do_branch_change, "--branch-change", 5, branch_change_range),
    REPORT_ROW(estimate_rootdist, "--estimate-rootdist", 0, rootdist_range),
    REPORT_ROW(do_histories, "--sample-histories", 0, histories_range),
};
#undef REPORT_ROW
const char* const family_mu_without_b = "--family-mu sets the death rates of -b: it is not supported without -b";

const char* search_batch_refusal(const driver_options& o) {
    const int K = o.gamma() ? std::max(1, o.k) : 1;
    if (o.search_batch < 2) return "--search-batch: G must be at least 2";
    if ((long)o.search_batch * K > 32) return "--search-batch: G x K (the -k categories) must not exceed 32";
    if (o.n_gpus > 1) return "--search-batch scores its points in one call on one GPU: --gpus N > 1 is not supported with it";
    if (o.per_family) return "--search-batch drives the search of one fitted model: -b is not supported with it";
    if (o.simulate_n >= 0) return "--search-batch drives a search: --simulate is not supported with it";
    return nullptr;
}

const char* simulate_refusal(const driver_options& o) {
    if (o.tree_path.empty()) return driver_usage_exit;
    if (o.estimate_mu) return "--simulate draws under given rates: --estimate-mu is not supported with it (give --mu)";
    if (!o.family_mu.empty()) return family_mu_without_b;
    const report_row* first = nullptr;
    for (const report_row& r : report_table)
        if (o.*r.flag && r.simulate_rank && (!first || r.simulate_rank < first->simulate_rank)) first = &r;
    return first ? first->not_with_simulate : nullptr;
}

// unknown cells are summed out by the scorer, -b and --leaf-predictive only
const char* missing_cells_refusal(const driver_options& o) {
    if (!o.missing_list.empty() && parse_missing_tokens(o.missing_list).empty()) return "--missing: TOKENS must name at least one spelling, e.g. NA,?,-";
    if (o.pvalue_sims > 0) return "--pvalues simulates complete families: it is not supported on a table with missing cells (--missing / --mask-cells)";
    if (o.do_reconstruct) return "--reconstruct reads every leaf count: it is not supported on a table with missing cells (--missing / --mask-cells)";
    if (o.do_marginal && o.gain_run()) return "the gain model's --reconstruct-marginal summarises every leaf at its observed count: it is not supported with --missing / --mask-cells";
    if (o.do_marginal) return "--reconstruct-marginal is not ported to missing cells: it is not supported with --missing / --mask-cells";
    if (o.do_histories) return "--sample-histories is not ported to missing cells: it is not supported with --missing / --mask-cells";
    if (o.do_standard_errors) return "--standard-errors is not ported to missing cells: it is not supported with --missing / --mask-cells";
    if (o.do_events) return "--expected-events is not ported to missing cells: it is not supported with --missing / --mask-cells";
    if (o.do_rate_shift) return "--rate-shift-scan is not ported to missing cells: it is not supported with --missing / --mask-cells";
    if (o.do_branch_change) return "--branch-change is not ported to missing cells: it is not supported with --missing / --mask-cells";
    return nullptr;
}

const char* death_rate_refusal(const driver_options& o) {
    if (o.estimate_mu && !o.mu_list.empty()) return "--mu fixes the death rates and --estimate-mu searches them: give one of the two";
    if (o.per_family) return "-b runs the lambda = mu kernel: --mu / --estimate-mu are not supported with it";
    if (o.estimate_mu && (o.fixed_lambda > 0 || !o.multi.empty())) return "--estimate-mu searches lambda and mu together: -l / -m are not supported with it";
    return nullptr;
}

// what -b cannot be combined with
const char* per_family_refusal(const driver_options& o) {
    if (o.k > 1 || o.alpha_given) return "-b estimates one lambda per family under the base model; -k > 1 and -a are not supported with it";
    if (o.use_err && o.err_path.empty()) return "-b with -e needs an error model file: estimating epsilon per family is not supported";
    if (o.gpus_given) return "-b runs on one GPU: --gpus is not supported with it";
    return nullptr;
}

}  // namespace

const char* const driver_usage_exit = "usage";

const char* driver_refusal(const driver_options& o) {
    const char* why = gain_refusal(gain_request_of(o));
    if (!why && o.search_batch_given) why = search_batch_refusal(o);
    if (why) return why;
    if (o.simulate_n >= 0) return simulate_refusal(o);
    if (o.tree_path.empty() || o.fam_path.empty()) return driver_usage_exit;
    if (!o.missing_list.empty() || !o.mask_path.empty()) why = missing_cells_refusal(o);
    if (!why && (o.estimate_mu || !o.mu_list.empty())) why = death_rate_refusal(o);
    if (!why && !o.family_mu.empty() && !o.per_family) why = family_mu_without_b;
    for (const report_row& r : report_table) {
        if (why) break;
        if (!(o.*r.flag)) continue;
        if (o.gpus_given) why = r.not_with_gpus;
        else if (o.per_family) why = r.not_with_b;
        else if (r.range) why = r.range(o);
    }
    if (!why && o.per_family) why = per_family_refusal(o);
    return why;
}

void normalise_options(driver_options& o) {
    if (o.simulate_n < 0) {                                      // (the simulator has no histories and no -b)
        if (o.do_histories && !o.have_history_seed && o.have_seed) o.history_seed = o.seed;
        if (o.per_family && (o.fixed_lambda > 0 || !o.multi.empty())) {       // execute.cpp:116 clears the lambda before every family's search
            std::fprintf(stderr, "cafexp_hip: -b estimates every lambda; -l / -m are ignored\n");
            o.fixed_lambda = 0; o.multi.clear();
        }
    }
    if (o.have_seed) randomizer_engine.seed(o.seed);
}

}  // namespace cafe
