// cafexp_hip's modes: what runs between an accepted command line (driver_options.cpp) and the one JSON object on stdout.
//   load_inputs, build_model     the files and the model every mode starts from
//   run_simulation               --simulate
//   run_gain_model               --gain / --estimate-gain: the nested fit, then its report stages
//   run_lambda_per_family        -b
//   run_fitted_model             everything else: the search, the result files, then the report stages
// A report stage is a function that returns the record its JSON fragment needs; the record prints the fragment.  The stages run
// in a fixed order (several draw from randomizer_engine or call the device), and the fragments print in a fixed order.
#include <sys/stat.h>

#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <sstream>

#include "cafe_host.h"
#include "../../include/cafe_mi355x.h"

namespace cafe {
namespace {

typedef std::chrono::steady_clock::time_point time_point;
time_point now() { return std::chrono::steady_clock::now(); }
double seconds_since(time_point t0) { return std::chrono::duration<double>(now() - t0).count(); }

std::string slurp_first_line(const std::string& path) {
    std::ifstream f(path);
    if (!f.is_open()) throw std::runtime_error("Failed to open " + path);
    std::string line;
    std::getline(f, line);
    return line;
}

void print_num(const char* key, double v, bool comma = true) {
    if (std::isinf(v)) std::printf("\"%s\": \"%sinf\"%s", key, v < 0 ? "-" : "", comma ? ", " : "");
    else if (std::isnan(v)) std::printf("\"%s\": \"nan\"%s", key, comma ? ", " : "");
    else std::printf("\"%s\": %.17g%s", key, v, comma ? ", " : "");
}

// "key": [v, ..]after -- a non-finite entry as %.17g spells it, or (nan_strings) as the string "nan"
void print_list(const char* key, const std::vector<double>& v, const char* after = "", bool nan_strings = false) {
    std::printf("\"%s\": [", key);
    for (size_t i = 0; i < v.size(); ++i) {
        if (nan_strings && !std::isfinite(v[i])) std::printf("%s\"nan\"", i ? ", " : "");
        else std::printf("%s%.17g", i ? ", " : "", v[i]);
    }
    std::printf("]%s", after);
}

void print_strings(const std::vector<std::string>& v) {
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s\"%s\"", i ? ", " : "", v[i].c_str());
}

// The directory the reports go to, created: -o, or results/ (filename(), core.h:196) for the stages that write without -o
std::string report_dir(const std::string& out_dir) {
    const std::string dir = out_dir.empty() ? "results" : out_dir;
    if (::mkdir(dir.c_str(), 0777) != 0 && errno != EEXIST) throw std::runtime_error("Failed to create directory " + dir);
    return dir;
}

// The nodes in the order of the reports' columns
cladevector node_order(const clade* tree) {
    cladevector order;
    tree->apply_reverse_level_order([&order](const clade* c) { order.push_back(c); });
    return order;
}

std::vector<std::string> family_ids(const std::vector<gene_family>& fams) {
    std::vector<std::string> ids;
    for (const gene_family& f : fams) ids.push_back(f.id());
    return ids;
}

// What a search estimated, in the order of its search vector: the lambdas, the mus, then one more parameter (alpha, or nu).
// lambdas / mus / extra: nullptr for what was held fixed.
struct searched_parameters {
    size_t nl;
    bool lambda, mu, extra;
    std::vector<std::string> names;
    std::vector<double> estimates;
    searched_parameters(size_t n_lambdas, const std::vector<double>* lambdas, const std::vector<double>* mus, const char* extra_name, const double* extra_value)
        : nl(n_lambdas), lambda(lambdas), mu(mus), extra(extra_value) {
        if (lambda) add_rates("Lambda", *lambdas);
        if (mu) add_rates("Mu", *mus);
        if (extra) { names.push_back(extra_name); estimates.push_back(*extra_value); }
    }
    // the scores of one family (or table entry) of gr in these parameters; extra_score: that of the last one, asked only if searched
    std::vector<double> score_row(const gradient_result& gr, size_t entry, const std::function<double()>& extra_score) const {
        std::vector<double> s;
        if (lambda) for (size_t i = 0; i < nl; ++i) s.push_back(gr.d_lambda[entry * nl + i]);
        if (mu) for (size_t i = 0; i < nl; ++i) s.push_back(gr.d_mu[entry * nl + i]);
        if (extra) s.push_back(extra_score());
        return s;
    }
private:
    std::string rate_name(const char* what, size_t i) const { return nl == 1 ? std::string(what) : what + std::to_string(i + 1); }
    void add_rates(const char* what, const std::vector<double>& v) {
        for (size_t i = 0; i < nl; ++i) { names.push_back(rate_name(what, i)); estimates.push_back(v[i]); }
    }
};

// Both standard-error stages: the outer product of the per-family scores, the warning, the JSON fragment
struct standard_errors_stage {
    standard_errors se;
    static standard_errors_stage compute(const searched_parameters& sp, const std::vector<double>& scores, size_t families) {
        standard_errors_stage s;
        s.se = compute_standard_errors(sp.names, sp.estimates, scores, families);
        if (!s.se.ok) std::fprintf(stderr, "cafexp_hip: warning: the information matrix of the scores is singular or ill-conditioned: no standard errors\n");
        return s;
    }
    void print_json(const std::vector<double>& slopes) const {                 // (no separator before or after)
        std::printf("\"standard_errors\": {\"parameters\": [");
        print_strings(se.names);
        std::printf("], ");
        print_list("estimate", se.estimate, ", ", true); print_list("se", se.se, ", ", true); print_list("total_score", se.total_score, ", ", true);
        if (!slopes.empty()) print_list("dmultiplier_dalpha", slopes, ", ", true);
        std::printf("\"families\": %zu, \"left_out\": %zu}", se.families_used, se.families_left_out);
    }
};

struct leaf_predictive_stage {
    double seconds = 0;
    leaf_predictive_summary summary;
    // lp is in hand; t0: when its call began
    static leaf_predictive_stage run(const leaf_predictive_result& lp, time_point t0, double pvalue, const std::string& model, const std::string& dir,
                                     const std::vector<gene_family>& fams) {
        leaf_predictive_stage s;
        s.summary = write_leaf_predictive_reports(lp, pvalue, model, dir, fams);
        if (count_missing(fams).cells > 0) write_imputed_counts(lp, model, dir, fams);
        s.seconds = seconds_since(t0);
        return s;
    }
    void print_json() const {
        std::printf("\"leaf_predictive\": {\"seconds\": %.3f, \"failed_cells\": %zu, \"outliers\": %zu, ", seconds, summary.failed_cells, summary.outliers);
        print_num("log_pseudo_likelihood", summary.log_pseudo_likelihood, false);
        std::printf("}");
    }
};

struct marginal_stage {
    double seconds = 0;
    size_t failed = 0;
    void print_json(double level) const { std::printf("\"marginal\": {\"seconds\": %.3f, \"level\": %.17g, \"failed\": %zu}", seconds, level, failed); }
};

}  // namespace

// ================================================================ inputs and model
void load_inputs(const driver_options& o, bool with_families, user_data& d) {
    d.p_tree.reset(parse_newick(slurp_first_line(o.tree_path), false));
    if (with_families) {
        {
            std::ifstream f(o.fam_path);
            if (!f.is_open()) throw std::runtime_error(o.fam_path + ": Failed to open. Exiting...");
            const std::set<std::string> tokens = parse_missing_tokens(o.missing_list);
            read_gene_families(f, d.p_tree.get(), d.gene_families, o.missing_list.empty() ? nullptr : &tokens);
        }
        if (!o.mask_path.empty()) {
            std::ifstream f(o.mask_path);
            if (!f.is_open()) throw std::runtime_error("Failed to open " + o.mask_path + ". Exiting...");
            mask_cells(f, d.gene_families);
        }
        compute_max_sizes(d.gene_families, d.max_family_size, d.max_root_family_size);
        if (o.force_m > 0) { d.max_family_size = o.force_m; d.max_root_family_size = o.force_r; }
    }
    if (!o.err_path.empty()) {
        std::ifstream f(o.err_path);
        if (!f.is_open()) throw std::runtime_error("Failed to open " + o.err_path + ". Exiting...");
        d.p_error_model.reset(new error_model);
        read_error_model_file(f, d.p_error_model.get());
    }
    if (!o.lambda_tree_path.empty()) {
        d.p_lambda_tree.reset(parse_newick(slurp_first_line(o.lambda_tree_path), true));
        d.p_tree->validate_lambda_tree(d.p_lambda_tree.get());
    }
    if (o.fixed_lambda > 0) d.p_lambda.reset(new single_lambda(o.fixed_lambda));
    if (!o.multi.empty()) {
        const std::vector<double> v = parse_rates(o.multi);
        d.p_lambda.reset(new multiple_lambda(d.p_lambda_tree->get_lambda_index_map(), v));
    }
    if (!o.rootdist_path.empty()) {
        std::ifstream f(o.rootdist_path);
        if (!f.is_open()) throw std::runtime_error("Failed to open file '" + o.rootdist_path + "'");
        read_rootdist(f, d.rootdist);
    }
    if (!with_families) return;
    if (!o.keep_all) {                                           // cafexp.cpp:189-199
        auto rem = std::remove_if(d.gene_families.begin(), d.gene_families.end(), [&](const gene_family& f) { return !f.exists_at_root(d.p_tree.get()); });
        d.gene_families.erase(rem, d.gene_families.end());
    }
    if (o.limit >= 0 && (size_t)o.limit < d.gene_families.size()) d.gene_families.resize(o.limit);
    if (!o.rootdist_probs.empty()) {
        std::ifstream f(o.rootdist_probs);
        if (!f.is_open()) throw std::runtime_error("Failed to open file '" + o.rootdist_probs + "'");
        d.p_prior.reset(new file_probability_distribution(read_rootdist_probabilities(f)));
    }
    else if (o.use_poisson && o.poisson > 0) d.p_prior.reset(new poisson_distribution(o.poisson));
    else if (o.use_poisson) d.p_prior.reset(new poisson_distribution(&d.gene_families));     // fitted to the leaf sizes (root_equilibrium_distribution.cpp:34)
    else d.p_prior.reset(new uniform_distribution());
}

void build_model(const driver_options& o, user_data& d, driver_model& m) {
    m.em = d.p_error_model.get();
    if (o.gamma()) {
        m.mdl.reset(new hip_gamma_model(d.p_lambda.get(), d.p_tree.get(), &d.gene_families, d.max_family_size, d.max_root_family_size, o.k, o.fixed_alpha, m.em));
    } else {
        if (o.use_err && !m.em) {
            m.default_em.reset(new error_model());
            m.default_em->set_probabilities(0, {0, .95, 0.05});
            m.default_em->set_probabilities(d.max_family_size, {0.05, .9, 0.05});
            m.em = m.default_em.get();
        }
        m.mdl.reset(new hip_base_model(d.p_lambda.get(), d.p_tree.get(), &d.gene_families, d.max_family_size, d.max_root_family_size, m.em));
    }
    m.mdl->set_device(o.device);
    m.mdl->set_search_batch(o.search_batch);                     // contexts with room for G x K categories
    m.mdl->set_root_rule(o.root_sum ? CAFE_ROOT_SUM : CAFE_ROOT_MAX);
    if (o.estimate_rootdist) {                                   // the starting prior as the floats a call reads, held where the rounds can replace it
        root_distribution rd;
        if (!d.rootdist.empty()) rd.vectorize(d.rootdist);
        else rd.vectorize_uniform(d.max_root_family_size);
        d.p_prior->initialize(&rd);
        std::vector<double> p((size_t)d.max_root_family_size);
        for (size_t j = 0; j < p.size(); ++j) p[j] = d.p_prior->compute(j);
        m.em_prior = new file_probability_distribution(p);
        d.p_prior.reset(m.em_prior);
    }
    if (!o.mu_list.empty()) {                                    // fixed death rates: one per lambda of the -y tree (one without)
        const std::vector<double> mus = parse_rates(o.mu_list);
        size_t n_lambdas = 1;
        if (d.p_lambda_tree) {
            std::set<int> uniq;
            d.p_lambda_tree->apply_prefix_order([&](const clade* c) { uniq.insert(c->get_lambda_index()); });
            n_lambdas = uniq.size();
        }
        if (mus.size() != n_lambdas) throw std::runtime_error("--mu needs one death rate per lambda (" + std::to_string(n_lambdas) + ")");
        m.mdl->set_death_rates(mus);
    }
}

// ================================================================ --simulate
// simulator::simulate (simulator.cpp:113-147) with the checks of input_parameters::check_input (io.cpp:55-98)
int run_simulation(const driver_options& o) {
    const uint64_t seed = o.have_seed ? o.seed : randomizer_engine();
    try {
        if (!o.multi.empty() && o.lambda_tree_path.empty()) throw std::runtime_error("Multiple lambda values (-m) specified with no lambda tree (-y)");
        if (!o.fam_path.empty() && !o.rootdist_path.empty()) throw std::runtime_error("Options -i and -f are mutually exclusive.");
        if (o.fixed_lambda <= 0.0 && o.multi.empty()) throw std::runtime_error("Cannot simulate without initial lambda values");
        const bool gamma = o.gamma();
        if (gamma && !(o.fixed_alpha > 0)) throw std::runtime_error("Cannot simulate gamma clusters without an alpha value");
        if (o.use_err && o.err_path.empty()) throw std::runtime_error("Simulation needs an error model file (-e FILE)");
        user_data d;
        load_inputs(o, false, d);
        const double alpha = gamma ? o.fixed_alpha : 0.0;
        const std::vector<double> mus = parse_rates(o.mu_list);     // one per lambda (checked by the simulator); empty: lambda = mu
        const time_point t0 = now();
        simulation sim = o.simulate_on_device
            ? simulate_families_device(d.p_tree.get(), d.p_lambda.get(), d.p_error_model.get(), d.rootdist, o.simulate_n, alpha, o.device, seed, o.sim_workspace, &mus)
            : simulate_families(d.p_tree.get(), d.p_lambda.get(), d.p_error_model.get(), d.rootdist, o.simulate_n, alpha, o.device, &mus);
        const double seconds = seconds_since(t0);
        const std::string out_dir = report_dir(o.out_dir);
        const time_point t1 = now();
        {
            std::ofstream leaves(out_dir + "/simulation.txt");
            print_simulations(leaves, false, sim);
            std::ofstream truth(out_dir + "/simulation_truth.txt");
            print_simulations(truth, true, sim);
            if (!leaves || !truth) throw std::runtime_error("Failed to write the simulations to " + out_dir);
        }
        const double write_s = seconds_since(t1);
        const double avg = average_multiplier(sim);
        if (o.fixed_lambda > 0) std::cout << "Average multiplier for simulated values: " << avg << std::endl;     // simulator.cpp:141-144
        std::printf("{\"model\": \"%s\", \"mode\": \"%s\", \"n_families\": %zu, \"max_family_size\": %d, \"seconds\": %.6f, \"write_seconds\": %.6f, ",
                    gamma ? "Gamma" : "Base", o.simulate_on_device ? "device" : "host", sim.n_families, sim.max_family_size, seconds, write_s);
        print_num("average_multiplier", avg, false);
        if (!mus.empty()) { std::printf(", "); print_list("mu", mus); }
        if (!sim.multipliers.empty() && sim.multipliers.size() <= 1000) { std::printf(", "); print_list("multipliers", sim.multipliers); }     // one per chunk of 50 families
        std::printf("}\n");
    } catch (const std::exception& e) {
        std::fflush(stdout);
        std::fprintf(stderr, "cafexp_hip: %s\n", e.what());
        return 1;
    }
    return 0;
}

// ================================================================ --gain / --estimate-gain (gain_model.cpp: the table's rates under a gene gain rate)
namespace {

struct gain_run {
    const driver_options& o;
    user_data& d;
    hip_base_model* base;
    int L;                                       // the number of lambdas
    gain_options go;
    gain_table table;
    cladevector order;
    std::string out_dir;
    gain_result res;
    double fit_seconds = 0;
};

// The nested search, then Gain_results.txt and Gain_family_likelihoods.txt
void gain_fit_stage(gain_run& r, lambda* shape) {
    const driver_options& o = r.o;
    user_data& d = r.d;
    const std::set<double> lengths = d.p_tree->get_branch_lengths();
    lambda_optimizer starts(shape, r.base, d.p_prior.get(), *std::max_element(lengths.begin(), lengths.end()), d.rootdist);
    const gain_scorer score = [&](const std::vector<double>& lambdas, const std::vector<double>& mus, double nu) {
        if (o.gain_dense) return r.base->gain_lnl(d.p_prior.get(), d.rootdist, r.table.family, lambdas, mus, nu, r.go.root_absent);
        const size_t n = r.table.family.size();
        std::vector<double> lam, mu, nus(n * r.L, nu);
        for (size_t i = 0; i < n; ++i) { lam.insert(lam.end(), lambdas.begin(), lambdas.end()); mu.insert(mu.end(), mus.begin(), mus.end()); }
        return r.base->per_family_gain_lnl(d.p_prior.get(), d.rootdist, r.table.family, lam, mu, nus, r.go.root_absent);
    };
    const time_point t0 = now();
    r.res = fit_gain_model(score, r.table, r.L, r.go, [&] { return starts.initial_guesses(); });
    r.fit_seconds = seconds_since(t0);
    r.out_dir = report_dir(o.out_dir);
    std::ofstream f(r.out_dir + "/Gain_results.txt");
    write_gain_results(f, r.res, r.go, r.table);
    if (!f) throw std::runtime_error("Failed to write " + r.out_dir + "/Gain_results.txt");
    std::ofstream g(r.out_dir + "/Gain_family_likelihoods.txt");
    g << "#FamilyID\tLikelihood of Family (lnL)\n" << std::setprecision(17);
    for (size_t i = 0; i < d.gene_families.size(); ++i) g << d.gene_families[i].id() << '\t' << r.res.with.lnl[r.table.entry_of[i]] << "\n";
    g << "(absent)\t" << r.res.with.lnl.back() << "\n";
    if (!g) throw std::runtime_error("Failed to write " + r.out_dir + "/Gain_family_likelihoods.txt");
}

// --gain-posterior (gain_origins.cpp): one call at the fitted rates over every distinct family
struct gain_posterior_stage {
    double seconds = 0;
    gain_branch_origins origins;
    static gain_posterior_stage run(const gain_run& r) {
        gain_posterior_stage s;
        const time_point t0 = now();
        const gain_fit& fit = r.res.with;
        const bool dense = r.o.gain_dense;
        const size_t sets = dense ? 1 : r.table.family.size();      // --gain-dense: the fitted rate set once, cafe_gain_posterior_dense
        std::vector<double> lam, mu, nus(sets * r.L, fit.nu);
        for (size_t i = 0; i < sets; ++i) { lam.insert(lam.end(), fit.lambdas.begin(), fit.lambdas.end()); mu.insert(mu.end(), fit.mus.begin(), fit.mus.end()); }
        const gain_origins go_res = r.base->gain_posterior(r.d.p_prior.get(), r.d.rootdist, r.table.family, lam, mu, nus, r.go.root_absent, r.order, dense);
        std::vector<std::string> names;
        size_t root = 0;
        for (size_t v = 0; v < r.order.size(); ++v) { names.push_back(clade_index_or_name(r.order[v], r.order)); if (r.order[v]->is_root()) root = v; }
        s.origins = gain_origin_totals(go_res, r.table.weight, root);
        std::ofstream cells(r.out_dir + "/Gain_origins.tab"), totals(r.out_dir + "/Gain_branch_origins.tab");
        write_gain_origins(cells, go_res, names, root, family_ids(r.d.gene_families), r.table.entry_of);
        write_gain_branch_origins(totals, s.origins, names, root);
        if (!cells || !totals) throw std::runtime_error("Failed to write " + r.out_dir + "/Gain_origins.tab or Gain_branch_origins.tab");
        s.seconds = seconds_since(t0);
        return s;
    }
    void print_json(bool dense) const {
        double originated = 0, lost = 0;
        for (double v : origins.originated) originated += v;
        for (double v : origins.lost) lost += v;
        std::printf("\"gain_posterior_path\": \"%s\", ", dense ? "cafe_gain_posterior_dense" : "cafe_gain_posterior");
        std::printf("\"gain_posterior_seconds\": %.3f, \"expected_origins\": %.12g, \"expected_losses\": %.12g, \"absent_at_root\": %.12g, "
                    "\"families_with_a_likely_origin\": %.12g, ", seconds, originated, lost, origins.absent_at_root, origins.origin_somewhere);
    }
};

// (with --gain-dense only) the leave-one-out check at the fitted rates
leaf_predictive_stage gain_leaf_predictive_stage(const gain_run& r) {
    const time_point t0 = now();
    const gain_fit& fit = r.res.with;
    const leaf_predictive_result lp = r.base->gain_leaf_predictive(r.d.p_prior.get(), r.d.rootdist, r.table.family, r.table.entry_of, fit.lambdas, fit.mus,
                                                                   fit.nu, r.go.root_absent);
    return leaf_predictive_stage::run(lp, t0, r.o.test_pvalue, "Gain", r.out_dir, r.d.gene_families);
}

// (with --gain-dense only) posterior sizes and change at the fitted rates
marginal_stage gain_marginal_stage(const gain_run& r) {
    marginal_stage s;
    const time_point t0 = now();
    const gain_fit& fit = r.res.with;
    const marginal_result mr = r.base->gain_marginal(r.d.p_prior.get(), r.d.rootdist, r.table.family, r.table.entry_of, fit.lambdas, fit.mus, fit.nu,
                                                     r.go.root_absent, r.o.marginal_level, r.order);
    s.failed = mr.failed_count();
    write_marginal_reports(mr, "Gain", r.out_dir, r.order, r.d.gene_families);
    s.seconds = seconds_since(t0);
    return s;
}

// (with --gain-dense only) the scores of the searched objective at the fitted rates
standard_errors_stage gain_standard_errors_stage(const gain_run& r) {
    const gain_fit& fit = r.res.with;
    const gain_options& go = r.go;
    const bool lambda_searched = go.fixed_lambdas.empty(), estimate_mu = r.o.estimate_mu, mu_tied = !estimate_mu && go.fixed_mus.empty();
    const gradient_result gr = r.base->gain_score_gradient(r.d.p_prior.get(), r.d.rootdist, r.table.family, fit.lambdas, fit.mus, fit.nu, go.root_absent, mu_tied);
    const size_t nl = (size_t)r.L, F = r.d.gene_families.size(), absent = r.table.family.size() - 1;
    const searched_parameters sp(nl, lambda_searched ? &fit.lambdas : nullptr, estimate_mu ? &fit.mus : nullptr, "Nu", go.estimate_nu ? &fit.nu : nullptr);
    if (sp.names.empty()) throw std::runtime_error("--standard-errors: no parameter was estimated (lambda, mu and nu are all fixed)");
    const size_t P = sp.names.size();
    auto score_of = [&](size_t entry) {                          // one nu for every rate index
        return sp.score_row(gr, entry, [&] { double t = 0; for (size_t i = 0; i < nl; ++i) t += gr.d_nu[entry * nl + i]; return t; });
    };
    const std::vector<double> s_abs = score_of(absent);
    const double p = std::exp(gr.family_lnl[absent]), odds = go.conditional ? p / (1 - p) : 0.0;
    std::vector<double> scores(F * P);
    for (size_t f = 0; f < F; ++f) {
        const std::vector<double> s = score_of(r.table.entry_of[f]);
        for (size_t k = 0; k < P; ++k) scores[f * P + k] = go.conditional ? s[k] + odds * s_abs[k] : s[k];
    }
    const standard_errors_stage stage = standard_errors_stage::compute(sp, scores, F);
    std::string cond = go.conditional ? "the family being seen in at least one species, root_absent as given" : "root_absent as given";
    if (!lambda_searched) cond += ", the fixed lambda";
    if (!estimate_mu) cond += mu_tied ? ", mu = lambda" : ", the fixed mu";
    if (!go.estimate_nu) cond += ", the fixed nu";
    write_standard_errors(stage.se, "Gain", r.out_dir, cond);
    return stage;
}

}  // namespace

void run_gain_model(const driver_options& o, user_data& d, driver_model& m) {
    hip_base_model* base = static_cast<hip_base_model*>(m.mdl.get());      // -k / -a were refused
    base->set_workspace_limit(o.sim_workspace);
    base->set_root_rule(CAFE_ROOT_SUM);                          // the absent profile's value is a probability under the sum rule only
    base->set_gain_scaling(o.gain_scaled);                       // the search and --gain-posterior, through the two dense calls
    base->initialize_lambda(d.p_lambda_tree.get());
    std::unique_ptr<lambda> shape(base->get_lambda());
    gain_run r{o, d, base, shape->count(), {}, {}, {}, {}, {}};
    gain_options& go = r.go;
    go.estimate_nu = o.estimate_gain; go.fixed_nu = o.gain_nu; go.root_absent = o.root_absent; go.conditional = !o.gain_unconditional;
    go.estimate_mu = o.estimate_mu; go.max_iterations = o.max_iter;
    if (o.fixed_lambda > 0) go.fixed_lambdas.assign(1, o.fixed_lambda);
    if (!o.multi.empty()) go.fixed_lambdas = parse_rates(o.multi);
    if (!o.mu_list.empty()) go.fixed_mus = parse_rates(o.mu_list);
    r.table = gain_distinct_families(d.gene_families);
    r.order = node_order(d.p_tree.get());
    gain_fit_stage(r, shape.get());
    gain_posterior_stage posterior;
    leaf_predictive_stage predictive;
    marginal_stage marginal;
    standard_errors_stage se;
    if (o.gain_posterior) posterior = gain_posterior_stage::run(r);
    if (o.do_leaf_predictive) predictive = gain_leaf_predictive_stage(r);
    if (o.do_marginal) marginal = gain_marginal_stage(r);
    if (o.do_standard_errors) se = gain_standard_errors_stage(r);
    base->set_lambda(nullptr);                                   // `shape` goes with this scope
    const gain_result& res = r.res;
    std::printf("{\"model\": \"Gain\", \"root_rule\": \"sum\", \"conditional\": %s, \"families\": %zu, \"distinct_families\": %zu, ",
                go.conditional ? "true" : "false", d.gene_families.size(), r.table.family.size() - 1);
    if (o.gain_dense) std::printf("\"gain_dense_mode\": \"%s\", ", o.gain_scaled ? "scaled" : "plain");
    std::printf("\"neg_lnl\": %.17g, ", res.with.neg_lnl);
    print_list("lambda", res.with.lambdas, ", "); print_list("mu", res.with.mus, ", ");
    std::printf("\"nu\": %.17g, \"root_absent\": %.17g, \"p_absent\": %.17g, \"neg_lnl_without_gain\": %.17g, ", res.with.nu, go.root_absent, res.with.p_absent,
                res.without.neg_lnl);
    print_list("lambda_without_gain", res.without.lambdas, ", "); print_list("mu_without_gain", res.without.mus, ", ");
    print_list("start_without_gain", res.without.start, ", "); print_list("start", res.with.start, ", ");
    if (o.gain_posterior) posterior.print_json(o.gain_dense);
    if (o.do_leaf_predictive) { predictive.print_json(); std::printf(", "); }
    if (o.do_marginal) { marginal.print_json(o.marginal_level); std::printf(", "); }
    if (o.do_standard_errors) { se.print_json({}); std::printf(", "); }
    std::printf("\"lr_statistic\": %.17g, \"calls\": %d, \"max_family_size\": %d, \"max_root_family_size\": %d, \"seconds\": %.3f}\n", res.lr_statistic,
                res.without.calls + res.with.calls, d.max_family_size, d.max_root_family_size, r.fit_seconds);
}

// ================================================================ -b: estimator::estimate_lambda_per_family (execute.cpp:104-128, :136-141)
void run_lambda_per_family(const driver_options& o, user_data& d, driver_model& m) {
    hip_base_model* base = static_cast<hip_base_model*>(m.mdl.get());      // -k / -a were refused
    base->set_workspace_limit(o.sim_workspace);
    const time_point t0 = now();
    per_family_mu fmu;
    if (o.family_mu == "estimate") fmu.mode = per_family_mu::ESTIMATE;
    else if (!o.family_mu.empty()) { fmu.mode = per_family_mu::FIXED; fmu.fixed = parse_rates(o.family_mu); }
    const per_family_result res = estimate_lambda_per_family(*base, d, o.max_iter, fmu);
    const double seconds = seconds_since(t0);
    const std::string out_dir = report_dir(o.out_dir);
    {
        std::unique_ptr<lambda> shape(d.p_lambda_tree ? (lambda*)new multiple_lambda(d.p_lambda_tree->get_lambda_index_map(), res.lambdas.empty() ? std::vector<double>() : res.lambdas[0])
                                                      : (lambda*)new single_lambda(0.0));
        auto write = [&](const std::string& path, const std::vector<std::vector<double>>& rates) {       // one line per family, in the -y shape
            std::ofstream f(path);
            for (size_t i = 0; i < d.gene_families.size(); ++i) {
                shape->update(rates[i].data());
                f << d.gene_families[i].id() << '\t' << shape->to_string() << "\n";
            }
            if (!f) throw std::runtime_error("Failed to write " + path);
        };
        write(out_dir + "/" + base->name() + "_lambda_per_family.txt", res.lambdas);
        if (fmu.mode != per_family_mu::NONE) write(out_dir + "/" + base->name() + "_mu_per_family.txt", res.mus);
    }
    std::printf("{\"model\": \"%s\", \"mode\": \"lambda_per_family\", \"families\": %zu, \"distinct_families\": %zu, \"rounds\": %d, \"evaluations\": %ld, \"restarts\": %ld, "
                "\"max_family_size\": %d, \"max_root_family_size\": %d, ", base->name().c_str(), d.gene_families.size(), res.distinct_families, res.rounds,
                res.evaluations, res.restarts, d.max_family_size, d.max_root_family_size);
    if (auto pd = dynamic_cast<poisson_distribution*>(d.p_prior.get())) print_num("poisson_lambda", pd->poisson_lambda());
    if (fmu.mode != per_family_mu::NONE) std::printf("\"family_mu\": \"%s\", ", fmu.mode == per_family_mu::FIXED ? "fixed" : "estimate");
    std::printf("\"seconds\": %.3f}\n", seconds);
}

// ================================================================ the fitted model
namespace {

struct fitted_run {
    const driver_options& o;
    user_data& d;
    hip_model_base* mdl;
    error_model* em;
    cladevector order;
    std::string out_dir;                         // -o; "results" from the moment --estimate-rootdist writes
    bool lambda_searched = false, alpha_searched = false;      // what the search estimated (the score reports condition on the rest)
    std::vector<double> slopes;                  // d multiplier / d alpha, when a score report needs them
    hip_gamma_model* gamma() const { return dynamic_cast<hip_gamma_model*>(mdl); }
    int root_rule() const { return o.root_sum ? CAFE_ROOT_SUM : CAFE_ROOT_MAX; }
    root_equilibrium_distribution* prior() const { return d.p_prior.get(); }
    const std::string name() const { return mdl->name(); }
};

// The search (estimate_missing_variables, execute.cpp:78) and, behind it, the EM rounds on the root distribution: the E step is
// one cafe_root_posterior call at the optimum, the M step total / n_used
struct search_stage {
    struct em_round { double neg_lnl; std::string rates; };
    std::unique_ptr<inference_optimizer_scorer> scorer;          // nullptr: every parameter was given
    std::unique_ptr<lambda> owned_lambda;
    optimizer_result opt;
    double seconds = 0;
    std::vector<em_round> rounds;

    optimizer_result search_once(const driver_options& o, const std::vector<double>* start) {
        optimizer opz(scorer.get());
        opz.max_iterations = o.max_iter;
        opz.batch = o.search_batch;
        if (start) opz.start = *start;
        const time_point t0 = now();
        optimizer_result found = opz.optimize();
        seconds += seconds_since(t0);
        scorer->finalize(found.values.data());
        return found;
    }
    static search_stage run(const fitted_run& r, file_probability_distribution* em_prior) {
        const driver_options& o = r.o;
        user_data& d = r.d;
        hip_model_base* mdl = r.mdl;
        search_stage s;
        s.scorer.reset(mdl->get_lambda_optimizer(d));
        if (o.estimate_mu)                                       // lambda is searched (-l / -m were refused), so the scorer leads with the lambdas
            s.scorer.reset(new lambda_mu_optimizer(s.scorer.release(), mdl->get_lambda(), mdl, r.prior(), d.rootdist));
        if (s.scorer) {
            if (!d.p_lambda) s.owned_lambda.reset(mdl->get_lambda());
            if (o.search_batch > 1 && !s.scorer->batchable())
                std::cout << "--search-batch: the error model is estimated (one error table per point): the look-ahead points are scored one call each" << std::endl;
            s.opt = s.search_once(o, nullptr);
        }
        if (!o.estimate_rootdist) return s;
        auto rates_now = [&] {
            std::string t = "Lambda: " + mdl->get_lambda()->to_string();
            if (!mdl->death_rates().empty()) t += " Mu: " + mdl->death_rates_to_string();
            if (auto gm = r.gamma()) { std::ostringstream os; os.precision(14); os << " Alpha: " << gm->get_alpha(); t += os.str(); }
            return t;
        };
        double prev = s.scorer ? s.opt.score : mdl->infer_family_likelihoods(r.prior(), d.rootdist, mdl->get_lambda());
        s.rounds.push_back({prev, rates_now()});
        for (int round = 1; round <= o.rootdist_rounds; ++round) {
            const root_posterior_result rp = mdl->root_posterior(r.prior(), d.rootdist);
            if (rp.n_used < 1) throw std::runtime_error("--estimate-rootdist: every family failed (zero likelihood) at the current optimum");
            std::vector<double> p(rp.total.size());
            for (size_t j = 0; j < p.size(); ++j) p[j] = (double)(float)(rp.total[j] / (double)rp.n_used);      // the float the ABI takes
            em_prior->set(p);
            double cur;
            if (s.scorer) {
                const optimizer_result again = s.search_once(o, &s.opt.values);
                s.opt.values = again.values; s.opt.score = again.score;
                s.opt.num_iterations += again.num_iterations; s.opt.num_scorer_calls += again.num_scorer_calls;
                s.opt.num_batches += again.num_batches; s.opt.num_points_scored += again.num_points_scored;
                cur = again.score;
            } else {
                cur = mdl->infer_family_likelihoods(r.prior(), d.rootdist, mdl->get_lambda());
            }
            s.rounds.push_back({cur, rates_now()});
            const bool settled = prev - cur < optimizer(nullptr).similarity_precision * std::fabs(prev);
            prev = cur;
            if (settled) break;
        }
        return s;
    }
    void print_json(const driver_options& o) const {
        if (scorer) {
            std::printf(", \"search\": {\"iterations\": %d, \"scorer_calls\": %d, \"seconds\": %.3f, ", opt.num_iterations, opt.num_scorer_calls, seconds);
            if (o.search_batch > 1) std::printf("\"batches\": %d, \"points_scored\": %d, ", opt.num_batches, opt.num_points_scored);
            print_num("score", opt.score, false);
            std::printf("}");
        }
        if (o.estimate_rootdist) {
            std::printf(", \"rootdist\": {\"rounds\": [");
            for (size_t i = 0; i < rounds.size(); ++i) {
                if (std::isfinite(rounds[i].neg_lnl)) std::printf("%s%.17g", i ? ", " : "", rounds[i].neg_lnl);
                else std::printf("%s\"inf\"", i ? ", " : "");
            }
            std::printf("], \"max_rounds\": %d}", o.rootdist_rounds);
        }
    }
};

// compute (execute.cpp:42) at the final parameters, --reps times, and the files of estimator::compute (execute.cpp:49-54)
struct score_stage {
    double score = 0, best_seconds = 1e300;
    static score_stage run(fitted_run& r, const search_stage& search, const file_probability_distribution* em_prior) {
        const driver_options& o = r.o;
        user_data& d = r.d;
        hip_model_base* mdl = r.mdl;
        score_stage s;
        for (int rep = 0; rep < o.reps; ++rep) {
            const time_point t0 = now();
            s.score = mdl->infer_family_likelihoods(r.prior(), d.rootdist, mdl->get_lambda());
            s.best_seconds = std::min(s.best_seconds, seconds_since(t0));
        }
        if (!o.family_out.empty()) {
            std::ofstream f(o.family_out);
            f.precision(17);
            mdl->write_family_likelihoods(f);
        }
        if (o.estimate_rootdist) r.out_dir = report_dir(r.out_dir);      // its files, the results file's rounds among them, default to results/
        if (!r.out_dir.empty()) {
            std::ofstream rf(r.out_dir + "/" + r.name() + "_results.txt");
            mdl->write_vital_statistics(rf, s.score);
            const missing_summary ms = count_missing(d.gene_families);
            if (ms.cells > 0) rf << "Missing cells: " << ms.cells << " in " << ms.families << " families (summed out)" << std::endl;
            rf.precision(17);
            for (size_t i = 0; i < search.rounds.size(); ++i)
                rf << "Root distribution round " << i << ": -lnL " << search.rounds[i].neg_lnl << " " << search.rounds[i].rates << std::endl;
            std::ofstream lf(r.out_dir + "/" + r.name() + "_family_likelihoods.txt");
            mdl->write_family_likelihoods(lf);
            if (o.use_err) {                                     // write_error_model_if_specified (execute.cpp:24-40)
                std::ofstream ef(r.out_dir + "/" + r.name() + "_error_model.txt");
                if (r.em) write_error_model_file(ef, *r.em);
                else {                                           // model::write_error_model's stand-in (core.cpp:118-127)
                    error_model none;
                    none.set_probabilities(d.max_family_size, {0, 1, 0});
                    write_error_model_file(ef, none);
                }
            }
        }
        if (o.estimate_rootdist) {
            std::ofstream f(r.out_dir + "/" + r.name() + "_root_distribution.txt");
            write_rootdist_probabilities(f, em_prior->probabilities());
            if (!f) throw std::runtime_error("Failed to write " + r.out_dir + "/" + r.name() + "_root_distribution.txt");
        }
        return s;
    }
};

// the posterior probability of every rate category per family, under the rule that was searched (no JSON fragment)
void category_posterior_stage(const fitted_run& r) {
    const root_posterior_result rp = r.mdl->root_posterior(r.prior(), r.d.rootdist);
    const std::string dir = report_dir(r.out_dir);
    std::ofstream f(dir + "/" + r.name() + "_category_posterior.tab");
    f.precision(17);
    f << "#FamilyID";
    for (double m : r.gamma()->get_lambda_multipliers()) f << '\t' << m;
    f << '\n';
    for (size_t i = 0; i < r.d.gene_families.size(); ++i) {
        f << r.d.gene_families[i].id();
        for (size_t c = 0; c < rp.n_categories; ++c) f << '\t' << rp.category_posterior[i * rp.n_categories + c];
        f << '\n';
    }
    if (!f) throw std::runtime_error("Failed to write " + dir + "/" + r.name() + "_category_posterior.tab");
}

// compute_pvalues with the model's plain lambda (execute.cpp:153-161); 1000 simulations in the reference
struct pvalue_stage {
    std::vector<double> pvalues;
    double seconds = 0;
    static pvalue_stage run(const fitted_run& r) {
        const driver_options& o = r.o;
        const user_data& d = r.d;
        pvalue_stage s;
        pvalue_work work;
        const time_point t0 = now();
        if (o.pvalues_on_device)    // simulation on the GPU too: same distribution, another random sample (cafe_pvalues)
            s.pvalues = r.mdl->device_pvalues(o.pvalue_sims, o.have_seed ? o.seed : 1u);
        else
            s.pvalues = compute_pvalues(d.p_tree.get(), d.gene_families, r.mdl->get_lambda(), o.pvalue_sims, d.max_family_size, d.max_root_family_size,
                                        o.device, &work, &r.mdl->death_rates());
        s.seconds = seconds_since(t0);
        if (!o.pvalues_out.empty()) {
            std::ofstream f(o.pvalues_out);
            f.precision(17);
            f << "#FamilyID\tpvalue\tobserved max likelihood\n";
            for (size_t i = 0; i < s.pvalues.size(); ++i)
                f << d.gene_families[i].id() << '\t' << s.pvalues[i] << '\t'
                  << (work.observed_max_likelihood.empty() ? 0.0 : work.observed_max_likelihood[i]) << '\n';
        }
        if (!o.pvalues_cond.empty()) {                           // FILE:K -> the first K sorted conditional distributions, one per line
            const size_t colon = o.pvalues_cond.rfind(':');
            const size_t kdump = std::min<size_t>(work.conditional_distribution.size(), std::stoul(o.pvalues_cond.substr(colon + 1)));
            std::ofstream f(o.pvalues_cond.substr(0, colon));
            f.precision(17);
            for (size_t i = 0; i < kdump; ++i) {
                for (size_t j = 0; j < work.conditional_distribution[i].size(); ++j) f << (j ? "\t" : "") << work.conditional_distribution[i][j];
                f << '\n';
            }
        }
        return s;
    }
    void print_json(int simulations) const {
        size_t sig = 0;
        for (double p : pvalues) if (p < 0.05) ++sig;
        std::printf(", \"pvalues\": {\"simulations\": %d, \"seconds\": %.3f, \"significant_at_0.05\": %zu}", simulations, seconds, sig);
    }
};

// reconstruct_ancestral_states, Viterbi branch probabilities of the significant families, reports (execute.cpp:163-180)
struct reconstruct_stage {
    double seconds = 0;
    size_t n_with_probs = 0;
    static reconstruct_stage run(const fitted_run& r, std::vector<double> pvalues) {
        const user_data& d = r.d;
        reconstruct_stage s;
        if (pvalues.empty()) pvalues.assign(d.gene_families.size(), 1.0);
        const time_point t0 = now();
        std::unique_ptr<reconstruction> rec(r.mdl->reconstruct_ancestral_states(d.gene_families, r.prior()));
        branch_probabilities probs = compute_branch_probabilities(*r.mdl, *rec, d.gene_families, pvalues, r.o.test_pvalue, r.order);
        s.seconds = seconds_since(t0);
        for (const auto& gf : d.gene_families) s.n_with_probs += probs.contains(gf);
        if (!r.out_dir.empty()) rec->write_results(r.name(), r.out_dir, d.p_tree.get(), d.gene_families, pvalues, r.o.test_pvalue, probs);
        return s;
    }
    void print_json() const { std::printf(", \"reconstruct\": {\"seconds\": %.3f, \"families_with_branch_probabilities\": %zu}", seconds, n_with_probs); }
};

// marginal reconstruction with the model's final parameters and prior: independent of --reconstruct
marginal_stage fitted_marginal_stage(const fitted_run& r) {
    marginal_stage s;
    const time_point t0 = now();
    const marginal_result mr = r.mdl->marginal_reconstruction(r.prior(), r.d.rootdist, r.o.marginal_level, r.order);
    s.seconds = seconds_since(t0);
    s.failed = mr.failed_count();
    if (!r.out_dir.empty()) write_marginal_reports(mr, r.name(), r.out_dir, r.order, r.d.gene_families);
    return s;
}

// histories drawn from the same posterior, counted per draw: independent of the two reconstructions
struct histories_stage {
    double seconds = 0;
    size_t failed = 0;
    static histories_stage run(const fitted_run& r) {
        histories_stage s;
        const time_point t0 = now();
        const history_result hr = r.mdl->sample_histories(r.prior(), r.d.rootdist, r.o.history_draws, r.o.history_seed, r.order);
        s.seconds = seconds_since(t0);
        s.failed = hr.failed_count();
        if (!r.out_dir.empty()) write_history_reports(hr, r.o.marginal_level, r.name(), r.out_dir, r.order);
        return s;
    }
    void print_json(int draws) const { std::printf(", \"histories\": {\"seconds\": %.3f, \"draws\": %d, \"failed\": %zu}", seconds, draws, failed); }
};

// expected gains and losses per branch under the same model: what the node sizes of the reconstructions do not show
struct events_stage {
    double seconds = 0;
    size_t failed = 0;
    static events_stage run(const fitted_run& r) {
        events_stage s;
        const time_point t0 = now();
        const events_result er = r.mdl->expected_events(r.prior(), r.d.rootdist, r.order);
        s.seconds = seconds_since(t0);
        s.failed = er.failed_count();
        if (!r.out_dir.empty()) write_events_reports(er, r.name(), r.out_dir, r.order, r.d.gene_families);
        return s;
    }
    void print_json() const { std::printf(", \"expected_events\": {\"seconds\": %.3f, \"failed\": %zu}", seconds, failed); }
};

// the leave-one-out predictive check of every leaf count under the same model: which cells of the table are surprising
leaf_predictive_stage fitted_leaf_predictive_stage(const fitted_run& r) {
    const time_point t0 = now();
    const leaf_predictive_result lp = r.mdl->leaf_predictive(r.prior(), r.d.rootdist);
    return leaf_predictive_stage::run(lp, t0, r.o.test_pvalue, r.name(), report_dir(r.out_dir), r.d.gene_families);
}

// the posterior of every branch's size change under the same model: by how much, and how sure
struct branch_change_stage {
    double seconds = 0;
    int band = 0;
    size_t failed = 0, clipped = 0;
    static branch_change_stage run(const fitted_run& r) {
        branch_change_stage s;
        const time_point t0 = now();
        s.band = std::min(r.o.branch_change_band, std::max(r.d.max_family_size, r.d.max_root_family_size));      // no change is larger
        const branch_change_result bc = r.mdl->branch_change(r.prior(), r.d.rootdist, s.band, 1.0 - r.o.test_pvalue, r.order);
        const std::string dir = report_dir(r.out_dir);
        s.clipped = write_branch_change_reports(bc, r.name(), dir, family_ids(r.d.gene_families));
        s.failed = bc.failed_count();
        s.seconds = seconds_since(t0);
        return s;
    }
    void print_json(double pvalue) const {
        std::printf(", \"branch_change\": {\"seconds\": %.3f, \"max_change\": %d, \"level\": %.17g, \"failed\": %zu, \"clipped\": %zu}", seconds, band,
                    1.0 - pvalue, failed, clipped);
    }
};

// what the search estimated, for a score record with nl lambdas
searched_parameters fitted_searched(const fitted_run& r, size_t nl) {
    const std::vector<double> lv = r.mdl->get_lambda()->values();
    const double alpha = r.alpha_searched ? r.gamma()->get_alpha() : 0.0;
    return searched_parameters(nl, r.lambda_searched ? &lv : nullptr, r.o.estimate_mu ? &r.mdl->death_rates() : nullptr, "Alpha",
                               r.alpha_searched ? &alpha : nullptr);
}

// standard errors of what the search estimated, from the per-family scores of the searched objective at the optimum
standard_errors_stage fitted_standard_errors_stage(const fitted_run& r) {
    const gradient_result gr = r.mdl->score_gradient(r.prior(), r.d.rootdist, r.root_rule());
    const size_t F = r.d.gene_families.size();
    const searched_parameters sp = fitted_searched(r, gr.n_lambdas);
    if (sp.names.empty()) throw std::runtime_error("--standard-errors: no parameter was estimated (lambda, mu and alpha are all fixed)");
    std::vector<double> scores;
    for (size_t f = 0; f < F; ++f) {
        const std::vector<double> row = sp.score_row(gr, f, [&] {
            double s = 0;
            for (size_t c = 0; c < gr.n_categories; ++c) s += gr.d_multiplier[f * gr.n_categories + c] * r.slopes[c];
            return s;
        });
        scores.insert(scores.end(), row.begin(), row.end());
    }
    const standard_errors_stage stage = standard_errors_stage::compute(sp, scores, F);
    std::string cond = r.em ? "the error model (epsilon is not differentiated)" : "the model as fitted";
    if (!r.lambda_searched) cond += ", the fixed lambda";
    if (!r.mdl->death_rates().empty() && !r.o.estimate_mu) cond += ", the fixed mu";
    if (r.gamma() && !r.alpha_searched) cond += ", the fixed alpha";
    write_standard_errors(stage.se, r.name(), report_dir(r.out_dir), cond);
    return stage;
}

// score tests of a rate shift on every branch and clade, from the branch scores and their information at the optimum
struct rate_shift_stage {
    rate_shift_scan scan;
    double seconds = 0;
    bool tree_written = false;
    static rate_shift_stage run(const fitted_run& r) {
        rate_shift_stage s;
        const time_point t0 = now();
        const branch_scores_result bs = r.mdl->branch_scores(r.prior(), r.d.rootdist, r.root_rule(), r.order);
        const searched_parameters sp = fitted_searched(r, bs.n_lambdas);
        std::vector<std::vector<double>> theta;              // one direction in the global parameters per searched parameter
        auto unit = [&](size_t at) { std::vector<double> v(bs.P, 0.0); v[at] = 1.0; return v; };
        if (sp.lambda) for (size_t i = 0; i < bs.n_lambdas; ++i) theta.push_back(unit(bs.global(i)));
        if (sp.mu) for (size_t i = 0; i < bs.n_lambdas; ++i) theta.push_back(unit(bs.global(bs.n_lambdas + i)));
        if (sp.extra) {
            std::vector<double> v(bs.P, 0.0);
            for (size_t c = 0; c < bs.n_categories; ++c) v[bs.global(bs.n_lambdas * bs.n_par + c)] = r.slopes[c];
            theta.push_back(v);
        }
        s.scan = compute_rate_shift_scan(bs, r.order, theta, sp.names);
        const std::string dir = report_dir(r.out_dir);
        write_rate_shift_scan(s.scan, r.name(), dir, r.order);
        s.tree_written = s.scan.best >= 0 && s.scan.rows[(size_t)s.scan.best].subtree.holm < r.o.test_pvalue;
        if (s.tree_written) write_rate_shift_lambda_tree(s.scan, r.d.p_tree.get(), r.name(), dir);
        else std::fprintf(stderr, "cafexp_hip: --rate-shift-scan: no rate shift passed the threshold %g (Holm-adjusted clade p)\n", r.o.test_pvalue);
        s.seconds = seconds_since(t0);
        return s;
    }
    void print_json(const std::vector<double>& slopes, double threshold) const {
        std::printf(", \"rate_shift_scan\": {\"seconds\": %.3f, \"families\": %zu, \"left_out\": %zu, \"profiled\": [", seconds, scan.families_used, scan.families_failed);
        print_strings(scan.profiled);
        std::printf("], ");
        print_list("dmultiplier_dalpha", slopes, ", ");
        std::printf("\"threshold\": %.17g, \"lambda_tree_written\": %s, ", threshold, tree_written ? "true" : "false");
        print_num("smallest_clade_holm_p", scan.best >= 0 ? scan.rows[(size_t)scan.best].subtree.holm : NAN, false);
        std::printf("}");
    }
};

// the model's own part of the JSON object: what was scored, and the parameters it ended at
void print_model_json(const fitted_run& r, const score_stage& scored) {
    std::printf("{\"model\": \"%s\", ", r.name().c_str());
    print_num("neg_lnl", scored.score);
    if (r.o.root_sum) std::printf("\"root_rule\": \"sum\", ");
    std::printf("\"n_families\": %zu, \"max_family_size\": %d, \"max_root_family_size\": %d, \"seconds_per_call\": %.6f, ",
                r.d.gene_families.size(), r.d.max_family_size, r.d.max_root_family_size, scored.best_seconds);
    print_list("lambda", r.mdl->get_lambda()->values());
    if (!r.mdl->death_rates().empty()) { std::printf(", "); print_list("mu", r.mdl->death_rates()); }
    if (auto g = r.gamma()) {
        std::printf(", "); print_num("alpha", g->get_alpha(), false);
        std::printf(", "); print_list("multipliers", g->get_lambda_multipliers());
    }
    if (r.em) { std::printf(", "); print_num("epsilon", r.em->get_epsilons().back(), false); }
}

}  // namespace

void run_fitted_model(const driver_options& o, user_data& d, driver_model& m) {
    hip_model_base* mdl = m.mdl.get();
    if (o.n_gpus > 1) {
        std::vector<int> devs(o.n_gpus);
        for (int g = 0; g < o.n_gpus; ++g) devs[g] = g;
        mdl->set_devices(devs);
    }
    fitted_run r{o, d, mdl, m.em, node_order(d.p_tree.get()), o.out_dir, false, false, {}};
    const search_stage search = search_stage::run(r, m.em_prior);
    const score_stage scored = score_stage::run(r, search, m.em_prior);
    if (o.root_sum && r.gamma()) category_posterior_stage(r);
    pvalue_stage pvalues;
    reconstruct_stage reconstruct;
    marginal_stage marginal;
    histories_stage histories;
    events_stage events;
    leaf_predictive_stage predictive;
    branch_change_stage change;
    standard_errors_stage se;
    rate_shift_stage shift;
    if (o.pvalue_sims > 0) pvalues = pvalue_stage::run(r);       // (draws from randomizer_engine before the reconstruction does)
    if (o.do_reconstruct) reconstruct = reconstruct_stage::run(r, pvalues.pvalues);
    if (o.do_marginal) marginal = fitted_marginal_stage(r);
    if (o.do_histories) histories = histories_stage::run(r);
    if (o.do_events) events = events_stage::run(r);
    if (o.do_leaf_predictive) predictive = fitted_leaf_predictive_stage(r);
    if (o.do_branch_change) change = branch_change_stage::run(r);
    r.lambda_searched = search.scorer && !d.p_lambda;
    r.alpha_searched = search.scorer && r.gamma() && !(o.fixed_alpha > 0);
    if ((o.do_standard_errors || o.do_rate_shift) && r.alpha_searched) r.slopes = multiplier_slopes(r.gamma()->get_lambda_multipliers().size(), r.gamma()->get_alpha());
    if (o.do_standard_errors) se = fitted_standard_errors_stage(r);
    if (o.do_rate_shift) shift = rate_shift_stage::run(r);

    print_model_json(r, scored);
    search.print_json(o);
    if (o.pvalue_sims > 0) pvalues.print_json(o.pvalue_sims);
    if (o.do_reconstruct) reconstruct.print_json();
    if (o.do_marginal) { std::printf(", "); marginal.print_json(o.marginal_level); }
    if (o.do_histories) histories.print_json(o.history_draws);
    if (o.do_events) events.print_json();
    if (o.do_branch_change) change.print_json(o.test_pvalue);
    if (o.do_leaf_predictive) { std::printf(", "); predictive.print_json(); }
    if (o.do_standard_errors) { std::printf(", "); se.print_json(r.slopes); }
    if (o.do_rate_shift) shift.print_json(r.slopes, o.test_pvalue);
    std::printf("}\n");
}

}  // namespace cafe
