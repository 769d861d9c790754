// The gene gain rate (--gain NU, --estimate-gain): one set of rates for the whole table under the linear birth-death process
// with immigration, n -> n+1 at rate n lambda + nu, n -> n-1 at rate n mu, scored by cafe_score_per_family_gain.
//
// Every model the scorer fits has size 0 absorbing, so a family that is absent in an ancestor has likelihood 0 below it; with
// nu > 0 it has not.  The price is that the all-zero profile becomes possible too, and a table never holds the families nobody
// saw.  So the objective is the likelihood CONDITIONAL on a family having been seen in at least one species,
//     -sum_f w_f lnL_f + F log(1 - exp(lnL_absent)),
// f over the DISTINCT families with their multiplicities w_f (sum F), lnL_absent the value of CAFE_FAMILY_ABSENT under the same
// rates -- one device call per point lists every distinct family once and the absent profile last.  It is evaluated under the
// SUM rule: only there is the absent profile's value a probability (the max rule's is the largest term of it), and the driver
// sets that rule for a gain run.  --gain-unconditional drops the correction.
//
// The search is the Nelder-Mead of every other fit (optimizer / nm_search), over [lambdas..., mus (--estimate-mu)..., nu], nested
// like -b --family-mu estimate: first the model without nu, then with nu from that optimum (start nu = lambda / 10, or nu held at
// --gain's value).  A Nelder-Mead search never ends above its start, but the second start has nu > 0 and may lie above the
// first optimum; a gain fit that ends above the nu = 0 fit is therefore replaced by it, so the gain fit is never worse than the
// fit it extends and the likelihood-ratio statistic is never negative.
#include "cafe_host.h"

#include <cmath>
#include <iomanip>
#include <limits>
#include <ostream>

namespace cafe {

gain_table gain_distinct_families(const std::vector<gene_family>& fams) {
    gain_table t;
    std::map<std::string, size_t> seen;
    for (size_t f = 0; f < fams.size(); ++f) {
        std::string key;
        for (const std::string& sp : fams[f].get_species()) key += sp + ':' + std::to_string(fams[f].get_species_size(sp)) + ',';
        const auto it = seen.emplace(key, t.family.size());
        if (it.second) { t.family.push_back((int64_t)f); t.weight.push_back(0.0); }
        t.weight[it.first->second] += 1.0;
    }
    t.n_families = (double)fams.size();
    t.family.push_back(kFamilyAbsent);
    t.weight.push_back(0.0);
    return t;
}

bool gain_layout::unpack(const double* x, std::vector<double>& lambdas, std::vector<double>& mus, double& nu) const {
    int at = 0;
    lambdas = fixed_lambdas;
    if (lambdas_free) { lambdas.assign(x, x + L); at += L; }
    mus = fixed_mus.empty() ? lambdas : fixed_mus;
    if (mus_free) { mus.assign(x + at, x + at + L); at += L; }
    nu = nu_free ? x[at] : fixed_nu;
    if ((int)lambdas.size() != L || (int)mus.size() != L) return false;
    for (int i = 0; i < L; ++i)
        if (!(lambdas[i] >= 0) || !(mus[i] >= 0) || (L == 1 && !(lambdas[i] > 0))) return false;
    return nu >= 0;
}

std::vector<double> gain_layout::pack(const std::vector<double>& lambdas, const std::vector<double>& mus, double nu) const {
    std::vector<double> x;
    if (lambdas_free) x.insert(x.end(), lambdas.begin(), lambdas.end());
    if (mus_free) x.insert(x.end(), mus.begin(), mus.end());
    if (nu_free) x.push_back(nu);
    return x;
}

double gain_objective(const std::vector<double>& lnl, const gain_table& table, bool conditional) {
    const double inf = std::numeric_limits<double>::infinity();
    if (lnl.size() != table.family.size() || lnl.empty()) throw std::runtime_error("gain_objective: one value per entry of the table is required");
    double total = 0;
    for (size_t i = 0; i + 1 < lnl.size(); ++i) {
        if (std::isnan(lnl[i]) || lnl[i] == -inf) return inf;
        total -= table.weight[i] * lnl[i];
    }
    if (!conditional) return total;
    const double absent = lnl.back();                           // log P(no species shows the family)
    if (std::isnan(absent) || absent >= 0) return inf;           // a model under which no family is ever seen
    return total + table.n_families * std::log(-std::expm1(absent));       // log(1 - exp(absent)) without the cancellation as absent -> 0-
}

namespace {

struct gain_search_scorer : optimizer_scorer {
    const gain_scorer& score;
    const gain_table& table;
    const gain_layout& layout;
    bool conditional;
    std::vector<double> start;
    int calls = 0;
    gain_search_scorer(const gain_scorer& s, const gain_table& t, const gain_layout& l, bool cond) : score(s), table(t), layout(l), conditional(cond) {}
    std::vector<double> initial_guesses() override { return start; }
    double calculate_score(const double* x) override {
        std::vector<double> lambdas, mus;
        double nu = 0;
        if (!layout.unpack(x, lambdas, mus, nu)) return std::numeric_limits<double>::infinity();
        ++calls;
        return gain_objective(score(lambdas, mus, nu), table, conditional);
    }
};

gain_fit search(const gain_scorer& score, const gain_table& table, const gain_layout& layout, const gain_options& opt, const std::vector<double>& start,
                const std::function<std::vector<double>()>* redraw) {
    gain_search_scorer sc(score, table, layout, opt.conditional);
    std::vector<double> best = start;
    double best_score = 0;
    if (layout.width() > 0) {
        sc.start = start;
        for (int attempt = 0; redraw && std::isinf(sc.calculate_score(sc.start.data())); ++attempt) {       // NUM_OPTIMIZER_INITIALIZATION_ATTEMPTS
            if (attempt >= 100) throw std::runtime_error("Failed to initialize any reasonable values");
            sc.start = (*redraw)();
        }
        optimizer o(&sc);
        o.max_iterations = opt.max_iterations;
        o.similarity_window = 0;                                 // the high-precision stop rule (tolx, tolf) alone: the two fits are compared
        o.start = sc.start;
        const optimizer_result r = o.optimize();
        best = r.values;
        best_score = r.score;
    } else {
        best_score = sc.calculate_score(nullptr);
    }
    gain_fit fit;
    if (!layout.unpack(best.data(), fit.lambdas, fit.mus, fit.nu)) throw std::runtime_error("the gain search ended at rates out of range");
    fit.lnl = score(fit.lambdas, fit.mus, fit.nu);
    fit.neg_lnl = gain_objective(fit.lnl, table, opt.conditional);
    fit.p_absent = std::exp(fit.lnl.back());
    fit.calls = sc.calls + 1;
    fit.start = layout.width() > 0 ? sc.start : std::vector<double>();
    (void)best_score;
    return fit;
}

}  // namespace

gain_result fit_gain_model(const gain_scorer& score, const gain_table& table, int n_lambdas, const gain_options& opt,
                           const std::function<std::vector<double>()>& draw_lambdas) {
    if (!(opt.root_absent >= 0 && opt.root_absent <= 1)) throw std::runtime_error("--root-absent: P0 must lie in [0, 1]");
    if (!opt.estimate_nu && !(opt.fixed_nu >= 0)) throw std::runtime_error("--gain: NU must not be negative");
    if (!opt.fixed_lambdas.empty() && (int)opt.fixed_lambdas.size() != n_lambdas) throw std::runtime_error("the gain model needs one lambda per lambda index (" + std::to_string(n_lambdas) + ")");
    if (!opt.fixed_mus.empty() && (int)opt.fixed_mus.size() != n_lambdas) throw std::runtime_error("--mu needs one death rate per lambda (" + std::to_string(n_lambdas) + ")");
    gain_layout layout;
    layout.L = n_lambdas;
    layout.lambdas_free = opt.fixed_lambdas.empty();
    layout.mus_free = opt.estimate_mu;
    layout.fixed_lambdas = opt.fixed_lambdas;
    layout.fixed_mus = opt.fixed_mus;

    gain_result res;
    std::function<std::vector<double>()> redraw = [&] {
        const std::vector<double> lam = layout.lambdas_free ? draw_lambdas() : opt.fixed_lambdas;
        return layout.pack(lam, lam, 0.0);                      // a searched mu starts at its lambda
    };
    res.without = search(score, table, layout, opt, redraw(), layout.lambdas_free ? &redraw : nullptr);

    gain_layout extended = layout;
    extended.nu_free = opt.estimate_nu;
    extended.fixed_nu = opt.fixed_nu;
    double nu0 = opt.fixed_nu;
    if (opt.estimate_nu) nu0 = *std::max_element(res.without.lambdas.begin(), res.without.lambdas.end()) / 10;
    res.with = search(score, table, extended, opt, extended.pack(res.without.lambdas, res.without.mus, nu0), nullptr);
    if (opt.estimate_nu && !(res.with.neg_lnl <= res.without.neg_lnl)) {      // the nested model's optimum is a point of this model
        const int calls = res.with.calls;
        res.with = res.without;
        res.with.calls = calls;
    }
    res.lr_statistic = 2 * (res.without.neg_lnl - res.with.neg_lnl);
    return res;
}

const char* gain_refusal(const gain_request& r) {
    if (!r.gain && !r.estimate_gain) {
        if (r.root_absent_given) return "--root-absent sets the root's mass at size 0 under the gain model: give --gain NU or --estimate-gain with it";
        if (r.unconditional) return "--gain-unconditional belongs to the gain model: give --gain NU or --estimate-gain with it";
        if (r.posterior) return "--gain-posterior reports where families originated under the gain model: give --gain NU or --estimate-gain with it";
        return nullptr;
    }
    if (r.gain && r.estimate_gain) return "--gain fixes the gain rate and --estimate-gain searches it: give one of the two";
    if (r.gain && !(r.nu >= 0)) return "--gain: NU must not be negative";
    if (!(r.root_absent >= 0 && r.root_absent <= 1)) return "--root-absent: P0 must lie in [0, 1]";
    if (r.gamma) return "the gain model is fitted under the base model: -k > 1 and -a are not supported with --gain / --estimate-gain";
    if (r.per_family) return "the gain model shares its rates over the table: -b is not supported with --gain / --estimate-gain";
    if (r.gpus) return "the gain model runs on one GPU: --gpus is not supported with --gain / --estimate-gain";
    if (r.simulate) return "the simulator has no gain rate: --simulate is not supported with --gain / --estimate-gain";
    if (r.pvalues) return "--pvalues simulates without a gain rate: it is not supported with --gain / --estimate-gain";
    if (r.reconstruct || r.marginal || r.histories) return "the reconstructions are not ported to the gain model: --reconstruct, --reconstruct-marginal and --sample-histories are not supported with --gain / --estimate-gain";
    if (r.standard_errors || r.events || r.rate_shift || r.leaf_predictive || r.branch_change || r.rootdist_em)
        return "the posterior reports are not ported to the gain model: --standard-errors, --expected-events, --rate-shift-scan, --leaf-predictive, --branch-change and --estimate-rootdist are not supported with --gain / --estimate-gain";
    if (r.search_batch) return "the gain search scores one point per call: --search-batch is not supported with --gain / --estimate-gain";
    if (r.estimate_error) return "the gain model needs an error model file: -e without FILE (estimating epsilon) is not supported with --gain / --estimate-gain";
    return nullptr;
}

void write_gain_results(std::ostream& ost, const gain_result& res, const gain_options& opt, const gain_table& table) {
    auto list = [&](const std::vector<double>& v) {
        for (size_t i = 0; i < v.size(); ++i) ost << (i ? "," : "") << v[i];
        ost << "\n";
    };
    ost << std::setprecision(17);
    ost << "Model Gain Final Likelihood (-lnL): " << res.with.neg_lnl << "\n";
    ost << "Lambda: "; list(res.with.lambdas);
    ost << "Mu: "; list(res.with.mus);
    ost << "Nu: " << res.with.nu << "\n";
    ost << "r (Nu / Lambda): ";
    std::vector<double> r;
    for (double l : res.with.lambdas) r.push_back(res.with.nu / l);
    list(r);
    ost << "Root absent: " << opt.root_absent << "\n";
    ost << "Root rule: sum\n";
    ost << "Likelihood: " << (opt.conditional ? "conditional on the family being seen in at least one species" : "unconditional") << "\n";
    ost << "P(absent): " << res.with.p_absent << "\n";
    ost << "Families: " << table.n_families << " (" << table.family.size() - 1 << " distinct)\n";
    ost << "Without gain (-lnL): " << res.without.neg_lnl << "\n";
    ost << "Without gain Lambda: "; list(res.without.lambdas);
    ost << "Without gain Mu: "; list(res.without.mus);
    ost << "Likelihood ratio statistic: " << res.lr_statistic << "\n";
}

}  // namespace cafe
