// CPU-only unit tests of the gain model's host side (gain_model.cpp): the table of distinct families and its weights, packing
// and unpacking the search vector, the conditional objective (as lnL_absent -> 0- too), the nested search on a mock scorer, the
// refusals and the results file.  No GPU, no HIP library linked.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <sstream>

#include "cafe_host.h"

using namespace cafe;

static int failures = 0, checks = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { ++failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)
#define CLOSE(a, b, tol) CHECK(std::fabs((a) - (b)) <= (tol))

static const double INF = std::numeric_limits<double>::infinity();

static gene_family family(const char* id, int a, int b) {
    gene_family f;
    f.set_id(id);
    f.set_species_size("A", a);
    f.set_species_size("B", b);
    return f;
}

static void test_table() {
    const std::vector<gene_family> fams = {family("f0", 1, 2), family("f1", 0, 3), family("f2", 1, 2), family("f3", 2, 1), family("f4", 1, 2)};
    const gain_table t = gain_distinct_families(fams);
    CHECK(t.family.size() == 4 && t.weight.size() == 4);
    CHECK(t.family[0] == 0 && t.family[1] == 1 && t.family[2] == 3 && t.family[3] == kFamilyAbsent);
    CHECK(t.weight[0] == 3 && t.weight[1] == 1 && t.weight[2] == 1 && t.weight[3] == 0);
    CHECK(t.n_families == 5);
    const gain_table none = gain_distinct_families({});
    CHECK(none.family.size() == 1 && none.family[0] == kFamilyAbsent && none.n_families == 0);
}

static void test_layout() {
    gain_layout l;
    l.L = 2; l.lambdas_free = true; l.mus_free = true; l.nu_free = true;
    CHECK(l.width() == 5);
    const std::vector<double> x = l.pack({0.01, 0.02}, {0.03, 0.04}, 0.005);
    CHECK(x.size() == 5 && x[0] == 0.01 && x[1] == 0.02 && x[2] == 0.03 && x[3] == 0.04 && x[4] == 0.005);
    std::vector<double> lam, mu;
    double nu = -1;
    CHECK(l.unpack(x.data(), lam, mu, nu) && lam == std::vector<double>({0.01, 0.02}) && mu == std::vector<double>({0.03, 0.04}) && nu == 0.005);
    std::vector<double> bad = x;
    bad[4] = -1e-12;                                             // a negative nu, a negative mu, a NaN lambda: out of range, never scored
    CHECK(!l.unpack(bad.data(), lam, mu, nu));
    bad = x; bad[3] = -0.001;
    CHECK(!l.unpack(bad.data(), lam, mu, nu));
    bad = x; bad[0] = NAN;
    CHECK(!l.unpack(bad.data(), lam, mu, nu));
    bad = x; bad[0] = 0.0;                                       // several lambdas: 0 is in range
    CHECK(l.unpack(bad.data(), lam, mu, nu));

    gain_layout tied;                                            // one lambda, mu tied to it, nu searched
    tied.nu_free = true;
    CHECK(tied.width() == 2);
    const double y[2] = {0.02, 0.001};
    CHECK(tied.unpack(y, lam, mu, nu) && lam.size() == 1 && mu == lam && nu == 0.001);
    const double z[2] = {0.0, 0.001};                            // one lambda: it must be positive
    CHECK(!tied.unpack(z, lam, mu, nu));

    gain_layout fixed;                                           // -l and --mu and --gain: nothing to search
    fixed.lambdas_free = false; fixed.fixed_lambdas = {0.01}; fixed.fixed_mus = {0.02}; fixed.fixed_nu = 0.003;
    CHECK(fixed.width() == 0 && fixed.pack({0.01}, {0.02}, 0.003).empty());
    CHECK(fixed.unpack(nullptr, lam, mu, nu) && lam[0] == 0.01 && mu[0] == 0.02 && nu == 0.003);
}

static void test_objective() {
    gain_table t;
    t.family = {0, 1, kFamilyAbsent};
    t.weight = {3, 1, 0};
    t.n_families = 4;
    const double absent = std::log(0.25);
    CLOSE(gain_objective({-2.0, -5.0, absent}, t, false), 11.0, 1e-15);
    CLOSE(gain_objective({-2.0, -5.0, absent}, t, true), 11.0 + 4 * std::log(0.75), 1e-14);
    CHECK(gain_objective({-2.0, -INF, absent}, t, true) == INF);             // an impossible family
    CHECK(gain_objective({-2.0, NAN, absent}, t, false) == INF);
    CHECK(gain_objective({-2.0, -5.0, -INF}, t, true) == 11.0);              // the absent profile impossible: nothing to correct
    // lnL_absent -> 0-: 1 - exp(a) = -expm1(a) ~ -a, no cancellation
    for (double a : {-1e-3, -1e-9, -1e-15, -1e-300}) {
        const double want = 11.0 + 4 * (std::log(-a) + std::log1p(a / 2));          // log(-a (1 + a/2 + ...)), the next term below 1e-6
        const double got = gain_objective({-2.0, -5.0, a}, t, true);
        CHECK(std::isfinite(got));
        CLOSE(got, want, 1e-6 * std::fabs(want));
    }
    CHECK(gain_objective({-2.0, -5.0, 0.0}, t, true) == INF);                // a model that never shows a family
    CHECK(gain_objective({-2.0, -5.0, NAN}, t, true) == INF);
    bool threw = false;
    try { gain_objective({-2.0, -5.0}, t, true); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw);
}

// a smooth mock: families drawn as if from lambda = 0.02, nu = 0.004; the absent profile has probability exp(-50 nu - 10 lambda)
static std::vector<double> mock(const std::vector<double>& lam, const std::vector<double>& mu, double nu) {
    const double a = std::log(lam[0] / 0.02), b = nu > 0 ? std::log(nu / 0.004) : -8.0, c = std::log(mu[0] / lam[0]);
    return {-3.0 - a * a - 0.5 * b * b - c * c, -4.0 - 2 * a * a - b * b - 0.5 * c * c, -50 * nu - 10 * lam[0]};
}

static void test_nested_search() {
    gain_table t;
    t.family = {0, 1, kFamilyAbsent};
    t.weight = {2, 1, 0};
    t.n_families = 3;
    int draws = 0;
    const auto draw = [&] { ++draws; return std::vector<double>{draws == 1 ? -1.0 : 0.05}; };    // the first draw is out of range: redrawn
    gain_options opt;
    opt.estimate_nu = true;
    const gain_result res = fit_gain_model(mock, t, 1, opt, draw);
    CHECK(draws == 2);
    CHECK(res.without.nu == 0 && res.with.nu > 0);
    CHECK(res.with.neg_lnl <= res.without.neg_lnl);
    CLOSE(res.lr_statistic, 2 * (res.without.neg_lnl - res.with.neg_lnl), 1e-12);
    CHECK(res.with.mus == res.with.lambdas);                     // mu tied to lambda
    CLOSE(res.with.neg_lnl, gain_objective(mock(res.with.lambdas, res.with.mus, res.with.nu), t, true), 1e-12);
    CLOSE(res.with.p_absent, std::exp(-50 * res.with.nu - 10 * res.with.lambdas[0]), 1e-12);
    // unconditional: the optimum of the mock is the point it was built around
    opt.conditional = false;
    const gain_result plain = fit_gain_model(mock, t, 1, opt, draw);
    CLOSE(plain.with.lambdas[0], 0.02, 2e-4);
    CLOSE(plain.with.nu, 0.004, 1e-4);
    CLOSE(plain.with.neg_lnl, 10.0, 1e-4);

    // a scorer that punishes every nu > 0: the gain fit falls back to the fit it extends
    const gain_scorer worse = [](const std::vector<double>& lam, const std::vector<double>& mu, double nu) {
        std::vector<double> v = mock(lam, mu, 0.004);
        v[0] -= 1000 * nu; v[1] -= 1000 * nu;
        return v;
    };
    const gain_result back = fit_gain_model(worse, t, 1, opt, draw);
    CHECK(back.with.neg_lnl <= back.without.neg_lnl && back.lr_statistic >= 0);

    // --gain NU with -l and --mu: nothing is searched, one evaluation each
    gain_options fixed;
    fixed.fixed_nu = 0.004; fixed.fixed_lambdas = {0.02}; fixed.fixed_mus = {0.02}; fixed.conditional = false;
    const gain_result f = fit_gain_model(mock, t, 1, fixed, draw);
    CLOSE(f.with.neg_lnl, 10.0, 1e-12);
    CHECK(f.with.nu == 0.004 && f.without.nu == 0);
    CLOSE(f.without.neg_lnl, 2 * (3.0 + 32.0) + 4.0 + 64.0, 1e-12);

    // --estimate-mu: [lambda, mu, nu]
    gain_options three;
    three.estimate_nu = three.estimate_mu = true; three.conditional = false;
    const gain_result m = fit_gain_model(mock, t, 1, three, draw);
    CHECK(m.with.neg_lnl <= m.without.neg_lnl && m.with.mus.size() == 1);
    bool threw = false;
    gain_options bad;
    bad.root_absent = 1.5;
    try { fit_gain_model(mock, t, 1, bad, draw); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw);
}

static void test_refusals() {
    gain_request none;
    CHECK(gain_refusal(none) == nullptr);
    none.root_absent_given = true;
    CHECK(std::strstr(gain_refusal(none), "--root-absent"));
    gain_request r;
    r.estimate_gain = true;
    CHECK(gain_refusal(r) == nullptr);
    r.root_absent = 0.3; r.root_absent_given = true;
    CHECK(gain_refusal(r) == nullptr);
    const struct { bool gain_request::*flag; const char* word; } cases[] = {
        {&gain_request::gamma, "-k"}, {&gain_request::per_family, "-b"}, {&gain_request::gpus, "--gpus"}, {&gain_request::simulate, "--simulate"},
        {&gain_request::pvalues, "--pvalues"}, {&gain_request::reconstruct, "--reconstruct"}, {&gain_request::marginal, "--reconstruct-marginal"},
        {&gain_request::histories, "--sample-histories"}, {&gain_request::standard_errors, "--standard-errors"}, {&gain_request::events, "--expected-events"},
        {&gain_request::rate_shift, "--rate-shift-scan"}, {&gain_request::leaf_predictive, "--leaf-predictive"}, {&gain_request::branch_change, "--branch-change"},
        {&gain_request::rootdist_em, "--estimate-rootdist"}, {&gain_request::search_batch, "--search-batch"}, {&gain_request::estimate_error, "-e"},
    };
    for (const auto& c : cases) {
        gain_request q = r;
        q.*(c.flag) = true;
        const char* why = gain_refusal(q);
        CHECK(why && std::strstr(why, c.word) && std::strstr(why, "--gain / --estimate-gain"));
    }
    gain_request both = r;
    both.gain = true;
    CHECK(std::strstr(gain_refusal(both), "one of the two"));
    gain_request neg;
    neg.gain = true; neg.nu = -0.1;
    CHECK(std::strstr(gain_refusal(neg), "NU must not be negative"));
    neg.nu = NAN;
    CHECK(gain_refusal(neg) != nullptr);
    gain_request p0 = r;
    p0.root_absent = 1.2;
    CHECK(std::strstr(gain_refusal(p0), "[0, 1]"));
}

static void test_results_file() {
    gain_result res;
    res.with.lambdas = {0.01, 0.02}; res.with.mus = {0.03, 0.04}; res.with.nu = 0.005; res.with.neg_lnl = 100.5; res.with.p_absent = 0.125;
    res.without.lambdas = {0.011, 0.021}; res.without.mus = {0.011, 0.021}; res.without.neg_lnl = 104.0;
    res.lr_statistic = 7.0;
    gain_options opt;
    opt.root_absent = 0.25;
    gain_table t;
    t.family = {0, 1, kFamilyAbsent}; t.weight = {2, 1, 0}; t.n_families = 3;
    std::ostringstream ost;
    write_gain_results(ost, res, opt, t);
    const std::string s = ost.str();
    for (const char* line : {"Model Gain Final Likelihood (-lnL): 100.5\n", "Lambda: 0.01,0.02\n", "Mu: 0.029999999999999999,0.040000000000000001\n", "Nu: 0.0050000000000000001\n",
                             "r (Nu / Lambda): 0.5,0.25\n", "Root absent: 0.25\n", "Root rule: sum\n", "Likelihood: conditional on the family being seen in at least one species\n",
                             "P(absent): 0.125\n", "Families: 3 (2 distinct)\n", "Without gain (-lnL): 104\n", "Likelihood ratio statistic: 7\n"})
        CHECK(s.find(line) != std::string::npos);
}

int main() {
    test_table();
    test_layout();
    test_objective();
    test_nested_search();
    test_refusals();
    test_results_file();
    std::printf("gain_tests: %d checks, %d failures\n", checks, failures);
    if (failures == 0) std::printf("gain_tests: all passed\n");
    return failures ? 1 : 0;
}
