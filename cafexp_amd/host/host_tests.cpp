// CPU-only unit tests of the host adapter (no GPU, no HIP library linked): the reference's own
// test cases for the pieces that stay on the host (test.cpp line cited per test), with mock models
// standing in for the GPU path exactly as test.cpp:37-86 mocks `model`.
#include <cmath>
#include <cstdio>
#include <iostream>
#include <limits>
#include <sstream>

#include "cafe_host.h"

using namespace cafe;

static int failures = 0, checks = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { ++failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)
#define CLOSE(a, b, tol) CHECK(std::fabs((a) - (b)) <= (tol))

struct mock_model : public model {                       // test.cpp:37-86
    double value;
    int calls = 0;
    explicit mock_model(double v) : model(nullptr, nullptr, nullptr, 0, 0, nullptr), value(v) {}
    double infer_family_likelihoods(root_equilibrium_distribution*, const std::map<int, int>&, const lambda*) override { ++calls; return value; }
    std::string name() const override { return "mock"; }
    void write_family_likelihoods(std::ostream&) override {}
    inference_optimizer_scorer* get_lambda_optimizer(user_data&) override { return nullptr; }
};

struct quadratic_scorer : public optimizer_scorer {      // stands in for test.cpp:2289 mock_scorer
    int calls = 0;
    std::vector<double> initial_guesses() override { return {0.3, -0.2}; }
    double calculate_score(const double* v) override { ++calls; return 5 + (v[0] - 1.25) * (v[0] - 1.25) + 3 * (v[1] + 0.5) * (v[1] + 0.5); }
};
struct inf_scorer : public optimizer_scorer {
    std::vector<double> initial_guesses() override { return {0.1}; }
    double calculate_score(const double*) override { return std::numeric_limits<double>::infinity(); }
};

static void test_newick() {
    std::unique_ptr<clade> t(parse_newick("(A:1,B:3):7"));                       // test.cpp:1642
    CHECK(t->descendants().size() == 2 && t->get_taxon_name() == "AB" && t->get_branch_length() == 7);
    auto bl = t->get_branch_lengths();
    CHECK(bl.size() == 3 && bl.count(7.0) == 1);
    std::unique_ptr<clade> u(parse_newick("((E:0.36,D:0.30)abc:1.00,(C:0.85,(A:0.59,B:0.35):0.42):0.39);"));
    CHECK(u->leaves().size() == 5 && u->find_descendant("AB") != nullptr && u->get_taxon_name() == "ABCDE");
    std::vector<std::string> order;                                               // children before parents
    u->apply_reverse_level_order([&](const clade* c) { order.push_back(c->get_taxon_name()); });
    CHECK(order.back() == "ABCDE" && order.size() == 9);
    bool threw = false;
    try { std::unique_ptr<clade> bad(parse_newick("(A:1,B:0);")); } catch (std::runtime_error&) { threw = true; }
    CHECK(threw);
    std::unique_ptr<clade> l(parse_newick("((A:1,B:1):2,C:1);", true));          // lambda tree: index map is index-1
    auto m = l->get_lambda_index_map();
    CHECK(m["A"] == 0 && m["AB"] == 1 && m["ABC"] == 0 && l->get_lambda_index() == 1);
    threw = false;
    try { l->get_branch_length(); } catch (std::runtime_error&) { threw = true; }
    CHECK(threw);
}

static void test_families_and_sizes() {
    std::istringstream in("Desc\tFamily ID\tA\tB\n\t (null)1\t5\t10\n\t (null)2\t5\t7\n\t (null)3\t5\t10\n\t (null)4\t5\t7\n");   // test.cpp:1626
    std::vector<gene_family> fams;
    read_gene_families(in, nullptr, fams);
    CHECK(fams.size() == 4 && fams[0].get_species_size("a") == 5 && fams[0].get_species_size("B") == 10);
    CHECK(fams[0].species_size_match(fams[2]) && !fams[0].species_size_match(fams[1]));
    int M = -1, R = -1;
    compute_max_sizes(fams, M, R);
    CHECK(M == 60 && R == 30);
    gene_family big;
    big.set_species_size("x", 90);
    std::vector<gene_family> one{big};
    M = R = -1;
    compute_max_sizes(one, M, R);
    CHECK(M == 140 && R == 112);
    std::unique_ptr<clade> t(parse_newick("((A:1,B:1):1,(C:1,D:1):1);"));
    gene_family f;
    f.set_species_size("A", 1); f.set_species_size("B", 0); f.set_species_size("C", 0); f.set_species_size("D", 0);
    CHECK(!f.exists_at_root(t.get()));
    f.set_species_size("D", 2);
    CHECK(f.exists_at_root(t.get()));
}

static void test_error_model() {
    std::istringstream in("maxcnt: 20\ncntdiff: -1 0 1\n0 0.0 0.8 0.2\n1 0.2 0.6 0.2\n20 0.2 0.6 0.2\n");               // test.cpp:1745
    error_model em;
    read_error_model_file(in, &em);
    CHECK(em.n_deviations() == 3 && em.get_max_family_size() == 21);
    CHECK(em.get_probs(3) == std::vector<double>({0.2, 0.6, 0.2}) && em.get_probs(0) == std::vector<double>({0.0, 0.8, 0.2}));
    // lambda_epsilon_optimizer (test.cpp:2178): rows {0,.94,.06} / {.06,.88,.06} style replacement by value
    error_model e2;
    e2.set_probabilities(0, {.0, .7, .3});
    e2.set_probabilities(1, {.4, .2, .4});
    mock_model m(0.0);
    single_lambda lam(0.05);
    uniform_distribution prior;
    std::map<int, int> rd;
    lambda_epsilon_optimizer opt(&m, &e2, &prior, rd, &lam, 10);
    opt.initial_guesses();
    std::vector<double> values = {0.05, 0.06, 0.04};                     // lambda, then epsilons in sorted order (.3 -> .06, .4 -> .04)
    opt.calculate_score(values.data());
    CHECK(e2.get_probs(0) == std::vector<double>({0, .94, .06}));
    CHECK(e2.get_probs(1) == std::vector<double>({.04, .92, .04}));
    bool threw = false;
    try { error_model bad; bad.set_probabilities(0, {0.1, 0.8, 0.1}); } catch (std::runtime_error&) { threw = true; }
    CHECK(threw);
}

static void test_priors_and_gamma() {
    root_distribution rd;
    rd.vectorize_uniform(10);
    uniform_distribution u;
    u.initialize(&rd);
    CLOSE(u.compute(5), 0.1, 1e-4);                                      // test.cpp:549
    CHECK(u.compute(10) == 0);
    root_distribution r112;
    r112.vectorize_uniform(112);
    u.initialize(&r112);
    CHECK((double)u.compute(0) == 0.0089285718277096748);                // float(1)/float(112)
    std::vector<double> probs(4), mult(4);
    get_gamma(probs, mult, 0.25);                                        // SURVEY 8c oracle values (compiled reference)
    CLOSE(mult[0], 0.0021117569167044, 1e-15);
    CLOSE(mult[1], 0.06668995694102, 1e-14);
    CLOSE(mult[2], 0.50148567146622, 1e-13);
    CLOSE(mult[3], 3.4297126146761, 1e-12);
    CHECK(probs[0] == 0.25 && probs[3] == 0.25);
}

static void test_scorers() {
    // NaN from the model becomes +inf (test.cpp:2250)
    mock_model nan_model(std::nan(""));
    single_lambda lam(0.05);
    uniform_distribution prior;
    std::map<int, int> rd;
    lambda_optimizer opt(&lam, &nan_model, &prior, 7, rd);
    double v = 0.05;
    CHECK(std::isinf(opt.calculate_score(&v)));
    // lambda_optimizer plumbs the value into the lambda object; initial guess is positive
    mock_model ok(1000.0);
    lambda_optimizer o2(&lam, &ok, &prior, 10, rd);
    double v2 = 0.0123;
    CHECK(o2.calculate_score(&v2) == 1000.0 && lam.get_single_lambda() == 0.0123);
    randomizer_engine.seed(10);
    auto g = o2.initial_guesses();
    CHECK(g.size() == 1 && g[0] > 0);
    // multiple lambda validity (test.cpp:1915) and lookup by node name
    std::map<std::string, int> idx{{"A", 0}, {"B", 1}, {"AB", 0}};
    multiple_lambda ml(idx, {0.03, 0.05});
    std::unique_ptr<clade> t(parse_newick("(A:1,B:2);"));
    CHECK(ml.get_value_for_clade(t->find_descendant("B")) == 0.05 && ml.is_valid());
    double neg[2] = {0.01, -0.01};
    ml.update(neg);
    CHECK(!ml.is_valid());
    single_lambda zero(0.0);
    CHECK(!zero.is_valid());
}

static void test_optimizer() {
    quadratic_scorer q;
    optimizer o(&q);
    o.similarity_window = 0;
    auto r = o.optimize();
    CLOSE(r.values[0], 1.25, 1e-4);
    CLOSE(r.values[1], -0.5, 1e-4);
    CLOSE(r.score, 5.0, 1e-8);
    CHECK(r.num_scorer_calls == q.calls && r.num_iterations > 10);
    inf_scorer bad;
    optimizer ob(&bad);
    bool threw = false;
    try { ob.optimize(); } catch (std::runtime_error&) { threw = true; }   // OptimizerInitializationFailure after 100 retries
    CHECK(threw);
}

static void test_pvalue() {                                   // test.cpp:1175-1183
    std::vector<double> cd(10);
    double n = 0;
    for (auto& x : cd) x = (n += 0.01);
    CLOSE(pvalue(0.05, cd), 0.5, 0.001);
    CLOSE(pvalue(0.0001, cd), 0.0, 0.001);
    CLOSE(pvalue(0.099, cd), 0.9, 0.001);
    CHECK(pvalue(1.0, cd) == 0.9);                            // beyond the last entry: index size-1, not size
}

// report writers of the reconstruction classes: the reference's own expectations
static void test_reconstruction_reports() {
    std::unique_ptr<clade> p_tree(parse_newick("((A:1,B:3):7,(C:11,D:17):23);"));           // TEST_GROUP(Reconstruction), test.cpp:865
    gene_family fam;
    fam.set_id("Family5");
    fam.set_species_size("A", 11); fam.set_species_size("B", 2); fam.set_species_size("C", 5); fam.set_species_size("D", 6);
    cladevector order;
    for (const char* nm : {"A", "B", "C", "D", "AB", "CD", "ABCD"}) order.push_back(p_tree->find_descendant(nm));
    const std::vector<gene_family> fams{fam};
    {   // test.cpp:912 star for significant values, root never significant
        base_model_reconstruction bmr;
        auto& values = bmr._reconstructions["Family5"];
        values[p_tree.get()] = 7; values[p_tree->find_descendant("AB")] = 8; values[p_tree->find_descendant("CD")] = 6;
        branch_probabilities bp;
        p_tree->apply_reverse_level_order([&](const clade* c) { bp.set(fam, c, branch_probabilities::branch_probability(.5)); });
        bp.set(fam, p_tree->find_descendant("AB"), 0.02);
        bp.set(fam, p_tree.get(), branch_probabilities::invalid());
        std::ostringstream sig, insig, plain;
        bmr.print_reconstructed_states(sig, order, fams, p_tree.get(), 0.05, bp);
        CHECK(sig.str().find("  TREE Family5 = ((A<0>_11:1,B<1>_2:3)<4>*_8:7,(C<2>_5:11,D<3>_6:17)<5>_6:23)<6>_7;") != std::string::npos);
        bmr.print_reconstructed_states(insig, order, fams, p_tree.get(), 0.01, bp);
        CHECK(insig.str().find("  TREE Family5 = ((A<0>_11:1,B<1>_2:3)<4>_8:7,(C<2>_5:11,D<3>_6:17)<5>_6:23)<6>_7;") != std::string::npos);
        branch_probabilities none;                                                       // test.cpp:993
        bmr.print_reconstructed_states(plain, order, fams, p_tree.get(), 0.05, none);
        CHECK(plain.str().find("#nexus\nBEGIN TREES;\n  TREE Family5 = ((A<0>_11:1,B<1>_2:3)<4>_8:7,(C<2>_5:11,D<3>_6:17)<5>_6:23)<6>_7;\n\nEND;\n") == 0);
        std::ostringstream fr, fr2, empty;                                               // test.cpp:2032-2083
        bmr.print_increases_decreases_by_family(fr, order, fams, {0.03}, 0.01);
        CHECK(fr.str() == "#FamilyID\tpvalue\tSignificant at 0.01\nFamily5\t0.03\tn\n");
        bmr.print_increases_decreases_by_family(fr2, order, fams, {0.07}, 0.00001);
        CHECK(fr2.str().find("#FamilyID\tpvalue\tSignificant at 1e-05\n") == 0);
        bmr.print_increases_decreases_by_family(empty, order, {}, {}, 0.05);
        CHECK(empty.str() == "No increases or decreases recorded\n");
        std::ostringstream cl;                                                           // test.cpp:2146: increases / decreases per clade
        bmr.print_increases_decreases_by_clade(cl, order, fams);
        CHECK(cl.str().find("#Taxon_ID\tIncrease\tDecrease\n") == 0 && cl.str().find("A<0>\t1\t0\n") != std::string::npos &&
              cl.str().find("B<1>\t0\t1\n") != std::string::npos && cl.str().find("<4>\t1\t0\n") != std::string::npos);
        CHECK(bmr.reconstructed_size(fam, p_tree->find_descendant("AB")) == 8 && bmr.reconstructed_size(fam, p_tree->find_descendant("A")) == 11);
    }
    {   // gamma: test.cpp:937, :957, :967, :1079
        gamma_model_reconstruction gmr(std::vector<double>({0.13, 1.4}));
        auto& rec = gmr._reconstructions["Family5"];
        rec.reconstruction[p_tree.get()] = 7; rec.reconstruction[p_tree->find_descendant("AB")] = 8; rec.reconstruction[p_tree->find_descendant("CD")] = 6;
        branch_probabilities none;
        std::ostringstream ost;
        gmr.print_reconstructed_states(ost, order, fams, p_tree.get(), 0.05, none);
        CHECK(ost.str().find("  TREE Family5 = ((A<0>_11:1,B<1>_2:3)<4>_8:7,(C<2>_5:11,D<3>_6:17)<5>_6:23)<6>_7;") != std::string::npos);
        CHECK(ost.str().find("\nBEGIN LAMBDA_MULTIPLIERS;\n  0.13;\n  1.4;\nEND;\n\n") != std::string::npos);
        gamma_model_reconstruction g4(std::vector<double>({0.3, 0.9, 1.4, 2.0}));
        g4._reconstructions["Family5"]._category_likelihoods = {0.01, 0.03, 0.09, 0.07};
        std::ostringstream cl;
        g4.print_category_likelihoods(cl, order, fams);
        CHECK(cl.str() == "Family ID\t0.3\t0.9\t1.4\t2\t\nFamily5\t0.01\t0.03\t0.09\t0.07\t\n");
        gamma_model_reconstruction g5(std::vector<double>({.5}));
        p_tree->apply_prefix_order([&](const clade* c) { g5._reconstructions["Family5"].reconstruction[c] = 5; });
        std::ostringstream nc;
        g5.print_node_counts(nc, order, fams, p_tree.get());
        CHECK(nc.str() == "FamilyID\tA<0>\tB<1>\tC<2>\tD<3>\t<4>\t<5>\t<6>\nFamily5\t11\t2\t5\t6\t5\t5\t5\n");
        std::ostringstream ch;
        g5.print_node_change(ch, order, fams, p_tree.get());
        CHECK(ch.str() == "FamilyID\tA<0>\tB<1>\tC<2>\tD<3>\t<4>\t<5>\t<6>\nFamily5\t+6\t-3\t+0\t+1\t+0\t+0\t+0\n");
    }
    {   // test.cpp:1061 weighted averages; :1109-1118 names; :1120-1143 branch probability table
        clade c1, c2;
        std::map<const clade*, int> rc1{{&c1, 10}, {&c2, 2}}, rc2{{&c1, 20}, {&c2, 8}};
        auto avg = get_weighted_averages({rc1, rc2}, {.25, .75});
        CLOSE(avg[&c1], 17.5, 1e-12);
        CLOSE(avg[&c2], 6.5, 1e-12);
        CHECK(clade_index_or_name(p_tree.get(), {p_tree.get()}) == "<0>");
        auto a = p_tree->find_descendant("A");
        CHECK(clade_index_or_name(a, {p_tree.get(), a}) == "A<1>");
        branch_probabilities probs;
        for (auto c : order) probs.set(fam, c, 0.05);
        probs.set(fam, p_tree->find_descendant("B"), branch_probabilities::invalid());
        probs.set(fam, p_tree.get(), branch_probabilities::invalid());
        std::ostringstream ost, skip;
        print_branch_probabilities(ost, order, fams, probs);
        CHECK(ost.str() == "#FamilyID\tA<0>\tB<1>\tC<2>\tD<3>\t<4>\t<5>\t<6>\t\nFamily5\t0.05\tN/A\t0.05\t0.05\t0.05\t0.05\tN/A\n");
        branch_probabilities nothing;
        print_branch_probabilities(skip, order, fams, nothing);
        CHECK(skip.str().find("Family5") == std::string::npos);
        bool threw = false;
        try { branch_probabilities::branch_probability bad(1.5); (void)bad; } catch (std::runtime_error&) { threw = true; }
        CHECK(threw);
    }
}

static void test_poisson_scorer() {                           // test.cpp:2270-2287 (fixture: A=1, B=2)
    std::vector<gene_family> fams(1);
    fams[0].set_id("TestFamily1"); fams[0].set_species_size("A", 1); fams[0].set_species_size("B", 2);
    double lambda = 0.05;
    poisson_scorer s1(fams);
    CLOSE(s1.lnLPoisson(&lambda), 3.095732, 1e-4);
    fams.resize(2);
    fams[1].set_id("TestFamily2"); fams[1].set_species_size("A", 3); fams[1].set_species_size("B", 175);
    poisson_scorer s2(fams);
    CLOSE(s2.lnLPoisson(&lambda), 9.830344, 1e-4);           // the 175 is incalculable at this rate and skipped
    fams[1].set_species_size("B", 4);
    randomizer_engine.seed(7);                                // (the fit starts from a random guess: one start in twenty ends 1e-3 off)
    poisson_distribution fitted(&fams);                       // maximum likelihood of a Poisson on sizes-1 = their mean
    CLOSE(fitted.poisson_lambda(), (0 + 1 + 2 + 3) / 4.0, 1e-3);
}

// ---------------------------------------------------------------- the driver's command line (driver_options.cpp)
static driver_options parsed(std::vector<std::string> words, bool* ok = nullptr) {
    words.insert(words.begin(), "cafexp_hip");
    std::vector<char*> argv;
    for (std::string& w : words) argv.push_back(&w[0]);
    driver_options o;
    const bool good = parse_options((int)argv.size(), argv.data(), o);
    if (ok) *ok = good;
    return o;
}
static driver_options estimation(std::vector<std::string> more) {        // "-t x -i y" and the rest
    more.insert(more.begin(), {"-t", "x", "-i", "y"});
    return parsed(more);
}
static bool refused(const driver_options& o, const std::string& why) {
    const char* got = driver_refusal(o);
    if (got && got != driver_usage_exit && why == got) return true;
    std::printf("  refusal: got \"%s\", expected \"%s\"\n", got ? got : "(none)", why.c_str());
    return false;
}

static void test_parse_options() {
    bool ok = false;
    driver_options o = parsed({"-t", "T", "-i", "F", "--estimate-rootdist", "-e", "--sizes", "40,30", "-s", "7", "--branch-change", "-P", "0.1"}, &ok);
    CHECK(ok && o.tree_path == "T" && o.fam_path == "F");
    CHECK(o.estimate_rootdist && o.root_sum && o.rootdist_rounds == 10);         // --estimate-rootdist implies --root-sum
    CHECK(o.use_err && o.err_path.empty());                                      // -e without FILE: epsilon is estimated
    CHECK(o.force_m == 40 && o.force_r == 30 && o.have_seed && o.seed == 7);
    CHECK(o.do_branch_change && o.branch_change_band == 10 && o.test_pvalue == 0.1);      // -P is not read as D
    o = parsed({"--estimate-rootdist", "3", "-e", "E", "--branch-change", "4", "--simulate", "--reconstruct-marginal", "0.5"}, &ok);
    CHECK(ok && o.rootdist_rounds == 3 && o.err_path == "E" && o.branch_change_band == 4 && o.simulate_n == 0 && o.marginal_level == 0.5);
    const driver_options defaults;
    CHECK(defaults.simulate_n == -1 && defaults.k == 1 && defaults.max_iter == 300 && defaults.n_gpus == 1 && defaults.reps == 1 && defaults.limit == -1);
    CHECK(defaults.fixed_alpha == -1 && defaults.marginal_level == 0.95 && defaults.test_pvalue == 0.05 && defaults.history_seed == 1 && defaults.search_batch == 1);
    parsed({"-t", "T", "--no-such-option"}, &ok);
    CHECK(!ok);                                                                  // the usage exit: an unknown option ...
    parsed({"-t", "T", "-i"}, &ok);
    CHECK(!ok);                                                                  // ... and an option without its value
    parsed({"--sizes"}, &ok);
    CHECK(!ok);
    CHECK(driver_refusal(parsed({"-i", "y"})) == driver_usage_exit && driver_refusal(parsed({"-t", "x"})) == driver_usage_exit);
    CHECK(driver_refusal(parsed({"--simulate", "-i", "y", "--standard-errors"})) == driver_usage_exit);      // before the --simulate refusals
    CHECK(driver_refusal(estimation({})) == nullptr && driver_refusal(parsed({"-t", "x", "--simulate", "5"})) == nullptr);
}

static void test_driver_refusals() {
    struct row { const char* flag; std::vector<std::string> args; bool simulate_refuses; };
    const std::vector<row> reports = {
        {"--standard-errors", {"--standard-errors"}, true}, {"--rate-shift-scan", {"--rate-shift-scan"}, true},
        {"--reconstruct-marginal", {"--reconstruct-marginal"}, false}, {"--expected-events", {"--expected-events"}, true},
        {"--leaf-predictive", {"--leaf-predictive"}, true}, {"--branch-change", {"--branch-change"}, true},
        {"--estimate-rootdist", {"--estimate-rootdist"}, false}, {"--sample-histories", {"--sample-histories", "5"}, false},
    };
    for (const row& r : reports) {
        std::vector<std::string> a = r.args;
        a.insert(a.end(), {"--gpus", "2"});
        CHECK(refused(estimation(a), std::string(r.flag) + " runs on one GPU: --gpus is not supported with it"));
        a = r.args; a.push_back("-b");
        CHECK(refused(estimation(a), std::string(r.flag) + " needs one fitted model: -b is not supported with it"));
        a = r.args; a.insert(a.end(), {"-t", "x", "--simulate", "10", "-l", "0.01"});
        if (r.simulate_refuses) CHECK(refused(parsed(a), std::string(r.flag) + " belongs to a fitted model: --simulate is not supported with it"));
        else CHECK(driver_refusal(parsed(a)) == nullptr);        // marginal, rootdist and histories are ignored by --simulate
        CHECK(driver_refusal(estimation(r.args)) == nullptr);
    }
    // the range checks
    CHECK(refused(estimation({"--reconstruct-marginal", "1"}), "--reconstruct-marginal: LEVEL must lie in (0, 1)"));
    CHECK(refused(estimation({"--reconstruct-marginal", "0"}), "--reconstruct-marginal: LEVEL must lie in (0, 1)"));
    driver_options o = estimation({"--branch-change"});
    o.branch_change_band = -1;                                   // (a negative D cannot be typed: it reads as an option)
    CHECK(refused(o, "--branch-change: D must not be negative"));
    CHECK(refused(estimation({"--branch-change", "3", "-P", "1"}), "--branch-change: PVALUE (-P) must lie in (0, 1)"));
    CHECK(refused(estimation({"--branch-change", "-P", "0"}), "--branch-change: PVALUE (-P) must lie in (0, 1)"));
    o = estimation({"--estimate-rootdist"});
    o.rootdist_rounds = -1;
    CHECK(refused(o, "--estimate-rootdist: ROUNDS must not be negative"));
    CHECK(driver_refusal(estimation({"--estimate-rootdist", "0"})) == nullptr);
    CHECK(refused(estimation({"--sample-histories", "0"}), "--sample-histories: N must lie in 1..65536"));
    CHECK(refused(estimation({"--sample-histories", "65537"}), "--sample-histories: N must lie in 1..65536"));
    CHECK(driver_refusal(estimation({"--sample-histories", "65536"})) == nullptr);
    CHECK(refused(estimation({"--sample-histories", "5", "--reconstruct-marginal", "2"}), "--reconstruct-marginal: LEVEL must lie in (0, 1)"));
    o = estimation({"--sample-histories", "5"});
    o.marginal_level = 2;                                        // (LEVEL without --reconstruct-marginal: only the histories read it)
    CHECK(refused(o, "--sample-histories: LEVEL must lie in (0, 1)"));
    CHECK(driver_refusal(estimation({"--leaf-predictive", "-P", "7"})) == nullptr);       // -P is range-checked by --branch-change only
    // the order: of two conflicts the earlier block's text
    CHECK(refused(estimation({"--expected-events", "--gpus", "2", "--standard-errors", "-b"}), "--standard-errors runs on one GPU: --gpus is not supported with it"));
    CHECK(refused(estimation({"--expected-events", "--standard-errors", "-b"}), "--standard-errors needs one fitted model: -b is not supported with it"));
    CHECK(refused(estimation({"-b", "--mu", "0.1", "--search-batch", "1"}), "--search-batch: G must be at least 2"));
    CHECK(refused(estimation({"-b", "--mu", "0.1"}), "-b runs the lambda = mu kernel: --mu / --estimate-mu are not supported with it"));
    CHECK(refused(estimation({"--search-batch", "1", "--standard-errors", "-b", "--gain-scaled"}), "--gain-scaled is the scaled mode of the dense prune: give --gain-dense with it"));
    CHECK(refused(estimation({"--gain", "0.1", "-b", "--mu", "0.1"}), "the gain model shares its rates over the table: -b is not supported with --gain / --estimate-gain"));
    CHECK(refused(parsed({"--gain", "0.1", "--simulate"}), "the simulator has no gain rate: --simulate is not supported with --gain / --estimate-gain"));      // (before the usage exit)
    CHECK(refused(estimation({"--sample-histories", "0", "--branch-change", "--gpus", "2"}), "--branch-change runs on one GPU: --gpus is not supported with it"));
    CHECK(refused(estimation({"-b", "-k", "2", "--family-mu", "0.1", "--estimate-rootdist"}), "--estimate-rootdist needs one fitted model: -b is not supported with it"));
    CHECK(refused(estimation({"--missing", "NA", "--reconstruct", "--mu", "0.1", "--estimate-mu"}),
                  "--reconstruct reads every leaf count: it is not supported on a table with missing cells (--missing / --mask-cells)"));
    // --simulate tries the reports in its own order, behind its own two refusals
    CHECK(refused(parsed({"-t", "x", "--simulate", "--rate-shift-scan", "--expected-events"}), "--expected-events belongs to a fitted model: --simulate is not supported with it"));
    CHECK(refused(parsed({"-t", "x", "--simulate", "--branch-change", "--leaf-predictive"}), "--leaf-predictive belongs to a fitted model: --simulate is not supported with it"));
    CHECK(refused(parsed({"-t", "x", "--simulate", "--standard-errors", "--estimate-mu"}), "--simulate draws under given rates: --estimate-mu is not supported with it (give --mu)"));
    CHECK(refused(parsed({"-t", "x", "--simulate", "--standard-errors", "--family-mu", "0.1"}), "--family-mu sets the death rates of -b: it is not supported without -b"));
    CHECK(refused(parsed({"-t", "x", "--simulate", "--search-batch", "4"}), "--search-batch drives a search: --simulate is not supported with it"));
    CHECK(driver_refusal(parsed({"-t", "x", "--simulate", "-b", "--gpus", "2", "--missing", ",", "--mu", "0.1"})) == nullptr);       // none of the estimation's blocks is tried
    // the other blocks
    CHECK(refused(estimation({"--search-batch", "17", "-k", "2"}), "--search-batch: G x K (the -k categories) must not exceed 32"));
    CHECK(refused(estimation({"--search-batch", "4", "--gpus", "2"}), "--search-batch scores its points in one call on one GPU: --gpus N > 1 is not supported with it"));
    CHECK(refused(estimation({"--search-batch", "4", "-b"}), "--search-batch drives the search of one fitted model: -b is not supported with it"));
    CHECK(refused(estimation({"--missing", ","}), "--missing: TOKENS must name at least one spelling, e.g. NA,?,-"));
    CHECK(refused(estimation({"--mask-cells", "m", "--gain", "0.1", "--gain-dense", "--reconstruct-marginal"}),
                  "the gain model's --reconstruct-marginal summarises every leaf at its observed count: it is not supported with --missing / --mask-cells"));
    CHECK(refused(estimation({"--mu", "0.1", "--estimate-mu"}), "--mu fixes the death rates and --estimate-mu searches them: give one of the two"));
    CHECK(refused(estimation({"--estimate-mu", "-l", "0.1"}), "--estimate-mu searches lambda and mu together: -l / -m are not supported with it"));
    CHECK(refused(estimation({"--family-mu", "estimate"}), "--family-mu sets the death rates of -b: it is not supported without -b"));
    CHECK(refused(estimation({"-b", "-a", "1"}), "-b estimates one lambda per family under the base model; -k > 1 and -a are not supported with it"));
    CHECK(refused(estimation({"-b", "-e"}), "-b with -e needs an error model file: estimating epsilon per family is not supported"));
    CHECK(refused(estimation({"-b", "--gpus", "1"}), "-b runs on one GPU: --gpus is not supported with it"));
    CHECK(driver_refusal(estimation({"-b", "-e", "E", "--family-mu", "0.1", "--missing", "NA"})) == nullptr);
    // what follows an accepted command line
    o = estimation({"-s", "11", "--sample-histories", "5", "-b", "-l", "0.1"});
    const gain_request g = gain_request_of(o);
    CHECK(g.per_family && g.histories && !g.gain && !g.gpus && !g.simulate && !g.estimate_error);
    normalise_options(o);                                        // (warns on stderr that -l is ignored)
    CHECK(o.history_seed == 11 && o.fixed_lambda == 0 && o.multi.empty());
    std::mt19937 same(11);
    CHECK(randomizer_engine() == same());                        // -s seeded the engine
    o = estimation({"-s", "11", "--sample-histories", "5", "--sample-seed", "3"});
    normalise_options(o);
    CHECK(o.history_seed == 3);
}

int main() {
    test_parse_options();
    test_driver_refusals();
    test_poisson_scorer();
    test_reconstruction_reports();
    test_pvalue();
    test_newick();
    test_families_and_sizes();
    test_error_model();
    test_priors_and_gamma();
    test_scorers();
    test_optimizer();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
