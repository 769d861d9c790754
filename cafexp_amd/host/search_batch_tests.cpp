// CPU-only tests of the look-ahead search (optimizer::batch > 1, nm_search::lookahead): on mock scorers the batched search feeds
// nm_search the very (point, value) sequence of the sequential one -- same iterations, best point, score and num_scorer_calls
// -- for n = 1, 2, 3 parameters and batch = 2, 3, 4, 8, on
//   (a) a quadratic in the logs of the parameters, +inf outside the positive orthant, started far above its optimum so that the
//       growing steps towards it reflect across zero;
//   (b) Rosenbrock from (-1.2, 1) and (-1.2, 1, 0.5), which shrinks many times;
//   (c) an objective that is +inf at vertex 1 of the first simplex: vertex 2 is then widened and is not the speculated point.
// The count: one batch for the first simplex, one per iteration, one per shrink, so for batch >= max(4, n + 1) on (a) and (b)
// num_batches <= num_iterations + shrinks + 1.
#include "cafe_host.h"

#include <cstdio>
#include <cstring>
#include <limits>

using namespace cafe;

static int failures = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

namespace {
const double INF = std::numeric_limits<double>::infinity();

typedef double (*objective_fn)(const std::vector<double>& x, const std::vector<double>& x0);

double log_quadratic(const std::vector<double>& x, const std::vector<double>&) {
    static const double c[3] = {0.01, 0.02, 0.005};
    double s = 0;
    for (size_t i = 0; i < x.size(); ++i) {
        if (!(x[i] > 0)) return INF;
        const double d = std::log(x[i]) - std::log(c[i]);
        s += (1 + i) * d * d;
    }
    return s;
}
double rosenbrock(const std::vector<double>& x, const std::vector<double>&) {
    double s = 0;
    for (size_t i = 0; i + 1 < x.size(); ++i) s += 100 * (x[i + 1] - x[i] * x[i]) * (x[i + 1] - x[i] * x[i]) + (1 - x[i]) * (1 - x[i]);
    return s;
}
double infinite_at_vertex_one(const std::vector<double>& x, const std::vector<double>& x0) {
    bool at = x[0] == (1 + 0.05) * x0[0];
    for (size_t i = 1; i < x.size(); ++i) at = at && x[i] == x0[i];
    if (at) return INF;
    double s = 0;
    for (size_t i = 0; i < x.size(); ++i) s += (1 + i) * (x[i] - 0.3 * (i + 1)) * (x[i] - 0.3 * (i + 1));
    return s;
}

// A scorer over an objective; vectorised: overrides calculate_scores (one "device call" per batch) instead of the loop
class mock_scorer : public optimizer_scorer {
public:
    objective_fn fn;
    std::vector<double> x0;
    bool vectorised;
    int single_calls = 0, batch_calls = 0, infinite = 0;
    mock_scorer(objective_fn f, const std::vector<double>& start, bool vec = false) : fn(f), x0(start), vectorised(vec) {}
    std::vector<double> initial_guesses() override { return x0; }
    double value(const double* v) {
        const double f = fn(std::vector<double>(v, v + x0.size()), x0);
        infinite += std::isinf(f);
        return f;
    }
    double calculate_score(const double* v) override { ++single_calls; return value(v); }
    void calculate_scores(const double* values, int n_points, int n_values, double* out) override {
        if (!vectorised) { optimizer_scorer::calculate_scores(values, n_points, n_values, out); return; }
        ++batch_calls;
        for (int i = 0; i < n_points; ++i) out[i] = value(values + (size_t)i * n_values);
    }
};

typedef std::vector<std::pair<std::vector<double>, double>> trace_t;

bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0);
}
bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

struct case_t { const char* name; objective_fn fn; std::vector<double> x0; bool use_start, counted; };

void run_case(const case_t& c) {
    const int n = (int)c.x0.size();
    // the sequential optimizer, and the sequence it feeds: optimize() is `feed(score(trial()))` on these settings
    mock_scorer seq_scorer(c.fn, c.x0);
    optimizer seq(&seq_scorer);
    if (c.use_start) seq.start = c.x0;
    const optimizer_result want = seq.optimize();
    trace_t fed;
    int shrinks = 0;
    {
        mock_scorer s(c.fn, c.x0);
        nm_search search(nm_settings{}, c.x0);
        while (!search.done()) {
            const std::vector<double> x = search.trial();
            const double f = s.calculate_score(x.data());
            fed.push_back({x, f});
            search.feed(f);
        }
        shrinks = search.shrinks();
        CHECK(same_bits(search.best(), want.values) && same_bits(search.best_score(), want.score) && search.iterations() == want.num_iterations);
        CHECK(search.calls() + (c.use_start ? 0 : 1) == want.num_scorer_calls);
    }
    CHECK(want.num_batches == 0 && want.num_points_scored == 0);
    std::printf("%-28s n %d: iterations %d, points consumed %d, shrinks %d, infinite scores %d\n", c.name, n, want.num_iterations,
                want.num_scorer_calls, shrinks, seq_scorer.infinite);
    for (const int batch : {2, 3, 4, 8})
        for (const bool vectorised : {false, true}) {
            mock_scorer scorer(c.fn, c.x0, vectorised);
            optimizer opt(&scorer);
            if (c.use_start) opt.start = c.x0;
            opt.batch = batch;
            trace_t trace;
            const optimizer_result got = opt.optimize([&](const std::vector<double>& x, double f) { trace.push_back({x, f}); });
            CHECK(trace.size() == fed.size());
            bool same = trace.size() == fed.size();
            for (size_t i = 0; same && i < fed.size(); ++i) same = same_bits(trace[i].first, fed[i].first) && same_bits(trace[i].second, fed[i].second);
            CHECK(same);
            CHECK(same_bits(got.values, want.values) && same_bits(got.score, want.score));
            CHECK(got.num_iterations == want.num_iterations && got.num_scorer_calls == want.num_scorer_calls);
            CHECK(got.num_batches >= 1 && got.num_batches < got.num_scorer_calls && got.num_points_scored >= got.num_batches);
            if (vectorised) CHECK(scorer.batch_calls == got.num_batches);
            else CHECK(scorer.batch_calls == 0 && scorer.single_calls == got.num_points_scored);
            if (c.counted && batch >= std::max(4, n + 1)) CHECK(got.num_batches <= got.num_iterations + shrinks + 1);
            if (!vectorised)
                std::printf("    batch %d: %d batches, %d points scored%s\n", batch, got.num_batches, got.num_points_scored,
                            c.counted && batch >= std::max(4, n + 1) ? "  (within iterations + shrinks + 1)" : "");
        }
}

void test_lookahead_lists_what_the_search_asks_next() {
    // first simplex: the remaining vertices; after it, before the reflected point's score: expansion, outside, inside
    const std::vector<double> x0{-1.2, 1.0, 0.5};
    nm_search search(nm_settings{}, x0);
    std::vector<std::vector<double>> ahead;
    search.lookahead(ahead);
    CHECK(ahead.size() == 3);
    for (int i = 0; i < 3; ++i) {
        search.feed(rosenbrock(search.trial(), x0));
        CHECK(same_bits(search.trial(), ahead[i]));
    }
    search.lookahead(ahead);
    CHECK(ahead.empty());                                           // the last vertex: the sort comes next
    search.feed(rosenbrock(search.trial(), x0));
    int seen[3] = {0, 0, 0}, shrunk = 0;
    while (!search.done() && !(seen[0] && seen[2] && shrunk)) {
        search.lookahead(ahead);                                    // at the reflected point
        CHECK(ahead.size() == 3);
        const std::vector<std::vector<double>> speculated = ahead;
        const int before = search.iterations(), shrinks = search.shrinks();
        search.feed(rosenbrock(search.trial(), x0));
        if (search.done() || search.iterations() != before) continue;     // accepted at once
        int which = -1;
        for (int i = 0; i < 3; ++i) if (same_bits(search.trial(), speculated[i])) which = i;
        CHECK(which >= 0);
        if (which >= 0) ++seen[which];
        search.lookahead(ahead);
        CHECK(ahead.empty());
        search.feed(rosenbrock(search.trial(), x0));
        if (search.shrinks() == shrinks) continue;
        ++shrunk;                                                   // the contraction failed: vertex 1 is the trial, 2 and 3 are listed
        search.lookahead(ahead);
        CHECK(ahead.size() == 2);
        const std::vector<std::vector<double>> rest = ahead;
        for (int i = 0; i < 2; ++i) {
            search.feed(rosenbrock(search.trial(), x0));
            CHECK(same_bits(search.trial(), rest[i]));
        }
        search.feed(rosenbrock(search.trial(), x0));
    }
    CHECK(seen[0] && seen[2] && shrunk);
    // the outside contraction follows a reflected point that TIES with the worst vertex: a flat objective
    nm_search flat(nm_settings{}, x0);
    for (int i = 0; i <= 3; ++i) flat.feed(1.0);
    flat.lookahead(ahead);
    CHECK(ahead.size() == 3);
    const std::vector<double> outside = ahead.size() == 3 ? ahead[1] : x0;
    flat.feed(1.0);
    CHECK(same_bits(flat.trial(), outside));
}
}  // namespace

int main() {
    test_lookahead_lists_what_the_search_asks_next();
    const case_t cases[] = {
        {"log-quadratic (a)", log_quadratic, {5.0}, false, true},
        {"log-quadratic (a)", log_quadratic, {5.0, 8.0}, false, true},
        {"log-quadratic (a)", log_quadratic, {5.0, 8.0, 3.0}, true, true},
        {"Rosenbrock (b)", rosenbrock, {-1.2, 1.0}, false, true},
        {"Rosenbrock (b)", rosenbrock, {-1.2, 1.0, 0.5}, true, true},
        {"infinite at vertex 1 (c)", infinite_at_vertex_one, {1.0}, false, false},
        {"infinite at vertex 1 (c)", infinite_at_vertex_one, {1.0, 2.0}, false, false},
        {"infinite at vertex 1 (c)", infinite_at_vertex_one, {1.0, 2.0, 0.5}, true, false},
    };
    for (const case_t& c : cases) run_case(c);
    if (failures) { std::printf("%d check(s) FAILED\n", failures); return 1; }
    std::printf("search_batch_tests: all passed\n");
    return 0;
}
