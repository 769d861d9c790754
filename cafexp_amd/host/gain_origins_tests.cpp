// CPU-only unit tests of the --gain-posterior reports (gain_origins.cpp): the weighted sums over the table's families, the
// families counted at p_gain > 0.5, failed entries, and the text of both files.  No GPU, no HIP library linked.
#include <cmath>
#include <cstdio>
#include <limits>
#include <sstream>

#include "cafe_host.h"

using namespace cafe;

static int failures = 0, checks = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { ++failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)
#define CLOSE(a, b, tol) CHECK(std::fabs((a) - (b)) <= (tol))

static const double NaN = std::numeric_limits<double>::quiet_NaN();
static const double INF = std::numeric_limits<double>::infinity();

// three nodes A, B and the root (index 2); three entries and the absent profile
static gain_origins example() {
    gain_origins o;
    o.n_nodes = 3;
    o.lnl = {-3.5, -7.25, -INF, -0.5};
    o.p_absent = {0.0, 1.0, 0.25,   1.0, 0.0, 0.75,   NaN, NaN, NaN,   0.9, 0.9, 0.8};
    o.mean =     {2.0, 0.0, 1.5,    0.0, 3.0, 0.5,    NaN, NaN, NaN,   0.1, 0.1, 0.2};
    o.p_gain =   {0.25, 0.0, NaN,   0.0, 0.75, NaN,   NaN, NaN, NaN,   0.05, 0.05, NaN};
    o.p_loss =   {0.0, 0.75, NaN,   0.25, 0.0, NaN,   NaN, NaN, NaN,   0.1, 0.1, NaN};
    return o;
}

static void test_totals() {
    const gain_origins o = example();
    const std::vector<double> weight = {3.0, 2.0, 1.0, 0.0};
    const gain_branch_origins t = gain_origin_totals(o, weight, 2);
    CHECK(t.used == 5.0 && t.failed == 1.0);
    CLOSE(t.originated[0], 3 * 0.25, 1e-15);
    CLOSE(t.originated[1], 2 * 0.75, 1e-15);
    CHECK(t.originated[2] == 0.0 && t.lost[2] == 0.0);       // the root has no branch
    CLOSE(t.lost[0], 2 * 0.25, 1e-15);
    CLOSE(t.lost[1], 3 * 0.75, 1e-15);
    CLOSE(t.present[0], 3.0, 1e-15);
    CLOSE(t.present[1], 2.0, 1e-15);
    CLOSE(t.present[2], 3 * 0.75 + 2 * 0.25, 1e-15);
    CLOSE(t.absent_at_root, 3 * 0.25 + 2 * 0.75, 1e-15);
    CLOSE(t.absent_at_root + t.present[2], t.used, 1e-15);
    CHECK(t.likely_origin[0] == 0.0 && t.likely_origin[1] == 2.0 && t.likely_origin[2] == 0.0);
    CHECK(t.origin_somewhere == 2.0);

    gain_origins edge = example();
    edge.p_gain[0] = 0.5;                                    // exactly one half does not exceed it
    CHECK(gain_origin_totals(edge, weight, 2).likely_origin[0] == 0.0);
    edge.p_gain[0] = std::nextafter(0.5, 1.0);
    edge.p_gain[1] = 0.9;                                    // two branches of one family: counted on each, once as a family
    const gain_branch_origins both = gain_origin_totals(edge, weight, 2);
    CHECK(both.likely_origin[0] == 3.0 && both.likely_origin[1] == 5.0 && both.origin_somewhere == 5.0);

    bool threw = false;
    try { gain_origin_totals(o, {1.0, 1.0}, 2); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw);
    threw = false;
    try { gain_origin_totals(o, weight, 3); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw);
    gain_origins empty;
    empty.n_nodes = 1;
    const gain_branch_origins none = gain_origin_totals(empty, {}, 0);
    CHECK(none.used == 0.0 && none.present.size() == 1 && none.present[0] == 0.0);
}

static void test_text() {
    const gain_origins o = example();
    const std::vector<std::string> names = {"A<0>", "B<1>", "<2>"};
    std::ostringstream cells;
    write_gain_origins(cells, o, names, 2, {"f0", "f1", "f2", "f3"}, {0, 1, 0, 2});
    const std::string want =
        "FamilyID\tA<0>\tB<1>\t<2>\tA<0>^\tB<1>^\n"
        "f0\t0:2\t1:0\t0.25:1.5\t0.25:0\t0:0.75\n"
        "f1\t1:0\t0:3\t0.75:0.5\t0:0.25\t0.75:0\n"
        "f2\t0:2\t1:0\t0.25:1.5\t0.25:0\t0:0.75\n"
        "f3\tnan:nan\tnan:nan\tnan:nan\tnan:nan\tnan:nan\n";
    CHECK(cells.str() == want);
    if (cells.str() != want) std::printf("%s", cells.str().c_str());

    std::ostringstream totals;
    write_gain_branch_origins(totals, gain_origin_totals(o, {3.0, 2.0, 1.0, 0.0}, 2), names, 2);
    const std::string want_totals =
        "#Node\toriginated\tlost\tpresent\tp_gain>0.5\t(expected numbers of families, summed over 5 families; 1 failed)\n"
        "A<0>\t0.75\t0.5\t3\t0\n"
        "B<1>\t1.5\t2.25\t2\t2\n"
        "#Root <2>\tabsent\t2.25\tpresent\t2.75\n";
    CHECK(totals.str() == want_totals);
    if (totals.str() != want_totals) std::printf("%s", totals.str().c_str());

    bool threw = false;
    std::ostringstream sink;
    try { write_gain_origins(sink, o, names, 2, {"f0"}, {4}); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw);
    threw = false;
    try { write_gain_origins(sink, o, {"A", "B"}, 2, {"f0"}, {0}); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw);
}

static void test_refusal() {
    gain_request r;
    r.posterior = true;
    const char* why = gain_refusal(r);
    CHECK(why && std::string(why).find("--gain-posterior") == 0 && std::string(why).find("--gain NU or --estimate-gain") != std::string::npos);
    r.gain = true; r.nu = 0.001;
    CHECK(gain_refusal(r) == nullptr);
    r.gain = false; r.estimate_gain = true;
    CHECK(gain_refusal(r) == nullptr);
}

int main() {
    test_totals();
    test_text();
    test_refusal();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
