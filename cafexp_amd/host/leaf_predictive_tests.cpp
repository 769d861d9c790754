// CPU-only unit tests of the arithmetic behind `cafexp_hip --leaf-predictive` (leaf_predictive.cpp): the two-sided p, Holm's
// adjustment over the finite cells, the order of the outliers and the summary per species.  No GPU, no HIP library linked.
#include <cmath>
#include <cstdio>

#include "cafe_host.h"

using namespace cafe;

static int failures = 0, checks = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { ++failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)
#define CLOSE(a, b, tol) CHECK(std::fabs((a) - (b)) <= (tol))

static void test_holm() {
    // sorted: 0.001 (x4), 0.01 (x3), 0.03 (x2 = 0.06), 0.04 (x1: stays at the running maximum 0.06)
    const std::vector<double> adj = holm_adjusted({0.04, 0.001, 0.03, 0.01});
    CLOSE(adj[1], 0.004, 1e-15); CLOSE(adj[3], 0.03, 1e-15); CLOSE(adj[2], 0.06, 1e-15); CLOSE(adj[0], 0.06, 1e-15);
    const std::vector<double> capped = holm_adjusted({0.6, 0.5});
    CHECK(capped[0] == 1.0 && capped[1] == 1.0);
    CHECK(holm_adjusted({}).empty());
}

// two species, three families; the cell (1, B) has no mass
static leaf_predictive_result table() {
    leaf_predictive_result r;
    r.species = {"A", "B"};
    r.observed = {0, 5, 9, 2, 3, 3};
    r.mean = {4.0, 5.0, 3.0, NAN, 3.0, 2.0};
    r.sd = {1.0, 2.0, 1.5, NAN, 0.0, 1.0};
    r.p_below = {0.0, 0.4, 0.9996, NAN, 0.0, 0.6};
    r.p_obs = {0.0001, 0.2, 0.0003, NAN, 1.0, 0.3};
    r.p_above = {0.9999, 0.4, 0.0001, NAN, 0.0, 0.1};
    r.failed = {0, 0, 0};
    return r;
}

static void test_cells_and_order() {
    const leaf_predictive_result r = table();
    const std::vector<leaf_cell> c = leaf_outliers(r);
    CHECK(c.size() == 5);                                        // the NaN cell takes no part, not even in Holm's count
    CHECK(c[0].family == 0 && c[0].species == 0 && c[0].low);    // p_low = 1e-4: p = 2e-4, x 5
    CLOSE(c[0].p, 2e-4, 1e-18); CLOSE(c[0].holm, 1e-3, 1e-17);
    CHECK(c[1].family == 1 && c[1].species == 0 && !c[1].low);   // p_high = 4e-4: p = 8e-4, x 4
    CLOSE(c[1].p_high, 4e-4, 1e-18); CLOSE(c[1].holm, 3.2e-3, 1e-17);
    CHECK(c[2].family == 2 && c[2].species == 1 && !c[2].low);   // p_high = 0.4: p = 0.8, x 3 -> 1
    CHECK(c[2].holm == 1.0 && c[3].holm == 1.0 && c[4].holm == 1.0);
    CHECK(c[3].p == 1.0 && c[4].p == 1.0);                       // min(1, 2 x 0.6) and the point mass: p_low = p_high = 1
    CHECK(c[3].family == 0 && c[3].species == 1 && c[4].family == 2 && c[4].species == 0);     // ties keep the table's order
}

static void test_species_fit() {
    const leaf_predictive_result r = table();
    const std::vector<leaf_cell> c = leaf_outliers(r);
    const std::vector<species_fit> fit = leaf_species_fit(r, c, 0.05);
    CHECK(fit.size() == 2 && fit[0].cells == 3 && fit[1].cells == 2);
    CHECK(fit[0].low == 1 && fit[0].high == 1 && fit[1].low == 0 && fit[1].high == 0);
    CLOSE(fit[0].mean_z, ((0 - 4.0) / 1.0 + (9 - 3.0) / 1.5) / 2, 1e-15);      // the cell with sd = 0 is left out of the mean
    CLOSE(fit[1].mean_z, ((5 - 5.0) / 2.0 + (3 - 2.0) / 1.0) / 2, 1e-15);
    CLOSE(fit[0].log_p_obs, std::log(0.0001) + std::log(0.0003) + std::log(1.0), 1e-12);
    CLOSE(fit[1].log_p_obs, std::log(0.2) + std::log(0.3), 1e-12);
    const std::vector<species_fit> strict = leaf_species_fit(r, c, 2e-3);
    CHECK(strict[0].low == 1 && strict[0].high == 0);
    leaf_predictive_result impossible = r;
    impossible.p_obs[0] = 0.0;                                   // an impossible observation: finite, p = 0, no logarithm
    const std::vector<leaf_cell> ci = leaf_outliers(impossible);
    CHECK(ci[0].p == 0.0 && ci[0].holm == 0.0 && ci[0].low);
    CLOSE(leaf_species_fit(impossible, ci, 0.05)[0].log_p_obs, std::log(0.0003), 1e-12);
}

int main() {
    test_holm();
    test_cells_and_order();
    test_species_fit();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
