// CPU-only unit tests of what `cafexp_hip --missing / --mask-cells` does on the host: reading a table with unknown cells, masking
// cells by (family, species), sizing and filtering on the observed cells only, counting, and the imputed-counts report's
// arithmetic.  No GPU, no HIP library linked.
#include <cmath>
#include <cstdio>
#include <sstream>

#include "cafe_host.h"

using namespace cafe;

static int failures = 0, checks = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { ++failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)
#define THROWS(expr) do { ++checks; bool t_ = false; try { expr; } catch (const std::exception&) { t_ = true; } if (!t_) { ++failures; std::printf("FAIL %s:%d  no throw: %s\n", __FILE__, __LINE__, #expr); } } while (0)

static const char* kTable = "Desc\tFamily ID\tA\tB\tC\tD\n(null)\tf1\t3\tNA\t1\t2\n(null)\tf2\t0\t ? \t2\t0\n(null)\tf3\t-\t70\t0\t1\n(null)\tf4\t4\t4\t4\t4\n";

static std::vector<gene_family> read(const char* tokens) {
    std::istringstream in(kTable);
    std::vector<gene_family> fams;
    const std::set<std::string> tk = parse_missing_tokens(tokens ? tokens : "");
    read_gene_families(in, nullptr, fams, tokens ? &tk : nullptr);
    return fams;
}

static void test_tokens() {
    CHECK(parse_missing_tokens("NA,?,-") == (std::set<std::string>{"NA", "?", "-"}));
    CHECK(parse_missing_tokens(" NA ,,").size() == 1 && parse_missing_tokens("").empty() && parse_missing_tokens(",").empty());
}

static void test_reading() {
    const std::vector<gene_family> plain = read(nullptr);            // as before: atoi makes 0 of every such cell
    CHECK(plain.size() == 4 && plain[0].get_species_size("B") == 0 && plain[1].get_species_size("B") == 0 && plain[2].get_species_size("A") == 0);
    CHECK(count_missing(plain).cells == 0 && count_missing(plain).families == 0);
    const std::vector<gene_family> empty_set = read("");             // an empty token set is no token set
    CHECK(empty_set[0].get_species_size("B") == 0);
    const std::vector<gene_family> fams = read("NA,?,-");
    CHECK(fams[0].get_species_size("B") == kCountMissing && fams[0].is_missing("b") && !fams[0].is_missing("A") && !fams[0].is_missing("nobody"));
    CHECK(fams[1].get_species_size("B") == kCountMissing);           // blanks around the token
    CHECK(fams[2].get_species_size("A") == kCountMissing && fams[2].get_species_size("B") == 70 && fams[3].n_missing() == 0);
    const missing_summary ms = count_missing(fams);
    CHECK(ms.cells == 3 && ms.families == 3);
    const std::vector<gene_family> some = read("NA");
    CHECK(some[0].get_species_size("B") == kCountMissing && some[1].get_species_size("B") == 0 && some[2].get_species_size("A") == 0);
}

static void test_sizes_and_root_filter() {
    std::vector<gene_family> fams = read("NA,?,-");
    int M = 0, R = 0, M0 = 0, R0 = 0;
    compute_max_sizes(fams, M, R);
    std::vector<gene_family> plain = read(nullptr);
    compute_max_sizes(plain, M0, R0);
    CHECK(M == M0 && R == R0 && M == 70 + 50 && R == 88);            // from the observed cells
    gene_family none;
    none.set_species_size("A", kCountMissing); none.set_species_size("B", kCountMissing);
    CHECK(none.get_max_size() == 0 && none.n_missing() == 2);
    std::unique_ptr<clade> t(parse_newick("((A:1,B:1):1,(C:1,D:1):1);"));
    CHECK(fams[0].exists_at_root(t.get()));                          // A = 3 under (A, B)
    CHECK(!fams[1].exists_at_root(t.get()));                         // A = 0, B missing: a missing cell counts as absent
    gene_family f = fams[3];
    f.set_species_size("C", kCountMissing); f.set_species_size("D", kCountMissing);
    CHECK(!f.exists_at_root(t.get()));
}

static void test_mask() {
    std::vector<gene_family> fams = read(nullptr);
    std::istringstream in("#FamilyID\tSpecies\tObserved\tMean\nf1\tB\t0\t2.5\tlow\n\nf3\tA\r\nf3\tA\n");
    CHECK(mask_cells(in, fams) == 2);                                // the repeated line marks nothing new
    const std::vector<gene_family> want = read("NA,-");
    CHECK(fams[0].species_size_match(want[0]) && fams[2].species_size_match(want[2]) && fams[1].n_missing() == 0);
    std::istringstream unknown_family("f9\tA\n"), unknown_species("f1\tZ\n"), short_line("f1\n");
    THROWS(mask_cells(unknown_family, fams));
    THROWS(mask_cells(unknown_species, fams));
    THROWS(mask_cells(short_line, fams));
    CHECK(count_missing(fams).cells == 2);                           // a refused file leaves the table as it was
}

static void test_imputed() {
    leaf_predictive_result r;
    r.species = {"A", "B"};
    r.observed = {3, kCountMissing, kCountMissing, 2, kCountMissing, 1};
    r.mean = {4.0, 10.0, 0.5, 2.0, NAN, 1.0};
    r.sd = {1.0, 2.0, 1.0, 1.0, NAN, 1.0};
    r.p_below = r.p_obs = r.p_above = {0.1, NAN, NAN, 0.1, NAN, 0.1};
    r.failed = {0, 0, 0};
    const std::vector<imputed_cell> c = imputed_cells(r);
    CHECK(c.size() == 3 && c[0].family == 0 && c[0].species == 1 && c[1].family == 1 && c[1].species == 0 && c[2].family == 2);
    CHECK(c[0].lo == 6 && c[0].hi == 14);                            // 10 -+ 3.92: floor 6.08, ceil 13.92
    CHECK(c[1].lo == 0 && c[1].hi == 3);                             // cut at 0
    CHECK(std::isnan(c[2].mean));
    const std::vector<leaf_cell> out = leaf_outliers(r);             // a missing cell is no observation: it takes no part
    CHECK(out.size() == 3);
}

int main() {
    test_tokens();
    test_reading();
    test_sizes_and_root_filter();
    test_mask();
    test_imputed();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
