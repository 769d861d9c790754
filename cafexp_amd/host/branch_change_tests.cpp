// CPU-only unit tests of the reports behind `cafexp_hip --branch-change` (branch_change.cpp): the cell text, the per-branch
// sums and counts, what a failed family and the root contribute, and the two files as written.  No GPU, no HIP library linked.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "cafe_host.h"

using namespace cafe;

static int failures = 0, checks = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { ++failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)
#define CLOSE(a, b, tol) CHECK(std::fabs((a) - (b)) <= (tol))

static const int32_t NONE = INT32_MIN;                          // CAFE_CHANGE_NONE (the C header is not needed here)

// three nodes (A, B, the root "3"), four families; family 2 failed; band +-2
static branch_change_result table() {
    branch_change_result r;
    r.max_change = 2; r.level = 0.9;
    r.names = {"A", "B", "3"};
    r.root = {0, 0, 1};
    //         family 0             family 1             family 2 (failed)    family 3
    r.mean  = {1.5, -0.25, NAN,     0.0, -2.75, NAN,     NAN, NAN, NAN,       4.0, 0.5, NAN};
    r.mode  = {1, 0, NONE,          0, -2, NONE,         NONE, NONE, NONE,    2, 0, NONE};
    r.lo    = {1, -1, NONE,         0, -3, NONE,         NONE, NONE, NONE,    2, -1, NONE};
    r.hi    = {2, 0, NONE,          0, -1, NONE,         NONE, NONE, NONE,    3, 2, NONE};
    r.below = {0.0, 0.001, NAN,     0.0, 0.4, NAN,       NAN, NAN, NAN,       0.0, 0.0, NAN};
    r.above = {0.01, 0.0, NAN,      0.0, 0.0, NAN,       NAN, NAN, NAN,       0.7, 0.02, NAN};
    r.failed = {0, 0, 1, 0};
    return r;
}

static void test_rows() {
    const branch_change_result r = table();
    const std::vector<branch_change_row> rows = branch_change_rows(r);
    CHECK(rows.size() == 3);
    CLOSE(rows[0].mean_sum, 1.5 + 0.0 + 4.0, 1e-15);             // the failed family's NaN takes no part
    CLOSE(rows[1].mean_sum, -0.25 - 2.75 + 0.5, 1e-15);
    CHECK(rows[0].expanded == 2 && rows[0].contracted == 0);     // lo = 1 and lo = 2; [0, 0] is neither
    CHECK(rows[1].expanded == 0 && rows[1].contracted == 1);     // [-3, -1]; [-1, 0] touches 0: not wholly below
    CHECK(rows[0].clipped == 1);                                 // hi = 3 = D + 1
    CHECK(rows[1].clipped == 1);                                 // lo = -3 = -D - 1; hi = 2 = D is inside the band
    CHECK(rows[2].mean_sum == 0.0 && rows[2].expanded == 0 && rows[2].contracted == 0 && rows[2].clipped == 0);      // the root
    CHECK(r.failed_count() == 1 && r.n_nodes() == 3);
}

static void test_cells() {
    const branch_change_result r = table();
    CHECK(branch_change_cell(r, 0, 0) == "1.5:1:[1,2]:0:0.01");
    CHECK(branch_change_cell(r, 0, 1) == "-0.25:0:[-1,0]:0.001:0");
    CHECK(branch_change_cell(r, 1, 1) == "-2.75:-2:[-3,-1]:0.4:0");
    CHECK(branch_change_cell(r, 3, 0) == "4:2:[2,3]:0:0.7");
    CHECK(branch_change_cell(r, 0, 2) == "-");                   // the root
    CHECK(branch_change_cell(r, 2, 0) == "-" && branch_change_cell(r, 2, 2) == "-");      // a failed family
}

static std::vector<std::string> lines_of(const std::string& path) {
    std::ifstream f(path);
    std::vector<std::string> out;
    for (std::string ln; std::getline(f, ln);) out.push_back(ln);
    return out;
}

static void test_files() {
    const branch_change_result r = table();
    char tmpl[] = "/tmp/branch_change_tests_XXXXXX";
    const char* dir = mkdtemp(tmpl);
    CHECK(dir != nullptr);
    if (!dir) return;
    const size_t clipped = write_branch_change_reports(r, "Base", dir, {"f0", "f1", "f2", "f3"});
    CHECK(clipped == 2);
    const std::string cells_path = std::string(dir) + "/Base_branch_change.tab", sum_path = std::string(dir) + "/Base_branch_change_summary.tab";
    const std::vector<std::string> cells = lines_of(cells_path);
    CHECK(cells.size() == 5);
    if (cells.size() == 5) {
        CHECK(cells[0] == "FamilyID\tA\tB\t3");
        CHECK(cells[1] == "f0\t1.5:1:[1,2]:0:0.01\t-0.25:0:[-1,0]:0.001:0\t-");
        CHECK(cells[3] == "f2\t-\t-\t-");
        CHECK(cells[4] == "f3\t4:2:[2,3]:0:0.7\t0.5:0:[-1,2]:0:0.02\t-");
    }
    const std::vector<std::string> sum = lines_of(sum_path);
    CHECK(sum.size() == 3);                                      // the header and the two branches: no line for the root
    if (sum.size() == 3) {
        CHECK(sum[0].rfind("#Node\tmean_change\texpanded\tcontracted\tclipped\t", 0) == 0);
        CHECK(sum[0].find("90 % interval") != std::string::npos && sum[0].find("+-2") != std::string::npos);
        CHECK(sum[0].find("over 3 families, 1 failed") != std::string::npos);
        CHECK(sum[1] == "A\t5.5\t2\t0\t1");
        CHECK(sum[2] == "B\t-2.5\t0\t1\t1");
    }
    std::remove(cells_path.c_str());
    std::remove(sum_path.c_str());
    std::remove(dir);
}

static void test_band_zero_and_no_families() {
    branch_change_result r = table();
    r.max_change = 0;                                            // every interval end other than 0 is beyond the band
    const std::vector<branch_change_row> rows = branch_change_rows(r);
    CHECK(rows[0].clipped == 2 && rows[1].clipped == 3);         // A: [1,2], [2,3]; B: [-1,0], [-3,-1], [-1,2]
    branch_change_result none;
    none.names = {"A", "3"}; none.root = {0, 1};
    CHECK(branch_change_rows(none).size() == 2 && branch_change_rows(none)[0].mean_sum == 0.0 && none.failed_count() == 0);
}

int main() {
    test_rows();
    test_cells();
    test_files();
    test_band_zero_and_no_families();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
