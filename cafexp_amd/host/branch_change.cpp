// The reports of `cafexp_hip --branch-change`: from cafe_branch_change's summaries per family and branch -- the mean, mode and
// equal-tailed interval of the size change and the posterior mass beyond the band -- the table of cells and the summary per
// branch.  Plain host arithmetic: the device call is hip_model_base::branch_change (hip_reconstruct.cpp).
#include <cstdio>
#include <fstream>

#include "cafe_host.h"

namespace cafe {

std::vector<branch_change_row> branch_change_rows(const branch_change_result& res) {
    const size_t m = res.n_nodes();
    std::vector<branch_change_row> rows(m);
    for (size_t f = 0; f < res.failed.size(); ++f) {
        if (res.failed[f]) continue;
        for (size_t v = 0; v < m; ++v) {
            if (res.root[v]) continue;
            const size_t at = f * m + v;
            branch_change_row& r = rows[v];
            r.mean_sum += res.mean[at];
            r.expanded += res.lo[at] > 0;
            r.contracted += res.hi[at] < 0;
            r.clipped += res.lo[at] < -res.max_change || res.hi[at] > res.max_change;
        }
    }
    return rows;
}

std::string branch_change_cell(const branch_change_result& res, size_t family, size_t node) {
    if (res.root[node] || res.failed[family]) return "-";
    const size_t at = family * res.n_nodes() + node;
    char buf[192];
    std::snprintf(buf, sizeof buf, "%.6g:%d:[%d,%d]:%.6g:%.6g", res.mean[at], res.mode[at], res.lo[at], res.hi[at], res.below[at], res.above[at]);
    return buf;
}

size_t write_branch_change_reports(const branch_change_result& res, const std::string& model_identifier, const std::string& dir,
                                   const std::vector<std::string>& family_ids) {
    const std::string prefix = (dir.empty() ? std::string("results") : dir) + "/" + model_identifier;
    std::ofstream cells(prefix + "_branch_change.tab"), summary(prefix + "_branch_change_summary.tab");
    const size_t m = res.n_nodes();
    cells << "FamilyID";
    for (size_t v = 0; v < m; ++v) cells << "\t" << res.names[v];
    cells << std::endl;
    for (size_t f = 0; f < family_ids.size(); ++f) {
        cells << family_ids[f];
        for (size_t v = 0; v < m; ++v) cells << "\t" << branch_change_cell(res, f, v);
        cells << std::endl;
    }
    const std::vector<branch_change_row> rows = branch_change_rows(res);
    summary << "#Node\tmean_change\texpanded\tcontracted\tclipped\t(sum of the posterior mean change; families whose " << 100.0 * res.level
            << " % interval lies wholly above 0 / wholly below 0 / ends beyond the band of +-" << res.max_change << "; over "
            << family_ids.size() - res.failed_count() << " families, " << res.failed_count() << " failed)" << std::endl;
    size_t clipped = 0;
    char buf[160];
    for (size_t v = 0; v < m; ++v) {
        if (res.root[v]) continue;
        std::snprintf(buf, sizeof buf, "\t%.12g\t%zu\t%zu\t%zu", rows[v].mean_sum, rows[v].expanded, rows[v].contracted, rows[v].clipped);
        summary << res.names[v] << buf << std::endl;
        clipped += rows[v].clipped;
    }
    return clipped;
}

}  // namespace cafe
