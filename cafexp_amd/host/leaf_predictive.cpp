// The reports of `cafexp_hip --leaf-predictive`: from cafe_leaf_predictive's five numbers per cell (family, species) -- the mean
// and sd of the species' count predicted from the counts of every other species, and the mass below, at and above the observed
// count -- the table of all cells, the outliers after Holm's adjustment over every finite cell, and a summary per species.  Pure
// host arithmetic: the device call is hip_model_base::leaf_predictive (hip_reconstruct.cpp).
#include <algorithm>
#include <cmath>
#include <fstream>

#include "cafe_host.h"

namespace cafe {

std::vector<leaf_cell> leaf_outliers(const leaf_predictive_result& res) {
    const size_t T = res.n_species();
    std::vector<leaf_cell> cells;
    std::vector<double> p;
    for (size_t at = 0; at < res.mean.size(); ++at) {
        if (!std::isfinite(res.p_obs[at]) || !std::isfinite(res.p_below[at]) || !std::isfinite(res.p_above[at])) continue;
        leaf_cell c;
        c.family = at / T; c.species = at % T;
        c.p_low = res.p_below[at] + res.p_obs[at];
        c.p_high = res.p_obs[at] + res.p_above[at];
        c.low = c.p_low <= c.p_high;
        c.p = std::min(1.0, 2 * std::min(c.p_low, c.p_high));
        cells.push_back(c);
        p.push_back(c.p);
    }
    const std::vector<double> adj = holm_adjusted(p);
    for (size_t i = 0; i < cells.size(); ++i) cells[i].holm = adj[i];
    std::stable_sort(cells.begin(), cells.end(), [](const leaf_cell& a, const leaf_cell& b) { return a.holm != b.holm ? a.holm < b.holm : a.p < b.p; });
    return cells;
}

std::vector<species_fit> leaf_species_fit(const leaf_predictive_result& res, const std::vector<leaf_cell>& cells, double threshold) {
    const size_t T = res.n_species();
    std::vector<species_fit> fit(T);
    std::vector<double> z(T, 0.0);
    std::vector<size_t> nz(T, 0);
    for (const leaf_cell& c : cells) {
        species_fit& s = fit[c.species];
        const size_t at = c.family * T + c.species;
        ++s.cells;
        if (res.sd[at] > 0) { z[c.species] += (res.observed[at] - res.mean[at]) / res.sd[at]; ++nz[c.species]; }
        if (c.holm <= threshold) ++(c.low ? s.low : s.high);
        if (res.p_obs[at] > 0) s.log_p_obs += std::log(res.p_obs[at]);
    }
    for (size_t t = 0; t < T; ++t) if (nz[t]) fit[t].mean_z = z[t] / (double)nz[t];
    return fit;
}

leaf_predictive_summary write_leaf_predictive_reports(const leaf_predictive_result& res, double threshold, const std::string& model_identifier,
                                                      const std::string& dir, const std::vector<gene_family>& families) {
    const std::string prefix = (dir.empty() ? std::string("results") : dir) + "/" + model_identifier;
    const size_t T = res.n_species();
    char buf[256];
    std::ofstream table(prefix + "_leaf_predictive.tab");
    table << "FamilyID";
    for (const std::string& s : res.species) table << "\t" << s;
    table << std::endl;
    leaf_predictive_summary sum;
    for (size_t f = 0; f < families.size(); ++f) {
        table << families[f].id();
        for (size_t t = 0; t < T; ++t) {
            const size_t at = f * T + t;
            if (res.observed[at] == kCountMissing && std::isfinite(res.mean[at])) {      // no observation: the prediction alone
                std::snprintf(buf, sizeof buf, "\t%.6g:%.6g:NA:NA", res.mean[at], res.sd[at]);
                table << buf;
                continue;
            }
            if (!std::isfinite(res.p_obs[at])) { table << "\t-"; ++sum.failed_cells; continue; }
            std::snprintf(buf, sizeof buf, "\t%.6g:%.6g:%.6g:%.6g", res.mean[at], res.sd[at], res.p_below[at] + res.p_obs[at], res.p_obs[at] + res.p_above[at]);
            table << buf;
        }
        table << std::endl;
    }
    const std::vector<leaf_cell> cells = leaf_outliers(res);
    std::ofstream out(prefix + "_leaf_outliers.tab");
    out << "#FamilyID\tSpecies\tObserved\tMean\tSD\tDirection\tP\tHolmP\t(two-sided p of the observed count under its leave-one-out predictive distribution; Holm over "
        << cells.size() << " cells; threshold " << threshold << ")" << std::endl;
    for (const leaf_cell& c : cells) {
        if (!(c.holm <= threshold)) break;
        const size_t at = c.family * T + c.species;
        std::snprintf(buf, sizeof buf, "\t%d\t%.6g\t%.6g\t%s\t%.6g\t%.6g", res.observed[at], res.mean[at], res.sd[at], c.low ? "low" : "high", c.p, c.holm);
        out << families[c.family].id() << "\t" << res.species[c.species] << buf << std::endl;
        ++sum.outliers;
    }
    const std::vector<species_fit> fit = leaf_species_fit(res, cells, threshold);
    std::ofstream sp(prefix + "_species_fit.tab");
    sp << "#Species\tCells\tMeanZ\tOutliersLow\tOutliersHigh\tSumLogPObs" << std::endl;
    for (size_t t = 0; t < T; ++t) {
        std::snprintf(buf, sizeof buf, "\t%zu\t%.6g\t%zu\t%zu\t%.12g", fit[t].cells, fit[t].mean_z, fit[t].low, fit[t].high, fit[t].log_p_obs);
        sp << res.species[t] << buf << std::endl;
        sum.log_pseudo_likelihood += fit[t].log_p_obs;
    }
    return sum;
}

std::vector<imputed_cell> imputed_cells(const leaf_predictive_result& res) {
    const size_t T = res.n_species();
    std::vector<imputed_cell> out;
    for (size_t at = 0; at < res.observed.size(); ++at) {
        if (res.observed[at] != kCountMissing) continue;
        imputed_cell c{at / T, at % T, res.mean[at], res.sd[at], 0, 0};
        if (std::isfinite(c.mean) && std::isfinite(c.sd)) {
            c.lo = std::max(0L, (long)std::floor(c.mean - 1.959963984540054 * c.sd));
            c.hi = std::max(c.lo, (long)std::ceil(c.mean + 1.959963984540054 * c.sd));
        }
        out.push_back(c);
    }
    return out;
}

size_t write_imputed_counts(const leaf_predictive_result& res, const std::string& model_identifier, const std::string& dir,
                            const std::vector<gene_family>& families) {
    std::ofstream f((dir.empty() ? std::string("results") : dir) + "/" + model_identifier + "_imputed_counts.tab");
    f << "#FamilyID\tSpecies\tMean\tSD\tLo95\tHi95\t(the count of a missing cell predicted from the family's observed species; Lo95 - Hi95: the central 95 % "
         "interval of the normal distribution with that mean and sd, in whole genes)" << std::endl;
    char buf[160];
    const std::vector<imputed_cell> cells = imputed_cells(res);
    for (const imputed_cell& c : cells) {
        if (std::isfinite(c.mean) && std::isfinite(c.sd)) std::snprintf(buf, sizeof buf, "\t%.6g\t%.6g\t%ld\t%ld", c.mean, c.sd, c.lo, c.hi);
        else std::snprintf(buf, sizeof buf, "\t-\t-\t-\t-");
        f << families[c.family].id() << "\t" << res.species[c.species] << buf << std::endl;
    }
    return cells.size();
}

}  // namespace cafe
