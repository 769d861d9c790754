// Standard errors of the fitted rates from the per-family scores (cafe_score_gradient): the information matrix is the outer
// product sum_f s_f s_f^T of the scores s_f = d lnL_f / d theta at the optimum, the covariance its inverse.  The reference
// reports no uncertainty; this is what `cafexp_hip --standard-errors` writes to <Model>_standard_errors.txt.
#include <cmath>
#include <fstream>
#include <limits>

#include "cafe_host.h"
#include "../../include/cafe_mi355x.h"

namespace cafe {

gradient_result hip_model_base::score_gradient(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist, int root_rule) {
    std::vector<double> mult, probs;
    double alpha = 0;
    category_parameters(mult, probs, alpha);
    const int K = mult.empty() ? 1 : (int)mult.size();
    ensure_context(K);
    std::vector<float> prior_f;
    std::vector<double> err, lambdas;
    gather_call_inputs(prior, rootdist, prior_f, err, lambdas);
    cafe_params pr{};
    pr.model = mult.empty() ? CAFE_MODEL_BASE : CAFE_MODEL_GAMMA;
    pr.lambdas = lambdas.data(); pr.n_categories = K;
    pr.multipliers = mult.empty() ? nullptr : mult.data();
    pr.cat_probs = probs.empty() ? nullptr : probs.data();
    pr.alpha = alpha; pr.prior = prior_f.data(); pr.error_model = err.empty() ? nullptr : err.data();
    const size_t F = _p_gene_families->size(), nl = lambdas.size();
    gradient_result res;
    res.n_lambdas = nl; res.n_categories = mult.empty() ? 0 : (size_t)K;
    res.family_lnl.resize(F); res.failed.resize(F); res.d_lambda.resize(F * nl);
    cafe_gradient_out out{};
    out.family_lnl = res.family_lnl.data(); out.failed = res.failed.data(); out.d_lambda = res.d_lambda.data();
    if (!_death_rates.empty()) { res.d_mu.resize(F * nl); out.d_mu = res.d_mu.data(); }
    if (!mult.empty()) { res.d_multiplier.resize(F * K); out.d_multiplier = res.d_multiplier.data(); }
    if (cafe_score_gradient(_ctx, &pr, root_rule, &out) != CAFE_OK)
        throw std::runtime_error(std::string("cafe_score_gradient: ") + cafe_last_error(_ctx));
    return res;
}

// The inverse of a symmetric positive definite matrix by Gauss-Jordan elimination with full pivoting on its correlation form
// (rows and columns scaled by 1 / sqrt(diagonal)); false when a diagonal entry is not positive or a pivot falls below 1e-12
// of the unit scale: singular or too ill-conditioned to report.  (rate_shift_scan.cpp inverts its T^T G T with it.)
bool invert_information(const std::vector<double>& A, size_t n, std::vector<double>& inv) {
    std::vector<double> s(n);
    for (size_t i = 0; i < n; ++i) {
        if (!(A[i * n + i] > 0) || !std::isfinite(A[i * n + i])) return false;
        s[i] = 1.0 / std::sqrt(A[i * n + i]);
    }
    std::vector<double> a(n * n), b(n * n, 0.0);
    for (size_t i = 0; i < n; ++i) {
        b[i * n + i] = 1.0;
        for (size_t j = 0; j < n; ++j) a[i * n + j] = A[i * n + j] * s[i] * s[j];
    }
    std::vector<size_t> colperm(n);
    for (size_t i = 0; i < n; ++i) colperm[i] = i;
    for (size_t k = 0; k < n; ++k) {
        size_t pr = k, pc = k;
        double best = 0;
        for (size_t i = k; i < n; ++i)
            for (size_t j = k; j < n; ++j) if (std::fabs(a[i * n + j]) > best) { best = std::fabs(a[i * n + j]); pr = i; pc = j; }
        if (!(best > 1e-12)) return false;
        if (pr != k) for (size_t j = 0; j < n; ++j) { std::swap(a[pr * n + j], a[k * n + j]); std::swap(b[pr * n + j], b[k * n + j]); }
        if (pc != k) { for (size_t i = 0; i < n; ++i) std::swap(a[i * n + pc], a[i * n + k]); std::swap(colperm[pc], colperm[k]); }
        const double piv = a[k * n + k];
        for (size_t j = 0; j < n; ++j) { a[k * n + j] /= piv; b[k * n + j] /= piv; }
        for (size_t i = 0; i < n; ++i) {
            if (i == k) continue;
            const double f = a[i * n + k];
            if (f == 0) continue;
            for (size_t j = 0; j < n; ++j) { a[i * n + j] -= f * a[k * n + j]; b[i * n + j] -= f * b[k * n + j]; }
        }
    }
    inv.assign(n * n, 0.0);                                  // row k of b solves for the unknown colperm[k]
    for (size_t k = 0; k < n; ++k)
        for (size_t j = 0; j < n; ++j) inv[colperm[k] * n + j] = b[k * n + j] * s[colperm[k]] * s[j];
    return true;
}

standard_errors compute_standard_errors(const std::vector<std::string>& names, const std::vector<double>& estimates,
                                        const std::vector<double>& scores, size_t n_families) {
    const size_t P = names.size();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    standard_errors se;
    se.names = names; se.estimate = estimates;
    se.se.assign(P, nan); se.correlation.assign(P * P, nan); se.total_score.assign(P, 0.0); se.information.assign(P * P, 0.0);
    for (size_t f = 0; f < n_families; ++f) {
        bool bad = false;
        for (size_t i = 0; i < P; ++i) bad = bad || !std::isfinite(scores[f * P + i]);
        if (bad) { ++se.families_left_out; continue; }
        ++se.families_used;
        for (size_t i = 0; i < P; ++i) {
            se.total_score[i] += scores[f * P + i];
            for (size_t j = 0; j < P; ++j) se.information[i * P + j] += scores[f * P + i] * scores[f * P + j];
        }
    }
    std::vector<double> cov;
    se.ok = P > 0 && se.families_used > 0 && invert_information(se.information, P, cov);
    if (se.ok)
        for (size_t i = 0; i < P; ++i) se.ok = se.ok && cov[i * P + i] > 0 && std::isfinite(cov[i * P + i]);
    if (!se.ok) return se;
    for (size_t i = 0; i < P; ++i) se.se[i] = std::sqrt(cov[i * P + i]);
    for (size_t i = 0; i < P; ++i)
        for (size_t j = 0; j < P; ++j) se.correlation[i * P + j] = i == j ? 1.0 : cov[i * P + j] / (se.se[i] * se.se[j]);
    return se;
}

std::vector<double> multiplier_slopes(size_t n_categories, double alpha) {
    const double h = 1e-2 * alpha;
    std::vector<double> probs(n_categories), up(n_categories), down(n_categories), out(n_categories);
    get_gamma(probs, up, alpha + h);
    get_gamma(probs, down, alpha - h);
    for (size_t k = 0; k < n_categories; ++k) out[k] = (up[k] - down[k]) / (2 * h);
    return out;
}

void write_standard_errors(const standard_errors& se, const std::string& model_identifier, const std::string& dir, const std::string& conditional_on) {
    const std::string path = (dir.empty() ? std::string("results") : dir) + "/" + model_identifier + "_standard_errors.txt";
    std::ofstream f(path);
    f.precision(17);
    const size_t P = se.names.size();
    f << "# Standard errors from the outer product of the per-family scores; " << se.families_used << " families";
    if (se.families_left_out) f << " (" << se.families_left_out << " left out: no finite score)";
    f << "\nParameter\tEstimate\tSE\tLower95\tUpper95\n";
    for (size_t i = 0; i < P; ++i)
        f << se.names[i] << '\t' << se.estimate[i] << '\t' << se.se[i] << '\t' << se.estimate[i] - 1.959963984540054 * se.se[i] << '\t'
          << se.estimate[i] + 1.959963984540054 * se.se[i] << '\n';
    f << "Correlation\n";
    for (size_t i = 0; i < P; ++i) {
        f << se.names[i];
        for (size_t j = 0; j < P; ++j) f << '\t' << se.correlation[i * P + j];
        f << '\n';
    }
    f << "Total score (sum over the families; near 0 at a converged optimum)\n";
    for (size_t i = 0; i < P; ++i) f << se.names[i] << '\t' << se.total_score[i] << '\n';
    f << "# The errors are conditional on " << conditional_on << ".\n";
    if (!f) throw std::runtime_error("Failed to write " + path);
}

}  // namespace cafe
