// Rate-shift scan: Rao's efficient score test of a change of the turnover rate on every branch and in every clade, from
// one cafe_branch_scores call at the fitted optimum -- the total U and the Gram matrix G of the per-family score vectors,
// formed on the device -- instead of one refit per candidate lambda tree.  The searched global parameters are profiled out
// through G as `cafexp_hip --standard-errors` treats them (lambda and mu as they are, alpha through d_multiplier and
// d multiplier_k / d alpha); this is what `cafexp_hip --rate-shift-scan` writes to <Model>_rate_shift_scan.tab.
#include <algorithm>
#include <cmath>
#include <fstream>
#include <limits>

#include "cafe_host.h"
#include "../../include/cafe_mi355x.h"

namespace cafe {

branch_scores_result hip_model_base::branch_scores(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist, int root_rule,
                                                   const std::vector<const clade*>& order) {
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
    int32_t P = 0;
    if (cafe_branch_scores_dim(_ctx, &pr, &P) != CAFE_OK) throw std::runtime_error("cafe_branch_scores_dim failed");
    branch_scores_result res;
    res.P = (size_t)P; res.n_branch = _order.size() - 1; res.n_par = _death_rates.empty() ? 1 : 2;
    res.n_lambdas = lambdas.size(); res.n_categories = mult.empty() ? 0 : (size_t)K;
    res.total.resize(res.P); res.gram.resize(res.P * res.P);
    std::vector<int32_t> failed(_p_gene_families->size());
    int64_t used = 0;
    cafe_branch_scores_out out{};
    out.total = res.total.data(); out.gram = res.gram.data(); out.n_used = &used; out.failed = failed.data();
    if (cafe_branch_scores(_ctx, &pr, root_rule, &out) != CAFE_OK)
        throw std::runtime_error(std::string("cafe_branch_scores: ") + cafe_last_error(_ctx));
    res.families_used = (size_t)used;
    for (int32_t f : failed) res.families_failed += f != 0;
    std::map<const clade*, int> slot;                        // the library's node order is _order; the root has no score
    int next = 0;
    for (const clade* c : _order) slot[c] = c->is_root() ? -1 : next++;
    for (const clade* c : order) res.slot.push_back(slot.at(c));
    return res;
}

namespace {

// x^T G y over sparse x and y (index lists with unit entries) or dense ones: the directions here are sums of unit vectors
double quad(const std::vector<double>& G, size_t P, const std::vector<size_t>& x, const std::vector<size_t>& y) {
    double s = 0;
    for (size_t i : x) for (size_t j : y) s += G[i * P + j];
    return s;
}

void holm_adjust(std::vector<score_test*>& tests) {
    std::vector<score_test*> t;
    std::vector<double> p;
    for (score_test* x : tests) if (x->testable) { t.push_back(x); p.push_back(x->p); }
    const std::vector<double> adj = holm_adjusted(p);
    for (size_t i = 0; i < t.size(); ++i) t[i]->holm = adj[i];
}

}  // namespace

rate_shift_scan compute_rate_shift_scan(const branch_scores_result& bs, const std::vector<const clade*>& order,
                                        const std::vector<std::vector<double>>& theta, const std::vector<std::string>& names) {
    const size_t P = bs.P, nt = theta.size();
    const std::vector<double>& G = bs.gram;
    rate_shift_scan scan;
    scan.two_rates = bs.n_par == 2;
    scan.families_used = bs.families_used; scan.families_failed = bs.families_failed;
    scan.profiled = names;
    // G T [P][nt], T^T U, (T^T G T)^-1
    std::vector<double> GT(P * nt, 0.0), Ut(nt, 0.0), Gtt(nt * nt, 0.0), inv;
    for (size_t a = 0; a < nt; ++a) {
        for (size_t i = 0; i < P; ++i) {
            double s = 0;
            for (size_t j = 0; j < P; ++j) s += G[i * P + j] * theta[a][j];
            GT[i * nt + a] = s;
        }
        for (size_t j = 0; j < P; ++j) Ut[a] += theta[a][j] * bs.total[j];
    }
    for (size_t a = 0; a < nt; ++a)
        for (size_t b = 0; b < nt; ++b)
            for (size_t i = 0; i < P; ++i) Gtt[a * nt + b] += theta[a][i] * GT[i * nt + b];
    if (nt && !invert_information(Gtt, nt, inv))
        throw std::runtime_error("--rate-shift-scan: the information matrix of the searched parameters is singular or ill-conditioned");
    std::vector<double> invUt(nt, 0.0);
    for (size_t a = 0; a < nt; ++a) for (size_t b = 0; b < nt; ++b) invUt[a] += inv[a * nt + b] * Ut[b];
    // U and V of directions x, y (sums of unit vectors): U_x, and V_xy = x^T G y - x^T G T inv T^T G y
    auto efficient_score = [&](const std::vector<size_t>& x) {
        double u = 0;
        for (size_t i : x) u += bs.total[i];
        for (size_t a = 0; a < nt; ++a) { double g = 0; for (size_t i : x) g += GT[i * nt + a]; u -= g * invUt[a]; }
        return u;
    };
    auto information = [&](const std::vector<size_t>& x, const std::vector<size_t>& y) {
        double v = quad(G, P, x, y);
        std::vector<double> gx(nt, 0.0), gy(nt, 0.0);
        for (size_t a = 0; a < nt; ++a) { for (size_t i : x) gx[a] += GT[i * nt + a]; for (size_t i : y) gy[a] += GT[i * nt + a]; }
        for (size_t a = 0; a < nt; ++a) for (size_t b = 0; b < nt; ++b) v -= gx[a] * inv[a * nt + b] * gy[b];
        return v;
    };
    auto one_df = [&](const std::vector<size_t>& x) {
        score_test t;
        t.U = efficient_score(x); t.V = information(x, x);
        t.testable = t.V > 1e-12 * quad(G, P, x, x);
        if (!t.testable) { t.U = t.V = NAN; return t; }
        t.T = t.U * t.U / t.V;
        t.p = std::erfc(std::sqrt(t.T / 2));
        t.multiplier = std::exp(t.U / t.V);
        return t;
    };
    std::map<const clade*, size_t> at;
    for (size_t i = 0; i < order.size(); ++i) at[order[i]] = i;
    for (size_t i = 0; i < order.size(); ++i) {
        if (bs.slot[i] < 0) continue;
        rate_shift_row row;
        row.node = order[i];
        std::vector<size_t> branch, below;
        std::vector<const clade*> todo{order[i]};
        while (!todo.empty()) {
            const clade* c = todo.back();
            todo.pop_back();
            for (size_t p = 0; p < bs.n_par; ++p) below.push_back(p * bs.n_branch + (size_t)bs.slot[at.at(c)]);
            for (const clade* d : c->descendants()) todo.push_back(d);
        }
        for (size_t p = 0; p < bs.n_par; ++p) branch.push_back(p * bs.n_branch + (size_t)bs.slot[i]);
        row.branch = one_df(branch);
        row.subtree = one_df(below);
        if (scan.two_rates) {
            const std::vector<size_t> b{branch[0]}, d{branch[1]};
            const double u0 = efficient_score(b), u1 = efficient_score(d);
            const double v00 = information(b, b), v01 = information(b, d), v11 = information(d, d);
            const double g00 = quad(G, P, b, b), g11 = quad(G, P, d, d), det = v00 * v11 - v01 * v01;
            row.joint_testable = v00 > 1e-12 * g00 && v11 > 1e-12 * g11 && det > 1e-12 * g00 * g11;
            if (row.joint_testable) {
                row.joint_T = (u0 * u0 * v11 - 2 * u0 * u1 * v01 + u1 * u1 * v00) / det;
                row.joint_p = std::exp(-row.joint_T / 2);
            }
        }
        scan.rows.push_back(row);
    }
    std::vector<score_test*> col;
    for (rate_shift_row& r : scan.rows) col.push_back(&r.branch);
    holm_adjust(col);
    col.clear();
    for (rate_shift_row& r : scan.rows) col.push_back(&r.subtree);
    holm_adjust(col);
    for (size_t i = 0; i < scan.rows.size(); ++i) {
        const score_test& t = scan.rows[i].subtree;
        if (!t.testable) continue;
        if (scan.best < 0 || t.holm < scan.rows[scan.best].subtree.holm ||
            (t.holm == scan.rows[scan.best].subtree.holm && t.p < scan.rows[scan.best].subtree.p)) scan.best = (int)i;
    }
    return scan;
}

void write_rate_shift_scan(const rate_shift_scan& scan, const std::string& model_identifier, const std::string& dir, const std::vector<const clade*>& order) {
    const std::string path = (dir.empty() ? std::string("results") : dir) + "/" + model_identifier + "_rate_shift_scan.tab";
    std::ofstream f(path);
    f << "# Score tests of a rate shift at the fitted optimum; " << scan.families_used << " families";
    if (scan.families_failed) f << " (" << scan.families_failed << " left out: no finite score)";
    f << "; profiled:";
    for (const std::string& n : scan.profiled) f << ' ' << n;
    if (scan.profiled.empty()) f << " nothing";
    f << "\n#Node\tBranchU\tBranchV\tBranchT\tBranchP\tBranchHolmP\tBranchMultiplier\tCladeU\tCladeV\tCladeT\tCladeP\tCladeHolmP\tCladeMultiplier";
    if (scan.two_rates) f << "\tBirthDeathT\tBirthDeathP";
    f << "\tNote\n";
    char buf[400];
    auto num = [&](double v) { std::snprintf(buf, sizeof buf, "\t%.12g", v); return std::isnan(v) ? std::string("\tnan") : std::string(buf); };
    for (const rate_shift_row& r : scan.rows) {
        f << clade_index_or_name(r.node, order);
        for (const score_test* t : {&r.branch, &r.subtree}) f << num(t->U) << num(t->V) << num(t->T) << num(t->p) << num(t->holm) << num(t->multiplier);
        if (scan.two_rates) f << num(r.joint_T) << num(r.joint_p);
        std::string note;
        if (!r.branch.testable) note += "branch not testable";
        if (!r.subtree.testable) note += std::string(note.empty() ? "" : "; ") + "clade not testable";
        if (scan.two_rates && !r.joint_testable) note += std::string(note.empty() ? "" : "; ") + "birth-death not testable";
        f << '\t' << (note.empty() ? "-" : note) << '\n';
    }
    if (!f) throw std::runtime_error("Failed to write " + path);
}

void write_rate_shift_lambda_tree(const rate_shift_scan& scan, const clade* tree, const std::string& model_identifier, const std::string& dir) {
    const std::string path = (dir.empty() ? std::string("results") : dir) + "/" + model_identifier + "_rate_shift_lambda_tree.txt";
    std::set<const clade*> shifted;
    std::vector<const clade*> todo{scan.rows.at((size_t)scan.best).node};
    while (!todo.empty()) {
        const clade* c = todo.back();
        todo.pop_back();
        shifted.insert(c);
        for (const clade* d : c->descendants()) todo.push_back(d);
    }
    std::ofstream f(path);
    tree->write_newick(f, [&](const clade* c) {
        std::string s = c->is_leaf() ? c->get_taxon_name() : std::string();
        if (!c->is_root()) s += shifted.count(c) ? ":2" : ":1";
        return s;
    });
    f << ";\n";
    if (!f) throw std::runtime_error("Failed to write " + path);
}

}  // namespace cafe
