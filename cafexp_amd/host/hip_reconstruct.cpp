// Pupko reconstruction and Viterbi branch probabilities of the hip models: the reference's
// model::reconstruct_ancestral_states (base_model.cpp:145, gamma_core.cpp:301) and the compute_viterbi_sum loop of
// estimator::execute (execute.cpp:163-176), forwarded to cafe_reconstruct / cafe_branch_probabilities.
#include "cafe_host.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>

#include "../../include/cafe_mi355x.h"

namespace cafe {

std::vector<int32_t> hip_model_base::device_reconstruct(const std::vector<gene_family>& families, root_equilibrium_distribution* p_prior,
                                                        const std::vector<double>* multipliers) {
    if (&families != _p_gene_families && families.size() != _p_gene_families->size())
        throw std::runtime_error("reconstruct_ancestral_states: the family list must be the model's own");
    const int K = multipliers ? (int)multipliers->size() : 1;
    ensure_context(K);
    const int jmax = std::min(_max_family_size, _max_root_family_size);
    std::vector<float> root_prior(jmax + 1);
    for (int j = 0; j <= jmax; ++j) root_prior[j] = p_prior->compute(j);       // as left by the last inference call (execute.cpp:163)
    std::vector<double> lambdas = _p_lambda->values();
    cafe_params pr{};
    pr.model = multipliers ? CAFE_MODEL_GAMMA : CAFE_MODEL_BASE;
    pr.lambdas = lambdas.data();
    pr.n_categories = K;
    pr.multipliers = multipliers ? multipliers->data() : nullptr;
    std::vector<int32_t> states((size_t)K * families.size() * _order.size());
    if (cafe_reconstruct(_ctx, &pr, root_prior.data(), states.data()) != CAFE_OK)
        throw std::runtime_error(std::string("cafe_reconstruct: ") + cafe_last_error(_ctx));
    return states;
}

std::vector<double> hip_model_base::device_pvalues(int number_of_simulations, uint64_t seed) {
    ensure_context(1);
    std::vector<double> lambdas = _p_lambda->values(), out(_p_gene_families->size());
    cafe_params pr{};
    pr.model = CAFE_MODEL_BASE; pr.lambdas = lambdas.data(); pr.n_categories = 1;
    if (cafe_pvalues(_ctx, &pr, number_of_simulations, seed, out.data()) != CAFE_OK)
        throw std::runtime_error(std::string("cafe_pvalues: ") + cafe_last_error(_ctx));
    return out;
}

std::vector<double> hip_model_base::branch_probability_table(const reconstruction& rec, const std::vector<gene_family>& families,
                                                             const std::vector<const clade*>& order) {
    ensure_context(1);
    const size_t n = _order.size(), F = families.size();
    std::vector<int32_t> sizes(F * n);
    for (size_t f = 0; f < F; ++f)
        for (size_t v = 0; v < n; ++v) sizes[f * n + v] = rec.reconstructed_size(families[f], _order[v]);
    std::vector<double> lambdas = _p_lambda->values(), flat(F * n);
    cafe_params pr{};
    pr.model = CAFE_MODEL_BASE; pr.lambdas = lambdas.data(); pr.n_categories = 1;
    if (cafe_branch_probabilities(_ctx, &pr, sizes.data(), flat.data()) != CAFE_OK)
        throw std::runtime_error(std::string("cafe_branch_probabilities: ") + cafe_last_error(_ctx));
    std::map<const clade*, size_t> pos;
    for (size_t v = 0; v < n; ++v) pos[_order[v]] = v;
    std::vector<double> out(F * order.size());
    for (size_t f = 0; f < F; ++f)
        for (size_t i = 0; i < order.size(); ++i) out[f * order.size() + i] = flat[f * n + pos.at(order[i])];
    return out;
}

marginal_result hip_model_base::marginal_reconstruction(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist, double level,
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
    const size_t n = _order.size(), F = _p_gene_families->size();
    std::vector<double> mean(F * n), pi(F * n), pd(F * n);
    std::vector<int32_t> mode(F * n), lo(F * n), hi(F * n);
    marginal_result res;
    res.level = level; res.n_nodes = order.size();
    res.log_evidence.resize(F); res.failed.resize(F);
    cafe_marginal_out out{};
    out.mean = mean.data(); out.mode = mode.data(); out.lo = lo.data(); out.hi = hi.data(); out.p_increase = pi.data(); out.p_decrease = pd.data();
    out.log_evidence = res.log_evidence.data(); out.failed = res.failed.data();
    if (cafe_marginal_reconstruct(_ctx, &pr, level, &out) != CAFE_OK)
        throw std::runtime_error(std::string("cafe_marginal_reconstruct: ") + cafe_last_error(_ctx));
    std::map<const clade*, size_t> pos;
    for (size_t v = 0; v < n; ++v) pos[_order[v]] = v;
    const size_t m = order.size();
    res.mean.resize(F * m); res.p_increase.resize(F * m); res.p_decrease.resize(F * m);
    res.mode.resize(F * m); res.lo.resize(F * m); res.hi.resize(F * m);
    for (size_t f = 0; f < F; ++f)
        for (size_t i = 0; i < m; ++i) {
            const size_t src = f * n + pos.at(order[i]), dst = f * m + i;
            res.mean[dst] = mean[src]; res.mode[dst] = mode[src]; res.lo[dst] = lo[src]; res.hi[dst] = hi[src];
            res.p_increase[dst] = pi[src]; res.p_decrease[dst] = pd[src];
        }
    return res;
}

void write_marginal_reports(const marginal_result& res, const std::string& model_identifier, const std::string& dir,
                            const std::vector<const clade*>& order, const std::vector<gene_family>& families) {
    const std::string prefix = (dir.empty() ? std::string("results") : dir) + "/" + model_identifier;
    std::ofstream sizes(prefix + "_posterior_sizes.tab"), change(prefix + "_posterior_change.tab");
    for (std::ofstream* f : {&sizes, &change}) {
        *f << "FamilyID";
        for (auto c : order) *f << "\t" << clade_index_or_name(c, order);
        *f << std::endl;
    }
    char buf[128];
    const size_t m = order.size();
    for (size_t i = 0; i < families.size(); ++i) {
        sizes << families[i].id();
        change << families[i].id();
        for (size_t v = 0; v < m; ++v) {
            const size_t at = i * m + v;
            std::snprintf(buf, sizeof buf, "\t%.6g:%d:%d-%d", res.mean[at], res.mode[at], res.lo[at], res.hi[at]);
            sizes << buf;
            if (order[v]->is_root()) change << "\t-";
            else {
                std::snprintf(buf, sizeof buf, "\t%.6g:%.6g", res.p_decrease[at], res.p_increase[at]);
                change << buf;
            }
        }
        sizes << std::endl;
        change << std::endl;
    }
}

events_result hip_model_base::expected_events(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist, const std::vector<const clade*>& order) {
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
    const size_t n = _order.size(), F = _p_gene_families->size(), m = order.size();
    std::vector<double> gains(F * n), losses(F * n);
    events_result res;
    res.n_nodes = m;
    res.failed.resize(F);
    cafe_events_out out{};
    out.gains = gains.data(); out.losses = losses.data(); out.failed = res.failed.data();
    if (cafe_expected_events(_ctx, &pr, &out) != CAFE_OK)
        throw std::runtime_error(std::string("cafe_expected_events: ") + cafe_last_error(_ctx));
    std::map<const clade*, size_t> pos;
    for (size_t v = 0; v < n; ++v) pos[_order[v]] = v;
    res.gains.resize(F * m); res.losses.resize(F * m);
    for (size_t f = 0; f < F; ++f)
        for (size_t i = 0; i < m; ++i) {
            const size_t src = f * n + pos.at(order[i]), dst = f * m + i;
            res.gains[dst] = gains[src]; res.losses[dst] = losses[src];
        }
    return res;
}

void write_events_reports(const events_result& res, const std::string& model_identifier, const std::string& dir,
                          const std::vector<const clade*>& order, const std::vector<gene_family>& families) {
    const std::string prefix = (dir.empty() ? std::string("results") : dir) + "/" + model_identifier;
    std::ofstream cells(prefix + "_expected_events.tab"), totals(prefix + "_branch_events.tab");
    cells << "FamilyID";
    for (auto c : order) cells << "\t" << clade_index_or_name(c, order);
    cells << std::endl;
    char buf[160];
    const size_t m = order.size();
    std::vector<double> g(m, 0.0), l(m, 0.0);
    size_t used = 0;
    for (size_t i = 0; i < families.size(); ++i) {
        cells << families[i].id();
        for (size_t v = 0; v < m; ++v) {
            const size_t at = i * m + v;
            if (order[v]->is_root()) { cells << "\t-"; continue; }
            std::snprintf(buf, sizeof buf, "\t%.6g:%.6g", res.gains[at], res.losses[at]);
            cells << buf;
            if (!res.failed[i]) { g[v] += res.gains[at]; l[v] += res.losses[at]; }
        }
        cells << std::endl;
        used += res.failed[i] == 0;
    }
    totals << "#Node\tgains\tlosses\tnet\tturnover\t(expected events summed over " << used << " families; " << families.size() - used << " failed)" << std::endl;
    for (size_t v = 0; v < m; ++v) {
        if (order[v]->is_root()) continue;
        std::snprintf(buf, sizeof buf, "\t%.12g\t%.12g\t%.12g\t%.12g", g[v], l[v], g[v] - l[v], g[v] + l[v]);
        totals << clade_index_or_name(order[v], order) << buf << std::endl;
    }
}

branch_change_result hip_model_base::branch_change(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist, int max_change, double level,
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
    const size_t n = _order.size(), F = _p_gene_families->size(), m = order.size();
    std::vector<double> mean(F * n), below(F * n), above(F * n);
    std::vector<int32_t> mode(F * n), lo(F * n), hi(F * n);
    branch_change_result res;
    res.max_change = max_change; res.level = level;
    res.failed.resize(F);
    cafe_branch_change_out out{};                            // the band itself is not asked for: nothing of its size leaves the call
    out.mean = mean.data(); out.below = below.data(); out.above = above.data(); out.mode = mode.data(); out.lo = lo.data(); out.hi = hi.data();
    out.failed = res.failed.data();
    if (cafe_branch_change(_ctx, &pr, max_change, level, &out) != CAFE_OK)
        throw std::runtime_error(std::string("cafe_branch_change: ") + cafe_last_error(_ctx));
    std::map<const clade*, size_t> pos;
    for (size_t v = 0; v < n; ++v) pos[_order[v]] = v;
    for (const clade* c : order) { res.names.push_back(clade_index_or_name(c, order)); res.root.push_back(c->is_root() ? 1 : 0); }
    for (std::vector<double>* v : {&res.mean, &res.below, &res.above}) v->resize(F * m);
    for (std::vector<int32_t>* v : {&res.mode, &res.lo, &res.hi}) v->resize(F * m);
    for (size_t f = 0; f < F; ++f)
        for (size_t i = 0; i < m; ++i) {
            const size_t src = f * n + pos.at(order[i]), dst = f * m + i;
            res.mean[dst] = mean[src]; res.below[dst] = below[src]; res.above[dst] = above[src];
            res.mode[dst] = mode[src]; res.lo[dst] = lo[src]; res.hi[dst] = hi[src];
        }
    return res;
}

leaf_predictive_result hip_model_base::leaf_predictive(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist) {
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
    leaf_predictive_result res;
    for (const clade* c : _order) if (c->is_leaf()) res.species.push_back(c->get_taxon_name());      // the columns of the context's counts
    const size_t F = _p_gene_families->size(), T = res.species.size();
    res.observed.resize(F * T);
    for (size_t f = 0; f < F; ++f)
        for (size_t t = 0; t < T; ++t) res.observed[f * T + t] = (*_p_gene_families)[f].get_species_size(res.species[t]);
    for (std::vector<double>* v : {&res.mean, &res.sd, &res.p_below, &res.p_obs, &res.p_above}) v->assign(F * T, NAN);
    res.failed.resize(F);
    cafe_leaf_predictive_out out{};
    out.mean = res.mean.data(); out.sd = res.sd.data(); out.p_below = res.p_below.data(); out.p_obs = res.p_obs.data();
    out.p_above = res.p_above.data(); out.failed = res.failed.data();
    if (cafe_leaf_predictive(_ctx, &pr, &out) != CAFE_OK)
        throw std::runtime_error(std::string("cafe_leaf_predictive: ") + cafe_last_error(_ctx));
    return res;
}

history_result hip_model_base::sample_histories(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist, int n_draws, uint64_t seed,
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
    if (n_draws < 1) throw std::runtime_error("cafe_sample_histories: the number of draws must be positive");
    const size_t n = _order.size(), D = (size_t)n_draws;
    std::vector<int64_t> inc(D * n), dec(D * n), net(D * n);
    history_result res;
    res.n_draws = D; res.n_nodes = order.size(); res.seed = seed;
    res.failed.resize(_p_gene_families->size());
    cafe_history_out out{};
    out.n_increase = inc.data(); out.n_decrease = dec.data(); out.net_change = net.data(); out.failed = res.failed.data();
    if (cafe_sample_histories(_ctx, &pr, n_draws, seed, &out) != CAFE_OK)
        throw std::runtime_error(std::string("cafe_sample_histories: ") + cafe_last_error(_ctx));
    std::map<const clade*, size_t> pos;
    for (size_t v = 0; v < n; ++v) pos[_order[v]] = v;
    const size_t m = order.size();
    res.n_increase.resize(D * m); res.n_decrease.resize(D * m); res.net_change.resize(D * m);
    for (size_t d = 0; d < D; ++d)
        for (size_t i = 0; i < m; ++i) {
            const size_t src = d * n + pos.at(order[i]), dst = d * m + i;
            res.n_increase[dst] = inc[src]; res.n_decrease[dst] = dec[src]; res.net_change[dst] = net[src];
        }
    return res;
}

void write_history_reports(const history_result& res, double level, const std::string& model_identifier, const std::string& dir,
                           const std::vector<const clade*>& order) {
    const std::string prefix = (dir.empty() ? std::string("results") : dir) + "/" + model_identifier;
    std::ofstream f(prefix + "_sampled_change.tab");
    f << "#Node\tn_increase\tn_decrease\tnet_change\t(mean:lo-hi over " << res.n_draws << " draws, level " << level << ", seed " << res.seed << ")" << std::endl;
    char buf[160];
    const size_t m = order.size(), D = res.n_draws;
    std::vector<int64_t> col(D);
    for (size_t v = 0; v < m; ++v) {
        f << clade_index_or_name(order[v], order);
        for (const std::vector<int64_t>* a : {&res.n_increase, &res.n_decrease, &res.net_change}) {
            double sum = 0;
            for (size_t d = 0; d < D; ++d) { col[d] = (*a)[d * m + v]; sum += (double)col[d]; }
            std::sort(col.begin(), col.end());
            // the least value whose empirical CDF (rank / D) reaches the threshold
            auto at = [&](double thr) { size_t r = 0; while (r + 1 < D && (double)(r + 1) / (double)D < thr) ++r; return col[r]; };
            std::snprintf(buf, sizeof buf, "\t%.6g:%lld-%lld", sum / (double)D, (long long)at(0.5 * (1.0 - level)), (long long)at(1.0 - 0.5 * (1.0 - level)));
            f << buf;
        }
        f << std::endl;
    }
}

reconstruction* hip_base_model::reconstruct_ancestral_states(const std::vector<gene_family>& families, root_equilibrium_distribution* p_prior) {
    const std::vector<int32_t> states = device_reconstruct(families, p_prior, nullptr);
    auto result = new base_model_reconstruction();
    const size_t n = _order.size();
    for (size_t f = 0; f < families.size(); ++f) {
        auto& m = result->_reconstructions[families[f].id()];
        for (size_t v = 0; v < n; ++v)
            if (!_order[v]->is_leaf()) m[_order[v]] = states[f * n + v];          // leaves are read from the family (base_model.cpp:183)
    }
    return result;
}

reconstruction* hip_gamma_model::reconstruct_ancestral_states(const std::vector<gene_family>& families, root_equilibrium_distribution* p_prior) {
    if (_category_likelihoods.size() != families.size())
        throw std::runtime_error("reconstruct_ancestral_states: run infer_family_likelihoods first (category likelihoods are copied, gamma_core.cpp:323)");
    const std::vector<int32_t> states = device_reconstruct(families, p_prior, &_lambda_multipliers);
    auto result = new gamma_model_reconstruction(_lambda_multipliers);
    const size_t n = _order.size(), F = families.size(), K = _lambda_multipliers.size();
    for (size_t f = 0; f < F; ++f) {
        auto& r = result->_reconstructions[families[f].id()];
        r._category_likelihoods = _category_likelihoods[f];
        r.category_reconstruction.resize(K);
        for (size_t k = 0; k < K; ++k)
            for (size_t v = 0; v < n; ++v)
                if (!_order[v]->is_leaf()) r.category_reconstruction[k][_order[v]] = states[(k * F + f) * n + v];
        r.reconstruction = get_weighted_averages(r.category_reconstruction, _gamma_cat_probs);
    }
    return result;
}

branch_probabilities compute_branch_probabilities(hip_model_base& mdl, const reconstruction& rec, const std::vector<gene_family>& families,
                                                  const std::vector<double>& pvalues, double test_pvalue, const cladevector& order) {
    branch_probabilities probs;
    bool any = false;
    for (double p : pvalues) any = any || p < test_pvalue;
    if (!any) return probs;
    const std::vector<double> table = mdl.branch_probability_table(rec, families, order);
    for (size_t i = 0; i < families.size(); ++i) {
        if (!(pvalues[i] < test_pvalue)) continue;
        for (size_t j = 0; j < order.size(); ++j) {
            const double v = table[i * order.size() + j];
            probs.set(families[i], order[j], std::isnan(v) ? branch_probabilities::invalid() : branch_probabilities::branch_probability(v));
        }
    }
    return probs;
}

}  // namespace cafe
