// The reference's simulator (-s; src/simulator.cpp:22-186, src/probability.cpp:320-377, src/root_distribution.cpp)
// above the C ABI.
//
// simulate_families follows the reference draw for draw on the global randomizer_engine: per chunk of
// LAMBDA_PERTURBATION_STEP_SIZE families the simulation lambda (a gamma draw for the gamma model), per family the root
// size, then the prefix traversal with the same libstdc++ distribution objects (the uniform_int draw a saturated branch
// throws away, the discrete_distribution over the S weights of row `parent size`, the error model's uniform at leaves).
// The rows come from cafe_build_matrices (order S, row-major): no transition probability is computed on the host.  With death
// rates (one mu per lambda; a chunk's multiplier scales both rates) they come from cafe_build_matrices_lm, and the draw a
// saturated branch throws away follows the library's rule for the pair (cafe_bd_rates).
//
// simulate_families_device draws only the root sizes and the chunk multipliers on the host (an engine seeded by the
// seed, the same distributions) and hands the families to cafe_simulate (cafe_simulate_lm with death rates): the same
// distribution, a different sample.
#include "cafe_host.h"

#include <algorithm>
#include <charconv>
#include <cmath>
#include <iostream>
#include <numeric>
#include <ostream>
#include <tuple>

#include "../../include/cafe_mi355x.h"

namespace cafe {

// ---------------------------------------------------------------- root_distribution (root_distribution.cpp)
void root_distribution::vectorize_increasing(int max) {
    _v.resize(max);
    std::iota(_v.begin(), _v.end(), 0);
}

int root_distribution::max() const {
    if (_v.empty()) throw std::runtime_error("Root distribution not created yet");
    return *std::max_element(_v.begin(), _v.end());
}

int root_distribution::select_randomly(std::mt19937& engine) const {
    std::uniform_int_distribution<> dis(0, (int)_v.size() - 1);
    return _v[dis(engine)];
}

void root_distribution::pare(size_t new_size, std::mt19937& engine) {
    if (_v.size() < new_size) return;
    std::shuffle(_v.begin(), _v.end(), engine);
    _v.erase(_v.begin() + new_size, _v.end());
    std::sort(_v.begin(), _v.end());
}

namespace {

const int kSimulationMaxSize = 100;               // simulator.cpp:45, :70 without a root distribution
const char* kErrorModelMessage = "Trying to simulate leaf family size that was not included in error model";   // probability.cpp:361

bool saturated(double branch_length, double lambda) {          // matrix_cache.cpp:113-118
    const double alpha = lambda * branch_length / (1 + lambda * branch_length);
    return (1 - 2 * alpha) < 0;
}

// simulate_processes' root distribution and family count (simulator.cpp:62-81)
root_distribution simulation_roots(const std::map<int, int>& rootdist, int nsims, std::mt19937& engine, size_t& n_families, int& S) {
    root_distribution rd;
    if (rootdist.empty()) {
        n_families = nsims > 0 ? (size_t)nsims : 0;
        S = kSimulationMaxSize;
        rd.vectorize_increasing(S);
    } else {
        rd.vectorize(rootdist);
        if (nsims > 0) rd.pare((size_t)nsims, engine);
        n_families = rd.size();
        S = 2 * rd.max();
    }
    return rd;
}

// get_simulation_lambda (base_model.cpp:170: x 1; gamma_core.cpp:88-95: x Gamma(alpha, 1/alpha))
double chunk_multiplier(double alpha, std::mt19937& engine) {
    if (alpha <= 0) return 1.0;
    std::gamma_distribution<double> dist(alpha, 1 / alpha);
    return dist(engine);
}

struct flat_tree {
    std::vector<int32_t> parent, leaf_taxon, lambda_index;
    std::vector<double> branch_length;
    int n_taxa = 0;
};

// the tree in reverse level order (children before parents, root last): the writers' column order
flat_tree flatten(const std::vector<const clade*>& order, const lambda* p_lambda) {
    flat_tree t;
    const int n = (int)order.size();
    std::map<const clade*, int> index;
    for (int i = 0; i < n; ++i) index[order[i]] = i;
    const multiple_lambda* ml = dynamic_cast<const multiple_lambda*>(p_lambda);
    t.parent.resize(n); t.leaf_taxon.resize(n); t.lambda_index.resize(n); t.branch_length.resize(n);
    for (int i = 0; i < n; ++i) {
        const clade* c = order[i];
        t.parent[i] = c->is_root() ? -1 : index.at(c->get_parent());
        t.branch_length[i] = c->is_root() ? 0.0 : c->get_branch_length();
        t.lambda_index[i] = (ml && !c->is_root()) ? ml->index_of(c) : 0;
        t.leaf_taxon[i] = c->is_leaf() ? t.n_taxa++ : -1;
    }
    return t;
}

void check_lambda(const lambda* p_lambda, const std::vector<double>* death_rates) {
    if (!p_lambda) throw std::runtime_error("Cannot simulate without initial lambda values");     // io.cpp:66-69
    if (death_rates && !death_rates->empty() && (int)death_rates->size() != p_lambda->count())
        throw std::runtime_error("--mu needs one death rate per lambda (" + std::to_string(p_lambda->count()) + ")");
}

// the death rate of the branch above c: the mu of its lambda's index
double mu_for_clade(const lambda* p_lambda, const std::vector<double>& mus, const clade* c) {
    const multiple_lambda* ml = dynamic_cast<const multiple_lambda*>(p_lambda);
    return mus[ml ? ml->index_of(c) : 0];
}

}  // namespace

simulation simulate_families(const clade* p_tree, const lambda* p_lambda, const error_model* p_error_model, const std::map<int, int>& rootdist,
                             int nsims, double gamma_alpha, int device, const std::vector<double>* death_rates) {
    check_lambda(p_lambda, death_rates);
    const bool two_rates = death_rates && !death_rates->empty();
    simulation sim;
    p_tree->apply_reverse_level_order([&](const clade* c) { sim.order.push_back(c); });
    const int n = (int)sim.order.size();
    std::map<const clade*, int> index;
    for (int i = 0; i < n; ++i) index[sim.order[i]] = i;
    std::vector<const clade*> prefix;
    p_tree->apply_prefix_order([&](const clade* c) { prefix.push_back(c); });

    int S = 0;
    root_distribution rd = simulation_roots(rootdist, nsims, randomizer_engine, sim.n_families, S);
    sim.max_family_size = S;
    sim.sizes.assign(sim.n_families * n, 0);
    const int root = index.at(p_tree);

    // per chunk: the matrix of every branch (by quantized key, matrix_cache.h:42-61), and the distribution objects per
    // (branch, parent size) -- they keep no state between draws, so one object serves every draw of its row
    std::vector<std::vector<double>> matrix(n);
    std::vector<std::map<int, std::discrete_distribution<int>>> dist(n);
    std::vector<double> chunk_lambda(n, -1.0), chunk_mu(n, -1.0);
    std::vector<char> chunk_saturated(n, 0);
    const size_t step = LAMBDA_PERTURBATION_STEP_SIZE;
    for (size_t i = 0; i < sim.n_families; i += step) {
        const double m = chunk_multiplier(gamma_alpha, randomizer_engine);
        if (gamma_alpha > 0) sim.multipliers.push_back(m);
        std::unique_ptr<lambda> sim_lambda(p_lambda->multiply(m));
        // the rows of this chunk's matrices; branches whose (lambda, t) did not change keep theirs
        std::map<std::tuple<long, long, long>, std::vector<int>> need;
        for (int v = 0; v < n; ++v) {
            if (v == root) continue;
            const double lam = sim_lambda->get_value_for_clade(sim.order[v]);
            const double mu = two_rates ? mu_for_clade(p_lambda, *death_rates, sim.order[v]) * m : lam;
            if (lam == chunk_lambda[v] && mu == chunk_mu[v]) continue;
            chunk_lambda[v] = lam;
            chunk_mu[v] = mu;
            dist[v].clear();
            const double t = sim.order[v]->get_branch_length();
            if (two_rates) {
                double r[3];
                cafe_bd_rates(lam, mu, t, r);
                chunk_saturated[v] = 1 - r[0] - r[1] < 0;
            } else {
                chunk_saturated[v] = saturated(t, lam);
            }
            need[{long(lam * 1000000000), long(mu * 1000000000), long(t * 1000)}].push_back(v);
        }
        if (!need.empty()) {
            std::vector<double> lams, mus, ts, out((size_t)need.size() * S * S);
            for (const auto& kv : need) {
                lams.push_back(chunk_lambda[kv.second[0]]);
                mus.push_back(chunk_mu[kv.second[0]]);
                ts.push_back(sim.order[kv.second[0]]->get_branch_length());
            }
            const int rc = two_rates ? cafe_build_matrices_lm(device, S, (int)need.size(), lams.data(), mus.data(), ts.data(), 0, out.data())
                                     : cafe_build_matrices(device, S, (int)need.size(), lams.data(), ts.data(), 0, out.data());
            if (rc != CAFE_OK) throw std::runtime_error(std::string(two_rates ? "cafe_build_matrices_lm" : "cafe_build_matrices") + " failed with code " + std::to_string(rc));
            size_t k = 0;
            for (const auto& kv : need) {
                for (int v : kv.second) matrix[v].assign(out.begin() + k * S * S, out.begin() + (k + 1) * S * S);
                ++k;
            }
        }
        const size_t end = std::min(sim.n_families, i + step);
        for (size_t j = i; j < end; ++j) {                              // create_trial (simulator.cpp:32-59)
            int32_t* sizes = sim.sizes.data() + j * n;
            sizes[root] = rootdist.empty() ? rd.select_randomly(randomizer_engine) : rd.at(j);
            for (const clade* c : prefix) {                             // set_weighted_random_family_size (:320-352)
                if (c->is_root()) continue;
                const int v = index.at(c);
                const int parent_family_size = sizes[index.at(c->get_parent())];
                int csize = 0;
                if (parent_family_size > 0) {
                    if (chunk_saturated[v]) {                               // drawn, then overwritten (:333-337)
                        std::uniform_int_distribution<int> distribution(0, S - 1);
                        csize = distribution(randomizer_engine);
                    }
                    auto it = dist[v].find(parent_family_size);
                    if (it == dist[v].end()) {
                        const double* p = matrix[v].data() + (size_t)parent_family_size * S;
                        it = dist[v].emplace(parent_family_size, std::discrete_distribution<int>(p, p + S)).first;
                    }
                    csize = it->second(randomizer_engine);
                }
                if (c->is_leaf() && p_error_model) {                    // adjust_for_error_model (:354-377)
                    if ((size_t)csize >= p_error_model->get_max_family_size()) throw std::runtime_error(kErrorModelMessage);
                    const std::vector<double> probs = p_error_model->get_probs((size_t)csize);
                    std::uniform_real_distribution<double> distribution(0.0, 1.0);
                    const double rnd = distribution(randomizer_engine);
                    if (rnd < probs[0]) csize--;
                    else if (rnd > (1 - probs[2])) csize++;
                }
                sizes[v] = csize;
            }
        }
    }
    return sim;
}

simulation simulate_families_device(const clade* p_tree, const lambda* p_lambda, const error_model* p_error_model, const std::map<int, int>& rootdist,
                                    int nsims, double gamma_alpha, int device, uint64_t seed, size_t workspace_limit,
                                    const std::vector<double>* death_rates) {
    check_lambda(p_lambda, death_rates);
    simulation sim;
    p_tree->apply_reverse_level_order([&](const clade* c) { sim.order.push_back(c); });
    const int n = (int)sim.order.size();
    std::mt19937 engine((std::mt19937::result_type)seed);
    int S = 0;
    root_distribution rd = simulation_roots(rootdist, nsims, engine, sim.n_families, S);
    sim.max_family_size = S;
    const size_t step = LAMBDA_PERTURBATION_STEP_SIZE;
    std::vector<int32_t> roots(sim.n_families);
    std::vector<double> mult;
    for (size_t i = 0; i < sim.n_families; i += step) {                // the same order of draws as simulate_processes
        mult.push_back(chunk_multiplier(gamma_alpha, engine));
        for (size_t j = i; j < std::min(sim.n_families, i + step); ++j) roots[j] = rootdist.empty() ? rd.select_randomly(engine) : rd.at(j);
    }
    if (gamma_alpha > 0) sim.multipliers = mult;
    sim.sizes.assign(sim.n_families * n, 0);
    if (sim.n_families == 0) return sim;

    const flat_tree t = flatten(sim.order, p_lambda);
    const std::vector<double> lambdas = p_lambda->values();
    std::vector<double> err_table;
    cafe_sim_problem pb{};
    pb.n_nodes = n; pb.parent = t.parent.data(); pb.branch_length = t.branch_length.data(); pb.lambda_index = t.lambda_index.data();
    pb.leaf_taxon = t.leaf_taxon.data(); pb.n_taxa = t.n_taxa;
    pb.n_lambdas = (int32_t)lambdas.size(); pb.lambdas = lambdas.data();
    pb.max_family_size = S;
    pb.n_families = (int64_t)sim.n_families; pb.root_size = roots.data();
    pb.chunk_size = (int32_t)step; pb.chunk_multiplier = gamma_alpha > 0 ? mult.data() : nullptr;
    if (p_error_model) {
        const int nd = (int)p_error_model->n_deviations();
        err_table.resize((size_t)S * nd);
        for (int c = 0; c < S; ++c) {
            const std::vector<double> pr = p_error_model->get_probs((size_t)c);
            std::copy(pr.begin(), pr.begin() + std::min<size_t>(pr.size(), nd), err_table.begin() + (size_t)c * nd);
        }
        pb.n_deviations = nd; pb.error_model = err_table.data();
        pb.error_model_max_size = (int32_t)p_error_model->get_max_family_size();
    }
    pb.device = device; pb.workspace_limit = workspace_limit;
    char err[512];
    const double* mus = death_rates && !death_rates->empty() ? death_rates->data() : nullptr;      // NULL: exactly cafe_simulate
    const int rc = cafe_simulate_lm(&pb, mus, seed, nullptr, sim.sizes.data(), err, sizeof err);
    if (rc != CAFE_OK) throw std::runtime_error(err);
    return sim;
}

double average_multiplier(const simulation& sim) {                     // write_average_multiplier (gamma_core.cpp:82-86)
    volatile double count = (double)sim.multipliers.size();            // the base model divides 0 by 0 at run time: -nan
    return std::accumulate(sim.multipliers.begin(), sim.multipliers.end(), 0.0) / count;
}

void print_simulations(std::ostream& ost, bool include_internal_nodes, const simulation& sim) {   // simulator.cpp:150-186
    if (sim.n_families == 0) {
        std::cerr << "No simulations created" << std::endl;
        return;
    }
    const size_t n = sim.order.size();
    std::string buf = "DESC\tFID";
    for (size_t i = 0; i < n; ++i) {
        if (sim.order[i]->is_leaf()) buf += '\t' + sim.order[i]->get_taxon_name();
        else if (include_internal_nodes) buf += '\t' + std::to_string(i);
    }
    buf += '\n';
    char num[16];
    for (size_t j = 0; j < sim.n_families; ++j) {
        buf += "NULL\tsimfam";
        buf.append(num, std::to_chars(num, num + sizeof num, j).ptr);
        const int32_t* row = sim.sizes.data() + j * n;
        for (size_t i = 0; i < n; ++i) {
            if (!include_internal_nodes && !sim.order[i]->is_leaf()) continue;
            buf += '\t';
            buf.append(num, std::to_chars(num, num + sizeof num, row[i]).ptr);
        }
        buf += '\n';
        if (buf.size() > (1u << 20)) { ost.write(buf.data(), (std::streamsize)buf.size()); buf.clear(); }
    }
    ost.write(buf.data(), (std::streamsize)buf.size());
}

}  // namespace cafe
