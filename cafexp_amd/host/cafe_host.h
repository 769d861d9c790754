// Host-side mirror of the reference's scorer/model interface above the C ABI
// (include/cafe_mi355x.h).  Same class names, argument meaning and error behaviour as the
// reference so that its optimizer (src/optimizer.cpp) and its tests read unchanged:
//   optimizer_scorer / inference_optimizer_scorer   src/optimizer_scorer.h:16-60
//   lambda_optimizer ... gamma_lambda_optimizer      src/optimizer_scorer.h:62-150
//   model::infer_family_likelihoods                  src/core.h:171
//   base_model / gamma_model                         src/base_model.h:22, src/gamma_core.h:47
//   lambda, single_lambda, multiple_lambda           src/lambda.h:21-100
//   error_model                                      src/error_model.h:29
//   root_equilibrium_distribution (float compute!)   src/root_equilibrium_distribution.h:12
// Everything is written from the behaviour described in SURVEY.md section 8; no reference code
// is reused.  The likelihood itself is never computed here: hip_base_model / hip_gamma_model
// forward to cafe_score (HIP kernels), and fail loudly when the library or a GPU is missing.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <iosfwd>
#include <deque>
#include <map>
#include <memory>
#include <random>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

struct cafe_ctx;
struct cafe_sharded;
struct cafe_params;
struct cafe_family_out;
struct cafe_sharded;

namespace cafe {

// ---------------------------------------------------------------- tree (src/clade.{h,cpp})
class clade {
public:
    clade() = default;
    clade(const std::string& name, double length) : _name(name), _length(length) {}
    ~clade();
    clade(const clade&) = delete;
    clade& operator=(const clade&) = delete;

    const clade* get_parent() const { return _parent; }
    bool is_leaf() const { return _children.empty(); }
    bool is_root() const { return _parent == nullptr; }
    double get_branch_length() const;          // throws on a lambda tree (clade.cpp:35)
    int get_lambda_index() const;              // throws on a branch-length tree (clade.cpp:43)
    std::string get_taxon_name() const { return _name; }
    const std::vector<clade*>& descendants() const { return _children; }
    void add_descendant(clade* c);
    const clade* find_descendant(const std::string& name) const;
    std::set<double> get_branch_lengths() const;                    // t > 0, root included (clade.cpp:196)
    std::map<std::string, int> get_lambda_index_map() const;        // name -> index - 1 (clade.cpp:154)
    void validate_lambda_tree(const clade* lambda_tree) const;      // clade.cpp:207
    void apply_prefix_order(const std::function<void(const clade*)>& f) const;
    void apply_reverse_level_order(const std::function<void(const clade*)>& f) const;   // children before parents
    void write_newick(std::ostream& ost, const std::function<std::string(const clade*)>& textwriter) const;   // clade.cpp:166
    std::vector<const clade*> post_order() const;                    // children before parents, root last
    std::vector<const clade*> leaves() const;

    friend clade* parse_newick(const std::string& text, bool parse_to_lambdas);

private:
    void rename_interior();                    // sorted, concatenated leaf names (clade.cpp:125)
    clade* _parent = nullptr;
    std::string _name;
    double _length = 0.0;
    int _lambda_index = 0;
    bool _is_lambda = false;
    std::vector<clade*> _children;
};
clade* parse_newick(const std::string& text, bool parse_to_lambdas = false);

// ---------------------------------------------------------------- families (src/gene_family.{h,cpp})
constexpr int kCountMissing = -1;            // CAFE_COUNT_MISSING: the cell's count is unknown and is summed out (include/cafe_mi355x.h)
class gene_family {
public:
    void set_id(const std::string& id) { _id = id; }
    void set_desc(const std::string& d) { _desc = d; }
    std::string id() const { return _id; }
    void set_species_size(const std::string& species, int count);
    int get_species_size(const std::string& species) const;          // throws when absent (gene_family.cpp:36)
    int get_max_size() const;                                        // over the observed cells (0 when none is)
    // a cell whose count is unknown (kCountMissing: `--missing`, `--mask-cells`); false for a species the family does not have
    bool is_missing(const std::string& species) const;
    size_t n_missing() const;
    std::vector<std::string> get_species() const;
    bool species_size_match(const gene_family& o) const { return _sizes == o._sizes; }
    bool exists_at_root(const clade* tree) const;                    // gene_family.cpp:60
private:
    std::string _id, _desc;
    std::map<std::string, int> _sizes;       // keys lower-cased: the reference's map compares case-insensitively
};

// ---------------------------------------------------------------- error model (src/error_model.{h,cpp})
class error_model {
public:
    error_model() : _deviations{-1, 0, 1} {}
    void set_max_family_size(size_t m) { _max_family_size = m; }
    void set_deviations(const std::vector<int>& d) { _deviations = d; }
    void set_probabilities(size_t fam_size, const std::vector<double>& probs);
    std::vector<double> get_probs(size_t fam_size) const;
    size_t n_deviations() const { return _deviations.size(); }
    size_t get_max_family_size() const { return _dists.size(); }
    std::vector<double> get_epsilons() const;
    void replace_epsilons(const std::map<double, double>& replacements);
    void update_single_epsilon(double eps);
    const std::vector<int>& deviations() const { return _deviations; }
private:
    size_t _max_family_size = 0;
    std::vector<int> _deviations;
    std::vector<std::vector<double>> _dists;
};

// ---------------------------------------------------------------- lambda holders (src/lambda.{h,cpp})
class lambda {
public:
    virtual ~lambda() {}
    virtual void update(const double* values) = 0;
    virtual int count() const = 0;
    virtual bool is_valid() const = 0;
    virtual double get_value_for_clade(const clade* c) const = 0;
    virtual lambda* multiply(double factor) const = 0;
    virtual lambda* clone() const = 0;
    virtual std::string to_string() const = 0;
    virtual std::vector<double> values() const = 0;          // get_lambda_values (matrix_cache.cpp:99)
};
class single_lambda : public lambda {
    double _lambda;
public:
    explicit single_lambda(double v) : _lambda(v) {}
    double get_single_lambda() const { return _lambda; }
    void update(const double* v) override { _lambda = *v; }
    int count() const override { return 1; }
    bool is_valid() const override { return _lambda > 0; }                     // lambda.h:58
    double get_value_for_clade(const clade*) const override { return _lambda; }
    lambda* multiply(double f) const override { return new single_lambda(_lambda * f); }
    lambda* clone() const override { return new single_lambda(_lambda); }
    std::string to_string() const override;
    std::vector<double> values() const override { return {_lambda}; }
};
class multiple_lambda : public lambda {
    std::map<std::string, int> _index;
    std::vector<double> _lambdas;
public:
    multiple_lambda(const std::map<std::string, int>& name_to_index, const std::vector<double>& v) : _index(name_to_index), _lambdas(v) {}
    void update(const double* v) override { std::copy(v, v + _lambdas.size(), _lambdas.begin()); }
    int count() const override { return (int)_lambdas.size(); }
    bool is_valid() const override;                                             // none < 0 (lambda.cpp:59)
    double get_value_for_clade(const clade* c) const override { return _lambdas[_index.at(c->get_taxon_name())]; }
    int index_of(const clade* c) const { return _index.at(c->get_taxon_name()); }
    lambda* multiply(double f) const override;
    lambda* clone() const override { return new multiple_lambda(_index, _lambdas); }
    std::string to_string() const override;
    std::vector<double> values() const override { return _lambdas; }
};

// ---------------------------------------------------------------- root priors
extern std::mt19937 randomizer_engine;                     // the reference's global engine (main.cpp:3)

class root_distribution {                                  // src/root_distribution.{h,cpp}
    std::vector<int> _v;
public:
    void vectorize(const std::map<int, int>& rootdist);
    void vectorize_uniform(int max) { _v.assign(max, 1); }
    void vectorize_increasing(int max);                    // 0, 1, .., max-1
    int max() const;
    bool empty() const { return _v.empty(); }
    int select_randomly(std::mt19937& engine = randomizer_engine) const;     // a uniformly chosen entry
    void pare(size_t new_size, std::mt19937& engine = randomizer_engine);    // shuffle, keep new_size, sort (if size >= new_size)
    void vector(const std::vector<int>& v) { _v = v; }
    size_t size() const { return _v.size(); }
    int at(size_t i) const;
    int sum() const;
};
class root_equilibrium_distribution {                      // compute() is a FLOAT in the reference
public:
    virtual ~root_equilibrium_distribution() {}
    virtual float compute(size_t val) const = 0;
    virtual void initialize(const root_distribution* rd) = 0;
};
class uniform_distribution : public root_equilibrium_distribution {
    root_distribution _rd;
    int _sum = 0;
public:
    void initialize(const root_distribution* rd) override { _rd = *rd; _sum = _rd.sum(); }
    float compute(size_t val) const override;
};
class poisson_distribution : public root_equilibrium_distribution {
    std::vector<double> _pdf;
    double _lambda;
public:
    explicit poisson_distribution(double pl) : _lambda(pl) {}
    explicit poisson_distribution(const std::vector<gene_family>* p_gene_families);     // fitted: root_equilibrium_distribution.cpp:34-45
    double poisson_lambda() const { return _lambda; }
    void initialize(const root_distribution* rd) override;
    float compute(size_t val) const override { return val >= _pdf.size() ? 0 : (float)_pdf[val]; }
};
// A root distribution given as probabilities, one per root size 1, 2, ..: what --estimate-rootdist writes and --rootdist-probs
// reads back (rootdist_arg / -f hold COUNTS, which uniform_distribution normalises in float arithmetic).  compute(j) is the
// probability of size j + 1 rounded to the float the ABI takes; sizes past the table have probability 0.
class file_probability_distribution : public root_equilibrium_distribution {
    std::vector<double> _p;
public:
    file_probability_distribution() {}
    explicit file_probability_distribution(const std::vector<double>& probabilities) : _p(probabilities) {}
    void set(const std::vector<double>& probabilities) { _p = probabilities; }
    const std::vector<double>& probabilities() const { return _p; }
    void initialize(const root_distribution*) override {}
    float compute(size_t val) const override { return val >= _p.size() ? 0 : (float)_p[val]; }
};
// "size<TAB>probability" lines, sizes 1, 2, .. in order without gaps ('#' lines skipped); throws on anything else
std::vector<double> read_rootdist_probabilities(std::istream& in);
void write_rootdist_probabilities(std::ostream& ost, const std::vector<double>& probabilities);     // 17 significant digits

// ---------------------------------------------------------------- discrete gamma (src/gamma.cpp, PAML)
double point_normal(double prob);
double incomplete_gamma(double x, double alpha, double ln_gamma_alpha);
double point_chi2(double prob, double v);
void get_gamma(std::vector<double>& cat_probs, std::vector<double>& multipliers, double alpha);

// ---------------------------------------------------------------- models (src/core.h, base_model.h, gamma_core.h)
struct family_info_stash {
    std::string family_id;
    double lambda_multiplier = 0, category_likelihood = 0, family_likelihood = 0, posterior_probability = 0;
    bool significant = false;
};
std::ostream& operator<<(std::ostream& o, const family_info_stash& r);

class event_monitor {
public:
    int attempts = 0, rejects = 0;
    std::map<std::string, int> failure_count;
    void summarize(std::ostream& ost) const;
};

class inference_optimizer_scorer;
struct user_data;
class reconstruction;

class model {
protected:
    lambda* _p_lambda;
    const clade* _p_tree;
    const std::vector<gene_family>* _p_gene_families;
    int _max_family_size, _max_root_family_size;
    error_model* _p_error_model;
    std::vector<family_info_stash> results;
    event_monitor _monitor;
    // Separate birth and death rates: one mu per lambda (index order); empty = the reference's model, lambda = mu
    std::vector<double> _death_rates;
    // What a scorer call makes of a family's root vector (cafe_set_root_rule): 0 = CAFE_ROOT_MAX, the reference's
    // max_s(L_s prior_s); 1 = CAFE_ROOT_SUM, the marginal likelihood sum_s L_s prior_s.  Held like the death rates.
    int _root_rule = 0;
public:
    void set_root_rule(int rule) { _root_rule = rule; }
    int root_rule() const { return _root_rule; }
    void set_death_rates(const std::vector<double>& mus) { _death_rates = mus; }
    const std::vector<double>& death_rates() const { return _death_rates; }
    std::string death_rates_to_string() const;                       // formatted like lambda::to_string
    model(lambda* l, const clade* tree, const std::vector<gene_family>* fams, int max_family_size, int max_root_family_size, error_model* em)
        : _p_lambda(l), _p_tree(tree), _p_gene_families(fams), _max_family_size(max_family_size), _max_root_family_size(max_root_family_size), _p_error_model(em) {}
    virtual ~model() {}
    lambda* get_lambda() const { return _p_lambda; }
    void set_lambda(lambda* l) { _p_lambda = l; }
    virtual double infer_family_likelihoods(root_equilibrium_distribution* prior, const std::map<int, int>& root_distribution_map, const lambda* p_lambda) = 0;
    virtual std::string name() const = 0;
    virtual void write_family_likelihoods(std::ostream& ost) = 0;
    virtual void write_vital_statistics(std::ostream& ost, double final_likelihood);     // core.cpp:96
    virtual inference_optimizer_scorer* get_lambda_optimizer(user_data& data) = 0;
    // core.h:177 without the matrix_cache argument (the device builds the matrices); default: not supported
    virtual reconstruction* reconstruct_ancestral_states(const std::vector<gene_family>& families, root_equilibrium_distribution* p_prior);
    const std::vector<family_info_stash>& get_results() const { return results; }
    const event_monitor& get_monitor() const { return _monitor; }
    // a parameter vector the search consumed whose score was already known (optimizer::batch): counted as the call it replaces
    void note_attempt() { _monitor.attempts++; }
    // scores made ahead of the search are not attempts of its trajectory: the monitor is put back behind them
    void restore_monitor(const event_monitor& m) { _monitor = m; }
    // Several parameter vectors in one device call (cafe_score_batch).  batch_begin: true when the model can score n_points
    // vectors at once -- the caller then sets each vector on the model through its own setters and calls batch_stage, which
    // records the model's parameters of that moment as the next point, and batch_score returns every point's
    // infer_family_likelihoods value (out[n_points]) without touching results or the monitor.  Default: cannot.
    virtual bool batch_begin(int n_points) { (void)n_points; return false; }
    virtual void batch_stage() {}
    virtual void batch_score(root_equilibrium_distribution*, const std::map<int, int>&, double*) {}
    void initialize_lambda(const clade* lambda_tree);                // core.cpp:76
    const clade* tree() const { return _p_tree; }
};

// Flattens (tree in `order` = children before parents, lambda structure, counts[n_families][leaves of `order`]) into a
// cafe_problem and creates the device context; throws std::runtime_error on failure.
cafe_ctx* create_device_context(const lambda* lam, const std::vector<const clade*>& order, const int32_t* counts, int64_t n_families,
                                 int max_family_size, int max_root_family_size, int max_categories, int n_deviations, int device,
                                 size_t workspace_limit = 0);

// cafe_marginal_reconstruct's outputs, [family][index in the caller's node order] (log_evidence, failed: [family])
struct marginal_result {
    double level = 0.95;
    size_t n_nodes = 0;
    std::vector<double> mean, p_increase, p_decrease, log_evidence;
    std::vector<int32_t> mode, lo, hi, failed;
    size_t failed_count() const { size_t k = 0; for (int32_t f : failed) k += f != 0; return k; }
};
// <Model>_posterior_sizes.tab (mean:mode:lo-hi) and <Model>_posterior_change.tab (p_decrease:p_increase, "-" at the root):
// header row, family order and node naming of <Model>_count.tab
void write_marginal_reports(const marginal_result& res, const std::string& model_identifier, const std::string& dir,
                            const std::vector<const clade*>& order, const std::vector<gene_family>& families);

// cafe_root_posterior's outputs: total[j] = sum over the families that did not fail of P(root size = j + 1 | data) (n_used of
// them; total / n_used is the EM update of the root distribution), category_posterior [family][K] under the gamma model
struct root_posterior_result {
    std::vector<double> total, mean, log_evidence, category_posterior;
    std::vector<int32_t> mode, failed;
    int64_t n_used = 0;
    size_t n_categories = 0;                                         // 0: base model
};

// cafe_expected_events' outputs, [family][index in the caller's node order] (NaN at the root and for a failed family; failed: [family])
struct events_result {
    size_t n_nodes = 0;
    std::vector<double> gains, losses;
    std::vector<int32_t> failed;
    size_t failed_count() const { size_t k = 0; for (int32_t f : failed) k += f != 0; return k; }
};
// <Model>_expected_events.tab (gains:losses per family and node, "-" at the root; header row, family order and node naming of
// <Model>_posterior_change.tab) and <Model>_branch_events.tab: per branch the expected gains, losses, net change (gains - losses)
// and turnover (gains + losses) summed in family order over the families that did not fail
void write_events_reports(const events_result& res, const std::string& model_identifier, const std::string& dir,
                          const std::vector<const clade*>& order, const std::vector<gene_family>& families);

// cafe_branch_change's summaries, [family][index in the caller's node order]: mean, mode and the equal-tailed interval at
// `level` of Delta = size(node) - size(parent) on the branch above the node, and the posterior mass beyond the band of
// +-max_change.  NaN / CAFE_CHANGE_NONE at the root and for a failed family; lo = -max_change - 1 / hi = max_change + 1: that end
// of the interval lies beyond the band (failed: [family]).  names, root: [node], what the reports print and leave out.
struct branch_change_result {
    int max_change = 10;
    double level = 0.95;
    std::vector<std::string> names;
    std::vector<char> root;
    std::vector<double> mean, below, above;
    std::vector<int32_t> mode, lo, hi, failed;
    size_t n_nodes() const { return names.size(); }
    size_t failed_count() const { size_t k = 0; for (int32_t f : failed) k += f != 0; return k; }
};
// One line of <Model>_branch_change_summary.tab: over the families that did not fail, the sum of the means, the families whose
// interval lies wholly above 0 (lo > 0) and wholly below 0 (hi < 0), and the ones with an interval end beyond the band
struct branch_change_row {
    double mean_sum = 0;
    size_t expanded = 0, contracted = 0, clipped = 0;
};
std::vector<branch_change_row> branch_change_rows(const branch_change_result& res);
// "mean:mode:[lo,hi]:p_below_band:p_above_band" of one family and node ("-" at the root and for a failed family)
std::string branch_change_cell(const branch_change_result& res, size_t family, size_t node);
// <Model>_branch_change.tab (one branch_change_cell per family and node under a header row of the nodes' names) and
// <Model>_branch_change_summary.tab (one branch_change_row per branch).  Returns the number of (family, branch) cells whose
// interval is clipped by the band: raise max_change when it is not small
size_t write_branch_change_reports(const branch_change_result& res, const std::string& model_identifier, const std::string& dir,
                                   const std::vector<std::string>& family_ids);

// cafe_leaf_predictive's outputs, [family][species] with the species in the order of `species` (NaN for a cell whose predictive
// distribution has no mass; failed: [family], judged on the family's evidence)
struct leaf_predictive_result {
    std::vector<std::string> species;
    std::vector<int> observed;                                       // [family][species]
    std::vector<double> mean, sd, p_below, p_obs, p_above;
    std::vector<int32_t> failed;
    size_t n_species() const { return species.size(); }
};
// Holm's step-down adjustment of the p-values p (any order): adjusted[i] = max over the entries at or before i in ascending
// order (ties in input order) of min(1, (n - rank) p)
inline std::vector<double> holm_adjusted(const std::vector<double>& p) {
    std::vector<size_t> idx(p.size());
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return p[a] < p[b]; });
    std::vector<double> adj(p.size());
    double run = 0;
    for (size_t r = 0; r < idx.size(); ++r) {
        run = std::max(run, std::min(1.0, (double)(idx.size() - r) * p[idx[r]]));
        adj[idx[r]] = run;
    }
    return adj;
}
// One finite cell of the table as an outlier candidate: the one-sided tails p_low = p_below + p_obs and p_high = p_obs + p_above,
// the two-sided p = min(1, 2 min(p_low, p_high)), its direction (low: p_low <= p_high) and, after leaf_outliers, Holm's adjustment
// over all finite cells of the table
struct leaf_cell {
    size_t family = 0, species = 0;
    double p_low = NAN, p_high = NAN, p = NAN, holm = NAN;
    bool low = false;
};
// every finite cell, most extreme first (Holm-adjusted p, then p, then table order)
std::vector<leaf_cell> leaf_outliers(const leaf_predictive_result& res);
// Per species: the finite cells, the mean of (x - mean) / sd over the cells with sd > 0, the outliers (holm <= threshold) low and
// high, and sum log p_obs over the cells with p_obs > 0
struct species_fit {
    size_t cells = 0, low = 0, high = 0;
    double mean_z = NAN, log_p_obs = 0;
};
std::vector<species_fit> leaf_species_fit(const leaf_predictive_result& res, const std::vector<leaf_cell>& cells, double threshold);
struct leaf_predictive_summary {
    size_t failed_cells = 0, outliers = 0;
    double log_pseudo_likelihood = 0;                                // sum log p_obs over the finite cells with p_obs > 0
};
// <Model>_leaf_predictive.tab (mean:sd:p_low:p_high per family and species, "-" for a cell without mass; family order of
// <Model>_count.tab), <Model>_leaf_outliers.tab (the cells with holm <= threshold, most extreme first: family, species, observed,
// mean, sd, direction, p, adjusted p) and <Model>_species_fit.tab (leaf_species_fit)
leaf_predictive_summary write_leaf_predictive_reports(const leaf_predictive_result& res, double threshold, const std::string& model_identifier,
                                                      const std::string& dir, const std::vector<gene_family>& families);
// One imputed cell: the model's prediction of a missing count from the family's observed species.  lo / hi: the central 95 %
// interval of the normal distribution with the predictive mean and sd, rounded outwards to whole genes and cut at 0 (the C ABI
// returns the two moments of the predictive distribution, not its quantiles)
struct imputed_cell { size_t family, species; double mean, sd; long lo, hi; };
std::vector<imputed_cell> imputed_cells(const leaf_predictive_result& res);
// <Model>_imputed_counts.tab: family, species, mean, sd, lo, hi -- one line per missing cell (observed < 0), table order.  Returns the lines
size_t write_imputed_counts(const leaf_predictive_result& res, const std::string& model_identifier, const std::string& dir,
                            const std::vector<gene_family>& families);

// cafe_sample_histories' counts, [draw][index in the caller's node order] (failed: [family])
struct history_result {
    size_t n_draws = 0, n_nodes = 0;
    uint64_t seed = 0;
    std::vector<int64_t> n_increase, n_decrease, net_change;
    std::vector<int32_t> failed;
    size_t failed_count() const { size_t k = 0; for (int32_t f : failed) k += f != 0; return k; }
};
// <Model>_sampled_change.tab: one row per node of `order`; for the number of families that expanded / contracted on the
// branch above it and the net change in genes, the mean across the draws and the equal-tailed interval at `level` on the
// draws' empirical CDF (the marginal reports' rule: lo = the least value whose CDF reaches (1 - level) / 2, hi likewise)
void write_history_reports(const history_result& res, double level, const std::string& model_identifier, const std::string& dir,
                           const std::vector<const clade*>& order);

// cafe_score_gradient's outputs in the table's family order: the per-family scores of the model's likelihood
struct gradient_result {
    size_t n_lambdas = 0, n_categories = 0;                          // n_categories: 0 for the base model
    std::vector<double> family_lnl, d_lambda, d_mu, d_multiplier;    // [family], [family][lambda] (d_mu: with death rates), [family][category]
    std::vector<int32_t> failed;
};
// Standard errors from per-family scores (standard_errors.cpp): information = sum_f s_f s_f^T over the families with finite
// scores, covariance = its inverse.  ok = false (every SE and correlation NaN) when the information matrix is singular or
// too ill-conditioned to invert.
struct standard_errors {
    std::vector<std::string> names;
    std::vector<double> estimate, se, correlation, total_score, information;     // correlation, information: [P][P]
    size_t families_used = 0, families_left_out = 0;
    bool ok = false;
};
// scores[family][parameter]
standard_errors compute_standard_errors(const std::vector<std::string>& names, const std::vector<double>& estimates,
                                        const std::vector<double>& scores, size_t n_families);
// The inverse of a symmetric positive definite matrix [n][n] by Gauss-Jordan elimination with full pivoting on its correlation
// form; false when a diagonal entry is not positive or a pivot falls below 1e-12 of the unit scale (standard_errors.cpp)
bool invert_information(const std::vector<double>& A, size_t n, std::vector<double>& inv);
// d multiplier_k / d alpha of the discrete gamma (get_gamma) by central differences with h = alpha / 100: the routine's
// quantiles are good to about 1e-6, so a smaller step would differentiate its noise
std::vector<double> multiplier_slopes(size_t n_categories, double alpha);
// <Model>_standard_errors.txt: one line per parameter (name, estimate, SE, Wald 95 % interval), the correlation matrix, the
// total score and what the errors are conditional on
void write_standard_errors(const standard_errors& se, const std::string& model_identifier, const std::string& dir, const std::string& conditional_on);

// cafe_branch_scores' total and Gram matrix over the score vector z (include/cafe_mi355x.h): n_par * n_branch branch scores
// (n_par = 2 under death rates: births, then deaths), then d_lambda [n_lambdas], d_mu [n_lambdas] (n_par = 2), d_multiplier
// [n_categories].  slot[i]: the index of the caller's node order[i] among the branch scores of one rate, -1 at the root.
struct branch_scores_result {
    size_t P = 0, n_branch = 0, n_par = 1, n_lambdas = 0, n_categories = 0;      // n_categories: 0 for the base model
    std::vector<int> slot;
    std::vector<double> total, gram;                                 // [P], [P][P]
    size_t families_used = 0, families_failed = 0;
    size_t global(size_t i) const { return n_par * n_branch + i; }   // z index of the i-th global score
};
// Rao's score test of a rate shift on every branch and clade (rate_shift_scan.cpp), from one cafe_branch_scores call at the
// fitted optimum.  For a direction a in branch-score space, with theta the searched global parameters (as directions in z),
//     U_a = a^T U - a^T G T (T^T G T)^-1 T^T U,   V_a = a^T G a - a^T G T (T^T G T)^-1 T^T G a,   T = U_a^2 / V_a,
// p = erfc(sqrt(T / 2)), and exp(U_a / V_a) the one-step estimate of the rate multiplier.  Not testable (NaN):
// V_a <= 1e-12 a^T G a.  holm: Holm's adjustment over the testable rows of the column.
struct score_test {
    bool testable = false;
    double U = NAN, V = NAN, T = NAN, p = NAN, multiplier = NAN, holm = NAN;
};
struct rate_shift_row {
    const clade* node = nullptr;
    score_test branch, subtree;          // a = the joint-rate score of the branch / of every branch at and below the node
    bool joint_testable = false;         // with death rates: the 2-df test on (birth, death) of the branch, p = exp(-T / 2)
    double joint_T = NAN, joint_p = NAN;
};
struct rate_shift_scan {
    std::vector<rate_shift_row> rows;    // the non-root nodes of the caller's order
    bool two_rates = false;
    int best = -1;                       // row with the smallest Holm-adjusted clade p, -1 when no clade is testable
    size_t families_used = 0, families_failed = 0;
    std::vector<std::string> profiled;   // names of the searched parameters
};
// theta: one direction [P] per searched parameter, named in `names`
rate_shift_scan compute_rate_shift_scan(const branch_scores_result& bs, const std::vector<const clade*>& order,
                                        const std::vector<std::vector<double>>& theta, const std::vector<std::string>& names);
// <Model>_rate_shift_scan.tab: one row per non-root node (naming of <Model>_branch_events.tab)
void write_rate_shift_scan(const rate_shift_scan& scan, const std::string& model_identifier, const std::string& dir, const std::vector<const clade*>& order);
// <Model>_rate_shift_lambda_tree.txt: the tree in -y format, the clade of row `best` labelled 2 and the rest 1
void write_rate_shift_lambda_tree(const rate_shift_scan& scan, const clade* tree, const std::string& model_identifier, const std::string& dir);

// The two models whose infer_family_likelihoods runs on the GPU through the C ABI.
class hip_model_base : public model {
protected:
    cafe_ctx* _ctx = nullptr;
    int _ctx_categories = 0;
    int _ctx_lambda_sig = -1;                                        // lambda kind/count the context was built for
    int _device = 0;
    size_t _workspace_limit = 0;
    // several GPUs: the scorer calls go to a cafe_sharded (family shards, one host thread per device, one RCCL
    // all-reduce per call); what runs once after the search (reconstruction, p-values) stays on the first device
    std::vector<int> _devices;
    cafe_sharded* _sharded = nullptr;
    int _sharded_categories = 0, _sharded_lambda_sig = -1;
    std::vector<const clade*> _order;                                // post-order used to flatten
    // (both leave the model's death rates set on what they return -- cafe_set_death_rates, NULL without any -- so every
    // call on _ctx / _sharded runs under the model's current pair)
    void ensure_context(int max_categories);                         // single-device context (_ctx)
    void ensure_scorer(int max_categories);                          // what infer_family_likelihoods calls: _sharded or _ctx
    int score_call(const cafe_params* pr, double* score);
    int family_results_call(const cafe_family_out* out);
    const char* scorer_error() const;
    // prior as floats (compute(j), j < R), error-model table, lambdas in index order
    void gather_call_inputs(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist, std::vector<float>& prior_f,
                            std::vector<double>& err_table, std::vector<double>& lambdas) const;
public:
    // Pupko reconstruction on the device: states[k][family][index in _order] (cafe_reconstruct)
    std::vector<int32_t> device_reconstruct(const std::vector<gene_family>& families, root_equilibrium_distribution* p_prior,
                                            const std::vector<double>* multipliers);
public:
    using model::model;
    ~hip_model_base() override;
    void set_device(int d) { _device = d; }
    void set_workspace_limit(size_t bytes) { _workspace_limit = bytes; }     // cafe_problem::workspace_limit of the contexts made from now on
    // G > 1: the contexts made from now on hold G times the model's categories, and batch_begin accepts up to G points
    void set_search_batch(int points) { _search_batch = points < 1 ? 1 : points; }
    bool batch_begin(int n_points) override;
    void batch_stage() override;
    void batch_score(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist, double* out) override;
    void set_devices(const std::vector<int>& d) { _devices = d; if (!d.empty()) _device = d[0]; }
    // compute_pvalues with the Monte-Carlo simulation on the device too (cafe_pvalues): statistical agreement with the
    // reference's procedure, not draw for draw
    std::vector<double> device_pvalues(int number_of_simulations, uint64_t seed);
    // Marginal reconstruction under the model's own likelihood (cafe_marginal_reconstruct): posterior mean, mode and
    // equal-tailed interval at `level` of every node's size, and the posterior probability that the branch above it
    // expanded / contracted -- with the model's lambda, prior, error model and (gamma) categories; columns in `order`
    marginal_result marginal_reconstruction(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist, double level,
                                            const std::vector<const clade*>& order);
    // Per-family scores of the model's likelihood at its current parameters (cafe_score_gradient; root_rule CAFE_ROOT_MAX is
    // what infer_family_likelihoods sums)
    gradient_result score_gradient(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist, int root_rule);
    // The total and the Gram matrix of the per-family score vectors with the scores kept per branch (cafe_branch_scores);
    // nothing per family crosses to the host.  slot in `order`
    branch_scores_result branch_scores(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist, int root_rule,
                                       const std::vector<const clade*>& order);
    // Expected number of births and of deaths on the branch above every node given the leaf counts, under the same model
    // (cafe_expected_events); columns in `order`
    events_result expected_events(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist, const std::vector<const clade*>& order);
    // The posterior of the size change on the branch above every node, in a band of +-max_change, summarised at `level`
    // (cafe_branch_change; the band itself stays on the device side of the call); columns in `order`
    branch_change_result branch_change(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist, int max_change, double level,
                                       const std::vector<const clade*>& order);
    // The posterior of every family's root size under the sum rule on the scorer's own prune, and its sum over the table
    // (cafe_root_posterior), at the model's current parameters
    root_posterior_result root_posterior(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist);
    // The leave-one-out predictive distribution of every leaf count under the same model (cafe_leaf_predictive): species in
    // the order of the table's columns on the device (the leaves of the post-order)
    leaf_predictive_result leaf_predictive(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist);
    // Whole ancestral histories drawn from the same posterior (cafe_sample_histories), counted per draw on the device:
    // how many families expanded / contracted on every branch and the net change, rows in `order`
    history_result sample_histories(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist, int n_draws, uint64_t seed,
                                    const std::vector<const clade*>& order);
protected:
    // gamma model: multipliers, category probabilities and alpha of the mixture; the base model leaves them empty
    virtual void category_parameters(std::vector<double>&, std::vector<double>&, double&) const {}
    // what infer_family_likelihoods tests before it goes to the device: false is +inf (and a reject of the monitor)
    virtual bool host_accepts() const { return _p_lambda->is_valid(); }
    int _search_batch = 1;
    // the points staged since batch_begin: flat [point][..]; accepted[point]: host_accepts at that moment
    std::vector<double> _staged_lambdas, _staged_mus, _staged_multipliers, _staged_probs, _staged_alpha;
    std::vector<char> _staged_accepted;
public:
    // compute_viterbi_sum (gene_family_reconstructor.cpp:361) for every family x node of `order` under the model's
    // plain lambda: [family][order index], NaN where the reference returns an invalid branch_probability
    std::vector<double> branch_probability_table(const reconstruction& rec, const std::vector<gene_family>& families,
                                                 const std::vector<const clade*>& order);
};
class hip_base_model : public hip_model_base {
public:
    using hip_model_base::hip_model_base;
    double infer_family_likelihoods(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist, const lambda* p_lambda) override;
    std::string name() const override { return "Base"; }
    void write_family_likelihoods(std::ostream& ost) override;
    inference_optimizer_scorer* get_lambda_optimizer(user_data& data) override;
    reconstruction* reconstruct_ancestral_states(const std::vector<gene_family>& families, root_equilibrium_distribution* p_prior) override;   // base_model.cpp:145
    // Scorer values (-lnL, +inf for a rejected vector or NaN) of the listed families of the model's table, each under its own
    // lambdas[i * count .. ): one cafe_score_per_family call.  The model's lambda gives the structure (count, lambda tree) only.
    // mus (laid out like lambdas): each family under its own (lambdas, mus), one cafe_score_per_family_lm call; the model's own
    // death rates are not read.
    std::vector<double> per_family_scores(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist,
                                          const std::vector<int64_t>& family, const std::vector<double>& lambdas,
                                          const std::vector<double>* mus = nullptr);
    // lnL (not negated; -inf and NaN as the call gives them) of the listed families under the gain model, each under its own
    // (lambdas, mus, nus) laid out like lambdas: one cafe_score_per_family_gain call under the model's root rule.  family may
    // hold kFamilyAbsent, the all-zero profile.
    std::vector<double> per_family_gain_lnl(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist,
                                            const std::vector<int64_t>& family, const std::vector<double>& lambdas,
                                            const std::vector<double>& mus, const std::vector<double>& nus, double root_absent);
    // cafe_gain_posterior at the same arguments: posterior absence, origin and loss of every listed family at every node, columns
    // in `order` (gain_origins.cpp has the reports)
    struct gain_origins gain_posterior(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist, const std::vector<int64_t>& family,
                                       const std::vector<double>& lambdas, const std::vector<double>& mus, const std::vector<double>& nus,
                                       double root_absent, const std::vector<const clade*>& order);
};
class hip_gamma_model : public hip_model_base {
    std::vector<double> _lambda_multipliers, _gamma_cat_probs;
    std::vector<std::vector<double>> _category_likelihoods;
    double _alpha;
public:
    hip_gamma_model(lambda* l, const clade* tree, const std::vector<gene_family>* fams, int max_family_size, int max_root_family_size,
                    int n_gamma_cats, double fixed_alpha, error_model* em);
    hip_gamma_model(lambda* l, const clade* tree, const std::vector<gene_family>* fams, int max_family_size, int max_root_family_size,
                    const std::vector<double>& gamma_categories, const std::vector<double>& multipliers, error_model* em);
    void set_alpha(double alpha);                                    // gamma_core.cpp:58
    double get_alpha() const { return _alpha; }
    std::vector<double> get_lambda_multipliers() const { return _lambda_multipliers; }
    bool can_infer() const;                                          // gamma_core.cpp:123
    bool host_accepts() const override { return can_infer(); }
    void category_parameters(std::vector<double>& multipliers, std::vector<double>& probs, double& alpha) const override {
        multipliers = _lambda_multipliers; probs = _gamma_cat_probs; alpha = _alpha;
    }
    double infer_family_likelihoods(root_equilibrium_distribution* prior, const std::map<int, int>& rootdist, const lambda* p_lambda) override;
    std::string name() const override { return "Gamma"; }
    void write_family_likelihoods(std::ostream& ost) override;
    void write_vital_statistics(std::ostream& ost, double final_likelihood) override;   // + "Alpha:" (gamma_core.cpp:43)
    inference_optimizer_scorer* get_lambda_optimizer(user_data& data) override;
    const std::vector<std::vector<double>>& category_likelihoods() const { return _category_likelihoods; }
    reconstruction* reconstruct_ancestral_states(const std::vector<gene_family>& families, root_equilibrium_distribution* p_prior) override;   // gamma_core.cpp:301
};

// ---------------------------------------------------------------- reconstruction reports (src/core.h:34-99,
// src/gene_family_reconstructor.cpp:167-359, base_model.cpp:181-228, gamma_core.cpp:283-299, :347-432)
typedef std::vector<const clade*> cladevector;
std::string clade_index_or_name(const clade* node, const cladevector& order);                     // clade.cpp:185

class branch_probabilities {
public:
    struct branch_probability {
        bool _is_valid;
        double _value;
        branch_probability(double value) : _is_valid(true), _value(value) {
            if (value < 0 || value > 1) throw std::runtime_error("Not a valid probability");
        }
        branch_probability() : _is_valid(false), _value(0.0) {}
    };
    bool contains(const gene_family& fam) const { return _probabilities.find(fam.id()) != _probabilities.end(); }
    branch_probability at(const gene_family& fam, const clade* c) const { return _probabilities.at(fam.id()).at(c); }
    void set(const gene_family& fam, const clade* c, branch_probability p) { _probabilities[fam.id()][c] = p; }
    static branch_probability invalid() { return branch_probability(); }
private:
    std::map<std::string, std::map<const clade*, branch_probability>> _probabilities;
};

class reconstruction {
public:
    typedef const std::vector<gene_family> familyvector;
    void print_node_change(std::ostream& ost, const cladevector& order, familyvector& gene_families, const clade* p_tree);
    void print_node_counts(std::ostream& ost, const cladevector& order, familyvector& gene_families, const clade* p_tree);
    void print_reconstructed_states(std::ostream& ost, const cladevector& order, familyvector& gene_families, const clade* p_tree, double test_pvalue,
                                    const branch_probabilities& branch_probabilities);
    // the reference walks a map keyed by node ADDRESS here, so its line order is an accident of the allocator;
    // this writer lists the same lines in `order`
    void print_increases_decreases_by_clade(std::ostream& ost, const cladevector& order, familyvector& gene_families);
    void print_increases_decreases_by_family(std::ostream& ost, const cladevector& order, familyvector& gene_families, const std::vector<double>& pvalues,
                                             double test_pvalue);
    void print_family_clade_table(std::ostream& ost, const cladevector& order, familyvector& gene_families, const clade* p_tree,
                                  const std::function<std::string(int family_index, const clade* c)>& get_family_clade_value);
    void write_results(const std::string& model_identifier, const std::string& output_prefix, const clade* p_tree, familyvector& families,
                       std::vector<double>& pvalues, double test_pvalue, const branch_probabilities& branch_probabilities);
    virtual int reconstructed_size(const gene_family& family, const clade* clade) const = 0;
    virtual ~reconstruction() {}
private:
    virtual void print_additional_data(const cladevector&, familyvector&, const std::string&) {}
    virtual int get_difference_from_parent(const gene_family* gf, const clade* c) = 0;
    virtual std::string get_reconstructed_state(const gene_family& gf, const clade* node) = 0;
    virtual void write_nexus_extensions(std::ostream&) {}
    virtual int get_node_count(const gene_family& gf, const clade* c) = 0;
};
void print_branch_probabilities(std::ostream& ost, const cladevector& order, const std::vector<gene_family>& gene_families,
                                const branch_probabilities& branch_probabilities);

class base_model_reconstruction : public reconstruction {
public:
    std::map<std::string, std::map<const clade*, int>> _reconstructions;
    int reconstructed_size(const gene_family& family, const clade* clade) const override;
private:
    std::string get_reconstructed_state(const gene_family& gf, const clade* node) override;
    int get_difference_from_parent(const gene_family* gf, const clade* c) override;
    int get_node_count(const gene_family& gf, const clade* c) override;
};

class gamma_model_reconstruction : public reconstruction {
    const std::vector<double> _lambda_multipliers;
    void write_nexus_extensions(std::ostream& ost) override;
    void print_additional_data(const cladevector& order, familyvector& gene_families, const std::string& output_prefix) override;
    std::string get_reconstructed_state(const gene_family& gf, const clade* node) override;
    int get_difference_from_parent(const gene_family* gf, const clade* c) override;
    int get_node_count(const gene_family& gf, const clade* c) override;
public:
    explicit gamma_model_reconstruction(const std::vector<double>& lambda_multipliers) : _lambda_multipliers(lambda_multipliers) {}
    void print_category_likelihoods(std::ostream& ost, const cladevector& order, familyvector& gene_families);
    int reconstructed_size(const gene_family& family, const clade* clade) const override;
    struct gamma_reconstruction {
        std::vector<std::map<const clade*, int>> category_reconstruction;
        std::map<const clade*, double> reconstruction;
        std::vector<double> _category_likelihoods;
    };
    std::map<std::string, gamma_reconstruction> _reconstructions;
};
// get_weighted_averages, gamma_core.cpp:283-299
std::map<const clade*, double> get_weighted_averages(const std::vector<std::map<const clade*, int>>& m, const std::vector<double>& probabilities);
// execute.cpp:163-176: Viterbi branch probabilities for the families with pvalue < test_pvalue
branch_probabilities compute_branch_probabilities(hip_model_base& mdl, const reconstruction& rec, const std::vector<gene_family>& families,
                                                  const std::vector<double>& pvalues, double test_pvalue, const cladevector& order);

// ---------------------------------------------------------------- scorers (src/optimizer_scorer.{h,cpp})
extern std::mt19937 randomizer_engine;

class optimizer_scorer {
public:
    virtual ~optimizer_scorer() {}
    virtual std::vector<double> initial_guesses() = 0;
    virtual double calculate_score(const double* values) = 0;
    // The scores of n_points vectors of n_values each (values[point][value]) -> out[point].  The default scores them one by one;
    // a scorer whose model can score several vectors in one device call (cafe_score_batch) may override it.  What it leaves in
    // the model is unspecified: optimizer::optimize prepares the point it consumes again.
    virtual void calculate_scores(const double* values, int n_points, int n_values, double* out) {
        for (int i = 0; i < n_points; ++i) out[i] = calculate_score(values + (size_t)i * n_values);
    }
};
// empirical Poisson prior: -lnL of the leaf sizes shifted by one (src/poisson.cpp:38-77)
class poisson_scorer : public optimizer_scorer {
    std::vector<int> leaf_family_sizes;
public:
    explicit poisson_scorer(const std::vector<gene_family>& gene_families);
    std::vector<double> initial_guesses() override;
    double calculate_score(const double* values) override { return lnLPoisson(values); }
    double lnLPoisson(const double* plambda);
};
class inference_optimizer_scorer : public optimizer_scorer {
protected:
    lambda* _p_lambda;
    model* _p_model;
    root_equilibrium_distribution* _p_distribution;
    const std::map<int, int>& _rootdist_map;
public:
    virtual void prepare_calculation(const double* values) = 0;
    virtual void report_precalculation() = 0;
    inference_optimizer_scorer(lambda* l, model* m, root_equilibrium_distribution* d, const std::map<int, int>& rootdist)
        : _p_lambda(l), _p_model(m), _p_distribution(d), _rootdist_map(rootdist) {}
    double calculate_score(const double* values) override;           // NaN -> +inf (optimizer_scorer.cpp:30)
    // one device call where the model can (model::batch_begin) and this scorer's vector is all a point needs (batchable):
    // every vector goes through prepare_calculation, the model stages itself; else the loop.  Either way the model's monitor is
    // left as it was: what the search consumes is counted when it is consumed (consumed_cached, or calculate_score for a reject)
    void calculate_scores(const double* values, int n_points, int n_values, double* out) override;
    virtual bool batchable() const { return true; }
    // optimizer::batch consumed a vector whose finite score it already had: prepare_calculation and report_precalculation ran
    void consumed_cached() { _p_model->note_attempt(); }
    virtual void finalize(double* result) = 0;
    bool quiet = true;
};
class lambda_optimizer : public inference_optimizer_scorer {
    double _longest_branch;
public:
    lambda_optimizer(lambda* l, model* m, root_equilibrium_distribution* d, double longest_branch, const std::map<int, int>& rootdist)
        : inference_optimizer_scorer(l, m, d, rootdist), _longest_branch(longest_branch) {}
    std::vector<double> initial_guesses() override;
    void prepare_calculation(const double* values) override { _p_lambda->update(values); }
    void report_precalculation() override;
    void finalize(double* results) override { _p_lambda->update(results); }
};
class lambda_epsilon_optimizer : public inference_optimizer_scorer {
    lambda_optimizer _lambda_optimizer;
    error_model* _p_error_model;
    std::vector<double> current_guesses;
public:
    lambda_epsilon_optimizer(model* m, error_model* em, root_equilibrium_distribution* d, const std::map<int, int>& rootdist, lambda* l, double longest_branch)
        : inference_optimizer_scorer(l, m, d, rootdist), _lambda_optimizer(l, m, d, longest_branch, rootdist), _p_error_model(em) {}
    std::vector<double> initial_guesses() override;
    void prepare_calculation(const double* values) override;
    void report_precalculation() override;
    void finalize(double* results) override;
    bool batchable() const override { return false; }                // one error table per point: a batch shares one
};
class gamma_optimizer : public inference_optimizer_scorer {
    hip_gamma_model* _p_gamma_model;
public:
    gamma_optimizer(hip_gamma_model* m, root_equilibrium_distribution* d, const std::map<int, int>& rootdist)
        : inference_optimizer_scorer(m->get_lambda(), m, d, rootdist), _p_gamma_model(m) {}
    std::vector<double> initial_guesses() override;
    void prepare_calculation(const double* values) override { _p_gamma_model->set_alpha(*values); }
    void report_precalculation() override;
    void finalize(double* result) override { _p_gamma_model->set_alpha(*result); }
    double get_alpha() const { return _p_gamma_model->get_alpha(); }
};
class gamma_lambda_optimizer : public inference_optimizer_scorer {
    lambda_optimizer _lambda_optimizer;
    gamma_optimizer _gamma_optimizer;
public:
    gamma_lambda_optimizer(lambda* l, hip_gamma_model* m, root_equilibrium_distribution* d, const std::map<int, int>& rootdist, double longest_branch)
        : inference_optimizer_scorer(l, m, d, rootdist), _lambda_optimizer(l, m, d, longest_branch, rootdist), _gamma_optimizer(m, d, rootdist) {}
    std::vector<double> initial_guesses() override;
    void prepare_calculation(const double* values) override;
    void report_precalculation() override;
    void finalize(double* results) override;
};
// Death rates searched with whatever `inner` searches: the vector is inner's followed by one mu per lambda ([lambda..., mu...]
// for the base model).  mu starts at the lambda guess (the nested model's point); a negative mu scores +inf like a negative
// lambda (the library's rule, cafe_set_death_rates).  `inner` must lead with the lambdas (every scorer above but gamma_optimizer).
class lambda_mu_optimizer : public inference_optimizer_scorer {
    std::unique_ptr<inference_optimizer_scorer> _inner;
    size_t _n_inner = 0;
    void apply(const double* values) { _p_model->set_death_rates(std::vector<double>(values + _n_inner, values + _n_inner + _p_lambda->count())); }
public:
    lambda_mu_optimizer(inference_optimizer_scorer* inner, lambda* l, model* m, root_equilibrium_distribution* d, const std::map<int, int>& rootdist)
        : inference_optimizer_scorer(l, m, d, rootdist), _inner(inner) {}
    std::vector<double> initial_guesses() override;
    void prepare_calculation(const double* values) override { _inner->prepare_calculation(values); apply(values); }
    void report_precalculation() override;
    void finalize(double* results) override { _inner->finalize(results); apply(results); }
    bool batchable() const override { return _inner->batchable(); }
};

// ---------------------------------------------------------------- inputs (src/io.cpp, src/user_data.cpp)
struct user_data {
    int max_family_size = -1, max_root_family_size = -1;
    std::unique_ptr<clade> p_tree, p_lambda_tree;
    std::unique_ptr<lambda> p_lambda;
    std::unique_ptr<error_model> p_error_model;
    std::unique_ptr<root_equilibrium_distribution> p_prior;
    std::vector<gene_family> gene_families;
    std::map<int, int> rootdist;
};
// missing_tokens (or nullptr: none): a cell spelled like one of them, blanks around it ignored, becomes kCountMissing; every
// other cell goes through atoi as in the reference (io.cpp:134), where "NA" reads as 0
void read_gene_families(std::istream& in, const clade* tree, std::vector<gene_family>& out, const std::set<std::string>* missing_tokens = nullptr);
// "NA,?,-" -> {"NA", "?", "-"} (empty entries dropped)
std::set<std::string> parse_missing_tokens(const std::string& list);
// Lines `family<TAB>species[<TAB>anything]` (a line that starts with '#' and empty lines are skipped; the first two columns of
// <Model>_leaf_outliers.tab are such a file): every family with that id gets kCountMissing for that species.  Throws on an id
// or a species the table does not have.  Returns the number of cells newly marked.
size_t mask_cells(std::istream& in, std::vector<gene_family>& fams);
struct missing_summary { size_t cells = 0, families = 0; };
missing_summary count_missing(const std::vector<gene_family>& fams);
void read_error_model_file(std::istream& in, error_model* em);                                  // io.cpp:226
void write_error_model_file(std::ostream& ost, const error_model& em);                          // io.cpp:275
void read_rootdist(std::istream& in, std::map<int, int>& out);                                  // user_data.cpp:103
void compute_max_sizes(const std::vector<gene_family>& fams, int& max_family_size, int& max_root_family_size);   // user_data.cpp:37-46

// ---------------------------------------------------------------- p-values (src/probability.cpp:255-454)
// The Monte-Carlo part follows the reference draw for draw on the global randomizer_engine (same libstdc++
// distributions, same traversal), so a run at the same seed sees the same simulated families; both prune batches
// (root sizes x simulations, and the observed families) run on the GPU through cafe_root_max.
struct pvalue_work {
    std::vector<std::vector<double>> conditional_distribution;     // [root size][simulation], sorted
    std::vector<double> observed_max_likelihood;                   // per family
};
double pvalue(double v, const std::vector<double>& conddist);                                        // probability.cpp:379
std::vector<double> compute_pvalues(const clade* p_tree, const std::vector<gene_family>& families, const lambda* p_lambda,
                                    int number_of_simulations, int max_family_size, int max_root_family_size, int device = 0,
                                    pvalue_work* keep = nullptr,                                      // probability.cpp:418
                                    const std::vector<double>* death_rates = nullptr);               // one mu per lambda: both prunes and the draws under the pair

// ---------------------------------------------------------------- simulation (the reference's -s; src/simulator.cpp)
const size_t LAMBDA_PERTURBATION_STEP_SIZE = 50;                    // families per simulation lambda (configure.ac default)
struct simulation {
    std::vector<const clade*> order;       // reverse level order: the writers' columns
    size_t n_families = 0;
    int max_family_size = 0;               // S: 100, or 2 * the root distribution's maximum
    std::vector<int32_t> sizes;            // [family][index in order]
    std::vector<double> multipliers;       // the gamma model's multiplier per chunk (empty for the base model)
};
// simulate_processes draw for draw on randomizer_engine; gamma_alpha > 0: the gamma model (one Gamma(alpha, 1/alpha)
// multiplier per chunk).  rootdist empty: nsims families with root sizes 0..99; else the vectorized distribution, pared to
// nsims when 0 < nsims <= its size.  Matrices from cafe_build_matrices on `device`.  death_rates (one mu per lambda, or
// null / empty: lambda = mu): the same draws on the rows of cafe_build_matrices_lm; a chunk's multiplier scales both rates.
simulation simulate_families(const clade* p_tree, const lambda* p_lambda, const error_model* p_error_model, const std::map<int, int>& rootdist,
                             int nsims, double gamma_alpha, int device, const std::vector<double>* death_rates = nullptr);
// the same families' distribution from cafe_simulate (cafe_simulate_lm with death rates): root sizes and multipliers from an
// engine seeded by `seed`
simulation simulate_families_device(const clade* p_tree, const lambda* p_lambda, const error_model* p_error_model, const std::map<int, int>& rootdist,
                                    int nsims, double gamma_alpha, int device, uint64_t seed, size_t workspace_limit = 0,
                                    const std::vector<double>* death_rates = nullptr);
double average_multiplier(const simulation& sim);                   // write_average_multiplier's value (NaN without draws)
// simulator::print_simulations (simulator.cpp:150-186): leaves only, or every node (interior ones by order index)
void print_simulations(std::ostream& ost, bool include_internal_nodes, const simulation& sim);

// ---------------------------------------------------------------- Nelder-Mead driver (src/optimizer.cpp)
struct optimizer_result {
    std::vector<double> values;
    double score = 0;
    int num_iterations = 0;
    int num_scorer_calls = 0;                    // points the search consumed (and the draws for a start)
    int num_batches = 0;                         // optimizer::batch > 1: calculate_scores calls
    int num_points_scored = 0;                   // ... and the points they and the re-scored rejects evaluated
};
// One Nelder-Mead search as a state machine (the moves and stop rules of optimizer::optimize, which drives one of these):
// trial() is the point whose score is needed next, feed() takes it.  A caller with many independent searches can gather
// their trials, score them together and feed each its own (lambda_per_family.cpp).
struct nm_settings {
    int max_iterations = 300;
    double tolx = 1e-6, tolf = 1e-6;
    int similarity_window = 12;
    double similarity_precision = 1e-3;
    double delta = 0.05;                         // the first simplex: vertex i is x0 with coordinate i-1 times (1 + delta)
};
class nm_search {
public:
    struct vertex { std::vector<double> x; double f = 0; };
    nm_search(const nm_settings& s, const std::vector<double>& x0);      // the first trial is x0 itself
    bool done() const { return _phase == DONE; }
    const std::vector<double>& trial() const { return _trial == kTrialReflected ? _xr : _trial == kTrialOther ? _xt : _simplex[_trial].x; }
    void feed(double score);
    const std::vector<double>& best() const { return _simplex[0].x; }
    double best_score() const { return _simplex[0].f; }
    int iterations() const { return _it; }
    int calls() const { return _calls; }
    int shrinks() const { return _shrinks; }
    // The points, other than trial(), whose score the search may ask for before it next sorts the simplex, in the order it
    // would ask: in the first simplex the remaining vertices (built with the unwidened delta: a vertex that follows an infinite
    // one is widened, and then is not the one listed here); before the reflected point's score the expansion, the outside and
    // the inside contraction; in a shrink the remaining shrunk vertices; otherwise none.  Each is computed by the expression
    // feed() uses, so that it has the bits of the later trial.
    void lookahead(std::vector<std::vector<double>>& points) const;
private:
    enum phase { INIT, REFLECT, EXPAND, CONTRACT_IN, CONTRACT_OUT, SHRINK, DONE };
    nm_settings _s;
    std::vector<double> _x0;
    int _n;
    std::vector<vertex> _simplex;
    std::vector<double> _mean, _xr, _xt;
    std::deque<double> _recent;
    static constexpr int kTrialReflected = -1, kTrialOther = -2;
    int _trial = 0;                              // the vertex whose point is the trial, or one of the two above
    phase _phase = INIT;
    int _i = 0, _it = 0, _calls = 0, _shrinks = 0;
    double _fr = 0;
    void begin_iteration();
    void end_iteration();
    void accept(const std::vector<double>& x, double f);
    void start_shrink();
};

class optimizer {
    optimizer_scorer* _scorer;
public:
    explicit optimizer(optimizer_scorer* s) : _scorer(s) {}
    int max_iterations = 300;                   // optimizer.h:28
    double tolx = 1e-6, tolf = 1e-6;            // OPTIMIZER_HIGH_PRECISION
    int similarity_window = 12;                 // OPTIMIZER_SIMILARITY_CUTOFF_SIZE, 0 = off
    double similarity_precision = 1e-3;         // OPTIMIZER_LOW_PRECISION
    std::vector<double> start;                  // not empty: the search starts here (no draws), e.g. from an earlier optimum
    // > 1: the same search, but a point whose score is not known yet goes to the scorer together with the points the search may
    // ask for next (nm_search::lookahead), at most `batch` in one calculate_scores call, and every score is kept for the rest of
    // this optimize() call under the exact bits of its vector.  The trajectory, the result and what the scorer prints are the
    // sequential search's; only the number of dependent scorer round trips falls (optimizer_result::num_batches).
    int batch = 1;
    typedef std::vector<std::pair<std::vector<double>, double>> scored_points;
    // <= 100 retries while +inf (optimizer.cpp:345); drawn: every (draw, score) it made, in order
    std::vector<double> get_initial_guesses(int& calls, scored_points* drawn = nullptr);
    // fed (batch > 1 only): called with every (point, score) as the search is fed it
    typedef std::function<void(const std::vector<double>&, double)> feed_observer;
    optimizer_result optimize(const feed_observer& fed = nullptr);
private:
    optimizer_result optimize_batched(const feed_observer& fed);
};

// ---------------------------------------------------------------- lambda per family (-b; src/execute.cpp:104-128)
// estimator::estimate_lambda_per_family as ONE lock-step search: every distinct family runs its own Nelder-Mead
// (nm_search: the reference's moves and stop rules), and per round the next trial of every unfinished family goes to the
// device in one cafe_score_per_family call.  Starts are lambda_optimizer::initial_guesses draws from randomizer_engine,
// one sequence per distinct family in order of first appearance, redrawn (<= 100 times) while the score is infinite.
// A finished search is begun again from its best point (inward first simplex, high-precision stop rule) while the last one
// still gained (lambda_per_family.cpp).
// M, R and the prior are the whole table's, as in the reference (set_families only swaps the family list).
// Separate death rates per family (--family-mu): FIXED searches every family's lambdas with mu held at the given rates (one
// per lambda); ESTIMATE searches [lambdas..., mus...] per family from the family's lambda-only optimum, every mu starting at
// its lambda, so that the result is never worse than plain -b's (lambda_per_family.cpp).  Either scores through
// cafe_score_per_family_lm.
struct per_family_mu {
    enum { NONE, FIXED, ESTIMATE } mode = NONE;
    std::vector<double> fixed;                   // FIXED: one per lambda
};
struct per_family_result {
    std::vector<std::vector<double>> lambdas;    // per family, table order
    std::vector<std::vector<double>> mus;        // per family with per_family_mu (empty without)
    size_t distinct_families = 0;
    int rounds = 0;                              // device calls
    long evaluations = 0;                        // (family, lambda vector) pairs scored
    long restarts = 0;                           // searches begun again from a family's best point
};
per_family_result estimate_lambda_per_family(hip_base_model& mdl, user_data& data, int max_iterations, const per_family_mu& family_mu = per_family_mu());
// what the reference prints when no start has a finite score (execute.cpp:192-206)
void initialization_failure_advice(std::ostream& ost, const std::vector<gene_family>& families);

// ---------------------------------------------------------------- gene gain rate (--gain / --estimate-gain; gain_model.cpp)
// One set of rates for the whole table under the birth-death process with a gain rate nu (cafe_score_per_family_gain), fitted to
// the likelihood CONDITIONAL on a family having been seen in at least one species, under the sum rule.
constexpr int64_t kFamilyAbsent = -1;           // CAFE_FAMILY_ABSENT
struct gain_options {
    bool estimate_nu = false;                    // --estimate-gain; else nu = fixed_nu (--gain NU)
    double fixed_nu = 0;
    double root_absent = 0;                      // --root-absent
    bool conditional = true;                     // false: --gain-unconditional
    bool estimate_mu = false;                    // --estimate-mu: mus searched, start mu = lambda
    std::vector<double> fixed_lambdas, fixed_mus;       // -l / -m and --mu (empty: searched / mu = lambda)
    int max_iterations = 300;
};
// every distinct family once (its first index in the table) with its multiplicity, then kFamilyAbsent with weight 0
struct gain_table {
    std::vector<int64_t> family;
    std::vector<double> weight;
    double n_families = 0;
};
gain_table gain_distinct_families(const std::vector<gene_family>& families);
// The search vector: [lambdas (unless fixed)..., mus (if searched)..., nu (if with_nu)]
struct gain_layout {
    int L = 1;
    bool lambdas_free = true, mus_free = false, nu_free = false;
    std::vector<double> fixed_lambdas, fixed_mus;
    double fixed_nu = 0;
    int width() const { return (lambdas_free ? L : 0) + (mus_free ? L : 0) + (nu_free ? 1 : 0); }
    // the rates of point x; false when a rate is out of range (lambda or mu negative, one lambda not positive, nu negative, NaN)
    bool unpack(const double* x, std::vector<double>& lambdas, std::vector<double>& mus, double& nu) const;
    std::vector<double> pack(const std::vector<double>& lambdas, const std::vector<double>& mus, double nu) const;
};
// -sum_f w_f lnL_f (+ F log(1 - exp(lnL_absent)) if conditional); lnl: one per entry of the table, the absent profile last.
// +inf when a weighted family is impossible, a value is NaN, or (conditional) the model never shows a family (lnL_absent >= 0).
double gain_objective(const std::vector<double>& lnl, const gain_table& table, bool conditional);
// lnL of every entry of the table under shared (lambdas, mus, nu): the device call, or a mock
typedef std::function<std::vector<double>(const std::vector<double>& lambdas, const std::vector<double>& mus, double nu)> gain_scorer;
struct gain_fit {
    std::vector<double> lambdas, mus;
    double nu = 0, neg_lnl = 0, p_absent = 0;
    std::vector<double> lnl;                     // per entry of the table at the optimum
    std::vector<double> start;                   // the search vector the search began at (empty: nothing was searched)
    int calls = 0;
};
struct gain_result {
    gain_fit without, with;                      // the nu = 0 fit, and the fit it was extended to
    double lr_statistic = 0;                     // 2 (neg_lnl(without) - neg_lnl(with))
};
// The nested search: first without nu (nothing to search: one evaluation), then with nu -- searched from nu = lambda / 10 or held
// at fixed_nu -- from that optimum.  A gain fit that ends above the nu = 0 fit is replaced by it.  draw_lambdas: a start for the
// lambdas of the first search.
gain_result fit_gain_model(const gain_scorer& score, const gain_table& table, int n_lambdas, const gain_options& opt,
                           const std::function<std::vector<double>()>& draw_lambdas);
// Why the gain options cannot be combined with what else was asked for, or nullptr
struct gain_request {
    bool gain = false, estimate_gain = false, root_absent_given = false, unconditional = false, posterior = false;
    double nu = 0, root_absent = 0;
    bool gamma = false, per_family = false, gpus = false, simulate = false, pvalues = false, reconstruct = false, marginal = false, histories = false,
         standard_errors = false, events = false, rate_shift = false, leaf_predictive = false, branch_change = false, rootdist_em = false,
         search_batch = false, estimate_error = false;
};
const char* gain_refusal(const gain_request& r);
void write_gain_results(std::ostream& ost, const gain_result& res, const gain_options& opt, const gain_table& table);

// ---------------------------------------------------------------- --gain-posterior (gain_origins.cpp): where a family originated and was lost
// cafe_gain_posterior at the fitted rates over the entries of a gain_table (every distinct family once, the absent profile last)
struct gain_origins {
    size_t n_nodes = 0;                          // columns, in the reports' node order
    std::vector<double> lnl;                     // [entries]; an entry without a finite lnl has failed and NaN everywhere else
    std::vector<double> p_absent, mean, p_gain, p_loss;       // [entries][n_nodes]; p_gain and p_loss are NaN at the root
};
// Sums over the table's families: entry e counts weight[e] times (the absent profile: 0), a failed entry not at all
struct gain_branch_origins {
    std::vector<double> originated, lost, present;            // [n_nodes] sum p_gain, sum p_loss, sum (1 - p_absent); 0 / 0 / sum at the root
    std::vector<double> likely_origin;           // [n_nodes] the number of families with p_gain > 0.5 on the branch above the node
    double absent_at_root = 0;                   // sum p_absent of the root
    double used = 0, failed = 0;                 // families summed, and families whose entry failed
    double origin_somewhere = 0;                 // families with p_gain > 0.5 on some branch
};
gain_branch_origins gain_origin_totals(const gain_origins& o, const std::vector<double>& weight, size_t root);
// Gain_origins.tab: a header row, then one line per family of the table -- for every node p_absent:mean, then for every branch
// (every node but the root, same order) p_gain:p_loss.  entry_of[i]: the entry of family i.
void write_gain_origins(std::ostream& ost, const gain_origins& o, const std::vector<std::string>& node_names, size_t root,
                        const std::vector<std::string>& family_ids, const std::vector<size_t>& entry_of);
// Gain_branch_origins.tab: one line per branch -- originated, lost, present, the families with p_gain > 0.5 -- and a root line
void write_gain_branch_origins(std::ostream& ost, const gain_branch_origins& t, const std::vector<std::string>& node_names, size_t root);

}  // namespace cafe
