// Nelder-Mead driver for the scorers.  Same moves and constants as the reference's
// fminsearch (src/optimizer.cpp:60-320: rho 1, chi 2, psi 0.5, sigma 0.5, delta 0.05, zero_delta
// 0.00025) and its default stop rule (NelderMeadSimilarityCutoff, optimizer.cpp:391-419: tolx/tolf
// 1e-6, or the best score moving < 1e-3 over 12 iterations).  Initial guesses are RNG-driven, so
// trajectories differ from the reference; optima are compared, not paths.
#include "cafe_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <map>

namespace cafe {

std::vector<double> optimizer::get_initial_guesses(int& calls, scored_points* drawn) {
    if (!start.empty()) return start;                             // (the search scores it as its first trial)
    std::vector<double> initial = _scorer->initial_guesses();
    double first = _scorer->calculate_score(initial.data());
    ++calls;
    if (drawn) drawn->push_back({initial, first});
    for (int i = 0; std::isinf(first) && i < 100; ++i) {          // NUM_OPTIMIZER_INITIALIZATION_ATTEMPTS
        initial = _scorer->initial_guesses();
        first = _scorer->calculate_score(initial.data());
        ++calls;
        if (drawn) drawn->push_back({initial, first});
    }
    if (std::isinf(first)) throw std::runtime_error("Failed to initialize any reasonable values");
    return initial;
}

// ---- the moves, as a state machine: trial() is the point whose score the search needs next, feed() takes that score.
// The scalar optimizer below and the lock-step search over many families (lambda_per_family.cpp) both drive it.
namespace {
const double rho = 1, chi = 2, psi = 0.5, sigma = 0.5, zero_delta = 0.00025;
bool by_score(const nm_search::vertex& a, const nm_search::vertex& b) { return a.f < b.f; }
}  // namespace

nm_search::nm_search(const nm_settings& s, const std::vector<double>& x0) : _s(s), _x0(x0), _n((int)x0.size()), _simplex(x0.size() + 1), _mean(x0.size()), _xr(x0.size()), _xt(x0.size()) {
    _phase = INIT;                                                   // __fminsearch_min_init
    _i = 0;
    _simplex[0].x = _x0;
    _trial = 0;
}

void nm_search::accept(const std::vector<double>& x, double f) {
    _simplex[_n].x = x;
    _simplex[_n].f = f;
    end_iteration();
}

void nm_search::end_iteration() {
    std::sort(_simplex.begin(), _simplex.end(), by_score);
    ++_it;
    begin_iteration();
}

void nm_search::begin_iteration() {
    const int n = _n;
    if (_it >= _s.max_iterations) { _phase = DONE; return; }
    double dx = 0, df = 0;                                           // threshold_achieved: checkV && checkF
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) dx = std::max(dx, std::fabs(_simplex[i + 1].x[j] - _simplex[i].x[j]));
    for (int i = 1; i <= n; ++i) df = std::max(df, std::fabs(_simplex[i].f - _simplex[0].f));
    if (dx <= _s.tolx && df <= _s.tolf) { _phase = DONE; return; }
    if (_s.similarity_window > 0) {
        _recent.push_back(_simplex[0].f);
        if ((int)_recent.size() > _s.similarity_window) _recent.pop_front();
        if ((int)_recent.size() == _s.similarity_window) {
            const auto mm = std::minmax_element(_recent.begin(), _recent.end());
            if (*mm.second - *mm.first < _s.similarity_precision) { _phase = DONE; return; }
        }
    }
    for (int j = 0; j < n; ++j) {
        _mean[j] = 0;
        for (int i = 0; i < n; ++i) _mean[j] += _simplex[i].x[j];
        _mean[j] /= n;
    }
    const vertex& worst = _simplex[n];
    for (int j = 0; j < n; ++j) _xr[j] = _mean[j] + rho * (_mean[j] - worst.x[j]);
    _phase = REFLECT;
    _trial = kTrialReflected;
}

void nm_search::start_shrink() {
    ++_shrinks;
    _phase = SHRINK;
    _i = 1;
    for (int j = 0; j < _n; ++j) _simplex[1].x[j] = _simplex[0].x[j] + sigma * (_simplex[1].x[j] - _simplex[0].x[j]);
    _trial = 1;
}

void nm_search::feed(double f) {
    const int n = _n;
    ++_calls;
    vertex& worst = _simplex[n];
    switch (_phase) {
    case INIT:
        _simplex[_i].f = f;
        if (++_i <= n) {
            const int i = _i, j = i - 1;
            const bool widen = i > 1 && std::isinf(_simplex[i - 1].f);
            _simplex[i].x = _x0;
            _simplex[i].x[j] = _x0[j] ? (1 + (widen ? _s.delta * 100 : _s.delta)) * _x0[j] : zero_delta;
            _trial = i;
        } else {
            std::sort(_simplex.begin(), _simplex.end(), by_score);
            begin_iteration();
        }
        break;
    case REFLECT:
        _fr = f;
        if (_fr < _simplex[0].f) {
            for (int j = 0; j < n; ++j) _xt[j] = _mean[j] + chi * (_xr[j] - _mean[j]);
            _phase = EXPAND; _trial = kTrialOther;
        } else if (_fr >= worst.f) {
            if (_fr > worst.f) {
                for (int j = 0; j < n; ++j) _xt[j] = _mean[j] + psi * (_mean[j] - worst.x[j]);     // contract inside
                _phase = CONTRACT_IN;
            } else {
                for (int j = 0; j < n; ++j) _xt[j] = _mean[j] + psi * (_xr[j] - _mean[j]);         // contract outside
                _phase = CONTRACT_OUT;
            }
            _trial = kTrialOther;
        } else {
            accept(_xr, _fr);
        }
        break;
    case EXPAND:
        if (f < _fr) accept(_xt, f); else accept(_xr, _fr);
        break;
    case CONTRACT_IN:
        if (f < worst.f) accept(_xt, f); else start_shrink();
        break;
    case CONTRACT_OUT:
        if (f <= _fr) accept(_xt, f); else start_shrink();
        break;
    case SHRINK:
        _simplex[_i].f = f;
        if (++_i <= n) {
            for (int j = 0; j < n; ++j) _simplex[_i].x[j] = _simplex[0].x[j] + sigma * (_simplex[_i].x[j] - _simplex[0].x[j]);
            _trial = _i;
        } else {
            end_iteration();
        }
        break;
    case DONE:
        break;
    }
}

void nm_search::lookahead(std::vector<std::vector<double>>& points) const {
    points.clear();
    const int n = _n;
    std::vector<double> x(n);
    switch (_phase) {
    case INIT:
        for (int i = _i + 1; i <= n; ++i) {
            const int j = i - 1;
            x = _x0;
            x[j] = _x0[j] ? (1 + _s.delta) * _x0[j] : zero_delta;
            points.push_back(x);
        }
        break;
    case REFLECT: {
        const vertex& worst = _simplex[n];
        for (int j = 0; j < n; ++j) x[j] = _mean[j] + chi * (_xr[j] - _mean[j]);
        points.push_back(x);
        for (int j = 0; j < n; ++j) x[j] = _mean[j] + psi * (_xr[j] - _mean[j]);
        points.push_back(x);
        for (int j = 0; j < n; ++j) x[j] = _mean[j] + psi * (_mean[j] - worst.x[j]);
        points.push_back(x);
        break;
    }
    case SHRINK:
        for (int i = _i + 1; i <= n; ++i) {
            for (int j = 0; j < n; ++j) x[j] = _simplex[0].x[j] + sigma * (_simplex[i].x[j] - _simplex[0].x[j]);
            points.push_back(x);
        }
        break;
    default:
        break;
    }
}

namespace {
typedef std::vector<uint64_t> point_key;                             // the exact bits of a parameter vector
point_key key_of(const std::vector<double>& x) {
    point_key k(x.size());
    if (!x.empty()) std::memcpy(k.data(), x.data(), sizeof(double) * x.size());
    return k;
}
}  // namespace

// optimize() with batch > 1.  The score cache lives for this call only: what a vector scores depends on state the caller may
// change between searches (the prior, between the rounds of a root-distribution estimate).
optimizer_result optimizer::optimize_batched(const feed_observer& fed) {
    optimizer_result res;
    std::map<point_key, double> cache;
    auto* inference = dynamic_cast<inference_optimizer_scorer*>(_scorer);
    scored_points drawn;                     // the draws for a start seed the cache
    const std::vector<double> x0 = get_initial_guesses(res.num_scorer_calls, &drawn);
    res.num_points_scored += (int)drawn.size();
    for (const auto& d : drawn) cache[key_of(d.first)] = d.second;
    nm_settings s;
    s.max_iterations = max_iterations; s.tolx = tolx; s.tolf = tolf;
    s.similarity_window = similarity_window; s.similarity_precision = similarity_precision;
    nm_search search(s, x0);
    const int n = (int)x0.size();
    std::vector<std::vector<double>> ahead;
    std::vector<double> flat, scores;
    while (!search.done()) {
        const std::vector<double> x = search.trial();
        auto hit = cache.find(key_of(x));
        if (hit == cache.end()) {            // the trial and what may follow it, not yet scored, in the order the search would ask
            search.lookahead(ahead);
            std::vector<point_key> keys{key_of(x)};
            flat.assign(x.begin(), x.end());
            for (const auto& p : ahead) {
                if ((int)keys.size() >= batch) break;
                const point_key k = key_of(p);
                if (cache.count(k) || std::find(keys.begin(), keys.end(), k) != keys.end()) continue;
                keys.push_back(k);
                flat.insert(flat.end(), p.begin(), p.end());
            }
            scores.assign(keys.size(), 0.0);
            _scorer->calculate_scores(flat.data(), (int)keys.size(), n, scores.data());
            ++res.num_batches;
            res.num_points_scored += (int)keys.size();
            for (size_t i = 0; i < keys.size(); ++i) cache[keys[i]] = scores[i];
            hit = cache.find(keys[0]);
        }
        double f = hit->second;
        if (std::isfinite(f)) {              // the model's state and the scorer's lines are the sequential search's
            if (inference) {
                inference->prepare_calculation(x.data());
                if (!inference->quiet) inference->report_precalculation();
                inference->consumed_cached();
            }
        } else {                             // a reject: scored the ordinary way, so that the model's monitor counts it as it did
            f = _scorer->calculate_score(x.data());
            ++res.num_points_scored;
        }
        if (fed) fed(x, f);
        search.feed(f);
    }
    res.values = search.best();
    res.score = search.best_score();
    res.num_iterations = search.iterations();
    res.num_scorer_calls += search.calls();
    return res;
}

optimizer_result optimizer::optimize(const feed_observer& fed) {
    if (batch > 1) return optimize_batched(fed);
    optimizer_result res;
    const std::vector<double> x0 = get_initial_guesses(res.num_scorer_calls);
    nm_settings s;
    s.max_iterations = max_iterations; s.tolx = tolx; s.tolf = tolf;
    s.similarity_window = similarity_window; s.similarity_precision = similarity_precision;
    nm_search search(s, x0);
    while (!search.done()) search.feed(_scorer->calculate_score(search.trial().data()));
    res.values = search.best();
    res.score = search.best_score();
    res.num_iterations = search.iterations();
    res.num_scorer_calls += search.calls();
    return res;
}

}  // namespace cafe
