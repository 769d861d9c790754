// Lambda-per-family mode (the reference's -b; estimator::estimate_lambda_per_family, src/execute.cpp:104-128).
//
// The reference runs one Nelder-Mead search per family, one family after the other, each scorer call on a one-family
// model.  The searches are independent, so here they advance in lock step: per round the host gathers the next trial
// vector of every unfinished family (nm_search: the moves and stop rules of optimizer::optimize), scores them all in one
// cafe_score_per_family call and feeds every family its own score.  A family whose search ended is restarted from its
// best point while that still gains (see below); then it leaves the list.  Families with identical counts are searched once.  Initial guesses are RNG-driven, so trajectories differ from the reference's;
// optima are compared, not paths.
// With separate death rates per family (per_family_mu) the same rounds score through cafe_score_per_family_lm: mu fixed at
// the given rates, or searched with the lambdas.  The latter runs the lock-step search twice: first over the lambdas with every
// mu tied to its lambda -- the draws, rounds and result of plain -b -- then over [lambdas..., mus...] from that result, every mu
// starting at its lambda.  A Nelder-Mead search never ends above its start, so a family's (lambda, mu) fit is never worse than
// its lambda-only fit: the models are nested, and the search says so by construction.  This DEVIATES from the plan of one
// search over [lambdas..., mus...] from the random guess (mu at the lambda guess), which was built first and gave no such
// thing: cafexp_hip -b --family-mu estimate -s 7 on tests/golden/data/mammals_24.txt, run on an MI355X, left family 0 at
// 8.5e-3 in lnL BELOW its lambda-only optimum (the lambdas and mus it printed, scored by cafe_score_per_family_lm).  The price is
// the rounds of plain -b on top of those of the second search (DESIGN section 8 has the counts).
#include "cafe_host.h"

#include <algorithm>
#include <cmath>
#include <iostream>
#include <memory>

namespace cafe {

void initialization_failure_advice(std::ostream& ost, const std::vector<gene_family>& families) {
    std::vector<std::pair<std::string, int>> m;                 // id, largest count - smallest count
    for (const gene_family& gf : families) {
        int lo = 0, hi = 0;
        bool first = true;
        for (const std::string& sp : gf.get_species()) {
            const int c = gf.get_species_size(sp);
            if (c == kCountMissing) continue;
            lo = first ? c : std::min(lo, c);
            hi = first ? c : std::max(hi, c);
            first = false;
        }
        m.emplace_back(gf.id(), hi - lo);
    }
    std::sort(m.begin(), m.end(), [](const std::pair<std::string, int>& a, const std::pair<std::string, int>& b) { return a.second > b.second; });
    if (m.size() > 20) m.resize(20);
    ost << "\nFamilies with largest size differentials:\n";
    for (const auto& t : m) ost << t.first << ": " << t.second << "\n";
    ost << "\nYou may want to try removing the top few families with the largest difference\nbetween the max and min counts and then re-run the analysis.\n\n";
}

per_family_result estimate_lambda_per_family(hip_base_model& mdl, user_data& data, int max_iterations, const per_family_mu& family_mu) {
    const std::vector<gene_family>& fams = data.gene_families;
    per_family_result res;
    res.lambdas.resize(fams.size());
    if (fams.empty()) return res;

    // the lambda structure (one lambda, or one per index of the lambda tree) and the starts' scale (execute.cpp:116,
    // base_model.cpp:114-131)
    mdl.initialize_lambda(data.p_lambda_tree.get());
    std::unique_ptr<lambda> owned(mdl.get_lambda());
    const int L = owned->count();
    if (family_mu.mode == per_family_mu::FIXED && (int)family_mu.fixed.size() != L)
        throw std::runtime_error("--family-mu needs one death rate per lambda (" + std::to_string(L) + ")");
    const std::set<double> lengths = data.p_tree->get_branch_lengths();
    lambda_optimizer starts(owned.get(), &mdl, data.p_prior.get(), *std::max_element(lengths.begin(), lengths.end()), data.rootdist);

    // families with identical counts are searched once
    std::vector<int64_t> rep;                                   // distinct family -> first family with these counts
    std::vector<size_t> distinct_of(fams.size());
    std::map<std::string, size_t> seen;
    for (size_t f = 0; f < fams.size(); ++f) {
        std::string key;
        for (const std::string& sp : fams[f].get_species()) key += sp + ':' + std::to_string(fams[f].get_species_size(sp)) + ',';
        const auto it = seen.emplace(key, rep.size());
        if (it.second) rep.push_back((int64_t)f);
        distinct_of[f] = it.first->second;
    }
    const size_t D = rep.size();
    res.distinct_families = D;

    // x: the points of `who`, W coordinates each -- W = L: the lambdas (mu fixed, or tied to lambda: the lambda = mu entry,
    // whose bits cafe_score_per_family_lm has at mu = lambda); W = 2L: [lambdas..., mus...]
    auto score = [&](const std::vector<size_t>& who, const std::vector<double>& x, int W) {
        std::vector<int64_t> family(who.size());
        for (size_t i = 0; i < who.size(); ++i) family[i] = rep[who[i]];
        ++res.rounds;
        res.evaluations += (long)who.size();
        if (W == L && family_mu.mode != per_family_mu::FIXED) return mdl.per_family_scores(data.p_prior.get(), data.rootdist, family, x);
        std::vector<double> lam, mu;
        for (size_t i = 0; i < who.size(); ++i) {
            lam.insert(lam.end(), x.begin() + i * W, x.begin() + i * W + L);
            if (W == L) mu.insert(mu.end(), family_mu.fixed.begin(), family_mu.fixed.end());
            else mu.insert(mu.end(), x.begin() + i * W + L, x.begin() + (i + 1) * W);
        }
        return mdl.per_family_scores(data.p_prior.get(), data.rootdist, family, lam, &mu);
    };

    // starts: one draw per distinct family in order of first appearance; the infinite ones are redrawn, in the same order
    std::vector<std::vector<double>> x0(D);
    std::vector<double> f0(D);
    std::vector<size_t> todo(D);
    for (size_t d = 0; d < D; ++d) todo[d] = d;
    for (int attempt = 0; !todo.empty(); ++attempt) {
        if (attempt > 100) {                                    // NUM_OPTIMIZER_INITIALIZATION_ATTEMPTS
            initialization_failure_advice(std::cerr, fams);
            throw std::runtime_error("Failed to initialize any reasonable values");
        }
        std::vector<double> lam;
        for (size_t d : todo) {
            x0[d] = starts.initial_guesses();
            lam.insert(lam.end(), x0[d].begin(), x0[d].end());
        }
        const std::vector<double> s = score(todo, lam, L);
        std::vector<size_t> again;
        for (size_t i = 0; i < todo.size(); ++i) {
            f0[todo[i]] = s[i];
            if (std::isinf(s[i])) again.push_back(todo[i]);
        }
        todo.swap(again);
    }

    // Restarts.  The similarity cutoff stops a search whose best score has not moved by 1e-3 in 12 iterations.  With several
    // lambdas the optimum often lies against saturation boundaries (1 / a branch length: every trial beyond scores +inf),
    // where a simplex spends 12 iterations contracting without a better vertex while another lambda is still far off: on
    // mammals with two lambdas one plain search in eight ended within 1e-3 of the optimum, the others 0.01 to 14 in lnL
    // short of it (the existing scalar search and this one alike).  So a family whose search ended is searched again from
    // its best point: the same moves, a first simplex that steps towards SMALLER lambdas (factor 1 - delta: valid points,
    // where 1 + delta would land beyond the boundary) and the high-precision stop rule (tolx, tolf) alone; again while the
    // last search still gained more than tolf.  No random draw is involved.  Measured over eight seeds on that family: five
    // now end within 1e-4 of the optimum, three still 0.013 to 0.04 short -- a simplex whose best vertex lies within 1e-8 of
    // a boundary cannot move along it, restarted or not.
    const int max_restarts = 20;
    nm_settings settings;
    settings.max_iterations = max_iterations;
    nm_settings inward = settings;                              // a restart's first simplex steps towards smaller lambdas: valid points
    inward.delta = -settings.delta;
    inward.similarity_window = 0;                               // and it runs to the high-precision rule (tolx, tolf) alone
    // one lock-step search of every distinct family from the points `from` (their scores known), W coordinates per point
    auto lock_step = [&](const std::vector<std::vector<double>>& from, const std::vector<double>& from_score, int W) {
        std::vector<nm_search> search;
        search.reserve(D);
        std::vector<size_t> active;
        std::vector<double> start_score(from_score);               // the score the family's current search began with
        std::vector<int> restarts(D, 0);
        // the family's search ended: true if it goes on from its best point
        auto restart = [&](size_t d) {
            const double gain = start_score[d] - search[d].best_score();
            if (!(gain > settings.tolf) || restarts[d] >= max_restarts) return false;
            ++restarts[d];
            ++res.restarts;
            start_score[d] = search[d].best_score();
            const std::vector<double> best = search[d].best();
            search[d] = nm_search(inward, best);
            search[d].feed(start_score[d]);                         // the first trial is the point itself: its score is known
            return !search[d].done();
        };
        for (size_t d = 0; d < D; ++d) {
            search.emplace_back(settings, from[d]);
            search[d].feed(from_score[d]);                          // the first trial is the start itself: its score is known
            if (!search[d].done() || restart(d)) active.push_back(d);
        }
        while (!active.empty()) {
            std::vector<double> lam;
            lam.reserve(active.size() * W);
            for (size_t d : active) lam.insert(lam.end(), search[d].trial().begin(), search[d].trial().end());
            const std::vector<double> s = score(active, lam, W);
            std::vector<size_t> still;
            for (size_t i = 0; i < active.size(); ++i) {
                search[active[i]].feed(s[i]);
                if (!search[active[i]].done() || restart(active[i])) still.push_back(active[i]);
            }
            active.swap(still);
        }
        return search;
    };
    std::vector<nm_search> search = lock_step(x0, f0, L);
    if (family_mu.mode == per_family_mu::ESTIMATE) {            // from the lambda-only optimum, mu = lambda: a point whose score is known
        std::vector<std::vector<double>> x1(D);
        std::vector<double> f1(D);
        for (size_t d = 0; d < D; ++d) {
            x1[d] = search[d].best();
            x1[d].insert(x1[d].end(), search[d].best().begin(), search[d].best().end());
            f1[d] = search[d].best_score();
        }
        search = lock_step(x1, f1, 2 * L);
    }
    if (family_mu.mode != per_family_mu::NONE) res.mus.resize(fams.size());
    for (size_t f = 0; f < fams.size(); ++f) {
        const std::vector<double>& best = search[distinct_of[f]].best();
        res.lambdas[f].assign(best.begin(), best.begin() + L);
        if (family_mu.mode == per_family_mu::FIXED) res.mus[f] = family_mu.fixed;
        else if (family_mu.mode == per_family_mu::ESTIMATE) res.mus[f].assign(best.begin() + L, best.end());
    }
    mdl.set_lambda(nullptr);                                    // `owned` goes with this scope
    return res;
}

}  // namespace cafe
