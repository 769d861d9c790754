// --gain-posterior: the reports of cafe_gain_posterior at the fitted rates of a gain run.  The device call lists every distinct
// family once (gain_table); the reports speak of the table's families, so a distinct entry counts with its multiplicity.
//   Gain_origins.tab          per family: p_absent:mean of every node, then p_gain:p_loss of every branch
//   Gain_branch_origins.tab   per branch: the expected number of families that originated on it (sum p_gain), that were lost on
//                             it (sum p_loss), that are present at the node below it (sum 1 - p_absent), and the number of
//                             families with p_gain > 0.5 there; a root line with the expected number of families absent at the root
// Pure arithmetic and text: no device, no HIP library (gain_origins_tests.cpp).
#include "cafe_host.h"

#include <cmath>
#include <cstdio>
#include <ostream>

namespace cafe {

gain_branch_origins gain_origin_totals(const gain_origins& o, const std::vector<double>& weight, size_t root) {
    const size_t m = o.n_nodes, entries = o.lnl.size();
    if (weight.size() != entries || root >= m || o.p_absent.size() != entries * m || o.mean.size() != entries * m || o.p_gain.size() != entries * m ||
        o.p_loss.size() != entries * m)
        throw std::runtime_error("gain_origin_totals: one weight per entry and [entries][nodes] tables are required");
    gain_branch_origins t;
    t.originated.assign(m, 0.0); t.lost.assign(m, 0.0); t.present.assign(m, 0.0); t.likely_origin.assign(m, 0.0);
    for (size_t e = 0; e < entries; ++e) {
        const double w = weight[e];
        if (!(w > 0)) continue;
        if (!std::isfinite(o.lnl[e])) { t.failed += w; continue; }
        t.used += w;
        bool somewhere = false;
        for (size_t v = 0; v < m; ++v) {
            const size_t at = e * m + v;
            t.present[v] += w * (1.0 - o.p_absent[at]);
            if (v == root) { t.absent_at_root += w * o.p_absent[at]; continue; }
            t.originated[v] += w * o.p_gain[at];
            t.lost[v] += w * o.p_loss[at];
            if (o.p_gain[at] > 0.5) { t.likely_origin[v] += w; somewhere = true; }
        }
        if (somewhere) t.origin_somewhere += w;
    }
    return t;
}

void write_gain_origins(std::ostream& ost, const gain_origins& o, const std::vector<std::string>& node_names, size_t root,
                        const std::vector<std::string>& family_ids, const std::vector<size_t>& entry_of) {
    const size_t m = o.n_nodes;
    if (node_names.size() != m || entry_of.size() != family_ids.size()) throw std::runtime_error("write_gain_origins: one name per node and one entry per family are required");
    ost << "FamilyID";
    for (size_t v = 0; v < m; ++v) ost << "\t" << node_names[v];
    for (size_t v = 0; v < m; ++v)
        if (v != root) ost << "\t" << node_names[v] << "^";                       // the branch above the node
    ost << "\n";
    char buf[96];
    for (size_t i = 0; i < family_ids.size(); ++i) {
        const size_t e = entry_of[i];
        if (e >= o.lnl.size()) throw std::runtime_error("write_gain_origins: family " + family_ids[i] + " has no entry");
        ost << family_ids[i];
        for (size_t v = 0; v < m; ++v) {
            std::snprintf(buf, sizeof buf, "\t%.6g:%.6g", o.p_absent[e * m + v], o.mean[e * m + v]);
            ost << buf;
        }
        for (size_t v = 0; v < m; ++v) {
            if (v == root) continue;
            std::snprintf(buf, sizeof buf, "\t%.6g:%.6g", o.p_gain[e * m + v], o.p_loss[e * m + v]);
            ost << buf;
        }
        ost << "\n";
    }
}

void write_gain_branch_origins(std::ostream& ost, const gain_branch_origins& t, const std::vector<std::string>& node_names, size_t root) {
    const size_t m = node_names.size();
    if (t.originated.size() != m || root >= m) throw std::runtime_error("write_gain_branch_origins: one name per node is required");
    char buf[200];
    std::snprintf(buf, sizeof buf, "#Node\toriginated\tlost\tpresent\tp_gain>0.5\t(expected numbers of families, summed over %.12g families; %.12g failed)\n", t.used,
                  t.failed);
    ost << buf;
    for (size_t v = 0; v < m; ++v) {
        if (v == root) continue;
        std::snprintf(buf, sizeof buf, "\t%.12g\t%.12g\t%.12g\t%.12g\n", t.originated[v], t.lost[v], t.present[v], t.likely_origin[v]);
        ost << node_names[v] << buf;
    }
    std::snprintf(buf, sizeof buf, "\tabsent\t%.12g\tpresent\t%.12g\n", t.absent_at_root, t.present[root]);
    ost << "#Root " << node_names[root] << buf;
}

}  // namespace cafe
