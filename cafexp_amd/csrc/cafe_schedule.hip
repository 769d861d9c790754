// Host planner of cafe_create (cafe_create.hip): subtree patterns, schedule emission, step levelling, panel arena, extent
// levels, leaf-transpose choice, launch grouping.  Nothing here calls HIP or reads the environment: every function reads
// its inputs from its arguments and the context's host fields and writes host fields only.
#include <algorithm>
#include <unordered_map>

#include "cafe_ctx.h"

namespace cafe {

namespace {

// Sethi-Ullman style need: panels live while evaluating node v (leaves need none).
int panel_need(const cafe_ctx* c, int v, std::vector<int>& need) {
    std::vector<int> kid;
    for (int u : c->inner[v]) kid.push_back(panel_need(c, u, need));
    std::sort(kid.begin(), kid.end(), std::greater<int>());
    int n = (int)kid.size() + 1;
    for (size_t i = 0; i < kid.size(); ++i) n = std::max(n, (int)i + kid[i]);
    need[v] = n;
    return n;
}

struct PanelAlloc {
    bool reuse = true;          // false: every panel gets an id of its own (grouped schedule; the arena is planned afterwards)
    std::vector<int> free_list;
    int high = 0;
    int get() { if (reuse && !free_list.empty()) { int p = free_list.back(); free_list.pop_back(); return p; } return high++; }
    void put(int p) { if (reuse) free_list.push_back(p); }
};

int emit_node(const cafe_ctx* c, bool dedup, int v, const std::vector<int>& need, PanelAlloc& pa, std::vector<Op>& ops) {
    const std::vector<int>& inner = c->inner[v];
    const std::vector<int>& leaves = c->leaves[v];
    std::vector<int> order = inner;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return need[x] > need[y]; });
    std::map<int, int> panel_of;
    for (size_t idx = 0; idx < order.size(); ++idx) panel_of[order[idx]] = emit_node(c, dedup, order[idx], need, pa, ops);
    const int dst = pa.get();
    bool init = false;
    // A parent with interior children folds (up to kMaxLeafPerOp of) its leaf children into the epilogue of
    // the first GEMM; a parent with leaf children only (a cherry) is a pure gather.  Extra leaves gather-multiply.
    // (one leaf, without an error model or with a 3-tap one: the specialised epilogues of prune_gemm.hip)
    // A child with fewer distinct columns than its parent (subtree-level de-duplication) first gets its factor
    // P . L over ITS columns in a scratch panel, which a combine pass spreads over the parent's columns.
    auto is_direct = [&](int u) { return !dedup || c->edge_identity[u]; };
    const bool first_direct = !inner.empty() && is_direct(inner[0]);
    // (a table with missing cells: K2's leaf epilogues turn the count into a buffer offset and know no missing count -- the leaf
    // goes to a K3 pass instead, whose MISSING instantiation does)
    size_t fused = (!first_direct || leaves.empty() || (c->n_dev != 0 && c->n_dev != 3) || c->has_missing) ? 0 : 1;
    std::vector<std::pair<int, int>> factors;             // (child, scratch panel) waiting to be assembled
    auto new_op = [&](int type, int dst_panel, int mode) { Op o{}; o.type = type; o.parent = v; o.to_root = (v == c->root); o.dst_panel = dst_panel; o.mode = mode; return o; };
    if (inner.size() == 2 && leaves.empty() && is_direct(inner[0]) != is_direct(inner[1])) {
        // one child shares the parent's columns, the other has fewer: the smaller one's factor GEMM runs first over ITS
        // columns, the other's GEMM then writes the parent's panel and multiplies the gathered factor in (the product
        // of two numbers: the same bits whichever child comes first)
        const int big = is_direct(inner[0]) ? inner[0] : inner[1], small = big == inner[0] ? inner[1] : inner[0];
        const int scratch = pa.get();
        Op f = new_op(1, scratch, 0);
        f.src_panel = panel_of[small]; f.child = small; f.to_factor = true;
        ops.push_back(f);
        Op g = new_op(1, dst, 0);
        g.src_panel = panel_of[big]; g.child = big; g.has_gath = true; g.gath_child = small; g.gath_panel = scratch;
        ops.push_back(g);
        pa.put(scratch);
        for (int u : inner) pa.put(panel_of[u]);
        return dst;
    }
    for (size_t gi = 0; gi < inner.size(); ++gi) {   // child order of the reference (probability.cpp:205 walks _descendants in order)
        const int u = inner[gi];
        const bool direct = is_direct(u);
        Op op = new_op(1, direct ? dst : pa.get(), direct && init ? 1 : 0);
        op.src_panel = panel_of[u]; op.child = u;
        if (direct) {
            if (gi == 0) {
                op.n_leaf = (int)fused;
                for (size_t l = 0; l < fused; ++l) op.leaf_node[l] = leaves[l];
            }
            init = true;
        } else {
            op.to_factor = true;
            factors.emplace_back(u, op.dst_panel);
        }
        ops.push_back(op);
    }
    // assemble the parent's panel: up to two factor panels and two leaf children per pass, written once
    size_t li = fused, fi = 0;
    while (li < leaves.size() || fi < factors.size()) {
        Op op = new_op(0, dst, init ? 1 : 0);
        const size_t max_leaf = factors.empty() ? (size_t)kMaxLeafPerOp : 2;     // the fast kernel takes two of each
        op.n_leaf = (int)std::min<size_t>(max_leaf, leaves.size() - li);
        for (int l = 0; l < op.n_leaf; ++l) op.leaf_node[l] = leaves[li + l];
        li += op.n_leaf;
        op.n_src = (int)std::min<size_t>(2, factors.size() - fi);
        for (int j = 0; j < op.n_src; ++j) { op.src_child[j] = factors[fi + j].first; op.src_panels[j] = factors[fi + j].second; }
        fi += op.n_src;
        ops.push_back(op);
        init = true;
    }
    for (auto& fs : factors) pa.put(fs.second);
    for (int u : inner) pa.put(panel_of[u]);
    return dst;
}

// Steps: an op runs one step after the last op it depends on -- the writers of what it reads (its children's panels,
// gathered factors, and its own destination when it multiplies).  Returns the number of steps.
int level_steps(std::vector<Op>& ops, size_t n_panels) {
    std::vector<int> last_writer(n_panels, -1);
    int n_steps = 0;
    for (size_t i = 0; i < ops.size(); ++i) {
        Op& op = ops[i];
        int st = 0;
        auto dep = [&](int panel) { if (last_writer[panel] >= 0) st = std::max(st, ops[last_writer[panel]].step + 1); };
        if (op.type == 1) { dep(op.src_panel); if (op.has_gath) dep(op.gath_panel); }
        for (int j = 0; j < op.n_src; ++j) dep(op.src_panels[j]);
        dep(op.dst_panel);                           // (a store is the first writer: no-op; a multiply follows the store)
        op.step = st;
        last_writer[op.dst_panel] = (int)i;
        n_steps = std::max(n_steps, st + 1);
    }
    return n_steps;
}

// Arena: first fit over the steps; a panel's place is free again after the step that reads it last.  Sets every panel's
// offset from its lifetime [first_step, last_step] and returns the arena's size in doubles.
int64_t place_panels(std::vector<Panel>& panels, int n_steps, int Kmax) {
    std::vector<std::pair<int64_t, int64_t>> holes;  // (offset, length) sorted by offset
    int64_t top = 0;
    std::vector<std::vector<int>> born(n_steps + 1), dies(n_steps + 1);
    for (size_t i = 0; i < panels.size(); ++i) { born[panels[i].first_step].push_back((int)i); dies[panels[i].last_step].push_back((int)i); }
    for (int st = 0; st <= n_steps; ++st) {
        std::sort(born[st].begin(), born[st].end(), [&](int x, int y) { return panels[x].kstride > panels[y].kstride; });
        for (int id : born[st]) {
            Panel& P = panels[id];
            const int64_t len = round_up64(P.kstride * Kmax, 64);          // 512-byte granules
            bool placed = false;
            for (size_t h = 0; h < holes.size() && !placed; ++h)
                if (holes[h].second >= len) {
                    P.offset = holes[h].first;
                    holes[h].first += len; holes[h].second -= len;
                    if (holes[h].second == 0) holes.erase(holes.begin() + h);
                    placed = true;
                }
            if (!placed) {
                P.offset = top;
                if (!holes.empty() && holes.back().first + holes.back().second == top) { P.offset = holes.back().first; holes.pop_back(); }   // grow the hole at the top
                top = P.offset + len;
            }
        }
        for (int id : dies[st]) {
            const Panel& P = panels[id];
            const int64_t len = round_up64(P.kstride * Kmax, 64);
            auto it = std::lower_bound(holes.begin(), holes.end(), std::make_pair(P.offset, (int64_t)0));
            it = holes.insert(it, std::make_pair(P.offset, len));
            if (it + 1 != holes.end() && it->first + it->second == (it + 1)->first) { it->second += (it + 1)->second; holes.erase(it + 1); }
            if (it != holes.begin() && (it - 1)->first + (it - 1)->second == it->first) { (it - 1)->second += it->second; holes.erase(it); }
        }
    }
    return top;
}

struct Schedule {                             // a candidate; plan_schedule commits the chosen one to the context
    bool dedup = false, grouped = false;
    std::vector<Op> ops;
    std::vector<Panel> panels;                // (grouped: offsets in the arena; slot pool: slots of a column chunk)
    int root_panel = -1;
    int64_t chunk_cols = 0;                  // 0: not even one 128-family tile fits the workspace
    size_t panel_doubles = 0;                // the arena
};

// GROUPED: every panel has a place of its own in an arena planned from the panels' lifetimes, one column chunk
Schedule grouped_schedule(const cafe_ctx* c, bool dedup, const std::vector<int>& need) {
    Schedule s;
    s.dedup = dedup; s.grouped = true; s.chunk_cols = c->Fp;
    PanelAlloc pa{false};                    // a place of its own for every panel
    s.root_panel = emit_node(c, dedup, c->root, need, pa, s.ops);
    s.panels.assign(pa.high, Panel());
    // what each panel is: the transposed factor of a child (its own columns) or a node's panel
    for (const Op& op : s.ops) {
        Panel& P = s.panels[op.dst_panel];
        P.factor = op.type == 1 && op.to_factor;
        P.cols = panel_cols(dedup, c, P.factor ? op.child : op.parent, c->Fp);
        P.kstride = P.cols * (P.factor ? c->factor_ld : c->rows_pad);
    }
    const int n_steps = level_steps(s.ops, s.panels.size());
    for (Panel& P : s.panels) { P.first_step = 0x7fffffff; P.last_step = -1; }
    for (const Op& op : s.ops) {
        auto use = [&](int panel) { Panel& P = s.panels[panel]; P.first_step = std::min(P.first_step, op.step); P.last_step = std::max(P.last_step, op.step); };
        use(op.dst_panel);
        if (op.type == 1) { use(op.src_panel); if (op.has_gath) use(op.gath_panel); }
        for (int j = 0; j < op.n_src; ++j) use(op.src_panels[j]);
    }
    s.panels[s.root_panel].last_step = n_steps;    // K4 and cafe_get_root_likelihoods read it after the last step
    s.panel_doubles = (size_t)place_panels(s.panels, n_steps, c->Kmax);
    return s;
}

// SLOT POOL: every slot as wide as the column chunk the workspace holds for all; a node uses a prefix with its own ld
Schedule slot_schedule(const cafe_ctx* c, bool dedup, const std::vector<int>& need, size_t budget, int64_t desc_cols) {
    Schedule s{dedup};
    PanelAlloc pa;                           // few live panels: their ids are slots
    s.root_panel = emit_node(c, dedup, c->root, need, pa, s.ops);
    const size_t per_col = (size_t)pa.high * c->Kmax * c->rows_pad * sizeof(double);
    const int64_t cols = std::min<int64_t>((int64_t)(budget / per_col) / kBN * kBN, desc_cols);
    s.chunk_cols = std::min<int64_t>(cols, c->Fp);
    const int64_t kstride = (int64_t)c->rows_pad * s.chunk_cols;
    s.panels.assign(pa.high, Panel());
    for (int i = 0; i < pa.high; ++i) { s.panels[i].cols = s.chunk_cols; s.panels[i].offset = (int64_t)i * kstride * c->Kmax; s.panels[i].kstride = kstride; }
    for (size_t i = 0; i < s.ops.size(); ++i) s.ops[i].step = (int)i;
    s.panel_doubles = (size_t)pa.high * kstride * c->Kmax;
    return s;
}

}  // namespace

// Subtree-level de-duplication (host side, once): the distinct patterns of leaf counts under every interior node, the
// column of each child for every column of its parent, and the leaf children's counts per parent column.  Columns are
// numbered by first occurrence in (distinct-)family order, so the root's columns are the distinct families themselves
// and a child with as many patterns as its parent has them in the same order (an identity map: no combine pass).
//
// cherry_swap: a node whose only children are two leaves on the same matrix (equal quantized branch length and lambda index --
// what plan_pools makes one pair of; mu goes by the lambda index) keys its patterns on the UNORDERED pair of counts.  Its
// column for counts (a, b) is P[s][a] * P[s][b] -- each factor formed from its leaf's count alone (one matrix column, or the
// error-model taps in tap order), the panel value their product in store mode (leaf_gather_fast_kernel, leaf_gather_kernel:
// v = 1.0 * fa * fb) -- and an IEEE product does not depend on the order of its factors, so (b, a) has the same bits and
// shares the column.  The representative keeps its counts in leaf order; parents see the merged pid and shrink by
// themselves.  A node with any further child is not covered: (F * fa) * fb and (F * fb) * fa may differ in the last bit.
void plan_patterns(cafe_ctx* c, const cafe_problem* p, const std::vector<int64_t>& uniq, bool cherry_swap, double inherit_all, double inherit_big) {
    const int n = c->n_nodes, T = c->n_taxa;
    const int64_t F = c->F_uniq;
    c->pat_cols.assign(n, 0);
    c->edge_identity.assign(n, 0);
    c->h_edge_map.assign(n, {});
    c->h_leaf_cnt.assign(n, {});
    c->leaf_rank.assign(n, 0);
    // ---- 1. every interior node's own patterns, children first.  Patterns are numbered in the order of the node's
    // HEAVY child's pattern numbers (the interior child with the most patterns; ties and cherries: first occurrence in
    // family order), so that along the heavy path a parent's columns map to non-decreasing child columns: the
    // gathers of the assemble passes and of K2's gathered-factor epilogue then read the big factor panel in order.
    std::vector<std::vector<int32_t>> pid(n);            // [interior node][distinct family] own pattern index
    std::vector<std::vector<int64_t>> rep(n);            // [interior node][own pattern] first distinct family showing it
    for (int v = 0; v < n; ++v) {
        if (c->leaf_taxon[v] >= 0) continue;
        const std::vector<int>& inner = c->inner[v];
        const std::vector<int>& leaves = c->leaves[v];
        const size_t kw = inner.size() + leaves.size();
        pid[v].resize(F);
        if (v == c->root) {                              // the root keeps one column per family of the context (K4 reads them
            rep[v].resize(F);                            // by family index), also when identical families were kept apart
            for (int64_t f = 0; f < F; ++f) { pid[v][f] = (int32_t)f; rep[v][f] = f; }
            continue;
        }
        std::unordered_map<std::string, int32_t> seen;
        seen.reserve((size_t)F * 2);
        std::vector<int64_t> first;                      // raw pattern (first-occurrence number) -> first family
        std::vector<int32_t> key(kw);
        const bool symmetric = cherry_swap && inner.empty() && leaves.size() == 2 && c->lam_idx[leaves[0]] == c->lam_idx[leaves[1]] &&
                               quantize_time(c->blen[leaves[0]]) == quantize_time(c->blen[leaves[1]]);
        for (int64_t f = 0; f < F; ++f) {
            size_t k = 0;
            for (int u : inner) key[k++] = pid[u][f];
            for (int u : leaves) key[k++] = p->counts[uniq[f] * T + c->leaf_taxon[u]];
            if (symmetric && key[0] > key[1]) std::swap(key[0], key[1]);
            std::string ks(reinterpret_cast<const char*>(key.data()), sizeof(int32_t) * kw);
            auto it = seen.find(ks);
            if (it == seen.end()) {
                it = seen.emplace(std::move(ks), (int32_t)first.size()).first;
                first.push_back(f);
            }
            pid[v][f] = it->second;
        }
        int heavy = -1;
        for (int u : inner) if (heavy < 0 || rep[u].size() > rep[heavy].size()) heavy = u;
        const size_t U = first.size();
        std::vector<int32_t> order(U), renum(U);
        for (size_t i = 0; i < U; ++i) order[i] = (int32_t)i;
        // largest leaf count under v, per pattern: the primary key (columns of similar size share a 128-column tile, whose
        // all-zero rows K2 skips); within equal sizes the heavy child's numbering
        std::vector<int32_t> big(U, 0), small(U, 0x7fffffff);
        std::vector<int> under, stack(1, v);              // taxa under v
        while (!stack.empty()) {
            const int w = stack.back(); stack.pop_back();
            if (c->leaf_taxon[w] >= 0) under.push_back(c->leaf_taxon[w]);
            for (int u : c->children[w]) stack.push_back(u);
        }
        for (size_t i = 0; i < U; ++i)
            for (int t : under) {
                const int32_t x = p->counts[uniq[first[i]] * T + t];
                if (count_is_missing(x)) continue;        // (a missing cell moves neither end of a column's non-zero rows)
                big[i] = std::max(big[i], x);
                small[i] = std::min(small[i], x);
            }
        // (the lower end of a column's non-zero rows follows its largest count, the upper end its smallest)
        std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
            if (big[x] != big[y]) return big[x] < big[y];
            if (small[x] != small[y]) return small[x] < small[y];
            return heavy >= 0 && pid[heavy][first[x]] < pid[heavy][first[y]];
        });
        rep[v].resize(U);
        for (size_t i = 0; i < U; ++i) { renum[order[i]] = (int32_t)i; rep[v][i] = first[order[i]]; }
        for (int64_t f = 0; f < F; ++f) pid[v][f] = renum[pid[v][f]];
    }
    // ---- 2. column space of every interior node, parents first: its own patterns, or its parent's columns, which makes
    // the edge direct (the GEMM's epilogue writes the parent's panel).  A GEMM column costs about 0.12 us, a column of an
    // assemble pass 0.024 us (one factor + leaf) to 0.036 us (two factors) at the bench shape, so:
    // (inherit_all = 0.15, inherit_big = 0.12 unless CAFE_INHERIT sweeps them)
    //  * all interior children inherit when together they add < 15 % GEMM columns (store / multiply epilogues, one leaf
    //    sibling fused);
    //  * of two interior children (no leaf sibling) the larger one inherits alone when it adds < 12 % (an assemble pass
    //    saved is worth about that many GEMM columns): the smaller one keeps its own columns and its factor is gathered
    //    in the larger one's epilogue -- no assemble pass either.
    std::vector<int> space(n, -1);
    space[c->root] = c->root;
    for (int v = n - 1; v >= 0; --v) {
        if (c->leaf_taxon[v] >= 0) continue;
        const std::vector<int>& inner = c->inner[v];
        const size_t n_leaves = c->leaves[v].size();
        const double Uv = (double)rep[space[v]].size();
        double extra = 0;
        for (int u : inner) extra += 1.0 - (double)rep[u].size() / Uv;
        const bool inherit = !inner.empty() && n_leaves <= 1 && extra < inherit_all;
        for (int u : inner) space[u] = inherit ? space[v] : u;
        if (!inherit && inner.size() == 2 && n_leaves == 0) {
            const int big = rep[inner[0]].size() >= rep[inner[1]].size() ? inner[0] : inner[1];
            if (1.0 - (double)rep[big].size() / Uv < inherit_big) space[big] = space[v];
        }
    }
    // ---- 3. tables (cafe_create uploads them)
    for (int v = 0; v < n; ++v) {
        if (c->leaf_taxon[v] >= 0) continue;
        const std::vector<int>& leaves = c->leaves[v];
        const std::vector<int64_t>& cols = rep[space[v]];                // representative family of every column of v's panel
        const int64_t U = (int64_t)cols.size(), Up = round_up64(U, kBN);
        c->pat_cols[v] = Up;
        for (size_t l = 0; l < leaves.size(); ++l) c->leaf_rank[leaves[l]] = (int)l;
        std::vector<int32_t>& tab = c->h_leaf_cnt[v];     // (empty without leaf children)
        tab.assign(leaves.size() * (size_t)Up, 0);
        for (size_t l = 0; l < leaves.size(); ++l)
            for (int64_t u2 = 0; u2 < U; ++u2) tab[l * Up + u2] = p->counts[uniq[cols[u2]] * T + c->leaf_taxon[leaves[l]]];
        for (int u : c->inner[v]) {
            if (space[u] == space[v]) { c->edge_identity[u] = 1; continue; }      // the child's columns ARE the parent's
            std::vector<int32_t> map((size_t)Up, 0);
            bool same = (int64_t)rep[u].size() == U;     // as many own patterns as the parent has columns, in the same order?
            for (int64_t u2 = 0; u2 < U; ++u2) { map[u2] = pid[u][cols[u2]]; same = same && map[u2] == (int32_t)u2; }
            if (same) { c->edge_identity[u] = 1; continue; }
            c->h_edge_map[u].swap(map);
        }
    }
}

// The schedule.  Preferred (the table fits one column chunk with a place of its own for every panel): GROUPED -- the ops
// are levelled by their dependencies into steps, a step's ops of one kernel variant share a launch, and the arena is
// planned from the panels' lifetimes.  Otherwise: one op per launch from the slot pool, in as many column chunks as the
// workspace asks for.  `budget`: bytes of workspace for the panels; `desc_cols`: the widest panel K2 can address.
size_t plan_schedule(cafe_ctx* c, bool dedup, bool try_grouped, size_t budget, int64_t desc_cols) {
    std::vector<int> need(c->n_nodes, 0);
    panel_need(c, c->root, need);
    Schedule s;                              // (not grouped)
    if (try_grouped) {
        s = grouped_schedule(c, dedup, need);
        int64_t widest = 0;
        for (const Panel& P : s.panels) widest = std::max(widest, P.cols);
        // (a place of its own for every panel takes several times the slot pool: not when that is more than half the workspace)
        if (s.panel_doubles * sizeof(double) + 65536 > budget / 2 || widest > desc_cols) s.grouped = false;
    }
    if (!s.grouped) {
        s = slot_schedule(c, dedup, need, budget, desc_cols);
        // several column chunks: the per-node column maps address whole panels, so this case keeps one column per
        // family in every panel (the schedule without combine passes needs no more panels than the one with them)
        if (dedup && s.chunk_cols < c->Fp) s = slot_schedule(c, false, need, budget, desc_cols);
    }
    c->subtree_dedup = s.dedup; c->grouped = s.grouped; c->root_panel = s.root_panel; c->chunk_cols = s.chunk_cols;
    c->ops = std::move(s.ops); c->panels = std::move(s.panels);
    c->n_panels = (int)c->panels.size();
    c->panel_kstride = (int64_t)c->rows_pad * c->chunk_cols;     // (grouped: the root panel's, what K4 reads)
    c->panel_stride = c->grouped ? 0 : c->panel_kstride * c->Kmax;
    c->stats.n_chunks = c->chunk_cols ? (c->Fp + c->chunk_cols - 1) / c->chunk_cols : 0;
    return s.panel_doubles;
}

// Zero extents of the panels: one descriptor per interior non-root node, children before parents, level by level (a
// node's level = 1 + its deepest interior child's).  Sets panel_extents and ext_levels; returns the nodes in descriptor order.
// (one column per family at every node -- CAFE_FLAG_NO_SUBTREE_DEDUP, device-written counts -- works the same way as long
// as the families fit one column chunk: every edge is the identity and the counts are the family table itself)
std::vector<int> plan_extent_levels(cafe_ctx* c, bool matrix_extents) {
    std::vector<int> order;
    c->panel_extents = (c->subtree_dedup || c->stats.n_chunks == 1) && matrix_extents;
    if (!c->panel_extents) return order;
    std::vector<int> level(c->n_nodes, -1);
    std::vector<std::vector<int>> of_level;              // (no level is empty: a node's deepest child is one level down)
    for (int v = 0; v < c->n_nodes; ++v) {
        if (c->leaf_taxon[v] >= 0 || v == c->root) continue;
        if ((int)c->leaves[v].size() > kMaxExtChildren || (int)c->inner[v].size() > kMaxExtChildren) { c->panel_extents = false; return order; }   // (a wide polytomy)
        level[v] = 0;
        for (int u : c->inner[v]) level[v] = std::max(level[v], level[u] + 1);
        of_level.resize(std::max<size_t>(of_level.size(), level[v] + 1));
        of_level[level[v]].push_back(v);
    }
    for (const std::vector<int>& nodes : of_level) {
        cafe_ctx::ExtLevel L{(int)order.size(), (int)nodes.size(), 0};
        for (int v : nodes) L.max_col_tiles = std::max(L.max_col_tiles, (int)(panel_cols(c, v, c->Fp) / kBN));
        order.insert(order.end(), nodes.begin(), nodes.end());
        c->ext_levels.push_back(L);
    }
    return order;
}

// Leaf branches whose matrix an assemble pass multiplies with a factor get a transposed copy (leaf_transpose_kernel, every
// call): the pass then reads the leaf's column as lines, like the factor's, instead of 8 bytes per matrix row (4.0 -> 6 TB/s).
// A copy costs 16 N^2 bytes per category and call whatever the number of columns, so a branch gets one only when the
// passes that read it write enough columns: >= lt_min N.  Bench table: 31 branches, 139.5 -> 137.9 ms per call; its 1/8
// shards copy 2 to 6 branches and take what they took (20.1 / 20.2 ms; with all 30 copied: +0.3 to +0.6 ms).
// The copies must fit a quarter of `free_bytes` (and an eighth of a given workspace limit).  Sets lt_pairs, Op::leaf_t and
// the copy of every leaf pair (-1: none); returns the bytes of the copies (0: none).
size_t plan_leaf_transposes(cafe_ctx* c, double lt_min, size_t free_bytes, std::vector<int>& lt_of_pair) {
    lt_of_pair.assign(std::max(1, c->n_pairs[0]), -1);
    if (c->has_missing) return 0;            // the copies are indexed by count: a table with missing cells gathers its leaves (leaf_reduce.hip)
    std::vector<int64_t> served(lt_of_pair.size(), 0);
    auto eligible = [](const Op& op) { return op.type == 0 && op.n_src >= 1 && op.n_src <= 2 && op.n_leaf >= 1 && op.n_leaf <= 2; };
    for (const Op& op : c->ops)
        if (eligible(op))
            for (int l = 0; l < op.n_leaf; ++l) served[c->pair_of[op.leaf_node[l]]] += panel_cols(c, op.parent, c->Fp) * std::max<int64_t>(1, c->stats.n_chunks);
    for (size_t pr = 0; pr < served.size(); ++pr)
        if (served[pr] > 0 && (double)served[pr] >= lt_min * c->N) { lt_of_pair[pr] = (int)c->lt_pairs.size(); c->lt_pairs.push_back((int)pr); }
    const size_t lt_bytes = sizeof(double) * ((size_t)c->lt_pairs.size() * c->Kmax * (size_t)(c->M + 1) * c->factor_ld + 2 * kBN);
    const bool fits = !c->lt_pairs.empty() && (size_t)c->lt_pairs.size() * c->Kmax <= 65535u && lt_bytes <= free_bytes / 4 &&
                      (!c->workspace_limit || lt_bytes <= c->workspace_limit / 8);
    if (!fits) { c->lt_pairs.clear(); return 0; }
    for (Op& op : c->ops)
        if (eligible(op)) op.leaf_t = std::all_of(op.leaf_node, op.leaf_node + op.n_leaf, [&](int u) { return lt_of_pair[c->pair_of[u]] >= 0; });
    return lt_bytes;
}

// Launches: the ops of a step that share a kernel variant go out together.  Sets groups, every op's descriptor index, the
// room the tile lists of the K2 launches need (plan_entries) and the schedule's counters in stats.
void group_launches(cafe_ctx* c) {
    std::vector<size_t> idx(c->ops.size());
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = i;
    auto key = [&](const Op& o) -> int {                 // launch order inside a step: factor GEMMs, the other GEMMs, then K3
        if (o.type == 1) return o.to_factor ? 0 : 1 + (o.has_gath ? 2 : (o.n_leaf ? 1 : 0)) * 2 + o.mode;
        return 16 + o.n_src * 32 + o.n_leaf * 2 + o.mode + (o.leaf_t ? 1024 : 0);
    };
    std::stable_sort(idx.begin(), idx.end(), [&](size_t x, size_t y) {
        const Op &a = c->ops[x], &b = c->ops[y];
        if (a.step != b.step) return a.step < b.step;
        if (a.to_root != b.to_root) return b.to_root;
        return key(a) < key(b);
    });
    for (size_t i : idx) {
        Op& o = c->ops[i];
        const bool fresh = c->groups.empty() || c->groups.back().step != o.step || c->groups.back().type != o.type ||
                           key(c->ops[c->groups.back().ops[0]]) != key(o) || c->groups.back().to_root != o.to_root ||
                           (int)c->groups.back().ops.size() >= (o.type == 1 ? kMaxGroupOps : 512);
        if (fresh) {
            Group g;
            g.type = o.type; g.step = o.step; g.to_root = o.to_root;
            g.first_desc = o.type == 1 ? c->n_gemm_ops : c->n_gather_ops;
            if (o.type == 1) g.variant = GemmVariant{o.mode, o.has_gath ? 2 : (o.n_leaf ? 1 : 0), o.to_factor ? 1 : 0};
            c->groups.push_back(g);
            c->n_gemm_groups += o.type == 1;
        }
        o.desc = o.type == 1 ? c->n_gemm_ops++ : c->n_gather_ops++;
        c->groups.back().ops.push_back((int)i);
        c->stats.n_gather_epilogues += o.type == 1 && o.has_gath;
        c->stats.n_assemble_passes += o.type == 0 && o.n_src > 0;
        c->stats.n_leaf_passes += o.type == 0 && o.n_src == 0;
    }
    // tile lists of the K2 launches: room for the tallest list any tile height can ask for
    // (the planner is one 64-lane wave per XCD, a lane per workgroup: MI355X has 32 CUs x 2 workgroups per XCD)
    c->plan_entries = 0;
    for (const Group& g : c->groups) {
        if (g.type != 1) continue;
        size_t worst = 0;
        for (int mi = 2; mi <= 9; ++mi) {
            int64_t tiles = 0;
            for (int oi : g.ops) {
                const Op& op = c->ops[oi];
                const int rows = op.to_root ? c->R : c->M;
                tiles += prune_gemm_tiles_xcd0(c->Kmax, (int)(panel_cols(c, op.child, c->chunk_cols) / kBN), (rows + 16 * mi - 1) / (16 * mi));
            }
            worst = std::max(worst, (size_t)8 * (size_t)(tiles + kPlanLanes * (1 + kPlanSlack)));   // >= 8 * nlb * (ceil(tiles / nlb) + slack), any K <= Kmax
        }
        c->plan_entries += worst;
    }
}

// diagnostic (CAFE_DUMP_SCHEDULE): the launch list with its column counts
void dump_schedule(const cafe_ctx* c) {
    std::fprintf(stderr, "cafe schedule: %s, %zu ops in %zu launches, %d panels, %.2f GB\n", c->grouped ? "grouped" : "one op per launch", c->ops.size(),
                 c->groups.size(), c->n_panels, c->stats.panel_bytes / 1e9);
    for (const Group& g : c->groups) {
        std::fprintf(stderr, "cafe schedule: step %d %s x%zu\n", g.step, g.type == 1 ? "K2" : "K3", g.ops.size());
        for (int oi : g.ops) {
            const Op& op = c->ops[oi];
            if (op.type == 1)
                std::fprintf(stderr, "cafe schedule:   gemm child %d -> parent %d cols %lld %s%s%s leaf %d\n", op.child, op.parent,
                             (long long)panel_cols(c, op.child, c->chunk_cols), op.to_factor ? "factor(transposed)" : (op.mode ? "multiply" : "store"),
                             op.has_gath ? " +gathered-factor" : "", op.to_root ? " root" : "", op.n_leaf);
            else
                std::fprintf(stderr, "cafe schedule:   %s parent %d cols %lld factors %d leaves %d %s\n", op.n_src ? "assemble" : "leaf-gather", op.parent,
                             (long long)panel_cols(c, op.parent, c->chunk_cols), op.n_src, op.n_leaf, op.mode ? "multiply" : "store");
        }
    }
}

}  // namespace cafe
