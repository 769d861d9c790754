// cafe_gain_posterior: where on the tree a family was absent, where it originated and where it was lost, under the gain model
// of family_gain.hip.  The up pass is cafe_score_per_family_gain's, launch for launch -- the frame of family_frame.h, the branch
// kernel level by level, the sum-rule root kernel -- so lnl has that entry's bits under the sum rule.  A posterior is a ratio
// against the marginal likelihood, so the call uses the sum rule always and neither reads nor changes cafe_set_root_rule.
// Behind the root kernel of a batch the frame's tail runs the down pass (family_gain_down_kernel.h): the root kernel of the
// down pass, then one launch per depth from the root.  Every output of a family is divided by its Z = exp(lnl).
#include "family_gain_down_kernel.h"

namespace cafe {
namespace {

struct GainPosteriorRates {
    using Slot = SlotParamGain;
    static constexpr const char* entry = "cafe_gain_posterior";
    static constexpr bool reads_context_rates = false;
    static constexpr bool absent_ok = true;
    double root_absent;

    static bool rates_ok(int L, const double* mus, const double*) { return death_rates_ok(L, mus); }
    static Slot slot(const cafe_ctx* c, int u, const double* lam, const double* mus, const double* nus) { return gain_branch_slot(c, u, lam, mus, nus); }
    static hipError_t branches(const FamLamArgs<Slot>& a, int n, int64_t nb, int nodes, hipStream_t s) { return launch_family_gain(a, n, nb, nodes, s); }
    hipError_t root(const cafe_ctx*, const FamRootArgs& ra, int64_t nb, hipStream_t s) const { return gain_root_sum(ra, root_absent, nb, s); }
};

// The frame's tail: the second [n_nodes][ld] array of a family (the outside vectors) and its outputs on the device, the
// tables of the down pass, and the way back to the caller's arrays.
struct GainPosteriorTail {
    const cafe_gain_posterior_out* out;
    const float* prior;
    double root_absent;
    bool want_posterior;

    std::vector<int32_t> tables;     // parent [n_nodes], the nodes by depth, the root's children
    std::vector<int> depth_off;
    std::vector<double> mass;
    size_t o_depth = 0, o_rootch = 0, n_rootch = 0;
    FamGainDownRootArgs ra{};
    std::vector<double> host;        // one batch of outputs
    size_t per_node = 0;             // doubles per (family, node) behind the outside vectors
    int nn = 0, N = 0;

    void plan(const cafe_ctx* c) {
        nn = c->n_nodes; N = c->N;
        std::vector<int32_t> depth(nn, 0), order{(int32_t)c->root};
        depth_off = {0};
        for (size_t at = 0; at < order.size(); ++at)           // breadth first: parents in front of their children
            for (int ch : c->children[order[at]]) { depth[ch] = depth[order[at]] + 1; order.push_back(ch); }
        tables.assign(c->parent.begin(), c->parent.end());
        o_depth = tables.size();
        for (size_t at = 1; at < order.size(); ++at) {
            if (depth[order[at]] != depth[order[at - 1]] && at > 1) depth_off.push_back((int)at - 1);
            tables.push_back(order[at]);
        }
        depth_off.push_back((int)order.size() - 1);
        o_rootch = tables.size();
        for (int ch : c->children[c->root]) tables.push_back(ch);
        n_rootch = tables.size() - o_rootch;
        mass.resize((size_t)c->R + 1);
        mass[0] = root_absent;
        for (int j = 1; j <= c->R; ++j) mass[j] = (1.0 - root_absent) * (double)prior[j - 1];
        per_node = 4 + (want_posterior ? (size_t)N : 0);
    }
    size_t static_bytes(const cafe_ctx*) const { return family_align_up(sizeof(int32_t) * tables.size()) + sizeof(double) * mass.size(); }
    size_t family_bytes(const cafe_ctx*, int ld) const { return sizeof(double) * (size_t)nn * ((size_t)ld + per_node); }

    int begin(cafe_ctx* c, const FamLamArgs<SlotParamGain>& a, const FamRootArgs& fra, char* dev_static, char* dev_family, int64_t batch, hipStream_t s) {
        const size_t o_mass = family_align_up(sizeof(int32_t) * tables.size());
        HIP_TRY(c, hipMemcpyAsync(dev_static, tables.data(), sizeof(int32_t) * tables.size(), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(dev_static + o_mass, mass.data(), sizeof(double) * mass.size(), hipMemcpyHostToDevice, s));
        const int32_t* d_tables = reinterpret_cast<const int32_t*>(dev_static);
        double* d = reinterpret_cast<double*>(dev_family);
        const size_t bn = (size_t)batch * nn;
        FamGainDownArgs& g = ra.d;
        g.f = a;
        g.parent = d_tables;
        g.lnl = fra.out;
        g.outside = d;
        g.p_absent = d + bn * a.ld;
        g.mean = g.p_absent + bn;
        g.p_gain = g.mean + bn;
        g.p_loss = g.p_gain + bn;
        g.posterior = want_posterior ? g.p_loss + bn : nullptr;
        g.N = N;
        ra.root_children = d_tables + o_rootch;
        ra.n_root_children = (int32_t)n_rootch;
        ra.mass = reinterpret_cast<const double*>(dev_static + o_mass);
        ra.R = c->R;
        ra.root = c->root;
        host.resize(bn * per_node);
        return CAFE_OK;
    }

    int run(cafe_ctx* c, int64_t nb, hipStream_t s) {
        (void)hipGetLastError();
        hipLaunchKernelGGL(family_gain_down_root_kernel, dim3((unsigned)nb), dim3(64), 0, s, ra);
        HIP_TRY(c, hipGetLastError());
        FamGainDownArgs g = ra.d;
        for (size_t d = 0; d + 1 < depth_off.size(); ++d) {
            g.f.nodes = g.parent + o_depth + depth_off[d];
            HIP_TRY(c, launch_family_gain_down(g, N, nb, depth_off[d + 1] - depth_off[d], s));
        }
        // the four node tables lie side by side, [batch][n_nodes] each with the batch's capacity as stride; the posterior behind them
        const size_t cap = host.size() / per_node;             // batch capacity * n_nodes
        for (int k = 0; k < 4; ++k)
            HIP_TRY(c, hipMemcpyAsync(host.data() + k * cap, g.p_absent + k * cap, sizeof(double) * (size_t)nb * nn, hipMemcpyDeviceToHost, s));
        if (want_posterior)
            HIP_TRY(c, hipMemcpyAsync(host.data() + 4 * cap, g.posterior, sizeof(double) * (size_t)nb * nn * N, hipMemcpyDeviceToHost, s));
        return CAFE_OK;
    }

    // which[b]: the caller's entry of the batch's family b; lnl[b]: its value.  A family without a finite lnl keeps its NaN.
    void collect(const int64_t* which, const double* lnl, int64_t nb) {
        const size_t cap = host.size() / per_node;
        double* const dst[4] = {out->p_absent, out->mean, out->p_gain, out->p_loss};
        for (int64_t b = 0; b < nb; ++b) {
            if (!std::isfinite(lnl[b])) continue;
            for (int k = 0; k < 4; ++k) std::memcpy(dst[k] + which[b] * nn, host.data() + k * cap + (size_t)b * nn, sizeof(double) * nn);
            if (want_posterior) std::memcpy(out->posterior + which[b] * nn * N, host.data() + 4 * cap + (size_t)b * nn * N, sizeof(double) * (size_t)nn * N);
        }
    }
};

int gain_posterior_impl(cafe_ctx* c, const cafe_params* pr, int64_t n, const int64_t* family, const double* lambdas, const double* mus, const double* nus,
                        double root_absent, const cafe_gain_posterior_out* out) {
    const char* const who = GainPosteriorRates::entry;
    if (!out || (n > 0 && (!out->p_absent || !out->mean || !out->p_gain || !out->p_loss))) {
        set_err(c, "%s: out with p_absent, mean, p_gain and p_loss is required", who);
        return CAFE_ERR_ARGUMENT;
    }
    if (const int rc = gain_rates_check(c, who, n, nus, root_absent)) return rc;
    std::vector<double> own_lnl;
    double* lnl = out->lnl;
    if (!lnl && n > 0) { own_lnl.resize((size_t)n); lnl = own_lnl.data(); }
    GainPosteriorTail tail{out, pr && pr->prior ? pr->prior : nullptr, root_absent, out->posterior != nullptr};
    if (tail.prior && n > 0) {
        tail.plan(c);
        const size_t nodes = (size_t)n * c->n_nodes;
        const double nan = std::numeric_limits<double>::quiet_NaN();
        std::fill(out->p_absent, out->p_absent + nodes, nan);
        std::fill(out->mean, out->mean + nodes, nan);
        std::fill(out->p_gain, out->p_gain + nodes, nan);
        std::fill(out->p_loss, out->p_loss + nodes, nan);
        if (out->posterior) std::fill(out->posterior, out->posterior + nodes * c->N, nan);
    }
    return per_family_frame(GainPosteriorRates{root_absent}, tail, c, pr, n, family, lambdas, mus, nus, lnl);
}

}  // namespace
}  // namespace cafe

int cafe_gain_posterior(cafe_ctx* ctx, const cafe_params* params, int64_t n, const int64_t* family, const double* lambdas, const double* mus,
                        const double* nus, double root_absent, const cafe_gain_posterior_out* out) {
    const int rc = cafe::guarded(ctx, "cafe_gain_posterior",
                                 [&] { return cafe::gain_posterior_impl(ctx, params, n, family, lambdas, mus, nus, root_absent, out); });
    if (rc == CAFE_ERR_DEVICE && ctx->device_ready && ctx->stream) (void)hipStreamSynchronize(ctx->stream);     // what the failed call left in flight
    return rc;
}
