// Covariant compositional networks (CCN_1D / CCN_2D) on gfx950.
//
// Reference: models/compnets/model_ccn.py (CCN_1D 18-64, CCN_2D 68-105) over
// functions/utils_ccn.py (receptive fields and chi matrices 66-145, base
// features 148-222, promotions 225-278, updates 281-324) and
// functions/contraction.py (collapse6to3, 106-121).
//
// Index construction (bit-exact with the reference's int semantics):
//   nbr_i = ascending nonzero(adj[i])  (utils_ccn.py:195-199), d_i = |nbr_i| (incl. self loop)
//   pos[i][a][x] = index of nbr_i[x] in nbr_{j_a} or -1, j_a = nbr_i[a]  == the chi_{i j_a}
//   matrices (utils_ccn.py:66-106) as position maps.
// CCN-1D layer, node i (n = d_i):  T[a][x] = F_{j_a}[pos(x)] ;  row[x] = sum_a T, col[a] = sum_x T;
//   F'_i[x] = relu(W [row[x] | col[x]] + b)                        (utils_ccn.py:303-324)
// CCN-2D layer: T[a][b][z] = F_{j_a}[pos(b)][pos(z)] (chi F chi^T), H = T (x) chi_ii = T (x) I, and
//   the 18 contractions of collapse6to3 reduce to (re-derived in DESIGN.md):
//     q0 = n Sc, q1 = q1[x], q2 = n Sa, q3 = q3[x], q4 = d_xy tot, q5 = Sc, q6..14 = n Sc,
//     q15 = T[x][y][y], q16 = T[y][x][y], q17 = d_xy sum_k T[k][k][k]
//   with Sc[a][b] = sum_z T, Sa[b][z] = sum_a T, q1[a] = sum_bz T, q3[b] = sum_az T.
//   O(n^3 C) per node instead of the reference's materialised n^5 C tensor.
// Backward is a gather over the transposed position maps (no atomics): node j collects,
// for every neighbour i, the gradient of the entries of T_i that read F_j.
//
// This file is the executor of the general path: the layout of the feature workspace and the forward / backward
// entry points, one straight sequence of launches per order.  The kernels are in ccn_plan.hip (index construction,
// the plan workspace), ccn1.hip, ccn2.hip (degrees <= 64), ccn2_big.hip (65..256) and ccn_readout.hip; ccn_general.h
// holds what they share.
#include "ccn_general.h"

namespace hgnn {
namespace {

// The feature workspace, offsets from its own start (the plan workspace is a separate buffer, ccn_plan.hip).
// Per-level arrays are sized by ccn_ok's limit of 15 levels.
struct CcnFeatLayout {
    size_t F[16];     // level l's features: [rows][h], rows = sum d (CCN-1D) or sum d^2 (CCN-2D)
    size_t coll[16];  // CCN-1D: [rows][2 cin] row | column sums
    size_t nsum[16];  // CCN-2D: [nodes][h] per-node sums of F for the readout
    size_t sc[16], sa[16], d1[16], d2[16], q1[16], q3[16], tot[16], d3[16];  // CCN-2D, nmax > 64: C2Save of the level
    size_t feat, rpart, g0, dsum, ppart, dF[2];
    size_t dcoll;                           // CCN-1D
    size_t rdp, trd;                        // CCN-2D: the dp format's row sums and trace
    size_t g_sc, g_sa, g_d1, g_d2, g_d3;    // CCN-2D, nmax > 64: C2Grad
    size_t xp, dxp;
    size_t bytes;
};

// sums: sum d, sum d^2, nodes, max d -- as the plan reported or bounded them
CcnFeatLayout feat_layout(const hgnn_ccn_config* c, const long long* sums) {
    CcnFeatLayout L{};
    const long long sum_d = sums[0], sum_d2 = sums[1];
    const long long nodes = (long long)c->bs * c->nmax;
    size_t t = 0;
    auto take = [&](size_t n) {
        const size_t o = t;
        t += al(n);
        return o;
    };
    const long long rows = c->order == 1 ? sum_d : sum_d2;
    const int Lv = c->layers;
    const int h = c->hidden, f = c->f_in;
    const int cmax = f > h ? f : h;
    const bool big = c->order == 2 && c->nmax > CCN_MAXD;  // degrees above 64 possible
    for (int l = 0; l < Lv; ++l) {
        const int cin = l == 0 ? f : h;
        L.F[l] = take(4 * (size_t)rows * h);
        if (c->order == 2) L.nsum[l] = take(4 * (size_t)nodes * h);
        if (c->order == 1) {
            L.coll[l] = take(4 * (size_t)rows * 2 * cin);
        } else if (big) {  // C2Save: only the large-degree kernels keep contraction statistics
            L.sc[l] = take(4 * (size_t)sum_d2 * cin);
            L.sa[l] = take(4 * (size_t)sum_d2 * cin);
            L.d1[l] = take(4 * (size_t)sum_d2 * cin);
            L.d2[l] = take(4 * (size_t)sum_d2 * cin);
            L.q1[l] = take(4 * (size_t)sum_d * cin);
            L.q3[l] = take(4 * (size_t)sum_d * cin);
            L.tot[l] = take(4 * (size_t)nodes * cin);
            L.d3[l] = take(4 * (size_t)nodes * cin);
        }
    }
    const int nf = f + Lv * h;
    L.feat = take(4 * (size_t)c->bs * nf);
    L.rpart = take(8 * (size_t)c->bs * RO_CH * nf);
    L.g0 = take(4 * (size_t)(sum_d > 0 ? sum_d : 1) * c->f_in);
    L.dsum = take(4 * (size_t)c->bs * nf);
    const int kmax = (c->order == 1 ? 2 : 18) * cmax;
    L.ppart = take(4 * (size_t)nodes * (h * kmax + h));
    L.dF[0] = take(4 * (size_t)rows * cmax);
    L.dF[1] = take(4 * (size_t)rows * cmax);
    if (c->order == 1) {
        L.dcoll = take(4 * (size_t)rows * 2 * cmax);
    } else {
        L.rdp = take(4 * (size_t)(sum_d > 0 ? sum_d : 1) * h);  // dp format: row sums and trace of dp
        L.trd = take(4 * (size_t)nodes * h);
        if (big) {  // C2Grad of the large-degree backward node pass
            L.g_sc = take(4 * (size_t)sum_d2 * cmax);
            L.g_sa = take(4 * (size_t)sum_d2 * cmax);
            L.g_d1 = take(4 * (size_t)sum_d2 * cmax);
            L.g_d2 = take(4 * (size_t)sum_d2 * cmax);
            L.g_d3 = take(4 * (size_t)nodes * cmax);
        }
    }
    L.xp = take(4 * (size_t)nodes * f);
    L.dxp = take(4 * (size_t)nodes * f);
    L.bytes = t;
    return L;
}

// One forward or backward call: the plan's view, the feature workspace and its layout, the stream
struct CcnRun {
    const hgnn_ccn_config* cfg;
    CcnPlanView v;
    const int* tot;   // device: the batch's node count
    int nodes;        // host: the node count, or its bound (grids)
    long long dmax;   // host: the largest degree, or its bound
    CcnFeatLayout L;
    void* ws;
    hipStream_t s;
    float* at(size_t off) const { return P<float>(ws, off); }
    C2Save save_of(int l) const {
        return C2Save{at(L.sc[l]), at(L.sa[l]), at(L.d1[l]), at(L.d2[l]), at(L.q1[l]), at(L.q3[l]), at(L.tot[l]),
                      at(L.d3[l])};
    }
    // degrees 65..256 present (or possible): their nodes go through the large-degree kernels
    bool bigd() const { return dmax > CCN_MAXD; }
};

CcnRun ccn_run(const hgnn_ccn_config* cfg, const long long* sums, void* plan_ws, long long max_sum_d2, void* workspace,
               void* stream) {
    const CcnPlanLayout Lp = plan_layout(cfg, max_sum_d2);
    return CcnRun{cfg, plan_view(cfg, Lp, plan_ws), P<int>(plan_ws, Lp.totals), (int)sums[2], sums[3],
                  feat_layout(cfg, sums), workspace, (hipStream_t)stream};
}

int ccn1_forward(const CcnRun& r, const float* Xp, const float* const* params) {
    const CcnFeatLayout& L = r.L;
    const int h = r.cfg->hidden, f = r.cfg->f_in;
    for (int l = 0; l < r.cfg->layers; ++l)
        TRY(launch_ccn1_fwd(r.v, r.tot, r.nodes, l == 0 ? nullptr : r.at(L.F[l - 1]), l == 0 ? 1 : 0, Xp,
                            l == 0 ? f : h, params[2 * l], params[2 * l + 1], h, r.at(L.coll[l]), r.at(L.F[l]), r.s));
    return HGNN_OK;
}

int ccn2_forward(const CcnRun& r, const float* Xp, const float* const* params) {
    const CcnFeatLayout& L = r.L;
    const int h = r.cfg->hidden, f = r.cfg->f_in;
    for (int l = 0; l < r.cfg->layers; ++l) {
        const int cin = l == 0 ? f : h, level0 = l == 0 ? 1 : 0;
        const float* fin = l == 0 ? nullptr : r.at(L.F[l - 1]);
        const float* w = params[2 * l];
        const float* b = params[2 * l + 1];
        TRY(launch_c2_fwd(r.v, r.tot, fin, level0, Xp, cin, w, b, h, r.dmax, r.nodes, r.at(L.F[l]), r.at(L.nsum[l]),
                          r.s));
        if (r.bigd())
            TRY(launch_c2_fwd_big(r.v, r.tot, r.nodes, fin, level0, Xp, cin, w, b, h, r.save_of(l), r.at(L.F[l]),
                                  r.at(L.nsum[l]), r.s));
    }
    return HGNN_OK;
}

// dsum: the readout's backward, [bs][nf]; every level adds its slice where its input gradient is formed
int ccn1_backward(const CcnRun& r, const float* const* params, float* const* grads, const float* dsum) {
    const CcnFeatLayout& L = r.L;
    const int h = r.cfg->hidden, f = r.cfg->f_in, Lv = r.cfg->layers;
    const int nf = f + Lv * h;
    float* dF = r.at(L.dF[0]);
    float* dFn = r.at(L.dF[1]);
    // dF of the top level = readout broadcast of its slice of dsum
    TRY(launch_ccn_bcast(r.v, r.tot, r.nodes, 1, dsum, nf, f + (Lv - 1) * h, h, dF, r.s));
    for (int l = Lv - 1; l >= 0; --l) {
        const int cin = l == 0 ? f : h, level0 = l == 0 ? 1 : 0;
        TRY(launch_ccn1_bwd_node(r.v, r.tot, r.nodes, dF, r.at(L.F[l]), r.at(L.coll[l]), cin, params[2 * l], h,
                                 r.at(L.dcoll), r.at(L.ppart), r.s));
        TRY(launch_ccn_param_reduce(r.at(L.ppart), r.tot, h * 2 * cin, h, grads[2 * l], grads[2 * l + 1], r.s));
        TRY(launch_ccn1_bwd_gather(r.v, r.tot, r.nodes, r.at(L.dcoll), cin, dsum, nf, level0 ? 0 : f + (l - 1) * h,
                                   level0, level0 ? r.at(L.dxp) : dFn, r.s));
        float* t = dF;
        dF = dFn;
        dFn = t;
    }
    return HGNN_OK;
}

int ccn2_backward(const CcnRun& r, const float* const* params, float* const* grads, const float* dsum) {
    const CcnFeatLayout& L = r.L;
    const int h = r.cfg->hidden, f = r.cfg->f_in, Lv = r.cfg->layers;
    const int nf = f + Lv * h;
    const bool bigd = r.bigd();
    float* dF = r.at(L.dF[0]);
    float* dFn = r.at(L.dF[1]);
    float* ppart = r.at(L.ppart);
    float* rdp = r.at(L.rdp);
    float* trd = r.at(L.trd);
    // without large-degree nodes the top level's backward reads the broadcast slice of dsum itself (dtop)
    if (bigd) TRY(launch_ccn_bcast(r.v, r.tot, r.nodes, 2, dsum, nf, f + (Lv - 1) * h, h, dF, r.s));
    for (int l = Lv - 1; l >= 0; --l) {
        const int cin = l == 0 ? f : h;
        const float* w = params[2 * l];
        const float* F = r.at(L.F[l]);
        float* g0 = l == 0 ? r.at(L.g0) : nullptr;
        if (bigd) {  // the large-degree nodes read the raw dF: before the dp rewrite
            const C2Grad gd{r.at(L.g_sc), r.at(L.g_sa), r.at(L.g_d1), r.at(L.g_d2), r.at(L.g_d3)};
            TRY(launch_c2_bwd_node_big(r.v, r.tot, r.nodes, dF, F, r.save_of(l), cin, w, h, gd, ppart, g0, r.s));
            TRY(launch_c2_dp_big(r.v, r.tot, r.nodes, dF, F, h, rdp, trd, r.s));
        }
        const float* dtop = !bigd && l == Lv - 1 ? dsum + f + (Lv - 1) * h : nullptr;
        TRY(launch_c2_bwd(r.v, r.tot, dF, dtop, nf, F, l == 0 ? nullptr : r.at(L.F[l - 1]), l == 0 ? 1 : 0,
                          r.at(L.xp), cin, w, h, r.dmax, r.nodes, rdp, trd, ppart, g0, r.s));
        TRY(launch_ccn_param_reduce(ppart, r.tot, h * 18 * cin, h, grads[2 * l], grads[2 * l + 1], r.s));
        if (l == 0) {
            TRY(launch_c2_dx0(r.v, r.tot, r.nodes, g0, cin, dsum, nf, r.at(L.dxp), r.s));
        } else {
            const C2Dp g{dF, rdp, trd};
            const int doff = f + (l - 1) * h;
            TRY(launch_c2_gather(r.v, r.tot, g, w, h, dsum, nf, doff, r.nodes, dFn, r.s));
            if (bigd) TRY(launch_c2_gather_big(r.v, r.tot, g, w, h, dsum, nf, doff, r.nodes, dFn, r.s));
        }
        float* t = dF;
        dF = dFn;
        dFn = t;
    }
    return HGNN_OK;
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

extern "C" {

size_t hgnn_ccn_workspace_bytes(const hgnn_ccn_config* cfg, const long long* sums) {
    if (!ccn_ok(cfg) || !sums) return 0;
    return feat_layout(cfg, sums).bytes;
}

int hgnn_ccn_forward(const hgnn_ccn_config* cfg, const long long* sums, const float* d_X, const float* const* params,
                     void* plan_ws, long long max_sum_d2, void* workspace, float* d_out, void* stream) {
    if (!ccn_ok(cfg) || !sums || !d_X || !params || !plan_ws || !workspace || !d_out) return HGNN_ERR_ARG;
    const CcnRun r = ccn_run(cfg, sums, plan_ws, max_sum_d2, workspace, stream);
    const CcnFeatLayout& L = r.L;
    float* Xp = r.at(L.xp);
    TRY(launch_ccn_pack_x(d_X, r.v.node_off, cfg->bs, cfg->nmax, cfg->f_in, Xp, r.s));
    TRY(cfg->order == 1 ? ccn1_forward(r, Xp, params) : ccn2_forward(r, Xp, params));
    ReadoutArgs ra{};
    ra.v = r.v;
    ra.order = cfg->order;
    ra.L = cfg->layers;
    ra.f = cfg->f_in;
    ra.h = cfg->hidden;
    ra.n_out = cfg->n_out;
    ra.bs = cfg->bs;
    ra.X = Xp;
    ra.per_node = cfg->order == 2;  // CCN-2D: the forward kernels left each node's row sum
    for (int l = 0; l < cfg->layers; ++l) ra.F[l] = r.at(cfg->order == 2 ? L.nsum[l] : L.F[l]);
    ra.fcw = params[2 * cfg->layers];
    ra.fcb = params[2 * cfg->layers + 1];
    ra.feat = r.at(L.feat);
    ra.out = d_out;
    return launch_ccn_readout(ra, cfg->order == 2 ? r.nodes : sums[0], P<double>(r.ws, L.rpart), r.s);
}

int hgnn_ccn_backward(const hgnn_ccn_config* cfg, const long long* sums, const float* const* params, void* plan_ws,
                      long long max_sum_d2, void* workspace, const float* d_dout, float* const* grads, float* d_dX,
                      void* stream) {
    if (!ccn_ok(cfg) || !sums || !params || !plan_ws || !workspace || !d_dout || !grads || !d_dX) return HGNN_ERR_ARG;
    const CcnRun r = ccn_run(cfg, sums, plan_ws, max_sum_d2, workspace, stream);
    const CcnFeatLayout& L = r.L;
    const int Lv = cfg->layers;
    const int nf = cfg->f_in + Lv * cfg->hidden;
    float* dsum = r.at(L.dsum);
    TRY(launch_ccn_readout_bwd(d_dout, r.at(L.feat), params[2 * Lv], cfg->bs, cfg->n_out, nf, dsum, grads[2 * Lv],
                               grads[2 * Lv + 1], r.s));
    TRY(cfg->order == 1 ? ccn1_backward(r, params, grads, dsum) : ccn2_backward(r, params, grads, dsum));
    return launch_ccn_unpack_dx(r.at(L.dxp), r.v.node_off, cfg->bs, cfg->nmax, cfg->f_in, d_dX, r.s);
}

}  // extern "C"
