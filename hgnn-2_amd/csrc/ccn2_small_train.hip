// CCN-2D on small graphs: the per-graph training loop in one dispatch (hgnn_ccn2_small_train*).
#include "ccn2_small.h"

namespace hgnn {
namespace {

// The per-graph training loop of scripts/train_ccn.py:31-73 in one dispatch, as k_ccn1_small_train (ccn_small.hip)
// does it for CCN-1D: ONE workgroup runs plan, forward, loss, backward and the optimizer step of graph 0, then of
// graph 1 on the weights graph 0 left, ...  The pieces are the stages k_ccn2_small_fwd and k_ccn2_small_bwd are made
// of (ccn2_small.h; the bs == 1 form: gradients written and reduced in the kernel), k_mse_loss's / xent_row's loss
// and optim_at.
// One graph region and one graph's ppart rows serve every graph (q_plan<true>: packed base 0); the readout
// features never leave LDS.
// Coherence: the block reads words it wrote itself earlier in the dispatch.  The parameter pointers it writes
// are plain float* (QTrain::p; QArgs' W / B / fcw / fcb alias them) and every read of a parameter is an
// agent-scope load (c2_ld<true>), so none can ride the scalar cache; the level, dp, rdp, trd and ppart rows are
// read at per-lane addresses (vector loads) behind the barriers the one-shot kernels already rely on, and a
// __threadfence() + barrier stands on both sides of the optimizer pass.
// Stages 1, 2 and 4 are the shared stage functions of ccn2_small.h, instantiated with FR = true (agent-scope
// parameter loads) -- except stage 4's level walk, which is q_backward's body written out (see there); the loss (3)
// and the optimizer (5) are this kernel's own.
constexpr size_t Q_TRAIN_STATIC = 4 * Q_OMAX + 8 * 8 + 64;  // sout, sred, sbad and alignment slack

struct QTrain {
    const float* y;       // (G, n_out) raw targets; XENT: (G,) class indices stored as float
    const float* clr;     // the scalars of the dispatch's k-th applied step at clr[k * cstride] (and + 1: Adam's
                          // second)
    float t_mean, t_div;  // yn = (y - mean) / div, div = std + 1e-8
    OptScalars h;         // the optimizer's fixed scalars (kernels.h)
    float* p[Q_TMAX];     // parameters, gradients (QArgs' gW / gB / gfcw / gfcb alias them) and optimizer state
    float* gr[Q_TMAX];
    float* m[Q_TMAX];
    float* u[Q_TMAX];     // SGD: not touched
    int numel[Q_TMAX];
    int nt;
    float* stats;         // [4] loss, mae and their RunningAverages
    int G;
    int cstride;          // 1: clr is (G,) lr / (1 - beta1^t); 2: the (G, 2) rows of hgnn_ccn2_small_train_opt
};

// OPT: the optimizer of stage 5 (HGNN_OPT_*), a template parameter like XENT, so the Adamax instantiations keep
// their instructions.
template <int CF, bool XENT, int OPT>
__global__ void __launch_bounds__(Q_NT) k_ccn2_small_train(QArgs a, QTrain t) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    __shared__ uint32_t sbad;
    __shared__ double sred[8];
    __shared__ float sout[Q_OMAX];  // out[g], then dout
    auto [g, w, sp, P] = q_carve(lds, a);  // P: forward P, backward dp
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int f = a.f, h = a.h, L = a.L, nf = f + L * h, n_out = a.n_out;
    float* G = a.gws;  // the one graph region
    const QRegion rg = q_region(a, G);
    float run_l = 0.f, run_m = 0.f;  // the RunningAverages (thread 0)
    int applied = 0;                 // optimizer steps taken so far in this dispatch
    if (threadIdx.x == 0) {
        run_l = t.stats[2];
        run_m = t.stats[3];
    }
    for (int gi = 0; gi < t.G; ++gi) {
        // 1. plan; the validation bits into the block's word
        if (threadIdx.x == 0) sbad = 0;
        uint32_t bad = 0;
        const int n = q_nodes(a, gi, bad);
        [[clang::always_inline]] bad |= q_plan<true>(a, gi, n, g);
        q_report(bad, sbad);
        // 2. forward on the current weights; the readout features stay in g.vec for the fc gradient; out[g] is what
        // the graph saw before its own update
        q_forward<CF, true>(a, g, w, sp, P, n, G);
        q_readout<true>(a, g, nf, sred, a.out + (long long)gi * n_out, sout);
        // a target that is no class index rejects the graph like a validation bit: set before the barrier the
        // read of sbad follows, so the branch below is block-uniform
        int ti = 0;
        if constexpr (XENT) {
            if (threadIdx.x == 0 && !xent_target(t.y[gi], n_out, ti)) atomicOr(&sbad, (uint32_t)ERR_CLASS_TARGET);
        }
        __syncthreads();
        const uint32_t gbad = sbad;
        __syncthreads();
        if (gbad) {  // a rejected graph: reported, no loss, no gradients, no step
            if (threadIdx.x == 0) a.err[0] = a.tag * 256 + (int)gbad;  // vector store (host-mapped word)
            continue;
        }
        // 3. loss, meters and dout; dout replaces out in sout
        if constexpr (XENT) {
            // k_xent_loss's arithmetic on one row (n = 1), by one thread in the row function's serial order;
            // stats[1] and stats[3] are never written (train_ccn.py:54-57)
            if (threadIdx.x == 0) {
                const float loss = (float)(double)xent_row(sout, ti, n_out, 1.0f, sout);
                run_l = run_l == 0.f ? loss : 0.9f * loss + 0.1f * run_l;
                t.stats[0] = loss;
                t.stats[2] = run_l;
            }
            __syncthreads();
        } else {
            // k_mse_loss's arithmetic on the normalised target
            double se = 0.0, ae = 0.0;
            if ((int)threadIdx.x < Q_RT)
                for (int i = threadIdx.x; i < n_out; i += Q_RT) {
                    const float yn = (t.y[(long long)gi * n_out + i] - t.t_mean) / t.t_div;
                    const float d = sout[i] - yn;
                    se += (double)d * d;
                    ae += fabs((double)d);
                    sout[i] = 2.0f * d / (float)n_out;
                }
            se = wave_sum_d(se);
            ae = wave_sum_d(ae);
            if (lane == 0 && wv < 4) {
                sred[wv] = se;
                sred[4 + wv] = ae;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                double S = 0.0, A = 0.0;
                for (int i = 0; i < Q_RT / 64; ++i) {
                    S += sred[i];
                    A += sred[4 + i];
                }
                const float loss = (float)(S / n_out), mae = (float)(A / n_out);
                run_l = run_l == 0.f ? loss : 0.9f * loss + 0.1f * run_l;
                run_m = run_m == 0.f ? mae : 0.9f * mae + 0.1f * run_m;
                t.stats[0] = loss;
                t.stats[1] = mae;
                t.stats[2] = run_l;
                t.stats[3] = run_m;
            }
        }
        // 4. backward, the one-graph form on the plan and levels of the forward: the fc gradients, dsum, then the
        // level walk with the parameter reduction.  No dX: the level-0 terms that feed only dX and its sum are left
        // out (q_node_bwd<.., DX = false>).
        // The fc gradients come first: they read the readout features where the forward left them, in g.vec (the
        // floats the one-shot forward stores to its feat row), before dsum takes that row.
        q_fc_grads(a, sout, g.vec, nf);
        __syncthreads();
        q_dsum<true>(a, g, sout, nf);
        __syncthreads();
        // The level walk is q_backward<CF, true, false>(.., reduce = true) written out: measured against the parent
        // commit's library, this kernel with the call was 0.8 to 0.9 % slower per graph on the classification arm of
        // tools/ab_ccn_train.py --order 2, at or beyond the parent's own min-max spread, and level with the parent
        // with the walk written here ("CCN-2D small-graph stages").  Keep the two in step.
        float* dcur = rg.dA;
        float* dnext = rg.dB;
        for (int l = L - 1; l >= 0; --l) {
            const int cin = l == 0 ? f : h;
            const int K = 18 * cin, stride = h * K + h;
            float* pl = a.ppart[l];
            const float* Fl = G + (long long)l * a.r2 * h;
            const float* fin = l == 0 ? nullptr : G + (long long)(l - 1) * a.r2 * h;
            const float* dtop = l == L - 1 ? g.vec + f + (L - 1) * h : nullptr;
            if (l == 0) c2_weights<Q_HC, CF, true>(reinterpret_cast<float(*)[Q_HC][CF]>(g.wc), a.W[l], cin, 0, h);
            else c2_weights<Q_HC, Q_HC, true>(reinterpret_cast<float(*)[Q_HC][Q_HC]>(g.wc), a.W[l], cin, 0, h);
            __syncthreads();
            for (int i = wv; i < n; i += Q_NW) {
                float* pp = pl + (long long)(g.base + i) * stride;
                if (l == 0)
                    [[clang::always_inline]] q_node_bwd<CF, 1, true, false>(a, g, w, sp, P, i, dcur, dtop, Fl, fin, cin,
                                                                            rg.rdp, rg.trd, pp, nullptr);
                else
                    [[clang::always_inline]] q_node_bwd<Q_HC, 8, false>(a, g, w, sp, P, i, dcur, dtop, Fl, fin, cin,
                                                                        rg.rdp, rg.trd, pp, nullptr);
            }
            __syncthreads();
            for (int k = wv; k < stride; k += Q_NW) {  // k_ccn_param_reduce's order over the graph's nodes
                double s = 0.0;
                if (lane < n) s += (double)pl[(long long)lane * stride + k];
                s = wave_sum_d(s);
                if (lane == 0) {
                    const double z = 0.0, tt = ((s + z) + z) + z;
                    if (k < h * K) a.gW[l][k] = (float)tt;
                    else a.gB[l][k - h * K] = (float)tt;
                }
            }
            if (l > 0)
                for (int j = wv; j < n; j += Q_NW)
                    [[clang::always_inline]] q_node_gather(a, g, w, sp, j, dcur, rg.rdp, rg.trd,
                                                           g.vec + f + (l - 1) * h, dnext);
            __syncthreads();
            float* x = dcur;
            dcur = dnext;
            dnext = x;
        }
        // 5. the optimizer over every parameter element, on the gradients other waves have just written: a tensor
        // per wave (tensors wv, wv + 8, ...), 64 elements at a time
        __threadfence();
        __syncthreads();
        const float* sc = t.clr + (long long)applied++ * t.cstride;
        const float clr = sc[0];
        float c1 = 0.f;
        if constexpr (OPT == HGNN_OPT_ADAM) c1 = sc[1];
        for (int k = uniform(wv); k < t.nt; k += Q_NW) {
            float* pk = t.p[k];
            float* mk = t.m[k];
            float* uk = t.u[k];
            const float* gk = t.gr[k];
            for (int q = lane; q < t.numel[k]; q += 64) optim_at<OPT>(pk, gk[q], mk, uk, q, clr, c1, t.h);
        }
        // 6. the new weights visible to the next graph's reads
        __threadfence();
        __syncthreads();
    }
}

}  // namespace

namespace {

// the training loop takes a model and an nmax, not a batch size: the one-graph form of the config
bool q_train_ok(const hgnn_ccn_config* c, hgnn_ccn_config& one) {
    if (!c) return false;
    one = *c;
    one.bs = 1;
    return ccn2_small_ok(&one) && one.n_out <= Q_OMAX && q_lds_bytes(one.nmax) + Q_TRAIN_STATIC <= Q_LDS_MAX;
}

// Every training entry: the argument checks and the launch; XENT picks the loss stage (and ignores the target
// statistics), OPT the optimizer stage; cstride is the row length of d_clr (1: the Adamax entries' step sizes, 2:
// the _opt entry's per-step pairs).
template <bool XENT, int OPT>
int q_train(const hgnn_ccn_config* cfg, const float* d_X, const float* d_adj, const int64_t* d_n_batch,
            const float* d_y, double t_mean, double t_std, float* const* params, float* const* grads,
            float* const* exp_avg, float* const* exp_inf, const float* d_clr, int cstride, double beta1, double beta2,
            double eps, double weight_decay, float* d_stats, float* d_out, void* d_ws, int32_t* d_err, int32_t tag,
            void* stream) {
    constexpr bool TWO = OPT != HGNN_OPT_SGD;  // whether the second state array is used
    hgnn_ccn_config one;
    if (!q_train_ok(cfg, one)) return HGNN_ERR_UNSUPPORTED;
    if (!d_X || !d_adj || !d_y || !params || !grads || !exp_avg || (TWO && !exp_inf) || !d_clr || !d_stats ||
        !d_out || !d_ws || !d_err || tag <= 0 || tag >= (1 << 23) || cfg->bs < 1 || cfg->bs > Q_TRAIN_GMAX ||
        (XENT && cfg->n_out < 2))
        return HGNN_ERR_ARG;
    const int nt = 2 * cfg->layers + 2;
    for (int k = 0; k < nt; ++k)
        if (!params[k] || !grads[k] || !exp_avg[k] || (TWO && !exp_inf[k])) return HGNN_ERR_ARG;
    // the one-graph layout of the workspace and of the backward (gradients written directly); the kernel reads
    // graph g's data at index g
    QArgs a = q_args(&one, d_X, d_adj, d_n_batch, params, d_ws, q_layout(&one, 1));
    a.out = d_out;
    a.err = d_err;
    a.tag = tag;
    q_set_grads(a, grads, cfg->layers);
    QTrain t{};
    t.y = d_y;
    t.clr = d_clr;
    t.cstride = cstride;
    // scalars combine in double and reach the kernel as fp32, as the reference's Python floats reach torch
    t.t_mean = (float)t_mean;
    t.t_div = (float)(t_std + 1e-8);  // scripts/train_ccn.py:42
    t.h = opt_scalars(OPT, beta1, beta2, eps, weight_decay);
    const int nf = q_nf(cfg);
    for (int k = 0; k < nt; ++k) {
        t.p[k] = params[k];
        t.gr[k] = grads[k];
        t.m[k] = exp_avg[k];
        t.u[k] = TWO ? exp_inf[k] : nullptr;
        const int l = k / 2;
        if (l < cfg->layers) t.numel[k] = k % 2 ? cfg->hidden : cfg->hidden * 18 * (l == 0 ? cfg->f_in : cfg->hidden);
        else t.numel[k] = k % 2 ? cfg->n_out : cfg->n_out * nf;
    }
    t.nt = nt;
    t.stats = d_stats;
    t.G = cfg->bs;
    static bool attr = false;
    q_lds_attr(&k_ccn2_small_train<Q_CF, XENT, OPT>, attr, Q_TRAIN_STATIC);
    HGNN_KLAUNCH((k_ccn2_small_train<Q_CF, XENT, OPT>), dim3(1), dim3(Q_NT), q_lds_bytes(one.nmax), (hipStream_t)stream, a,
                 t);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

extern "C" {

int hgnn_ccn2_small_train_supported(const hgnn_ccn_config* cfg) {
    hgnn_ccn_config one;
    return q_train_ok(cfg, one) ? 1 : 0;
}

size_t hgnn_ccn2_small_train_workspace_bytes(const hgnn_ccn_config* cfg) {
    hgnn_ccn_config one;
    return q_train_ok(cfg, one) ? ccn2_small_workspace_bytes(&one) : 0;
}

int hgnn_ccn2_small_train(const hgnn_ccn_config* cfg, const float* d_X, const float* d_adj, const int64_t* d_n_batch,
                          const float* d_y, double t_mean, double t_std, float* const* params, float* const* grads,
                          float* const* exp_avg, float* const* exp_inf, const float* d_clr, double beta1,
                          double beta2, double eps, double weight_decay, float* d_stats, float* d_out,
                          void* workspace, int32_t* d_err, int32_t tag, void* stream) {
    return q_train<false, HGNN_OPT_ADAMAX>(cfg, d_X, d_adj, d_n_batch, d_y, t_mean, t_std, params, grads, exp_avg,
                                           exp_inf, d_clr, 1, beta1, beta2, eps, weight_decay, d_stats, d_out,
                                           workspace, d_err, tag, stream);
}

int hgnn_ccn2_small_train_xent(const hgnn_ccn_config* cfg, const float* d_X, const float* d_adj,
                               const int64_t* d_n_batch, const float* d_y, float* const* params, float* const* grads,
                               float* const* exp_avg, float* const* exp_inf, const float* d_clr, double beta1,
                               double beta2, double eps, double weight_decay, float* d_stats, float* d_out,
                               void* workspace, int32_t* d_err, int32_t tag, void* stream) {
    return q_train<true, HGNN_OPT_ADAMAX>(cfg, d_X, d_adj, d_n_batch, d_y, 0.0, 1.0, params, grads, exp_avg, exp_inf,
                                          d_clr, 1, beta1, beta2, eps, weight_decay, d_stats, d_out, workspace, d_err,
                                          tag, stream);
}

int hgnn_ccn2_small_train_opt(const hgnn_ccn_config* cfg, int kind, int xent, const float* d_X, const float* d_adj,
                              const int64_t* d_n_batch, const float* d_y, double t_mean, double t_std,
                              float* const* params, float* const* grads, float* const* state1, float* const* state2,
                              const float* d_steps, double beta1_or_momentum, double beta2, double eps,
                              double weight_decay, float* d_stats, float* d_out, void* workspace, int32_t* d_err,
                              int32_t tag, void* stream) {
    hgnn_ccn_config one;
    if (!q_train_ok(cfg, one)) return HGNN_ERR_UNSUPPORTED;
    return opt_dispatch(kind, xent, [&](auto X, auto O) {
        return q_train<X(), O()>(cfg, d_X, d_adj, d_n_batch, d_y, X() ? 0.0 : t_mean, X() ? 1.0 : t_std, params, grads,
                                 state1, state2, d_steps, 2, beta1_or_momentum, beta2, eps, weight_decay, d_stats,
                                 d_out, workspace, d_err, tag, stream);
    });
}

}  // extern "C"
