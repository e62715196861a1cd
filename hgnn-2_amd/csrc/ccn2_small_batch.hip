// CCN-2D mini-batch training on small graphs: one optimizer step per mini-batch of B graphs, the B graphs in
// parallel, everything on the device (hgnn_ccn2_small_train_batch).  The CCN-2D counterpart of ccn_small_batch.hip.
//
// The per-graph loop (ccn2_small_train.hip k_ccn2_small_train) is sequential by definition, so one workgroup walks
// the list.  A mini-batch's B graphs see the same weights; from the library's pieces it costs five dispatches, two
// plans, the level-0 terms that feed only dX and a feat / dout round trip through torch.  Here: two dispatches per
// mini-batch, ordered by the stream and by nothing else (no grid barrier, no block waits for another):
//   1. k_ccn2_small_batch   one workgroup per graph: stages 1 to 4 of k_ccn2_small_train for that graph in the batch
//      layout (q_plan<false>: the packed base is the prefix of n_batch within the mini-batch; every level in the
//      graph's own region), the fp64 readout, out, the graph's own dout row, the backward walk without dX.  One plan
//      serves forward and backward.  It leaves the node partials, the readout features and the dout row in the
//      workspace.  The weights do not change inside the dispatch, so every parameter read is a plain load.
//   2. k_ccn2_small_apply   k_ccn2_small_reduce's sums (one block per level-parameter element over the mini-batch's
//      packed nodes, one wave per fc element over its graphs), the gradient, then the optimizer's update of that
//      element by the thread that holds the sum; one more block writes the meters.
// A graph with validation bits (or a class target that is no index) ORs them into the mini-batch's reject word;
// the apply kernel reads that word first and does nothing when it is set.
// The arithmetic is that of the library's own pieces on the mini-batch -- hgnn_ccn_small_forward, hgnn_mse_loss /
// hgnn_xent_loss, hgnn_ccn_small_backward, hgnn_optim_step -- bit for bit: the stages and the per-element sums are
// the one-shot kernels' own (ccn2_small.h: q_forward, q_readout, q_dsum, q_backward, q_sum_level_elem,
// q_sum_fc_elem), the loss rows and optimizer elements are kernels.h's.
#include "ccn2_small.h"

namespace hgnn {
namespace {

constexpr size_t QB_STATIC = 4 * Q_OMAX + 8 * 4 + 64;  // sout, sred, sbad and alignment slack

// One mini-batch: what both kernels need besides QArgs (whose X / adj / n_batch / out point at the mini-batch's
// first graph and whose bs is the mini-batch's size; feat / ppart / gws are the workspace regions).
struct QbBatch {
    const float* y;       // raw targets of the mini-batch: (B, n_out), classification: (B,) class indices
    float t_mean, t_div;  // yn = (y - mean) / div, div = std + 1e-8
    int B;                // graphs of this mini-batch: the divisor of its loss
    float* dout;          // [B][n_out] workspace region
    uint32_t* reject;     // the mini-batch's reject word (cleared by the entry)
};

struct QbApply {
    const float* steps;  // the mini-batch's two per-step scalars (hgnn_ccn2_small_train_opt's row)
    OptScalars h;
    float* p[Q_TMAX];
    float* m[Q_TMAX];
    float* u[Q_TMAX];    // SGD: not touched
    float* stats;        // [4] loss, mae and their RunningAverages
};

// Stages 1, 2 and 4 are the shared stage functions of ccn2_small.h (FR = false: plain parameter loads); the dout
// row (3) is this kernel's own.
template <int CF, bool XENT>
__global__ void __launch_bounds__(Q_NT) k_ccn2_small_batch(QArgs a, QbBatch t) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    __shared__ uint32_t sbad;
    __shared__ double sred[4];
    __shared__ float sout[Q_OMAX];  // out[b], then dout[b]
    auto [g, w, sp, P] = q_carve(lds, a);  // P: forward P, backward dp
    const int b = blockIdx.x;
    const int nf = a.f + a.L * a.h, n_out = a.n_out;
    float* G = a.gws + (long long)b * a.gstride;  // the graph's own region
    // 1. plan; the validation bits into the block's word
    if (threadIdx.x == 0) sbad = 0;
    uint32_t bad = 0;
    const int n = q_nodes(a, b, bad);
    [[clang::always_inline]] bad |= q_plan<false>(a, b, n, g);
    q_report(bad, sbad);
    // 2. forward, every level kept in the graph's region; out[b]; the readout features stay in g.vec
    q_forward<CF, false>(a, g, w, sp, P, n, G);
    q_readout<false>(a, g, nf, sred, a.out + (long long)b * n_out, sout);
    // a target that is no class index rejects the graph like a validation bit: set before the barrier the read
    // of sbad follows, so the branch below is block-uniform
    int ti = 0;
    if constexpr (XENT) {
        if (threadIdx.x == 0 && !xent_target(t.y[b], n_out, ti)) atomicOr(&sbad, (uint32_t)ERR_CLASS_TARGET);
    }
    __syncthreads();
    const uint32_t gbad = sbad;
    if (gbad) {  // a rejected graph: its out row, the mini-batch's reject word, the error word -- nothing else
        if (threadIdx.x == 0) {
            atomicOr(t.reject, gbad);
            a.err[0] = a.tag * 256 + (int)gbad;  // vector store (host-mapped word)
        }
        return;
    }
    // 3. the graph's dout row (elementwise, so local to the block); dout replaces out in sout
    if constexpr (XENT) {
        // k_xent_loss's row with n = B, by one thread in the row function's serial order
        if (threadIdx.x == 0) (void)xent_row(sout, ti, n_out, 1.0f / (float)t.B, sout);
    } else {
        // mse_block's elements on the normalised target, n = B n_out
        const int nel = t.B * n_out;
        for (int i = threadIdx.x; i < n_out; i += Q_NT) {
            float yn = t.y[(long long)b * n_out + i] - t.t_mean;
            yn = yn / t.t_div;
            const float d = sout[i] - yn;
            sout[i] = 2.0f * d / (float)nel;
        }
    }
    __syncthreads();
    // the readout features and the row for the apply kernel's fc gradients, before dsum replaces the features
    const float* dob = sout;
    for (int k = threadIdx.x; k < nf; k += Q_NT) a.feat[(long long)b * nf + k] = g.vec[k];
    for (int i = threadIdx.x; i < n_out; i += Q_NT) t.dout[(long long)b * n_out + i] = dob[i];
    __syncthreads();
    // 4. backward, the batch form on the plan and levels of the forward: dsum, then the level walk (partials at the
    // packed node index).  No dX: the level-0 terms that feed only dX and its sum are left out (DX = false); no
    // parameter reduction: the apply kernel sums over the nodes.
    q_dsum<false>(a, g, dob, nf);
    __syncthreads();
    q_backward<CF, false, false>(a, g, w, sp, P, b, n, G, q_region(a, G), false);
}

// k_ccn2_small_reduce's sums over one mini-batch, each followed by the optimizer's update of its element.  Blocks
// [0, np): one per level-parameter element over the packed nodes; the next nfc blocks: one wave per fc element over
// the graphs; the last block: the meters.
template <int OPT, bool XENT>
__global__ void __launch_bounds__(256) k_ccn2_small_apply(QArgs a, QbBatch t, QbApply q, int np, int nfc) {
    // a rejected mini-batch: no gradients, no meters, no step (block-uniform: every block reads the word first)
    if (*t.reject != 0u) return;
    __shared__ double red[4];
    __shared__ int s_tot;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int L = a.L, nf = a.f + L * a.h, n_out = a.n_out, B = t.B;
    float c1 = 0.f;
    if constexpr (OPT == HGNN_OPT_ADAM) c1 = q.steps[1];
    if ((int)blockIdx.x < np) {
        int k = blockIdx.x, l, K;
        q_level_elem(a, k, l, K);
        const double tt = q_sum_level_elem(a, B, l, k, a.h * K + a.h, red, s_tot);
        if (threadIdx.x == 0) {
            const float gv = (float)tt;
            if (k < a.h * K) {
                a.gW[l][k] = gv;
                optim_at<OPT>(q.p[2 * l], gv, q.m[2 * l], q.u[2 * l], k, q.steps[0], c1, q.h);
            } else {
                const int e = k - a.h * K;
                a.gB[l][e] = gv;
                optim_at<OPT>(q.p[2 * l + 1], gv, q.m[2 * l + 1], q.u[2 * l + 1], e, q.steps[0], c1, q.h);
            }
        }
        return;
    }
    if ((int)blockIdx.x < np + nfc) {
        const int e = ((int)blockIdx.x - np) * 4 + wv;
        if (e >= n_out * nf + n_out) return;
        const double s = q_sum_fc_elem(a, t.dout, B, e, nf);
        if (lane != 0) return;
        const float gv = (float)s;
        if (e < n_out * nf) {
            a.gfcw[e] = gv;
            optim_at<OPT>(q.p[2 * L], gv, q.m[2 * L], q.u[2 * L], e, q.steps[0], c1, q.h);
        } else {
            const int o = e - n_out * nf;
            a.gfcb[o] = gv;
            optim_at<OPT>(q.p[2 * L + 1], gv, q.m[2 * L + 1], q.u[2 * L + 1], o, q.steps[0], c1, q.h);
        }
        return;
    }
    // the meters of the mini-batch
    if constexpr (XENT) {
        // k_xent_loss's mean of the row losses, in its order
        double se = 0.0;
        for (int i = threadIdx.x; i < B; i += 256) {
            int ti;
            (void)xent_target(t.y[i], n_out, ti);  // valid: the batch kernel rejected the mini-batch otherwise
            se += (double)xent_row(a.out + (long long)i * n_out, ti, n_out, 1.0f / (float)B, nullptr);
        }
        se = wave_sum_d(se);
        if (lane == 0) red[wv] = se;
        __syncthreads();
        if (threadIdx.x == 0) {
            const float loss = (float)((red[0] + red[1] + red[2] + red[3]) / B);
            q.stats[0] = loss;
            q.stats[2] = q.stats[2] == 0.f ? loss : 0.9f * loss + 0.1f * q.stats[2];
        }
    } else {
        // hgnn_mse_loss's bits for the normalised target: the same subtraction and division, then the block sums
        float loss, mae;
        mse_block(a.out, t.y, B * n_out, t.t_mean, t.t_div, nullptr, loss, mae);
        if (threadIdx.x == 0) {
            q.stats[0] = loss;
            q.stats[1] = mae;
            q.stats[2] = q.stats[2] == 0.f ? loss : 0.9f * loss + 0.1f * q.stats[2];
            q.stats[3] = q.stats[3] == 0.f ? mae : 0.9f * mae + 0.1f * q.stats[3];
        }
    }
}

// Workspace: the reject words first (cfg->bs of them reserved, so the size never shrinks as `batch` grows and a
// workspace sized for (bs, batch) serves every call with no more graphs and no larger mini-batches; a call uses and
// clears the first ceil(bs / batch)), then one mini-batch's regions, each 256-byte aligned and reused by successive
// mini-batches: feat [B][nf], dout [B][n_out], per level ppart [B nmax][prow_l], B graph regions of q_gstride floats.
QLayout qb_layout(const hgnn_ccn_config* c, int batch) {
    return q_layout(c, batch, q_al256(4 * (size_t)c->bs), 4 * (size_t)batch * c->n_out);  // .extra: dout
}

template <bool XENT, int OPT>
int qb_train(const hgnn_ccn_config* cfg, int batch, const float* d_X, const float* d_adj, const int64_t* d_n_batch,
             const float* d_y, double t_mean, double t_std, float* const* params, float* const* grads,
             float* const* state1, float* const* state2, const float* d_steps, double beta1_or_momentum,
             double beta2, double eps, double weight_decay, float* d_stats, float* d_out, void* workspace,
             int32_t* d_err, int32_t tag, hipStream_t s) {
    constexpr bool TWO = OPT != HGNN_OPT_SGD;  // whether the second state array is used
    const int L = cfg->layers, nt = 2 * L + 2, G = cfg->bs;
    if (TWO && !state2) return HGNN_ERR_ARG;
    for (int k = 0; k < nt; ++k)
        if (!params[k] || !grads[k] || !state1[k] || (TWO && !state2[k])) return HGNN_ERR_ARG;
    const QLayout lay = qb_layout(cfg, batch);
    char* ws = static_cast<char*>(workspace);
    QArgs a = q_args(cfg, d_X, d_adj, d_n_batch, params, workspace, lay);
    q_set_grads(a, grads, L);
    a.err = d_err;
    a.tag = tag;
    QbBatch t{};
    // scalars combine in double and reach the kernels as fp32, as the reference's Python floats reach torch
    t.t_mean = (float)t_mean;
    t.t_div = (float)(t_std + 1e-8);  // scripts/train_ccn.py:42
    t.dout = reinterpret_cast<float*>(ws + lay.extra);
    QbApply q{};
    q.h = opt_scalars(OPT, beta1_or_momentum, beta2, eps, weight_decay);
    for (int k = 0; k < nt; ++k) {
        q.p[k] = params[k];
        q.m[k] = state1[k];
        q.u[k] = TWO ? state2[k] : nullptr;
    }
    q.stats = d_stats;
    const int K = (G + batch - 1) / batch;
    uint32_t* reject = reinterpret_cast<uint32_t*>(ws);
    HGNN_HOST_CHECK(hipMemsetAsync(reject, 0, 4 * (size_t)K, s));
    static bool attr = false;
    q_lds_attr(&k_ccn2_small_batch<Q_CF, XENT>, attr, QB_STATIC);
    const size_t lds = q_lds_bytes(cfg->nmax);
    const int np = q_np(cfg), nfc = q_nfc(cfg);
    for (int k = 0; k < K; ++k) {
        const long long g0 = (long long)k * batch;
        const int B = (int)(G - g0 < batch ? G - g0 : batch);  // the last mini-batch may be shorter
        a.bs = B;
        a.X = d_X + g0 * a.nmax * a.f;
        a.adj = d_adj + g0 * a.nmax * a.nmax;
        a.n_batch = d_n_batch ? d_n_batch + g0 : nullptr;
        a.out = d_out + g0 * a.n_out;
        t.y = d_y + (XENT ? g0 : g0 * a.n_out);
        t.B = B;
        t.reject = reject + k;
        q.steps = d_steps + 2 * (long long)k;  // row k is mini-batch k's, applied or not
        HGNN_KLAUNCH((k_ccn2_small_batch<Q_CF, XENT>), dim3(B), dim3(Q_NT), lds, s, a, t);
        HGNN_LAUNCH_CHECK();
        HGNN_KLAUNCH((k_ccn2_small_apply<OPT, XENT>), dim3(np + nfc + 1), dim3(256), 0, s, a, t, q, np, nfc);
        HGNN_LAUNCH_CHECK();
    }
    return HGNN_OK;
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

extern "C" {

int hgnn_ccn2_small_train_batch_supported(const hgnn_ccn_config* cfg) {
    return cfg && hgnn_ccn2_small_train_supported(cfg) ? 1 : 0;
}

size_t hgnn_ccn2_small_train_batch_workspace_bytes(const hgnn_ccn_config* cfg, int batch) {
    if (!hgnn_ccn2_small_train_batch_supported(cfg) || batch < 1 || cfg->bs < 1 || cfg->bs > Q_TRAIN_GMAX) return 0;
    return qb_layout(cfg, batch).total;
}

int hgnn_ccn2_small_train_batch(const hgnn_ccn_config* cfg, int batch, int kind, int xent, const float* d_X,
                                const float* d_adj, const int64_t* d_n_batch, const float* d_y, double t_mean,
                                double t_std, float* const* params, float* const* grads, float* const* state1,
                                float* const* state2, const float* d_steps, double beta1_or_momentum, double beta2,
                                double eps, double weight_decay, float* d_stats, float* d_out, void* workspace,
                                int32_t* d_err, int32_t tag, void* stream) {
    if (!hgnn_ccn2_small_train_batch_supported(cfg)) return HGNN_ERR_UNSUPPORTED;
    if (!d_X || !d_adj || !d_y || !params || !grads || !state1 || !d_steps || !d_stats || !d_out || !workspace ||
        !d_err || tag <= 0 || tag >= (1 << 23) || batch < 1 || cfg->bs < 1 || cfg->bs > Q_TRAIN_GMAX ||
        (xent && cfg->n_out < 2))
        return HGNN_ERR_ARG;
    // the meters come from mse_block, which leaves the division out below its own threshold (normalize_data's
    // rule); the CCN rule always divides, so such a divisor is refused rather than silently treated differently
    if (!xent && (float)(t_std + 1e-8) < 1e-5f) return HGNN_ERR_ARG;
    return opt_dispatch(kind, xent, [&](auto X, auto O) {
        return qb_train<X(), O()>(cfg, batch, d_X, d_adj, d_n_batch, d_y, X() ? 0.0 : t_mean, X() ? 1.0 : t_std, params,
                                  grads, state1, state2, d_steps, beta1_or_momentum, beta2, eps, weight_decay, d_stats,
                                  d_out, workspace, d_err, tag, (hipStream_t)stream);
    });
}

}  // extern "C"
