// CCN-1D mini-batch training on small graphs: one optimizer step per mini-batch of B graphs, the B graphs in
// parallel, everything on the device (hgnn_ccn_small_train_batch).
//
// The per-graph loop (ccn_small.hip k_ccn1_small_train) is sequential by definition -- graph g + 1 reads the weights
// graph g wrote -- so one workgroup walks the list and the rest of the device idles.  A mini-batch has no such
// dependence: its B graphs see the same weights, the loss is nn.MSELoss / nn.CrossEntropyLoss over the (B, n_out)
// block, the parameter gradients are summed over the graphs and one step follows.  Two dispatches per mini-batch,
// ordered by the stream and by nothing else (no grid barrier, no block waits for another):
//   1. k_ccn1_small_batch   one workgroup per graph: stages 1 to 4 of k_ccn1_small_train for that graph (stage and
//      plan, every level kept in LDS, the fp64 readout sums, out, the graph's own dout row, the backward walk in its
//      batch form).  Plan and levels are built once for forward and backward.  It leaves the level partials, the
//      readout features and the dout row in the workspace.
//   2. k_ccn1_small_apply   one wave per parameter element: k_ccn1_small_reduce's fp64 sum over the B graphs, the
//      gradient, then the optimizer's element update (all three optimizers are elementwise); block 0 also writes
//      the meters.
// A graph with validation bits (or a class target that is no index) ORs them into the mini-batch's reject word;
// the apply kernel reads that word first and does nothing when it is set.
// The arithmetic is that of the library's own pieces on the mini-batch -- hgnn_ccn_small_forward, hgnn_mse_loss /
// hgnn_xent_loss, hgnn_ccn_small_backward, hgnn_optim_step -- bit for bit: the device functions are shared
// (ccn_small.h, kernels.h) and the sums run in the same order.  k_ccn1_small_apply lives here, behind cb_launch_apply,
// for the LDS and the SPILL form.
#include "ccn_small_batch_kernels.h"

using namespace hgnn;

namespace {

// One wave per parameter element (the level entries, then fc weight and bias from dout and the readout features):
// k_ccn1_small_reduce's sum over the mini-batch's graphs, the gradient, the optimizer's update of that element.
template <int OPT, bool XENT>
__global__ void __launch_bounds__(256) k_ccn1_small_apply(CsArgs a, CbBatch t, CbApply q) {
    // a rejected mini-batch: no gradients, no meters, no step (block-uniform: every block reads the word first)
    if (*t.reject != 0u) return;
    const int nf = a.f + a.L * a.h, n_out = a.n_out, B = t.B;
    if (blockIdx.x == 0) {  // the meters of the mini-batch
        if constexpr (XENT) {
            // k_xent_loss's mean of the row losses, in its order
            __shared__ double red[4];
            double se = 0.0;
            for (int i = threadIdx.x; i < B; i += 256) {
                int ti;
                (void)xent_target(t.y[i], n_out, ti);  // valid: the batch kernel rejected the mini-batch otherwise
                se += (double)xent_row(a.out + (long long)i * n_out, ti, n_out, 1.0f / (float)B, nullptr);
            }
            se = wave_sum_d(se);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = se;
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
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int nw = cs_woff(a.L, a.f, a.h);
    if (w >= nw + n_out * nf + n_out) return;
    const float g = (float)cs_sum_elem(a, t.dout, B, w);
    if ((threadIdx.x & 63) != 0) return;
    int ti, e;
    cs_param_elem(a, nw, n_out * nf, w, ti, e);
    cs_grad(a, ti)[e] = g;
    float c1 = 0.f;
    if constexpr (OPT == HGNN_OPT_ADAM) c1 = q.steps[1];
    optim_at<OPT>(q.p[ti], g, q.m[ti], q.u[ti], e, q.steps[0], c1, q.h);
}

}  // namespace

template <int OPT, bool XENT>
int hgnn::cb_launch_apply(const CsArgs& a, const CbBatch& t, const CbApply& q, int outs, hipStream_t s) {
    HGNN_KLAUNCH((k_ccn1_small_apply<OPT, XENT>), dim3((outs + 3) / 4), dim3(256), 0, s, a, t, q);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}
#define CB_APPLY(OPT)                                                                                             \
    template int hgnn::cb_launch_apply<OPT, false>(const CsArgs&, const CbBatch&, const CbApply&, int, hipStream_t); \
    template int hgnn::cb_launch_apply<OPT, true>(const CsArgs&, const CbBatch&, const CbApply&, int, hipStream_t);
CB_APPLY(HGNN_OPT_ADAMAX)
CB_APPLY(HGNN_OPT_SGD)
CB_APPLY(HGNN_OPT_ADAM)
#undef CB_APPLY

extern "C" {

int hgnn_ccn_small_train_batch_supported(const hgnn_ccn_config* cfg) {
    return cfg && cfg->order == 1 && hgnn_ccn_small_train_supported(cfg) ? 1 : 0;
}

size_t hgnn_ccn_small_train_batch_workspace_bytes(const hgnn_ccn_config* cfg, int batch) {
    if (!hgnn_ccn_small_train_batch_supported(cfg) || batch < 1 || cfg->bs < 1 || cfg->bs > CS_TRAIN_GMAX) return 0;
    return cb_layout(cfg, batch).total;
}

int hgnn_ccn_small_train_batch(const hgnn_ccn_config* cfg, int batch, int kind, int xent, const float* d_X,
                               const float* d_adj, const int64_t* d_n_batch, const float* d_y, double t_mean,
                               double t_std, float* const* params, float* const* grads, float* const* state1,
                               float* const* state2, const float* d_steps, double beta1_or_momentum, double beta2,
                               double eps, double weight_decay, float* d_stats, float* d_out, void* workspace,
                               int32_t* d_err, int32_t tag, void* stream) {
    if (!hgnn_ccn_small_train_batch_supported(cfg)) return HGNN_ERR_UNSUPPORTED;
    if (!d_X || !d_adj || !d_y || !params || !grads || !state1 || !d_steps || !d_stats || !d_out || !workspace ||
        !d_err || tag <= 0 || tag >= (1 << 23) || batch < 1 || cfg->bs < 1 || cfg->bs > CS_TRAIN_GMAX ||
        (xent && cfg->n_out < 2))
        return HGNN_ERR_ARG;
    // the meters come from mse_block, which leaves the division out below its own threshold (normalize_data's
    // rule); the CCN rule always divides, so such a divisor is refused rather than silently treated differently
    if (!xent && (float)(t_std + 1e-8) < 1e-5f) return HGNN_ERR_ARG;
    return opt_dispatch(kind, xent, [&](auto X, auto O) {
        return cb_train<X(), O()>(cfg, batch, d_X, d_adj, d_n_batch, d_y, X() ? 0.0 : t_mean, X() ? 1.0 : t_std, params,
                                  grads, state1, state2, d_steps, beta1_or_momentum, beta2, eps, weight_decay, d_stats,
                                  d_out, workspace, d_err, tag, (hipStream_t)stream);
    });
}

}  // extern "C"
