// CCN-1D on small graphs (n <= 64 nodes): one workgroup per graph, the whole call in LDS.
//
// The reference's driver calls the network one graph at a time (scripts/train_ccn.py:31-73: net(X, A + I),
// loss, backward and an optimizer step per graph), and QM9 graphs have at most 29 nodes: there the general
// path (ccn*.hip) spends the call on dispatches, not arithmetic (5 plan + 5 forward + 9 backward launches,
// ~0.18 ms of GPU time and more of host time per graph).  Here one workgroup per graph
//   * builds the receptive fields in LDS: row bit sets over the graph's nodes (utils_ccn.py:195-199,
//     nbr_i = ascending nonzero(adj[i])), degrees, row offsets, and reads every chi position by popcount
//     (index of u in N(j) = bits below u in j's row, utils_ccn.py:66-106),
//   * runs every level (promotion + the two contractions + Linear + ReLU, utils_ccn.py:281-324) and the
//     readout (model_ccn.py:50-64) -- forward: one dispatch,
//   * backward: rebuilds the plan and the levels in LDS, then walks them back (one dispatch for one
//     graph; a batch adds one reduction of the per-graph parameter partials),
//   * training (k_ccn1_small_train): ONE workgroup runs the reference's whole per-graph loop -- forward, loss,
//     backward, Adamax, then the next graph on the new weights -- in one dispatch.
// Per level the arithmetic is the one-chunk path of k_ccn1_fwd / k_ccn1_bwd_node / k_ccn1_bwd_gather in
// the same order, so forward values and input gradients are those of the general path; the weight
// gradients are summed per lane over a wave's nodes, then over lanes and waves (fp32), where the general
// path sums per node and then over nodes in fp64.
// The stages (cs_*) are in ccn_small.h, which ccn_small_batch.hip (the mini-batch training step) shares; the kernels
// are the SPILL = false instantiations of ccn_small_kernels.h (ccn_small_spill.hip has the other form: the row-sized
// arrays in a global workspace, for graphs the LDS layout does not hold).  k_ccn1_small_reduce lives here, behind
// cs_launch_reduce, for both forms.
#include "ccn_small_kernels.h"

using namespace hgnn;

namespace {

// Batches: parameter gradient = sum over graphs in fp64, one wave per entry (the level entries, then fc
// weight and bias from dout and the readout features, k_ccn_readout_bwd's order).
__global__ void __launch_bounds__(256) k_ccn1_small_reduce(CsArgs a) {
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int nw = cs_woff(a.L, a.f, a.h), nfc = a.n_out * (a.f + a.L * a.h);
    if (w >= nw + nfc + a.n_out) return;
    const double s = cs_sum_elem(a, a.dout, a.bs, w);
    if ((threadIdx.x & 63) != 0) return;
    int ti, q;
    cs_param_elem(a, nw, nfc, w, ti, q);
    cs_grad(a, ti)[q] = (float)s;
}

}  // namespace

int hgnn::cs_launch_reduce(const hgnn_ccn_config* cfg, const CsArgs& a, hipStream_t s) {
    HGNN_KLAUNCH(k_ccn1_small_reduce, dim3((cs_nouts(cfg) + 3) / 4), dim3(256), 0, s, a);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

extern "C" {

int hgnn_ccn_small_supported(const hgnn_ccn_config* cfg) {
    if (cfg && cfg->order == 2) return ccn2_small_ok(cfg) ? 1 : 0;
    return cs_ok(cfg) ? 1 : 0;
}

int hgnn_host_word_alloc(void** host_ptr, void** dev_ptr) {
    if (!host_ptr || !dev_ptr) return HGNN_ERR_ARG;
    void* h = nullptr;
    HGNN_HOST_CHECK(hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocCoherent));
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
        (void)hipHostFree(h);
        return HGNN_ERR_HIP;
    }
    static_cast<int32_t*>(h)[0] = 0;
    *host_ptr = h;
    *dev_ptr = d;
    return HGNN_OK;
}

size_t hgnn_ccn_small_workspace_bytes(const hgnn_ccn_config* cfg) {
    if (cfg && cfg->order == 2) return ccn2_small_workspace_bytes(cfg);
    if (!cs_ok(cfg)) return 0;
    return cs_head_bytes(cfg);
}

int hgnn_ccn_small_forward(const hgnn_ccn_config* cfg, const float* d_X, const float* d_adj,
                           const int64_t* d_n_batch, const float* const* params, void* workspace, int32_t* d_err,
                           int32_t tag, float* d_out, void* stream) {
    const bool two = cfg && cfg->order == 2;
    if (two ? !ccn2_small_ok(cfg) : !cs_ok(cfg)) return HGNN_ERR_UNSUPPORTED;
    if (!d_X || !d_adj || !params || !workspace || !d_err || !d_out || tag <= 0 || tag >= (1 << 23))
        return HGNN_ERR_ARG;
    if (two)
        return ccn2_small_forward(cfg, d_X, d_adj, d_n_batch, params, workspace, d_err, tag, d_out,
                                  (hipStream_t)stream);
    return cs_forward_call<false>(cfg, d_X, d_adj, d_n_batch, params, workspace, d_err, tag, d_out,
                                  (hipStream_t)stream);
}

int hgnn_ccn_small_backward(const hgnn_ccn_config* cfg, const float* d_X, const float* d_adj,
                            const int64_t* d_n_batch, const float* const* params, void* workspace,
                            const float* d_dout, float* const* grads, float* d_dX, void* stream) {
    const bool two = cfg && cfg->order == 2;
    if (two ? !ccn2_small_ok(cfg) : !cs_ok(cfg)) return HGNN_ERR_UNSUPPORTED;
    if (!d_X || !d_adj || !params || !workspace || !d_dout || !grads || !d_dX) return HGNN_ERR_ARG;
    if (two)
        return ccn2_small_backward(cfg, d_X, d_adj, d_n_batch, params, workspace, d_dout, grads, d_dX,
                                   (hipStream_t)stream);
    return cs_backward_call<false>(cfg, d_X, d_adj, d_n_batch, params, workspace, d_dout, grads, d_dX,
                                   (hipStream_t)stream);
}

int hgnn_ccn_small_train_supported(const hgnn_ccn_config* cfg) {
    // a property of the model and nmax: the dispatch walks its graphs one at a time
    return cs_train_ok<false>(cfg) ? 1 : 0;
}

int hgnn_ccn_small_train(const hgnn_ccn_config* cfg, const float* d_X, const float* d_adj, const int64_t* d_n_batch,
                         const float* d_y, double t_mean, double t_std, float* const* params, float* const* grads,
                         float* const* exp_avg, float* const* exp_inf, const float* d_clr, double beta1,
                         double beta2, double eps, double weight_decay, float* d_stats, float* d_out,
                         int32_t* d_err, int32_t tag, void* stream) {
    return cs_train<false, HGNN_OPT_ADAMAX>(cfg, d_X, d_adj, d_n_batch, d_y, t_mean, t_std, params, grads, exp_avg,
                                            exp_inf, d_clr, 1, beta1, beta2, eps, weight_decay, d_stats, d_out, d_err,
                                            tag, stream);
}

int hgnn_ccn_small_train_xent(const hgnn_ccn_config* cfg, const float* d_X, const float* d_adj,
                              const int64_t* d_n_batch, const float* d_y, float* const* params, float* const* grads,
                              float* const* exp_avg, float* const* exp_inf, const float* d_clr, double beta1,
                              double beta2, double eps, double weight_decay, float* d_stats, float* d_out,
                              int32_t* d_err, int32_t tag, void* stream) {
    return cs_train<true, HGNN_OPT_ADAMAX>(cfg, d_X, d_adj, d_n_batch, d_y, 0.0, 1.0, params, grads, exp_avg, exp_inf,
                                           d_clr, 1, beta1, beta2, eps, weight_decay, d_stats, d_out, d_err, tag,
                                           stream);
}

int hgnn_ccn_small_train_opt(const hgnn_ccn_config* cfg, int kind, int xent, const float* d_X, const float* d_adj,
                             const int64_t* d_n_batch, const float* d_y, double t_mean, double t_std,
                             float* const* params, float* const* grads, float* const* state1, float* const* state2,
                             const float* d_steps, double beta1_or_momentum, double beta2, double eps,
                             double weight_decay, float* d_stats, float* d_out, int32_t* d_err, int32_t tag,
                             void* stream) {
    if (!hgnn_ccn_small_train_supported(cfg)) return HGNN_ERR_UNSUPPORTED;
    return opt_dispatch(kind, xent, [&](auto X, auto O) {
        return cs_train<X(), O()>(cfg, d_X, d_adj, d_n_batch, d_y, X() ? 0.0 : t_mean, X() ? 1.0 : t_std, params, grads,
                                  state1, state2, d_steps, 2, beta1_or_momentum, beta2, eps, weight_decay, d_stats,
                                  d_out, d_err, tag, stream);
    });
}

}  // extern "C"
