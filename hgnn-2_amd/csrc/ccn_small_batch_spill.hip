// CCN-1D mini-batch training past the LDS bound: the SPILL instantiation of k_ccn1_small_batch
// (ccn_small_batch_kernels.h).  Workgroup b of a mini-batch keeps its row arrays in region b of the spill workspace
// (ccn_small_spill.hip says what a region is and why that is coherent); the regions are reused mini-batch after
// mini-batch, ordered by the stream like the rest of the workspace.  The workspace of hgnn_ccn_small_train_batch is used
// as it is, and the apply kernel is ccn_small_batch.hip's (cb_launch_apply).
#include "ccn_small_batch_kernels.h"

using namespace hgnn;

extern "C" {

int hgnn_ccn_small_spill_train_batch(const hgnn_ccn_config* cfg, int batch, int kind, int xent, const float* d_X,
                                     const float* d_adj, const int64_t* d_n_batch, const float* d_y, double t_mean,
                                     double t_std, float* const* params, float* const* grads, float* const* state1,
                                     float* const* state2, const float* d_steps, double beta1_or_momentum,
                                     double beta2, double eps, double weight_decay, float* d_stats, float* d_out,
                                     void* workspace, void* spill_workspace, int32_t* d_err, int32_t tag,
                                     void* stream) {
    if (!hgnn_ccn_small_spill_train_supported(cfg)) return HGNN_ERR_UNSUPPORTED;
    if (!d_X || !d_adj || !d_y || !params || !grads || !state1 || !d_steps || !d_stats || !d_out || !workspace ||
        !spill_workspace || !d_err || tag <= 0 || tag >= (1 << 23) || batch < 1 || cfg->bs < 1 ||
        cfg->bs > CS_TRAIN_GMAX || (xent && cfg->n_out < 2))
        return HGNN_ERR_ARG;
    // hgnn_ccn_small_train_batch's rule for the MSE meters' divisor
    if (!xent && (float)(t_std + 1e-8) < 1e-5f) return HGNN_ERR_ARG;
    return opt_dispatch(kind, xent, [&](auto X, auto O) {
        return cb_train<X(), O(), true>(cfg, batch, d_X, d_adj, d_n_batch, d_y, X() ? 0.0 : t_mean,
                                        X() ? 1.0 : t_std, params, grads, state1, state2, d_steps,
                                        beta1_or_momentum, beta2, eps, weight_decay, d_stats, d_out, workspace, d_err,
                                        tag, (hipStream_t)stream, spill_workspace);
    });
}

}  // extern "C"
