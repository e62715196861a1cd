// CCN-1D small graphs past the LDS bound: the SPILL instantiations of the one-shot forward and backward and of the
// per-graph training loop (ccn_small_kernels.h).
//
// The LDS kernels keep every row-sized array of a graph (the L levels, dcoll, dF0, dF1; nmax^2 rows each) in LDS, so
// the depth bounds the graph size: 42 nodes at (f, h, L) = (5, 2, 2), 31 at (5, 2, 10), 22 at (8, 8, 4).  Here those
// four arrays live in region blockIdx.x of a caller-allocated global workspace (ccn_small.h CsSpillArgs; the training
// loop has one region, reused graph after graph) and only the plan, the staged inputs and the reduction scratch stay
// in LDS: every shape within nmax <= 64, f, h <= 8, L <= 15 fits.  The device code is the LDS kernels' -- same
// arithmetic, same order, same bits -- with the row pointers set under `if constexpr`.
//   * A region is written and read by its own workgroup only, at per-lane addresses (vector loads and stores), behind
//     the __syncthreads() the kernels have anyway; no new fence.  The training loop keeps its __threadfence() pair
//     around the optimizer pass.
//   * The staged adjacency, which aliases F in the LDS kernels, has nmax^2 floats of LDS of its own.
// k_ccn1_small_reduce does not touch the row arrays: the batch backward launches ccn_small.hip's (cs_launch_reduce).
#include "ccn_small_kernels.h"

using namespace hgnn;

namespace {

size_t spill_rows_bytes(const hgnn_ccn_config* c, int regions) {
    const size_t stride = 4 * cs_spill_stride(c->nmax * c->nmax, c->f_in, c->hidden, c->layers);
    size_t total;
    if (regions < 1 || __builtin_mul_overflow(stride, (size_t)regions, &total)) return 0;
    return total;
}

}  // namespace

extern "C" {

int hgnn_ccn_small_spill_supported(const hgnn_ccn_config* cfg) { return cs_spill_ok(cfg) ? 1 : 0; }

int hgnn_ccn_small_spill_train_supported(const hgnn_ccn_config* cfg) { return cs_train_ok<true>(cfg) ? 1 : 0; }

size_t hgnn_ccn_small_spill_workspace_bytes(const hgnn_ccn_config* cfg, int regions) {
    if (!cs_spill_ok(cfg)) return 0;
    const size_t rows = spill_rows_bytes(cfg, regions);
    size_t total;
    if (!rows || __builtin_add_overflow(rows, cs_head_bytes(cfg), &total)) return 0;
    return total;
}

int hgnn_ccn_small_spill_forward(const hgnn_ccn_config* cfg, const float* d_X, const float* d_adj,
                                 const int64_t* d_n_batch, const float* const* params, void* workspace,
                                 int32_t* d_err, int32_t tag, float* d_out, void* stream) {
    if (!cs_spill_ok(cfg)) return HGNN_ERR_UNSUPPORTED;
    if (!d_X || !d_adj || !params || !workspace || !d_err || !d_out || tag <= 0 || tag >= (1 << 23))
        return HGNN_ERR_ARG;
    return cs_forward_call<true>(cfg, d_X, d_adj, d_n_batch, params, workspace, d_err, tag, d_out,
                                 (hipStream_t)stream);
}

int hgnn_ccn_small_spill_backward(const hgnn_ccn_config* cfg, const float* d_X, const float* d_adj,
                                  const int64_t* d_n_batch, const float* const* params, void* workspace,
                                  const float* d_dout, float* const* grads, float* d_dX, void* stream) {
    if (!cs_spill_ok(cfg)) return HGNN_ERR_UNSUPPORTED;
    if (!d_X || !d_adj || !params || !workspace || !d_dout || !grads || !d_dX) return HGNN_ERR_ARG;
    return cs_backward_call<true>(cfg, d_X, d_adj, d_n_batch, params, workspace, d_dout, grads, d_dX,
                                  (hipStream_t)stream);
}

int hgnn_ccn_small_spill_train(const hgnn_ccn_config* cfg, int kind, int xent, const float* d_X, const float* d_adj,
                               const int64_t* d_n_batch, const float* d_y, double t_mean, double t_std,
                               float* const* params, float* const* grads, float* const* state1,
                               float* const* state2, const float* d_steps, double beta1_or_momentum, double beta2,
                               double eps, double weight_decay, float* d_stats, float* d_out, void* workspace,
                               int32_t* d_err, int32_t tag, void* stream) {
    if (!cs_train_ok<true>(cfg)) return HGNN_ERR_UNSUPPORTED;
    return opt_dispatch(kind, xent, [&](auto X, auto O) {
        return cs_train<X(), O(), true>(cfg, d_X, d_adj, d_n_batch, d_y, X() ? 0.0 : t_mean, X() ? 1.0 : t_std, params,
                                        grads, state1, state2, d_steps, 2, beta1_or_momentum, beta2, eps,
                                        weight_decay, d_stats, d_out, d_err, tag, stream, workspace);
    });
}

}  // extern "C"
