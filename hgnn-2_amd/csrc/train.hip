// Device-resident training step pieces: the loss and the
// optimizer of scripts/train_mnb.py:41-91 without host round trips.
//
//  * hgnn_mse_loss: T' = normalize_data(T, mean, std) (functions/utils.py:84-95,
//    mean only when std < 1e-5, Q14), loss = mean((out - T')^2) (nn.MSELoss,
//    scripts/train_mnb.py:76), the seed gradient dout = 2 (out - T') / n, the MAE
//    of utils.evaluation (functions/utils.py:98-102) and the RunningAverage
//    updates of both (functions/utils.py:134-146) -- one block, no host sync
//    (the reference calls .item() twice per batch).
//  * hgnn_optim_step: torch.optim.Adamax (scripts/main_gnn_qm9.py:185), torch.optim.SGD or
//    torch.optim.Adam (scripts/main_gnn.py:161-167) over every parameter tensor in one
//    launch (multi-tensor apply); the element updates are in kernels.h.  Adamax, per element
//      g += wd p;  m = lerp(m, g, 1 - b1);  u = max(b2 u, |g| + eps);
//      p -= lr / (1 - b1^t) * m / u
//    in torch's operation order (lerp as a + w (b - a) for w < 0.5).
//  * hgnn_eval_loss / hgnn_eval_xent: the AverageMeters of scripts/test_mnb.py:25-92 accumulated on the device
//    over the batches of a set (six doubles), so a validation pass has no host round trip either.
#include "kernels.h"

namespace hgnn {
namespace {

__global__ void __launch_bounds__(256) k_mse_loss(const float* __restrict__ out, const float* __restrict__ t, int n,
                                                  float t_mean, float t_std, float* __restrict__ stats,
                                                  float* __restrict__ dout) {
    float loss, mae;
    mse_block(out, t, n, t_mean, t_std, dout, loss, mae);
    if (threadIdx.x == 0) {
        stats[0] = loss;
        stats[1] = mae;
        // RunningAverage(momentum = 0.1): first value taken as is, then 0.9 new + 0.1 old
        stats[2] = stats[2] == 0.f ? loss : 0.9f * loss + 0.1f * stats[2];
        stats[3] = stats[3] == 0.f ? mae : 0.9f * mae + 0.1f * stats[3];
    }
}

// Classification branch of the reference step (scripts/train_mnb.py:50-51: mean == 0 ->
// T = T.squeeze().long(); the drivers pass nn.CrossEntropyLoss, scripts/main_generate.py:147):
// loss = mean_i (logsumexp(out_i) - out_i[t_i]), dout = (softmax(out_i) - onehot(t_i)) / n,
// the running loss as in k_mse_loss; the MAE meters are not updated (train_mnb.py:81-82).
// One block; a thread per row, classes in a serial loop (C is the model's dim_output).
__global__ void __launch_bounds__(256) k_xent_loss(const float* __restrict__ out, const float* __restrict__ t, int n,
                                                   int c, float* __restrict__ stats, float* __restrict__ dout,
                                                   uint32_t* __restrict__ err) {
    __shared__ double red[4];
    double se = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float* x = out + (long long)i * c;
        int ti;
        if (!xent_target(t[i], c, ti)) {
            // a rejected row contributes nothing: its dout row is zero, never uninitialised memory
            atomicOr(err, 1u);
            if (dout)
                for (int k = 0; k < c; ++k) dout[(long long)i * c + k] = 0.f;
            continue;
        }
        se += (double)xent_row(x, ti, c, 1.0f / (float)n, dout ? dout + (long long)i * c : nullptr);
    }
    se = wave_sum_d(se);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = se;
    __syncthreads();
    if (threadIdx.x == 0) {
        double S = 0.0;
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) S += red[i];
        const float loss = n > 0 ? (float)(S / n) : 0.f;
        stats[0] = loss;
        stats[2] = stats[2] == 0.f ? loss : 0.9f * loss + 0.1f * stats[2];
    }
}

constexpr int OPT_MAX = 64;

struct OptTable {
    float* p[OPT_MAX];
    const float* g[OPT_MAX];
    float* s1[OPT_MAX];
    float* s2[OPT_MAX];  // SGD: not read
    int n[OPT_MAX];
    int start[OPT_MAX + 1];  // prefix of per-tensor block counts
    int count;
};

// One optimizer step over up to 64 tensors; OPT picks the element update (kernels.h optim_at), c0 / c1 are the
// step's scalars.
template <int OPT>
__global__ void __launch_bounds__(256) k_optim(OptTable tab, float c0, float c1, OptScalars h) {
    // block -> tensor by the block prefix (uniform scan over <= 64 entries)
    int t = 0;
    while (t + 1 < tab.count && (int)blockIdx.x >= tab.start[t + 1]) ++t;
    const int i = ((int)blockIdx.x - tab.start[t]) * 256 + threadIdx.x;
    if (i >= tab.n[t]) return;
    optim_at<OPT>(tab.p[t], tab.g[t][i], tab.s1[t], tab.s2[t], i, c0, c1, h);
}

// Evaluation meters of scripts/test_ccn.py:34-67 over G graphs' outputs: [mean_g MSE_g, mean_g MAE_g] with the
// target normalised as in the training kernel (true division by the fp32 divisor).  One block; fp64 sums in a
// fixed order (graphs strided over the threads, lanes, then the waves in order): the same bits every call.
__global__ void __launch_bounds__(256) k_ccn_eval_loss(const float* __restrict__ out, const float* __restrict__ y,
                                                       int G, int n_out, float t_mean, float t_div,
                                                       float* __restrict__ res) {
    __shared__ double red[2][4];
    double se = 0.0, ae = 0.0;
    for (int g = threadIdx.x; g < G; g += 256) {
        double s = 0.0, a = 0.0;
        for (int o = 0; o < n_out; ++o) {
            const float yn = (y[(long long)g * n_out + o] - t_mean) / t_div;
            const float d = out[(long long)g * n_out + o] - yn;
            s += (double)d * d;
            a += fabs((double)d);
        }
        se += s / n_out;
        ae += a / n_out;
    }
    se = wave_sum_d(se);
    ae = wave_sum_d(ae);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = se;
        red[1][threadIdx.x >> 6] = ae;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double S = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        const double A = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        res[0] = G > 0 ? (float)(S / G) : 0.f;
        res[1] = G > 0 ? (float)(A / G) : 0.f;
    }
}

// The classification branch of the same loop (test_ccn.py:40-41, 52-55: the target cast to a class index, the
// output viewed as (1, n_out), nn.CrossEntropyLoss): [mean_g xent_g, 0, accuracy].  error.avg is never updated
// on that branch and stays 0; the accuracy counts the graphs whose first maximum (torch.argmax's tie rule) is
// the target.  A target that is no class index is reported and adds to neither sum; the divisor stays G.  One
// block, fp64 sums in k_ccn_eval_loss's fixed order.
__global__ void __launch_bounds__(256) k_ccn_eval_xent(const float* __restrict__ out, const float* __restrict__ y,
                                                       int G, int c, float* __restrict__ res,
                                                       uint32_t* __restrict__ err) {
    __shared__ double red[2][4];
    double se = 0.0, hit = 0.0;
    for (int g = threadIdx.x; g < G; g += 256) {
        const float* x = out + (long long)g * c;
        int ti;
        if (!xent_target(y[g], c, ti)) {
            atomicOr(err, 1u);
            continue;
        }
        se += (double)xent_row(x, ti, c, 1.0f, nullptr);
        int am = 0;
        for (int k = 1; k < c; ++k)
            if (x[k] > x[am]) am = k;
        hit += am == ti ? 1.0 : 0.0;
    }
    se = wave_sum_d(se);
    hit = wave_sum_d(hit);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = se;
        red[1][threadIdx.x >> 6] = hit;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double S = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        const double H = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        res[0] = G > 0 ? (float)(S / G) : 0.f;
        res[1] = 0.f;
        res[2] = G > 0 ? (float)(H / G) : 0.f;
    }
}

// The evaluation meters of scripts/test_mnb.py:25-92 (two AverageMeters, update(value, bs) per batch) kept on the
// device: m[0] = loss.sum, m[1] = error.sum, m[2] = count, m[3] = hits, m[4] = loss.val, m[5] = error.val.  One
// thread updates them with plain loads and stores -- stream order serialises the batches of a set -- in double,
// product and sum rounded separately as AverageMeter's Python floats are.  This is the regression branch
// (test_mnb.py:52, 64-70): the batch loss and MAE are k_mse_loss's (mse_block), bit for bit.
__global__ void __launch_bounds__(256) k_eval_loss(const float* __restrict__ out, const float* __restrict__ t, int n,
                                                   int rows, float t_mean, float t_std, double* __restrict__ m) {
    float loss, mae;
    mse_block(out, t, n, t_mean, t_std, nullptr, loss, mae);
    if (threadIdx.x == 0) {
#pragma clang fp contract(off)
        const double ls = (double)loss * (double)rows;
        const double es = (double)mae * (double)rows;
        m[0] = m[0] + ls;
        m[1] = m[1] + es;
        m[2] = m[2] + (double)rows;
        m[4] = (double)loss;
        m[5] = (double)mae;
    }
}

// The classification branch (test_mnb.py:49-50, nn.CrossEntropyLoss): the batch's mean cross entropy as in
// k_xent_loss (xent_target, xent_row; a thread per row) and the hit count by k_ccn_eval_xent's rule (the first
// maximum, torch.argmax's tie rule).  A target that is no class index is reported and adds to neither sum; the
// divisor stays `rows`.  m[1] and m[5] are never written: the reference leaves `error` untouched on this branch.
__global__ void __launch_bounds__(256) k_eval_xent(const float* __restrict__ out, const float* __restrict__ t,
                                                   int rows, int c, double* __restrict__ m,
                                                   uint32_t* __restrict__ err) {
    __shared__ double red[2][4];
    double se = 0.0, hit = 0.0;
    for (int i = threadIdx.x; i < rows; i += 256) {
        const float* x = out + (long long)i * c;
        int ti;
        if (!xent_target(t[i], c, ti)) {
            atomicOr(err, 1u);
            continue;
        }
        se += (double)xent_row(x, ti, c, 1.0f, nullptr);
        int am = 0;
        for (int k = 1; k < c; ++k)
            if (x[k] > x[am]) am = k;
        hit += am == ti ? 1.0 : 0.0;
    }
    se = wave_sum_d(se);
    hit = wave_sum_d(hit);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = se;
        red[1][threadIdx.x >> 6] = hit;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma clang fp contract(off)
        const double S = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        const double H = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        const float loss = (float)(S / rows);
        const double ls = (double)loss * (double)rows;
        m[0] = m[0] + ls;
        m[2] = m[2] + (double)rows;
        m[3] = m[3] + H;
        m[4] = (double)loss;
    }
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

extern "C" {

int hgnn_mse_loss(const float* d_out, const float* d_t, int n, float t_mean, float t_std, float* d_stats,
                  float* d_dout, void* stream) {
    if (!d_out || !d_t || !d_stats || n < 0) return HGNN_ERR_ARG;
    HGNN_KLAUNCH(k_mse_loss, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), d_out, d_t, n, t_mean,
                       t_std, d_stats, d_dout);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

int hgnn_xent_loss(const float* d_out, const float* d_t, int n, int c, float* d_stats, float* d_dout,
                   uint32_t* d_err, void* stream) {
    if (!d_out || !d_t || !d_stats || !d_err || n < 0 || c < 1) return HGNN_ERR_ARG;
    HGNN_KLAUNCH(k_xent_loss, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), d_out, d_t, n, c,
                       d_stats, d_dout, d_err);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

int hgnn_ccn_eval_loss(const float* d_out, const float* d_y, int n_graphs, int n_out, double t_mean, double t_std,
                       float* d_res, void* stream) {
    if (!d_out || !d_y || !d_res || n_graphs < 0 || n_out < 1) return HGNN_ERR_ARG;
    const float div = (float)(t_std + 1e-8);  // std + 10 ** -8 in double, then fp32 (test_ccn.py:43)
    HGNN_KLAUNCH(k_ccn_eval_loss, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), d_out, d_y, n_graphs,
                       n_out, (float)t_mean, div, d_res);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

int hgnn_ccn_eval_xent(const float* d_out, const float* d_y, int n_graphs, int n_out, float* d_res, uint32_t* d_err,
                       void* stream) {
    if (!d_out || !d_y || !d_res || !d_err || n_graphs < 0 || n_out < 1) return HGNN_ERR_ARG;
    HGNN_KLAUNCH(k_ccn_eval_xent, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), d_out, d_y, n_graphs,
                       n_out, d_res, d_err);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

int hgnn_eval_loss(const float* d_out, const float* d_t, int rows, int dim_out, float t_mean, float t_std,
                   double* d_meters, void* stream) {
    if (!d_out || !d_t || !d_meters || rows < 0 || dim_out < 1) return HGNN_ERR_ARG;
    if ((long long)rows * dim_out >= (1ll << 31)) return HGNN_ERR_ARG;
    if (rows == 0) return HGNN_OK;  // an empty batch updates no meter
    HGNN_KLAUNCH(k_eval_loss, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), d_out, d_t, rows * dim_out,
                       rows, t_mean, t_std, d_meters);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

int hgnn_eval_xent(const float* d_out, const float* d_t, int rows, int c, double* d_meters, uint32_t* d_err,
                   void* stream) {
    if (!d_out || !d_t || !d_meters || !d_err || rows < 0 || c < 1) return HGNN_ERR_ARG;
    if ((long long)rows * c >= (1ll << 31)) return HGNN_ERR_ARG;
    if (rows == 0) return HGNN_OK;
    HGNN_KLAUNCH(k_eval_xent, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), d_out, d_t, rows, c,
                       d_meters, d_err);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

int hgnn_optim_step(int kind, int n_tensors, float* const* params, const float* const* grads, float* const* state1,
                    float* const* state2, const int64_t* numel, double lr, double beta1_or_momentum, double beta2,
                    double eps, double weight_decay, long long step, void* stream) {
    if (kind != HGNN_OPT_ADAMAX && kind != HGNN_OPT_SGD && kind != HGNN_OPT_ADAM) return HGNN_ERR_ARG;
    const bool two = kind != HGNN_OPT_SGD;  // whether state2 is used
    if (n_tensors < 0 || (n_tensors > 0 && (!params || !grads || !state1 || (two && !state2) || !numel)) || step < 1)
        return HGNN_ERR_ARG;
    for (int k = 0; k < n_tensors; ++k) {
        if (numel[k] < 0 || numel[k] > (1ll << 30)) return HGNN_ERR_ARG;
        if (numel[k] > 0 && (!params[k] || !grads[k] || !state1[k] || (two && !state2[k]))) return HGNN_ERR_ARG;
    }
    // hyper-parameters combine in double (Python floats) and reach the kernel as fp32 scalars, as torch's scalar
    // arguments do: Adamax / Adam c0 = lr / (1 - beta1^step), Adam c1 = sqrt(1 - beta2^step); SGD c0 = lr
    float c0 = (float)lr, c1 = 0.f;
    if (kind != HGNN_OPT_SGD) c0 = (float)(lr / (1.0 - pow(beta1_or_momentum, (double)step)));
    if (kind == HGNN_OPT_ADAM) c1 = (float)sqrt(1.0 - pow(beta2, (double)step));
    const OptScalars h = opt_scalars(kind, beta1_or_momentum, beta2, eps, weight_decay);
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int base = 0; base < n_tensors; base += OPT_MAX) {
        OptTable tab{};
        tab.count = 0;
        int blocks = 0;
        for (int k = base; k < n_tensors && tab.count < OPT_MAX; ++k) {
            const int c = tab.count++;
            tab.p[c] = params[k];
            tab.g[c] = grads[k];
            tab.s1[c] = state1[k];
            tab.s2[c] = two ? state2[k] : nullptr;
            tab.n[c] = (int)numel[k];
            tab.start[c] = blocks;
            blocks += (int)ceil_div<long long>(numel[k], 256);
        }
        tab.start[tab.count] = blocks;
        if (blocks == 0) continue;
        if (kind == HGNN_OPT_SGD) HGNN_KLAUNCH(k_optim<HGNN_OPT_SGD>, dim3(blocks), dim3(256), 0, s, tab, c0, c1, h);
        else if (kind == HGNN_OPT_ADAM) HGNN_KLAUNCH(k_optim<HGNN_OPT_ADAM>, dim3(blocks), dim3(256), 0, s, tab, c0, c1, h);
        else HGNN_KLAUNCH(k_optim<HGNN_OPT_ADAMAX>, dim3(blocks), dim3(256), 0, s, tab, c0, c1, h);
        HGNN_LAUNCH_CHECK();
    }
    return HGNN_OK;
}

int hgnn_adamax_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                     float* const* exp_inf, const int64_t* numel, double lr, double beta1, double beta2,
                     double eps, double weight_decay, long long step, void* stream) {
    return hgnn_optim_step(HGNN_OPT_ADAMAX, n_tensors, params, grads, exp_avg, exp_inf, numel, lr, beta1, beta2, eps,
                           weight_decay, step, stream);
}

}  // extern "C"
