// The CCN-1D mini-batch kernel, a list of ccn_small.h's stages, and the launch loop, as templates on SPILL:
// ccn_small_batch.hip instantiates the LDS form, ccn_small_batch_spill.hip the form whose row arrays live in
// per-workgroup global regions (ccn_small.h CsSpillArgs).  k_ccn1_small_apply does not touch the row arrays: it is
// compiled once, in ccn_small_batch.hip, behind cb_launch_apply.
#pragma once
#include "ccn_small.h"

namespace hgnn {

// One mini-batch: what both kernels need besides CsArgs (whose X / adj / n_batch / out point at the mini-batch's
// first graph, feat / ppart at the workspace regions; CsArgs::bs only selects cs_bwd_level's batch form).
struct CbBatch {
    const float* y;      // raw targets of the mini-batch: (B, n_out), classification: (B,) class indices
    float t_mean, t_div;  // yn = (y - mean) / div, div = std + 1e-8
    int B;               // graphs of this mini-batch: the divisor of its loss
    float* dout;         // [B][n_out] workspace region
    uint32_t* reject;    // the mini-batch's reject word (cleared by the entry)
};

struct CbApply {
    const float* steps;  // the mini-batch's two per-step scalars (hgnn_ccn_small_train_opt's row)
    OptScalars h;
    float* p[CS_TMAX];
    float* m[CS_TMAX];
    float* u[CS_TMAX];   // SGD: not touched
    float* stats;        // [4] loss, mae and their RunningAverages
};

// k_ccn1_small_apply<OPT, XENT> over `outs` parameter elements (ccn_small_batch.hip)
template <int OPT, bool XENT>
int cb_launch_apply(const CsArgs& a, const CbBatch& t, const CbApply& q, int outs, hipStream_t s);

namespace {

template <int CF, int CH, bool XENT, bool SPILL = false>
__global__ void __launch_bounds__(CS_NT) k_ccn1_small_batch(CsArgsT<SPILL> a, CbBatch t) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    __shared__ uint32_t sbad;
    const int b = blockIdx.x;
    const CsLds s = cs_carve<SPILL>(lds, a, true);
    float* As = cs_adj<SPILL>(lds, s);
    const int nf = a.f + a.L * a.h, n_out = a.n_out;
    const float* Xg = s.Xs;
    // 1. stage and plan
    if (threadIdx.x == 0) sbad = 0;
    uint32_t bad = 0;
    const int n = cs_open(a, b, s, As, bad);
    cs_report(bad, sbad);
    const int G = s.off1[66];
    const int rows = s.off1[n];
    // 2. every level, kept; the readout sums; out = fc(feat)
    cs_levels_keep<CF, SPILL>(a, s, n, G, Xg);
    cs_readout_sums<CF>(a, s, n, rows, Xg);
    cs_out_row(a, s, nf, n_out, a.out + (long long)b * n_out, s.red);
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
    // 3. the graph's dout row (elementwise, so local to the block); dout replaces out in red
    if constexpr (XENT) {
        // k_xent_loss's row with n = B, by one thread in the row function's serial order
        if (threadIdx.x == 0) (void)xent_row(s.red, ti, n_out, 1.0f / (float)t.B, s.red);
    } else {
        // mse_block's elements on the normalised target, n = B n_out
        const int nel = t.B * n_out;
        for (int i = threadIdx.x; i < n_out; i += CS_NT) {
            float yn = t.y[(long long)b * n_out + i] - t.t_mean;
            yn = yn / t.t_div;
            const float d = s.red[i] - yn;
            s.red[i] = 2.0f * d / (float)nel;
        }
    }
    __syncthreads();
    // the readout features and the row for the apply kernel's fc gradients, before dsum replaces the features
    const float* dob = s.red;
    for (int k = threadIdx.x; k < nf; k += CS_NT) a.feat[(long long)b * nf + k] = s.vec[k];
    for (int i = threadIdx.x; i < n_out; i += CS_NT) t.dout[(long long)b * n_out + i] = dob[i];
    __syncthreads();
    // 4. backward, k_ccn1_small_bwd's batch form: dsum, then the levels (their partials go to ppart[b])
    cs_dsum(a, s, dob, nf);
    __syncthreads();
    cs_backward<CF, CH, false, SPILL>(a, s, b, n, G, Xg);
}

size_t cb_align(size_t n) { return (n + 255) / 256 * 256; }

// Workspace: the reject words first (cfg->bs of them reserved, so the size grows with `batch` and a workspace sized
// for (bs, batch) serves every call with no more graphs and no larger mini-batches; a call uses and clears the first
// ceil(bs / batch)), then one mini-batch's regions, each 256-byte aligned.
struct CbLayout {
    size_t ppart, feat, dout, total;  // byte offsets
};

CbLayout cb_layout(const hgnn_ccn_config* c, int batch) {
    CbLayout w;
    w.ppart = cb_align(4 * (size_t)c->bs);
    w.feat = w.ppart + cb_align(4 * (size_t)batch * cs_ptot(c));
    w.dout = w.feat + cb_align(4 * (size_t)batch * cs_nf(c));
    w.total = w.dout + cb_align(4 * (size_t)batch * c->n_out);
    return w;
}

// SPILL: `rows` holds `batch` row regions (region b is the mini-batch's graph b, reused mini-batch after mini-batch:
// the stream orders the dispatches).
template <bool XENT, int OPT, bool SPILL = false>
int cb_train(const hgnn_ccn_config* cfg, int batch, const float* d_X, const float* d_adj, const int64_t* d_n_batch,
             const float* d_y, double t_mean, double t_std, float* const* params, float* const* grads,
             float* const* state1, float* const* state2, const float* d_steps, double beta1_or_momentum,
             double beta2, double eps, double weight_decay, float* d_stats, float* d_out, void* workspace,
             int32_t* d_err, int32_t tag, hipStream_t s, void* rows = nullptr) {
    constexpr bool TWO = OPT != HGNN_OPT_SGD;  // whether the second state array is used
    const int nt = 2 * cfg->layers + 2, G = cfg->bs;
    if (TWO && !state2) return HGNN_ERR_ARG;
    for (int k = 0; k < nt; ++k)
        if (!params[k] || !grads[k] || !state1[k] || (TWO && !state2[k])) return HGNN_ERR_ARG;
    // X / adj / n_batch / out follow per mini-batch
    CsArgsT<SPILL> a = cs_args<SPILL>(cfg, nullptr, nullptr, nullptr, params, nullptr);
    if constexpr (SPILL) a.rows = static_cast<float*>(rows);
    a.bs = 2;  // cs_bwd_level's batch form (partials to ppart[b]), also for a mini-batch of one graph
    cs_set_grads(a, grads);
    a.err = d_err;
    a.tag = tag;
    const CbLayout lay = cb_layout(cfg, batch);
    char* ws = static_cast<char*>(workspace);
    a.ppart = reinterpret_cast<float*>(ws + lay.ppart);
    a.feat = reinterpret_cast<float*>(ws + lay.feat);
    CbBatch t{};
    // scalars combine in double and reach the kernels as fp32, as the reference's Python floats reach torch
    t.t_mean = (float)t_mean;
    t.t_div = (float)(t_std + 1e-8);  // scripts/train_ccn.py:42
    t.dout = reinterpret_cast<float*>(ws + lay.dout);
    CbApply q{};
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
    const size_t lds = cs_lds_for<SPILL>(a, true);
    for (int k = 0; k < K; ++k) {
        const long long g0 = (long long)k * batch;
        const int B = (int)(G - g0 < batch ? G - g0 : batch);  // the last mini-batch may be shorter
        a.X = d_X + g0 * a.nmax * a.f;
        a.adj = d_adj + g0 * a.nmax * a.nmax;
        a.n_batch = d_n_batch ? d_n_batch + g0 : nullptr;
        a.out = d_out + g0 * a.n_out;
        t.y = d_y + (XENT ? g0 : g0 * a.n_out);
        t.B = B;
        t.reject = reject + k;
        q.steps = d_steps + 2 * (long long)k;  // row k is mini-batch k's, applied or not
        cs_launch_ch<&k_ccn1_small_batch<CS_CF, 2, XENT, SPILL>, &k_ccn1_small_batch<CS_CF, CS_CF, XENT, SPILL>, SPILL>(
            cfg->hidden, B, lds, s, a, t);
        HGNN_LAUNCH_CHECK();
        TRY((cb_launch_apply<OPT, XENT>(a, t, q, cs_nouts(cfg), s)));
    }
    return HGNN_OK;
}

}  // namespace
}  // namespace hgnn
