// The CCN-1D mini-batch kernels and their launch loop, as templates on SPILL: ccn_small_batch.hip instantiates the LDS
// form, ccn_small_batch_spill.hip the form whose row arrays live in per-workgroup global regions (ccn_small.h
// CsSpillArgs).  k_ccn1_small_apply does not touch the row arrays and is the same kernel for both.
#pragma once
#include "ccn_small.h"

namespace hgnn {
namespace {

constexpr int CB_TMAX = 2 * CS_LMAX + 2;  // parameter tensors: level weights and biases, fc weight and bias
constexpr int CB_GMAX = 4096;             // graphs per call (k_ccn1_small_train's bound)

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
    float* p[CB_TMAX];
    float* m[CB_TMAX];
    float* u[CB_TMAX];   // SGD: not touched
    float* stats;        // [4] loss, mae and their RunningAverages
};

template <int CF, int CH, bool XENT, bool SPILL = false>
__global__ void __launch_bounds__(CS_NT) k_ccn1_small_batch(CsArgsT<SPILL> a, CbBatch t) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    __shared__ uint32_t sbad;
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const CsLds s = cs_carve<SPILL>(lds, a, true);
    float* As = cs_adj<SPILL>(lds, s);
    const int h = a.h, f = a.f, L = a.L, nf = f + L * h, n_out = a.n_out;
    const float* Xg = s.Xs;
    // 1. stage and plan
    if (threadIdx.x == 0) sbad = 0;
    uint32_t bad = 0;
    const int n = cs_nodes(a, b, bad);
    cs_stage(a, b, n, s, As);
    bad |= cs_plan(n, s, As);
    bad = wave_or(bad);
    if (lane == 0 && bad) atomicOr(&sbad, bad);
    const int G = s.off1[66];
    const int rows = s.off1[n];
    // 2. every level, kept; the readout sums; out = fc(feat)
    for (int l = 0; l < L; ++l) {
        const int cin = l == 0 ? f : h;
        const float* fin = l == 0 ? nullptr : s.F + (size_t)(l - 1) * a.rcap * h;
        float* fout = s.F + (size_t)l * a.rcap * h;
        const float* Wl = s.Ws + cs_woff(l, f, h);
        if (cin <= 2) cs_fwd_level<2, SPILL>(s, n, G, Xg, fin, cin, Wl, h, fout);
        else cs_fwd_level<CF, SPILL>(s, n, G, Xg, fin, cin, Wl, h, fout);
        __syncthreads();
    }
    cs_colsum<CF>(s, n, f, 0, [&](int r, int c) { return (double)s.deg[r] * (double)Xg[r * f + c]; });
    for (int l = 0; l < L; ++l) {
        const float* fl = s.F + (size_t)l * a.rcap * h;
        cs_colsum<CF>(s, rows, h, f + l * h, [&](int r, int c) { return (double)fl[r * h + c]; });
    }
    for (int o = 0; o < n_out; ++o) {
        const double v = cs_fc(a, s, o, nf);
        if (threadIdx.x == 0) {
            const float ov = (float)(v + (double)a.fcb[o]);
            a.out[(long long)b * n_out + o] = ov;
            s.red[o] = ov;
        }
    }
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
    for (int k = threadIdx.x; k < nf; k += CS_NT) {
        float v = 0.f;
        for (int o = 0; o < n_out; ++o) v = fmaf(dob[o], a.fcw[o * nf + k], v);
        s.vec[k] = v;
    }
    __syncthreads();
    float* dFc = s.dF0;
    float* dFn = s.dF1;
    for (int l = L - 1; l >= 0; --l) {
        if ((l == 0 ? f : h) <= 2) cs_bwd_level<2, CH, false, SPILL>(a, s, b, l, n, G, Xg, dFc, dFn);
        else cs_bwd_level<CF, CH, false, SPILL>(a, s, b, l, n, G, Xg, dFc, dFn);
        float* x = dFc;
        dFc = dFn;
        dFn = x;
    }
}

// One wave per parameter element (the level entries, then fc weight and bias from dout and the readout features):
// k_ccn1_small_reduce's sum over the mini-batch's graphs, the gradient, the optimizer's update of that element.
template <int OPT, bool XENT>
__global__ void __launch_bounds__(256) k_ccn1_small_apply(CsArgs a, CbBatch t, CbApply q) {
    // a rejected mini-batch: no gradients, no meters, no step (block-uniform: every block reads the word first)
    if (*t.reject != 0u) return;
    const int h = a.h, f = a.f, L = a.L, nf = f + L * h, n_out = a.n_out, B = t.B;
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
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int p0 = h * 2 * f + h, p1 = h * 2 * h + h, ptot = p0 + (L - 1) * p1;
    if (w >= ptot + n_out * nf + n_out) return;
    double s = 0.0;
    if (w < ptot) {
        for (int b = lane; b < B; b += 64) s += (double)a.ppart[(long long)b * ptot + w];
    } else if (w < ptot + n_out * nf) {
        const int o = (w - ptot) / nf, k = (w - ptot) % nf;
        for (int b = lane; b < B; b += 64) s += (double)t.dout[b * n_out + o] * (double)a.feat[(long long)b * nf + k];
    } else {
        const int o = w - ptot - n_out * nf;
        for (int b = lane; b < B; b += 64) s += (double)t.dout[b * n_out + o];
    }
    s = wave_sum_d(s);
    if (lane != 0) return;
    const float g = (float)s;
    int ti, e;
    if (w < ptot) {
        const int l = w < p0 ? 0 : 1 + (w - p0) / p1;
        const int p = l == 0 ? w : (w - p0) % p1;
        const int k2 = 2 * (l == 0 ? f : h);
        if (p < h * k2) {
            a.gW[l][p] = g;
            ti = 2 * l;
            e = p;
        } else {
            a.gB[l][p - h * k2] = g;
            ti = 2 * l + 1;
            e = p - h * k2;
        }
    } else if (w < ptot + n_out * nf) {
        a.gfcw[w - ptot] = g;
        ti = 2 * L;
        e = w - ptot;
    } else {
        a.gfcb[w - ptot - n_out * nf] = g;
        ti = 2 * L + 1;
        e = w - ptot - n_out * nf;
    }
    float c1 = 0.f;
    if constexpr (OPT == HGNN_OPT_ADAM) c1 = q.steps[1];
    optim_at<OPT>(q.p[ti], g, q.m[ti], q.u[ti], e, q.steps[0], c1, q.h);
}

size_t cb_align(size_t n) { return (n + 255) / 256 * 256; }

// Workspace: the reject words first (cfg->bs of them reserved, so the size grows with `batch` and a workspace sized
// for (bs, batch) serves every call with no more graphs and no larger mini-batches; a call uses and clears the first
// ceil(bs / batch)), then one mini-batch's regions, each 256-byte aligned.
struct CbLayout {
    size_t ppart, feat, dout, total;  // byte offsets
};

CbLayout cb_layout(const hgnn_ccn_config* c, int batch) {
    const int h = c->hidden, f = c->f_in, nf = f + c->layers * h;
    const size_t ptot = (size_t)(h * 2 * f + h) + (size_t)(c->layers - 1) * (h * 2 * h + h);
    CbLayout w;
    w.ppart = cb_align(4 * (size_t)c->bs);
    w.feat = w.ppart + cb_align(4 * (size_t)batch * ptot);
    w.dout = w.feat + cb_align(4 * (size_t)batch * nf);
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
    const int L = cfg->layers, nt = 2 * L + 2, G = cfg->bs;
    if (TWO && !state2) return HGNN_ERR_ARG;
    for (int k = 0; k < nt; ++k)
        if (!params[k] || !grads[k] || !state1[k] || (TWO && !state2[k])) return HGNN_ERR_ARG;
    CsArgsT<SPILL> a{};
    a.bs = 2;  // cs_bwd_level's batch form (partials to ppart[b]), also for a mini-batch of one graph
    a.nmax = cfg->nmax;
    a.f = cfg->f_in;
    a.h = cfg->hidden;
    a.L = L;
    a.n_out = cfg->n_out;
    a.rcap = cfg->nmax * cfg->nmax;
    if constexpr (SPILL) {
        a.rows = static_cast<float*>(rows);
        a.rstride = (long long)cs_spill_stride(a.rcap, a.f, a.h, a.L);
    }
    for (int l = 0; l < L; ++l) {
        a.W[l] = params[2 * l];
        a.B[l] = params[2 * l + 1];
        a.gW[l] = grads[2 * l];
        a.gB[l] = grads[2 * l + 1];
    }
    a.fcw = params[2 * L];
    a.fcb = params[2 * L + 1];
    a.gfcw = grads[2 * L];
    a.gfcb = grads[2 * L + 1];
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
    // SPILL: at most 37.2 KB at nmax = 64, within the static limit (no opt-in)
    const size_t lds = SPILL ? cs_spill_lds_bytes(a.rcap) : cs_lds_bytes(a.rcap, a.f, a.h, a.L, true);
    const CsArgs& base = a;  // what the apply kernel takes: it does not touch the row arrays
    const int nf = a.f + L * a.h;
    const int ptot = (a.h * 2 * a.f + a.h) + (L - 1) * (a.h * 2 * a.h + a.h);
    const int outs = ptot + a.n_out * nf + a.n_out;
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
        if (cfg->hidden <= 2) {
            static bool attr = SPILL;
            cs_lds_attr(&k_ccn1_small_batch<CS_CF, 2, XENT, SPILL>, attr);
            HGNN_KLAUNCH((k_ccn1_small_batch<CS_CF, 2, XENT, SPILL>), dim3(B), dim3(CS_NT), lds, s, a, t);
        } else {
            static bool attr = SPILL;
            cs_lds_attr(&k_ccn1_small_batch<CS_CF, CS_CF, XENT, SPILL>, attr);
            HGNN_KLAUNCH((k_ccn1_small_batch<CS_CF, CS_CF, XENT, SPILL>), dim3(B), dim3(CS_NT), lds, s, a, t);
        }
        HGNN_LAUNCH_CHECK();
        HGNN_KLAUNCH((k_ccn1_small_apply<OPT, XENT>), dim3((outs + 3) / 4), dim3(256), 0, s, base, t, q);
        HGNN_LAUNCH_CHECK();
    }
    return HGNN_OK;
}

}  // namespace
}  // namespace hgnn
