// The CCN-1D small-graph kernels that own the carve (one-shot forward and backward as lists of ccn_small.h's stages, the
// per-graph training loop with its stages written out) and their host calls, as templates on SPILL: ccn_small.hip instantiates the LDS form,
// ccn_small_spill.hip the form whose row arrays live in a global region (ccn_small.h CsSpillArgs).  Two translation
// units, so that neither form's callers touch the other's inlining.  k_ccn1_small_reduce does not touch the row arrays:
// it is compiled once, in ccn_small.hip, behind cs_launch_reduce.
#pragma once
#include <cstdio>

#include "ccn_small.h"

namespace hgnn {

// The batch backward's sum of the per-graph partials into the gradients (ccn_small.hip)
int cs_launch_reduce(const hgnn_ccn_config* cfg, const CsArgs& a, hipStream_t s);

namespace {

template <int CF, bool SPILL = false>
__global__ void __launch_bounds__(CS_NT) k_ccn1_small_fwd(CsArgsT<SPILL> a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    __shared__ uint32_t sbad;
    const int b = blockIdx.x;
    const CsLds s = cs_carve<SPILL>(lds, a, false);
    float* As = cs_adj<SPILL>(lds, s);
    CS_STAMP(0);
    if (threadIdx.x == 0) sbad = 0;
    uint32_t bad = 0;
    const int n = cs_open<true>(a, b, s, As, bad);
    const float* Xg = s.Xs;
    const int h = a.h, f = a.f, nf = f + a.L * h;
    const int G = s.off1[66];
    // level 0 of the readout: sum_i d_i X[i]  (utils_ccn.py:212-216 tiles X[i] d_i times)
    cs_colsum<CF>(s, n, f, 0, [&](int r, int c) { return (double)s.deg[r] * (double)Xg[r * f + c]; });
    CS_STAMP(3);
    const int rows = s.off1[n];
    const float* fin = nullptr;
    // its own level loop, not cs_levels_keep / cs_readout_sums: two ping-pong level buffers (the forward's LDS figure),
    // each level's column sums between the levels, the phase stamps
    for (int l = 0; l < a.L; ++l) {
        const int cin = l == 0 ? f : h;
        float* fout = s.F + (size_t)(l & 1) * a.rcap * h;
        const float* Wl = s.Ws + cs_woff(l, f, h);
        if (cin <= 2) cs_fwd_level<2, SPILL>(s, n, G, Xg, fin, cin, Wl, h, fout);
        else cs_fwd_level<CF, SPILL>(s, n, G, Xg, fin, cin, Wl, h, fout);
        __syncthreads();
        CS_STAMP(4 + 2 * l);
        cs_colsum<CF>(s, rows, h, f + l * h, [&](int r, int c) { return (double)fout[r * h + c]; });
        CS_STAMP(5 + 2 * l);
        fin = fout;
    }
    for (int k = threadIdx.x; k < nf; k += CS_NT) a.feat[(long long)b * nf + k] = s.vec[k];
    cs_out_row(a, s, nf, a.n_out, a.out + (long long)b * a.n_out, nullptr);
    CS_STAMP(30);
    cs_report(bad, sbad);
    __syncthreads();
    if (threadIdx.x == 0 && sbad) a.err[0] = a.tag * 256 + (int)sbad;  // vector store (host-mapped word)
    CS_STAMP(31);
}

template <int CF, int CH, bool SPILL = false>
__global__ void __launch_bounds__(CS_NT) k_ccn1_small_bwd(CsArgsT<SPILL> a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int b = blockIdx.x;
    const CsLds s = cs_carve<SPILL>(lds, a, true);
    float* As = cs_adj<SPILL>(lds, s);
    uint32_t bad = 0;  // discarded: the forward reported the batch's validation bits
    const int n = cs_open(a, b, s, As, bad);
    const float* Xg = s.Xs;
    const int nf = a.f + a.L * a.h;
    const int G = s.off1[66];
    cs_levels_keep<CF, SPILL>(a, s, n, G, Xg);
    // dsum; one graph: the fc gradients here (a batch's come from k_ccn1_small_reduce)
    const float* dob = a.dout + (long long)b * a.n_out;
    cs_dsum(a, s, dob, nf);
    if (a.bs == 1) cs_fc_grads(a, dob, a.feat, nf);
    __syncthreads();
    cs_backward<CF, CH, true, SPILL>(a, s, b, n, G, Xg);
    for (int e = threadIdx.x; e < (a.nmax - n) * a.f; e += CS_NT) a.dX[((long long)b * a.nmax + n) * a.f + e] = 0.f;
}

// The per-graph training loop of scripts/train_ccn.py:31-73 in one dispatch: one workgroup runs forward, loss,
// backward and the Adamax step of graph 0, then of graph 1, ... (per-graph SGD is sequential: graph g + 1 reads
// the weights graph g wrote).  The pieces are the forward's and the backward's (ccn_small.h's stages, the one-graph
// form: CsArgs::bs = 1), k_mse_loss's loss and meters and k_optim's element update (adamax_elem, sgd_elem or adam_elem).
struct CsTrain {
    const float* y;       // (G, n_out) raw targets
    const float* clr;     // the scalars of the dispatch's k-th applied step at clr[k * cstride] (and + 1: Adam's
                          // second); a rejected graph takes none
    float t_mean, t_div;  // yn = (y - mean) / div, div = std + 1e-8
    OptScalars h;         // the optimizer's fixed scalars (kernels.h)
    // the parameters (mutable: CsArgs' W / B / fcw / fcb alias them; none of these is const __restrict__, so
    // the re-staging of the next graph reads them by vector loads, after the fence) and the optimizer state
    float* p[CS_TMAX];
    float* m[CS_TMAX];
    float* u[CS_TMAX];    // SGD: not touched
    float* stats;         // [4] loss, mae and their RunningAverages
    int G;
    int cstride;          // 1: clr is (G,) lr / (1 - beta1^t); 2: the (G, 2) rows of hgnn_ccn_small_train_opt
};

// a word this block wrote earlier in the dispatch, read at a wave-uniform address: an agent-scope load keeps it
// on the vector path (the scalar cache is not coherent with the block's own stores)
__device__ __forceinline__ float cs_fresh(const float* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// XENT: the reference's `mean == 0` branch (train_ccn.py:39-41, 56-57) -- y[g] is a class index, the loss is
// nn.CrossEntropyLoss on the graph's row (xent_row, k_xent_loss's arithmetic with n = 1) and the MAE meters are
// never written.  A template parameter, so the MSE instantiations keep their instructions.
// OPT: the optimizer of stage 5 (HGNN_OPT_*), a template parameter for the same reason: the Adamax instantiations
// keep theirs.
template <int CF, int CH, bool XENT, int OPT, bool SPILL = false>
__global__ void __launch_bounds__(CS_NT) k_ccn1_small_train(CsArgsT<SPILL> a, CsTrain t) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    __shared__ uint32_t sbad;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const CsLds s = cs_carve<SPILL>(lds, a, true);
    float* As = cs_adj<SPILL>(lds, s);
    const int h = a.h, f = a.f, L = a.L, nf = f + L * h, n_out = a.n_out;
    const int nw = cs_woff(L, f, h), ntot = nw + n_out * nf + n_out;
    const float* Xg = s.Xs;
    float run_l = 0.f, run_m = 0.f;  // the RunningAverages (thread 0)
    int applied = 0;                 // optimizer steps taken so far in this dispatch
    if (threadIdx.x == 0) {
        run_l = t.stats[2];
        run_m = t.stats[3];
    }
    for (int g = 0; g < t.G; ++g) {
        // 1. stage (the current weights) and plan.  Stages 1, 2 and 5 are written out too (they mirror cs_open /
        // cs_report, cs_levels_keep, cs_readout_sums, cs_out_row and cs_param_elem; a change there comes here): as calls
        // they change this kernel's instruction stream, and the classification loop measured 0.6 % slower
        if (threadIdx.x == 0) sbad = 0;
        uint32_t bad = 0;
        const int n = cs_nodes(a, g, bad);
        cs_stage(a, g, n, s, As);
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
        // the readout features stay in vec for the fc gradient; out[g] is what the graph saw before its update
        for (int o = 0; o < n_out; ++o) {
            const double v = cs_fc(a, s, o, nf);
            if (threadIdx.x == 0) {
                const float ov = (float)(v + (double)cs_fresh(a.fcb + o));
                a.out[(long long)g * n_out + o] = ov;
                s.red[o] = ov;
            }
        }
        // a target that is no class index rejects the graph like a validation bit: set before the barrier the
        // read of sbad follows, so the branch below is block-uniform
        int ti = 0;
        if constexpr (XENT) {
            if (threadIdx.x == 0 && !xent_target(t.y[g], n_out, ti)) atomicOr(&sbad, (uint32_t)ERR_CLASS_TARGET);
        }
        __syncthreads();
        const uint32_t gbad = sbad;
        __syncthreads();
        if (gbad) {  // a rejected graph: reported, no loss, no gradients, no step
            if (threadIdx.x == 0) a.err[0] = a.tag * 256 + (int)gbad;  // vector store (host-mapped word)
            continue;
        }
        // 3. loss, meters and dout; dout replaces out in red
        if constexpr (XENT) {
            // k_xent_loss's arithmetic on one row (n = 1: the mean is the row's loss, 1 / n = 1.0f), by one thread
            // in the row function's serial order; stats[1] and stats[3] are never written (train_ccn.py:54-57)
            if (threadIdx.x == 0) {
                const float loss = (float)(double)xent_row(s.red, ti, n_out, 1.0f, s.red);
                run_l = run_l == 0.f ? loss : 0.9f * loss + 0.1f * run_l;
                t.stats[0] = loss;
                t.stats[2] = run_l;
            }
            __syncthreads();
        } else {
            // k_mse_loss's arithmetic on the normalised target
            double se = 0.0, ae = 0.0;
            if (threadIdx.x < CS_RT)
                for (int i = threadIdx.x; i < n_out; i += CS_RT) {
                    const float yn = (t.y[(long long)g * n_out + i] - t.t_mean) / t.t_div;
                    const float d = s.red[i] - yn;
                    se += (double)d * d;
                    ae += fabs((double)d);
                    s.red[i] = 2.0f * d / (float)n_out;
                }
            se = wave_sum_d(se);
            ae = wave_sum_d(ae);
            if (lane == 0) {
                s.dred[wv] = se;
                s.dred[CS_NW + wv] = ae;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                double S = 0.0, A = 0.0;
                for (int i = 0; i < CS_RT / 64; ++i) {
                    S += s.dred[i];
                    A += s.dred[CS_NW + i];
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
        // 4. backward, k_ccn1_small_bwd's one-graph form: fc gradients from dout and feat, dsum, the levels.  Written
        // out: cs_fc_grads, cs_dsum and cs_backward<CF, CH, false, SPILL> as calls cost the SPILL instantiations of
        // CH = CS_CF 4 bytes of scratch per lane (profiles/ccn1_small_stages_resources.txt); a change there comes here
        const float* dob = s.red;
        for (int w = threadIdx.x; w < n_out * nf + n_out; w += CS_NT) {
            if (w < n_out * nf) a.gfcw[w] = (float)((double)dob[w / nf] * (double)s.vec[w % nf]);
            else a.gfcb[w - n_out * nf] = (float)(double)dob[w - n_out * nf];
        }
        __syncthreads();
        for (int k = threadIdx.x; k < nf; k += CS_NT) {
            float v = 0.f;
            for (int o = 0; o < n_out; ++o) v = fmaf(dob[o], a.fcw[o * nf + k], v);
            s.vec[k] = v;
        }
        __syncthreads();
        float* dFc = s.dF0;
        float* dFn = s.dF1;
        for (int l = L - 1; l >= 0; --l) {
            if ((l == 0 ? f : h) <= 2) cs_bwd_level<2, CH, false, SPILL>(a, s, g, l, n, G, Xg, dFc, dFn);
            else cs_bwd_level<CF, CH, false, SPILL>(a, s, g, l, n, G, Xg, dFc, dFn);
            float* x = dFc;
            dFc = dFn;
            dFn = x;
        }
        // 5. the optimizer over every parameter element (flat: the levels in Ws' order, then fc weight and bias), on
        // the gradients other threads have just written
        __threadfence();
        __syncthreads();
        const float* sc = t.clr + (long long)applied++ * t.cstride;
        const float clr = sc[0];
        float c1 = 0.f;
        if constexpr (OPT == HGNN_OPT_ADAM) c1 = sc[1];
        for (int e = threadIdx.x; e < ntot; e += CS_NT) {
            int ti, q;
            const float* gp;
            if (e < nw) {
                int l = 0;
                while (l + 1 < L && e >= cs_woff(l + 1, f, h)) ++l;
                q = e - cs_woff(l, f, h);
                const int hk = h * 2 * (l == 0 ? f : h);
                const bool isw = q < hk;
                ti = 2 * l + (isw ? 0 : 1);
                gp = isw ? a.gW[l] : a.gB[l];
                q = isw ? q : q - hk;
            } else if (e < nw + n_out * nf) {
                ti = 2 * L;
                gp = a.gfcw;
                q = e - nw;
            } else {
                ti = 2 * L + 1;
                gp = a.gfcb;
                q = e - nw - n_out * nf;
            }
            optim_at<OPT>(t.p[ti], gp[q], t.m[ti], t.u[ti], q, clr, c1, t.h);
        }
        // 6. the new weights visible to the next graph's staging
        __threadfence();
        __syncthreads();
    }
}

// The one-shot forward behind hgnn_ccn_small_forward / hgnn_ccn_small_spill_forward, their checks done.  SPILL: `ws`
// starts with cfg->bs row regions.
template <bool SPILL>
int cs_forward_call(const hgnn_ccn_config* cfg, const float* d_X, const float* d_adj, const int64_t* d_n_batch,
                    const float* const* params, void* ws, int32_t* d_err, int32_t tag, float* d_out, hipStream_t s) {
    CsArgsT<SPILL> a = cs_args<SPILL>(cfg, d_X, d_adj, d_n_batch, params, ws, cfg->bs);
    a.out = d_out;
    a.err = d_err;
    a.tag = tag;
    const size_t lds = cs_lds_for<SPILL>(a, false);
    static bool attr = SPILL;
    cs_lds_attr(&k_ccn1_small_fwd<CS_CF, SPILL>, attr);
    if constexpr (!SPILL) {
        if (switches().ccn_small_prof) {  // diagnostic: phase cycles of graph 0 (synchronises)
            static unsigned long long* dprof = nullptr;
            if (!dprof) HGNN_HOST_CHECK(hipMalloc(&dprof, 32 * 8));
            HGNN_HOST_CHECK(hipMemsetAsync(dprof, 0, 32 * 8, s));
            a.prof = dprof;
            HGNN_KLAUNCH((k_ccn1_small_fwd<CS_CF, SPILL>), dim3(cfg->bs), dim3(CS_NT), lds, s, a);
            HGNN_LAUNCH_CHECK();
            unsigned long long hp[32];
            HGNN_HOST_CHECK(hipMemcpyAsync(hp, dprof, sizeof(hp), hipMemcpyDeviceToHost, s));
            HGNN_HOST_CHECK(hipStreamSynchronize(s));
            fprintf(stderr, "ccn_small_fwd cycles:");
            for (int k = 1; k < 32; ++k)
                if (hp[k]) fprintf(stderr, " %d:%llu", k, hp[k] - hp[0]);
            fprintf(stderr, "\n");
            return HGNN_OK;
        }
    }
    HGNN_KLAUNCH((k_ccn1_small_fwd<CS_CF, SPILL>), dim3(cfg->bs), dim3(CS_NT), lds, s, a);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

// The one-shot backward behind hgnn_ccn_small_backward / hgnn_ccn_small_spill_backward
template <bool SPILL>
int cs_backward_call(const hgnn_ccn_config* cfg, const float* d_X, const float* d_adj, const int64_t* d_n_batch,
                     const float* const* params, void* ws, const float* d_dout, float* const* grads, float* d_dX,
                     hipStream_t s) {
    CsArgsT<SPILL> a = cs_args<SPILL>(cfg, d_X, d_adj, d_n_batch, params, ws, cfg->bs);
    a.dout = d_dout;
    a.dX = d_dX;
    cs_set_grads(a, grads);
    cs_launch_ch<&k_ccn1_small_bwd<CS_CF, 2, SPILL>, &k_ccn1_small_bwd<CS_CF, CS_CF, SPILL>, SPILL>(
        cfg->hidden, cfg->bs, cs_lds_for<SPILL>(a, true), s, a);
    HGNN_LAUNCH_CHECK();
    return cfg->bs > 1 ? cs_launch_reduce(cfg, a, s) : HGNN_OK;
}

// Every training entry: the argument checks and the launch; XENT picks the loss stage (and ignores the target
// statistics), OPT the optimizer stage; cstride is the row length of d_clr (1: the Adamax entries' step sizes, 2:
// the _opt entry's per-step pairs).  SPILL: `ws` holds the loop's one row region, reused graph after graph.
template <bool XENT, int OPT, bool SPILL = false>
int cs_train(const hgnn_ccn_config* cfg, const float* d_X, const float* d_adj, const int64_t* d_n_batch,
             const float* d_y, double t_mean, double t_std, float* const* params, float* const* grads,
             float* const* exp_avg, float* const* exp_inf, const float* d_clr, int cstride, double beta1,
             double beta2, double eps, double weight_decay, float* d_stats, float* d_out, int32_t* d_err,
             int32_t tag, void* stream, void* ws = nullptr) {
    constexpr bool TWO = OPT != HGNN_OPT_SGD;  // whether the second state array is used
    if (!cs_train_ok<SPILL>(cfg)) return HGNN_ERR_UNSUPPORTED;
    if (SPILL && !ws) return HGNN_ERR_ARG;
    if (!d_X || !d_adj || !d_y || !params || !grads || !exp_avg || (TWO && !exp_inf) || !d_clr || !d_stats ||
        !d_out || !d_err || tag <= 0 || tag >= (1 << 23) || cfg->bs < 1 || cfg->bs > CS_TRAIN_GMAX ||
        (XENT && cfg->n_out < 2))
        return HGNN_ERR_ARG;
    const int nt = 2 * cfg->layers + 2;
    for (int k = 0; k < nt; ++k)
        if (!params[k] || !grads[k] || !exp_avg[k] || (TWO && !exp_inf[k])) return HGNN_ERR_ARG;
    CsArgsT<SPILL> a = cs_args<SPILL>(cfg, d_X, d_adj, d_n_batch, params, nullptr);
    if constexpr (SPILL) a.rows = static_cast<float*>(ws);
    a.bs = 1;  // the one-graph form of the backward: gradients written directly; the kernel passes b = g
    a.out = d_out;
    a.err = d_err;
    a.tag = tag;
    cs_set_grads(a, grads);
    CsTrain t{};
    t.y = d_y;
    t.clr = d_clr;
    t.cstride = cstride;
    // scalars combine in double and reach the kernel as fp32, as the reference's Python floats reach torch
    t.t_mean = (float)t_mean;
    t.t_div = (float)(t_std + 1e-8);  // scripts/train_ccn.py:42
    t.h = opt_scalars(OPT, beta1, beta2, eps, weight_decay);
    for (int k = 0; k < nt; ++k) {
        t.p[k] = params[k];
        t.m[k] = exp_avg[k];
        t.u[k] = TWO ? exp_inf[k] : nullptr;
    }
    t.stats = d_stats;
    t.G = cfg->bs;
    cs_launch_ch<&k_ccn1_small_train<CS_CF, 2, XENT, OPT, SPILL>, &k_ccn1_small_train<CS_CF, CS_CF, XENT, OPT, SPILL>,
                 SPILL>(cfg->hidden, 1, cs_lds_for<SPILL>(a, true), (hipStream_t)stream, a, t);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

}  // namespace
}  // namespace hgnn
