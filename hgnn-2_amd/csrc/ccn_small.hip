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
// The device functions (cs_*) are in ccn_small.h, which ccn_small_batch.hip (the mini-batch training step) shares.
#include <cstdio>

#include "ccn_small.h"

namespace hgnn {
namespace {

template <int CF>
__global__ void __launch_bounds__(CS_NT) k_ccn1_small_fwd(CsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    __shared__ uint32_t sbad;
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const CsLds s = cs_carve(lds, a, false);
    CS_STAMP(0);
    if (threadIdx.x == 0) sbad = 0;
    uint32_t bad = 0;
    const int n = cs_nodes(a, b, bad);
    cs_stage(a, b, n, s, s.F);
    CS_STAMP(1);
    bad |= cs_plan(n, s, s.F);
    CS_STAMP(2);
    const float* Xg = s.Xs;
    const int h = a.h, f = a.f, nf = f + a.L * h;
    const int G = s.off1[66];
    // level 0 of the readout: sum_i d_i X[i]  (utils_ccn.py:212-216 tiles X[i] d_i times)
    cs_colsum<CF>(s, n, f, 0, [&](int r, int c) { return (double)s.deg[r] * (double)Xg[r * f + c]; });
    CS_STAMP(3);
    const int rows = s.off1[n];
    const float* fin = nullptr;
    for (int l = 0; l < a.L; ++l) {
        const int cin = l == 0 ? f : h;
        float* fout = s.F + (size_t)(l & 1) * a.rcap * h;
        const float* Wl = s.Ws + cs_woff(l, f, h);
        if (cin <= 2) cs_fwd_level<2>(s, n, G, Xg, fin, cin, Wl, h, fout);
        else cs_fwd_level<CF>(s, n, G, Xg, fin, cin, Wl, h, fout);
        __syncthreads();
        CS_STAMP(4 + 2 * l);
        cs_colsum<CF>(s, rows, h, f + l * h, [&](int r, int c) { return (double)fout[r * h + c]; });
        CS_STAMP(5 + 2 * l);
        fin = fout;
    }
    for (int k = threadIdx.x; k < nf; k += CS_NT) a.feat[(long long)b * nf + k] = s.vec[k];
    // out = fc(feat) in fp64 (k_ccn_readout's order)
    for (int o = 0; o < a.n_out; ++o) {
        const double v = cs_fc(a, s, o, nf);
        if (threadIdx.x == 0) a.out[(long long)b * a.n_out + o] = (float)(v + (double)a.fcb[o]);
    }
    CS_STAMP(30);
    bad = wave_or(bad);
    if (lane == 0 && bad) atomicOr(&sbad, bad);
    __syncthreads();
    if (threadIdx.x == 0 && sbad) a.err[0] = a.tag * 256 + (int)sbad;  // vector store (host-mapped word)
    CS_STAMP(31);
}

template <int CF, int CH>
__global__ void __launch_bounds__(CS_NT) k_ccn1_small_bwd(CsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int b = blockIdx.x;
    const CsLds s = cs_carve(lds, a, true);
    uint32_t bad = 0;
    const int n = cs_nodes(a, b, bad);
    cs_stage(a, b, n, s, s.F);
    (void)cs_plan(n, s, s.F);  // the forward reported the batch's validation bits
    const float* Xg = s.Xs;
    const int h = a.h, f = a.f, L = a.L, nf = f + L * h;
    const int G = s.off1[66];
    // the levels again, all kept
    for (int l = 0; l < L; ++l) {
        const int cin = l == 0 ? f : h;
        const float* fin = l == 0 ? nullptr : s.F + (size_t)(l - 1) * a.rcap * h;
        float* fout = s.F + (size_t)l * a.rcap * h;
        const float* Wl = s.Ws + cs_woff(l, f, h);
        if (cin <= 2) cs_fwd_level<2>(s, n, G, Xg, fin, cin, Wl, h, fout);
        else cs_fwd_level<CF>(s, n, G, Xg, fin, cin, Wl, h, fout);
        __syncthreads();
    }
    // dsum[k] = sum_o dout[b][o] fcw[o][k] (k_ccn_readout_bwd's order); one graph: the fc gradients here
    const float* dob = a.dout + (long long)b * a.n_out;
    for (int k = threadIdx.x; k < nf; k += CS_NT) {
        float t = 0.f;
        for (int o = 0; o < a.n_out; ++o) t = fmaf(dob[o], a.fcw[o * nf + k], t);
        s.vec[k] = t;
    }
    if (a.bs == 1)
        for (int w = threadIdx.x; w < a.n_out * nf + a.n_out; w += CS_NT) {
            if (w < a.n_out * nf) a.gfcw[w] = (float)((double)dob[w / nf] * (double)a.feat[w % nf]);
            else a.gfcb[w - a.n_out * nf] = (float)(double)dob[w - a.n_out * nf];
        }
    __syncthreads();
    float* dFc = s.dF0;
    float* dFn = s.dF1;
    for (int l = L - 1; l >= 0; --l) {
        if ((l == 0 ? f : h) <= 2) cs_bwd_level<2, CH>(a, s, b, l, n, G, Xg, dFc, dFn);
        else cs_bwd_level<CF, CH>(a, s, b, l, n, G, Xg, dFc, dFn);
        float* t = dFc;
        dFc = dFn;
        dFn = t;
    }
    for (int e = threadIdx.x; e < (a.nmax - n) * f; e += CS_NT) a.dX[((long long)b * a.nmax + n) * f + e] = 0.f;
}

// The per-graph training loop of scripts/train_ccn.py:31-73 in one dispatch: one workgroup runs forward, loss,
// backward and the Adamax step of graph 0, then of graph 1, ... (per-graph SGD is sequential: graph g + 1 reads
// the weights graph g wrote).  The pieces are the forward's and the backward's (cs_* above, the one-graph form:
// CsArgs::bs = 1), k_mse_loss's loss and meters and k_optim's element update (adamax_elem, sgd_elem or adam_elem).
constexpr int CS_TMAX = 2 * CS_LMAX + 2;    // parameter tensors: level weights and biases, fc weight and bias
constexpr int CS_TRAIN_GMAX = 4096;         // graphs per dispatch
constexpr int CS_OMAX = CS_NW * CS_PMAX;    // n_out bound: out / dout of the graph live in CsLds::red

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
template <int CF, int CH, bool XENT, int OPT>
__global__ void __launch_bounds__(CS_NT) k_ccn1_small_train(CsArgs a, CsTrain t) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    __shared__ uint32_t sbad;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const CsLds s = cs_carve(lds, a, true);
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
        // 1. stage (the current weights) and plan
        if (threadIdx.x == 0) sbad = 0;
        uint32_t bad = 0;
        const int n = cs_nodes(a, g, bad);
        cs_stage(a, g, n, s, s.F);
        bad |= cs_plan(n, s, s.F);
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
            if (cin <= 2) cs_fwd_level<2>(s, n, G, Xg, fin, cin, Wl, h, fout);
            else cs_fwd_level<CF>(s, n, G, Xg, fin, cin, Wl, h, fout);
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
        // 4. backward, k_ccn1_small_bwd's one-graph form: fc gradients from dout and feat, dsum, the levels
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
            if ((l == 0 ? f : h) <= 2) cs_bwd_level<2, CH, false>(a, s, g, l, n, G, Xg, dFc, dFn);
            else cs_bwd_level<CF, CH, false>(a, s, g, l, n, G, Xg, dFc, dFn);
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

// Batches: parameter gradient = sum over graphs in fp64, one wave per entry (the level entries, then fc
// weight and bias from dout and the readout features, k_ccn_readout_bwd's order).
__global__ void __launch_bounds__(256) k_ccn1_small_reduce(CsArgs a) {
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int h = a.h, f = a.f, L = a.L, nf = f + L * h;
    const int p0 = h * 2 * f + h, p1 = h * 2 * h + h, ptot = p0 + (L - 1) * p1;
    if (w >= ptot + a.n_out * nf + a.n_out) return;
    double s = 0.0;
    if (w < ptot) {
        for (int b = lane; b < a.bs; b += 64) s += (double)a.ppart[(long long)b * ptot + w];
    } else if (w < ptot + a.n_out * nf) {
        const int o = (w - ptot) / nf, k = (w - ptot) % nf;
        for (int b = lane; b < a.bs; b += 64) s += (double)a.dout[b * a.n_out + o] * (double)a.feat[(long long)b * nf + k];
    } else {
        const int o = w - ptot - a.n_out * nf;
        for (int b = lane; b < a.bs; b += 64) s += (double)a.dout[b * a.n_out + o];
    }
    s = wave_sum_d(s);
    if (lane != 0) return;
    if (w < ptot) {
        const int l = w < p0 ? 0 : 1 + (w - p0) / p1;
        const int p = l == 0 ? w : (w - p0) % p1;
        const int k2 = 2 * (l == 0 ? f : h);
        if (p < h * k2) a.gW[l][p] = (float)s;
        else a.gB[l][p - h * k2] = (float)s;
    } else if (w < ptot + a.n_out * nf) {
        a.gfcw[w - ptot] = (float)s;
    } else {
        a.gfcb[w - ptot - a.n_out * nf] = (float)s;
    }
}

bool cs_ok(const hgnn_ccn_config* c) {
    return c && c->order == 1 && c->bs > 0 && c->nmax > 0 && c->nmax <= 64 && c->f_in > 0 && c->f_in <= CS_CF &&
           c->hidden > 0 && c->hidden <= CS_CF && c->layers >= 1 && c->layers <= CS_LMAX && c->n_out > 0 &&
           cs_lds_bytes(c->nmax * c->nmax, c->f_in, c->hidden, c->layers, true) <= CS_LDS_MAX;
}

size_t cs_ptot(const hgnn_ccn_config* c) {
    const int h = c->hidden, f = c->f_in;
    return (size_t)(h * 2 * f + h) + (size_t)(c->layers - 1) * (h * 2 * h + h);
}

CsArgs cs_args(const hgnn_ccn_config* c, const float* X, const float* adj, const int64_t* nb,
               const float* const* params, void* ws) {
    CsArgs a{};
    a.adj = adj;
    a.n_batch = nb;
    a.X = X;
    a.bs = c->bs;
    a.nmax = c->nmax;
    a.f = c->f_in;
    a.h = c->hidden;
    a.L = c->layers;
    a.n_out = c->n_out;
    a.rcap = c->nmax * c->nmax;
    for (int l = 0; l < c->layers; ++l) {
        a.W[l] = params[2 * l];
        a.B[l] = params[2 * l + 1];
    }
    a.fcw = params[2 * c->layers];
    a.fcb = params[2 * c->layers + 1];
    const int nf = c->f_in + c->layers * c->hidden;
    a.feat = static_cast<float*>(ws);
    if (ws) a.ppart = reinterpret_cast<float*>(static_cast<char*>(ws) + (4 * (size_t)c->bs * nf + 255) / 256 * 256);
    return a;
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

namespace {

// Every training entry: the argument checks and the launch; XENT picks the loss stage (and ignores the target
// statistics), OPT the optimizer stage; cstride is the row length of d_clr (1: the Adamax entries' step sizes, 2:
// the _opt entry's per-step pairs).
template <bool XENT, int OPT>
int cs_train(const hgnn_ccn_config* cfg, const float* d_X, const float* d_adj, const int64_t* d_n_batch,
             const float* d_y, double t_mean, double t_std, float* const* params, float* const* grads,
             float* const* exp_avg, float* const* exp_inf, const float* d_clr, int cstride, double beta1,
             double beta2, double eps, double weight_decay, float* d_stats, float* d_out, int32_t* d_err,
             int32_t tag, void* stream) {
    constexpr bool TWO = OPT != HGNN_OPT_SGD;  // whether the second state array is used
    if (!hgnn_ccn_small_train_supported(cfg)) return HGNN_ERR_UNSUPPORTED;
    if (!d_X || !d_adj || !d_y || !params || !grads || !exp_avg || (TWO && !exp_inf) || !d_clr || !d_stats ||
        !d_out || !d_err || tag <= 0 || tag >= (1 << 23) || cfg->bs < 1 || cfg->bs > CS_TRAIN_GMAX ||
        (XENT && cfg->n_out < 2))
        return HGNN_ERR_ARG;
    const int nt = 2 * cfg->layers + 2;
    for (int k = 0; k < nt; ++k)
        if (!params[k] || !grads[k] || !exp_avg[k] || (TWO && !exp_inf[k])) return HGNN_ERR_ARG;
    CsArgs a = cs_args(cfg, d_X, d_adj, d_n_batch, params, nullptr);
    a.bs = 1;  // the one-graph form of the backward: gradients written directly; the kernel passes b = g
    a.out = d_out;
    a.err = d_err;
    a.tag = tag;
    for (int l = 0; l < cfg->layers; ++l) {
        a.gW[l] = grads[2 * l];
        a.gB[l] = grads[2 * l + 1];
    }
    a.gfcw = grads[2 * cfg->layers];
    a.gfcb = grads[2 * cfg->layers + 1];
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
    const size_t lds = cs_lds_bytes(a.rcap, a.f, a.h, a.L, true);
    hipStream_t s = (hipStream_t)stream;
    if (cfg->hidden <= 2) {
        static bool attr = false;
        cs_lds_attr(&k_ccn1_small_train<CS_CF, 2, XENT, OPT>, attr);
        HGNN_KLAUNCH((k_ccn1_small_train<CS_CF, 2, XENT, OPT>), dim3(1), dim3(CS_NT), lds, s, a, t);
    } else {
        static bool attr = false;
        cs_lds_attr(&k_ccn1_small_train<CS_CF, CS_CF, XENT, OPT>, attr);
        HGNN_KLAUNCH((k_ccn1_small_train<CS_CF, CS_CF, XENT, OPT>), dim3(1), dim3(CS_NT), lds, s, a, t);
    }
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

}  // namespace

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
    const int nf = cfg->f_in + cfg->layers * cfg->hidden;
    return (4 * (size_t)cfg->bs * nf + 255) / 256 * 256 + (cfg->bs > 1 ? 4 * (size_t)cfg->bs * cs_ptot(cfg) : 0);
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
    CsArgs a = cs_args(cfg, d_X, d_adj, d_n_batch, params, workspace);
    a.out = d_out;
    a.err = d_err;
    a.tag = tag;
    const size_t lds = cs_lds_bytes(a.rcap, a.f, a.h, a.L, false);
    static bool attr = false;
    cs_lds_attr(&k_ccn1_small_fwd<CS_CF>, attr);
    const bool prof = switches().ccn_small_prof;
    static unsigned long long* dprof = nullptr;
    if (prof) {
        if (!dprof) HGNN_HOST_CHECK(hipMalloc(&dprof, 32 * 8));
        HGNN_HOST_CHECK(hipMemsetAsync(dprof, 0, 32 * 8, (hipStream_t)stream));
        a.prof = dprof;
    }
    HGNN_KLAUNCH(k_ccn1_small_fwd<CS_CF>, dim3(cfg->bs), dim3(CS_NT), lds, (hipStream_t)stream, a);
    HGNN_LAUNCH_CHECK();
    if (prof) {  // diagnostic: phase cycles of graph 0 (synchronises)
        unsigned long long hp[32];
        HGNN_HOST_CHECK(hipMemcpyAsync(hp, dprof, sizeof(hp), hipMemcpyDeviceToHost, (hipStream_t)stream));
        HGNN_HOST_CHECK(hipStreamSynchronize((hipStream_t)stream));
        fprintf(stderr, "ccn_small_fwd cycles:");
        for (int k = 1; k < 32; ++k)
            if (hp[k]) fprintf(stderr, " %d:%llu", k, hp[k] - hp[0]);
        fprintf(stderr, "\n");
    }
    return HGNN_OK;
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
    hipStream_t s = (hipStream_t)stream;
    CsArgs a = cs_args(cfg, d_X, d_adj, d_n_batch, params, workspace);
    a.dout = d_dout;
    a.dX = d_dX;
    for (int l = 0; l < cfg->layers; ++l) {
        a.gW[l] = grads[2 * l];
        a.gB[l] = grads[2 * l + 1];
    }
    a.gfcw = grads[2 * cfg->layers];
    a.gfcb = grads[2 * cfg->layers + 1];
    const size_t lds = cs_lds_bytes(a.rcap, a.f, a.h, a.L, true);
    if (cfg->hidden <= 2) {
        static bool attr = false;
        cs_lds_attr(&k_ccn1_small_bwd<CS_CF, 2>, attr);
        HGNN_KLAUNCH((k_ccn1_small_bwd<CS_CF, 2>), dim3(cfg->bs), dim3(CS_NT), lds, s, a);
    } else {
        static bool attr = false;
        cs_lds_attr(&k_ccn1_small_bwd<CS_CF, CS_CF>, attr);
        HGNN_KLAUNCH((k_ccn1_small_bwd<CS_CF, CS_CF>), dim3(cfg->bs), dim3(CS_NT), lds, s, a);
    }
    HGNN_LAUNCH_CHECK();
    if (cfg->bs > 1) {
        const int nf = cfg->f_in + cfg->layers * cfg->hidden;
        const int outs = (int)cs_ptot(cfg) + cfg->n_out * nf + cfg->n_out;
        HGNN_KLAUNCH(k_ccn1_small_reduce, dim3((outs + 3) / 4), dim3(256), 0, s, a);
        HGNN_LAUNCH_CHECK();
    }
    return HGNN_OK;
}

int hgnn_ccn_small_train_supported(const hgnn_ccn_config* cfg) {
    if (!cfg) return 0;
    hgnn_ccn_config one = *cfg;  // a property of the model and nmax: the dispatch walks its graphs one at a time
    one.bs = 1;
    return cs_ok(&one) && one.n_out <= CS_OMAX ? 1 : 0;
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
