// CCN-2D on small graphs (nmax <= 32): one workgroup per graph, every level of a call in one dispatch.
//
// The reference's driver runs CCN_2D one graph per step (scripts/train_ccn.py:31-73: net(X, A + I), loss,
// backward, an optimizer step), and a QM9 graph has at most 29 nodes of degree ~2-6.  The general path
// (ccn*.hip) spends such a call on dispatches: 3 plan kernels, pack, a level kernel per layer, two readout
// kernels forward; the readout backward, per level a node pass, a parameter reduction and a gather, and an
// unpack backward.  Here one 512-thread workgroup per graph
//   * builds the receptive fields in LDS (row bit sets of the adjacency, utils_ccn.py:159-163; degrees,
//     self positions, the exclusive prefixes of d and d^2; every chi position by popcount, 66-106),
//   * runs each level node by node, one wave per node: the promotion, the closed-form collapse6to3 and the
//     Linear + ReLU of k_c2_fwd (utils_ccn.py:281-300, contraction.py:106-121), then the readout
//     (model_ccn.py:102-105) -- forward: one dispatch;
//   * backward: the readout backward, then per level the node pass of k_c2_bwd (dp format, parameter
//     partials), the gather of k_c2_gather (levels >= 1) or the level-0 sum of k_ccn2_dx0 -- one dispatch
//     (+ one reduction over the graphs when bs > 1).
// Same arithmetic in the same order as the general kernels, so outputs, dX and (bs = 1) the parameter
// gradients are those of the general path bit for bit: where k_c2_fwd / k_c2_bwd give the receptive-field
// rows b to four waves (b = w, w + 4, ...) and add the four waves' partials, the node's one wave walks the
// same four row classes one after the other and adds their partials in the same order; where a general
// kernel spreads n^2 entries over 256 threads (e = t, t + 256, ...), the wave walks the four 64-entry
// classes of t likewise.  The helpers the two paths share are in ccn2_shared.h.
//
// Levels F_l, the dp format and the level-0 terms live in a per-graph global workspace region (the rows of
// a graph's levels: sum_i d_i^2 <= nmax^3); plan, weights and per-node scratch in LDS.
//
// The layout and the node functions are in ccn2_small.h, shared with the per-graph training loop
// (ccn2_small_train.hip); this unit holds the one-shot forward and backward kernels and their launches.
#include "ccn2_small.h"

namespace hgnn {
namespace {

template <int CF>
__global__ void __launch_bounds__(Q_NT) k_ccn2_small_fwd(QArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    __shared__ uint32_t sbad;
    __shared__ double sred[4];
    QGraph& g = *reinterpret_cast<QGraph*>(lds);
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    char* wbase = lds + q_al16(sizeof(QGraph)) + (size_t)wv * q_wave_bytes(a.nmax);
    QWave& w = *reinterpret_cast<QWave*>(wbase);
    short* sp = reinterpret_cast<short*>(wbase + q_al16(sizeof(QWave)));
    float* P = reinterpret_cast<float*>(wbase + q_al16(sizeof(QWave)) + q_sp_bytes(a.nmax));
    if (threadIdx.x == 0) sbad = 0;
    uint32_t bad = 0;
    const int n = q_nodes(a, b, bad);
    bad |= q_plan(a, b, n, g);
    const int f = a.f, h = a.h, nf = f + a.L * h;
    float* G = a.gws + (long long)b * a.gstride;
    // level 0 of the readout: sum_i d_i^2 X[i] (utils_ccn.py:167-172 tile X[i] d_i x d_i times)
    q_colsum(g, n, f, 0, [&](int r, int c, double& acc) {
        const double d = g.deg[r];
        const double wgt = d * d;
        acc += wgt * (double)g.Xs[r * f + c];
    });
    for (int l = 0; l < a.L; ++l) {
        const int cin = l == 0 ? f : h;
        float* fout = G + (long long)l * a.r2 * h;
        const float* fin = l == 0 ? nullptr : G + (long long)(l - 1) * a.r2 * h;
        if (l == 0) c2_weights<Q_HC, CF>(reinterpret_cast<float(*)[Q_HC][CF]>(g.wc), a.W[l], cin, 0, h);
        else c2_weights<Q_HC, Q_HC>(reinterpret_cast<float(*)[Q_HC][Q_HC]>(g.wc), a.W[l], cin, 0, h);
        __syncthreads();
        for (int i = wv; i < n; i += Q_NW) {
            if (l == 0) q_node_fwd<CF, 1, true>(a, g, w, sp, P, i, l, fin, cin, fout);
            else q_node_fwd<Q_HC, 8, false>(a, g, w, sp, P, i, l, fin, cin, fout);
        }
        __syncthreads();
        q_colsum(g, n, h, f + l * h, [&](int r, int c, double& acc) { acc += (double)g.nsum[l][r][c]; });
    }
    for (int k = threadIdx.x; k < nf; k += Q_NT) a.feat[(long long)b * nf + k] = g.vec[k];
    // out = fc(feat) in fp64 (k_ccn_readout's order)
    for (int o = 0; o < a.n_out; ++o) {
        double s = 0.0;
        if ((int)threadIdx.x < Q_RT)
            for (int k = threadIdx.x; k < nf; k += Q_RT) s += (double)a.fcw[o * nf + k] * (double)g.vec[k];
        s = wave_sum_d(s);
        __syncthreads();
        if (lane == 0 && wv < 4) sred[wv] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            const double t = sred[0] + sred[1] + sred[2] + sred[3];
            a.out[(long long)b * a.n_out + o] = (float)(t + (double)a.fcb[o]);
        }
    }
    for (int o = 32; o > 0; o >>= 1) bad |= (uint32_t)__shfl_xor((int)bad, o, 64);
    if (lane == 0 && bad) atomicOr(&sbad, bad);
    __syncthreads();
    if (threadIdx.x == 0 && sbad) a.err[0] = a.tag * 256 + (int)sbad;  // vector store (host-mapped word)
}

template <int CF>
__global__ void __launch_bounds__(Q_NT) k_ccn2_small_bwd(QArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    QGraph& g = *reinterpret_cast<QGraph*>(lds);
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    char* wbase = lds + q_al16(sizeof(QGraph)) + (size_t)wv * q_wave_bytes(a.nmax);
    QWave& w = *reinterpret_cast<QWave*>(wbase);
    short* sp = reinterpret_cast<short*>(wbase + q_al16(sizeof(QWave)));
    float* dpL = reinterpret_cast<float*>(wbase + q_al16(sizeof(QWave)) + q_sp_bytes(a.nmax));
    uint32_t bad = 0;
    const int n = q_nodes(a, b, bad);
    (void)q_plan(a, b, n, g);  // the forward reported the batch's validation bits
    const int f = a.f, h = a.h, L = a.L, nf = f + L * h;
    float* G = a.gws + (long long)b * a.gstride;
    float* dA = G + (long long)L * a.r2 * h;
    float* dB = dA + a.r2 * h;
    float* rdp = dB + a.r2 * h;
    float* trd = rdp + a.r1 * h;
    float* g0 = trd + (long long)a.nmax * h;
    // dsum[k] = sum_o dout[b][o] fcw[o][k] (k_ccn_readout_bwd's order)
    const float* dob = a.dout + (long long)b * a.n_out;
    for (int k = threadIdx.x; k < nf; k += Q_NT) {
        float s = 0.f;
        for (int o = 0; o < a.n_out; ++o) s = fmaf(dob[o], a.fcw[o * nf + k], s);
        g.vec[k] = s;
    }
    if (a.bs == 1)  // fc gradients: k_ccn_readout_bwd's wave per output over one graph
        for (int q = wv; q < a.n_out * nf + a.n_out; q += Q_NW) {
            double s = 0.0;
            if (q < a.n_out * nf) {
                const int o = q / nf, k = q % nf;
                if (lane < 1) s += (double)dob[o] * (double)a.feat[k];
            } else if (lane < 1) {
                s += (double)dob[q - a.n_out * nf];
            }
            s = wave_sum_d(s);
            if (lane == 0) {
                if (q < a.n_out * nf) a.gfcw[q] = (float)s;
                else a.gfcb[q - a.n_out * nf] = (float)s;
            }
        }
    __syncthreads();
    float* dcur = dA;
    float* dnext = dB;
    for (int l = L - 1; l >= 0; --l) {
        const int cin = l == 0 ? f : h;
        const int K = 18 * cin, stride = h * K + h;
        float* pl = a.ppart[l];
        const float* Fl = G + (long long)l * a.r2 * h;
        const float* fin = l == 0 ? nullptr : G + (long long)(l - 1) * a.r2 * h;
        const float* dtop = l == L - 1 ? g.vec + f + (L - 1) * h : nullptr;
        if (l == 0) c2_weights<Q_HC, CF>(reinterpret_cast<float(*)[Q_HC][CF]>(g.wc), a.W[l], cin, 0, h);
        else c2_weights<Q_HC, Q_HC>(reinterpret_cast<float(*)[Q_HC][Q_HC]>(g.wc), a.W[l], cin, 0, h);
        __syncthreads();
        for (int i = wv; i < n; i += Q_NW) {
            float* pp = pl + (long long)(g.base + i) * stride;
            if (l == 0) q_node_bwd<CF, 1, true>(a, g, w, sp, dpL, i, dcur, dtop, Fl, fin, cin, rdp, trd, pp, g0);
            else q_node_bwd<Q_HC, 8, false>(a, g, w, sp, dpL, i, dcur, dtop, Fl, fin, cin, rdp, trd, pp, nullptr);
        }
        __syncthreads();
        if (a.bs == 1)  // parameter gradients: k_ccn_param_reduce's order over the graph's nodes
            for (int k = wv; k < stride; k += Q_NW) {
                double s = 0.0;
                if (lane < n) s += (double)pl[(long long)lane * stride + k];
                s = wave_sum_d(s);
                if (lane == 0) {
                    const double z = 0.0, t = ((s + z) + z) + z;
                    if (k < h * K) a.gW[l][k] = (float)t;
                    else a.gB[l][k - h * K] = (float)t;
                }
            }
        if (l > 0) {  // dF_{l-1} (the combined weights in g.wc are this level's: c2_dT_weights' values)
            for (int j = wv; j < n; j += Q_NW)
                q_node_gather(a, g, w, sp, j, dcur, rdp, trd, g.vec + f + (l - 1) * h, dnext);
        } else {  // dX[j] = sum over neighbours i of G_i[a_j] + d_j^2 dsum0 (k_ccn2_dx0)
            for (int j = wv; j < n; j += Q_NW) {
                const int nj = g.deg[j];
                float t[Q_CF];
#pragma unroll
                for (int c = 0; c < Q_CF; ++c) t[c] = 0.f;
                for (int x = lane; x < nj; x += 64) {
                    const int i = g.nbr[j * Q_N + x];
                    const unsigned long long mi = g.bits[i];
                    const int aj = __popcll(mi & ((1ull << j) - 1ull));  // position of j in N(i)
                    const float* gi = g0 + ((long long)g.off1[i] + aj) * cin;
#pragma unroll
                    for (int c = 0; c < Q_CF; ++c)
                        if (c < cin) t[c] += gi[c];
                }
#pragma unroll
                for (int c = 0; c < Q_CF; ++c) {
                    if (c >= cin) break;
                    const float s = wave_sum(t[c]);
                    if (lane == 0) {
                        const float rd = g.vec[c];
                        a.dX[((long long)b * a.nmax + j) * f + c] = s + (float)(nj * nj) * rd;
                    }
                }
            }
        }
        __syncthreads();
        float* t = dcur;
        dcur = dnext;
        dnext = t;
    }
    for (int e = threadIdx.x; e < (a.nmax - n) * f; e += Q_NT) a.dX[((long long)b * a.nmax + n) * f + e] = 0.f;
}

// Batches: the parameter gradients summed over the batch's nodes in k_ccn_param_reduce's order (blocks
// [0, np)), the fc gradients over the graphs in k_ccn_readout_bwd's order (the remaining blocks, a wave each)
__global__ void __launch_bounds__(256) k_ccn2_small_reduce(QArgs a, int np) {
    __shared__ double red[4];
    __shared__ int s_tot;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int h = a.h, f = a.f, L = a.L, nf = f + L * h;
    if ((int)blockIdx.x < np) {
        int k = blockIdx.x, l = 0;
        for (; l < L; ++l) {
            const int K = 18 * (l == 0 ? f : h), st = h * K + h;
            if (k < st) break;
            k -= st;
        }
        const int K = 18 * (l == 0 ? f : h), stride = h * K + h;
        if (threadIdx.x < 64) {  // total nodes of the batch (the packed index range)
            int s = 0;
            for (int q = lane; q < a.bs; q += 64) {
                const long long v = a.n_batch ? a.n_batch[q] : a.nmax;
                s += v < 0 ? 0 : (v > a.nmax ? a.nmax : (int)v);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (lane == 0) s_tot = s;
        }
        __syncthreads();
        const int n = s_tot;
        double s = 0.0;
        for (int i = threadIdx.x; i < n; i += 256) s += (double)a.ppart[l][(long long)i * stride + k];
        s = wave_sum_d(s);
        if (lane == 0) red[wv] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            const double t = red[0] + red[1] + red[2] + red[3];
            if (k < h * K) a.gW[l][k] = (float)t;
            else a.gB[l][k - h * K] = (float)t;
        }
        return;
    }
    const int q = ((int)blockIdx.x - np) * 4 + wv;
    if (q >= a.n_out * nf + a.n_out) return;
    double s = 0.0;
    if (q < a.n_out * nf) {
        const int o = q / nf, k = q % nf;
        for (int b = lane; b < a.bs; b += 64) s += (double)a.dout[b * a.n_out + o] * (double)a.feat[(long long)b * nf + k];
    } else {
        const int o = q - a.n_out * nf;
        for (int b = lane; b < a.bs; b += 64) s += (double)a.dout[b * a.n_out + o];
    }
    s = wave_sum_d(s);
    if (lane == 0) {
        if (q < a.n_out * nf) a.gfcw[q] = (float)s;
        else a.gfcb[q - a.n_out * nf] = (float)s;
    }
}

}  // namespace

bool ccn2_small_ok(const hgnn_ccn_config* c) {
    return c && c->order == 2 && c->bs > 0 && c->nmax > 0 && c->nmax <= Q_N && c->f_in > 0 && c->f_in <= Q_CF &&
           c->hidden > 0 && c->hidden <= Q_H && c->layers >= 1 && c->layers <= Q_LMAX && c->n_out > 0 &&
           q_nf(c) <= Q_NF && q_lds_bytes(c->nmax) <= Q_LDS_MAX;
}

size_t ccn2_small_workspace_bytes(const hgnn_ccn_config* c) {
    if (!ccn2_small_ok(c)) return 0;
    size_t t = q_al256(4 * (size_t)c->bs * q_nf(c));
    for (int l = 0; l < c->layers; ++l) t += q_al256(4 * (size_t)c->bs * c->nmax * q_prow(c, l));
    return t + 4 * (size_t)c->bs * q_gstride(c);
}

int ccn2_small_forward(const hgnn_ccn_config* c, const float* X, const float* adj, const int64_t* nb,
                       const float* const* params, void* ws, int32_t* err, int32_t tag, float* out, hipStream_t s) {
    QArgs a = q_args(c, X, adj, nb, params, ws);
    a.out = out;
    a.err = err;
    a.tag = tag;
    static bool attr = false;
    q_lds_attr(&k_ccn2_small_fwd<Q_CF>, attr);
    HGNN_KLAUNCH(k_ccn2_small_fwd<Q_CF>, dim3(c->bs), dim3(Q_NT), q_lds_bytes(c->nmax), s, a);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

int ccn2_small_backward(const hgnn_ccn_config* c, const float* X, const float* adj, const int64_t* nb,
                        const float* const* params, void* ws, const float* dout, float* const* grads, float* dX,
                        hipStream_t s) {
    QArgs a = q_args(c, X, adj, nb, params, ws);
    a.dout = dout;
    a.dX = dX;
    for (int l = 0; l < c->layers; ++l) {
        a.gW[l] = grads[2 * l];
        a.gB[l] = grads[2 * l + 1];
    }
    a.gfcw = grads[2 * c->layers];
    a.gfcb = grads[2 * c->layers + 1];
    static bool attr = false;
    q_lds_attr(&k_ccn2_small_bwd<Q_CF>, attr);
    HGNN_KLAUNCH(k_ccn2_small_bwd<Q_CF>, dim3(c->bs), dim3(Q_NT), q_lds_bytes(c->nmax), s, a);
    HGNN_LAUNCH_CHECK();
    if (c->bs > 1) {
        int np = 0;
        for (int l = 0; l < c->layers; ++l) np += (int)q_prow(c, l);
        const int nf = q_nf(c);
        HGNN_KLAUNCH(k_ccn2_small_reduce, dim3(np + (c->n_out * nf + c->n_out + 3) / 4), dim3(256), 0, s, a, np);
        HGNN_LAUNCH_CHECK();
    }
    return HGNN_OK;
}

}  // namespace hgnn
