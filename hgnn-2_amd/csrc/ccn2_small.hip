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
// The layout, the node functions and the stages (q_forward, q_readout, q_dsum, q_fc_grads, q_backward, the
// per-element sums) are in ccn2_small.h, shared with the per-graph training loop (ccn2_small_train.hip) and the
// mini-batch kernels (ccn2_small_batch.hip); this unit holds the one-shot forward and backward kernels, each a list
// of those stages, and their launches.
#include "ccn2_small.h"

namespace hgnn {
namespace {

// plan, forward, the feat row, readout, the validation bits
template <int CF>
__global__ void __launch_bounds__(Q_NT) k_ccn2_small_fwd(QArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    __shared__ uint32_t sbad;
    __shared__ double sred[4];
    auto [g, w, sp, P] = q_carve(lds, a);
    const int b = blockIdx.x;
    if (threadIdx.x == 0) sbad = 0;
    uint32_t bad = 0;
    const int n = q_nodes(a, b, bad);
    [[clang::always_inline]] bad |= q_plan(a, b, n, g);
    const int nf = a.f + a.L * a.h;
    q_forward<CF, false>(a, g, w, sp, P, n, a.gws + (long long)b * a.gstride);
    for (int k = threadIdx.x; k < nf; k += Q_NT) a.feat[(long long)b * nf + k] = g.vec[k];
    q_readout<false>(a, g, nf, sred, a.out + (long long)b * a.n_out, nullptr);
    q_report(bad, sbad);
    __syncthreads();
    if (threadIdx.x == 0 && sbad) a.err[0] = a.tag * 256 + (int)sbad;  // vector store (host-mapped word)
}

// plan, dsum, (bs == 1: the fc gradients), the level walk with dX (bs == 1: and the parameter reduction), the zero
// rows of dX
template <int CF>
__global__ void __launch_bounds__(Q_NT) k_ccn2_small_bwd(QArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    auto [g, w, sp, dpL] = q_carve(lds, a);
    const int b = blockIdx.x;
    uint32_t bad = 0;
    const int n = q_nodes(a, b, bad);
    [[clang::always_inline]] (void)q_plan(a, b, n, g);  // the forward reported the batch's validation bits
    const int nf = a.f + a.L * a.h;
    float* G = a.gws + (long long)b * a.gstride;
    const float* dob = a.dout + (long long)b * a.n_out;
    q_dsum<false>(a, g, dob, nf);
    if (a.bs == 1) q_fc_grads(a, dob, a.feat, nf);
    __syncthreads();
    q_backward<CF, false, true>(a, g, w, sp, dpL, b, n, G, q_region(a, G), a.bs == 1);
    for (int e = threadIdx.x; e < (a.nmax - n) * a.f; e += Q_NT) a.dX[((long long)b * a.nmax + n) * a.f + e] = 0.f;
}

// Batches: the parameter gradients summed over the batch's nodes (blocks [0, np), q_sum_level_elem), the fc
// gradients over the graphs (the remaining blocks, a wave each, q_sum_fc_elem)
__global__ void __launch_bounds__(256) k_ccn2_small_reduce(QArgs a, int np) {
    __shared__ double red[4];
    __shared__ int s_tot;
    const int nf = a.f + a.L * a.h;
    if ((int)blockIdx.x < np) {
        int k = blockIdx.x, l, K;
        q_level_elem(a, k, l, K);
        const double t = q_sum_level_elem(a, a.bs, l, k, a.h * K + a.h, red, s_tot);
        if (threadIdx.x == 0) {
            if (k < a.h * K) a.gW[l][k] = (float)t;
            else a.gB[l][k - a.h * K] = (float)t;
        }
        return;
    }
    const int q = ((int)blockIdx.x - np) * 4 + (int)(threadIdx.x >> 6);
    if (q >= a.n_out * nf + a.n_out) return;
    const double s = q_sum_fc_elem(a, a.dout, a.bs, q, nf);
    if ((threadIdx.x & 63) == 0) {
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
    return ccn2_small_ok(c) ? q_layout(c, c->bs).total : 0;
}

int ccn2_small_forward(const hgnn_ccn_config* c, const float* X, const float* adj, const int64_t* nb,
                       const float* const* params, void* ws, int32_t* err, int32_t tag, float* out, hipStream_t s) {
    QArgs a = q_args(c, X, adj, nb, params, ws, q_layout(c, c->bs));
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
    QArgs a = q_args(c, X, adj, nb, params, ws, q_layout(c, c->bs));
    a.dout = dout;
    a.dX = dX;
    q_set_grads(a, grads, c->layers);
    static bool attr = false;
    q_lds_attr(&k_ccn2_small_bwd<Q_CF>, attr);
    HGNN_KLAUNCH(k_ccn2_small_bwd<Q_CF>, dim3(c->bs), dim3(Q_NT), q_lds_bytes(c->nmax), s, a);
    HGNN_LAUNCH_CHECK();
    if (c->bs > 1) {
        const int np = q_np(c);
        HGNN_KLAUNCH(k_ccn2_small_reduce, dim3(np + q_nfc(c)), dim3(256), 0, s, a, np);
        HGNN_LAUNCH_CHECK();
    }
    return HGNN_OK;
}

}  // namespace hgnn
