// What the files of the general CCN path (ccn_plan.hip, ccn1.hip, ccn2.hip, ccn2_big.hip, ccn_readout.hip and
// the executor ccn.hip) share: the plan view and the kernels' argument structs, the degree / channel bounds, the
// device helpers more than one of them uses (one definition each), the instantiation choices by channel count,
// and the launchers they call each other through.  The kernels stay local to their files.
#pragma once
#include "ccn2_shared.h"

namespace hgnn {

constexpr int CCN_MAXD = 64;     // CCN-2D fast-path degree bound (one wave per receptive-field row, 64-bit ballots)
constexpr int CCN_BIGD = 256;    // CCN-2D degree bound: degrees 65..256 take the _big kernels (rows in 64-lane
                                 // chunks, membership as 4 x 64-bit words, position maps read from L2)
constexpr int CCN_BW = CCN_BIGD / 64;
constexpr int CCN1_MAXD = 1024;  // CCN-1D degree bound (rows walked in 64-lane chunks; per-wave LDS row sums)
constexpr int C1F = 8, C1H = 8;  // CCN-1D one-chunk fast path: channels (f_in / hidden) and outputs
constexpr int C2_CMAX = 8;  // channels of a CCN-2D level (f_in or hidden) handled per pass (narrow kernels)
constexpr int C2_HMAX = 8;  // hidden size bound of the fused output stage (narrow kernels)
constexpr int C2_CMAX_WIDE = 16;  // the wide instantiations: f_in, hidden <= 16
constexpr int C2_HMAX_WIDE = 16;
constexpr int C2_NCAP = 64;  // receptive-field bound of the CCN-2D kernels of degrees <= 64 (their LDS arrays)
constexpr int RO_CH = 32;    // readout: most row chunks per graph (ccn_readout.hip ro_chunks)

struct CcnPlanView {
    const int* node_off;   // (bs + 1)
    const int* deg;        // per node
    const int* nbr;        // per node: slot of nmax global node ids
    const int* selfpos;    // index of i in nbr_i
    const int* graph;      // node -> graph
    const int* off1;       // exclusive prefix of deg      (row offsets of 1D features)
    const int* off2;       // exclusive prefix of deg^2    (row offsets of 2D features, pos maps)
    const int* pos;        // [sum deg^2] position maps
    int nmax;
};

// contraction statistics the forward of the degrees 65..256 keeps for their backward (k_ccn2_fwd_big)
struct C2Save {
    float* Sc;   // [sum d^2][C]  Sc[a][b]
    float* Sa;   // [sum d^2][C]  Sa[b][z]
    float* D1;   // [sum d^2][C]  T[a][b][b]
    float* D2;   // [sum d^2][C]  T[a][b][a]
    float* q1;   // [sum d][C]
    float* q3;   // [sum d][C]
    float* tot;  // [nodes][C]
    float* d3;   // [nodes][C]
};

struct C2Grad {
    float* dSc;  // [sum d^2][C]  (dSc + dq1 folded)
    float* dSa;  // [sum d^2][C]  (dSa + dq3 + dtot folded)
    float* dD1;  // [sum d^2][C]
    float* dD2;  // [sum d^2][C]  indexed [a][b]
    float* dd3;  // [nodes][C]
};

// the dp format the two gathers rebuild dT from (written by k_c2_bwd and k_c2_dp_big)
struct C2Dp {
    const float* dp;   // [sum d^2][h]
    const float* rdp;  // [sum d][h]
    const float* trd;  // [nodes][h]
};

// feat[b] = cat_l (sum over the graph's rows of F_l); level 0: sum_i d_i^order X[i]
struct ReadoutArgs {
    int nch;              // chunks per graph of k_ccn_readout_part
    int per_node;         // F[l] holds per-node sums ([nodes][h], CCN-2D) instead of feature rows
    CcnPlanView v;
    int order, L, f, h, n_out, bs;
    const float* X;
    const float* F[16];   // levels 1..L (packed)
    const float* fcw;
    const float* fcb;
    float* feat;          // [bs][f + L h]
    float* out;           // [bs][n_out]
};

namespace {

// bit x of a multi-word set (CCN-2D common neighbourhoods of the large-degree kernels)
__device__ __forceinline__ bool mbit(const unsigned long long* m, int x) { return (m[x >> 6] >> (x & 63)) & 1ull; }

// node i's position maps into LDS as int16, all loads of a thread in flight before the stores
__device__ __forceinline__ void c2_copy_pos(const int* __restrict__ pos, int nn, short* sp) {
    for (int e0 = threadIdx.x; e0 < nn; e0 += 256 * 8) {
        int t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = e0 + k * 256 < nn ? pos[e0 + k * 256] : 0;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (e0 + k * 256 < nn) sp[e0 + k * 256] = (short)t[k];
    }
}

// Gather of one CCN-2D level's input gradient from the dp format (no atomics): node j collects, for
// every neighbour i = i_a with u, w in C_a, the gradient of the entry of T_i that read F_j[u][w]:
//   dF_{l-1}[j][u][w] = sum_a dT_i[aj][b][z] (+ readout),  b = p_a(u), z = p_a(w), aj = position of j in N(i),
//   dT[a][b][z] = dSc[a][b] + dSa[b][z] + [z = b] dD1[a][b] + [z = a] dD2[a][b] + [a = b = z] dd3,
//   dSc[a][b] = (n_i A + W5)^T dp[a][b] + W1^T rdp[a],   dSa[b][z] = n_i W2^T dp[b][z] + W3^T rdp[b] + W4^T tr,
//   dD1[a][b] = W15^T dp[a][b],   dD2[a][b] = W16^T dp[b][a],   dd3 = W17^T tr      (A = W0 + W6 + ... + W14).
// Per (u, a) the wave-uniform part is five h-vectors of node i, the lane part one row piece dp[b][z].
// The level's input has cin = h channels (levels >= 1 only: level 0 goes through k_ccn2_dx0).
template <int H>
__device__ __forceinline__ void c2_dT_weights(float (*wc)[H][H], const float* __restrict__ W, int h) {
    const int K = 18 * h;
    for (int t = threadIdx.x; t < H * H; t += blockDim.x) {
        const int o = t / H, c = t % H;
        const bool ok = o < h && c < h;
        const float* w = W + (long long)(ok ? o : 0) * K;
        float r[18];
#pragma unroll
        for (int q = 0; q < 18; ++q) r[q] = ok ? w[q * h + c] : 0.f;
        float a = r[0];
#pragma unroll
        for (int q = 6; q < 15; ++q) a += r[q];
        wc[WA][o][c] = a;
        wc[WB][o][c] = r[5];
        wc[WQ1][o][c] = r[1];
        wc[WQ2][o][c] = r[2];
        wc[WQ3][o][c] = r[3];
        wc[WQ4][o][c] = r[4];
        wc[WQ15][o][c] = r[15];
        wc[WQ16][o][c] = r[16];
        wc[WQ17][o][c] = r[17];
    }
}

// loads of one (i, a) pair: ld[0] dp[aj][b], ld[1] dp[b][aj], ld[2] rdp[aj], ld[3] rdp[b], ld[4] tr, ld[5] dp[b][z]
template <int H>
__device__ __forceinline__ void c2_dT_load(const C2Dp& g, int h, long long oi, long long o1i, int i, int di, int aj,
                                           int b, int z, float (&ld)[6][H]) {
    const float* pab = g.dp + (oi + (long long)aj * di + b) * h;
    const float* pba = g.dp + (oi + (long long)b * di + aj) * h;
    const float* pbz = g.dp + (oi + (long long)b * di + z) * h;
#pragma unroll
    for (int o = 0; o < H; ++o) {
        const bool ok = o < h;
        ld[0][o] = ok ? pab[o] : 0.f;
        ld[1][o] = ok ? pba[o] : 0.f;
        ld[2][o] = ok ? g.rdp[(o1i + aj) * h + o] : 0.f;
        ld[3][o] = ok ? g.rdp[(o1i + b) * h + o] : 0.f;
        ld[4][o] = ok ? g.trd[(long long)i * h + o] : 0.f;
        ld[5][o] = ok ? pbz[o] : 0.f;
    }
}

template <int H>
__device__ __forceinline__ void c2_dT_add(const float (*wc)[H][H], const float (&ld)[6][H], int h, float nfi, int aj,
                                          int b, int z, float (&acc)[H]) {
    const bool e1 = z == b, e2 = z == aj, e3 = aj == b && b == z;
#pragma unroll
    for (int c = 0; c < H; ++c) {
        if (c >= h) break;
        float s = 0.f;
#pragma unroll
        for (int o = 0; o < H; ++o) {
            if (o >= h) break;
            s = fmaf(fmaf(nfi, wc[WA][o][c], wc[WB][o][c]), ld[0][o], s);
            s = fmaf(wc[WQ1][o][c], ld[2][o], s);
            s = fmaf(wc[WQ3][o][c], ld[3][o], s);
            s = fmaf(wc[WQ4][o][c], ld[4][o], s);
            s = fmaf(nfi * wc[WQ2][o][c], ld[5][o], s);
            if (e1) s = fmaf(wc[WQ15][o][c], ld[0][o], s);
            if (e2) s = fmaf(wc[WQ16][o][c], ld[1][o], s);
            if (e3) s = fmaf(wc[WQ17][o][c], ld[4][o], s);
        }
        acc[c] += s;
    }
}

}  // namespace

// ------------------------------------------------------------------ instantiation choices
// Each family's thresholds and template tuples, stated once; a launcher hands the chosen tuple (an empty tag
// struct) to a generic lambda that names the kernel.

template <int CM_, int HC_, int NB_, bool L0_>
struct C2Inst {
    static constexpr int CM = CM_, HC = HC_, NB = NB_;
    static constexpr bool L0 = L0_;
};
// k_c2_fwd / k_c2_bwd <CM, HC, NB, L0> by the level's input channels: cin <= 2 (the reference's hidden_size = 2
// levels), <= 8, <= 16; level 0 has no neighbour batches (NB = 1).
template <bool BWD, typename F>
int c2_select(int level0, int cin, F&& f) {
    if (level0) return cin <= 8 ? f(C2Inst<8, 2, 1, true>{}) : f(C2Inst<16, 2, 1, true>{});
    if (cin <= 2) return f(C2Inst<2, 2, 8, false>{});
    if (cin <= 8) return f(C2Inst<8, 2, 4, false>{});
    // the one intended difference: a wide level takes two output channels per pass forward (HC = 2) and one
    // backward (HC = 1)
    return f(C2Inst<16, BWD ? 1 : 2, 2, false>{});
}

template <int H_, int NB_>
struct C2GatherInst {
    static constexpr int H = H_, NB = NB_;
};
// k_c2_gather / k_c2_gather_big <H, NB> by the hidden size; NB2: the neighbours per batch at H = 2 (8 and 4)
template <int NB2, typename F>
int c2_gather_select(int h, F&& f) {
    if (h <= 2) return f(C2GatherInst<2, NB2>{});
    if (h <= 8) return f(C2GatherInst<8, 1>{});
    return f(C2GatherInst<16, 1>{});
}

template <int CM_, int HM_>
struct C2BigInst {
    static constexpr int CM = CM_, HM = HM_;
};
// k_ccn2_fwd_big / k_ccn2_bwd_node_big <CM, HM>: narrow while input channels and hidden size are both <= 8
template <typename F>
int c2_big_select(int cin, int h, F&& f) {
    if (cin <= C2_CMAX && h <= C2_HMAX) return f(C2BigInst<C2_CMAX, C2_HMAX>{});
    return f(C2BigInst<C2_CMAX_WIDE, C2_HMAX_WIDE>{});
}

// ------------------------------------------------------------------ host side
inline size_t al(size_t x) { return (x + 255) / 256 * 256; }

template <typename T>
T* P(void* base, size_t off) {
    return reinterpret_cast<T*>(static_cast<char*>(base) + off);
}

inline bool ccn_ok(const hgnn_ccn_config* c) {
    return c && (c->order == 1 || c->order == 2) && c->bs > 0 && c->nmax > 0 && c->f_in > 0 && c->hidden > 0 &&
           c->layers >= 1 && c->layers <= 15 && c->n_out > 0 &&
           (c->order == 1 || (c->f_in <= C2_CMAX_WIDE && c->hidden <= C2_CMAX_WIDE && c->hidden <= C2_HMAX_WIDE));
}

// grids: a block per node, or a wave per node (four to a block); at least one block
inline dim3 ccn_grid1(int nodes) { return dim3(nodes > 0 ? nodes : 1); }
inline dim3 ccn_grid4(int nodes) { return dim3(nodes > 0 ? (nodes + 3) / 4 : 1); }

// The plan workspace (ccn_plan.hip), offsets from its own start
struct CcnPlanLayout {
    size_t node_off, deg, nbr, selfpos, graph, off1, off2, totals, err, bits, bcnt, pos;
    size_t bytes;
};
CcnPlanLayout plan_layout(const hgnn_ccn_config* c, long long max_sum_d2);
CcnPlanView plan_view(const hgnn_ccn_config* c, const CcnPlanLayout& L, void* plan_ws);

// ccn1.hip: one CCN-1D level
int launch_ccn1_fwd(const CcnPlanView& v, const int* tot, int nodes, const float* fin, int level0, const float* X,
                    int cin, const float* W, const float* b, int h, float* coll, float* fout, hipStream_t s);
int launch_ccn1_bwd_node(const CcnPlanView& v, const int* tot, int nodes, const float* dF, const float* F,
                         const float* coll, int cin, const float* W, int h, float* dcoll, float* ppart, hipStream_t s);
int launch_ccn1_bwd_gather(const CcnPlanView& v, const int* tot, int nodes, const float* dcoll, int cin,
                           const float* dsum, int dsum_ld, int dsum_off, int level0, float* dout, hipStream_t s);

// ccn2.hip: one CCN-2D level, nodes of degree <= 64 (dmax: the batch's largest degree, or its bound)
int launch_c2_fwd(const CcnPlanView& v, const int* tot, const float* fin, int level0, const float* X, int cin,
                  const float* W, const float* b, int h, long long dmax, int nodes, float* fout, float* nsum,
                  hipStream_t s);
int launch_c2_bwd(const CcnPlanView& v, const int* tot, float* dF, const float* dtop, int dtop_ld, const float* F,
                  const float* fin, int level0, const float* X, int cin, const float* W, int h, long long dmax,
                  int nodes, float* rdp, float* trd, float* ppart, float* g0, hipStream_t s);
int launch_c2_dx0(const CcnPlanView& v, const int* tot, int nodes, const float* g0, int cin, const float* dsum,
                  int dsum_ld, float* dout, hipStream_t s);
int launch_c2_gather(const CcnPlanView& v, const int* tot, const C2Dp& g, const float* W, int h, const float* dsum,
                     int dsum_ld, int dsum_off, int nodes, float* dout, hipStream_t s);

// ccn2_big.hip: the same level for the nodes of degree 65..256 (every other node exits at once)
int launch_c2_fwd_big(const CcnPlanView& v, const int* tot, int nodes, const float* fin, int level0, const float* X,
                      int cin, const float* W, const float* b, int h, const C2Save& sv, float* fout, float* nsum,
                      hipStream_t s);
int launch_c2_bwd_node_big(const CcnPlanView& v, const int* tot, int nodes, const float* dF, const float* F,
                           const C2Save& sv, int cin, const float* W, int h, const C2Grad& gd, float* ppart,
                           float* g0, hipStream_t s);
int launch_c2_dp_big(const CcnPlanView& v, const int* tot, int nodes, float* dF, const float* F, int h, float* rdp,
                     float* trd, hipStream_t s);
int launch_c2_gather_big(const CcnPlanView& v, const int* tot, const C2Dp& g, const float* W, int h,
                         const float* dsum, int dsum_ld, int dsum_off, int nodes, float* dout, hipStream_t s);

// ccn_readout.hip: what both orders share.  launch_ccn_readout takes the rows a level sums per batch (feature
// rows for CCN-1D, nodes for CCN-2D) to choose the chunks per graph; rpart holds [bs][RO_CH][f + L h] doubles.
int launch_ccn_readout(ReadoutArgs ra, long long rows, double* rpart, hipStream_t s);
int launch_ccn_readout_bwd(const float* dout, const float* feat, const float* fcw, int bs, int n_out, int nf,
                           float* dsum, float* dfcw, float* dfcb, hipStream_t s);
int launch_ccn_param_reduce(const float* ppart, const int* tot, int kw, int kb, float* dw, float* db, hipStream_t s);
int launch_ccn_bcast(const CcnPlanView& v, const int* tot, int nodes, int order, const float* dsum, int ld, int off,
                     int h, float* dF, hipStream_t s);
int launch_ccn_pack_x(const float* X, const int* node_off, int bs, int nmax, int f, float* Xp, hipStream_t s);
int launch_ccn_unpack_dx(const float* dXp, const int* node_off, int bs, int nmax, int f, float* dX, hipStream_t s);

}  // namespace hgnn
