// Device and host helpers of the CCN-1D small-graph kernels, shared by ccn_small.hip (the one-shot forward and backward
// and the per-graph training loop), ccn_small_batch.hip (the mini-batch training step) and their SPILL units:
//   * the LDS layout (CsLds, cs_carve), the staging round (cs_stage) and the plan (cs_plan);
//   * one level of the forward and of the backward walk: cs_collect, cs_update, cs_fwd_level, cs_bwd_level;
//   * the stages the kernels are lists of, each defined once: cs_open, cs_report, cs_levels_keep, cs_readout_sums,
//     cs_out_row, cs_dsum, cs_fc_grads, cs_backward, and the per-element pair of the reductions over graphs,
//     cs_param_elem / cs_sum_elem.  A stage inlines its level functions ([[clang::always_inline]]): the kernels run at
//     the register cap, and an outlined level would spill the wave's state around every call;
//   * the host side: the bounds, CsArgs from a config (cs_args, cs_set_grads), the workspace head, the LDS figures and
//     the launch of a kernel's CH = 2 or CH = CS_CF instantiation.
// k_ccn1_small_train (ccn_small_kernels.h) is the exception: it carries written-out copies of every stage, kept because
// as calls they change its instruction stream (scratch of its SPILL instantiations, and a measured 0.6 % of the
// classification loop); a change to a stage here goes there too.
// Every stage carries a bitwise contract (fused step == pieces, mini-batch == pieces, spill == LDS), which is why there
// is one definition.  The units stay separate translation units, so that one kernel's callers leave the others'
// inlining, and with it their code, alone.  The kernels themselves are templates in ccn_small_kernels.h and
// ccn_small_batch_kernels.h; their SPILL instantiations (ccn_small_spill.hip, ccn_small_batch_spill.hip) keep the
// row-sized arrays in global memory and take this code as it is, bar the three places marked SPILL below.
#pragma once
#include <cstdint>
#include <type_traits>

#include "kernels.h"

namespace hgnn {

constexpr int CS_NT = 512, CS_NW = CS_NT / 64;   // 8 waves (~4 nodes of a QM9 graph each; 256 VGPRs a lane)
constexpr int CS_RT = 256;                         // threads of the fp64 readout sums (the general path's order)
constexpr int CS_CF = 8;                              // f_in and hidden bound
constexpr int CS_LMAX = 15;
constexpr int CS_NFMAX = CS_CF + CS_LMAX * CS_CF;     // readout width bound
constexpr int CS_PMAX = CS_CF * 2 * CS_CF + CS_CF;    // one level's weight + bias entries
constexpr int CS_XMAX = 64 * CS_CF;                 // staged node features
constexpr int CS_WMAX = CS_LMAX * CS_PMAX;            // staged level weights and biases
constexpr size_t CS_FIXED = 512 + 256 + 272 + 4096 + 4 * CS_NW * CS_PMAX + 4 * CS_NFMAX + 8 * CS_NW * CS_CF +
                            4 * CS_XMAX + 4 * CS_WMAX;
constexpr size_t CS_LDS_MAX = 150 * 1024;  // dynamic LDS opt-in (the forward also has a static word)
// the training kernels (the per-graph loop and the mini-batch pair)
constexpr int CS_TMAX = 2 * CS_LMAX + 2;    // parameter tensors: level weights and biases, fc weight and bias
constexpr int CS_TRAIN_GMAX = 4096;         // graphs per call
constexpr int CS_OMAX = CS_NW * CS_PMAX;    // n_out bound: out / dout of the graph live in CsLds::red

struct CsArgs {
    const float* adj;        // (bs, nmax, nmax) with self loops
    const int64_t* n_batch;  // (bs,) or null: every graph has nmax nodes
    const float* X;          // (bs, nmax, f)
    int bs, nmax, f, h, L, n_out, rcap;  // rcap = nmax^2 bounds sum_i d_i of any graph
    const float* W[CS_LMAX];
    const float* B[CS_LMAX];
    const float* fcw;
    const float* fcb;
    float* feat;             // [bs][nf] readout features (forward writes, backward reads)
    float* out;              // (bs, n_out)
    int* err;                // forward: graphs with validation bits store tag * 256 + bits
    int tag;
    const float* dout;       // backward
    float* ppart;            // backward, bs > 1: [bs][ptot] level weight / bias partials, levels ascending
    float* gW[CS_LMAX];      // backward, bs == 1: gradients written directly
    float* gB[CS_LMAX];
    float* gfcw;
    float* gfcb;
    float* dX;               // (bs, nmax, f), padding rows zeroed
    unsigned long long* prof;  // diagnostic phase stamps of graph 0 (HGNN_CCN_SMALL_PROF), or null
};

namespace {

// phase stamp k of graph 0 (s_memtime core cycles), diagnostic builds of the timing only
#define CS_STAMP(k)                                                          \
    do {                                                                     \
        if (a.prof && blockIdx.x == 0 && threadIdx.x == 0) a.prof[k] = clock64(); \
    } while (0)

// The SPILL instantiation (ccn_small_spill.hip, ccn_small_batch_spill.hip): the four row-sized arrays (F, dcoll,
// dF0, dF1) of workgroup blockIdx.x live in region blockIdx.x of a caller-allocated global workspace instead of
// LDS, so the graph size is no longer bounded by the depth.  A region is written and read by its workgroup only,
// at per-lane addresses, behind the barriers the kernels have anyway (as ccn2_small.h's graph regions are).
struct CsSpillArgs : CsArgs {
    float* rows;         // regions of `rstride` floats, each 256-byte aligned
    long long rstride;
};
template <bool SPILL>
using CsArgsT = std::conditional_t<SPILL, CsSpillArgs, CsArgs>;

// Tail padding of a region, in floats.  The LDS carve's CS_CF floats cover the level walks' reads past a row; the
// backward's node pass also reads dF at row off1[i] + p for every lane p < G of node i, the graph's rows or not
// (idle lanes, dropped by the selects): up to rcap + 62 rows of hidden channels plus CS_CF - 1.  LDS answers such
// a read with whatever is there; a global read must stay inside the allocation.
constexpr int CS_SPILL_PAD = 64 * CS_CF;

// floats of one region: the LDS carve's order and strides (cs_carve, backward form), the padding, to 256 bytes
__host__ __device__ inline size_t cs_spill_stride(int rcap, int f, int h, int L) {
    const int cmax = f > h ? f : h;
    const size_t fl = (size_t)rcap * ((size_t)h * L + 2 * cmax + 2 * h) + CS_SPILL_PAD;
    return (fl + 63) / 64 * 64;
}

// LDS of a SPILL kernel: the fixed arrays and the staged adjacency (which aliases F in the LDS kernels)
__host__ __device__ inline size_t cs_spill_lds_bytes(int rcap) { return CS_FIXED + 4 * (size_t)rcap + 4 * CS_CF; }

struct CsLds {
    unsigned long long* bits;  // [64] row bit sets
    int* deg;                  // [64]
    int* off1;                 // [65] exclusive prefix of deg
    unsigned char* nbr;        // [64][64] ascending neighbour ids
    float* red;                // [CS_NW][CS_PMAX]
    float* vec;                // [CS_NFMAX] readout features (forward) / dsum (backward)
    double* dred;              // [CS_NW][CS_CF]
    float* Xs;                 // [n][f] the graph's node features
    float* Ws;                 // level l: W_l [h][2 cin] then b_l [h], levels ascending
    float* F;                  // forward: 2 levels (ping-pong); backward: all L levels, [rcap][h] each
    float* dcoll;              // backward: [rcap][2 cmax]
    float* dF0;                // backward: [rcap][h] x 2
    float* dF1;
};

// The level walks read CF channels of a row unconditionally and drop the ones past the row's width by
// selects: up to CF - 1 floats past the last region (F's second ping-pong buffer forward, dF1 backward),
// so the request carries CS_CF floats of padding and every such read stays inside the allocation.
__host__ __device__ inline size_t cs_lds_bytes(int rcap, int f, int h, int L, bool bwd) {
    const int cmax = f > h ? f : h;
    return CS_FIXED + 4 * (size_t)rcap * (bwd ? (size_t)h * L + 2 * cmax + 2 * h : 2 * (size_t)h) + 4 * CS_CF;
}

template <bool SPILL = false>
__device__ inline CsLds cs_carve(char* base, const CsArgsT<SPILL>& a, bool bwd) {
    CsLds s;
    size_t o = 0;
    s.bits = reinterpret_cast<unsigned long long*>(base + o);
    o += 512;
    s.deg = reinterpret_cast<int*>(base + o);
    o += 256;
    s.off1 = reinterpret_cast<int*>(base + o);
    o += 272;
    s.nbr = reinterpret_cast<unsigned char*>(base + o);
    o += 4096;
    s.red = reinterpret_cast<float*>(base + o);
    o += 4 * CS_NW * CS_PMAX;
    s.vec = reinterpret_cast<float*>(base + o);
    o += 4 * CS_NFMAX;
    s.dred = reinterpret_cast<double*>(base + o);
    o += 8 * CS_NW * CS_CF;
    s.Xs = reinterpret_cast<float*>(base + o);
    o += 4 * CS_XMAX;
    s.Ws = reinterpret_cast<float*>(base + o);
    o += 4 * CS_WMAX;
    if constexpr (SPILL) {  // one address space per instantiation: the rows in this workgroup's region
        float* r = a.rows + (size_t)blockIdx.x * a.rstride;
        const int cmax = a.f > a.h ? a.f : a.h;
        s.F = r;
        s.dcoll = s.F + (size_t)a.rcap * a.h * a.L;
        s.dF0 = s.dcoll + (size_t)a.rcap * 2 * cmax;
        s.dF1 = s.dF0 + (size_t)a.rcap * a.h;
        return s;
    }
    s.F = reinterpret_cast<float*>(base + o);
    o += 4 * (size_t)a.rcap * a.h * (bwd ? a.L : 2);
    s.dcoll = s.dF0 = s.dF1 = nullptr;
    if (bwd) {
        const int cmax = a.f > a.h ? a.f : a.h;
        s.dcoll = reinterpret_cast<float*>(base + o);
        o += 4 * (size_t)a.rcap * 2 * cmax;
        s.dF0 = reinterpret_cast<float*>(base + o);
        o += 4 * (size_t)a.rcap * a.h;
        s.dF1 = reinterpret_cast<float*>(base + o);
    }
    return s;
}

// where cs_stage puts the adjacency block: over F (dead until level 0 writes it, after the plan), SPILL: LDS of its own
template <bool SPILL = false>
__device__ __forceinline__ float* cs_adj(char* base, const CsLds& s) {
    if constexpr (SPILL) return reinterpret_cast<float*>(base + CS_FIXED);
    else return s.F;
}

__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// offset of level l's weights in Ws
__device__ __forceinline__ int cs_woff(int l, int f, int h) {
    return l == 0 ? 0 : (h * 2 * f + h) + (l - 1) * (h * 2 * h + h);
}

// One round of loads for the whole call: the graph's adjacency block (into As, stride n), its node
// features and every level's weights; every later access is to LDS (the dependent global round trips
// of a per-node walk were most of a QM9 graph's time).
__device__ void cs_stage(const CsArgs& a, int b, int n, const CsLds& s, float* As) {
    const float* A = a.adj + (long long)b * a.nmax * a.nmax;
    const float* Xg = a.X + (long long)b * a.nmax * a.f;
    const int na = n * n, nx = n * a.f, nw = cs_woff(a.L, a.f, a.h);
    const int total = na + nx + nw;
    constexpr int U = 4;
    for (int e0 = threadIdx.x; e0 < total; e0 += CS_NT * U) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * CS_NT;
            v[u] = 0.f;
            if (e < na) {
                const int r = e / n;
                v[u] = A[(long long)r * a.nmax + (e - r * n)];
            } else if (e < na + nx) {
                v[u] = Xg[e - na];
            } else if (e < total) {
                int p = e - na - nx, l = 0;
                while (l + 1 < a.L && p >= cs_woff(l + 1, a.f, a.h)) ++l;
                const int q = p - cs_woff(l, a.f, a.h), hk = a.h * 2 * (l == 0 ? a.f : a.h);
                v[u] = q < hk ? a.W[l][q] : a.B[l][q - hk];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * CS_NT;
            if (e < na) As[e] = v[u];
            else if (e < na + nx) s.Xs[e - na] = v[u];
            else if (e < total) s.Ws[e - na - nx] = v[u];
        }
    }
    __syncthreads();
}

// Graph b's receptive fields from the staged adjacency: nbr, bits, deg, off1 in LDS.  Returns this lane's
// validation bits (self loop missing, pattern not symmetric -- the general plan's ERR_CCN_SELFLOOP /
// ERR_CCN_ASYM).
__device__ uint32_t cs_plan(int n, const CsLds& s, const float* As) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t bad = 0;
    // row 0's first entry is what an idle lane (past the graph) reads as its neighbour id: defined even
    // for an empty slot (n = 0), so its bits / off1 reads stay inside the arrays
    if (n == 0 && threadIdx.x == 0) s.nbr[0] = 0;
    for (int r = wv; r < n; r += CS_NW) {
        const bool nz = lane < n && As[r * n + lane] > 0.f;  // utils_ccn.py:195 (A > 0)
        const unsigned long long m = __ballot(nz);
        if (nz) s.nbr[r * 64 + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned char)lane;
        if (lane == 0) {
            s.bits[r] = m;
            s.deg[r] = __popcll(m);
        }
        if (!((m >> r) & 1ull)) bad |= ERR_CCN_SELFLOOP;
    }
    __syncthreads();
    if (wv == 0) {
        const int d = lane < n ? s.deg[lane] : 0;
        int x = d;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(x, o, 64);
            if (lane >= o) x += t;
        }
        s.off1[lane] = x - d;
        if (lane == 63) s.off1[64] = x;
        // lanes per node of the level walks: the power of two >= the largest receptive field
        int dm = d;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dm = max(dm, __shfl_xor(dm, o, 64));
        int g = 1;
        while (g < dm) g <<= 1;
        if (lane == 0) s.off1[66] = g;
    }
    // every neighbour j of r must list r (the backward gathers node j's readers from N(j))
    for (int r = wv; r < n; r += CS_NW) {
        const unsigned long long m = s.bits[r];
        if (lane < n && ((m >> lane) & 1ull) && !((s.bits[lane] >> r) & 1ull)) bad |= ERR_CCN_ASYM;
    }
    __syncthreads();
    return bad;
}

// SPILL: where a walk reads either an LDS array or a row array by a block-uniform choice, the two pointers carry
// their address spaces, so the choice stays a branch between an LDS and a global load (as plain pointers the
// compiler folds it into one select of the two, and every such load becomes a flat load).
typedef const __attribute__((address_space(3))) float* CsLdsPtr;
typedef const __attribute__((address_space(1))) float* CsGlobalPtr;

// cs_collect's batch of loads from one base (SPILL)
template <int CF, typename P>
__device__ __forceinline__ void cs_rows(P src, const int (&a1)[4], const int (&a2)[4], float (&t1)[4][CF],
                                        float (&t2)[4][CF]) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < CF; ++c) {
            t1[q][c] = src[a1[q] + c];
            t2[q][c] = src[a2[q] + c];
        }
}

// Level walks pack several nodes into a wave: G lanes per node (G = the power of two >= the graph's largest
// receptive field, off1[66]), lane p of group g serves position / neighbour p of node i = base + wv * 64/G + g
// (-1 past the graph).  A QM9 graph (d <= 5, G = 8) takes 8 nodes per wave: one pass of the 8 waves.
struct CsSlot {
    int i, p;
};
__device__ __forceinline__ CsSlot cs_slot(int base, int G, int n) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = base + wv * (64 / G) + lane / G;
    return CsSlot{i < n ? i : -1, lane & (G - 1)};
}

// Node i, lane p < d_i (w = nbr_i[p]):  rs[c] = sum_a T[a][p][c] (p as the position x: w read from N(j_a), a
// ascending) and colv[c] = sum_x T[p][x][c] (p as the neighbour a: every u_x read from N(w), x ascending),
// T[a][x] = F_{j_a}[pos(u_x in N(j_a))] (level 0: X[j_a] when present).  Lane-local loops over the node's
// neighbours -- no cross-lane reduction -- in the order of k_ccn1_fwd's one-chunk path.  Branch-free: the
// four neighbours' ids, their rows and offsets, then every channel of both reads go out as one batch of LDS
// loads each (reads past a row are discarded by the selects; cs_lds_bytes pads the allocation for them).
template <int CF, bool SPILL = false>
__device__ __forceinline__ void cs_collect(const CsLds& s, CsSlot sl, int G, const float* __restrict__ Xg,
                                           const float* Fin, int cin, float (&rs)[CF], float (&colv)[CF]) {
    const int ib = (sl.i >= 0 ? sl.i : 0) * 64;
    const int d = sl.i >= 0 ? s.deg[sl.i] : 0;
    const bool v = sl.p < d;
    const bool lv0 = Fin == nullptr;
    const float* B = lv0 ? Xg : Fin;
    const int wl = s.nbr[ib + (v ? sl.p : 0)];
    const unsigned long long ml = s.bits[wl];
    const unsigned long long bl = (1ull << wl) - 1ull;
    const int ol = s.off1[wl];
    const int dl = d > 0 ? d - 1 : 0;
#pragma unroll
    for (int c = 0; c < CF; ++c) rs[c] = colv[c] = 0.f;
    for (int k0 = 0; k0 < G; k0 += 4) {
        int jk[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) jk[q] = s.nbr[ib + min(k0 + q, dl)];
        unsigned long long mk[4];
        int ok_[4], a1[4], a2[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            mk[q] = s.bits[jk[q]];
            ok_[q] = s.off1[jk[q]];
        }
        bool g1[4], g2[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool live = v && k0 + q < d;
            g1[q] = live && ((mk[q] >> wl) & 1ull);
            g2[q] = live && ((ml >> jk[q]) & 1ull);
            a1[q] = lv0 ? jk[q] * cin : (ok_[q] + __popcll(mk[q] & bl)) * cin;
            a2[q] = lv0 ? wl * cin : (ol + __popcll(ml & ((1ull << jk[q]) - 1ull))) * cin;
        }
        float t1[4][CF], t2[4][CF];
        if constexpr (SPILL) {  // Xg is LDS, Fin global: a block-uniform branch
            if (lv0) cs_rows<CF>((CsLdsPtr)Xg, a1, a2, t1, t2);
            else cs_rows<CF>((CsGlobalPtr)Fin, a1, a2, t1, t2);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int c = 0; c < CF; ++c) {
                    t1[q][c] = B[a1[q] + c];
                    t2[q][c] = B[a2[q] + c];
                }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < CF; ++c) {
                rs[c] += (c < cin && g1[q]) ? t1[q][c] : 0.f;
                colv[c] += (c < cin && g2[q]) ? t2[q][c] : 0.f;
            }
    }
}

// F_l rows of node i: relu(b + W [rs | colv]) in k_ccn1_fwd's order
template <int CF>
__device__ __forceinline__ void cs_update(const CsLds& s, CsSlot sl, const float (&rs)[CF], const float (&colv)[CF],
                                          int cin, const float* __restrict__ W, const float* __restrict__ bias, int h,
                                          float* Fout) {
    if (sl.i < 0 || sl.p >= s.deg[sl.i]) return;
    const int k2 = 2 * cin;
    const int row = s.off1[sl.i] + sl.p;
    for (int o = 0; o < h; ++o) {
        float v = bias[o];
#pragma unroll
        for (int c = 0; c < CF; ++c)
            if (c < cin) v = fmaf(W[o * k2 + c], rs[c], v);
#pragma unroll
        for (int c = 0; c < CF; ++c)
            if (c < cin) v = fmaf(W[o * k2 + cin + c], colv[c], v);
        Fout[row * h + o] = v < 0.f ? 0.f : v;
    }
}

// One level of the forward walk: F_l of every node (CF = the level's channel bound)
template <int CF, bool SPILL = false>
__device__ __forceinline__ void cs_fwd_level(const CsLds& s, int n, int G, const float* Xg, const float* fin, int cin,
                                             const float* Wl, int h, float* fout) {
    for (int base = 0; base < n; base += CS_NW * (64 / G)) {
        const CsSlot sl = cs_slot(base, G, n);
        float rs[CF], colv[CF];
        cs_collect<CF, SPILL>(s, sl, G, Xg, fin, cin, rs, colv);
        cs_update<CF>(s, sl, rs, colv, cin, Wl, Wl + h * 2 * cin, h, fout);
    }
}

// Readout column sums in fp64 (k_ccn_readout_part's order for a one-chunk graph): vec[col0 + c] =
// sum over rows r of val(r, c), rows over the first 256 threads, then their 4 waves.
template <int CF, typename V>
__device__ __forceinline__ void cs_colsum(const CsLds& s, int rows, int C, int col0, V val) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double acc[CF];
#pragma unroll
    for (int c = 0; c < CF; ++c) acc[c] = 0.0;
    if (threadIdx.x < CS_RT)
        for (int r = threadIdx.x; r < rows; r += CS_RT)
#pragma unroll
            for (int c = 0; c < CF; ++c)
                if (c < C) acc[c] += val(r, c);
#pragma unroll
    for (int c = 0; c < CF; ++c) {
        if (c >= C) break;
        const double t = wave_sum_d(acc[c]);
        if (lane == 0) s.dred[wv * CS_CF + c] = t;
    }
    __syncthreads();
    if ((int)threadIdx.x < C) {
        const int c = threadIdx.x;
        s.vec[col0 + c] = (float)(s.dred[c] + s.dred[CS_CF + c] + s.dred[2 * CS_CF + c] + s.dred[3 * CS_CF + c]);
    }
    __syncthreads();
}

__device__ __forceinline__ int cs_nodes(const CsArgs& a, int b, uint32_t& bad) {
    int n = a.n_batch ? (int)a.n_batch[b] : a.nmax;
    if (n < 0 || n > a.nmax) {
        bad |= ERR_SIZES;
        n = n < 0 ? 0 : a.nmax;
    }
    return n;
}

// Output o of the fc layer without its bias, in fp64 (k_ccn_readout's order): sum_k fcw[o][k] vec[k] over the
// first 256 threads, then their 4 waves.  Valid in thread 0.
__device__ __forceinline__ double cs_fc(const CsArgs& a, const CsLds& s, int o, int nf) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double acc = 0.0;
    if (threadIdx.x < CS_RT)
        for (int k = threadIdx.x; k < nf; k += CS_RT) acc += (double)a.fcw[o * nf + k] * (double)s.vec[k];
    acc = wave_sum_d(acc);
    __syncthreads();
    if (lane == 0) s.dred[wv] = acc;
    __syncthreads();
    return s.dred[0] + s.dred[1] + s.dred[2] + s.dred[3];
}

// One level of the backward walk (node pass, parameter gradients, gather), CF = this level's channel
// bound (levels of hidden <= 2 take CF = 2: a quarter of the loads and selects of the 8-channel form).
// DX = false (the training kernel, which needs no input gradient): level 0 ends after its parameter gradients.
template <int CF, int CH, bool DX = true, bool SPILL = false>
__device__ void cs_bwd_level(const CsArgs& a, const CsLds& s, int b, int l, int n, int G, const float* Xg,
                             const float* dFc, float* dFn) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    (void)wv;
    const int h = a.h, f = a.f, L = a.L;
    (void)L;
    const int p0 = h * 2 * f + h, p1 = h * 2 * h + h;
    const int cin = l == 0 ? f : h, k2 = 2 * cin;
    const float* W = s.Ws + cs_woff(l, f, h);
    const float* Fl = s.F + (size_t)l * a.rcap * h;
    const float* fin = l == 0 ? nullptr : s.F + (size_t)(l - 1) * a.rcap * h;
    const bool top = l == L - 1;
    const float* dtop = s.vec + f + (L - 1) * h;
    // node pass: dpre = dF relu', per-lane parameter sums, dcoll = W^T dpre (k_ccn1_bwd_node's order)
    float aw[CH][CF], ac[CH][CF], ab[CH];
#pragma unroll
    for (int o = 0; o < CH; ++o) {
        ab[o] = 0.f;
#pragma unroll
        for (int c = 0; c < CF; ++c) aw[o][c] = ac[o][c] = 0.f;
    }
    for (int base = 0; base < n; base += CS_NW * (64 / G)) {
        const CsSlot sl = cs_slot(base, G, n);
        float rs[CF], colv[CF];
        cs_collect<CF, SPILL>(s, sl, G, Xg, fin, cin, rs, colv);
        const int ii = sl.i >= 0 ? sl.i : 0;
        const bool vx = sl.i >= 0 && sl.p < s.deg[ii];
        const int row = s.off1[ii] + sl.p;
        float dp[CH];
#pragma unroll
        for (int o = 0; o < CH; ++o) {
            float g;
            if constexpr (SPILL) g = top ? ((CsLdsPtr)dtop)[o] : ((CsGlobalPtr)dFc)[row * h + o];
            else g = top ? dtop[o] : dFc[row * h + o];  // unconditional LDS reads
            dp[o] = (vx && o < h && Fl[row * h + o] > 0.f) ? g : 0.f;
            ab[o] += dp[o];
#pragma unroll
            for (int c = 0; c < CF; ++c) {
                aw[o][c] = fmaf(dp[o], rs[c], aw[o][c]);
                ac[o][c] = fmaf(dp[o], colv[c], ac[o][c]);
            }
        }
        if (vx)
            for (int k = 0; k < k2; ++k) {
                float t = 0.f;
#pragma unroll
                for (int o = 0; o < CH; ++o)
                    if (o < h) t = fmaf(W[o * k2 + k], dp[o], t);
                s.dcoll[row * k2 + k] = t;
            }
    }
    // level parameter gradients: lanes, then the waves in order
#pragma unroll
    for (int o = 0; o < CH; ++o) {
        if (o >= h) break;
#pragma unroll
        for (int c = 0; c < CF; ++c) {
            if (c >= cin) break;
            const float tw = wave_total(aw[o][c]);
            const float tc = wave_total(ac[o][c]);
            if (lane == 0) {
                s.red[wv * CS_PMAX + o * k2 + c] = tw;
                s.red[wv * CS_PMAX + o * k2 + cin + c] = tc;
            }
        }
        const float tb = wave_total(ab[o]);
        if (lane == 0) s.red[wv * CS_PMAX + h * k2 + o] = tb;
    }
    __syncthreads();
    const int P = h * k2 + h;
    for (int p = threadIdx.x; p < P; p += CS_NT) {
        float v = s.red[p];
#pragma unroll
        for (int w = 1; w < CS_NW; ++w) v += s.red[w * CS_PMAX + p];
        if (a.bs == 1) {
            if (p < h * k2) a.gW[l][p] = v;
            else a.gB[l][p - h * k2] = v;
        } else {
            const int poff = l == 0 ? 0 : p0 + (l - 1) * p1;
            a.ppart[(long long)b * (p0 + (L - 1) * p1) + poff + p] = v;
        }
    }
    if (!DX && l == 0) {  // no dX wanted: the level-0 gather is skipped
        __syncthreads();
        return;
    }
    // gather: dF_{l-1}[j][u] = sum_{i in N(j)} [q valid] (drow_i[q] + dcol_i[pos of j]) + readout term;
    // level 0: dX[j] = the sum over u + d_j dsum  (k_ccn1_bwd_gather's order)
    for (int base = 0; base < n; base += CS_NW * (64 / G)) {
        const CsSlot sl = cs_slot(base, G, n);
        const int j = sl.i >= 0 ? sl.i : 0;
        const int d = sl.i >= 0 ? s.deg[j] : 0;
        const bool vu = sl.p < d;
        const int uu = s.nbr[j * 64 + (vu ? sl.p : 0)];
        const unsigned long long bu = (1ull << uu) - 1ull, bj = (1ull << j) - 1ull;
        const int dl = d > 0 ? d - 1 : 0;
        float acc[CF];
#pragma unroll
        for (int c = 0; c < CF; ++c) acc[c] = 0.f;
        for (int a0 = 0; a0 < G; a0 += 4) {
            int ik[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) ik[q] = s.nbr[j * 64 + min(a0 + q, dl)];
            unsigned long long m[4];
            int ri[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                m[q] = s.bits[ik[q]];
                ri[q] = s.off1[ik[q]];
            }
            float t1[4][CF], t2[4][CF];
            bool ok[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                ok[q] = vu && ((m[q] >> uu) & 1ull) && a0 + q < d;
                const float* s1 = s.dcoll + (ri[q] + __popcll(m[q] & bu)) * k2;
                const float* s2 = s.dcoll + (ri[q] + __popcll(m[q] & bj)) * k2 + cin;
#pragma unroll
                for (int c = 0; c < CF; ++c) {  // unconditional LDS reads, discarded by the selects
                    t1[q][c] = s1[c];
                    t2[q][c] = s2[c];
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int c = 0; c < CF; ++c)
                    acc[c] += (c < cin && ok[q]) ? t1[q][c] + t2[q][c] : 0.f;
        }
        if (l > 0) {
            if (vu)
#pragma unroll
                for (int c = 0; c < CF; ++c)
                    if (c < cin) dFn[(s.off1[j] + sl.p) * cin + c] = acc[c] + s.vec[f + (l - 1) * h + c];
        } else {
            // the node's G lanes summed by an xor tree: with zeros past d this is wave_total's association
#pragma unroll
            for (int c = 0; c < CF; ++c) {
                if (c >= cin) break;
                float tot = vu ? acc[c] : 0.f;
                for (int o = 1; o < G; o <<= 1) tot += __shfl_xor(tot, o, 64);
                if (sl.i >= 0 && sl.p == 0) a.dX[((long long)b * a.nmax + j) * f + c] = tot + (float)d * s.vec[c];
            }
        }
    }
    __syncthreads();
}

// ---------------------------------------------------------------- the stages of a kernel
// Graph b opened: its node count, the staging round and the plan (n, nbr, bits, deg, off1 in LDS); the lanes'
// validation bits are OR-ed into `bad`.  ST: the one-shot forward's phase stamps.
template <bool ST = false>
__device__ __forceinline__ int cs_open(const CsArgs& a, int b, const CsLds& s, float* As, uint32_t& bad) {
    const int n = cs_nodes(a, b, bad);
    cs_stage(a, b, n, s, As);
    if constexpr (ST) CS_STAMP(1);
    bad |= cs_plan(n, s, As);
    if constexpr (ST) CS_STAMP(2);
    return n;
}

// the lanes' validation bits into the block's word
__device__ __forceinline__ void cs_report(uint32_t bad, uint32_t& sbad) {
    bad = wave_or(bad);
    if ((threadIdx.x & 63) == 0 && bad) atomicOr(&sbad, bad);
}

// Forward walk with every level kept: level l's rows at s.F + l * rcap * h (levels of <= 2 input channels take the
// CF = 2 form)
template <int CF, bool SPILL>
__device__ __forceinline__ void cs_levels_keep(const CsArgs& a, const CsLds& s, int n, int G, const float* Xg) {
    const int f = a.f, h = a.h;
    for (int l = 0; l < a.L; ++l) {
        const int cin = l == 0 ? f : h;
        const float* fin = l == 0 ? nullptr : s.F + (size_t)(l - 1) * a.rcap * h;
        float* fout = s.F + (size_t)l * a.rcap * h;
        const float* Wl = s.Ws + cs_woff(l, f, h);
        if (cin <= 2) [[clang::always_inline]] cs_fwd_level<2, SPILL>(s, n, G, Xg, fin, cin, Wl, h, fout);
        else [[clang::always_inline]] cs_fwd_level<CF, SPILL>(s, n, G, Xg, fin, cin, Wl, h, fout);
        __syncthreads();
    }
}

// The readout features of the kept levels into s.vec: level 0's sum_i d_i X[i] (utils_ccn.py:212-216 tiles X[i] d_i
// times), then every level's column sums over the graph's `rows` rows
template <int CF>
__device__ __forceinline__ void cs_readout_sums(const CsArgs& a, const CsLds& s, int n, int rows, const float* Xg) {
    const int f = a.f, h = a.h;
    cs_colsum<CF>(s, n, f, 0, [&](int r, int c) { return (double)s.deg[r] * (double)Xg[r * f + c]; });
    for (int l = 0; l < a.L; ++l) {
        const float* fl = s.F + (size_t)l * a.rcap * h;
        cs_colsum<CF>(s, rows, h, f + l * h, [&](int r, int c) { return (double)fl[r * h + c]; });
    }
}

// out = fc(feat) in fp64 (k_ccn_readout's order) from the features in s.vec: out_row[o], and keep[o] when the kernel
// goes on with the row (keep: LDS, read after the caller's next barrier)
__device__ __forceinline__ void cs_out_row(const CsArgs& a, const CsLds& s, int nf, int n_out, float* out_row,
                                           float* keep) {
    for (int o = 0; o < n_out; ++o) {
        const double v = cs_fc(a, s, o, nf);
        if (threadIdx.x == 0) {
            const float ov = (float)(v + (double)a.fcb[o]);
            out_row[o] = ov;
            if (keep) keep[o] = ov;
        }
    }
}

// dsum[k] = sum_o dout[o] fcw[o][k] (k_ccn_readout_bwd's order) into s.vec, dob being the graph's dout row.
__device__ __forceinline__ void cs_dsum(const CsArgs& a, const CsLds& s, const float* dob, int nf) {
    for (int k = threadIdx.x; k < nf; k += CS_NT) {
        float t = 0.f;
        for (int o = 0; o < a.n_out; ++o) t = fmaf(dob[o], a.fcw[o * nf + k], t);
        s.vec[k] = t;
    }
}

// The fc gradients of one graph, written directly; feat: the graph's readout features, its workspace row or s.vec
// before cs_dsum takes it
__device__ __forceinline__ void cs_fc_grads(const CsArgs& a, const float* dob, const float* feat, int nf) {
    for (int w = threadIdx.x; w < a.n_out * nf + a.n_out; w += CS_NT) {
        if (w < a.n_out * nf) a.gfcw[w] = (float)((double)dob[w / nf] * (double)feat[w % nf]);
        else a.gfcb[w - a.n_out * nf] = (float)(double)dob[w - a.n_out * nf];
    }
}

// Backward level walk on the plan and the kept levels, dsum in s.vec: the top level down, the two dF buffers swapped
// after each (graph b's partials or gradients, and with DX its dX rows)
template <int CF, int CH, bool DX, bool SPILL>
__device__ __forceinline__ void cs_backward(const CsArgs& a, const CsLds& s, int b, int n, int G, const float* Xg) {
    float* dFc = s.dF0;
    float* dFn = s.dF1;
    for (int l = a.L - 1; l >= 0; --l) {
        if ((l == 0 ? a.f : a.h) <= 2)
            [[clang::always_inline]] cs_bwd_level<2, CH, DX, SPILL>(a, s, b, l, n, G, Xg, dFc, dFn);
        else [[clang::always_inline]] cs_bwd_level<CF, CH, DX, SPILL>(a, s, b, l, n, G, Xg, dFc, dFn);
        float* t = dFc;
        dFc = dFn;
        dFn = t;
    }
}

// ---------------------------------------------------------------- per-element pair of the sums over graphs
// Flat parameter element e (the levels in Ws' order -- ppart's -- then fc weight and bias) -> tensor ti (the
// parameter list's index) and offset q in it.  nw = cs_woff(L, f, h) level entries and nfc = n_out nf fc weights: the
// caller's, which has them for its bound (and the training loop keeps them out of its per-graph loop).
__device__ __forceinline__ void cs_param_elem(const CsArgs& a, int nw, int nfc, int e, int& ti, int& q) {
    if (e < nw) {
        int l = 0;
        while (l + 1 < a.L && e >= cs_woff(l + 1, a.f, a.h)) ++l;
        q = e - cs_woff(l, a.f, a.h);
        const int hk = a.h * 2 * (l == 0 ? a.f : a.h);
        ti = 2 * l + (q < hk ? 0 : 1);
        q = q < hk ? q : q - hk;
    } else {
        ti = 2 * a.L + (e < nw + nfc ? 0 : 1);
        q = e - nw - (e < nw + nfc ? 0 : nfc);
    }
}
// tensor ti's gradient
__device__ __forceinline__ float* cs_grad(const CsArgs& a, int ti) {
    if (ti < 2 * a.L) return (ti & 1) ? a.gB[ti >> 1] : a.gW[ti >> 1];
    return ti == 2 * a.L ? a.gfcw : a.gfcb;
}

// Flat element w summed over B graphs in fp64, lane-strided (k_ccn_readout_bwd's order for the fc entries, from
// dout [B][n_out] and the readout features); the wave's sum
__device__ __forceinline__ double cs_sum_elem(const CsArgs& a, const float* dout, int B, int w) {
    const int lane = threadIdx.x & 63;
    const int nf = a.f + a.L * a.h, ptot = cs_woff(a.L, a.f, a.h);
    double s = 0.0;
    if (w < ptot) {
        for (int b = lane; b < B; b += 64) s += (double)a.ppart[(long long)b * ptot + w];
    } else if (w < ptot + a.n_out * nf) {
        const int o = (w - ptot) / nf, k = (w - ptot) % nf;
        for (int b = lane; b < B; b += 64) s += (double)dout[b * a.n_out + o] * (double)a.feat[(long long)b * nf + k];
    } else {
        const int o = w - ptot - a.n_out * nf;
        for (int b = lane; b < B; b += 64) s += (double)dout[b * a.n_out + o];
    }
    return wave_sum_d(s);
}

// ---------------------------------------------------------------- host
// the advertised bounds; the SPILL kernels take every shape within them
bool cs_spill_ok(const hgnn_ccn_config* c) {
    return c && c->order == 1 && c->bs > 0 && c->nmax > 0 && c->nmax <= 64 && c->f_in > 0 && c->f_in <= CS_CF &&
           c->hidden > 0 && c->hidden <= CS_CF && c->layers >= 1 && c->layers <= CS_LMAX && c->n_out > 0;
}

// the LDS kernels: also the backward's LDS figure
bool cs_ok(const hgnn_ccn_config* c) {
    return cs_spill_ok(c) && cs_lds_bytes(c->nmax * c->nmax, c->f_in, c->hidden, c->layers, true) <= CS_LDS_MAX;
}

// whether the training kernels take graphs of this model padded to cfg->nmax (bs is not looked at)
template <bool SPILL>
bool cs_train_ok(const hgnn_ccn_config* cfg) {
    if (!cfg) return false;
    hgnn_ccn_config one = *cfg;
    one.bs = 1;
    return (SPILL ? cs_spill_ok(&one) : cs_ok(&one)) && one.n_out <= CS_OMAX;
}

// readout width, level parameter entries, and all parameter entries (the grid of the sums over graphs)
int cs_nf(const hgnn_ccn_config* c) { return c->f_in + c->layers * c->hidden; }
size_t cs_ptot(const hgnn_ccn_config* c) {
    const int h = c->hidden, f = c->f_in;
    return (size_t)(h * 2 * f + h) + (size_t)(c->layers - 1) * (h * 2 * h + h);
}
int cs_nouts(const hgnn_ccn_config* c) { return (int)cs_ptot(c) + c->n_out * cs_nf(c) + c->n_out; }

// bytes of the one-shot calls' feat / ppart part of the workspace
size_t cs_head_bytes(const hgnn_ccn_config* c) {
    return (4 * (size_t)c->bs * cs_nf(c) + 255) / 256 * 256 + (c->bs > 1 ? 4 * (size_t)c->bs * cs_ptot(c) : 0);
}

// SPILL: the workspace starts with the row regions (region b at b * rstride floats; `regions` of them), then the
// feat / ppart part as the LDS kernels lay it out
template <bool SPILL = false>
CsArgsT<SPILL> cs_args(const hgnn_ccn_config* c, const float* X, const float* adj, const int64_t* nb,
                       const float* const* params, void* ws, int regions = 0) {
    CsArgsT<SPILL> a{};
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
    if constexpr (SPILL) {
        a.rows = static_cast<float*>(ws);
        a.rstride = (long long)cs_spill_stride(a.rcap, a.f, a.h, a.L);
        ws = ws ? static_cast<char*>(ws) + 4 * (size_t)regions * a.rstride : nullptr;
    }
    a.feat = static_cast<float*>(ws);
    if (ws) a.ppart = reinterpret_cast<float*>(static_cast<char*>(ws) + (4 * (size_t)c->bs * cs_nf(c) + 255) / 256 * 256);
    return a;
}

void cs_set_grads(CsArgs& a, float* const* grads) {
    for (int l = 0; l < a.L; ++l) {
        a.gW[l] = grads[2 * l];
        a.gB[l] = grads[2 * l + 1];
    }
    a.gfcw = grads[2 * a.L];
    a.gfcb = grads[2 * a.L + 1];
}

// dynamic LDS of a launch; SPILL: at most 37.2 KB at nmax = 64, within the static limit (no opt-in)
template <bool SPILL>
size_t cs_lds_for(const CsArgs& a, bool bwd) {
    return SPILL ? cs_spill_lds_bytes(a.rcap) : cs_lds_bytes(a.rcap, a.f, a.h, a.L, bwd);
}

// dynamic LDS opt-in of a kernel, once per instantiation (`done` is the caller's static flag)
template <typename K>
void cs_lds_attr(K kernel, bool& done) {
    if (!done) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)CS_LDS_MAX);
        (void)hipGetLastError();  // a refused opt-in shows at the launch, not here
        done = true;
    }
}

// Launch of a kernel that exists as K2 (CH = 2, hidden <= 2) and K8 (CH = CS_CF), with the pick's LDS opt-in
template <auto K2, auto K8, bool SPILL, typename... Args>
void cs_launch_ch(int hidden, int blocks, size_t lds, hipStream_t s, const Args&... args) {
    static bool attr2 = SPILL, attr8 = SPILL;
    if (hidden <= 2) {
        cs_lds_attr(K2, attr2);
        HGNN_KLAUNCH(K2, dim3(blocks), dim3(CS_NT), lds, s, args...);
    } else {
        cs_lds_attr(K8, attr8);
        HGNN_KLAUNCH(K8, dim3(blocks), dim3(CS_NT), lds, s, args...);
    }
}

}  // namespace
}  // namespace hgnn
