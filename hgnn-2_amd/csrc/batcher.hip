// Device batcher: the CSR batch image of csrc/builder.cpp (hgnn_csr_batch_build), built on the device from
// a resident graph pack (hgnn_amd.dataset.DevicePack), byte for byte.
//
// k_batch_graph   one workgroup per graph: the graph's operators, restated from builder.cpp, in LDS.
//                 COUNT: only the graph's record {n, m, nnz[6], flags, 0}; otherwise the graph's rows,
//                 entries, packed x and xl at the places k_batch_offsets gave it.
// k_batch_offsets one workgroup per batch: exclusive prefixes of the batch's records -> node_off, edge_off,
//                 totals, N_batch, E_batch in the image and each graph's starts in the scratch table.
//
// The image equals the host's because every number in it is formed as the host forms it: the operator
// values are copies of A's weights, fp64 sums over ascending k with a separate multiply and add (the host is
// compiled without FMA contraction: __dmul_rn / __dadd_rn here), rounded to fp32 once per squaring, and
// everything else is integer counting.  A dense accumulation over a row's pattern visits exactly the terms
// the host's sparse rows hold, in the same order.
//
// Bounds: J + 2 <= 5, and per graph what one workgroup holds in LDS (BtCaps): with the line graph (dual) n <= 32,
// m <= 72 (k_extract_reg's QM9 bounds); the node family alone (dual == 0) n <= 64, where a row's pattern is two
// 32-bit words.  Both are instantiations of the one kernel.  A dual == 0 batch whose largest graph has at most
// 32 nodes is built by the narrow instantiation.  LDS per workgroup at J + 2 = 3 / 4 / 5: see DESIGN.md §4 (the
// m x m fp32 tiles of base^2 and base^4 are the bulk; the base slice is not stored: A is its own tile, and
// AL[a][b] is w(b) under a condition on the edge table).
#include <string.h>

#include "common.h"

namespace hgnn {

// csrc/builder.cpp: the image's field order and offsets from the counts
void csr_layout_offsets(hgnn_csr_layout& L);

namespace {

constexpr int BT_THREADS = 256;
constexpr int BT_HDR = 4;    // scratch: header words {ok, 0, 0, 0}
constexpr int BT_TAB = 12;   // scratch words per batch graph: {graph, skip, node0, edge0, entry start[6], 0, 0}
enum { K_W = 0, K_WT = 1, K_WL = 2, K_WLT = 3, K_PN = 4, K_PE = 5, K_N = 6 };

// What one workgroup can hold.  NCAP: nodes, and the stride of the A tile; MCAP: rows of the widest family (edge
// slots with the line graph, nodes without), and the stride of the base^2 / base^4 tiles; MW: 32-bit words of a
// row's column bitmap; LINE: the line-graph family (edge table, WL, Pm / Pd) is built when the launch is dual.
template <int NCAP_, int MCAP_, bool LINE_>
struct BtCaps {
    static constexpr int NCAP = NCAP_, MCAP = MCAP_, MW = (MCAP_ + 31) / 32;
    static constexpr bool LINE = LINE_;
    static constexpr int LN = LINE_ ? NCAP_ : 1, LM = LINE_ ? MCAP_ : 1;  // extents of what only LINE uses
};
using BtNarrow = BtCaps<32, 72, true>;  // both families (k_extract_reg's QM9 bounds); the builder of every dual launch
using BtWide = BtCaps<64, 64, false>;   // the node family alone: a row's pattern is 64 bits

template <int JT, class C>
struct BtLds {
    float A[C::NCAP * C::NCAP];
    uint32_t mb[C::MCAP][C::MW], m2[C::MCAP][C::MW], m4[C::MCAP][C::MW];  // patterns of base, base^2, base^4
    uint32_t U[C::MCAP][C::MW], UT[C::MCAP][C::MW];                        // the union pattern and its transpose
    int rstart[C::MCAP], tstart[C::MCAP];
    float deg[C::MCAP];
    int esrc[C::LM], etgt[C::LM];
    float ew[C::LM];
    uint32_t pn[C::LN][C::MW], pe[C::LM];  // incidence patterns: node -> slots, slot -> nodes
    int pnstart[C::LN], pestart[C::LM];
    uint32_t rowmask[C::LN];
    int rowpre[C::LN];
    int m, B, bad, nnz, nnzp;
    unsigned char inc[C::LN][C::LM];  // 0: none, 1: Pm = 1, Pd = 1, 2: Pm = 1, Pd = -1
    // (not zeroed: written over [0, dim) x [0, dim) before they are read)
    float p2[JT >= 4 ? C::MCAP * C::MCAP : 1];
    float p4[JT >= 5 ? C::MCAP * C::MCAP : 1];
};

template <int MW>
__device__ __forceinline__ int bt_bits(const uint32_t* row) {
    int p = __popc(row[0]);
#pragma unroll
    for (int w = 1; w < MW; ++w) p += __popc(row[w]);
    return p;
}
// set bits of the row below column c
template <int MW>
__device__ __forceinline__ int bt_rank(const uint32_t* row, int c) {
    int p = __popc(row[c >> 5] & ((1u << (c & 31)) - 1u));
#pragma unroll
    for (int w = 1; w < MW; ++w)
        if (c >= 32 * w) p += __popc(row[w - 1]);
    return p;
}
__device__ __forceinline__ bool bt_has(const uint32_t* row, int c) { return (row[c >> 5] >> (c & 31)) & 1u; }

template <int LD>
struct BaseA {  // the node graph: A itself
    const float* A;
    __device__ __forceinline__ float val(int r, int c) const { return A[r * LD + c]; }
};
struct BaseL {  // the line graph: AL[a][b] = w(b) iff tgt(a) == src(b) and src(a) != tgt(b) (builder.cpp line_graph)
    const int *src, *tgt;
    const float* w;
    __device__ __forceinline__ float val(int a, int b) const {
        return tgt[a] == src[b] && src[a] != tgt[b] ? w[b] : 0.f;
    }
};

struct BtOut {  // where one operator family of one graph goes (not read in COUNT mode)
    RowInfo *rows, *rowsT;
    float *ent, *entT;
    float* deg;  // xl, or null
    int row0, ent0, entT0, expect, expectT;
};

struct BtArgs {
    hgnn_pack_view v;
    const int32_t* counts;  // the pack's records (build mode)
    int32_t* counts_out;    // COUNT mode
    const int32_t* tab;     // scratch of k_batch_offsets (build mode)
    int dual;
    float *x, *xl;
    RowInfo* rows[K_N];
    float* ent[K_N];
};

// dst = src^2 over the pattern `mask` of src, as builder.cpp square(): per (i, j) the products a(i,k) * b(k,j) of
// the entries both rows hold, k ascending, in fp64; an entry where the sum is not 0.0, its value rounded to fp32.
template <class C, class Src>
__device__ __forceinline__ void bt_square(int dim, Src src, const uint32_t (*mask)[C::MW], float* dst,
                                          uint32_t (*dmask)[C::MW]) {
    for (int idx = threadIdx.x; idx < dim * dim; idx += BT_THREADS) {
        const int i = idx / dim, j = idx - i * dim;
        double acc = 0.0;
        for (int w = 0; w < C::MW; ++w) {
            uint32_t bits = mask[i][w];
            while (bits) {
                const int k = 32 * w + __ffs(bits) - 1;
                bits &= bits - 1u;
                if (bt_has(mask[k], j)) acc = __dadd_rn(acc, __dmul_rn((double)src(i, k), (double)src(k, j)));
            }
        }
        dst[i * C::MCAP + j] = (float)acc;
        if (acc != 0.0) atomicOr(&dmask[i][j >> 5], 1u << (j & 31));
    }
}

// One operator family (builder.cpp slices() + transpose()) of a dim x dim base: the slices I, diag(row sum), base,
// base^2, base^4 as one row list over the union pattern, and its transpose.  Returns the entry count; writes the
// lists only if it is the count the records promised.  Every thread of the workgroup calls it.
template <int JT, bool COUNT, class C, class Base>
__device__ int bt_family(BtLds<JT, C>& s, int dim, Base base, const BtOut& o, int col0) {
    constexpr int SW = JT <= 3 ? 4 : 8;
    const int tid = threadIdx.x;
    for (int t = tid; t < C::MCAP * C::MW; t += BT_THREADS) {
        const int r = t / C::MW, w = t - r * C::MW;
        uint32_t bits = 0u;
        if (r < dim)
            for (int c = 32 * w; c < min(32 * w + 32, dim); ++c) bits |= (uint32_t)(base.val(r, c) != 0.f) << (c & 31);
        s.mb[r][w] = bits;
        s.m2[r][w] = 0u;
        s.m4[r][w] = 0u;
    }
    __syncthreads();
    if (tid < dim) {
        double d = 0.0;
        for (int w = 0; w < C::MW; ++w) {
            uint32_t bits = s.mb[tid][w];
            while (bits) {
                const int c = 32 * w + __ffs(bits) - 1;
                bits &= bits - 1u;
                d = __dadd_rn(d, (double)base.val(tid, c));
            }
        }
        s.deg[tid] = (float)d;
    }
    if constexpr (JT >= 4) {
        bt_square<C>(dim, [&](int r, int c) { return base.val(r, c); }, s.mb, s.p2, s.m2);
        __syncthreads();
    }
    if constexpr (JT >= 5) {
        bt_square<C>(dim, [&](int r, int c) { return s.p2[r * C::MCAP + c]; }, s.m2, s.p4, s.m4);
        __syncthreads();
    }
    for (int t = tid; t < dim * C::MW; t += BT_THREADS) {
        const int r = t / C::MW, w = t - r * C::MW;
        uint32_t u = s.mb[r][w] | s.m2[r][w] | s.m4[r][w];
        if ((r >> 5) == w) u |= 1u << (r & 31);  // the diagonal is always present (slice I)
        s.U[r][w] = u;
    }
    __syncthreads();
    for (int t = tid; t < dim * C::MW; t += BT_THREADS) {
        const int c = t / C::MW, w = t - c * C::MW;
        uint32_t bits = 0u;
        for (int r = 32 * w; r < min(32 * w + 32, dim); ++r) bits |= (uint32_t)bt_has(s.U[r], c) << (r & 31);
        s.UT[c][w] = bits;
    }
    __syncthreads();
    if (tid < dim) {
        int rs = 0, ts = 0;
        for (int q = 0; q < tid; ++q) {
            rs += bt_bits<C::MW>(s.U[q]);
            ts += bt_bits<C::MW>(s.UT[q]);
        }
        s.rstart[tid] = rs;
        s.tstart[tid] = ts;
        if (tid == dim - 1) s.nnz = rs + bt_bits<C::MW>(s.U[tid]);
    }
    if (dim == 0 && tid == 0) s.nnz = 0;
    __syncthreads();
    const int nnz = s.nnz;
    if constexpr (!COUNT) {
        if (nnz == o.expect && nnz == o.expectT) {
            if (tid < dim) {
                o.rows[o.row0 + tid] = RowInfo{o.ent0 + s.rstart[tid], bt_bits<C::MW>(s.U[tid])};
                o.rowsT[o.row0 + tid] = RowInfo{o.entT0 + s.tstart[tid], bt_bits<C::MW>(s.UT[tid])};
                if (o.deg) o.deg[tid] = s.deg[tid];
            }
            for (int idx = tid; idx < dim * dim; idx += BT_THREADS) {
                const int r = idx / dim, c = idx - r * dim;
                if (!bt_has(s.U[r], c)) continue;
                const bool dg = r == c;
                const float v0 = dg ? 1.f : 0.f, v1 = dg ? s.deg[r] : 0.f, v2 = base.val(r, c);
                float* e = o.ent + (size_t)(o.ent0 + s.rstart[r] + bt_rank<C::MW>(s.U[r], c)) * SW;
                float* et = o.entT + (size_t)(o.entT0 + s.tstart[c] + bt_rank<C::MW>(s.UT[c], r)) * SW;
                *reinterpret_cast<float4*>(e) = make_float4(__int_as_float(col0 + c), v0, v1, v2);
                *reinterpret_cast<float4*>(et) = make_float4(__int_as_float(col0 + r), v0, v1, v2);
                if constexpr (SW == 8) {
                    const float v3 = s.p2[r * C::MCAP + c], v4 = JT >= 5 ? s.p4[r * C::MCAP + c] : 0.f;
                    *reinterpret_cast<float4*>(e + 4) = make_float4(v3, v4, 0.f, 0.f);
                    *reinterpret_cast<float4*>(et + 4) = make_float4(v3, v4, 0.f, 0.f);
                }
            }
        }
    }
    __syncthreads();  // the patterns and tiles are reused by the next family
    return nnz;
}

__device__ __forceinline__ void bt_record(int32_t* out, long long g, int n, int m, int w, int l, int p, int flags) {
    if (threadIdx.x != 0) return;
    int32_t* r = out + g * HGNN_PACK_COUNT_WORDS;
    r[0] = n;
    r[1] = m;
    r[2] = r[3] = w;
    r[4] = r[5] = l;
    r[6] = r[7] = p;
    r[8] = flags;
    r[9] = 0;
}

template <int JT, bool COUNT, class C>
__global__ void __launch_bounds__(BT_THREADS) k_batch_graph(BtArgs a) {
    using Lds = BtLds<JT, C>;
    __shared__ Lds s;
    const int tid = threadIdx.x;
    long long g;
    const int32_t *tab = nullptr, *rec = nullptr;
    int node0 = 0, edge0 = 0;
    if constexpr (COUNT) {
        g = blockIdx.x;
    } else {
        if (a.tab[0] != 1) return;  // the batch's records do not add up to the layout
        tab = a.tab + BT_HDR + (size_t)blockIdx.x * BT_TAB;
        if (tab[1]) return;
        g = tab[0];
        rec = a.counts + g * HGNN_PACK_COUNT_WORDS;
        node0 = tab[2];
        edge0 = tab[3];
    }
    const long long nn0 = a.v.d_node_off[g], n64 = a.v.d_node_off[g + 1] - nn0;
    const long long a0 = a.v.d_adj_off[g], c64 = a.v.d_adj_off[g + 1] - a0;
    int flags = 0;
    if (n64 < 1 || n64 > C::NCAP) flags = HGNN_PACK_FLAG_BOUNDS;
    else if (c64 < 0 || c64 > n64 * n64) flags = HGNN_PACK_FLAG_COO;  // strictly ascending entries are at most n^2
    if (flags) {
        if constexpr (COUNT) bt_record(a.counts_out, g, (int)max(min(n64, 0x7fffffffll), 0ll), 0, 0, 0, 0, flags);
        return;
    }
    const int n = (int)n64, cnt = (int)c64;
    {
        uint32_t* z = reinterpret_cast<uint32_t*>(&s);
        for (int i = tid; i < (int)(offsetof(Lds, p2) / 4); i += BT_THREADS) z[i] = 0u;
    }
    __syncthreads();
    for (int e = tid; e < cnt; e += BT_THREADS) {
        const int i = a.v.d_adj_ij[2 * (a0 + e)], j = a.v.d_adj_ij[2 * (a0 + e) + 1];
        bool ok = (unsigned)i < (unsigned)n && (unsigned)j < (unsigned)n;
        if (e > 0) {
            const int pi = a.v.d_adj_ij[2 * (a0 + e) - 2], pj = a.v.d_adj_ij[2 * (a0 + e) - 1];
            ok = ok && (pi < i || (pi == i && pj < j));
        }
        if (ok) s.A[i * C::NCAP + j] = a.v.d_adj_w[a0 + e];
        else s.bad = 1;
    }
    __syncthreads();
    if (s.bad) {
        if constexpr (COUNT) bt_record(a.counts_out, g, n, 0, 0, 0, 0, HGNN_PACK_FLAG_COO);
        return;
    }
    int m = 0, B = 0;  // without the line graph there are no edge slots
    if constexpr (C::LINE) {
        static_assert(C::NCAP == 32, "the edge table holds a row of A in one 32-bit word");
        if (tid < n) {
            uint32_t bits = 0u;
            for (int c = 0; c < n; ++c) bits |= (uint32_t)(s.A[tid * C::NCAP + c] != 0.f) << c;
            s.rowmask[tid] = bits;
        }
        __syncthreads();
        if (tid == 0) {
            // m = nnz(A) with the diagonal (Q2); B = the bonds, the upper-triangle nonzeros, ranked row-major
            int m = 0, B = 0;
            for (int r = 0; r < n; ++r) {
                m += __popc(s.rowmask[r]);
                s.rowpre[r] = B;
                B += __popc(s.rowmask[r] & ~((2u << r) - 1u));
            }
            s.m = a.dual ? m : 0;
            s.B = B;
        }
        __syncthreads();
        m = s.m;
        B = s.B;
        if (a.dual && m > C::MCAP) flags = HGNN_PACK_FLAG_BOUNDS;
        else if (a.dual && B > 0 && B >= m) flags = HGNN_PACK_FLAG_INDEX;  // edge_slots(): bond B - 1 writes column B
        if (flags) {
            if constexpr (COUNT) bt_record(a.counts_out, g, n, m, 0, 0, 0, flags);
            return;
        }
    }
    BtOut ow{}, ol{};
    if constexpr (!COUNT) {
        if (rec[0] != n || rec[1] != m || rec[8] != 0) return;
        for (int i = tid; i < n * a.v.f_in; i += BT_THREADS)
            a.x[(size_t)node0 * a.v.f_in + i] = a.v.d_x[nn0 * a.v.f_in + i];
        ow = BtOut{a.rows[K_W], a.rows[K_WT], a.ent[K_W], a.ent[K_WT], nullptr, node0, tab[4 + K_W], tab[4 + K_WT],
                   rec[2 + K_W], rec[2 + K_WT]};
        ol = BtOut{a.rows[K_WL], a.rows[K_WLT], a.ent[K_WL], a.ent[K_WLT], a.xl + edge0, edge0, tab[4 + K_WL],
                   tab[4 + K_WLT], rec[2 + K_WL], rec[2 + K_WLT]};
    }
    const int nnz_w = bt_family<JT, COUNT>(s, n, BaseA<C::NCAP>{s.A}, ow, node0);
    int nnz_l = 0, nnz_p = 0;
    // (without C::LINE this block is never entered and the compiler drops it: the arrays it names have extent 1)
    if (C::LINE && a.dual) {
        // the edge table with the reference's quirk Q1: slot k < B is forward(bond k), slot B is reverse(bond B - 1),
        // later slots stay (0, 0, 0)
        for (int idx = tid; idx < n * C::NCAP; idx += BT_THREADS) {
            const int i = idx >> 5, j = idx & 31;
            const uint32_t up = s.rowmask[i] & ~((2u << i) - 1u);
            if (j > i && ((up >> j) & 1u)) {
                const int k = s.rowpre[i] + __popc(up & ((1u << j) - 1u));
                const float w = s.A[i * C::NCAP + j];
                s.esrc[k] = i;
                s.etgt[k] = j;
                s.ew[k] = w;
                if (k == B - 1) {  // B < m here
                    s.esrc[B] = j;
                    s.etgt[B] = i;
                    s.ew[B] = w;
                }
            }
        }
        __syncthreads();
        // Pm / Pd column k as edge_slots() leaves it: reverse(bond k - 1), then forward(bond k) over it
        if (tid < m) {
            const int k = tid;
            uint32_t nodes = 0u;
            if (k >= 1 && k <= B) {
                const int i = s.esrc[k - 1], j = s.etgt[k - 1];
                s.inc[j][k] = 1;
                s.inc[i][k] = 2;
                nodes |= (1u << i) | (1u << j);
            }
            if (k < B) {
                const int i = s.esrc[k], j = s.etgt[k];
                s.inc[i][k] = 1;
                s.inc[j][k] = 2;
                nodes |= (1u << i) | (1u << j);
            }
            s.pe[k] = nodes;
            while (nodes) {
                const int i = __ffs(nodes) - 1;
                nodes &= nodes - 1u;
                atomicOr(&s.pn[i][k >> 5], 1u << (k & 31));
            }
        }
        __syncthreads();
        if (tid < max(n, m)) {
            int ps = 0, es = 0;
            for (int q = 0; q < tid; ++q) {
                if (q < n) ps += bt_bits<C::MW>(s.pn[q]);
                if (q < m) es += __popc(s.pe[q]);
            }
            if (tid < n) s.pnstart[tid] = ps;
            if (tid < m) s.pestart[tid] = es;
            if (tid == m - 1) s.nnzp = es + __popc(s.pe[tid]);
        }
        if (m == 0 && tid == 0) s.nnzp = 0;
        __syncthreads();
        nnz_p = s.nnzp;
        if constexpr (!COUNT) {
            if (nnz_p == rec[2 + K_PN] && nnz_p == rec[2 + K_PE]) {
                const int pn0 = tab[4 + K_PN], pe0 = tab[4 + K_PE];
                if (tid < n) a.rows[K_PN][node0 + tid] = RowInfo{pn0 + s.pnstart[tid], bt_bits<C::MW>(s.pn[tid])};
                if (tid < m) a.rows[K_PE][edge0 + tid] = RowInfo{pe0 + s.pestart[tid], (int)__popc(s.pe[tid])};
                for (int idx = tid; idx < n * m; idx += BT_THREADS) {
                    const int i = idx / m, k = idx - i * m;
                    const int c = s.inc[i][k];
                    if (!c) continue;
                    const float pd = c == 1 ? 1.f : -1.f;
                    float* e = a.ent[K_PN] + (size_t)(pn0 + s.pnstart[i] + bt_rank<C::MW>(s.pn[i], k)) * 4;
                    float* et = a.ent[K_PE] + (size_t)(pe0 + s.pestart[k] + __popc(s.pe[k] & ((1u << i) - 1u))) * 4;
                    *reinterpret_cast<float4*>(e) = make_float4(__int_as_float(edge0 + k), 1.f, pd, 0.f);
                    *reinterpret_cast<float4*>(et) = make_float4(__int_as_float(node0 + i), 1.f, pd, 0.f);
                }
            }
        }
        nnz_l = bt_family<JT, COUNT>(s, m, BaseL{s.esrc, s.etgt, s.ew}, ol, edge0);
    }
    if constexpr (COUNT) bt_record(a.counts_out, g, n, m, nnz_w, nnz_l, nnz_p, 0);
}

struct BtOffArgs {
    const int32_t *counts, *idx;
    int bs;
    long long graphs;
    int32_t *node_off, *edge_off, *totals;
    long long *nb, *eb;
    int32_t* tab;
    long long expect[8];  // nodes, edges, nnz[6] of the layout
};

// Exclusive prefixes over the batch's records, 256 graphs per pass with a running carry.
__global__ void __launch_bounds__(BT_THREADS) k_batch_offsets(BtOffArgs a) {
    __shared__ long long wsum[BT_THREADS / 64][8];
    __shared__ int bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) bad = 0;
    long long run[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) run[q] = 0;
    __syncthreads();
    for (int base = 0; base < a.bs; base += BT_THREADS) {
        const int b = base + tid;
        long long v[8], x[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = 0;
        int g = -1, skip = 1;
        if (b < a.bs) {
            g = a.idx[b];
            if (g >= 0 && g < a.graphs) {
                const int32_t* rec = a.counts + (long long)g * HGNN_PACK_COUNT_WORDS;
                if (rec[8] == 0) {
                    skip = 0;
#pragma unroll
                    for (int q = 0; q < 8; ++q) v[q] = rec[q];
                }
            }
            if (skip) bad = 1;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            long long t = v[q];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const long long y = __shfl_up(t, o, 64);
                if (lane >= o) t += y;
            }
            x[q] = t;
            if (lane == 63) wsum[wave][q] = t;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            long long before = run[q];
            for (int w = 0; w < BT_THREADS / 64; ++w) {
                if (w < wave) before += wsum[w][q];
                run[q] += wsum[w][q];
            }
            x[q] += before - v[q];
        }
        if (b < a.bs) {
            a.node_off[b] = (int32_t)x[0];
            a.edge_off[b] = (int32_t)x[1];
            a.nb[b] = v[0];
            a.eb[b] = v[1];
            int32_t* t = a.tab + BT_HDR + (size_t)b * BT_TAB;
            t[0] = g;
            t[1] = skip;
#pragma unroll
            for (int q = 0; q < 8; ++q) t[2 + q] = (int32_t)x[q];
            t[10] = t[11] = 0;
        }
        __syncthreads();
    }
    if (tid == 0) {
        a.node_off[a.bs] = (int32_t)run[0];
        a.edge_off[a.bs] = (int32_t)run[1];
        a.totals[0] = (int32_t)run[0];
        a.totals[1] = (int32_t)run[1];
        int ok = bad ? 0 : 1;
        for (int q = 0; q < 8; ++q)
            if (run[q] != a.expect[q] || run[q] > 0x7fffffffll) ok = 0;
        a.tab[0] = ok;
        a.tab[1] = a.tab[2] = a.tab[3] = 0;
    }
}

template <bool COUNT, class C>
int bt_launch(const BtArgs& a, int jt, long long blocks, hipStream_t s) {
    const dim3 grid((unsigned)blocks), block(BT_THREADS);
    switch (jt) {
        case 3: HGNN_KLAUNCH(k_batch_graph<3, COUNT, C>, grid, block, 0, s, a); break;
        case 4: HGNN_KLAUNCH(k_batch_graph<4, COUNT, C>, grid, block, 0, s, a); break;
        case 5: HGNN_KLAUNCH(k_batch_graph<5, COUNT, C>, grid, block, 0, s, a); break;
        default: return HGNN_ERR_UNSUPPORTED;
    }
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

bool view_ok(const hgnn_pack_view* v) {
    return v && v->d_node_off && v->d_x && v->d_adj_off && v->d_adj_ij && v->d_adj_w && v->graphs > 0 &&
           v->graphs < (1ll << 31) && v->f_in > 0;
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

extern "C" {

int hgnn_pack_count(const hgnn_pack_view* view, int J, int dual, int32_t* d_counts, void* stream) {
    if (!view_ok(view) || !d_counts || J < 1) return HGNN_ERR_ARG;
    if (J > 3) return HGNN_ERR_UNSUPPORTED;
    BtArgs a{};
    a.v = *view;
    a.counts_out = d_counts;
    a.dual = dual ? 1 : 0;
    // without the line graph the records are the wide builder's, whichever builder a batch then takes
    hipStream_t s = static_cast<hipStream_t>(stream);
    return a.dual ? bt_launch<true, BtNarrow>(a, J + 2, view->graphs, s)
                  : bt_launch<true, BtWide>(a, J + 2, view->graphs, s);
}

size_t hgnn_csr_batch_build_device_scratch_bytes(int bs) {
    return bs > 0 ? sizeof(int32_t) * (BT_HDR + (size_t)bs * BT_TAB) : 0;
}

int hgnn_csr_batch_build_device(const hgnn_pack_view* view, const int32_t* d_counts, const int32_t* d_idx, int bs,
                                int J, int dual, const hgnn_csr_layout* layout, void* d_image, void* d_scratch,
                                size_t scratch_bytes, void* stream) {
    if (!view_ok(view) || !d_counts || !d_idx || bs <= 0 || J < 1 || !layout || !d_image || !d_scratch)
        return HGNN_ERR_ARG;
    if (J > 3) return HGNN_ERR_UNSUPPORTED;
    if (scratch_bytes < hgnn_csr_batch_build_device_scratch_bytes(bs)) return HGNN_ERR_ARG;
    const int jt = J + 2;
    const hgnn_csr_layout& L = *layout;
    if (L.bs != bs || L.f_in != view->f_in || L.j_tot != jt || L.dual != (dual ? 1 : 0) ||
        L.stride_w != (jt <= 3 ? 4 : 8) || L.nodes < 0 || L.edges < 0)
        return HGNN_ERR_ARG;
    for (int k = 0; k < K_N; ++k)
        if (L.nnz[k] < 0) return HGNN_ERR_ARG;
    hgnn_csr_layout chk = L;  // the offsets must be the ones these counts give: the kernels write by them
    csr_layout_offsets(chk);
    if (memcmp(&chk, &L, sizeof(L)) != 0) return HGNN_ERR_ARG;

    hipStream_t s = static_cast<hipStream_t>(stream);
    char* img = static_cast<char*>(d_image);
    // the host image is memset to 0: alignment gaps and unused stride words must match
    HGNN_HOST_CHECK(hipMemsetAsync(img, 0, (size_t)L.bytes, s));
    BtOffArgs o{};
    o.counts = d_counts;
    o.idx = d_idx;
    o.bs = bs;
    o.graphs = view->graphs;
    o.node_off = reinterpret_cast<int32_t*>(img + L.off_node_off);
    o.edge_off = reinterpret_cast<int32_t*>(img + L.off_edge_off);
    o.totals = reinterpret_cast<int32_t*>(img + L.off_totals);
    o.nb = reinterpret_cast<long long*>(img + L.off_n_batch);
    o.eb = reinterpret_cast<long long*>(img + L.off_e_batch);
    o.tab = static_cast<int32_t*>(d_scratch);
    o.expect[0] = L.nodes;
    o.expect[1] = L.edges;
    for (int k = 0; k < K_N; ++k) o.expect[2 + k] = L.nnz[k];
    HGNN_KLAUNCH(k_batch_offsets, dim3(1), dim3(BT_THREADS), 0, s, o);
    HGNN_LAUNCH_CHECK();
    BtArgs a{};
    a.v = *view;
    a.counts = d_counts;
    a.tab = static_cast<const int32_t*>(d_scratch);
    a.dual = dual ? 1 : 0;
    a.x = reinterpret_cast<float*>(img + L.off_x);
    a.xl = reinterpret_cast<float*>(img + L.off_xl);
    for (int k = 0; k < K_N; ++k) {
        a.rows[k] = reinterpret_cast<RowInfo*>(img + L.off_rows[k]);
        a.ent[k] = reinterpret_cast<float*>(img + L.off_entries[k]);
    }
    // a node-family batch whose largest graph fits the narrow builder takes it; a graph past the chosen builder's
    // node cap (a layout that is not of these records) is left as zeros
    if (!a.dual && L.nmax > BtNarrow::NCAP) return bt_launch<false, BtWide>(a, jt, bs, s);
    return bt_launch<false, BtNarrow>(a, jt, bs, s);
}

}  // extern "C"
