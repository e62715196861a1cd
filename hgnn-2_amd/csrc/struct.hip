// Batch plan + dense padded operators -> per-row sparse operator lists.
//
// The reference keeps every operator as a dense zero-padded tensor and walks it
// with one torch.mm per graph and slice (models/layers/layers_mnb.py:403-409,
// 426-432).  Here the dense inputs of one batch are read once, on device, and
// turned into per-row neighbour lists that the aggregation kernels walk:
//   W  (bs, Nmax, Nmax, J+2)  -> S_W (rows n) and S_WT (rows m)
//   WL (bs, Emax, Emax, J+2)  -> S_WL, S_WLT
//   Pm, Pd (bs, Nmax, Emax)   -> S_PN (node rows) and S_PE (edge rows)
// Each packed row owns a fixed slot of `cap` entries (cap = the dense row
// length) so the build is one pass with no prefix sum across graphs; a ballot
// compacts the nonzeros of each 64-column chunk.  The union of the J+2 slices
// (or of Pm and Pd) is stored once per (row, col), so one gathered feature row
// feeds every slice.
#include "kernels.h"

namespace hgnn {

// Block 0: the batch plan.  Blocks 1..: the weight repack (repack_part), folded into this launch.
__global__ void __launch_bounds__(256) k_plan(const int64_t* __restrict__ nb,
                                              const int64_t* __restrict__ eb, int bs,
                                              int nmax, int emax, BatchMeta m, RepackTable rt) {
    WaveStamp stamp(rt.stamps);
    if (blockIdx.x > 0) {
        const int b = blockIdx.x - 1;
        repack_part(rt, b / rt.y, b % rt.y);
        return;
    }
    __shared__ int sn[256];
    __shared__ int se[256];
    __shared__ int carry[2];
    const int t = threadIdx.x;
    if (t == 0) {
        carry[0] = 0;
        carry[1] = 0;
        *m.err = 0u;  // the call's validation word (this kernel is the first of the forward)
    }
    for (int i = t; i < m.zero64_n; i += 256) m.zero64[i] = 0.0;
    __syncthreads();
    for (int base = 0; base < bs; base += 256) {
        const int i = base + t;
        int vn = 0, ve = 0;
        if (i < bs) {
            long long n = nb[i];
            long long e = eb ? eb[i] : 0;
            if (n < 0 || n > nmax || e < 0 || e > emax) {
                atomicOr(m.err, (uint32_t)ERR_SIZES);
                n = n < 0 ? 0 : (n > nmax ? nmax : n);
                e = e < 0 ? 0 : (e > emax ? emax : e);
            }
            vn = (int)n;
            ve = (int)e;
        }
        sn[t] = vn;
        se[t] = ve;
        __syncthreads();
        // Hillis-Steele inclusive scan (bs is small: one pass per 256 graphs)
        for (int o = 1; o < 256; o <<= 1) {
            int an = t >= o ? sn[t - o] : 0;
            int ae = t >= o ? se[t - o] : 0;
            __syncthreads();
            sn[t] += an;
            se[t] += ae;
            __syncthreads();
        }
        if (i < bs) {
            m.node_off[i] = carry[0] + sn[t] - vn;
            m.edge_off[i] = carry[1] + se[t] - ve;
        }
        __syncthreads();
        if (t == 255) {
            carry[0] += sn[255];
            carry[1] += se[255];
        }
        __syncthreads();
    }
    if (t == 0) {
        m.node_off[bs] = carry[0];
        m.edge_off[bs] = carry[1];
        m.totals[0] = carry[0];
        m.totals[1] = carry[1];
    }
}

int launch_plan(const int64_t* nb, const int64_t* eb, int bs, int nmax, int emax, BatchMeta m,
                hipStream_t s, const RepackTable* rt) {
    RepackTable t{};
    if (rt) t = *rt;
    t.y = repack_y(t);
    t.stamps = clock_stamps((long long)(1 + t.n * t.y) * 4);
    HGNN_KLAUNCH(k_plan, dim3(1 + t.n * t.y), dim3(256), 0, s, nb, eb, bs, nmax, emax, m, t);
    HGNN_LAUNCH_CHECK();
    return 0;
}

// One workgroup per (graph, structure kind).  NC = number of coefficients per
// entry (J+2 for W/WL, 2 for Pm/Pd).  A wave takes RU rows at a time and issues all their
// loads before the first ballot: the per-row load -> ballot -> store chain was latency-bound.
template <int NC>
__device__ void extract_rows(int rows, int cols, int row_packed0, int col_packed0,
                             long long slot0, int cap, const float* __restrict__ s0,
                             const float* __restrict__ s1, long long rs, long long cs,
                             long long js, RowInfo* __restrict__ out_rows,
                             float* __restrict__ entries, int stride, int part = 0, int nparts = 1) {
    constexpr int RU = 8, CH = 2;  // rows per batch, 64-column chunks loaded per batch
    const int lane = threadIdx.x & 63;
    const int nw = blockDim.x >> 6;
    const int wv = part * nw + (threadIdx.x >> 6);  // the block's waves over nparts blocks
    // Loads are unconditional (clamped to a live element) and masked after they land: a load
    // under a per-lane condition made hipcc wait vmcnt(0) right after it, serialising the batch.
    auto ld = [&](int r, int c, float (&v)[NC]) {
        const long long o = (long long)min(r, rows - 1) * rs + (long long)min(c, cols - 1) * cs;
        if constexpr (NC == 2) {  // Pm / Pd
            v[0] = s0[o];
            v[1] = s1[o];
        } else {
#pragma unroll
            for (int j = 0; j < NC; ++j) v[j] = s0[o + j * js];
        }
    };
    auto live = [&](int r, int c, float (&v)[NC]) {
        if (!(r < rows && c < cols))
#pragma unroll
            for (int j = 0; j < NC; ++j) v[j] = 0.f;
    };
    for (int rb = wv * RU; rb < rows; rb += nw * nparts * RU) {
        int cnt[RU];
#pragma unroll
        for (int u = 0; u < RU; ++u) cnt[u] = 0;
        for (int cb = 0; cb < cols; cb += 64 * CH) {
            float v[RU][CH][NC];
#pragma unroll
            for (int u = 0; u < RU; ++u)
#pragma unroll
                for (int h = 0; h < CH; ++h) ld(rb + u, cb + h * 64 + lane, v[u][h]);
#pragma unroll
            for (int u = 0; u < RU; ++u)
#pragma unroll
                for (int h = 0; h < CH; ++h) live(rb + u, cb + h * 64 + lane, v[u][h]);
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                const int r = rb + u;
                if (r >= rows) break;
                const long long slot = slot0 + (long long)r * cap;
#pragma unroll
                for (int h = 0; h < CH; ++h) {
                    const int c = cb + h * 64 + lane;
                    bool nz = false;
#pragma unroll
                    for (int j = 0; j < NC; ++j) nz |= (v[u][h][j] != 0.f);
                    const unsigned long long mask = __ballot(nz);
                    const int pos = __popcll(mask & ((1ull << lane) - 1ull));
                    if (nz) {
                        float* e = entries + (slot + cnt[u] + pos) * stride;
                        e[0] = __int_as_float(col_packed0 + c);
#pragma unroll
                        for (int j = 0; j < NC; ++j) e[1 + j] = v[u][h][j];
                    }
                    cnt[u] += __popcll(mask);
                }
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                const int r = rb + u;
                if (r < rows) {
                    RowInfo ri;
                    ri.start = (int)(slot0 + (long long)r * cap);
                    ri.count = cnt[u];
                    out_rows[row_packed0 + r] = ri;
                }
            }
        }
    }
}

// Transposed kinds (S_WT, S_WLT, S_PE): output row r' is column r' of the dense block, so the
// lanes take 64 consecutive output rows and walk the block's rows in order, CU rows' loads in
// flight at a time -- every load is one coalesced row segment, and each lane appends its own
// row's entries (ascending column, the order extract_rows produces).  (Reading a column per
// wave, as extract_rows does, touched a separate cache line per lane.  Measured alternative, not
// kept: the dense rows split over 16 waves of a 1024-thread block with an LDS count scan --
// 104 vs 40 us for the whole extraction, the redundant waves and barriers cost more than the
// serial walk.)
template <int NC>
__device__ void extract_cols(int rows, int cols, int row_packed0, int col_packed0, long long slot0,
                             int cap, const float* __restrict__ s0, const float* __restrict__ s1,
                             long long rs, long long js, RowInfo* __restrict__ out_rows,
                             float* __restrict__ entries, int stride) {
    const int lane = threadIdx.x & 63;
    const int nw = blockDim.x >> 6, wv = threadIdx.x >> 6;
    constexpr long long cstep = NC == 2 ? 1 : NC;  // dense column stride of this kind
    constexpr int CU = 16;                         // dense rows loaded per batch
    for (int r0 = wv * 64; r0 < rows; r0 += nw * 64) {
        const int r = r0 + lane;
        const int rl = min(r, rows - 1);  // lanes past the last row load a live one, store nothing
        const long long slot = slot0 + (long long)r * cap;
        int cnt = 0;
        for (int cb = 0; cb < cols; cb += CU) {
            float v[CU][NC];
#pragma unroll
            for (int u = 0; u < CU; ++u) {
                const long long o = (long long)min(cb + u, cols - 1) * rs + rl * cstep;  // clamped
                if constexpr (NC == 2) {
                    v[u][0] = s0[o];
                    v[u][1] = s1[o];
                } else {
#pragma unroll
                    for (int j = 0; j < NC; ++j) v[u][j] = s0[o + j * js];
                }
            }
#pragma unroll
            for (int u = 0; u < CU; ++u) {
                const int c = cb + u;
                bool nz = false;
#pragma unroll
                for (int j = 0; j < NC; ++j) nz |= (v[u][j] != 0.f);
                if (nz && c < cols && r < rows) {
                    float* e = entries + (slot + cnt) * stride;
                    e[0] = __int_as_float(col_packed0 + c);
#pragma unroll
                    for (int j = 0; j < NC; ++j) e[1 + j] = v[u][j];
                    ++cnt;
                }
            }
        }
        if (r < rows) out_rows[row_packed0 + r] = RowInfo{(int)slot, cnt};
    }
}

// Flags any nonzero of a dense (R, C, NC) block outside [0, rr) x [0, rc).
__device__ void validate_block(const float* __restrict__ blk, int R, int C, int NC, int rr,
                               int rc, uint32_t* err) {
    const int row = C * NC;
    bool bad = false;
    // whole rows past rr: one flat sweep; rows below rr: only their columns past rc
    // (8 loads in flight per thread: one load per iteration made these sweeps the slowest part
    // of the extraction, 20-30 dependent round trips per block)
    constexpr int U = 8;
    const long long tail0 = (long long)rr * row, total = (long long)R * row;
    const int nt = blockDim.x;
    for (long long i0 = tail0 + threadIdx.x; i0 < total; i0 += (long long)U * nt) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long i = i0 + (long long)u * nt;
            v[u] = blk[i < total ? i : total - 1];  // clamped, unconditional (see extract_rows)
        }
#pragma unroll
        for (int u = 0; u < U; ++u) bad |= v[u] != 0.f;
    }
    const int pad = row - rc * NC;  // padded columns per live row
    if (pad > 0)
        for (int i0 = threadIdx.x; i0 < rr * pad; i0 += U * nt) {
            float v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = min(i0 + u * nt, rr * pad - 1);
                const int r = i / pad, q = i - r * pad;
                v[u] = blk[(long long)r * row + rc * NC + q];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) bad |= v[u] != 0.f;
        }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(err, (uint32_t)ERR_PAD_NONZERO);
}

__device__ void validate_mask(const float* __restrict__ mask, int n, int real, uint32_t* err) {
    // mask[b, i, 0] must be 1 for i < real and 0 beyond (functions/batching.py:182-183)
    bool bad = false;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float v = mask[(long long)i * n];
        const float want = (i < real && real > 0) ? 1.f : 0.f;
        if (v != want) bad = true;
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(err, (uint32_t)ERR_MASK);
}

// Block slots per graph.  Line graph: the dense WL block is the big one (Emax^2 (J+2) floats),
// so its row extraction takes two blocks and all validation sweeps a block of their own; the
// slow slots come first in dispatch order.  GNN_simple: W (+ its validation) and WT.
enum ExtractSlot : int {
    X_WL0 = 0, X_WL1, X_VALID, X_WLT, X_PN, X_W, X_PE, X_WT, X_SLOTS,
};

constexpr int X_THREADS = 256;

template <int JT>
__global__ void __launch_bounds__(X_THREADS) k_extract(ExtractArgs a) {
    const int b = blockIdx.x;
    const int slot = a.dual ? (int)blockIdx.y + a.kind0 : ((int)blockIdx.y + a.kind0 == 0 ? X_W : X_WT);
    const int n0 = a.meta.node_off[b];
    const int nb = a.meta.node_off[b + 1] - n0;
    const int nmax = a.nmax;
    const long long wblk = (long long)nmax * nmax * JT;
    const int emax = a.emax;
    const int e0 = a.dual ? a.meta.edge_off[b] : 0;
    const int eb = a.dual ? a.meta.edge_off[b + 1] - e0 : 0;
    const long long lblk = (long long)emax * emax * JT;
    const long long pblk = (long long)nmax * emax;
    switch (slot) {
        case X_W: {
            const float* src = a.W + b * wblk;
            extract_rows<JT>(nb, nb, n0, n0, (long long)b * nmax * nmax, nmax, src, nullptr,
                             (long long)nmax * JT, JT, 1, a.rows[S_W], a.entries[S_W],
                             a.entry_stride_w);
            if (a.validate) {
                validate_block(src, nmax, nmax, JT, nb, nb, a.meta.err);
                validate_mask(a.mask + (long long)b * nmax * nmax, nmax, nb, a.meta.err);
            }
            break;
        }
        case X_WT: {
            const float* src = a.W + b * wblk;
            extract_cols<JT>(nb, nb, n0, n0, (long long)b * nmax * nmax, nmax, src, nullptr,
                             (long long)nmax * JT, 1, a.rows[S_WT], a.entries[S_WT], a.entry_stride_w);
            break;
        }
        case X_WL0:
        case X_WL1: {
            const float* src = a.WL + b * lblk;
            extract_rows<JT>(eb, eb, e0, e0, (long long)b * emax * emax, emax, src, nullptr,
                             (long long)emax * JT, JT, 1, a.rows[S_WL], a.entries[S_WL],
                             a.entry_stride_w, slot - X_WL0, 2);
            break;
        }
        case X_VALID: {
            if (!a.validate) break;
            validate_block(a.WL + b * lblk, emax, emax, JT, eb, eb, a.meta.err);
            validate_mask(a.mask_lg + (long long)b * emax * emax, emax, eb, a.meta.err);
            validate_block(a.Pm + b * pblk, nmax, emax, 1, nb, eb, a.meta.err);
            validate_block(a.Pd + b * pblk, nmax, emax, 1, nb, eb, a.meta.err);
            break;
        }
        case X_WLT: {
            const float* src = a.WL + b * lblk;
            extract_cols<JT>(eb, eb, e0, e0, (long long)b * emax * emax, emax, src, nullptr,
                             (long long)emax * JT, 1, a.rows[S_WLT], a.entries[S_WLT],
                             a.entry_stride_w);
            break;
        }
        case X_PN: {
            const float* pm = a.Pm + b * pblk;
            const float* pd = a.Pd + b * pblk;
            extract_rows<2>(nb, eb, n0, e0, (long long)b * nmax * emax, emax, pm, pd, emax,
                            1, 0, a.rows[S_PN], a.entries[S_PN], 4);
            break;
        }
        default: {  // X_PE
            const float* pm = a.Pm + b * pblk;
            const float* pd = a.Pd + b * pblk;
            extract_cols<2>(eb, nb, e0, n0, (long long)b * emax * nmax, nmax, pm, pd, emax, 0,
                            a.rows[S_PE], a.entries[S_PE], 4);
        }
    }
}

// ---- LDS-staged extraction: one 512-thread block per (graph, family) loads the graph's dense
// blocks into LDS in rounds of unconditional loads (16 per thread in flight), then builds the
// row lists of both orientations and checks the padding from LDS.  Families: 0 = WL (line graph
// only), 1 = W + Pm/Pd.  Same lists, entry for entry, as k_extract (ascending columns per row).
// 512 threads: the 1 024 blocks of config 2 resident in one round (4 per CU); 38.3 us per launch against 42.9
// (1 024 threads, two rounds) and 55.0 (256), step 1.237-1.255 vs 1.250-1.262 ms in three alternating pairs
constexpr int XL_THREADS = 512;

__device__ __forceinline__ void lds_fill(float* __restrict__ dst, const float* __restrict__ src, int n) {
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0 && (n & 3) == 0) {
        // 16-B loads (the line-graph block of config 2: 3 675 float4, one round of 8 per thread)
        constexpr int U = 8;
        const int n4 = n >> 2;
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int base = 0; base < n4; base += XL_THREADS * U) {
            float4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = s4[min(base + u * XL_THREADS + (int)threadIdx.x, n4 - 1)];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = base + u * XL_THREADS + threadIdx.x;
                if (i < n4) d4[i] = v[u];
            }
        }
        return;
    }
    constexpr int U = 16;
    for (int base = 0; base < n; base += XL_THREADS * U) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = src[min(base + u * XL_THREADS + (int)threadIdx.x, n - 1)];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = base + u * XL_THREADS + threadIdx.x;
            if (i < n) dst[i] = v[u];
        }
    }
}

// Rows of an LDS block: element (r, c, j) at S0[r * rs + c * cs + j * js] (NC == 2: S0 / S1 hold the
// two coefficients).  Wave per output row, lanes over 64-column chunks, ballot compaction.
template <int NC>
__device__ void lds_rows(const float* S0, const float* S1, int rows, int cols, int rs, int cs, int js,
                         int row_packed0, int col_packed0, long long slot0, int cap, RowInfo* __restrict__ out_rows,
                         float* __restrict__ entries, int stride) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = XL_THREADS / 64;
    for (int r = wv; r < rows; r += nw) {
        const long long slot = slot0 + (long long)r * cap;
        int cnt = 0;
        for (int c0 = 0; c0 < cols; c0 += 64) {
            const int c = c0 + lane;
            float v[NC];
            bool nz = false;
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                v[j] = 0.f;
                if (c < cols) v[j] = NC == 2 ? (j == 0 ? S0 : S1)[r * rs + c * cs] : S0[r * rs + c * cs + j * js];
                nz |= v[j] != 0.f;
            }
            const unsigned long long mask = __ballot(nz);
            if (nz) {
                float* e = entries + (slot + cnt + __popcll(mask & ((1ull << lane) - 1ull))) * stride;
                e[0] = __int_as_float(col_packed0 + c);
#pragma unroll
                for (int j = 0; j < NC; ++j) e[1 + j] = v[j];
            }
            cnt += __popcll(mask);
        }
        if (lane == 0) out_rows[row_packed0 + r] = RowInfo{(int)slot, cnt};
    }
}

// Any nonzero of an LDS (R, C, NC) block outside [0, rr) x [0, rc) (NC = 1 per array for Pm / Pd): a wave per
// row, lanes along the row -- rows past rr whole, live rows from column rc on.  (A flat sweep with the row and
// column recovered by two integer divisions per element cost ~2 000 VALU per thread on the line-graph block.)
__device__ void lds_validate(const float* S, int R, int C, int NC, int rr, int rc, uint32_t* err) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = XL_THREADS / 64;
    const int row = C * NC, live = rc * NC;
    bool bad = false;
    for (int r = wv; r < R; r += nw)
        for (int k = (r < rr ? live : 0) + lane; k < row; k += 64) bad |= S[r * row + k] != 0.f;
    if (__any(bad) && lane == 0) atomicOr(err, (uint32_t)ERR_PAD_NONZERO);
}

// validate_mask's loads issued ahead of the LDS fill (n <= XL_THREADS: one per thread), checked after it
struct MaskProbe {
    float v = 0.f;
    bool on = false;
    __device__ void issue(const float* __restrict__ mask, int n, bool validate) {
        on = validate && n <= XL_THREADS;
        if (on && (int)threadIdx.x < n) v = mask[(long long)threadIdx.x * n];
    }
    __device__ void check(const float* __restrict__ mask, int n, int real, bool validate, uint32_t* err) const {
        if (!validate) return;
        if (!on) {
            validate_mask(mask, n, real, err);
            return;
        }
        const int i = threadIdx.x;
        const bool bad = i < n && v != ((i < real && real > 0) ? 1.f : 0.f);
        if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(err, (uint32_t)ERR_MASK);
    }
};

template <int JT>
__global__ void __launch_bounds__(XL_THREADS) k_extract_lds(ExtractArgs a) {
    WaveStamp stamp(a.stamps);
    extern __shared__ __attribute__((aligned(16))) float S[];
    const int b = blockIdx.x;
    const int fam = a.dual ? (int)blockIdx.y : 1;
    const int n0 = a.meta.node_off[b], nb = a.meta.node_off[b + 1] - n0;
    const int nmax = a.nmax, emax = a.emax;
    if (fam == 0) {
        const int e0 = a.meta.edge_off[b], eb = a.meta.edge_off[b + 1] - e0;
        const int n = emax * emax * JT;
        const float* mk = a.mask_lg + (long long)b * emax * emax;
        MaskProbe mp;
        mp.issue(mk, emax, a.validate);
        lds_fill(S, a.WL + (long long)b * n, n);
        __syncthreads();
        const long long slot0 = (long long)b * emax * emax;
        // WL rows e (cols e'), and the transpose: rows e' (cols e) read down the LDS columns
        lds_rows<JT>(S, nullptr, eb, eb, emax * JT, JT, 1, e0, e0, slot0, emax, a.rows[S_WL], a.entries[S_WL],
                     a.entry_stride_w);
        lds_rows<JT>(S, nullptr, eb, eb, JT, emax * JT, 1, e0, e0, slot0, emax, a.rows[S_WLT], a.entries[S_WLT],
                     a.entry_stride_w);
        if (a.validate) {
            lds_validate(S, emax, emax, JT, eb, eb, a.meta.err);
            mp.check(mk, emax, eb, true, a.meta.err);
        }
        if (a.xlo)  // the packed edge input (k_pack_edges' work)
            for (int i = threadIdx.x; i < eb; i += XL_THREADS) a.xlo[e0 + i] = a.XL[(long long)b * emax + i];
        return;
    }
    if (a.xo)  // the packed node input (k_pack_nodes' work): [nodes][f] from (bs, f, nmax)
        for (int i = threadIdx.x; i < nb * a.f; i += XL_THREADS) {
            const int n = i / a.f, c = i - n * a.f;
            a.xo[(long long)(n0 + n) * a.f + c] = a.X[((long long)b * a.f + c) * nmax + n];
        }
    const int nw_ = nmax * nmax * JT, np = nmax * emax;
    float* SW = S;
    float* SM = S + nw_;
    float* SD = SM + np;
    const float* mk = a.mask + (long long)b * nmax * nmax;
    MaskProbe mp;
    mp.issue(mk, nmax, a.validate);
    lds_fill(SW, a.W + (long long)b * nw_, nw_);
    if (a.dual) {
        lds_fill(SM, a.Pm + (long long)b * np, np);
        lds_fill(SD, a.Pd + (long long)b * np, np);
    }
    __syncthreads();
    const long long slotw = (long long)b * nmax * nmax;
    lds_rows<JT>(SW, nullptr, nb, nb, nmax * JT, JT, 1, n0, n0, slotw, nmax, a.rows[S_W], a.entries[S_W],
                 a.entry_stride_w);
    lds_rows<JT>(SW, nullptr, nb, nb, JT, nmax * JT, 1, n0, n0, slotw, nmax, a.rows[S_WT], a.entries[S_WT],
                 a.entry_stride_w);
    if (a.validate) {
        lds_validate(SW, nmax, nmax, JT, nb, nb, a.meta.err);
        mp.check(mk, nmax, nb, true, a.meta.err);
    }
    if (!a.dual) return;
    const int e0 = a.meta.edge_off[b], eb = a.meta.edge_off[b + 1] - e0;
    // Pm/Pd (n, e): node rows over edge cols, and edge rows over node cols
    lds_rows<2>(SM, SD, nb, eb, emax, 1, 0, n0, e0, (long long)b * nmax * emax, emax, a.rows[S_PN], a.entries[S_PN], 4);
    lds_rows<2>(SM, SD, eb, nb, 1, emax, 0, e0, n0, (long long)b * emax * nmax, nmax, a.rows[S_PE], a.entries[S_PE], 4);
    if (a.validate) {
        lds_validate(SM, nmax, emax, 1, nb, eb, a.meta.err);
        lds_validate(SD, nmax, emax, 1, nb, eb, a.meta.err);
    }
}

// ---- Register-staged extraction: one 512-thread block per graph takes all of the graph's dense operator blocks
// (WL, W, Pm / Pd) into registers -- a wave per dense row, lanes along the row, every load of the block in flight
// at once -- marks the live nonzeros in two LDS bitmaps (row-major and transposed), then writes every nonzero
// entry straight to its place in both lists: the position is the count of set bits before it in its row (its
// column) of the bitmap.  The lists are k_extract's, entry for entry (ascending columns per row, ascending rows
// in a transposed row).  Padding is checked on the registers.  Against k_extract_lds: no 58.8-KB LDS copy of
// the line-graph block, so the 512 blocks of config 2 are resident in one round (two per CU) -- the LDS kernel
// ran its W / Pm / Pd blocks in a second round behind the line-graph blocks (per-wave stamps,
// tools/wave_stats.py) -- and no flat LDS sweep for the padding check.  Shapes: a line-graph block of at most
// 8 XR_MR_L rows of 256 floats, node blocks of at most 8 XR_MR_N rows of 128 floats (config 2: 70 x 210 and
// 29 x 87 / 29 x 70); larger shapes take k_extract_lds / k_extract.
constexpr int XR_THREADS = 512, XR_WAVES = XR_THREADS / 64, XR_MR_L = 9, XR_MCH_L = 4, XR_MR_N = 4, XR_MCH_N = 2;
constexpr int XR_BITS = 2048;  // LDS words per block: bitmaps and their prefix counts

struct XrList {  // one orientation's output: rows[row_packed0 + r] = {slot0 + r cap, count}, entries at slot
    RowInfo* rows;
    float* ent;
    long long slot0;
    int cap, row_packed0, col_packed0;
};

// A dense block of R x C elements, NC coefficients each: interleaved in s0 (W / WL: (r, c, j) at
// s0[(r C + c) NC + j]) or, TWO, one in s0 and one in s1 (Pm / Pd: (r, c) at r C + c).  Live: [0, rr) x [0, rc).
// LDS: the row-major bitmap [R][WR], the transposed one [C][WT], then their word prefix counts (same shapes).
template <int NC, bool TWO, int MR, int MCH>
struct XrBlock {
    float v[MR][MCH];
    float w[TWO ? MR : 1][TWO ? MCH : 1];
    int R, C, rr, rc, L, WR, WT;
    uint32_t* bits;
    uint32_t* bitsT;
    uint32_t* pre;   // [R][WR]: set bits of the row's words before this one
    uint32_t* preT;  // [C][WT]

    __device__ int words() const { return 2 * (R * WR + C * WT); }
    __device__ void init(int R_, int C_, int rr_, int rc_, uint32_t* b) {
        R = R_;
        C = C_;
        rr = rr_;
        rc = rc_;
        L = TWO ? C : C * NC;
        WR = (C + 31) >> 5;
        WT = (R + 31) >> 5;
        bits = b;
        bitsT = bits + R * WR;
        pre = bitsT + C * WT;
        preT = pre + R * WR;
    }
    // every load unconditional (clamped to a live address) and in flight before the first use
    __device__ void load(const float* __restrict__ s0, const float* __restrict__ s1) {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
        for (int i = 0; i < MR; ++i) {
            const int rb = min(wv + XR_WAVES * i, R - 1) * L;
#pragma unroll
            for (int h = 0; h < MCH; ++h) {
                const int o = rb + min(h * 64 + lane, L - 1);
                v[i][h] = s0[o];
                if constexpr (TWO) w[i][h] = s1[o];
            }
        }
    }
    __device__ bool nz(int i, int h) const {
        if constexpr (TWO) return v[i][h] != 0.f || w[i][h] != 0.f;
        return v[i][h] != 0.f;
    }
    // set the live nonzeros' bits; any nonzero outside the live region -> bad
    __device__ void mark(bool& bad) const {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
        for (int i = 0; i < MR; ++i) {
            const int r = wv + XR_WAVES * i;
            if (r >= R) break;
#pragma unroll
            for (int h = 0; h < MCH; ++h) {
                const int k = h * 64 + lane, c = TWO ? k : k / NC;
                if (k < L && nz(i, h)) {
                    if (r < rr && c < rc) {
                        atomicOr(&bits[r * WR + (c >> 5)], 1u << (c & 31));
                        atomicOr(&bitsT[c * WT + (r >> 5)], 1u << (r & 31));
                    } else {
                        bad = true;
                    }
                }
            }
        }
    }
    // after the marks' barrier: the word prefix counts (a barrier follows before scatter)
    __device__ void prefix() const {
        for (int x = threadIdx.x; x < R * WR + C * WT; x += XR_THREADS) {
            const bool t = x >= R * WR;
            const int y = t ? x - R * WR : x, W = t ? WT : WR, q = y % W;
            const uint32_t* bw = (t ? bitsT : bits) + (y - q);
            uint32_t n = 0;
            for (int z = 0; z < q; ++z) n += __popc(bw[z]);
            (t ? preT : pre)[y] = n;
        }
    }
    __device__ void scatter(const XrList& o, const XrList& t, int stride) const {
        const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
        if (tid < rr) {
            const int q = (tid + 1) * WR - 1;
            o.rows[o.row_packed0 + tid] = RowInfo{(int)(o.slot0 + (long long)tid * o.cap), (int)(pre[q] + __popc(bits[q]))};
        }
        if (tid < rc) {
            const int q = (tid + 1) * WT - 1;
            t.rows[t.row_packed0 + tid] = RowInfo{(int)(t.slot0 + (long long)tid * t.cap), (int)(preT[q] + __popc(bitsT[q]))};
        }
        // per row: its elements' bitmap and prefix reads first (clamped, unconditional), then the positions and
        // the stores (32-bit entry indices within the graph's lists: checked on the host)
        float* const oe = o.ent + o.slot0 * stride;
        float* const te = t.ent + t.slot0 * stride;
#pragma unroll
        for (int i = 0; i < MR; ++i) {
            const int r = wv + XR_WAVES * i;
            if (r >= rr) break;
            uint32_t bw[MCH], bp[MCH], tw[MCH], tp[MCH];
#pragma unroll
            for (int h = 0; h < MCH; ++h) {
                const int k = min(h * 64 + lane, L - 1), c = min(TWO ? k : k / NC, C - 1);
                const int x = r * WR + (c >> 5), y = c * WT + (r >> 5);
                bw[h] = bits[x];
                bp[h] = pre[x];
                tw[h] = bitsT[y];
                tp[h] = preT[y];
            }
#pragma unroll
            for (int h = 0; h < MCH; ++h) {
                const int k = h * 64 + lane, c = TWO ? k : k / NC, j = TWO ? 0 : k - c * NC;
                const uint32_t bit = 1u << (c & 31), rbit = 1u << (r & 31);
                if (k < L && c < rc && (bw[h] & bit)) {
                    const int pos = (int)(bp[h] + __popc(bw[h] & (bit - 1u)));
                    const int tpos = (int)(tp[h] + __popc(tw[h] & (rbit - 1u)));
                    float* e = oe + (r * o.cap + pos) * stride;
                    float* et = te + (c * t.cap + tpos) * stride;
                    if constexpr (TWO) {
                        e[0] = __int_as_float(o.col_packed0 + c);
                        e[1] = v[i][h];
                        e[2] = w[i][h];
                        et[0] = __int_as_float(t.col_packed0 + r);
                        et[1] = v[i][h];
                        et[2] = w[i][h];
                    } else {
                        if (j == 0) {
                            e[0] = __int_as_float(o.col_packed0 + c);
                            et[0] = __int_as_float(t.col_packed0 + r);
                        }
                        e[1 + j] = v[i][h];
                        et[1 + j] = v[i][h];
                    }
                }
            }
        }
    }
};

// (at most 128 VGPRs: two blocks per CU, so config 2's 512 blocks are resident in one round)
template <int JT>
__global__ void __launch_bounds__(XR_THREADS) __attribute__((amdgpu_waves_per_eu(4))) k_extract_reg(ExtractArgs a) {
    WaveStamp stamp(a.stamps);
    __shared__ uint32_t xb[XR_BITS];
    const int b = blockIdx.x;
    const int nmax = a.nmax, emax = a.emax;
    const int n0 = a.meta.node_off[b], nb = a.meta.node_off[b + 1] - n0;
    const int e0 = a.dual ? a.meta.edge_off[b] : 0, eb = a.dual ? a.meta.edge_off[b + 1] - e0 : 0;
    const long long wblk = (long long)nmax * nmax * JT, lblk = (long long)emax * emax * JT,
                    pblk = (long long)nmax * emax;
    XrBlock<JT, false, XR_MR_L, XR_MCH_L> gl;
    XrBlock<JT, false, XR_MR_N, XR_MCH_N> gw;
    XrBlock<2, true, XR_MR_N, XR_MCH_N> gp;
    gw.init(nmax, nmax, nb, nb, xb);
    int used = gw.words();
    if (a.dual) {
        gl.init(emax, emax, eb, eb, xb + used);
        used += gl.words();
        gp.init(nmax, emax, nb, eb, xb + used);
        used += gp.words();
    }
    for (int i = threadIdx.x; i < used; i += XR_THREADS) xb[i] = 0u;
    __syncthreads();
    const float* mkn = a.mask + (long long)b * nmax * nmax;
    const float* mke = a.dual ? a.mask_lg + (long long)b * emax * emax : nullptr;
    MaskProbe mpn, mpe;
    mpn.issue(mkn, nmax, a.validate);
    if (a.dual) {
        mpe.issue(mke, emax, a.validate);
        gl.load(a.WL + b * lblk, nullptr);
        gp.load(a.Pm + b * pblk, a.Pd + b * pblk);
    }
    gw.load(a.W + b * wblk, nullptr);
    // the packed inputs (k_pack_nodes / k_pack_edges' work) while the loads are in flight
    if (a.xo)
        for (int i = threadIdx.x; i < nb * a.f; i += XR_THREADS) {
            const int n = i / a.f, c = i - n * a.f;
            a.xo[(long long)(n0 + n) * a.f + c] = a.X[((long long)b * a.f + c) * nmax + n];
        }
    if (a.dual && a.xlo)
        for (int i = threadIdx.x; i < eb; i += XR_THREADS) a.xlo[e0 + i] = a.XL[(long long)b * emax + i];
    bool bad = false;
    if (a.dbg == 1) {  // diagnostics: the loads only
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < XR_MR_L; ++i)
#pragma unroll
            for (int h = 0; h < XR_MCH_L; ++h) t += gl.v[i][h];
#pragma unroll
        for (int i = 0; i < XR_MR_N; ++i)
#pragma unroll
            for (int h = 0; h < XR_MCH_N; ++h) t += gw.v[i][h] + gp.v[i][h] + gp.w[i][h];
        if (t == 1.2345f) atomicOr(a.meta.err, 0u);
        return;
    }
    if (a.dual) {
        gl.mark(bad);
        gp.mark(bad);
    }
    gw.mark(bad);
    __syncthreads();
    if (a.dbg == 2) return;
    gw.prefix();
    if (a.dual) {
        gl.prefix();
        gp.prefix();
    }
    __syncthreads();
    const long long sw = (long long)b * nmax * nmax;
    gw.scatter(XrList{a.rows[S_W], a.entries[S_W], sw, nmax, n0, n0},
               XrList{a.rows[S_WT], a.entries[S_WT], sw, nmax, n0, n0}, a.entry_stride_w);
    if (a.dual) {
        const long long sl = (long long)b * emax * emax, sp = (long long)b * nmax * emax;
        gl.scatter(XrList{a.rows[S_WL], a.entries[S_WL], sl, emax, e0, e0},
                   XrList{a.rows[S_WLT], a.entries[S_WLT], sl, emax, e0, e0}, a.entry_stride_w);
        gp.scatter(XrList{a.rows[S_PN], a.entries[S_PN], sp, emax, n0, e0},
                   XrList{a.rows[S_PE], a.entries[S_PE], sp, nmax, e0, n0}, 4);
    }
    if (a.validate) {
        if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(a.meta.err, (uint32_t)ERR_PAD_NONZERO);
        mpn.check(mkn, nmax, nb, true, a.meta.err);
        if (a.dual) mpe.check(mke, emax, eb, true, a.meta.err);
    }
}

// the register-staged extraction's shape limits (see k_extract_reg)
static bool extract_reg_fits(const ExtractArgs& a) {
    const int J = a.jtot;
    if (J < 3 || J > 4) return false;  // k_extract_reg is instantiated for J_tot 3 and 4 only
    if (a.nmax < 1 || a.nmax > XR_WAVES * XR_MR_N || a.nmax * J > 64 * XR_MCH_N) return false;
    long long words = a.nmax * ((a.nmax + 31) / 32) * 2;
    if (a.dual) {
        if (a.emax < 1 || a.emax > XR_WAVES * XR_MR_L || a.emax * J > 64 * XR_MCH_L || a.emax > 64 * XR_MCH_N)
            return false;
        words += 2 * a.emax * ((a.emax + 31) / 32) + a.nmax * ((a.emax + 31) / 32) + a.emax * ((a.nmax + 31) / 32);
    }
    // (bitmaps and prefix counts; entry indices within one graph's lists in 32 bits)
    const long long blk = (long long)std::max(a.nmax, a.emax) * std::max(a.nmax, a.emax) * std::max(a.entry_stride_w, 4);
    return 2 * words <= XR_BITS && a.entry_stride_w >= 1 + J && blk < (1ll << 31);
}

// LDS bytes of the staged extraction (0: does not fit, use k_extract)
static size_t extract_lds_bytes(const ExtractArgs& a) {
    const size_t wl = a.dual ? (size_t)a.emax * a.emax * a.jtot : 0;
    const size_t wp = (size_t)a.nmax * a.nmax * a.jtot + (a.dual ? 2 * (size_t)a.nmax * a.emax : 0);
    const size_t b = 4 * (wl > wp ? wl : wp);
    return b <= 96 * 1024 ? b : 0;
}

template <int JT>
static void extract_lds_launch(const ExtractArgs& a, size_t lds, hipStream_t s) {
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_extract_lds<JT>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
        attr = true;
    }
    ExtractArgs as = a;
    as.stamps = clock_stamps((long long)a.bs * (a.dual ? 2 : 1) * (XL_THREADS / 64));
    HGNN_KLAUNCH(k_extract_lds<JT>, dim3(a.bs, a.dual ? 2 : 1), dim3(XL_THREADS), lds, s, as);
}

static int extract_one(const ExtractArgs& a, dim3 grid, hipStream_t s) {
    switch (a.jtot) {
        case 3: HGNN_KLAUNCH(k_extract<3>, grid, dim3(X_THREADS), 0, s, a); break;
        case 4: HGNN_KLAUNCH(k_extract<4>, grid, dim3(X_THREADS), 0, s, a); break;
        case 5: HGNN_KLAUNCH(k_extract<5>, grid, dim3(X_THREADS), 0, s, a); break;
        case 6: HGNN_KLAUNCH(k_extract<6>, grid, dim3(X_THREADS), 0, s, a); break;
        case 7: HGNN_KLAUNCH(k_extract<7>, grid, dim3(X_THREADS), 0, s, a); break;
        default: return 2;
    }
    HGNN_LAUNCH_CHECK();
    return 0;
}

int extract_variant(const ExtractArgs& a) {
    const Switches& sw = switches();
    // HGNN_EXTRACT_LDS=0: the general kernel
    if (!sw.extract_lds || a.kind0 != 0) return 0;
    // HGNN_EXTRACT_REG=0: the LDS-staged kernel for the shapes the register-staged one takes
    if (sw.extract_reg && extract_reg_fits(a)) return 2;
    return extract_lds_bytes(a) > 0 ? 1 : 0;
}

int launch_extract(const ExtractArgs& a, hipStream_t s) {
    const Switches& sw = switches();
    const int variant = extract_variant(a);
    if (variant == 2) {
        ExtractArgs as = a;
        const int dbg = sw.xr_dbg;
        // (diagnostics, HGNN_XR_DBG: a truncated launch ahead of the real one, which then runs as always)
        for (int pass = dbg > 0 ? 0 : 1; pass < 2; ++pass) {
            as.dbg = pass == 0 ? dbg : 0;
            as.stamps = clock_stamps((long long)a.bs * XR_WAVES);
            switch (a.jtot) {
                case 3: HGNN_KLAUNCH(k_extract_reg<3>, dim3(a.bs), dim3(XR_THREADS), 0, s, as); break;
                case 4: HGNN_KLAUNCH(k_extract_reg<4>, dim3(a.bs), dim3(XR_THREADS), 0, s, as); break;
                default: return 2;  // (extract_reg_fits admits J_tot 3 and 4 only)
            }
        }
        HGNN_LAUNCH_CHECK();
        return 0;
    }
    if (variant == 1) {
        const size_t lds = extract_lds_bytes(a);
        switch (a.jtot) {
            case 3: extract_lds_launch<3>(a, lds, s); break;
            case 4: extract_lds_launch<4>(a, lds, s); break;
            case 5: extract_lds_launch<5>(a, lds, s); break;
            case 6: extract_lds_launch<6>(a, lds, s); break;
            case 7: extract_lds_launch<7>(a, lds, s); break;
            default: return 2;
        }
        HGNN_LAUNCH_CHECK();
        return 0;
    }
    // the general kernel leaves the input packing to its own launches
    if (a.xo) {
        const int r = launch_pack_nodes(a.X, a.bs, a.f, a.nmax, a.meta, a.xo, s);
        if (r) return r;
    }
    if (a.xlo) {
        const int r = launch_pack_edges(a.XL, a.bs, a.emax, a.meta, a.xlo, s);
        if (r) return r;
    }
    const int kinds = a.dual ? X_SLOTS : 2;
    // HGNN_EXTRACT_SPLIT=1 (diagnostics): one launch per block slot, so a kernel trace times
    // each slot
    if (!sw.extract_split) return extract_one(a, dim3(a.bs, kinds), s);
    for (int k = 0; k < kinds; ++k) {
        ExtractArgs b = a;
        b.kind0 = k;
        const int r = extract_one(b, dim3(a.bs, 1), s);
        if (r) return r;
    }
    return 0;
}

__global__ void k_pack_nodes(const float* __restrict__ X, int f, int nmax, BatchMeta m,
                             float* __restrict__ out) {
    const int b = blockIdx.x;
    const int n0 = m.node_off[b];
    const int nb = m.node_off[b + 1] - n0;
    const float* xb = X + (long long)b * f * nmax;
    for (int i = threadIdx.x; i < nb * f; i += blockDim.x) {
        const int n = i / f, c = i % f;
        out[(long long)(n0 + n) * f + c] = xb[(long long)c * nmax + n];
    }
}

int launch_pack_nodes(const float* X, int bs, int f, int nmax, BatchMeta m, float* out,
                      hipStream_t s) {
    HGNN_KLAUNCH(k_pack_nodes, dim3(bs), dim3(128), 0, s, X, f, nmax, m, out);
    HGNN_LAUNCH_CHECK();
    return 0;
}

__global__ void k_pack_edges(const float* __restrict__ XL, int emax, BatchMeta m,
                             float* __restrict__ out) {
    const int b = blockIdx.x;
    const int e0 = m.edge_off[b];
    const int eb = m.edge_off[b + 1] - e0;
    for (int i = threadIdx.x; i < eb; i += blockDim.x) out[e0 + i] = XL[(long long)b * emax + i];
}

int launch_pack_edges(const float* XL, int bs, int emax, BatchMeta m, float* out, hipStream_t s) {
    HGNN_KLAUNCH(k_pack_edges, dim3(bs), dim3(128), 0, s, XL, emax, m, out);
    HGNN_LAUNCH_CHECK();
    return 0;
}

__global__ void k_unpack_nodes(const float* __restrict__ in, int f, int nmax, BatchMeta m,
                               float* __restrict__ X, uint64_t* stamps) {
    WaveStamp stamp(stamps);
    const int b = blockIdx.x;
    const int n0 = m.node_off[b];
    const int nb = m.node_off[b + 1] - n0;
    float* xb = X + (long long)b * f * nmax;
    for (int i = threadIdx.x; i < nmax * f; i += blockDim.x) {
        const int c = i / nmax, n = i % nmax;
        xb[i] = n < nb ? in[(long long)(n0 + n) * f + c] : 0.f;
    }
}

int launch_unpack_nodes(const float* in, int bs, int f, int nmax, BatchMeta m, float* X,
                        hipStream_t s) {
    HGNN_KLAUNCH(k_unpack_nodes, dim3(bs), dim3(128), 0, s, in, f, nmax, m, X, clock_stamps((long long)bs * 2));
    HGNN_LAUNCH_CHECK();
    return 0;
}

}  // namespace hgnn
