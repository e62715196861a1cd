// Sparse operator x feature aggregation (the graph_oper / P_multi hot loops).
//
// Forward (models/layers/layers_mnb.py:391-434): for one packed output row r
//   out[r, j*Cg + c]          = sum_{e in G(r)} v_j(e) * Xg[col(e), c]   j < J+2
//   out[r, J*Cg + c]          = sum_{e in P(r)} Pm(e)  * Xp[col(e), c]
//   out[r, J*Cg + Cp + c]     = sum_{e in P(r)} Pd(e)  * Xp[col(e), c]
// i.e. the reference's cat(graph_oper(W, X), P_multi(Pm, Y), P_multi(Pd, Y)) of
// one layer, built row by row.  One wave per row; the row's entry list is
// wave-uniform (scalar loads); each gathered feature row is one coalesced
// vector load of 64 lanes x CPL channels and feeds all J+2 (or both P)
// coefficients.  Variable degree = a loop of wave-uniform trip count, so the
// segmented reduction needs no cross-lane traffic at all.
//
// Backward: the transposed lists (S_WT, S_PE/S_PN) gather the upstream
// gradient blocks:  out[r, c] (+)= sum_e sum_j v_j * dA[col, j*C + c]
//                                + sum_e Pm * dA[col, m_off + c] + Pd * dA[col, d_off + c].
#include "kernels.h"

#include <initializer_list>

namespace hgnn {

// Row loads / stores of one wave (lane owns channels lane*CPL ..).  V = the host checked that
// C == 64*CPL and every row address is aligned for the vector width (the executor's layouts
// always are), so the vector form is straight-line code; otherwise a guarded scalar form.
template <int CPL, bool V>
__device__ __forceinline__ void load_row(const float* __restrict__ p, int C, int lane, float (&x)[CPL]) {
    const int c0 = lane * CPL;
    if constexpr (V) {
        if constexpr (CPL == 1) {
            x[0] = p[c0];
        } else if constexpr (CPL == 2) {
            const float2 v = *reinterpret_cast<const float2*>(p + c0);
            x[0] = v.x;
            x[1] = v.y;
        } else {
#pragma unroll
            for (int i = 0; i < CPL; i += 4) {
                const float4 v = *reinterpret_cast<const float4*>(p + c0 + i);
                x[i] = v.x;
                x[i + 1] = v.y;
                x[i + 2] = v.z;
                x[i + 3] = v.w;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < CPL; ++i) x[i] = (c0 + i < C) ? p[c0 + i] : 0.f;
    }
}

template <int CPL, bool V>
__device__ __forceinline__ void store_row(float* __restrict__ p, int C, int lane, const float (&x)[CPL]) {
    const int c0 = lane * CPL;
    if constexpr (V) {
        if constexpr (CPL == 1) {
            p[c0] = x[0];
        } else if constexpr (CPL == 2) {
            *reinterpret_cast<float2*>(p + c0) = make_float2(x[0], x[1]);
        } else {
#pragma unroll
            for (int i = 0; i < CPL; i += 4)
                *reinterpret_cast<float4*>(p + c0 + i) = make_float4(x[i], x[i + 1], x[i + 2], x[i + 3]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < CPL; ++i)
            if (c0 + i < C) p[c0 + i] = x[i];
    }
}

// Host side of V: channel count fills the lanes exactly, base pointers and every offset /
// leading dimension keep the vector alignment.
static bool vec_ok(int cpl, int c, const void* base, std::initializer_list<long long> offs) {
    if (c != 64 * cpl) return false;
    const int w = cpl >= 4 ? 4 : cpl;  // floats per vector access
    if (reinterpret_cast<uintptr_t>(base) % (4 * w)) return false;
    for (long long o : offs)
        if (o % w) return false;
    return true;
}

// Entry lists are fetched lane-parallel (lane e holds entry e of a 64-entry chunk)
// and broadcast with readlane, and U feature rows are loaded before any is used,
// so a row of n entries costs ~n/U dependent memory round trips instead of 2n.
#ifndef AGG_UNROLL
#define AGG_UNROLL 4
#endif
constexpr int AGG_U = AGG_UNROLL;
// rows (waves) per block of the aggregation kernels; AGG_BLOCK_WAVES at build time (A/B)
#ifndef AGG_BLOCK_WAVES
#define AGG_BLOCK_WAVES 4
#endif
constexpr int AGG_WV = AGG_BLOCK_WAVES, AGG_NT = 64 * AGG_WV;

__device__ __forceinline__ float4 lane_entry(const float* __restrict__ entries, int stride, int start, int n, int lane) {
    // W / WL entries: (col, v_0..v_{J-1}) padded to `stride` floats; P entries: (col, pm, pd, -)
    if (lane < n) return *reinterpret_cast<const float4*>(entries + (long long)(start + lane) * stride);
    return make_float4(__int_as_float(0), 0.f, 0.f, 0.f);
}

// Row info through the constant address space: a wave-uniform index then becomes one scalar
// load (lgkmcnt, not the vector counter the gathers wait on) and the row's counts live in SGPRs.
// The lists are written by an earlier launch and only read here.
__device__ __forceinline__ RowInfo row_info(const RowInfo* rows, int r) {
    typedef const __attribute__((address_space(4))) int* ConstInts;
    const ConstInts q = (ConstInts)(reinterpret_cast<const int*>(rows) + 2 * (long long)r);
    RowInfo v;
    v.start = q[0];
    v.count = q[1];
    return v;
}

__device__ __forceinline__ float bcast(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// Per-lane BN constants of the CPL channels a lane owns (lane * CPL + i).
template <int CPL>
struct LaneBn {
    float mu[CPL], sc[CPL], w, b;  // sc = w / std per channel
    bool on;
    __device__ __forceinline__ void init(const BnView& v, int C, int lane) {
        on = v.mean != nullptr;
        w = b = 0.f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) mu[i] = 0.f, sc[i] = 1.f;
        if (!on) return;
        w = *v.w;
        b = *v.b;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = lane * CPL + i;
            if (c < C) mu[i] = v.mean[c], sc[i] = bn_scale(w, v.std[c]);
        }
    }
    __device__ __forceinline__ void apply(float (&x)[CPL]) const {
        if (!on) return;
#pragma unroll
        for (int i = 0; i < CPL; ++i) x[i] = bn_z_s(x[i], mu[i], sc[i], b);
    }
};

// Diagonal I / D mode (AggFwdArgs::j0 = 2): the row's entries of one 64-entry chunk (lane e: entry e, m = (col,
// v_0, v_1, ..)) -- the diagonal entry's (v_0, v_1) go to diag[r]; an off-diagonal entry with v_0 or v_1 nonzero
// is an operator the GEMMs' diagonal form cannot take (ERR_DIAG_ID).  found: a diagonal entry was met (uniform).
__device__ __forceinline__ void diag_scan(const AggFwdArgs& a, int r, float4 m, int n, int lane, bool& found) {
    const bool live = lane < n;
    const int col = __float_as_int(m.x);
    const bool on = live && col == r;
    if (on) a.diag[r] = make_float2(m.y, m.z);
    if (__ballot(on)) found = true;
    const bool bad = live && col != r && (m.y != 0.f || m.z != 0.f);
    if (__ballot(bad) && lane == 0) atomicOr(a.err, ERR_DIAG_ID);
}

template <int JT, int CG, int CP, bool V, int J0>
__global__ void __launch_bounds__(AGG_NT) k_agg_fwd(AggFwdArgs a) {
    WaveStamp stamp(a.stamps);
    const int r = __builtin_amdgcn_readfirstlane(blockIdx.x * AGG_WV + (threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    if (r >= *a.total_rows) return;
    float* o = a.out + (long long)r * a.ldo;
    constexpr int CGx = CG > 0 ? CG : 1, CPx = CP > 0 ? CP : 1;
    float acc[JT][CGx], am[CPx], ad[CPx];
#pragma unroll
    for (int j = 0; j < JT; ++j)
#pragma unroll
        for (int i = 0; i < CGx; ++i) acc[j][i] = 0.f;
#pragma unroll
    for (int i = 0; i < CPx; ++i) am[i] = ad[i] = 0.f;
    // The G and P chains (row info -> entry chunk -> feature gathers) run interleaved: both
    // row infos, then both entry chunks, then the gathers of both lists in one batch, so a
    // row costs ~3 dependent memory round trips instead of 6.
    RowInfo rg{0, 0}, rp{0, 0};
    if constexpr (CG > 0) rg = row_info(a.g.rows, r);
    if constexpr (CP > 0) rp = row_info(a.p.rows, r);
    LaneBn<CGx> bng;
    LaneBn<CPx> bnp;
    if constexpr (CG > 0) bng.init(a.gbn, a.cg, lane);
    if constexpr (CP > 0) bnp.init(a.pbn, a.cp, lane);
    const int stride = a.g.stride;
    const int nmax = max(rg.count, rp.count);
    bool dfound = false;
    for (int e0 = 0; e0 < nmax; e0 += 64) {
        const int ng = min(64, max(0, rg.count - e0)), np = min(64, max(0, rp.count - e0));
        float4 mg = make_float4(0.f, 0.f, 0.f, 0.f), mp = mg;
        float mx[JT > 3 ? JT - 3 : 1];
        if constexpr (CG > 0) {
            // JT <= 3: one float4 per entry; larger JT reads the extra coefficients below
            mg = lane_entry(a.g.entries, stride, rg.start + e0, ng, lane);
            if constexpr (JT > 3) {
#pragma unroll
                for (int j = 3; j < JT; ++j)
                    mx[j - 3] = lane < ng ? a.g.entries[(long long)(rg.start + e0 + lane) * stride + 1 + j] : 0.f;
            }
            if constexpr (J0 > 0)
                if (a.diag) diag_scan(a, r, mg, ng, lane, dfound);
        }
        if constexpr (CP > 0) mp = lane_entry(a.p.entries, 4, rp.start + e0, np, lane);
        const int nn = max(ng, np);
        for (int e = 0; e < nn; e += AGG_U) {
            float xg[AGG_U][CGx], v[AGG_U][JT], xp[AGG_U][CPx], vm[AGG_U], vd[AGG_U];
            if constexpr (CG > 0) {
#pragma unroll
                for (int u = 0; u < AGG_U; ++u) {
                    // dead slots re-read the last live row with zero coefficients (no branch)
                    const int eu = max(0, min(e + u, ng - 1));
                    const int col = __builtin_amdgcn_readlane(__float_as_int(mg.x), eu);
                    const bool live = e + u < ng;
                    v[u][0] = live ? bcast(mg.y, eu) : 0.f;
                    if constexpr (JT > 1) v[u][1] = live ? bcast(mg.z, eu) : 0.f;
                    if constexpr (JT > 2) v[u][2] = live ? bcast(mg.w, eu) : 0.f;
#pragma unroll
                    for (int j = 3; j < JT; ++j) v[u][j] = live ? bcast(mx[j - 3], eu) : 0.f;
                    if (ng > 0) load_row<CG, V>(a.xg + (long long)col * a.cg, a.cg, lane, xg[u]);
                    else
#pragma unroll
                        for (int i = 0; i < CG; ++i) xg[u][i] = 0.f;
                }
            }
            if constexpr (CP > 0) {
#pragma unroll
                for (int u = 0; u < AGG_U; ++u) {
                    const int eu = max(0, min(e + u, np - 1));
                    const int col = __builtin_amdgcn_readlane(__float_as_int(mp.x), eu);
                    const bool live = e + u < np;
                    vm[u] = live ? bcast(mp.y, eu) : 0.f;
                    vd[u] = live ? bcast(mp.z, eu) : 0.f;
                    if (np > 0) load_row<CP, V>(a.xp + (long long)col * a.cp, a.cp, lane, xp[u]);
                    else
#pragma unroll
                        for (int i = 0; i < CP; ++i) xp[u][i] = 0.f;
                }
            }
            if constexpr (CG > 0) {
#pragma unroll
                for (int u = 0; u < AGG_U; ++u) bng.apply(xg[u]);
#pragma unroll
                for (int u = 0; u < AGG_U; ++u)
#pragma unroll
                    for (int j = J0; j < JT; ++j)
#pragma unroll
                        for (int i = 0; i < CG; ++i) acc[j][i] = fmaf(v[u][j], xg[u][i], acc[j][i]);
            }
            if constexpr (CP > 0) {
#pragma unroll
                for (int u = 0; u < AGG_U; ++u) bnp.apply(xp[u]);
#pragma unroll
                for (int u = 0; u < AGG_U; ++u)
#pragma unroll
                    for (int i = 0; i < CP; ++i) {
                        am[i] = fmaf(vm[u], xp[u][i], am[i]);
                        ad[i] = fmaf(vd[u], xp[u][i], ad[i]);
                    }
            }
        }
    }
    if constexpr (CG > 0) {
#pragma unroll
        for (int j = J0; j < JT; ++j) store_row<CG, V>(o + (j - J0) * a.cg, a.cg, lane, acc[j]);
        if constexpr (J0 > 0)
            if (a.diag && !dfound && lane == 0) a.diag[r] = make_float2(0.f, 0.f);
    }
    if constexpr (CP > 0) {
        const int base = (JT - J0) * a.cg;
        store_row<CP, V>(o + base, a.cp, lane, am);
        store_row<CP, V>(o + base + a.cp, a.cp, lane, ad);
    }
    // zero the row padding [K, ldo): the GEMMs run over the padded width
    if (a.pad_from >= 0) {
        const int kk = a.pad_from > 0 ? a.pad_from : (JT - J0) * a.cg + (CP > 0 ? 2 * a.cp : 0);
        if (lane < a.ldo - kk) o[kk + lane] = 0.f;
    }
}

// k_agg_fwd with RPW rows per wave (rows RPW w .. RPW w + RPW - 1): the row infos of all of them, then the first entry
// chunk of all of them, are fetched before the first row's gathers, so RPW rows cost RPW + 2 dependent round
// trips instead of 3 RPW.
template <int JT, int CG, int CP, bool V, int RPW, int J0>
__global__ void __launch_bounds__(AGG_NT) k_agg_fwd_rpw(AggFwdArgs a) {
    WaveStamp stamp(a.stamps);
    const int r0 = __builtin_amdgcn_readfirstlane((blockIdx.x * AGG_WV + (threadIdx.x >> 6)) * RPW);
    const int lane = threadIdx.x & 63;
    const int total = *a.total_rows;
    if (r0 >= total) return;
    constexpr int CGx = CG > 0 ? CG : 1, CPx = CP > 0 ? CP : 1, MX = JT > 3 ? JT - 3 : 1;
    // The G and P chains (row info -> entry chunk -> feature gathers) run interleaved: both
    // row infos, then both entry chunks, then the gathers of both lists in one batch, so a
    // row costs ~3 dependent memory round trips instead of 6.
    RowInfo rgk[RPW], rpk[RPW];
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
        const int r = min(r0 + k, total - 1);  // (rows past the total: a live row, never stored)
        rgk[k] = RowInfo{0, 0};
        rpk[k] = RowInfo{0, 0};
        if constexpr (CG > 0) rgk[k] = row_info(a.g.rows, r);
        if constexpr (CP > 0) rpk[k] = row_info(a.p.rows, r);
    }
    LaneBn<CGx> bng;
    LaneBn<CPx> bnp;
    if constexpr (CG > 0) bng.init(a.gbn, a.cg, lane);
    if constexpr (CP > 0) bnp.init(a.pbn, a.cp, lane);
    const int stride = a.g.stride;
    // the first 64-entry chunk of every row's lists
    float4 mgk[RPW], mpk[RPW];
    float mxk[RPW][MX];
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
        mgk[k] = mpk[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        const int ng = min(64, rgk[k].count), np = min(64, rpk[k].count);
        if constexpr (CG > 0) {
            mgk[k] = lane_entry(a.g.entries, stride, rgk[k].start, ng, lane);
            if constexpr (JT > 3) {
#pragma unroll
                for (int j = 3; j < JT; ++j)
                    mxk[k][j - 3] = lane < ng ? a.g.entries[(long long)(rgk[k].start + lane) * stride + 1 + j] : 0.f;
            }
        }
        if constexpr (CP > 0) mpk[k] = lane_entry(a.p.entries, 4, rpk[k].start, np, lane);
    }
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
    const int r = r0 + k;
    if (r >= total) break;
    const RowInfo rg = rgk[k], rp = rpk[k];
    float* o = a.out + (long long)r * a.ldo;
    float acc[JT][CGx], am[CPx], ad[CPx];
#pragma unroll
    for (int j = 0; j < JT; ++j)
#pragma unroll
        for (int i = 0; i < CGx; ++i) acc[j][i] = 0.f;
#pragma unroll
    for (int i = 0; i < CPx; ++i) am[i] = ad[i] = 0.f;
    const int nmax = max(rg.count, rp.count);
    bool dfound = false;
    for (int e0 = 0; e0 < nmax; e0 += 64) {
        const int ng = min(64, max(0, rg.count - e0)), np = min(64, max(0, rp.count - e0));
        float4 mg = mgk[k], mp = mpk[k];
        float mx[MX];
#pragma unroll
        for (int j = 0; j < MX; ++j) mx[j] = mxk[k][j];
        if (e0 > 0) {
            if constexpr (CG > 0) {
                // JT <= 3: one float4 per entry; larger JT reads the extra coefficients below
                mg = lane_entry(a.g.entries, stride, rg.start + e0, ng, lane);
                if constexpr (JT > 3) {
#pragma unroll
                    for (int j = 3; j < JT; ++j)
                        mx[j - 3] = lane < ng ? a.g.entries[(long long)(rg.start + e0 + lane) * stride + 1 + j] : 0.f;
                }
            }
            if constexpr (CP > 0) mp = lane_entry(a.p.entries, 4, rp.start + e0, np, lane);
        }
        if constexpr (J0 > 0 && CG > 0)
            if (a.diag) diag_scan(a, r, mg, ng, lane, dfound);
        const int nn = max(ng, np);
        for (int e = 0; e < nn; e += AGG_U) {
            float xg[AGG_U][CGx], v[AGG_U][JT], xp[AGG_U][CPx], vm[AGG_U], vd[AGG_U];
            if constexpr (CG > 0) {
#pragma unroll
                for (int u = 0; u < AGG_U; ++u) {
                    // dead slots re-read the last live row with zero coefficients (no branch)
                    const int eu = max(0, min(e + u, ng - 1));
                    const int col = __builtin_amdgcn_readlane(__float_as_int(mg.x), eu);
                    const bool live = e + u < ng;
                    v[u][0] = live ? bcast(mg.y, eu) : 0.f;
                    if constexpr (JT > 1) v[u][1] = live ? bcast(mg.z, eu) : 0.f;
                    if constexpr (JT > 2) v[u][2] = live ? bcast(mg.w, eu) : 0.f;
#pragma unroll
                    for (int j = 3; j < JT; ++j) v[u][j] = live ? bcast(mx[j - 3], eu) : 0.f;
                    if (ng > 0) load_row<CG, V>(a.xg + (long long)col * a.cg, a.cg, lane, xg[u]);
                    else
#pragma unroll
                        for (int i = 0; i < CG; ++i) xg[u][i] = 0.f;
                }
            }
            if constexpr (CP > 0) {
#pragma unroll
                for (int u = 0; u < AGG_U; ++u) {
                    const int eu = max(0, min(e + u, np - 1));
                    const int col = __builtin_amdgcn_readlane(__float_as_int(mp.x), eu);
                    const bool live = e + u < np;
                    vm[u] = live ? bcast(mp.y, eu) : 0.f;
                    vd[u] = live ? bcast(mp.z, eu) : 0.f;
                    if (np > 0) load_row<CP, V>(a.xp + (long long)col * a.cp, a.cp, lane, xp[u]);
                    else
#pragma unroll
                        for (int i = 0; i < CP; ++i) xp[u][i] = 0.f;
                }
            }
            if constexpr (CG > 0) {
#pragma unroll
                for (int u = 0; u < AGG_U; ++u) bng.apply(xg[u]);
#pragma unroll
                for (int u = 0; u < AGG_U; ++u)
#pragma unroll
                    for (int j = J0; j < JT; ++j)
#pragma unroll
                        for (int i = 0; i < CG; ++i) acc[j][i] = fmaf(v[u][j], xg[u][i], acc[j][i]);
            }
            if constexpr (CP > 0) {
#pragma unroll
                for (int u = 0; u < AGG_U; ++u) bnp.apply(xp[u]);
#pragma unroll
                for (int u = 0; u < AGG_U; ++u)
#pragma unroll
                    for (int i = 0; i < CP; ++i) {
                        am[i] = fmaf(vm[u], xp[u][i], am[i]);
                        ad[i] = fmaf(vd[u], xp[u][i], ad[i]);
                    }
            }
        }
    }
    if constexpr (CG > 0) {
#pragma unroll
        for (int j = J0; j < JT; ++j) store_row<CG, V>(o + (j - J0) * a.cg, a.cg, lane, acc[j]);
        if constexpr (J0 > 0)
            if (a.diag && !dfound && lane == 0) a.diag[r] = make_float2(0.f, 0.f);
    }
    if constexpr (CP > 0) {
        const int base = (JT - J0) * a.cg;
        store_row<CP, V>(o + base, a.cp, lane, am);
        store_row<CP, V>(o + base + a.cp, a.cp, lane, ad);
    }
    // zero the row padding [K, ldo): the GEMMs run over the padded width
    if (a.pad_from >= 0) {
        const int kk = a.pad_from > 0 ? a.pad_from : (JT - J0) * a.cg + (CP > 0 ? 2 * a.cp : 0);
        if (lane < a.ldo - kk) o[kk + lane] = 0.f;
    }
    }
}

// ---- Narrow rows (c <= AGG_NLPR channels: layer 0 of the line-graph networks, every layer of GNN_simple).  One
// row per wave leaves 1 to 8 of the 64 lanes with work and makes a row cost a wave's three dependent round trips.
// Here a group of AGG_NLPR lanes serves one row (lane i of the group: channel i) and a wave takes 64 / AGG_NLPR
// consecutive rows: one lane-parallel load fetches all the groups' row infos, the next all their entry chunks (lane
// i of a group: entry i of the chunk), then the gathers of all groups go out together; an entry is broadcast
// within its group by __shfl.  The chunk loop's trip count is the wave's longest row; no per-lane condition
// guards a load (addresses are clamped to a live entry / row / channel and the value is selected afterwards).
// Every output element is the same fmaf chain in list order as in k_agg_fwd / agg_bwd_g / agg_bwd_p.
// AGG_NARROW=0 at build time (A/B) leaves these rows to the one-row-per-wave kernels.
#ifndef AGG_NARROW
#define AGG_NARROW 1
#endif
constexpr int AGG_NLPR = 8, AGG_NGPW = 64 / AGG_NLPR, AGG_NU = 4;

__device__ __forceinline__ RowInfo row_info_lane(const RowInfo* rows, int r) {
    const int2 v = *reinterpret_cast<const int2*>(reinterpret_cast<const int*>(rows) + 2 * (long long)r);
    return RowInfo{v.x, v.y};
}

// One list of the wave's rows, per lane: cnt the group's row count; base its first entry, or -- for an empty row --
// the first entry of a row of the wave that has one, so a clamped entry address is always a live entry; wmax the
// wave's longest row (uniform; 0: no row of the wave has an entry and nothing of the list is read).
struct NarrowList {
    int base, cnt, wmax;
    __device__ __forceinline__ void init(RowInfo ri) {
        cnt = ri.count;
        const unsigned long long m = __ballot(ri.count > 0);
        const int fs = __shfl(ri.start, m ? __ffsll(m) - 1 : 0, 64);
        base = ri.count > 0 ? ri.start : fs;
        int w = max(ri.count, 0);
#pragma unroll
        for (int o = AGG_NLPR; o < 64; o <<= 1) w = max(w, __shfl_xor(w, o, 64));
        wmax = __builtin_amdgcn_readfirstlane(w);
    }
    // the entry this lane holds of the chunk at e0 (i: lane of the group): its index, clamped to the row's last
    // entry, and whether it is one of the row's
    __device__ __forceinline__ long long at(int e0, int i, bool& live) const {
        live = e0 + i < cnt;
        return (long long)base + min(e0 + i, max(cnt - 1, 0));
    }
};

__device__ __forceinline__ float grp_bcast(float v, int src) { return __shfl(v, src, 64); }
__device__ __forceinline__ float f4_at(const float4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

// (HG / HP: the launch has a G / P part; a.cg, a.cp <= AGG_NLPR, j0 = 0)
template <int JT, bool HG, bool HP>
__global__ void __launch_bounds__(AGG_NT) k_agg_fwd_narrow(AggFwdArgs a) {
    WaveStamp stamp(a.stamps);
    const int r0 = __builtin_amdgcn_readfirstlane((blockIdx.x * AGG_WV + (threadIdx.x >> 6)) * AGG_NGPW);
    const int lane = threadIdx.x & 63, i = lane & (AGG_NLPR - 1), g0 = lane & ~(AGG_NLPR - 1);
    const int total = *a.total_rows;
    if (r0 >= total) return;
    const int r = r0 + (lane >> 3);
    const int rc = min(r, total - 1);  // (rows past the total: a live row, never stored)
    NarrowList gl{0, 0, 0}, pl{0, 0, 0};
    {
        RowInfo rg{0, 0}, rp{0, 0};
        if constexpr (HG) rg = row_info_lane(a.g.rows, rc);
        if constexpr (HP) rp = row_info_lane(a.p.rows, rc);
        if constexpr (HG) gl.init(rg);
        if constexpr (HP) pl.init(rp);
    }
    // BN constants of the lane's channel (clamped: lanes past the width hold a copy, never stored)
    const int ig = min(i, max(a.cg - 1, 0)), ip = min(i, max(a.cp - 1, 0));
    const bool gbn = HG && a.gbn.mean != nullptr, pbn = HP && a.pbn.mean != nullptr;
    float gmu = 0.f, gsc = 1.f, gb = 0.f, pmu = 0.f, psc = 1.f, pb = 0.f;
    if (gbn) gmu = a.gbn.mean[ig], gsc = bn_scale(*a.gbn.w, a.gbn.std[ig]), gb = *a.gbn.b;
    if (pbn) pmu = a.pbn.mean[ip], psc = bn_scale(*a.pbn.w, a.pbn.std[ip]), pb = *a.pbn.b;
    const int stride = a.g.stride;
    float acc[JT], am = 0.f, ad = 0.f;
#pragma unroll
    for (int j = 0; j < JT; ++j) acc[j] = 0.f;
    const int nmax = max(gl.wmax, pl.wmax);
    for (int e0 = 0; e0 < nmax; e0 += AGG_NLPR) {
        const bool gon = HG && e0 < gl.wmax, pon = HP && e0 < pl.wmax;  // uniform
        float4 mg = make_float4(0.f, 0.f, 0.f, 0.f), mp = mg, mx4 = mg;
        if (gon) {
            bool live;
            const float* q = a.g.entries + gl.at(e0, i, live) * stride;
            mg = *reinterpret_cast<const float4*>(q);
            if constexpr (JT > 3) mx4 = *reinterpret_cast<const float4*>(q + 4);
            if (!live) {
                mg.y = mg.z = mg.w = 0.f;
                mx4 = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        if (pon) {
            bool live;
            mp = *reinterpret_cast<const float4*>(a.p.entries + pl.at(e0, i, live) * 4);
            if (!live) mp.y = mp.z = 0.f;
        }
        const int nn = min(AGG_NLPR, nmax - e0);
        for (int e = 0; e < nn; e += AGG_NU) {
            float xg[AGG_NU], v[AGG_NU][JT], xp[AGG_NU], vm[AGG_NU], vd[AGG_NU];
#pragma unroll
            for (int u = 0; u < AGG_NU; ++u) {
                // a dead slot holds its row's last entry (or a live row's first) with zero coefficients
                const int src = g0 + e + u;
                xg[u] = xp[u] = 0.f;
#pragma unroll
                for (int j = 0; j < JT; ++j) v[u][j] = 0.f;
                vm[u] = vd[u] = 0.f;
                if (gon) {
                    const int col = __float_as_int(grp_bcast(mg.x, src));
                    v[u][0] = grp_bcast(mg.y, src);
                    if constexpr (JT > 1) v[u][1] = grp_bcast(mg.z, src);
                    if constexpr (JT > 2) v[u][2] = grp_bcast(mg.w, src);
#pragma unroll
                    for (int j = 3; j < JT; ++j) v[u][j] = grp_bcast(f4_at(mx4, j - 3), src);
                    xg[u] = a.xg[(long long)col * a.cg + ig];
                }
                if (pon) {
                    const int col = __float_as_int(grp_bcast(mp.x, src));
                    vm[u] = grp_bcast(mp.y, src);
                    vd[u] = grp_bcast(mp.z, src);
                    xp[u] = a.xp[(long long)col * a.cp + ip];
                }
            }
            if (gon) {
#pragma unroll
                for (int u = 0; u < AGG_NU; ++u) {
                    if (gbn) xg[u] = bn_z_s(xg[u], gmu, gsc, gb);
#pragma unroll
                    for (int j = 0; j < JT; ++j) acc[j] = fmaf(v[u][j], xg[u], acc[j]);
                }
            }
            if (pon) {
#pragma unroll
                for (int u = 0; u < AGG_NU; ++u) {
                    if (pbn) xp[u] = bn_z_s(xp[u], pmu, psc, pb);
                    am = fmaf(vm[u], xp[u], am);
                    ad = fmaf(vd[u], xp[u], ad);
                }
            }
        }
    }
    if (r >= total) return;
    float* o = a.out + (long long)r * a.ldo;
    if constexpr (HG) {
        if (i < a.cg) {
#pragma unroll
            for (int j = 0; j < JT; ++j) o[j * a.cg + i] = acc[j];
        }
    }
    if constexpr (HP) {
        const int base = JT * a.cg;
        if (i < a.cp) {
            o[base + i] = am;
            o[base + a.cp + i] = ad;
        }
    }
    // zero the row padding [K, ldo): the GEMMs run over the padded width
    if (a.pad_from >= 0) {
        const int kk = a.pad_from > 0 ? a.pad_from : JT * a.cg + (HP ? 2 * a.cp : 0);
        for (int p = kk + i; p < a.ldo; p += AGG_NLPR) o[p] = 0.f;
    }
}

template <int JT>
static int agg_fwd_narrow(const AggFwdArgs& a0, bool hg, bool hp, hipStream_t s) {
    AggFwdArgs a = a0;
    const dim3 g(ceil_div(ceil_div(a.cap_rows, AGG_NGPW), AGG_WV));
    a.stamps = clock_stamps((long long)g.x * AGG_WV);
    if (hg && hp) HGNN_KLAUNCH((k_agg_fwd_narrow<JT, true, true>), g, dim3(AGG_NT), 0, s, a);
    else if (hg) HGNN_KLAUNCH((k_agg_fwd_narrow<JT, true, false>), g, dim3(AGG_NT), 0, s, a);
    else HGNN_KLAUNCH((k_agg_fwd_narrow<JT, false, true>), g, dim3(AGG_NT), 0, s, a);
    HGNN_LAUNCH_CHECK();
    return 0;
}

static int cpl_of(int c) {
    if (c <= 0) return 0;
    if (c <= 64) return 1;
    if (c <= 128) return 2;
    if (c <= 256) return 4;
    if (c <= 512) return 8;
    return -1;
}

template <int JT, int CG, int CP, int J0>
static void agg_fwd_v(const AggFwdArgs& a0, dim3 g, hipStream_t s) {
    AggFwdArgs a = a0;
    const int kk = (JT - J0) * a.cg + (CP > 0 ? 2 * a.cp : 0);
    const bool v = (CG == 0 || vec_ok(CG, a.cg, a.xg, {})) && (CP == 0 || vec_ok(CP, a.cp, a.xp, {})) &&
                   (CG == 0 || vec_ok(CG, a.cg, a.out, {a.ldo, (long long)kk})) &&
                   (CP == 0 || vec_ok(CP, a.cp, a.out, {a.ldo, (long long)(JT - J0) * a.cg, (long long)a.cp}));
    // HGNN_AGG_RPW, rows per wave: 1 (k_agg_fwd), 2 or 4 (k_agg_fwd_rpw; J_tot = 3 only); 3 runs as 2
    const int rpw = switches().agg_rpw == 3 ? 2 : switches().agg_rpw;
    if constexpr (JT == 3) {
        if (rpw > 1) {
            const dim3 g2(ceil_div(a.cap_rows, rpw * AGG_WV));
            a.stamps = clock_stamps((long long)g2.x * AGG_WV);
            if (rpw == 4) {
                if (v) HGNN_KLAUNCH((k_agg_fwd_rpw<JT, CG, CP, true, 4, J0>), g2, dim3(AGG_NT), 0, s, a);
                else HGNN_KLAUNCH((k_agg_fwd_rpw<JT, CG, CP, false, 4, J0>), g2, dim3(AGG_NT), 0, s, a);
            } else {
                if (v) HGNN_KLAUNCH((k_agg_fwd_rpw<JT, CG, CP, true, 2, J0>), g2, dim3(AGG_NT), 0, s, a);
                else HGNN_KLAUNCH((k_agg_fwd_rpw<JT, CG, CP, false, 2, J0>), g2, dim3(AGG_NT), 0, s, a);
            }
            return;
        }
    }
    a.stamps = clock_stamps((long long)g.x * AGG_WV);
    if (v) HGNN_KLAUNCH((k_agg_fwd<JT, CG, CP, true, J0>), g, dim3(AGG_NT), 0, s, a);
    else HGNN_KLAUNCH((k_agg_fwd<JT, CG, CP, false, J0>), g, dim3(AGG_NT), 0, s, a);
}

template <int JT, int CG, int CP>
static int agg_fwd_j0(const AggFwdArgs& a, dim3 g, hipStream_t s) {
    // the diagonal I / D form is built for the layer widths the executor gives it: G and P inputs of the
    // same 2d <= 256 channels (or no P part, GNN_simple)
    if (a.j0 == 2) {
        if constexpr (CG > 0 && CG <= 4 && (CP == 0 || CP == CG)) {
            agg_fwd_v<JT, CG, CP, 2>(a, g, s);
            return 0;
        }
        return 2;
    }
    agg_fwd_v<JT, CG, CP, 0>(a, g, s);
    return 0;
}

template <int JT, int CG>
static int agg_fwd_cp(const AggFwdArgs& a, dim3 g, hipStream_t s) {
    int r = 0;
    switch (cpl_of(a.xp ? a.cp : 0)) {
        case 0: r = agg_fwd_j0<JT, CG, 0>(a, g, s); break;
        case 1: r = agg_fwd_j0<JT, CG, 1>(a, g, s); break;
        case 2: r = agg_fwd_j0<JT, CG, 2>(a, g, s); break;
        case 4: r = agg_fwd_j0<JT, CG, 4>(a, g, s); break;
        case 8: r = agg_fwd_j0<JT, CG, 8>(a, g, s); break;
        default: return 2;
    }
    if (r) return r;
    HGNN_LAUNCH_CHECK();
    return 0;
}

template <int JT>
static int agg_fwd_cg(const AggFwdArgs& a, dim3 g, hipStream_t s) {
    switch (cpl_of(a.xg ? a.cg : 0)) {
        case 0:  // P part only (its columns still start at jtot * cg)
            if (!a.xp) return 2;
            return agg_fwd_cp<JT, 0>(a, g, s);
        case 1: return agg_fwd_cp<JT, 1>(a, g, s);
        case 2: return agg_fwd_cp<JT, 2>(a, g, s);
        case 4: return agg_fwd_cp<JT, 4>(a, g, s);
        case 8: return agg_fwd_cp<JT, 8>(a, g, s);
        default: return 2;
    }
}

int launch_agg_fwd(const AggFwdArgs& a, hipStream_t s) {
    if (a.cap_rows <= 0) return 0;
    if (a.j0 != 0 && (a.j0 != 2 || !a.xg || (a.diag && !a.err))) return HGNN_ERR_ARG;
    const dim3 g(ceil_div(a.cap_rows, AGG_WV));
    // both parts at most AGG_NLPR channels wide (or absent): several rows per wave
    const int cgn = a.xg && a.cg > 0 ? a.cg : 0, cpn = a.xp && a.cp > 0 ? a.cp : 0;
    if (AGG_NARROW && a.j0 == 0 && cgn <= AGG_NLPR && cpn <= AGG_NLPR && (cgn > 0 || cpn > 0)) {
        switch (a.jtot) {
            case 3: return agg_fwd_narrow<3>(a, cgn > 0, cpn > 0, s);
            case 4: return agg_fwd_narrow<4>(a, cgn > 0, cpn > 0, s);
            case 5: return agg_fwd_narrow<5>(a, cgn > 0, cpn > 0, s);
            case 6: return agg_fwd_narrow<6>(a, cgn > 0, cpn > 0, s);
            case 7: return agg_fwd_narrow<7>(a, cgn > 0, cpn > 0, s);
            default: return 2;
        }
    }
    switch (a.jtot) {
        case 3: return agg_fwd_cg<3>(a, g, s);
        case 4: return agg_fwd_cg<4>(a, g, s);
        case 5: return agg_fwd_cg<5>(a, g, s);
        case 6: return agg_fwd_cg<6>(a, g, s);
        case 7: return agg_fwd_cg<7>(a, g, s);
        default: return 2;
    }
}

// Backward gathers.  The G gather (transposed operator lists, output = the gradient of the
// half's own features) and the P gather (transposed Pm/Pd lists, output = the other kind's
// features) write different tensors; launch_agg_bwd_pair runs both in one grid (blocks
// [0, gb) gather G, the rest P), so neither runs alone on a partly filled chip.
// Entries [0, n) of one 64-entry chunk of a G row, UB entries in flight (x the slices with a
// nonzero coefficient).
template <int JT, int C, bool V, int UB>
__device__ __forceinline__ void agg_bwd_g_chunk(const AggBwdArgs& a, float4 me, const float (&mx)[JT > 3 ? JT - 3 : 1],
                                                int n, int lane, float (&acc)[C]) {
    for (int e = 0; e < n; e += UB) {
        float x[UB][JT][C], v[UB][JT];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int eu = min(e + u, n - 1);
            const int col = __builtin_amdgcn_readlane(__float_as_int(me.x), eu);
            const bool live = e + u < n;
            v[u][0] = live ? bcast(me.y, eu) : 0.f;
            if constexpr (JT > 1) v[u][1] = live ? bcast(me.z, eu) : 0.f;
            if constexpr (JT > 2) v[u][2] = live ? bcast(me.w, eu) : 0.f;
#pragma unroll
            for (int j = 3; j < JT; ++j) v[u][j] = live ? bcast(mx[j - 3], eu) : 0.f;
            const float* src = a.ing + (long long)col * a.ldg + a.gofs;
            // slices with a zero coefficient are skipped (wave-uniform): I and D live on the
            // diagonal entry only and A^k has no diagonal in general, so an entry needs 1-2
            // of its J+2 gradient blocks -- about half the gathered bytes
#pragma unroll
            for (int j = 0; j < JT; ++j) {
                if (v[u][j] != 0.f) {
                    load_row<C, V>(src + j * a.c, a.c, lane, x[u][j]);
                } else {
#pragma unroll
                    for (int i = 0; i < C; ++i) x[u][j][i] = 0.f;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < UB; ++u)
#pragma unroll
            for (int j = 0; j < JT; ++j)
#pragma unroll
                for (int i = 0; i < C; ++i) acc[i] = fmaf(v[u][j], x[u][j][i], acc[i]);
    }
}

// Long rows (the transposed line-graph lists hold rows of up to ~35 entries: 8 % of the rows,
// 59 % of the entries at config 2) take 8 entries per round trip instead of 4 (serial trace:
// 127.9 -> 122.6 us per step).
constexpr int AGG_LONG = 8;

template <int JT, int C, bool V>
__device__ __forceinline__ void agg_bwd_g(const AggBwdArgs& a, int r, int lane) {
    float acc[C];
    float* o = a.out + (long long)r * a.ldo;
    if (a.accumulate) {
        load_row<C, V>(o, a.c, lane, acc);
    } else {
#pragma unroll
        for (int i = 0; i < C; ++i) acc[i] = 0.f;
    }
    const RowInfo ri = row_info(a.g.rows, r);
    const int stride = a.g.stride;
    for (int e0 = 0; e0 < ri.count; e0 += 64) {
        const int n = min(64, ri.count - e0);
        const float4 me = lane_entry(a.g.entries, stride, ri.start + e0, n, lane);
        float mx[JT > 3 ? JT - 3 : 1];
        mx[0] = 0.f;
        if constexpr (JT > 3) {
#pragma unroll
            for (int j = 3; j < JT; ++j)
                mx[j - 3] = lane < n ? a.g.entries[(long long)(ri.start + e0 + lane) * stride + 1 + j] : 0.f;
        }
        if (n > AGG_LONG) agg_bwd_g_chunk<JT, C, V, AGG_LONG>(a, me, mx, n, lane, acc);
        else agg_bwd_g_chunk<JT, C, V, 4>(a, me, mx, n, lane, acc);
    }
    store_row<C, V>(o, a.c, lane, acc);
}

template <int C, bool V>
__device__ __forceinline__ void agg_bwd_p(const AggBwdArgs& a, int r, int lane) {
    float acc[C];
    float* o = a.out + (long long)r * a.ldo;
    if (a.accumulate) {
        load_row<C, V>(o, a.c, lane, acc);
    } else {
#pragma unroll
        for (int i = 0; i < C; ++i) acc[i] = 0.f;
    }
    const RowInfo ri = row_info(a.p.rows, r);
    for (int e0 = 0; e0 < ri.count; e0 += 64) {
        const int n = min(64, ri.count - e0);
        const float4 me = lane_entry(a.p.entries, 4, ri.start + e0, n, lane);
        for (int e = 0; e < n; e += AGG_U) {
            float xm[AGG_U][C], xd[AGG_U][C], vm[AGG_U], vd[AGG_U];
#pragma unroll
            for (int u = 0; u < AGG_U; ++u) {
                const int eu = min(e + u, n - 1);
                const int col = __builtin_amdgcn_readlane(__float_as_int(me.x), eu);
                const bool live = e + u < n;
                vm[u] = live ? bcast(me.y, eu) : 0.f;
                vd[u] = live ? bcast(me.z, eu) : 0.f;
                const float* src = a.inp + (long long)col * a.ldp;
                load_row<C, V>(src + a.pofs_m, a.c, lane, xm[u]);
                load_row<C, V>(src + a.pofs_d, a.c, lane, xd[u]);
            }
#pragma unroll
            for (int u = 0; u < AGG_U; ++u)
#pragma unroll
                for (int i = 0; i < C; ++i) acc[i] = fmaf(vd[u], xd[u][i], fmaf(vm[u], xm[u][i], acc[i]));
        }
    }
    store_row<C, V>(o, a.c, lane, acc);
}

// MODE 1: G only (ga); 2: P only (pa); 3: blocks [0, gb) G on ga, the rest P on pa.
template <int JT, int CG, int CP, bool V, int MODE>
__global__ void __launch_bounds__(AGG_NT) k_agg_bwd(AggBwdArgs ga, AggBwdArgs pa, int gb) {
    WaveStamp stamp(ga.stamps);
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    if (MODE == 1 || (MODE == 3 && (int)blockIdx.x < gb)) {
        if constexpr (MODE != 2) {
            const int r = __builtin_amdgcn_readfirstlane((int)blockIdx.x * AGG_WV + wv);
            if (r >= *ga.total_rows) return;
            agg_bwd_g<JT, CG, V>(ga, r, lane);
        }
    } else {
        if constexpr (MODE != 1) {
            const int r = __builtin_amdgcn_readfirstlane(((int)blockIdx.x - (MODE == 3 ? gb : 0)) * AGG_WV + wv);
            if (r >= *pa.total_rows) return;
            agg_bwd_p<CP, V>(pa, r, lane);
        }
    }
}

// The backward gathers for c <= AGG_NLPR channels, AGG_NGPW rows per wave (see k_agg_fwd_narrow).  MODE 1: G, 2: P.
// agg_bwd_g / agg_bwd_p run the fmaf chain over the row's entry slots padded per 64-entry chunk to their batch
// (a dead slot: zero coefficients, so x = 0 in G and the last live row in P); here the wave runs to its longest
// row, and a slot past the row's own padded count leaves the accumulator as it is, so the old value of an
// accumulating launch meets the same operations.  A G slice with a zero coefficient is loaded (the slices of a
// narrow row share its cache lines) and selected to 0: fmaf(0, 0, acc) as in agg_bwd_g_chunk.
template <int JT, int MODE>
__global__ void __launch_bounds__(AGG_NT) k_agg_bwd_narrow(AggBwdArgs a) {
    WaveStamp stamp(a.stamps);
    const int r0 = __builtin_amdgcn_readfirstlane((blockIdx.x * AGG_WV + (threadIdx.x >> 6)) * AGG_NGPW);
    const int lane = threadIdx.x & 63, i = lane & (AGG_NLPR - 1), g0 = lane & ~(AGG_NLPR - 1);
    const int total = *a.total_rows;
    if (r0 >= total) return;
    const int r = r0 + (lane >> 3);
    const int rc = min(r, total - 1);  // (rows past the total: a live row, never stored)
    const int ic = min(i, a.c - 1);
    float acc = 0.f;
    if (a.accumulate) acc = a.out[(long long)rc * a.ldo + ic];
    NarrowList l;
    l.init(row_info_lane(MODE == 1 ? a.g.rows : a.p.rows, rc));
    // the slots agg_bwd_g / agg_bwd_p process of this row: whole 64-entry chunks, the last one padded to the batch
    const int cnt = max(l.cnt, 0), rem = cnt & 63;
    const int ub = MODE == 1 && rem > AGG_LONG ? AGG_LONG : 4;
    const int proc = (cnt - rem) + (rem + ub - 1) / ub * ub;
    const int stride = MODE == 1 ? a.g.stride : 4;
    const float* entries = MODE == 1 ? a.g.entries : a.p.entries;
    for (int e0 = 0; e0 < l.wmax; e0 += AGG_NLPR) {
        bool live;
        const float* q = entries + l.at(e0, i, live) * stride;
        float4 me = *reinterpret_cast<const float4*>(q), mx4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (MODE == 1 && JT > 3) mx4 = *reinterpret_cast<const float4*>(q + 4);
        if (!live) {
            me.y = me.z = me.w = 0.f;
            mx4 = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const int nn = min(AGG_NLPR, l.wmax - e0);
        for (int e = 0; e < nn; e += AGG_NU) {
            constexpr int NS = MODE == 1 ? JT : 2;
            float x[AGG_NU][NS], v[AGG_NU][NS];
#pragma unroll
            for (int u = 0; u < AGG_NU; ++u) {
                const int src = g0 + e + u;
                const int col = __float_as_int(grp_bcast(me.x, src));
                v[u][0] = grp_bcast(me.y, src);
                v[u][1] = grp_bcast(me.z, src);
                if constexpr (MODE == 1) {
                    if constexpr (JT > 2) v[u][2] = grp_bcast(me.w, src);
#pragma unroll
                    for (int j = 3; j < JT; ++j) v[u][j] = grp_bcast(f4_at(mx4, j - 3), src);
                    const float* s = a.ing + (long long)col * a.ldg + a.gofs + ic;
#pragma unroll
                    for (int j = 0; j < JT; ++j) x[u][j] = s[j * a.c];
                } else {
                    const float* s = a.inp + (long long)col * a.ldp + ic;
                    x[u][0] = s[a.pofs_m];
                    x[u][1] = s[a.pofs_d];
                }
            }
#pragma unroll
            for (int u = 0; u < AGG_NU; ++u) {
                float t = acc;
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    const float xv = MODE == 1 && v[u][j] == 0.f ? 0.f : x[u][j];
                    t = fmaf(v[u][j], xv, t);
                }
                acc = e0 + e + u < proc ? t : acc;
            }
        }
    }
    if (r < total && i < a.c) a.out[(long long)r * a.ldo + i] = acc;
}

template <int JT>
static int agg_bwd_narrow(const AggBwdArgs& a0, hipStream_t s) {
    const dim3 g(ceil_div(ceil_div(a0.cap_rows, AGG_NGPW), AGG_WV));
    AggBwdArgs a = a0;
    a.stamps = clock_stamps((long long)g.x * AGG_WV);
    if (a.ing) HGNN_KLAUNCH((k_agg_bwd_narrow<JT, 1>), g, dim3(AGG_NT), 0, s, a);
    else HGNN_KLAUNCH((k_agg_bwd_narrow<3, 2>), g, dim3(AGG_NT), 0, s, a);
    HGNN_LAUNCH_CHECK();
    return 0;
}

static bool bwd_vec_g(int cpl, const AggBwdArgs& a) {
    return vec_ok(cpl, a.c, a.ing, {a.ldg, a.gofs}) && vec_ok(cpl, a.c, a.out, {a.ldo});
}
static bool bwd_vec_p(int cpl, const AggBwdArgs& a) {
    return vec_ok(cpl, a.c, a.inp, {a.ldp, a.pofs_m, a.pofs_d}) && vec_ok(cpl, a.c, a.out, {a.ldo});
}

template <int JT, int C>
static int agg_bwd_single(const AggBwdArgs& a0, hipStream_t s) {
    const dim3 g(ceil_div(a0.cap_rows, AGG_WV));
    AggBwdArgs a = a0;
    a.stamps = clock_stamps((long long)g.x * AGG_WV);
    if (a.ing) {
        if (bwd_vec_g(C, a)) HGNN_KLAUNCH((k_agg_bwd<JT, C, C, true, 1>), g, dim3(AGG_NT), 0, s, a, a, 0);
        else HGNN_KLAUNCH((k_agg_bwd<JT, C, C, false, 1>), g, dim3(AGG_NT), 0, s, a, a, 0);
    } else {
        if (bwd_vec_p(C, a)) HGNN_KLAUNCH((k_agg_bwd<3, C, C, true, 2>), g, dim3(AGG_NT), 0, s, a, a, 0);
        else HGNN_KLAUNCH((k_agg_bwd<3, C, C, false, 2>), g, dim3(AGG_NT), 0, s, a, a, 0);
    }
    HGNN_LAUNCH_CHECK();
    return 0;
}

template <int JT>
static int agg_bwd_c(const AggBwdArgs& a, hipStream_t s) {
    if (AGG_NARROW && a.c > 0 && a.c <= AGG_NLPR) return agg_bwd_narrow<JT>(a, s);
    switch (cpl_of(a.c)) {
        case 1: return agg_bwd_single<JT, 1>(a, s);
        case 2: return agg_bwd_single<JT, 2>(a, s);
        case 4: return agg_bwd_single<JT, 4>(a, s);
        case 8: return agg_bwd_single<JT, 8>(a, s);
        default: return 2;
    }
}

int launch_agg_bwd(const AggBwdArgs& a, hipStream_t s) {
    if (a.cap_rows <= 0) return 0;
    if ((a.ing != nullptr) == (a.inp != nullptr)) return 1;  // exactly one of the two gathers
    switch (a.jtot) {
        case 3: return agg_bwd_c<3>(a, s);
        case 4: return agg_bwd_c<4>(a, s);
        case 5: return agg_bwd_c<5>(a, s);
        case 6: return agg_bwd_c<6>(a, s);
        case 7: return agg_bwd_c<7>(a, s);
        default: return 2;
    }
}

template <int JT, int C>
static int agg_bwd_pair_c(const AggBwdArgs& ga0, const AggBwdArgs& pa, hipStream_t s) {
    const int gb = ceil_div(ga0.cap_rows, AGG_WV), pb = ceil_div(pa.cap_rows, AGG_WV);
    AggBwdArgs ga = ga0;
    ga.stamps = clock_stamps((long long)(gb + pb) * AGG_WV);
    HGNN_KLAUNCH((k_agg_bwd<JT, C, C, true, 3>), dim3(gb + pb), dim3(AGG_NT), 0, s, ga, pa, gb);
    HGNN_LAUNCH_CHECK();
    return 0;
}

template <int JT>
static int agg_bwd_pair_j(const AggBwdArgs& ga, const AggBwdArgs& pa, hipStream_t s) {
    switch (cpl_of(ga.c)) {
        case 1: return agg_bwd_pair_c<JT, 1>(ga, pa, s);
        case 2: return agg_bwd_pair_c<JT, 2>(ga, pa, s);
        case 4: return agg_bwd_pair_c<JT, 4>(ga, pa, s);
        case 8: return agg_bwd_pair_c<JT, 8>(ga, pa, s);
        default: return 2;
    }
}

int launch_agg_bwd_pair(const AggBwdArgs& ga, const AggBwdArgs& pa, hipStream_t s) {
    // one grid for both gathers when they share the lane layout and the vector path;
    // otherwise two launches
    const int cpl = cpl_of(ga.c);
    const bool pair = ga.ing && !ga.inp && pa.inp && !pa.ing && ga.cap_rows > 0 && pa.cap_rows > 0 &&
                      cpl > 0 && cpl == cpl_of(pa.c) && ga.jtot == pa.jtot && bwd_vec_g(cpl, ga) &&
                      bwd_vec_p(cpl, pa);
    if (!pair) {
        int r = launch_agg_bwd(ga, s);
        if (r) return r;
        return launch_agg_bwd(pa, s);
    }
    switch (ga.jtot) {
        case 3: return agg_bwd_pair_j<3>(ga, pa, s);
        case 4: return agg_bwd_pair_j<4>(ga, pa, s);
        case 5: return agg_bwd_pair_j<5>(ga, pa, s);
        case 6: return agg_bwd_pair_j<6>(ga, pa, s);
        case 7: return agg_bwd_pair_j<7>(ga, pa, s);
        default: return 2;
    }
}

}  // namespace hgnn
