// CCN-1D on the general path: the three kernels of a level (ccn.hip's header comment has the math) and their
// launchers.
#include "ccn_general.h"

namespace hgnn {
namespace {

// One wave per node; lane x = receptive-field position, in 64-lane chunks for degrees above 64
// (SBM-1000 nodes reach d ~ 200).  Level-0 input is X tiled (utils_ccn.py:212-216): F_0[j][p] = X[j].
// Row sums (over a) accumulate per position in the wave's LDS row, column sums (over x) are wave
// sums of the chunks; for d <= 64 the summation order is the single-chunk one.
__global__ void __launch_bounds__(256) k_ccn1_fwd(CcnPlanView v, const int* total_nodes, const float* __restrict__ fin,
                                                  int level0, const float* __restrict__ X, int cin,
                                                  const float* __restrict__ W, const float* __restrict__ bias, int h,
                                                  float* __restrict__ coll, float* __restrict__ fout) {
    __shared__ float srow[4][CCN1_MAXD];
    const int wv = threadIdx.x >> 6;
    const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv);
    const int lane = threadIdx.x & 63;
    if (i >= *total_nodes) return;
    const int n = v.deg[i];
    if (n > CCN1_MAXD) return;
    const int* ni = v.nbr + (long long)i * v.nmax;
    const int* pi = v.pos + v.off2[i];
    const long long r0 = v.off1[i];
    const int k2 = 2 * cin;
    if (n <= 64 && cin <= C1F) {
        // one chunk, no cross-lane reduction: lane l keeps the row sum of position x = l (a ascending) and
        // the column sum of neighbour a = l (x ascending), four neighbours per round, every channel at once
        const int l = lane;
        const bool vl = l < n;
        const int jl = ni[vl ? l : 0];
        const float* fl = level0 ? X + (long long)jl * cin : fin + (long long)v.off1[jl] * cin;
        float rs[C1F], colv[C1F];
#pragma unroll
        for (int c = 0; c < C1F; ++c) rs[c] = colv[c] = 0.f;
        for (int k0 = 0; k0 < n; k0 += 4) {
            float t1[4][C1F], t2[4][C1F];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = min(k0 + q, n - 1);
                const int j = ni[k];
                const int p1 = vl ? pi[(long long)k * n + l] : -1;  // position x = l in N(j_k)
                const int p2 = vl ? pi[(long long)l * n + k] : -1;  // position x = k in N(j_l)
                const bool ok1 = p1 >= 0 && k0 + q < n, ok2 = p2 >= 0 && k0 + q < n;
                const float* s1 = level0 ? X + (long long)j * cin : fin + ((long long)v.off1[j] + max(p1, 0)) * cin;
                const float* s2 = level0 ? fl : fl + (long long)max(p2, 0) * cin;
#pragma unroll
                for (int c = 0; c < C1F; ++c) {
                    t1[q][c] = (c < cin && ok1) ? s1[c] : 0.f;
                    t2[q][c] = (c < cin && ok2) ? s2[c] : 0.f;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int c = 0; c < C1F; ++c) {
                    rs[c] += t1[q][c];
                    colv[c] += t2[q][c];
                }
        }
        if (vl) {
            const long long row = r0 + l;
#pragma unroll
            for (int c = 0; c < C1F; ++c)
                if (c < cin) {
                    coll[row * k2 + c] = rs[c];
                    coll[row * k2 + cin + c] = colv[c];
                }
            for (int o = 0; o < h; ++o) {
                float s = bias[o];
#pragma unroll
                for (int c = 0; c < C1F; ++c)
                    if (c < cin) s = fmaf(W[o * k2 + c], rs[c], s);
#pragma unroll
                for (int c = 0; c < C1F; ++c)
                    if (c < cin) s = fmaf(W[o * k2 + cin + c], colv[c], s);
                fout[row * h + o] = s < 0.f ? 0.f : s;
            }
        }
        return;
    }
    float* rs = srow[wv];  // wave-private; each position owned by one lane
    for (int c = 0; c < cin; ++c) {
        for (int x = lane; x < n; x += 64) rs[x] = 0.f;
        for (int a = 0; a < n; ++a) {
            const int j = ni[a];
            const long long rj = v.off1[j];
            float cs = 0.f;
            for (int x0 = 0; x0 < n; x0 += 64) {
                const int x = x0 + lane;
                float t = 0.f;
                if (x < n) {
                    const int p = pi[(long long)a * n + x];
                    if (p >= 0) t = level0 ? X[(long long)j * cin + c] : fin[(rj + p) * cin + c];
                    rs[x] += t;
                }
                cs += wave_sum(t);
            }
            if (lane == 0) coll[(r0 + a) * k2 + cin + c] = cs;
        }
        for (int x = lane; x < n; x += 64) coll[(r0 + x) * k2 + c] = rs[x];
    }
    for (int x = lane; x < n; x += 64) {
        const long long row = r0 + x;
        for (int o = 0; o < h; ++o) {
            float s = bias[o];
            for (int k = 0; k < k2; ++k) s = fmaf(W[o * k2 + k], coll[row * k2 + k], s);
            fout[row * h + o] = s < 0.f ? 0.f : s;
        }
    }
}

// dpre = dF * relu'; param partials per node; dcoll = W^T dpre  -> [drow | dcol]
__global__ void __launch_bounds__(256) k_ccn1_bwd_node(CcnPlanView v, const int* total_nodes,
                                                       const float* __restrict__ dF, const float* __restrict__ F,
                                                       const float* __restrict__ coll, int cin,
                                                       const float* __restrict__ W, int h, float* __restrict__ dcoll,
                                                       float* __restrict__ ppart) {
    const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    if (i >= *total_nodes) return;
    int n = v.deg[i];
    if (n > CCN1_MAXD) n = 0;  // flagged by the plan; partials written as zeros
    const int k2 = 2 * cin;
    const long long r0 = v.off1[i];
    float* pp = ppart + (long long)i * (h * k2 + h);
    auto dpre = [&](long long row, int o) { return F[row * h + o] > 0.f ? dF[row * h + o] : 0.f; };
    if (n <= 64 && cin <= C1F && h <= C1H) {  // one chunk: every value of lane x's row loaded once
        const int x = lane;
        const bool vx = x < n;
        const long long row = r0 + x;
        float dp[C1H], cl[2 * C1F];
#pragma unroll
        for (int o = 0; o < C1H; ++o) dp[o] = (vx && o < h) ? dpre(row, o) : 0.f;
#pragma unroll
        for (int k = 0; k < 2 * C1F; ++k) cl[k] = (vx && k < k2) ? coll[row * k2 + k] : 0.f;
#pragma unroll
        for (int o = 0; o < C1H; ++o) {
            if (o >= h) break;
#pragma unroll
            for (int k = 0; k < 2 * C1F; ++k) {
                if (k >= k2) break;
                const float t = wave_total(dp[o] * cl[k]);
                if (lane == 0) pp[o * k2 + k] = t;
            }
            const float sb = wave_total(dp[o]);
            if (lane == 0) pp[h * k2 + o] = sb;
        }
        if (vx)
#pragma unroll
            for (int k = 0; k < 2 * C1F; ++k) {
                if (k >= k2) break;
                float t = 0.f;
#pragma unroll
                for (int o = 0; o < C1H; ++o)
                    if (o < h) t = fmaf(W[o * k2 + k], dp[o], t);
                dcoll[row * k2 + k] = t;
            }
        return;
    }
    for (int o = 0; o < h; ++o) {
        for (int k = 0; k < k2; ++k) {
            float acc = 0.f;
            for (int x = lane; x < n; x += 64) acc += dpre(r0 + x, o) * coll[(r0 + x) * k2 + k];
            const float s = wave_sum(acc);
            if (lane == 0) pp[o * k2 + k] = s;
        }
        float accb = 0.f;
        for (int x = lane; x < n; x += 64) accb += dpre(r0 + x, o);
        const float sb = wave_sum(accb);
        if (lane == 0) pp[h * k2 + o] = sb;
    }
    for (int x = lane; x < n; x += 64) {
        const long long row = r0 + x;
        for (int k = 0; k < k2; ++k) {
            float s = 0.f;
            for (int o = 0; o < h; ++o) s = fmaf(W[o * k2 + k], dpre(row, o), s);
            dcoll[row * k2 + k] = s;
        }
    }
}

// dF_prev[j][u] = sum_{i in N(j)} [q(u) valid] (drow_i[q(u)] + dcol_i[aj]) (+ readout term);
// level 0: dX[j] = sum_u of it + d_j * dsum0
__global__ void __launch_bounds__(256) k_ccn1_bwd_gather(CcnPlanView v, const int* total_nodes,
                                                         const float* __restrict__ dcoll, int cin,
                                                         const float* __restrict__ dsum, int dsum_ld, int dsum_off,
                                                         int level0, float* __restrict__ dout) {
    const int j = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    if (j >= *total_nodes) return;
    const int n = v.deg[j];
    if (n > CCN1_MAXD) return;
    const int* nj = v.nbr + (long long)j * v.nmax;
    const int* pj = v.pos + v.off2[j];
    const int sj = v.selfpos[j];
    const int g = v.graph[j];
    const int k2 = 2 * cin;
    if (n <= 64 && cin <= C1F) {  // one chunk: the indices of a neighbour once for every channel
        const int u = lane;
        const bool vu = u < n;
        float acc[C1F];
#pragma unroll
        for (int c = 0; c < C1F; ++c) acc[c] = 0.f;
        for (int a0 = 0; a0 < n; a0 += 4) {
            float t1[4][C1F], t2[4][C1F];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int a = min(a0 + q, n - 1);
                const int i = nj[a];
                const int aj = pj[(long long)a * n + sj];
                const int qq = vu ? pj[(long long)a * n + u] : -1;
                const bool ok = qq >= 0 && a0 + q < n;
                const long long ri = v.off1[i];
                const float* s1 = dcoll + (ri + max(qq, 0)) * k2;
                const float* s2 = dcoll + (ri + aj) * k2 + cin;
#pragma unroll
                for (int c = 0; c < C1F; ++c) {
                    t1[q][c] = (c < cin && ok) ? s1[c] : 0.f;
                    t2[q][c] = (c < cin && ok) ? s2[c] : 0.f;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int c = 0; c < C1F; ++c) acc[c] += t1[q][c] + t2[q][c];
        }
#pragma unroll
        for (int c = 0; c < C1F; ++c) {
            if (c >= cin) break;
            const float rd = dsum ? dsum[(long long)g * dsum_ld + dsum_off + c] : 0.f;
            if (level0) {
                const float tot = wave_total(vu ? acc[c] : 0.f);
                if (lane == 0) dout[(long long)j * cin + c] = tot + (float)n * rd;
            } else if (vu) {
                dout[((long long)v.off1[j] + u) * cin + c] = acc[c] + rd;
            }
        }
        return;
    }
    for (int c = 0; c < cin; ++c) {
        const float rd = dsum ? dsum[(long long)g * dsum_ld + dsum_off + c] : 0.f;
        float tot = 0.f;
        for (int u = lane; u < n; u += 64) {
            float acc = 0.f;
            for (int a = 0; a < n; ++a) {
                const int i = nj[a];
                const int q = pj[(long long)a * n + u];
                if (q < 0) continue;
                const int aj = pj[(long long)a * n + sj];
                const long long ri = v.off1[i];
                acc += dcoll[(ri + q) * k2 + c] + dcoll[(ri + aj) * k2 + cin + c];
            }
            if (level0) tot += acc;
            else dout[((long long)v.off1[j] + u) * cin + c] = acc + rd;
        }
        if (level0) {
            const float s = wave_sum(tot);
            if (lane == 0) dout[(long long)j * cin + c] = s + (float)n * rd;
        }
    }
}

}  // namespace

int launch_ccn1_fwd(const CcnPlanView& v, const int* tot, int nodes, const float* fin, int level0, const float* X,
                    int cin, const float* W, const float* b, int h, float* coll, float* fout, hipStream_t s) {
    HGNN_KLAUNCH(k_ccn1_fwd, ccn_grid4(nodes), dim3(256), 0, s, v, tot, fin, level0, X, cin, W, b, h, coll, fout);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

int launch_ccn1_bwd_node(const CcnPlanView& v, const int* tot, int nodes, const float* dF, const float* F,
                         const float* coll, int cin, const float* W, int h, float* dcoll, float* ppart, hipStream_t s) {
    HGNN_KLAUNCH(k_ccn1_bwd_node, ccn_grid4(nodes), dim3(256), 0, s, v, tot, dF, F, coll, cin, W, h, dcoll, ppart);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

int launch_ccn1_bwd_gather(const CcnPlanView& v, const int* tot, int nodes, const float* dcoll, int cin,
                           const float* dsum, int dsum_ld, int dsum_off, int level0, float* dout, hipStream_t s) {
    HGNN_KLAUNCH(k_ccn1_bwd_gather, ccn_grid4(nodes), dim3(256), 0, s, v, tot, dcoll, cin, dsum, dsum_ld, dsum_off,
                 level0, dout);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

}  // namespace hgnn
