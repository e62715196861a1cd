// CCN-2D on the general path, receptive fields of degree 65..256: a different algorithm from ccn2.hip's (the
// forward saves the contraction statistics, C2Save, and the backward node pass reads them), with its launchers.
#include "ccn_general.h"

namespace hgnn {
namespace {

// The same passes as k_ccn2_fwd / k_ccn2_bwd_node / k_ccn2_bwd_gather for the nodes whose receptive
// field exceeds one wave (SBM graphs of several hundred nodes: d ~ 70-210): the lane index walks its
// range in 64-lane chunks, the common-neighbour sets C_a are CCN_BW 64-bit words per row (LDS), and
// the position maps are read from global memory (n^2 ints per node, L2-resident) instead of LDS.
// Launched only when a batch can hold such degrees (nmax > 64); nodes with d <= 64 exit at once
// (they are the fast kernels'), so every node is computed by exactly one of the two.
template <int CM, int HM>
__global__ void __launch_bounds__(256) k_ccn2_fwd_big(CcnPlanView v, const int* total_nodes,
                                                      const float* __restrict__ fin, int level0,
                                                      const float* __restrict__ X, int cin,
                                                      const float* __restrict__ W, const float* __restrict__ bias,
                                                      int h, C2Save sv, float* __restrict__ fout,
                                                      float* __restrict__ nsum) {
    __shared__ unsigned long long vmask[CCN_BIGD][CCN_BW];  // bit x of row a: x in C_a
    __shared__ int s_j[CCN_BIGD], s_dj[CCN_BIGD], s_oj[CCN_BIGD], s_mc[CCN_BIGD];
    __shared__ float sred[2][4][CM];
    const int i = blockIdx.x;
    if (i >= *total_nodes) return;
    const int n = v.deg[i];
    if (n <= CCN_MAXD || n > CCN_BIGD || cin > CM || h > HM) return;
    const int nw = (n + 63) >> 6;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int* ni = v.nbr + (long long)i * v.nmax;
    const long long o2 = v.off2[i], o1 = v.off1[i];
    const int* sp = v.pos + o2;  // sp[a n + x]
    for (int t = threadIdx.x; t < n; t += 256) {
        const int j = ni[t];
        s_j[t] = j;
        s_dj[t] = v.deg[j];
        s_oj[t] = v.off2[j];
    }
    for (int a = wv; a < n; a += 4) {
        int cnt = 0;
        for (int w = 0; w < nw; ++w) {
            const int x = w * 64 + lane;
            const unsigned long long m = __ballot(x < n && sp[(long long)a * n + x] >= 0);
            if (lane == 0) vmask[a][w] = m;
            cnt += __popcll(m);
        }
        if (lane == 0) s_mc[a] = cnt;
    }
    __syncthreads();

    // ---- pass A: wave per neighbour a, lane b (64-lane chunks)
    float tq[CM], td3[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) tq[c] = td3[c] = 0.f;
    for (int a = wv; a < n; a += 4) {
        const int j = s_j[a], dj = s_dj[a];
        const bool va = mbit(vmask[a], a);
        float qa[CM];
#pragma unroll
        for (int c = 0; c < CM; ++c) qa[c] = 0.f;
        for (int b0 = 0; b0 < n; b0 += 64) {
            const int b = b0 + lane;
            const int pb = b < n ? sp[(long long)a * n + b] : -1;
            const bool vb = pb >= 0;
            float sc[CM], d1[CM], d2[CM];
#pragma unroll
            for (int c = 0; c < CM; ++c) sc[c] = d1[c] = d2[c] = 0.f;
            if (level0) {
                const float mf = (float)s_mc[a];
#pragma unroll
                for (int c = 0; c < CM; ++c) {
                    if (c >= cin) break;
                    const float xj = X[(long long)j * cin + c];
                    sc[c] = vb ? mf * xj : 0.f;
                    d1[c] = vb ? xj : 0.f;
                    d2[c] = (vb && va) ? xj : 0.f;
                }
            } else {
                const float* row = fin + ((long long)s_oj[a] + (long long)(vb ? pb : 0) * dj) * cin;
                for (int w = 0; w < nw; ++w) {
                    unsigned long long zs = vmask[a][w];
                    while (zs) {
                        int zz[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            zz[u] = zs ? w * 64 + __ffsll((long long)zs) - 1 : -1;
                            zs &= zs ? zs - 1ull : 0ull;
                        }
                        float t[4][CM];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int pz = zz[u] >= 0 ? sp[(long long)a * n + zz[u]] : 0;
#pragma unroll
                            for (int c = 0; c < CM; ++c) t[u][c] = c < cin ? row[(long long)pz * cin + c] : 0.f;
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int z = zz[u];
                            if (z < 0) break;
                            if (vb) {
#pragma unroll
                                for (int c = 0; c < CM; ++c) {
                                    if (c >= cin) break;
                                    sc[c] += t[u][c];
                                    if (z == b) d1[c] = t[u][c];
                                    if (z == a) d2[c] = t[u][c];
                                }
                            }
                        }
                    }
                }
            }
            if (b < n) {
                const long long r = (o2 + (long long)a * n + b) * cin;
#pragma unroll
                for (int c = 0; c < CM; ++c) {
                    if (c >= cin) break;
                    sv.Sc[r + c] = sc[c];
                    sv.D1[r + c] = d1[c];
                    sv.D2[r + c] = d2[c];
                }
            }
#pragma unroll
            for (int c = 0; c < CM; ++c) {
                if (c >= cin) break;
                qa[c] += wave_sum(sc[c]);
                if (b == a) td3[c] += d1[c];  // T[a][a][a]
            }
        }
#pragma unroll
        for (int c = 0; c < CM; ++c) {
            if (c >= cin) break;
            if (lane == 0) sv.q1[(o1 + a) * cin + c] = qa[c];
            tq[c] += qa[c];
        }
    }
#pragma unroll
    for (int c = 0; c < CM; ++c) {
        if (c >= cin) break;
        const float t3 = wave_sum(td3[c]);
        if (lane == 0) {
            sred[0][wv][c] = tq[c];
            sred[1][wv][c] = t3;
        }
    }

    // ---- pass B: wave per receptive-field row b, lane z (chunks); the a with b in C_a ascending
    for (int b = wv; b < n; b += 4) {
        float q3[CM];
#pragma unroll
        for (int c = 0; c < CM; ++c) q3[c] = 0.f;
        for (int z0 = 0; z0 < n; z0 += 64) {
            const int z = z0 + lane;
            float sa[CM];
#pragma unroll
            for (int c = 0; c < CM; ++c) sa[c] = 0.f;
            for (int a0 = 0; a0 < n; a0 += 64) {
                const int al = a0 + lane < n ? a0 + lane : 0;
                unsigned long long as = __ballot(a0 + lane < n && mbit(vmask[al], b));
                while (as) {
                    int aa[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        aa[u] = as ? a0 + __ffsll((long long)as) - 1 : -1;
                        as &= as ? as - 1ull : 0ull;
                    }
                    float t[4][CM];
                    bool vz[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int a = aa[u] >= 0 ? aa[u] : 0;
                        vz[u] = aa[u] >= 0 && z < n && mbit(vmask[a], z);
                        const float* q;
                        if (level0) {
                            q = X + (long long)s_j[a] * cin;
                        } else {
                            const int pb = max(sp[(long long)a * n + b], 0), pz = vz[u] ? sp[(long long)a * n + z] : 0;
                            q = fin + ((long long)s_oj[a] + (long long)pb * s_dj[a] + pz) * cin;
                        }
#pragma unroll
                        for (int c = 0; c < CM; ++c) t[u][c] = c < cin ? q[c] : 0.f;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (aa[u] < 0) break;
                        if (vz[u]) {
#pragma unroll
                            for (int c = 0; c < CM; ++c) {
                                if (c >= cin) break;
                                sa[c] += t[u][c];
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < CM; ++c) {
                if (c >= cin) break;
                if (z < n) sv.Sa[(o2 + (long long)b * n + z) * cin + c] = sa[c];
                q3[c] += wave_sum(sa[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < CM; ++c) {
            if (c >= cin) break;
            if (lane == 0) sv.q3[(o1 + b) * cin + c] = q3[c];
        }
    }
    __syncthreads();
    if (threadIdx.x < cin) {
        const int c = threadIdx.x;
        float t = 0.f, t3 = 0.f;
        for (int w = 0; w < 4; ++w) {
            t += sred[0][w][c];
            t3 += sred[1][w][c];
        }
        sv.tot[(long long)i * cin + c] = t;
        sv.d3[(long long)i * cin + c] = t3;
    }
    __syncthreads();
    // output stage: as k_ccn2_fwd
    const float nf = (float)n;
    const int K = 18 * cin;
    __shared__ float sw[HM * 18 * CM];
    for (int t = threadIdx.x; t < h * K; t += 256) sw[t] = W[t];
    __syncthreads();
    float ns[HM];  // this node's sum of F_out (readout)
#pragma unroll
    for (int o = 0; o < HM; ++o) ns[o] = 0.f;
    for (int e = threadIdx.x; e < n * n; e += 256) {
        const int x = e / n, y = e % n;
        float s[HM];
#pragma unroll
        for (int o = 0; o < HM; ++o) s[o] = o < h ? bias[o] : 0.f;
        for (int c = 0; c < cin; ++c) {
            const float sc = sv.Sc[(o2 + e) * cin + c];
            const float sa = sv.Sa[(o2 + e) * cin + c];
            float blk[18];
            blk[0] = nf * sc;
            blk[1] = sv.q1[(o1 + x) * cin + c];
            blk[2] = nf * sa;
            blk[3] = sv.q3[(o1 + x) * cin + c];
            blk[4] = x == y ? sv.tot[(long long)i * cin + c] : 0.f;
            blk[5] = sc;
#pragma unroll
            for (int q = 6; q < 15; ++q) blk[q] = nf * sc;
            blk[15] = sv.D1[(o2 + e) * cin + c];
            blk[16] = sv.D2[(o2 + (long long)y * n + x) * cin + c];
            blk[17] = x == y ? sv.d3[(long long)i * cin + c] : 0.f;
#pragma unroll
            for (int o = 0; o < HM; ++o) {
                if (o >= h) break;
                const float* w = sw + o * K;
#pragma unroll
                for (int q = 0; q < 18; ++q) s[o] = fmaf(w[q * cin + c], blk[q], s[o]);
            }
        }
#pragma unroll
        for (int o = 0; o < HM; ++o) {
            if (o >= h) break;
            s[o] = s[o] < 0.f ? 0.f : s[o];
            fout[(o2 + e) * h + o] = s[o];
            ns[o] += s[o];
        }
    }
    __shared__ float s_ns[4][HM];
#pragma unroll
    for (int o = 0; o < HM; ++o) {
        const float t = wave_total(ns[o]);
        if (lane == 0) s_ns[wv][o] = t;
    }
    __syncthreads();
    if ((int)threadIdx.x < h)
        nsum[(long long)i * h + threadIdx.x] =
            (s_ns[0][threadIdx.x] + s_ns[1][threadIdx.x]) + (s_ns[2][threadIdx.x] + s_ns[3][threadIdx.x]);
}

// Backward node pass of the degrees 65..256 (their forward: k_ccn2_fwd_big, which saves the
// contraction statistics C2Save): parameter partials from the saved statistics, the gradient
// matrices of the contraction blocks (C2Grad, this node only) and, at level 0, the per-neighbour
// sums G[a] for k_ccn2_dx0; the dp format for the gather kernels follows in k_c2_dp_big.
// One sweep over the n^2 entries per output o for the parameter partials (the 9 distinct
// contraction blocks x cin accumulate in registers, then one wave-sum + LDS combine each), and one
// sweep for the input-side gradients (every channel of an entry from one read of dpre); the level-0
// reduction walks 64-lane chunks and multi-word common-neighbour sets.
template <int CM, int HM>
__global__ void __launch_bounds__(256) k_ccn2_bwd_node_big(CcnPlanView v, const int* total_nodes,
                                                       const float* __restrict__ dF, const float* __restrict__ F,
                                                       C2Save sv, int cin, const float* __restrict__ W, int h,
                                                       C2Grad gd, float* __restrict__ ppart,
                                                       float* __restrict__ g0) {
    constexpr int MAXN = CCN_BIGD;
    __shared__ float sdq1[MAXN * CM], sdq3[MAXN * CM];
    // the sums whose rounding error does not average out are summed in fp64: dq1[a] and dtot reach whole rows / every
    // entry (the node's G[a] carries them m_a^2 times), dd3 every diagonal one; the bias partial and G[a] are single
    // long sums.  On a star's hub (n = 130) fp32 sums and LDS float atomics here left dX 34 ulp off.
    __shared__ double sdtot[CM], sdd3[CM], redb[4], strd[4][HM];
    __shared__ float red[4][10 * CM];
    __shared__ float sw[HM * 18 * CM];
    const int i = blockIdx.x;
    if (i >= *total_nodes) return;
    const int n = v.deg[i];
    if (n <= CCN_MAXD || n > CCN_BIGD || cin > CM || h > HM) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long o2 = v.off2[i], o1 = v.off1[i];
    const float nf = (float)n;
    const int K = 18 * cin;
    float* pp = ppart + (long long)i * (h * K + h);
    for (int t = threadIdx.x; t < h * K; t += 256) sw[t] = W[t];
    // parameter partials: dW[o][q*C + c] = sum_xy dpre[x][y][o] * block_q[x][y][c]
    // distinct blocks: 0 (n Sc; also 6..14), 1 q1, 2 n Sa, 3 q3, 4 tot (diag), 5 Sc, 15 D1, 16 D2^T, 17 d3 (diag)
    for (int o = 0; o < h; ++o) {
        float acc[9][CM];
        double sb = 0.0;
#pragma unroll
        for (int q = 0; q < 9; ++q)
#pragma unroll
            for (int c = 0; c < CM; ++c) acc[q][c] = 0.f;
        for (int e = threadIdx.x; e < n * n; e += 256) {
            const int x = e / n, y = e % n;
            const long long r = o2 + e;
            const float dp = F[r * h + o] > 0.f ? dF[r * h + o] : 0.f;
            sb += dp;
#pragma unroll
            for (int c = 0; c < CM; ++c) {
                if (c >= cin) break;
                const float sc = sv.Sc[r * cin + c];
                acc[0][c] = fmaf(dp, nf * sc, acc[0][c]);
                acc[1][c] = fmaf(dp, sv.q1[(o1 + x) * cin + c], acc[1][c]);
                acc[2][c] = fmaf(dp, nf * sv.Sa[r * cin + c], acc[2][c]);
                acc[3][c] = fmaf(dp, sv.q3[(o1 + x) * cin + c], acc[3][c]);
                if (x == y) {
                    acc[4][c] = fmaf(dp, sv.tot[(long long)i * cin + c], acc[4][c]);
                    acc[8][c] = fmaf(dp, sv.d3[(long long)i * cin + c], acc[8][c]);
                }
                acc[5][c] = fmaf(dp, sc, acc[5][c]);
                acc[6][c] = fmaf(dp, sv.D1[r * cin + c], acc[6][c]);
                acc[7][c] = fmaf(dp, sv.D2[(o2 + y * n + x) * cin + c], acc[7][c]);
            }
        }
#pragma unroll
        for (int q = 0; q < 9; ++q)
#pragma unroll
            for (int c = 0; c < CM; ++c) {
                if (c >= cin) break;
                const float t = wave_sum(acc[q][c]);
                if (lane == 0) red[wv][q * CM + c] = t;
            }
        sb = wave_sum_d(sb);
        if (lane == 0) redb[wv] = sb;
        __syncthreads();
        for (int t = threadIdx.x; t < 18 * cin; t += 256) {
            const int q = t / cin, c = t % cin;
            const int d = q < 6 ? q : (q < 15 ? 0 : q - 9);  // distinct-block index of q
            pp[o * K + q * cin + c] = red[0][d * CM + c] + red[1][d * CM + c] + red[2][d * CM + c] +
                                      red[3][d * CM + c];
        }
        if (threadIdx.x == 0) pp[h * K + o] = (float)((redb[0] + redb[1]) + (redb[2] + redb[3]));
        __syncthreads();
    }
    // q1 / q3 receive the row sums of dpre and tot / d3 its trace (g_q is linear in dpre): wave per row, fp64 sums,
    // then the h-term projections  dq1[x] = W1^T rdp[x], dq3[x] = W3^T rdp[x], dtot = W4^T tr, dd3 = W17^T tr
    {
        double tr[HM];
#pragma unroll
        for (int o = 0; o < HM; ++o) tr[o] = 0.0;
        for (int x = wv; x < n; x += 4) {
            double rs[HM];
#pragma unroll
            for (int o = 0; o < HM; ++o) rs[o] = 0.0;
            for (int y = lane; y < n; y += 64) {
                const long long r = o2 + (long long)x * n + y;
#pragma unroll
                for (int o = 0; o < HM; ++o) {
                    if (o >= h) break;
                    const double dp = F[r * h + o] > 0.f ? (double)dF[r * h + o] : 0.0;
                    rs[o] += dp;
                    if (y == x) tr[o] += dp;
                }
            }
#pragma unroll
            for (int o = 0; o < HM; ++o)
                if (o < h) rs[o] = wave_sum_d(rs[o]);
            if (lane < cin) {
                double s1 = 0.0, s3 = 0.0;
#pragma unroll
                for (int o = 0; o < HM; ++o) {
                    if (o >= h) break;
                    s1 += (double)sw[o * K + cin + lane] * rs[o];
                    s3 += (double)sw[o * K + 3 * cin + lane] * rs[o];
                }
                sdq1[x * CM + lane] = (float)s1;
                sdq3[x * CM + lane] = (float)s3;
            }
        }
#pragma unroll
        for (int o = 0; o < HM; ++o) {
            const double t = wave_sum_d(tr[o]);
            if (lane == 0) strd[wv][o] = t;
        }
        __syncthreads();
        if ((int)threadIdx.x < cin) {
            double t4 = 0.0, t17 = 0.0;
            for (int o = 0; o < h; ++o) {
                const double t = (strd[0][o] + strd[1][o]) + (strd[2][o] + strd[3][o]);
                t4 += (double)sw[o * K + 4 * cin + threadIdx.x] * t;
                t17 += (double)sw[o * K + 17 * cin + threadIdx.x] * t;
            }
            sdtot[threadIdx.x] = t4;
            sdd3[threadIdx.x] = t17;
        }
    }
    // input-side gradients of the contraction blocks: g_q = W_q^T dpre
    for (int e = threadIdx.x; e < n * n; e += 256) {
        const int x = e / n, y = e % n;
        const long long r = o2 + e;
        float dp[HM];
#pragma unroll
        for (int o = 0; o < HM; ++o) dp[o] = (o < h && F[r * h + o] > 0.f) ? dF[r * h + o] : 0.f;
        for (int c = 0; c < cin; ++c) {
            float g[18];
#pragma unroll
            for (int q = 0; q < 18; ++q) g[q] = 0.f;
#pragma unroll
            for (int o = 0; o < HM; ++o) {
                if (o >= h) break;
                const float* w = sw + o * K;
#pragma unroll
                for (int q = 0; q < 18; ++q) g[q] = fmaf(w[q * cin + c], dp[o], g[q]);
            }
            float s9 = 0.f;
#pragma unroll
            for (int q = 6; q < 15; ++q) s9 += g[q];
            gd.dSc[r * cin + c] = nf * (g[0] + s9) + g[5];
            gd.dSa[r * cin + c] = nf * g[2];
            gd.dD1[r * cin + c] = g[15];
            gd.dD2[(o2 + y * n + x) * cin + c] = g[16];
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n * n; e += 256) {
        const int a = e / n;
        const long long r = o2 + e;
        for (int c = 0; c < cin; ++c) {
            gd.dSc[r * cin + c] += sdq1[a * CM + c];                 // q1[a] = sum_b Sc[a][b]
            gd.dSa[r * cin + c] += sdq3[a * CM + c] + (float)sdtot[c];  // q3[b] = sum_z Sa[b][z]; tot: every entry
        }
    }
    if (threadIdx.x < cin) gd.dd3[(long long)i * cin + threadIdx.x] = (float)sdd3[threadIdx.x];
    if (!g0) return;
    // Level 0 (F_0[j] = X[j] tiled): dX[j] needs only the sum of dT_i[a_j][b][z] over the valid (b, z),
    // so node i reduces its own gradient matrices per neighbour a (coalesced, L2-hot) instead of
    // every j gathering them:  G[a] = m_a sum_{b in C_a} dSc[a][b] + sum_{b,z in C_a} dSa[b][z]
    //   + sum_{b in C_a} dD1[a][b] + [a in C_a] (sum_{b in C_a} dD2[a][b] + dd3),  C_a = {x: pos_a(x) >= 0}
    // dSa of one channel is staged in LDS so the masked row sums read LDS, not scattered HBM rows
    __shared__ unsigned long long vmb[CCN_BIGD][CCN_BW];
    __shared__ int smc[CCN_BIGD];
    const int nw = (n + 63) >> 6;
    __syncthreads();
    for (int a = wv; a < n; a += 4) {
        int cnt = 0;
        for (int w = 0; w < nw; ++w) {
            const int x = w * 64 + lane;
            const unsigned long long m = __ballot(x < n && v.pos[o2 + (long long)a * n + x] >= 0);
            if (lane == 0) vmb[a][w] = m;
            cnt += __popcll(m);
        }
        if (lane == 0) smc[a] = cnt;
    }
    __syncthreads();
    for (int c = 0; c < cin; ++c)
        for (int a = wv; a < n; a += 4) {
            const bool va = mbit(vmb[a], a);
            const float mf = (float)smc[a];
            double t = 0.0;  // up to n^2 / 64 terms a lane: fp64, or the hub of a star loses ~sqrt(n) ulp here
            for (int b = lane; b < n; b += 64) {
                if (!mbit(vmb[a], b)) continue;
                const long long rab = (o2 + (long long)a * n + b) * cin + c;
                t += (double)mf * (double)gd.dSc[rab] + (double)gd.dD1[rab] + (va ? (double)gd.dD2[rab] : 0.0);
                for (int w = 0; w < nw; ++w) {
                    unsigned long long zs = vmb[a][w];
                    while (zs) {
                        const int z = w * 64 + __ffsll((long long)zs) - 1;
                        zs &= zs - 1ull;
                        t += (double)gd.dSa[(o2 + (long long)b * n + z) * cin + c];
                    }
                }
            }
            t = wave_sum_d(t);
            if (lane == 0) g0[(o1 + a) * cin + c] = (float)(t + (va ? sdd3[c] : 0.0));
        }
}

// dp format for the nodes of degree 65..256 (their parameter partials and level-0 terms come from
// k_ccn2_bwd_node_big, which reads the raw dF): dp in place, row sums, trace
__global__ void __launch_bounds__(256) k_c2_dp_big(CcnPlanView v, const int* total_nodes, float* __restrict__ dF,
                                                   const float* __restrict__ F, int h, float* __restrict__ rdp_g,
                                                   float* __restrict__ trd_g) {
    const int i = blockIdx.x;
    if (i >= *total_nodes) return;
    const int n = v.deg[i];
    if (n <= C2_NCAP || n > CCN_BIGD) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long o2 = v.off2[i], o1 = v.off1[i];
    __shared__ float trp[4];
    for (int o = 0; o < h; ++o) {
        float tr = 0.f;
        for (int x = wv; x < n; x += 4) {
            float s = 0.f;
            for (int y = lane; y < n; y += 64) {
                const long long r = (o2 + (long long)x * n + y) * h + o;
                const float d = F[r] > 0.f ? dF[r] : 0.f;
                dF[r] = d;
                s += d;
                if (y == x) tr += d;
            }
            s = wave_total(s);
            if (lane == 0) rdp_g[(o1 + x) * h + o] = s;
        }
        tr = wave_total(tr);
        if (lane == 0) trp[wv] = tr;
        __syncthreads();
        if (threadIdx.x == 0) trd_g[(long long)i * h + o] = (trp[0] + trp[1]) + (trp[2] + trp[3]);
        __syncthreads();
    }
}

// k_c2_gather for degrees 65..256: lane w of row u in 64-lane chunks, the neighbours a with u in C_a
// in 64-wide ballot chunks (ascending), position maps read from global memory (L2-resident)
template <int H, int NB>
__global__ void __launch_bounds__(256) k_c2_gather_big(CcnPlanView v, const int* total_nodes, C2Dp g,
                                                       const float* __restrict__ W, int h,
                                                       const float* __restrict__ dsum, int dsum_ld, int dsum_off,
                                                       float* __restrict__ dout) {
    __shared__ unsigned long long vmask[CCN_BIGD][CCN_BW];
    __shared__ int s_i[CCN_BIGD], s_di[CCN_BIGD], s_oi[CCN_BIGD], s_o1[CCN_BIGD], s_aj[CCN_BIGD];
    __shared__ float wc[NWC][H][H];
    const int j = blockIdx.x;
    if (j >= *total_nodes) return;
    const int n = v.deg[j];
    if (n <= C2_NCAP || n > CCN_BIGD || h > H) return;
    const int nw = (n + 63) >> 6;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long o2 = v.off2[j];
    const int* sp = v.pos + o2;
    const int* nj = v.nbr + (long long)j * v.nmax;
    const int sj = v.selfpos[j];
    const int gr = v.graph[j];
    c2_dT_weights<H>(wc, W, h);
    for (int t = threadIdx.x; t < n; t += 256) {
        const int i = nj[t];
        s_i[t] = i;
        s_di[t] = v.deg[i];
        s_oi[t] = v.off2[i];
        s_o1[t] = v.off1[i];
        s_aj[t] = sp[(long long)t * n + sj];  // position of j in N(i_a)
    }
    for (int a = wv; a < n; a += 4)
        for (int w = 0; w < nw; ++w) {
            const int x = w * 64 + lane;
            const unsigned long long m = __ballot(x < n && sp[(long long)a * n + x] >= 0);
            if (lane == 0) vmask[a][w] = m;
        }
    __syncthreads();
    float rd[H];
#pragma unroll
    for (int c = 0; c < H; ++c) rd[c] = (dsum && c < h) ? dsum[(long long)gr * dsum_ld + dsum_off + c] : 0.f;
    for (int u = wv; u < n; u += 4) {
        for (int w0 = 0; w0 < n; w0 += 64) {
            const int wl = w0 + lane;
            float acc[H];
#pragma unroll
            for (int c = 0; c < H; ++c) acc[c] = 0.f;
            for (int a0 = 0; a0 < n; a0 += 64) {
                const int al = a0 + lane < n ? a0 + lane : 0;
                unsigned long long as = __ballot(a0 + lane < n && mbit(vmask[al], u));
                while (as) {
                    int aa[NB];
                    c2_take<NB>(as, aa);
                    float ld[NB][6][H];
                    int zb[NB], zz[NB];
                    bool vz[NB];
#pragma unroll
                    for (int q = 0; q < NB; ++q) {
                        const int a = aa[q] >= 0 ? a0 + aa[q] : 0;
                        vz[q] = aa[q] >= 0 && wl < n && mbit(vmask[a], wl);
                        zb[q] = max(sp[(long long)a * n + u], 0);
                        zz[q] = vz[q] ? sp[(long long)a * n + wl] : 0;
                        c2_dT_load<H>(g, h, s_oi[a], s_o1[a], s_i[a], s_di[a], s_aj[a], zb[q], zz[q], ld[q]);
                    }
#pragma unroll
                    for (int q = 0; q < NB; ++q) {
                        if (aa[q] < 0) break;
                        if (!vz[q]) continue;
                        const int a = a0 + aa[q];
                        c2_dT_add<H>(wc, ld[q], h, (float)s_di[a], s_aj[a], zb[q], zz[q], acc);
                    }
                }
            }
            if (wl < n)
#pragma unroll
                for (int c = 0; c < H; ++c) {
                    if (c >= h) break;
                    dout[(o2 + (long long)u * n + wl) * h + c] = acc[c] + rd[c];
                }
        }
    }
}

}  // namespace

int launch_c2_fwd_big(const CcnPlanView& v, const int* tot, int nodes, const float* fin, int level0, const float* X,
                      int cin, const float* W, const float* b, int h, const C2Save& sv, float* fout, float* nsum,
                      hipStream_t s) {
    return c2_big_select(cin, h, [&](auto t) -> int {
        using T = decltype(t);
        HGNN_KLAUNCH((k_ccn2_fwd_big<T::CM, T::HM>), ccn_grid1(nodes), dim3(256), 0, s, v, tot, fin, level0, X, cin,
                     W, b, h, sv, fout, nsum);
        HGNN_LAUNCH_CHECK();
        return HGNN_OK;
    });
}

int launch_c2_bwd_node_big(const CcnPlanView& v, const int* tot, int nodes, const float* dF, const float* F,
                           const C2Save& sv, int cin, const float* W, int h, const C2Grad& gd, float* ppart,
                           float* g0, hipStream_t s) {
    return c2_big_select(cin, h, [&](auto t) -> int {
        using T = decltype(t);
        HGNN_KLAUNCH((k_ccn2_bwd_node_big<T::CM, T::HM>), ccn_grid1(nodes), dim3(256), 0, s, v, tot, dF, F, sv, cin,
                     W, h, gd, ppart, g0);
        HGNN_LAUNCH_CHECK();
        return HGNN_OK;
    });
}

int launch_c2_dp_big(const CcnPlanView& v, const int* tot, int nodes, float* dF, const float* F, int h, float* rdp,
                     float* trd, hipStream_t s) {
    HGNN_KLAUNCH(k_c2_dp_big, ccn_grid1(nodes), dim3(256), 0, s, v, tot, dF, F, h, rdp, trd);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

int launch_c2_gather_big(const CcnPlanView& v, const int* tot, const C2Dp& g, const float* W, int h,
                         const float* dsum, int dsum_ld, int dsum_off, int nodes, float* dout, hipStream_t s) {
    return c2_gather_select<4>(h, [&](auto t) -> int {
        using T = decltype(t);
        HGNN_KLAUNCH((k_c2_gather_big<T::H, T::NB>), ccn_grid1(nodes), dim3(256), 0, s, v, tot, g, W, h, dsum,
                     dsum_ld, dsum_off, dout);
        HGNN_LAUNCH_CHECK();
        return HGNN_OK;
    });
}

}  // namespace hgnn
