// CCN-2D on the general path, receptive fields of degree <= 64: the level kernels k_c2_fwd / k_c2_bwd, the
// level-0 input gradient k_ccn2_dx0 and the gather k_c2_gather (ccn.hip's header comment has the math; the nodes
// of degree 65..256 are ccn2_big.hip's), with their launchers.
#include "ccn_general.h"

namespace hgnn {
namespace {

// CCN-2D layer, receptive fields of degree <= 64 (SBM-200: d ~ 20-60; QM9: d <= 6).
//
// Block per node i (n = d_i), one wave per receptive-field row b.  The wave walks the neighbours a
// with b in C_a (C_a = {x : p_a(x) >= 0}, the common neighbourhood N(i) n N(j_a), ascending) and
// loads the row segment t[z] = T[a][b][z] = F_{j_a}[p_a(b)][p_a(z)] (lane z, z in C_a: one
// coalesced piece of a row of F_{j_a}).  Every contraction statistic comes from that one load:
//   Sa[b][z] += t                         lane z; the wave owns row b of Sa
//   Sc[a][b]  = sum_z t                   wave total (DPP)           -> entry (a, b)
//   D1[a][b]  = t[b]                      lane b's value             -> entry (a, b)
//   D2[a][b]  = t[a]                      lane a's value (a in C_a)  -> entry (b, a), lane a here
//   q1[a]    += Sc[a][b] (W1-projected, per-wave LDS partials), d3 = sum_b t[b] at a == b
// The Linear of the 18 blocks (q0 = n Sc, q1, q2 = n Sa, q3, q4 = [x=y] tot, q5 = Sc,
// q6..14 = n Sc, q15 = D1, q16 = D2^T, q17 = [x=y] d3) is applied with combined weights
// (A = W0 + W6 + ... + W14: alpha = n A + W5 multiplies Sc) and assembled in LDS:
//   pre[x][y] = P[x][y] + W1 q1[x] + W3 q3[x] + [x = y](W4 tot + W17 d3) + bias,
// where P[x][y] receives at most two additions onto zero -- the row wave's part (n W2 Sa + W16 D2^T)
// and the column wave's (alpha Sc + W15 D1) -- so its value does not depend on their order.
// Nothing but F_out is written: the backward (k_c2_bwd) recomputes these sums instead of reading
// saved n^2 C arrays.  Level 0 (F_0[j] = X[j] tiled, utils_ccn.py:167-172): t = X[j_a] on C_a,
// Sc = m_a X[j_a], D1 = X[j_a], no gather and no reduction.
// Output channels are processed HC at a time (one pass each; h = 2 -- the reference's default --
// is one pass).  Dynamic LDS: P [ncap^2][HC] floats, then the position map [ncap^2] int16.
size_t c2_dyn_lds(int ncap, int hc_max) { return (size_t)ncap * ncap * (4 * hc_max + 2); }

// node prologue shared by k_c2_fwd / k_c2_bwd: position map (int16) and neighbour data in LDS,
// then the common-neighbourhood masks
template <int CM>
__device__ __forceinline__ void c2_prologue(const CcnPlanView& v, int i, int n, int level0, const float* __restrict__ X,
                                            int cin, short* sp, unsigned long long* vmask, int* s_oj, int* s_dj,
                                            float (*s_x)[CM]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int* ni = v.nbr + (long long)i * v.nmax;
    const long long o2 = v.off2[i];
    c2_copy_pos(v.pos + o2, n * n, sp);
    if ((int)threadIdx.x < n) {
        const int j = ni[threadIdx.x];
        s_oj[threadIdx.x] = v.off2[j];
        s_dj[threadIdx.x] = v.deg[j];
#pragma unroll
        for (int c = 0; c < CM; ++c) s_x[threadIdx.x][c] = (level0 && c < cin) ? X[(long long)j * cin + c] : 0.f;
    }
    __syncthreads();
    for (int a = wv; a < n; a += 4) {
        const unsigned long long m = __ballot(lane < n && sp[a * n + lane] >= 0);
        if (lane == 0) vmask[a] = m;
    }
    __syncthreads();
}

template <int CM, int HC, int NB, bool L0>
__global__ void __launch_bounds__(256) k_c2_fwd(CcnPlanView v, const int* total_nodes, const float* __restrict__ fin,
                                                const float* __restrict__ X, int cin, const float* __restrict__ W,
                                                const float* __restrict__ bias, int h, int ncap,
                                                float* __restrict__ fout, float* __restrict__ nsum) {
    extern __shared__ float c2_dyn[];
    __shared__ unsigned long long vmask[C2_NCAP];
    __shared__ int s_oj[C2_NCAP], s_dj[C2_NCAP];
    __shared__ float s_x[C2_NCAP][CM];
    __shared__ float wc[NWC][HC][CM];
    __shared__ float qw[4][C2_NCAP][HC];  // per-wave sums of W1 Sc[a][b] over the wave's rows b (W1 q1[a])
    __shared__ float q3p[C2_NCAP][HC];    // W3 q3[b]
    __shared__ float q3s[C2_NCAP][CM];    // q3[b] (tot = sum_b q3[b])
    __shared__ float d3s[C2_NCAP][CM];    // T[b][b][b]
    __shared__ float s_diag[HC];
    __shared__ float s_ns[4][HC];
    const int i = blockIdx.x;
    if (i >= *total_nodes) return;
    const int n = v.deg[i];
    if (n > C2_NCAP || n > ncap || cin > CM) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float* P = c2_dyn;
    short* sp = reinterpret_cast<short*>(c2_dyn + ncap * ncap * HC);
    c2_prologue<CM>(v, i, n, L0 ? 1 : 0, X, cin, sp, vmask, s_oj, s_dj, s_x);
    const long long o2 = v.off2[i];
    const float nf = (float)n;
    // lane a holds neighbour a's mask, row offset and degree (read by the walks with readlane)
    const bool la = lane < n;
    const unsigned long long my_mask = la ? vmask[lane] : 0ull;
    const int my_oj = la ? s_oj[lane] : 0, my_dj = la ? s_dj[lane] : 0;
    for (int o0 = 0; o0 < h; o0 += HC) {
        const int hc = min(HC, h - o0);
        c2_weights<HC, CM>(wc, W, cin, o0, hc);
        for (int e = threadIdx.x; e < n * n * HC; e += 256) P[e] = 0.f;
        __syncthreads();
        float vacc[HC];  // lane a: sum over this wave's rows b of W1 Sc[a][b]
#pragma unroll
        for (int o = 0; o < HC; ++o) vacc[o] = 0.f;
        if constexpr (L0) {
            // T = X[j_a] on C_a x C_a: every block of the Linear is a per-neighbour vector (lane a)
            //   Sc[a][b] = m_a X_a, D1[a][b] = X_a, D2[a][b] = [a in C_a] X_a (b in C_a),
            //   Sa[b][z] = sum_{a: b,z in C_a} X_a, q1[a] = m_a^2 X_a, q3[b] = sum_{a: b in C_a} m_a X_a,
            //   tot = sum_a m_a^2 X_a, d3 = sum_a [a in C_a] X_a
            const float mf = (float)__popcll(my_mask);
            const bool va = la && ((my_mask >> lane) & 1ull);
            float u[HC], dl[HC], bx[HC], q3a[HC];
#pragma unroll
            for (int o = 0; o < HC; ++o) {
                u[o] = dl[o] = bx[o] = q3a[o] = 0.f;
#pragma unroll
                for (int c = 0; c < CM; ++c) {
                    if (c >= cin) break;
                    const float x = la ? s_x[lane][c] : 0.f;
                    u[o] = fmaf(fmaf(fmaf(nf, wc[WA][o][c], wc[WB][o][c]), mf, wc[WQ15][o][c]), x, u[o]);
                    dl[o] = fmaf(wc[WQ16][o][c], x, dl[o]);
                    bx[o] = fmaf(nf * wc[WQ2][o][c], x, bx[o]);
                    vacc[o] = fmaf(wc[WQ1][o][c], x, vacc[o]);
                    q3a[o] = fmaf(wc[WQ3][o][c], x, q3a[o]);
                }
                dl[o] = va ? dl[o] : 0.f;
                vacc[o] *= mf * mf;  // W1 q1[a]
                q3a[o] *= mf;
            }
            if (wv == 0) {
                float dg[HC];
#pragma unroll
                for (int o = 0; o < HC; ++o) dg[o] = 0.f;
#pragma unroll
                for (int c = 0; c < CM; ++c) {
                    if (c >= cin) break;
                    const float x = la ? s_x[lane][c] : 0.f;
                    const float tt = wave_total(mf * mf * x), dd = wave_total(va ? x : 0.f);
#pragma unroll
                    for (int o = 0; o < HC; ++o) dg[o] = fmaf(wc[WQ4][o][c], tt, fmaf(wc[WQ17][o][c], dd, dg[o]));
                }
                if (lane < HC) {
#pragma unroll
                    for (int o = 0; o < HC; ++o)
                        if (lane == o) s_diag[o] = dg[o];
                }
            }
            for (int b = wv; b < n; b += 4) {
                const unsigned long long ab = __ballot(la && ((my_mask >> b) & 1ull));  // a with b in C_a
                const bool in = (ab >> lane) & 1ull;
                float s[HC];
#pragma unroll
                for (int o = 0; o < HC; ++o) {
                    if (in && o < hc) atomicAdd(&P[(lane * n + b) * HC + o], u[o]);  // entry (a, b): alpha Sc + W15 D1
                    s[o] = in ? dl[o] : 0.f;                                            // entry (b, a): W16 D2[a][b]
                    const float q = wave_total(in ? q3a[o] : 0.f);
                    if (lane == 0) q3p[b][o] = q;
                }
                unsigned long long as = ab;
                while (as) {
                    const int a = __ffsll((long long)as) - 1;
                    as &= as - 1ull;
                    const bool vz = (lane_value_u64(my_mask, a) >> lane) & 1ull;
#pragma unroll
                    for (int o = 0; o < HC; ++o) {
                        const float bxa = lane_value(bx[o], a);  // readlane outside any lane-dependent branch
                        s[o] += vz ? bxa : 0.f;                  // n W2 Sa[b][z]
                    }
                }
                if (la)
#pragma unroll
                    for (int o = 0; o < HC; ++o)
                        if (o < hc) atomicAdd(&P[(b * n + lane) * HC + o], s[o]);
            }
            if (wv != 0)
#pragma unroll
                for (int o = 0; o < HC; ++o) vacc[o] = 0.f;  // W1 q1[a] once (wave 0's copy)
        } else {
            for (int b = wv; b < n; b += 4) {
                // lane a (a in A_b) keeps Sc[a][b], D1[a][b] = T[a][b][b] and D2[a][b] = T[a][b][a]; the
                // projections through the weights follow once per row
                float sa[CM], sck[CM], d1k[CM], d2k[CM];
#pragma unroll
                for (int c = 0; c < CM; ++c) sa[c] = sck[c] = d1k[c] = d2k[c] = 0.f;
                if (lane == 0)
#pragma unroll
                    for (int c = 0; c < CM; ++c) d3s[b][c] = 0.f;
                const unsigned long long ab = __ballot(la && ((my_mask >> b) & 1ull));
                const bool in = (ab >> lane) & 1ull;
                const float* my_row = c2_row_of(fin, cin, sp, n, b, in, my_oj, my_dj);
                unsigned long long as = ab;
                while (as) {
                    int aa[NB];
                    c2_take<NB>(as, aa);
                    float t[NB][CM];
                    c2_load_rows<CM, NB>(cin, n, aa, sp, my_mask, my_row, t);
#pragma unroll
                    for (int u = 0; u < NB; ++u) {
                        const int a = aa[u];
                        if (a < 0) break;
                        const bool me = lane == a;
#pragma unroll
                        for (int c = 0; c < CM; ++c) {
                            if (c >= cin) break;
                            const float sc = wave_total(t[u][c]);
                            const float d1 = lane_value(t[u][c], b);
                            sck[c] = me ? sc : sck[c];
                            d1k[c] = me ? d1 : d1k[c];
                            d2k[c] = me ? t[u][c] : d2k[c];
                            sa[c] += t[u][c];
                        }
                        if (a == b && lane == b)
#pragma unroll
                            for (int c = 0; c < CM; ++c) d3s[b][c] = t[u][c];
                    }
                }
                // row b done: the column part of P[a][b] (lanes a in A_b), the row part of P[b][z], q3[b]
                float q3[CM];
#pragma unroll
                for (int c = 0; c < CM; ++c) q3[c] = c < cin ? wave_total(sa[c]) : 0.f;
#pragma unroll
                for (int o = 0; o < HC; ++o) {
                    if (o >= hc) break;
                    float U = 0.f, V = 0.f, S = 0.f;
#pragma unroll
                    for (int c = 0; c < CM; ++c) {
                        if (c >= cin) break;
                        U = fmaf(fmaf(nf, wc[WA][o][c], wc[WB][o][c]), sck[c], U);
                        U = fmaf(wc[WQ15][o][c], d1k[c], U);
                        V = fmaf(wc[WQ1][o][c], sck[c], V);
                        S = fmaf(nf * wc[WQ2][o][c], sa[c], S);
                        S = fmaf(wc[WQ16][o][c], d2k[c], S);  // entry (b, a): W16 D2[a][b], lane a
                    }
                    if (in) atomicAdd(&P[(lane * n + b) * HC + o], U);  // entry (a, b): alpha Sc + W15 D1
                    vacc[o] += in ? V : 0.f;                            // q1[a]
                    if (la) atomicAdd(&P[(b * n + lane) * HC + o], S);
                    if (lane == 0) {
                        float q = 0.f;
#pragma unroll
                        for (int c = 0; c < CM; ++c) q = fmaf(wc[WQ3][o][c], q3[c], q);
                        q3p[b][o] = q;
                    }
                }
                if (lane == 0)
#pragma unroll
                    for (int c = 0; c < CM; ++c) q3s[b][c] = q3[c];
            }
            __syncthreads();
            if ((int)threadIdx.x < hc) {  // [x = y](W4 tot + W17 d3), sums over b in a fixed order
                const int o = threadIdx.x;
                float dg = 0.f;
                for (int c = 0; c < cin; ++c) {
                    float tt = 0.f, dd = 0.f;
                    for (int b = 0; b < n; ++b) {
                        tt += q3s[b][c];
                        dd += d3s[b][c];
                    }
                    dg = fmaf(wc[WQ4][o][c], tt, dg);
                    dg = fmaf(wc[WQ17][o][c], dd, dg);
                }
                s_diag[o] = dg;
            }
        }
        if (la)
#pragma unroll
            for (int o = 0; o < HC; ++o) qw[wv][lane][o] = vacc[o];
        __syncthreads();
        float ns[HC];  // this node's sum of F_out (the readout's per-level feature, model_ccn.py:102)
#pragma unroll
        for (int o = 0; o < HC; ++o) ns[o] = 0.f;
        for (int e = threadIdx.x; e < n * n; e += 256) {
            const int x = e / n, y = e - x * n;
#pragma unroll
            for (int o = 0; o < HC; ++o) {
                if (o >= hc) break;
                float s = bias[o0 + o] + P[e * HC + o];
                s += (qw[0][x][o] + qw[1][x][o]) + (qw[2][x][o] + qw[3][x][o]);
                s += q3p[x][o];
                if (x == y) s += s_diag[o];
                s = s < 0.f ? 0.f : s;
                fout[(o2 + e) * h + o0 + o] = s;
                ns[o] += s;
            }
        }
#pragma unroll
        for (int o = 0; o < HC; ++o) {
            const float t = wave_total(ns[o]);
            if (lane == 0) s_ns[wv][o] = t;
        }
        __syncthreads();
        if ((int)threadIdx.x < hc)
            nsum[(long long)i * h + o0 + threadIdx.x] =
                (s_ns[0][threadIdx.x] + s_ns[1][threadIdx.x]) + (s_ns[2][threadIdx.x] + s_ns[3][threadIdx.x]);
        __syncthreads();
    }
}

// dX[j] (level 0) = sum over neighbours i of G_i[a_j] (k_ccn2_bwd_node) + d_j^2 dsum0.
__global__ void __launch_bounds__(256) k_ccn2_dx0(CcnPlanView v, const int* total_nodes, const float* __restrict__ g0,
                                                  int cin, const float* __restrict__ dsum, int dsum_ld,
                                                  float* __restrict__ dout) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= *total_nodes) return;
    const int n = v.deg[j];
    if (n > CCN_BIGD) return;
    const long long o2 = v.off2[j];
    const int* nj = v.nbr + (long long)j * v.nmax;
    const int sj = v.selfpos[j];
    const int g = v.graph[j];
    float t[C2_CMAX_WIDE];
#pragma unroll
    for (int c = 0; c < C2_CMAX_WIDE; ++c) t[c] = 0.f;
    for (int x = lane; x < n; x += 64) {  // one chunk for d <= 64; the indices once for every channel
        const int i = nj[x];
        const int aj = v.pos[o2 + (long long)x * n + sj];  // position of j in N(i)
        const float* gi = g0 + ((long long)v.off1[i] + aj) * cin;
#pragma unroll
        for (int c = 0; c < C2_CMAX_WIDE; ++c)
            if (c < cin) t[c] += gi[c];
    }
#pragma unroll
    for (int c = 0; c < C2_CMAX_WIDE; ++c) {
        if (c >= cin) break;
        const float s = wave_sum(t[c]);
        if (lane == 0) {
            const float rd = dsum ? dsum[(long long)g * dsum_ld + c] : 0.f;
            dout[(long long)j * cin + c] = s + (float)(n * n) * rd;
        }
    }
}

// Backward of one CCN-2D level for the nodes of degree <= 64, block per node i:
//   dp = dF * relu'(F_out) (written back in place of dF; dF of the top level read straight from the readout's
//   per-graph slice dtop when given), rdp[x] = sum_y dp[x][y], tr = sum_x dp[x][x]
//   -- the "dp format" the gather kernels rebuild dT from (k_c2_gather);
//   parameter partials  dW_q[o][c] = sum_xy dp[x][y][o] block_q[x][y][c], db[o] = sum dp, with
//     P0 = sum dp Sc, P1 = sum_x rdp[x] q1[x], P2 = sum dp Sa, P3 = sum_x rdp[x] q3[x],
//     P15 = sum dp D1, P16 = sum dp[x][y] D2[y][x], tot, d3:
//     dW_{0,6..14} = n P0, dW_5 = P0, dW_1 = P1, dW_2 = n P2, dW_3 = P3, dW_4 = tr tot, dW_15 = P15,
//     dW_16 = P16, dW_17 = tr d3.
// Level >= 1: the forward's row walk again (same loads), every sum lane-level (dp[a][b] . t summed
// over the walk, wave totals once at the end).  Level 0 (T = X[j_a] on C_a) in closed form from the
// per-neighbour masked sums R1[a] = sum_{b in C_a} dp[a][b], R2[a] = sum_{b in C_a} dp[b][a],
// R3[a] = sum_{b in C_a} rdp[b], BS[a] = sum_{b,z in C_a} dp[b][z], which also give dX's per-node
// terms  G[a] = sum_{b,z in C_a} dT[a][b][z]  (k_ccn2_dx0 adds them up per input node).
template <int CM, int HC, int NB, bool L0>
__global__ void __launch_bounds__(256) k_c2_bwd(CcnPlanView v, const int* total_nodes, float* __restrict__ dF,
                                                const float* __restrict__ dtop, int dtop_ld,
                                                const float* __restrict__ F, const float* __restrict__ fin,
                                                const float* __restrict__ X, int cin,
                                                const float* __restrict__ W, int h, int ncap,
                                                float* __restrict__ rdp_g, float* __restrict__ trd_g,
                                                float* __restrict__ ppart, float* __restrict__ g0) {
    extern __shared__ float c2_dyn[];
    __shared__ unsigned long long vmask[C2_NCAP];
    __shared__ int s_oj[C2_NCAP], s_dj[C2_NCAP];
    __shared__ float s_x[C2_NCAP][CM];
    __shared__ float wc[NWC][HC][CM];
    __shared__ float rdpL[C2_NCAP][HC];
    __shared__ float trL[HC];
    __shared__ float red[4][C2_NACC][HC][CM];
    __shared__ float redt[4][2][CM];  // tot, d3
    __shared__ float redb[4][HC];
    __shared__ float gs[C2_NCAP][CM];
    __shared__ float rs[C2_NCAP][4][HC];  // level 0: R1, R2, R3, BS per neighbour
    const int i = blockIdx.x;
    if (i >= *total_nodes) return;
    const int n = v.deg[i];
    if (n > C2_NCAP || n > ncap || cin > CM) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float* dpL = c2_dyn;
    short* sp = reinterpret_cast<short*>(c2_dyn + ncap * ncap * HC);
    c2_prologue<CM>(v, i, n, L0 ? 1 : 0, X, cin, sp, vmask, s_oj, s_dj, s_x);
    const long long o2 = v.off2[i], o1 = v.off1[i];
    const int gi = v.graph[i];
    const bool la = lane < n;
    const unsigned long long my_mask = la ? vmask[lane] : 0ull;
    const int my_oj = la ? s_oj[lane] : 0, my_dj = la ? s_dj[lane] : 0;
    const float nf = (float)n;
    const int K = 18 * cin;
    float* pp = ppart + (long long)i * (h * K + h);
    for (int e = threadIdx.x; e < C2_NCAP * CM; e += 256) (&gs[0][0])[e] = 0.f;
    for (int o0 = 0; o0 < h; o0 += HC) {
        const int hc = min(HC, h - o0);
        c2_weights<HC, CM>(wc, W, cin, o0, hc);
        float sb[HC];
#pragma unroll
        for (int o = 0; o < HC; ++o) sb[o] = 0.f;
        for (int e = threadIdx.x; e < n * n; e += 256) {
#pragma unroll
            for (int o = 0; o < HC; ++o) {
                float d = 0.f;
                if (o < hc) {
                    const long long r = (o2 + e) * h + o0 + o;
                    d = F[r] > 0.f ? (dtop ? dtop[(long long)gi * dtop_ld + o0 + o] : dF[r]) : 0.f;
                    dF[r] = d;
                }
                dpL[e * HC + o] = d;
                sb[o] += d;
            }
        }
#pragma unroll
        for (int o = 0; o < HC; ++o) {
            const float t = wave_total(sb[o]);
            if (lane == 0) redb[wv][o] = t;
        }
        __syncthreads();
        // row sums and trace of dp
        for (int x = wv; x < n; x += 4)
#pragma unroll
            for (int o = 0; o < HC; ++o) {
                const float r = wave_total(lane < n ? dpL[(x * n + lane) * HC + o] : 0.f);
                if (lane == 0) {
                    rdpL[x][o] = r;
                    if (o < hc) rdp_g[(o1 + x) * h + o0 + o] = r;
                }
            }
        if (wv == 0)
#pragma unroll
            for (int o = 0; o < HC; ++o) {
                const float r = wave_total(lane < n ? dpL[(lane * n + lane) * HC + o] : 0.f);
                if (lane == 0) {
                    trL[o] = r;
                    if (o < hc) trd_g[(long long)i * h + o0 + o] = r;
                }
            }
        __syncthreads();
        if constexpr (L0) {
            // per neighbour a (wave per a): the masked sums of dp the closed forms need
            for (int a = wv; a < n; a += 4) {
                const unsigned long long ma = vmask[a];
                const bool vb = lane < n && ((ma >> lane) & 1ull);
#pragma unroll
                for (int o = 0; o < HC; ++o) {
                    const float r1 = wave_total(vb ? dpL[(a * n + lane) * HC + o] : 0.f);
                    const float r2 = wave_total(vb ? dpL[(lane * n + a) * HC + o] : 0.f);
                    const float r3 = wave_total(vb ? rdpL[lane][o] : 0.f);
                    float s = 0.f;
                    unsigned long long zs = ma;
                    while (zs) {
                        const int z = __ffsll((long long)zs) - 1;
                        zs &= zs - 1ull;
                        s += vb ? dpL[(lane * n + z) * HC + o] : 0.f;
                    }
                    const float bs = wave_total(s);
                    if (lane == 0) {
                        rs[a][0][o] = r1;
                        rs[a][1][o] = r2;
                        rs[a][2][o] = r3;
                        rs[a][3][o] = bs;
                    }
                }
            }
            __syncthreads();
            // parameter partials: (o, c) pairs over the waves, lanes over the neighbours a, wave totals
            for (int p = wv; p < hc * cin; p += 4) {
                const int o = p / cin, c = p % cin;
                const float mf = (float)__popcll(my_mask);
                const bool va = la && ((my_mask >> lane) & 1ull);
                const float x = la ? s_x[lane][c] : 0.f;
                const float r1 = la ? rs[lane][0][o] : 0.f, r2 = la ? rs[lane][1][o] : 0.f;
                const float r3 = la ? rs[lane][2][o] : 0.f, bs = la ? rs[lane][3][o] : 0.f;
                const float ra = la ? rdpL[lane][o] : 0.f;
                const float s0 = wave_total(mf * x * r1), s1 = wave_total(mf * mf * x * ra);
                const float s2 = wave_total(x * bs), s3 = wave_total(mf * x * r3);
                const float s15 = wave_total(x * r1), s16 = wave_total(va ? x * r2 : 0.f);
                const float tt = wave_total(mf * mf * x), dd = wave_total(va ? x : 0.f);
                if (lane == 0)
                    c2_write_partials(pp + (long long)(o0 + o) * K, cin, c, nf, s0, s1, s2, s3, s15, s16, trL[o] * tt,
                                      trL[o] * dd);
            }
            // G[a] = m_a sum dSc[a][.] + sum dSa + sum dD1[a][.] + [a in C_a](sum dD2[a][.] + dd3), this chunk's o
            for (int t = threadIdx.x; t < n * cin; t += 256) {
                const int a = t / cin, c = t % cin;
                const unsigned long long ma = vmask[a];
                const float mf = (float)__popcll(ma);
                const bool va = (ma >> a) & 1ull;
                float g = 0.f;
                for (int o = 0; o < hc; ++o) {
                    const float r1 = rs[a][0][o], r2 = rs[a][1][o], r3 = rs[a][2][o], bs = rs[a][3][o];
                    float s = mf * fmaf(fmaf(nf, wc[WA][o][c], wc[WB][o][c]), r1, mf * wc[WQ1][o][c] * rdpL[a][o]);
                    s = fmaf(nf * wc[WQ2][o][c], bs, s);
                    s = fmaf(mf * wc[WQ3][o][c], r3, s);
                    s = fmaf(mf * mf * wc[WQ4][o][c], trL[o], s);
                    s = fmaf(wc[WQ15][o][c], r1, s);
                    if (va) s = fmaf(wc[WQ16][o][c], r2, fmaf(wc[WQ17][o][c], trL[o], s));
                    g += s;
                }
                gs[a][c] += g;
            }
        } else {
            float acc[C2_NACC][HC][CM], tot[CM], d3[CM];
#pragma unroll
            for (int k = 0; k < C2_NACC; ++k)
#pragma unroll
                for (int o = 0; o < HC; ++o)
#pragma unroll
                    for (int c = 0; c < CM; ++c) acc[k][o][c] = 0.f;
#pragma unroll
            for (int c = 0; c < CM; ++c) tot[c] = d3[c] = 0.f;
            for (int b = wv; b < n; b += 4) {
                float sa[CM];
#pragma unroll
                for (int c = 0; c < CM; ++c) sa[c] = 0.f;
                unsigned long long as = __ballot(la && ((my_mask >> b) & 1ull));
                const float* my_row = c2_row_of(fin, cin, sp, n, b, (as >> lane) & 1ull, my_oj, my_dj);
                // lane a: dp[a][b], dp[b][a], rdp[a] of this row (read once, then by readlane)
                float my_ab[HC], my_ba[HC], my_ra[HC];
#pragma unroll
                for (int o = 0; o < HC; ++o) {
                    my_ab[o] = la ? dpL[(lane * n + b) * HC + o] : 0.f;
                    my_ba[o] = la ? dpL[(b * n + lane) * HC + o] : 0.f;
                    my_ra[o] = la ? rdpL[lane][o] : 0.f;
                }
                while (as) {
                    int aa[NB];
                    c2_take<NB>(as, aa);
                    float t[NB][CM];
                    c2_load_rows<CM, NB>(cin, n, aa, sp, my_mask, my_row, t);
#pragma unroll
                    for (int u = 0; u < NB; ++u) {
                        const int a = aa[u];
                        if (a < 0) break;
#pragma unroll
                        for (int o = 0; o < HC; ++o) {
                            const float dab = lane_value(my_ab[o], a), dba = lane_value(my_ba[o], a);
                            const float ra = lane_value(my_ra[o], a);
                            const float d15 = lane == b ? dab : 0.f, d16 = lane == a ? dba : 0.f;
#pragma unroll
                            for (int c = 0; c < CM; ++c) {
                                acc[0][o][c] = fmaf(dab, t[u][c], acc[0][o][c]);
                                acc[1][o][c] = fmaf(ra, t[u][c], acc[1][o][c]);
                                acc[4][o][c] = fmaf(d15, t[u][c], acc[4][o][c]);
                                acc[5][o][c] = fmaf(d16, t[u][c], acc[5][o][c]);
                            }
                        }
                        if (a == b && lane == b)
#pragma unroll
                            for (int c = 0; c < CM; ++c) d3[c] += t[u][c];
#pragma unroll
                        for (int c = 0; c < CM; ++c) sa[c] += t[u][c];
                    }
                }
#pragma unroll
                for (int o = 0; o < HC; ++o) {
                    const float dbz = lane < n ? dpL[(b * n + lane) * HC + o] : 0.f;
#pragma unroll
                    for (int c = 0; c < CM; ++c) acc[2][o][c] = fmaf(dbz, sa[c], acc[2][o][c]);
                }
#pragma unroll
                for (int c = 0; c < CM; ++c) {
                    if (c >= cin) break;
                    const float q3 = wave_total(sa[c]);  // uniform: P3 and tot kept in lane 0 only
                    if (lane == 0) {
#pragma unroll
                        for (int o = 0; o < HC; ++o) acc[3][o][c] = fmaf(rdpL[b][o], q3, acc[3][o][c]);
                        tot[c] += q3;
                    }
                }
            }
            // lane-level sums -> wave totals (P3 and tot are lane 0's)
#pragma unroll
            for (int k = 0; k < C2_NACC; ++k) {
                if (k == 3) continue;
#pragma unroll
                for (int o = 0; o < HC; ++o)
#pragma unroll
                    for (int c = 0; c < CM; ++c) {
                        if (c >= cin) break;
                        acc[k][o][c] = wave_total(acc[k][o][c]);
                    }
            }
#pragma unroll
            for (int c = 0; c < CM; ++c) {
                if (c >= cin) break;
                d3[c] = wave_total(d3[c]);
            }
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < C2_NACC; ++k)
#pragma unroll
                    for (int o = 0; o < HC; ++o)
#pragma unroll
                        for (int c = 0; c < CM; ++c) red[wv][k][o][c] = acc[k][o][c];
#pragma unroll
                for (int c = 0; c < CM; ++c) {
                    redt[wv][0][c] = tot[c];
                    redt[wv][1][c] = d3[c];
                }
            }
            __syncthreads();
            for (int t = threadIdx.x; t < hc * cin; t += 256) {
                const int o = t / cin, c = t % cin;
                float s[C2_NACC];
#pragma unroll
                for (int k = 0; k < C2_NACC; ++k)
                    s[k] = (red[0][k][o][c] + red[1][k][o][c]) + (red[2][k][o][c] + red[3][k][o][c]);
                const float tt = (redt[0][0][c] + redt[1][0][c]) + (redt[2][0][c] + redt[3][0][c]);
                const float dd = (redt[0][1][c] + redt[1][1][c]) + (redt[2][1][c] + redt[3][1][c]);
                c2_write_partials(pp + (long long)(o0 + o) * K, cin, c, nf, s[0], s[1], s[2], s[3], s[4], s[5],
                                  trL[o] * tt, trL[o] * dd);
            }
        }
        if ((int)threadIdx.x < hc)
            pp[(long long)h * K + o0 + threadIdx.x] = (redb[0][threadIdx.x] + redb[1][threadIdx.x]) +
                                                      (redb[2][threadIdx.x] + redb[3][threadIdx.x]);
        __syncthreads();
    }
    if (L0 && g0) {
        __syncthreads();
        for (int t = threadIdx.x; t < n * cin; t += 256) g0[(o1 + t / cin) * cin + t % cin] = gs[t / cin][t % cin];
    }
}

// The gather of a level's input gradient from the dp format (ccn_general.h: c2_dT_weights / _load / _add)
template <int H, int NB>
__global__ void __launch_bounds__(256) k_c2_gather(CcnPlanView v, const int* total_nodes, C2Dp g,
                                                   const float* __restrict__ W, int h, const float* __restrict__ dsum,
                                                   int dsum_ld, int dsum_off, float* __restrict__ dout) {
    __shared__ short sp[C2_NCAP * C2_NCAP];
    __shared__ unsigned long long vmask[C2_NCAP];
    __shared__ int s_i[C2_NCAP], s_di[C2_NCAP], s_oi[C2_NCAP], s_o1[C2_NCAP], s_aj[C2_NCAP];
    __shared__ float wc[NWC][H][H];
    const int j = blockIdx.x;
    if (j >= *total_nodes) return;
    const int n = v.deg[j];
    if (n > C2_NCAP || h > H) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long o2 = v.off2[j];
    const int* nj = v.nbr + (long long)j * v.nmax;
    const int sj = v.selfpos[j];
    const int gr = v.graph[j];
    c2_dT_weights<H>(wc, W, h);
    c2_copy_pos(v.pos + o2, n * n, sp);
    if ((int)threadIdx.x < n) {
        const int i = nj[threadIdx.x];
        s_i[threadIdx.x] = i;
        s_di[threadIdx.x] = v.deg[i];
        s_oi[threadIdx.x] = v.off2[i];
        s_o1[threadIdx.x] = v.off1[i];
    }
    __syncthreads();
    for (int a = wv; a < n; a += 4) {
        const unsigned long long m = __ballot(lane < n && sp[a * n + lane] >= 0);
        if (lane == 0) {
            vmask[a] = m;
            s_aj[a] = sp[a * n + sj];  // position of j in N(i_a)
        }
    }
    __syncthreads();
    float rd[H];
#pragma unroll
    for (int c = 0; c < H; ++c) rd[c] = (dsum && c < h) ? dsum[(long long)gr * dsum_ld + dsum_off + c] : 0.f;
    // lane a holds neighbour i_a's mask, node, degree, offsets, the position aj of j in N(i_a), and the
    // row-independent parts of its dp format (rdp_i[aj], tr_i)
    const bool la = lane < n;
    const unsigned long long my_mask = la ? vmask[lane] : 0ull;
    const int my_i = la ? s_i[lane] : 0, my_di = la ? s_di[lane] : 0, my_oi = la ? s_oi[lane] : 0;
    const int my_o1 = la ? s_o1[lane] : 0, my_aj = la ? s_aj[lane] : 0;
    float my_ra[H], my_tr[H];
#pragma unroll
    for (int o = 0; o < H; ++o) {
        my_ra[o] = (la && o < h) ? g.rdp[((long long)my_o1 + my_aj) * h + o] : 0.f;
        my_tr[o] = (la && o < h) ? g.trd[(long long)my_i * h + o] : 0.f;
    }
    for (int u = wv; u < n; u += 4) {
        float acc[H];
#pragma unroll
        for (int c = 0; c < H; ++c) acc[c] = 0.f;
        // lanes a with u in C_a: b = p_a(u), and every part of dT_i[aj][b][.] that does not depend on z,
        // projected through the weights once per row:
        //   base = (n_i A + W5)^T dp[aj][b] + W1^T rdp[aj] + W3^T rdp[b] + W4^T tr,
        //   e1 = W15^T dp[aj][b] (z = b), e2 = W16^T dp[b][aj] (z = aj), e3 = W17^T tr (aj = b = z);
        // the walk then adds n_i W2^T dp[b][z] per lane
        const unsigned long long au = __ballot(la && ((my_mask >> u) & 1ull));
        const bool in = (au >> lane) & 1ull;
        const int my_b = in ? (int)sp[lane * n + u] : 0;
        const float nfi = (float)my_di;
        float base[H], e1[H], e2[H], e3[H];
        {
            const float* pab = g.dp + ((long long)my_oi + (long long)my_aj * my_di + my_b) * h;
            const float* pba = g.dp + ((long long)my_oi + (long long)my_b * my_di + my_aj) * h;
            const float* prb = g.rdp + ((long long)my_o1 + my_b) * h;
            float vab[H], vba[H], vrb[H];
#pragma unroll
            for (int o = 0; o < H; ++o) {
                vab[o] = (in && o < h) ? pab[o] : 0.f;
                vba[o] = (in && o < h) ? pba[o] : 0.f;
                vrb[o] = (in && o < h) ? prb[o] : 0.f;
            }
#pragma unroll
            for (int c = 0; c < H; ++c) {
                float b0 = 0.f, x1 = 0.f, x2 = 0.f, x3 = 0.f;
#pragma unroll
                for (int o = 0; o < H; ++o) {
                    if (o >= h) break;
                    b0 = fmaf(fmaf(nfi, wc[WA][o][c], wc[WB][o][c]), vab[o], b0);
                    b0 = fmaf(wc[WQ1][o][c], my_ra[o], b0);
                    b0 = fmaf(wc[WQ3][o][c], vrb[o], b0);
                    b0 = fmaf(wc[WQ4][o][c], my_tr[o], b0);
                    x1 = fmaf(wc[WQ15][o][c], vab[o], x1);
                    x2 = fmaf(wc[WQ16][o][c], vba[o], x2);
                    x3 = fmaf(wc[WQ17][o][c], my_tr[o], x3);
                }
                base[c] = b0;
                e1[c] = x1;
                e2[c] = x2;
                e3[c] = x3;
            }
        }
        const float* my_row = g.dp + ((long long)my_oi + (long long)my_b * my_di) * h;  // row b of dp_i
        // the neighbours a with u in C_a, ascending, NB at a time: one row piece dp_i[b][z] per lane each
        unsigned long long as = au;
        while (as) {
            int aa[NB];
            c2_take<NB>(as, aa);
            float dz[NB][H];
            int zz[NB];
            bool vz[NB];
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const int a = aa[q] >= 0 ? aa[q] : 0;
                vz[q] = aa[q] >= 0 && ((lane_value_u64(my_mask, a) >> lane) & 1ull);
                zz[q] = vz[q] ? (int)sp[a * n + lane] : 0;
                const float* pz = lane_value_ptr(my_row, a) + zz[q] * h;
#pragma unroll
                for (int o = 0; o < H; ++o) dz[q][o] = o < h ? pz[o] : 0.f;
            }
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const int a = aa[q];
                if (a < 0) break;
                const int b = lane_value_i(my_b, a), aj = lane_value_i(my_aj, a);
                const float nfa = lane_value(nfi, a);
                const bool f1 = zz[q] == b, f2 = zz[q] == aj, f3 = f1 && aj == b;
#pragma unroll
                for (int c = 0; c < H; ++c) {
                    if (c >= h) break;
                    float w2 = 0.f;
#pragma unroll
                    for (int o = 0; o < H; ++o) {
                        if (o >= h) break;
                        w2 = fmaf(wc[WQ2][o][c], dz[q][o], w2);
                    }
                    const float x1 = lane_value(e1[c], a), x2 = lane_value(e2[c], a), x3 = lane_value(e3[c], a);
                    float t = fmaf(nfa, w2, lane_value(base[c], a));
                    t += f1 ? x1 : 0.f;
                    t += f2 ? x2 : 0.f;
                    t += f3 ? x3 : 0.f;
                    acc[c] += vz[q] ? t : 0.f;
                }
            }
        }
        if (lane < n)
#pragma unroll
            for (int c = 0; c < H; ++c) {
                if (c >= h) break;
                dout[(o2 + (long long)u * n + lane) * h + c] = acc[c] + rd[c];
            }
    }
}

// The kernels above take the receptive-field bound ncap = min(max degree, 64) for their
// dynamic LDS (P or dp [ncap^2][HC] fp32 + the int16 position map): 40 KB at ncap = 64.
int c2_ncap(long long dmax) { return dmax < C2_NCAP ? (int)(dmax > 1 ? dmax : 1) : C2_NCAP; }

}  // namespace

int launch_c2_fwd(const CcnPlanView& v, const int* tot, const float* fin, int level0, const float* X, int cin,
                  const float* W, const float* b, int h, long long dmax, int nodes, float* fout, float* nsum,
                  hipStream_t s) {
    const int ncap = c2_ncap(dmax);
    return c2_select<false>(level0, cin, [&](auto t) -> int {
        using T = decltype(t);
        HGNN_KLAUNCH((k_c2_fwd<T::CM, T::HC, T::NB, T::L0>), ccn_grid1(nodes), dim3(256), c2_dyn_lds(ncap, T::HC), s,
                     v, tot, fin, X, cin, W, b, h, ncap, fout, nsum);
        HGNN_LAUNCH_CHECK();
        return HGNN_OK;
    });
}

int launch_c2_bwd(const CcnPlanView& v, const int* tot, float* dF, const float* dtop, int dtop_ld, const float* F,
                  const float* fin, int level0, const float* X, int cin, const float* W, int h, long long dmax,
                  int nodes, float* rdp, float* trd, float* ppart, float* g0, hipStream_t s) {
    const int ncap = c2_ncap(dmax);
    return c2_select<true>(level0, cin, [&](auto t) -> int {
        using T = decltype(t);
        HGNN_KLAUNCH((k_c2_bwd<T::CM, T::HC, T::NB, T::L0>), ccn_grid1(nodes), dim3(256), c2_dyn_lds(ncap, T::HC), s,
                     v, tot, dF, dtop, dtop_ld, F, fin, X, cin, W, h, ncap, rdp, trd, ppart, g0);
        HGNN_LAUNCH_CHECK();
        return HGNN_OK;
    });
}

int launch_c2_dx0(const CcnPlanView& v, const int* tot, int nodes, const float* g0, int cin, const float* dsum,
                  int dsum_ld, float* dout, hipStream_t s) {
    HGNN_KLAUNCH(k_ccn2_dx0, ccn_grid4(nodes), dim3(256), 0, s, v, tot, g0, cin, dsum, dsum_ld, dout);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

int launch_c2_gather(const CcnPlanView& v, const int* tot, const C2Dp& g, const float* W, int h, const float* dsum,
                     int dsum_ld, int dsum_off, int nodes, float* dout, hipStream_t s) {
    return c2_gather_select<8>(h, [&](auto t) -> int {
        using T = decltype(t);
        HGNN_KLAUNCH((k_c2_gather<T::H, T::NB>), ccn_grid1(nodes), dim3(256), 0, s, v, tot, g, W, h, dsum, dsum_ld,
                     dsum_off, dout);
        HGNN_LAUNCH_CHECK();
        return HGNN_OK;
    });
}

}  // namespace hgnn
