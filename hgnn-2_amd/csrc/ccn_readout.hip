// What both orders of the general CCN path share around their levels: the readout and its backward, the reduction
// of the per-node parameter partials, the top level's broadcast, the pack of X / unpack of dX, and the general
// collapse6to3 with its two entry points of include/hgnn_amd.h.
#include "ccn_general.h"

namespace hgnn {
namespace {

// Two stages so a graph's rows (Σd² of them per level on SBM-200: 261 K) are summed by many blocks:
// part[b][k][col] over row chunk k of graph b (fp64, fixed order), then one block per graph adds
// the chunks and applies fc.  Chunks per graph (gridDim.y of the first stage) from the rows per graph:
// up to RO_CH for SBM-200-size levels, one for QM9-size graphs (a few hundred rows).
int ro_chunks(long long rows, int bs) {
    const long long per = bs > 0 ? rows / bs : rows;
    const long long c = per / 4096 + 1;
    return (int)(c < RO_CH ? c : RO_CH);
}

__global__ void __launch_bounds__(256) k_ccn_readout_part(ReadoutArgs r, double* __restrict__ part) {
    __shared__ double red[4][C2_CMAX];
    const int b = blockIdx.x, k = blockIdx.y;
    const int n0 = r.v.node_off[b], n1 = r.v.node_off[b + 1];
    const int* off = r.order == 1 ? r.v.off1 : r.v.off2;
    const int nf = r.f + r.L * r.h;
    const int nch = gridDim.y;
    double* pb = part + ((long long)b * nch + k) * nf;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    auto flush = [&](double (&acc)[C2_CMAX], int nc, int col0) {
        for (int c = 0; c < nc; ++c) {
            const double t = wave_sum_d(acc[c]);
            if (lane == 0) red[wv][c] = t;
        }
        __syncthreads();
        if ((int)threadIdx.x < nc)
            pb[col0 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] +
                                     red[3][threadIdx.x];
        __syncthreads();
    };
    // level 0: sum_i d_i^order X[i]  (utils_ccn.py:212-216 / 167-172 tile X[i] d_i or d_i^2 times)
    for (int c0 = 0; c0 < r.f; c0 += C2_CMAX) {
        const int nc = min(C2_CMAX, r.f - c0);
        double acc[C2_CMAX];
        for (int c = 0; c < C2_CMAX; ++c) acc[c] = 0.0;
        const int len = n1 - n0, per = (len + nch - 1) / nch;
        const int i0 = n0 + k * per, i1 = min(n1, i0 + per);
        for (int i = i0 + (int)threadIdx.x; i < i1; i += 256) {
            const double d = r.v.deg[i];
            const double wgt = r.order == 1 ? d : d * d;
            for (int c = 0; c < nc; ++c) acc[c] += wgt * (double)r.X[(long long)i * r.f + c0 + c];
        }
        flush(acc, nc, c0);
    }
    for (int l = 0; l < r.L; ++l) {
        const long long r0 = r.per_node ? n0 : off[n0], r1 = r.per_node ? n1 : off[n1];
        const long long len = r1 - r0, per = (len + nch - 1) / nch;
        const long long q0 = r0 + k * per, q1 = min(r1, q0 + per);
        for (int c0 = 0; c0 < r.h; c0 += C2_CMAX) {
            const int nc = min(C2_CMAX, r.h - c0);
            double acc[C2_CMAX];
            for (int c = 0; c < C2_CMAX; ++c) acc[c] = 0.0;
            for (long long q = q0 + threadIdx.x; q < q1; q += 256)
                for (int c = 0; c < nc; ++c) acc[c] += (double)r.F[l][q * r.h + c0 + c];
            flush(acc, nc, r.f + l * r.h + c0);
        }
    }
}

__global__ void __launch_bounds__(256) k_ccn_readout(ReadoutArgs r, const double* __restrict__ part) {
    __shared__ double red[4];
    const int b = blockIdx.x;
    const int nf = r.f + r.L * r.h;
    float* feat = r.feat + (long long)b * nf;
    auto bsum = [&](double x) {
        x = wave_sum_d(x);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
        __syncthreads();
        return red[0] + red[1] + red[2] + red[3];
    };
    for (int col = threadIdx.x; col < nf; col += 256) {
        double t = 0.0;
        for (int k = 0; k < r.nch; ++k) t += part[((long long)b * r.nch + k) * nf + col];
        feat[col] = (float)t;
    }
    __syncthreads();
    for (int o = 0; o < r.n_out; ++o) {
        double s = 0.0;
        for (int k = threadIdx.x; k < nf; k += 256) s += (double)r.fcw[o * nf + k] * (double)feat[k];
        const double t = bsum(s);
        if (threadIdx.x == 0) r.out[(long long)b * r.n_out + o] = (float)(t + (double)r.fcb[o]);
    }
}

// dsum[b][k] = sum_o dout[b][o] fcw[o][k] (blocks [0, nd)); dfcw[o][k], dfcb[o] summed over the graphs in
// fp64, one wave per output (the remaining blocks; was one block doing all of it serially)
__global__ void __launch_bounds__(256) k_ccn_readout_bwd(const float* __restrict__ dout, const float* __restrict__ feat,
                                                         const float* __restrict__ fcw, int bs, int n_out, int nf,
                                                         float* __restrict__ dsum, float* __restrict__ dfcw,
                                                         float* __restrict__ dfcb) {
    const int nd = (bs * nf + 255) / 256;
    if ((int)blockIdx.x < nd) {
        const int e = blockIdx.x * 256 + threadIdx.x;
        if (e < bs * nf) {
            const int b = e / nf, k = e % nf;
            float s = 0.f;
            for (int o = 0; o < n_out; ++o) s = fmaf(dout[b * n_out + o], fcw[o * nf + k], s);
            dsum[e] = s;
        }
        return;
    }
    const int w = ((int)blockIdx.x - nd) * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (w >= n_out * nf + n_out) return;
    double s = 0.0;
    if (w < n_out * nf) {
        const int o = w / nf, k = w % nf;
        for (int b = lane; b < bs; b += 64) s += (double)dout[b * n_out + o] * (double)feat[(long long)b * nf + k];
    } else {
        const int o = w - n_out * nf;
        for (int b = lane; b < bs; b += 64) s += (double)dout[b * n_out + o];
    }
    s = wave_sum_d(s);
    if (lane == 0) {
        if (w < n_out * nf) dfcw[w] = (float)s;
        else dfcb[w - n_out * nf] = (float)s;
    }
}

// sum the per-node parameter partials: out[k] = sum_i part[i][k]  (k < kw: weight, then bias)
__global__ void __launch_bounds__(256) k_ccn_param_reduce(const float* __restrict__ part, const int* total_nodes,
                                                          int kw, int kb, float* __restrict__ dw, float* __restrict__ db) {
    __shared__ double red[4];
    const int k = blockIdx.x;
    const int n = *total_nodes;
    const int stride = kw + kb;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)part[(long long)i * stride + k];
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double t = red[0] + red[1] + red[2] + red[3];
        if (k < kw) dw[k] = (float)t;
        else db[k - kw] = (float)t;
    }
}

// dF[row][c] = dsum[graph][off + c] for every feature row of the node (top level)
__global__ void k_ccn_bcast(CcnPlanView v, const int* total_nodes, int order, const float* __restrict__ dsum, int ld,
                            int off, int h, float* __restrict__ dF) {
    const int i = blockIdx.x;
    if (i >= *total_nodes) return;
    const int g = v.graph[i];
    const long long r0 = order == 1 ? v.off1[i] : v.off2[i];
    const long long r1 = order == 1 ? v.off1[i + 1] : v.off2[i + 1];
    for (long long q = r0 * h + threadIdx.x; q < r1 * h; q += blockDim.x) dF[q] = dsum[(long long)g * ld + off + (int)(q % h)];
}

// X (bs, nmax, f) padded -> packed [nodes][f]; and the inverse for dX (zero padding)
__global__ void k_ccn_pack_x(const float* __restrict__ X, const int* node_off, int nmax, int f, float* __restrict__ Xp) {
    const int b = blockIdx.x;
    const int n0 = node_off[b], nb = node_off[b + 1] - n0;
    for (int e = threadIdx.x; e < nb * f; e += blockDim.x) Xp[(long long)n0 * f + e] = X[(long long)b * nmax * f + e];
}

__global__ void k_ccn_unpack_dx(const float* __restrict__ dXp, const int* node_off, int nmax, int f,
                                float* __restrict__ dX) {
    const int b = blockIdx.x;
    const int n0 = node_off[b], nb = node_off[b + 1] - n0;
    for (int e = threadIdx.x; e < nmax * f; e += blockDim.x)
        dX[(long long)b * nmax * f + e] = e < nb * f ? dXp[(long long)n0 * f + e] : 0.f;
}

// collapse6to3 on a general F (C, n, n, n, n, n): out[x][y][q*C + ch]
// (functions/contraction.py: _c6to2_111 44-61, _c6to2_12 64-85, _c6to2_3 88-103)
__global__ void k_collapse6to3(const float* __restrict__ F, float* __restrict__ out, int C, int n) {
    const long long tot = (long long)n * n * 18 * C;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= tot) return;
    const int ch = (int)(idx % C), q = (int)((idx / C) % 18);
    const int y = (int)((idx / (18LL * C)) % n), x = (int)(idx / (18LL * C * n));
    auto G = [&](int a, int b, int c, int d, int e) {
        return F[(((((long long)ch * n + a) * n + b) * n + c) * n + d) * n + e];
    };
    float s = 0.f;
    if (q == 0) {
        for (int c = 0; c < n; ++c) for (int d = 0; d < n; ++d) for (int e = 0; e < n; ++e) s += G(x, y, c, d, e);
    } else if (q == 1) {
        for (int b = 0; b < n; ++b) for (int c = 0; c < n; ++c) for (int e = 0; e < n; ++e) s += G(x, b, c, y, e);
    } else if (q == 2) {
        for (int a = 0; a < n; ++a) for (int d = 0; d < n; ++d) for (int e = 0; e < n; ++e) s += G(a, x, y, d, e);
    } else if (q == 3) {
        for (int a = 0; a < n; ++a) for (int c = 0; c < n; ++c) for (int e = 0; e < n; ++e) s += G(a, x, c, y, e);
    } else if (q == 4) {
        for (int a = 0; a < n; ++a) for (int b = 0; b < n; ++b) for (int c = 0; c < n; ++c) s += G(a, b, c, x, y);
    } else if (q == 5) {
        for (int e = 0; e < n; ++e) for (int c = 0; c < n; ++c) s += G(x, y, c, c, e);
    } else if (q < 15) {
        for (int c = 0; c < n; ++c) for (int d = 0; d < n; ++d) s += G(x, y, c, d, d);
    } else if (q == 15) {
        for (int b = 0; b < n; ++b) s += G(x, b, b, y, b);
    } else if (q == 16) {
        for (int a = 0; a < n; ++a) s += G(a, x, a, y, a);
    } else {
        for (int a = 0; a < n; ++a) s += G(a, a, a, x, y);
    }
    out[idx] = s;
}

// adjoint of k_collapse6to3: dF[ch][a][b][c][d][e] from dOut[x][y][q*C + ch]
__global__ void k_collapse6to3_bwd(const float* __restrict__ dO, float* __restrict__ dF, int C, int n) {
    const long long tot = (long long)C * n * n * n * n * n;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= tot) return;
    long long t = idx;
    const int e = (int)(t % n); t /= n;
    const int d = (int)(t % n); t /= n;
    const int c = (int)(t % n); t /= n;
    const int b = (int)(t % n); t /= n;
    const int a = (int)(t % n); t /= n;
    const int ch = (int)t;
    auto g = [&](int x, int y, int q) { return dO[((long long)x * n + y) * 18 * C + q * C + ch]; };
    float s = g(a, b, 0) + g(a, d, 1) + g(b, c, 2) + g(b, d, 3) + g(d, e, 4);
    if (c == d) s += g(a, b, 5);
    if (d == e)
        for (int q = 6; q < 15; ++q) s += g(a, b, q);
    if (b == c && c == e) s += g(a, d, 15);
    if (a == c && c == e) s += g(b, d, 16);
    if (a == b && b == c) s += g(d, e, 17);
    dF[idx] = s;
}

}  // namespace

int launch_ccn_readout(ReadoutArgs ra, long long rows, double* rpart, hipStream_t s) {
    ra.nch = ro_chunks(rows, ra.bs);
    HGNN_KLAUNCH(k_ccn_readout_part, dim3(ra.bs, ra.nch), dim3(256), 0, s, ra, rpart);
    HGNN_LAUNCH_CHECK();
    HGNN_KLAUNCH(k_ccn_readout, dim3(ra.bs), dim3(256), 0, s, ra, rpart);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

int launch_ccn_readout_bwd(const float* dout, const float* feat, const float* fcw, int bs, int n_out, int nf,
                           float* dsum, float* dfcw, float* dfcb, hipStream_t s) {
    HGNN_KLAUNCH(k_ccn_readout_bwd, dim3((bs * nf + 255) / 256 + (n_out * nf + n_out + 3) / 4), dim3(256), 0, s, dout,
                 feat, fcw, bs, n_out, nf, dsum, dfcw, dfcb);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

int launch_ccn_param_reduce(const float* ppart, const int* tot, int kw, int kb, float* dw, float* db, hipStream_t s) {
    HGNN_KLAUNCH(k_ccn_param_reduce, dim3(kw + kb), dim3(256), 0, s, ppart, tot, kw, kb, dw, db);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

int launch_ccn_bcast(const CcnPlanView& v, const int* tot, int nodes, int order, const float* dsum, int ld, int off,
                     int h, float* dF, hipStream_t s) {
    HGNN_KLAUNCH(k_ccn_bcast, ccn_grid1(nodes), dim3(64), 0, s, v, tot, order, dsum, ld, off, h, dF);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

int launch_ccn_pack_x(const float* X, const int* node_off, int bs, int nmax, int f, float* Xp, hipStream_t s) {
    HGNN_KLAUNCH(k_ccn_pack_x, dim3(bs), dim3(256), 0, s, X, node_off, nmax, f, Xp);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

int launch_ccn_unpack_dx(const float* dXp, const int* node_off, int bs, int nmax, int f, float* dX, hipStream_t s) {
    HGNN_KLAUNCH(k_ccn_unpack_dx, dim3(bs), dim3(256), 0, s, dXp, node_off, nmax, f, dX);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

}  // namespace hgnn

using namespace hgnn;

extern "C" {

int hgnn_collapse6to3(const float* d_F, float* d_out, int c, int n, void* stream) {
    if (!d_F || !d_out || c <= 0 || n <= 0) return HGNN_ERR_ARG;
    const long long tot = (long long)n * n * 18 * c;
    HGNN_KLAUNCH(k_collapse6to3, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_F,
                       d_out, c, n);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

int hgnn_collapse6to3_backward(const float* d_dout, float* d_dF, int c, int n, void* stream) {
    if (!d_dout || !d_dF || c <= 0 || n <= 0) return HGNN_ERR_ARG;
    const long long tot = (long long)c * n * n * n * n * n;
    HGNN_KLAUNCH(k_collapse6to3_bwd, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       d_dout, d_dF, c, n);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

}  // extern "C"
