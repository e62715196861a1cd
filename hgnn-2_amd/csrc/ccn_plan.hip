// The plan of the general CCN path: a batch's neighbour lists, degrees, prefix offsets and chi position maps
// (ccn.hip's header comment has the index construction), the layout of the plan workspace and the plan entry
// points of include/hgnn_amd.h.
#include "ccn_general.h"

namespace hgnn {
namespace {

// Row r of graph b (wave per row, CCN_NB_ROWS rows per block): the neighbour list (ascending), degree and
// self position, and the row's pattern as a bit set over the graph's local node ids (64-bit words) with
// the exclusive prefix count of each word, from which k_ccn_pos reads positions by popcount.
constexpr int CCN_NB_ROWS = 16;
__global__ void __launch_bounds__(256) k_ccn_nbrs(const float* __restrict__ adj, int nmax, const int* node_off,
                                                  int* deg, int* nbr, int* selfpos, int* graph,
                                                  unsigned long long* bits, int* bcnt, uint32_t* err, int maxd) {
    const int b = blockIdx.x;
    const int n0 = node_off[b];
    const int nb = node_off[b + 1] - n0;
    const int nw = (nmax + 63) >> 6;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float* A = adj + (long long)b * nmax * nmax;
    const int r1 = min(nb, (int)(blockIdx.y + 1) * CCN_NB_ROWS);
    for (int r = blockIdx.y * CCN_NB_ROWS + wv; r < r1; r += 4) {
        const int gi = n0 + r;
        int cnt = 0, sp = -1;
        for (int c0 = 0; c0 < nb; c0 += 64) {
            const int c = c0 + lane;
            const bool nz = c < nb && A[(long long)r * nmax + c] > 0.f;   // utils_ccn.py:195 (A > 0)
            const unsigned long long m = __ballot(nz);
            const int p = __popcll(m & ((1ull << lane) - 1ull));
            if (nz) {
                nbr[(long long)gi * nmax + cnt + p] = n0 + c;
                if (c == r) sp = cnt + p;
            }
            if (lane == 0) {
                bits[(long long)gi * nw + (c0 >> 6)] = m;
                bcnt[(long long)gi * nw + (c0 >> 6)] = cnt;
            }
            cnt += __popcll(m);
        }
        // self position: the lane that saw c == r holds it
        const unsigned long long hs = __ballot(sp >= 0);
        if (lane == 0) {
            deg[gi] = cnt;
            graph[gi] = b;
            if (cnt > maxd) atomicOr(err, (uint32_t)ERR_CCN_DEGREE);
        }
        if (hs == 0ull) {
            if (lane == 0) {
                selfpos[gi] = -1;
                atomicOr(err, (uint32_t)ERR_CCN_SELFLOOP);
            }
        } else if (sp >= 0) {
            selfpos[gi] = sp;
        }
    }
}

// exclusive scans of deg and deg^2 over all nodes (single block of 1024: a serial run of consecutive
// nodes per thread, then a scan of the 1024 run totals); totals[0..1] = the sums, totals[2] = max degree
__global__ void __launch_bounds__(1024) k_ccn_scan(const int* deg, const int* total_nodes, int* off1, int* off2,
                                                   int* totals) {
    __shared__ int s1[1024], s2[1024];
    const int t = threadIdx.x;
    const int n = *total_nodes;
    const int per = (n + 1023) / 1024;
    const int i0 = min(n, t * per), i1 = min(n, i0 + per);
    __shared__ int smax[16];
    int a1 = 0, a2 = 0, dm = 0;
    for (int i = i0; i < i1; ++i) {
        const int d = deg[i];
        a1 += d;
        a2 += d * d;
        dm = max(dm, d);
    }
    s1[t] = a1;
    s2[t] = a2;
    for (int o = 32; o > 0; o >>= 1) dm = max(dm, __shfl_xor(dm, o, 64));
    if ((t & 63) == 0) smax[t >> 6] = dm;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int b1 = t >= o ? s1[t - o] : 0, b2 = t >= o ? s2[t - o] : 0;
        __syncthreads();
        s1[t] += b1;
        s2[t] += b2;
        __syncthreads();
    }
    int c1 = s1[t] - a1, c2 = s2[t] - a2;
    for (int i = i0; i < i1; ++i) {
        const int d = deg[i];
        off1[i] = c1;
        off2[i] = c2;
        c1 += d;
        c2 += d * d;
    }
    if (t == 1023) {
        off1[n] = s1[1023];
        off2[n] = s2[1023];
        totals[0] = s1[1023];
        totals[1] = s2[1023];
        int m = 0;
        for (int w = 0; w < 16; ++w) m = max(m, smax[w]);
        totals[2] = m;  // largest receptive field
    }
}

// pos[off2[i] + a*d_i + x] = index of nbr_i[x] in nbr_{nbr_i[a]}, or -1: the count of j's neighbours
// below u = nbr_i[x] in j's row bit set (prefix count of u's word + popcount of the bits below u).
// The position of i itself in N(j) must exist for every j in N(i): the gather-form backward walks
// N(j) for the readers of F_j, so the pattern has to be symmetric.
__global__ void __launch_bounds__(256) k_ccn_pos(CcnPlanView v, const int* total_nodes,
                                                 const unsigned long long* __restrict__ bits,
                                                 const int* __restrict__ bcnt, int* pos, long long pos_cap,
                                                 uint32_t* err) {
    const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    if (i >= *total_nodes) return;
    // an asynchronous plan sized pos by a bound: a batch beyond it is refused, never overrun
    if ((long long)v.off2[*total_nodes] > pos_cap) {
        if (i == 0 && lane == 0) atomicOr(err, (uint32_t)ERR_SIZES);
        return;
    }
    const int n = v.deg[i];
    if (n > CCN1_MAXD) return;
    const int nw = (v.nmax + 63) >> 6;
    const int n0 = v.node_off[v.graph[i]];
    const int si = v.selfpos[i];
    const int* ni = v.nbr + (long long)i * v.nmax;
    const long long pb = v.off2[i];
    for (int x0 = 0; x0 < n; x0 += 64) {
        const int x = x0 + lane;
        const int u = x < n ? ni[x] - n0 : 0;
        const int uw = u >> 6;
        const unsigned long long below = (1ull << (u & 63)) - 1ull;
        for (int a = 0; a < n; a += 4) {
            unsigned long long w[4];
            int c[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = ni[a + q < n ? a + q : a];
                w[q] = bits[(long long)j * nw + uw];
                c[q] = bcnt[(long long)j * nw + uw];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (a + q >= n) break;
                if (x < n) {
                    const bool in = (w[q] >> (u & 63)) & 1ull;
                    const int p = in ? c[q] + __popcll(w[q] & below) : -1;
                    pos[pb + (long long)(a + q) * n + x] = p;
                    if (x == si && p < 0) atomicOr(err, (uint32_t)ERR_CCN_ASYM);
                }
            }
        }
    }
}

}  // namespace

// The plan workspace; pos, sized by the caller's bound on sum d_i^2, comes last.
CcnPlanLayout plan_layout(const hgnn_ccn_config* c, long long max_sum_d2) {
    CcnPlanLayout L{};
    const long long nodes = (long long)c->bs * c->nmax;
    size_t t = 0;
    auto take = [&](size_t n) {
        const size_t o = t;
        t += al(n);
        return o;
    };
    L.node_off = take(4 * (c->bs + 1));
    L.deg = take(4 * nodes);
    L.nbr = take(4 * nodes * c->nmax);
    L.selfpos = take(4 * nodes);
    L.graph = take(4 * nodes);
    L.off1 = take(4 * (nodes + 1));
    L.off2 = take(4 * (nodes + 1));
    L.totals = take(32);
    L.err = take(16);
    const int nw = (c->nmax + 63) / 64;
    L.bits = take(8 * nodes * nw);
    L.bcnt = take(4 * nodes * nw);
    L.pos = take(4 * (size_t)(max_sum_d2 > 0 ? max_sum_d2 : 1));
    L.bytes = t;
    return L;
}

CcnPlanView plan_view(const hgnn_ccn_config* c, const CcnPlanLayout& L, void* plan_ws) {
    CcnPlanView v;
    v.node_off = P<int>(plan_ws, L.node_off);
    v.deg = P<int>(plan_ws, L.deg);
    v.nbr = P<int>(plan_ws, L.nbr);
    v.selfpos = P<int>(plan_ws, L.selfpos);
    v.graph = P<int>(plan_ws, L.graph);
    v.off1 = P<int>(plan_ws, L.off1);
    v.off2 = P<int>(plan_ws, L.off2);
    v.pos = P<int>(plan_ws, L.pos);
    v.nmax = c->nmax;
    return v;
}

}  // namespace hgnn

using namespace hgnn;

extern "C" {

int hgnn_ccn_plan_offsets(const hgnn_ccn_config* cfg, long long max_sum_d2, size_t* offs) {
    if (!ccn_ok(cfg) || !offs) return HGNN_ERR_ARG;
    const CcnPlanLayout L = plan_layout(cfg, max_sum_d2);
    const size_t o[9] = {L.node_off, L.deg, L.nbr, L.selfpos, L.graph, L.off1, L.off2, L.pos, L.err};
    for (int i = 0; i < 9; ++i) offs[i] = o[i];
    return HGNN_OK;
}

size_t hgnn_ccn_plan_bytes(const hgnn_ccn_config* cfg, long long max_sum_d2) {
    if (!ccn_ok(cfg)) return 0;
    return plan_layout(cfg, max_sum_d2).bytes;
}

static int ccn_plan(const hgnn_ccn_config* cfg, const float* d_adj, const int64_t* d_n_batch, void* plan_ws,
                    long long max_sum_d2, long long* h_sums, hipStream_t s, bool sync) {
    if (!ccn_ok(cfg) || !d_adj || !d_n_batch || !plan_ws || !h_sums) return HGNN_ERR_ARG;
    const CcnPlanLayout L = plan_layout(cfg, max_sum_d2);
    BatchMeta m;
    m.node_off = P<int>(plan_ws, L.node_off);
    m.edge_off = P<int>(plan_ws, L.off1);  // scratch, overwritten by the scan
    m.totals = P<int>(plan_ws, L.totals);
    m.err = P<uint32_t>(plan_ws, L.err);
    HGNN_HOST_CHECK(hipMemsetAsync(m.err, 0, 4, s));
    int r = launch_plan(d_n_batch, nullptr, cfg->bs, cfg->nmax, 0, m, s);
    if (r) return r;
    CcnPlanView v = plan_view(cfg, L, plan_ws);
    HGNN_KLAUNCH(k_ccn_nbrs, dim3(cfg->bs, (cfg->nmax + CCN_NB_ROWS - 1) / CCN_NB_ROWS), dim3(256), 0, s, d_adj,
                       cfg->nmax, v.node_off, P<int>(plan_ws, L.deg), P<int>(plan_ws, L.nbr),
                       P<int>(plan_ws, L.selfpos), P<int>(plan_ws, L.graph), P<unsigned long long>(plan_ws, L.bits),
                       P<int>(plan_ws, L.bcnt), m.err, cfg->order == 1 ? CCN1_MAXD : CCN_BIGD);
    HGNN_LAUNCH_CHECK();
    HGNN_KLAUNCH(k_ccn_scan, dim3(1), dim3(1024), 0, s, P<int>(plan_ws, L.deg), m.totals,
                       P<int>(plan_ws, L.off1), P<int>(plan_ws, L.off2), m.totals + 2);
    HGNN_LAUNCH_CHECK();
    long long nodes = (long long)cfg->bs * cfg->nmax;
    if (sync) {
        int hbuf[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        HGNN_HOST_CHECK(hipMemcpyAsync(hbuf, m.totals, 32, hipMemcpyDeviceToHost, s));
        HGNN_HOST_CHECK(hipStreamSynchronize(s));
        nodes = hbuf[0];
        h_sums[0] = hbuf[2];
        h_sums[1] = hbuf[3];
        h_sums[2] = nodes;
        h_sums[3] = hbuf[4];
        if (h_sums[1] > max_sum_d2) return HGNN_ERR_ARG;  // caller re-plans with a larger bound
    } else {
        // bounds, no host sync: every graph's d_i <= n_b <= nmax; the kernels read the device totals
        h_sums[0] = nodes * cfg->nmax;
        h_sums[1] = max_sum_d2;
        h_sums[2] = nodes;
        h_sums[3] = cfg->nmax;
    }
    HGNN_KLAUNCH(k_ccn_pos, dim3((unsigned)((nodes + 3) / 4 > 0 ? (nodes + 3) / 4 : 1)), dim3(256), 0, s, v,
                       m.totals, P<unsigned long long>(plan_ws, L.bits), P<int>(plan_ws, L.bcnt),
                       P<int>(plan_ws, L.pos), max_sum_d2, m.err);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

int hgnn_ccn_plan(const hgnn_ccn_config* cfg, const float* d_adj, const int64_t* d_n_batch, void* plan_ws,
                  long long max_sum_d2, long long* h_sums, void* stream) {
    return ccn_plan(cfg, d_adj, d_n_batch, plan_ws, max_sum_d2, h_sums, (hipStream_t)stream, true);
}

int hgnn_ccn_plan_async(const hgnn_ccn_config* cfg, const float* d_adj, const int64_t* d_n_batch, void* plan_ws,
                        long long max_sum_d2, long long* h_sums_bound, void* stream) {
    // the bound must hold for any content, so no later kernel can meet an unplanned position map
    if (!cfg || max_sum_d2 < (long long)cfg->bs * cfg->nmax * cfg->nmax * cfg->nmax) return HGNN_ERR_ARG;
    return ccn_plan(cfg, d_adj, d_n_batch, plan_ws, max_sum_d2, h_sums_bound, (hipStream_t)stream, false);
}

uint32_t* hgnn_ccn_error_word(const hgnn_ccn_config* cfg, void* plan_ws, long long max_sum_d2) {
    if (!ccn_ok(cfg) || !plan_ws) return nullptr;
    return P<uint32_t>(plan_ws, plan_layout(cfg, max_sum_d2).err);
}

}  // extern "C"
