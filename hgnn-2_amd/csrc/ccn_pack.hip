// CCN chunks from a resident graph pack: the padded (X, A + I, n_batch, y) batch that
// hgnn_amd.train.CcnTrainStep._chunks assembles on the host per graph (scripts/train_ccn.py:35-37 plus padding),
// built on the device from hgnn_amd.dataset.DevicePack's arrays in one dispatch.
//
// k_ccn_pack_chunk  one workgroup of one wave per chunk slot b, graph g = idx[b].  The slot's X block
//                   (nmax x f_in) and adjacency block (nmax x nmax) are each one contiguous run of floats, so
//                   they are written as runs, not as rows: up to three single floats to the first 16-byte
//                   boundary, float4 stores over the body, up to three single floats at the end.  f_in = 5 and an
//                   odd nmax leave almost no ROW aligned; the run's head and tail are all that is ragged.
//
// Pure data movement and one exact `w + 1.0f` on the diagonal: the result is bit for bit the host's.  No LDS:
// the only thing the lanes agree on is "the graph is malformed", one wave-wide vote.
//
// Every element of the four outputs is written exactly once, except the adjacency elements that hold a stored
// entry, which are written twice: first by the fill (0, or 1 on the diagonal), then by the entry (w, or w + 1).
// The order is fixed by construction: all lanes of the slot's single wave issue their fill stores, pass the
// __syncthreads() below (a workgroup-scope release / acquire fence around the barrier), and only then issue the
// entry stores.  Two entries never share an address: a graph whose (i, j) are not strictly ascending row-major
// is refused like one with an index outside [0, n), before anything is written.
#include "common.h"

namespace hgnn {
namespace {

constexpr int CP_THREADS = HGNN_WAVE;  // one wave: the malformed-graph vote is a ballot, not an LDS reduction

struct CpArgs {
    hgnn_pack_view v;
    const int32_t* idx;
    int n_targets, nmax, task;
    float *X, *adj;
    long long* nb;
    float* y;
    int32_t* err;
};

// p[e] = val(e) for e in [0, len): single floats up to the first 16-byte boundary, float4 over the body, single
// floats at the end.  p is 4-byte aligned; head and tail are at most 3 elements each (< CP_THREADS).
template <class F>
__device__ __forceinline__ void cp_fill(float* p, int len, F val) {
    const int lane = threadIdx.x;
    const int head = min(len, (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2));
    if (lane < head) p[lane] = val(lane);
    const int nv = (len - head) >> 2;
    float4* q = reinterpret_cast<float4*>(p + head);
    for (int v = lane; v < nv; v += CP_THREADS) {
        const int e = head + 4 * v;
        q[v] = make_float4(val(e), val(e + 1), val(e + 2), val(e + 3));
    }
    const int e = head + 4 * nv + lane;
    if (e < len) p[e] = val(e);
}

__global__ void __launch_bounds__(CP_THREADS) k_ccn_pack_chunk(CpArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int nmax = a.nmax, f = a.v.f_in;
    const long long g = a.idx[b];
    // everything up to the vote is uniform over the wave
    bool bad = g < 0 || g >= a.v.graphs;
    long long nn0 = 0, a0 = 0;
    int n = 0, cnt = 0;
    if (!bad) {
        nn0 = a.v.d_node_off[g];
        a0 = a.v.d_adj_off[g];
        const long long n64 = a.v.d_node_off[g + 1] - nn0, c64 = a.v.d_adj_off[g + 1] - a0;
        // strictly ascending entries are at most n^2 (n <= nmax, nmax^2 < 2^31: the host checked)
        bad = n64 < 0 || n64 > nmax || c64 < 0 || c64 > n64 * n64;
        if (!bad) {
            n = (int)n64;
            cnt = (int)c64;
        }
    }
    if (!bad) {
        int wrong = 0;
        for (int e = lane; e < cnt; e += CP_THREADS) {
            const int i = a.v.d_adj_ij[2 * (a0 + e)], j = a.v.d_adj_ij[2 * (a0 + e) + 1];
            bool ok = (unsigned)i < (unsigned)n && (unsigned)j < (unsigned)n;
            if (e > 0) {
                const int pi = a.v.d_adj_ij[2 * (a0 + e) - 2], pj = a.v.d_adj_ij[2 * (a0 + e) - 1];
                ok = ok && (pi < i || (pi == i && pj < j));
            }
            wrong |= !ok;
        }
        bad = __any(wrong);
    }
    if (bad) n = cnt = 0;  // the empty slot the CCN kernels skip: all zero, n_batch = 0

    const float* xs = a.v.d_x + nn0 * f;
    const int nf = n * f;
    cp_fill(a.X + (size_t)b * nmax * f, nmax * f, [&](int e) { return e < nf ? xs[e] : 0.f; });
    // I on the real block: element r * nmax + r = r * (nmax + 1), r < n
    float* A = a.adj + (size_t)b * nmax * nmax;
    const int dstep = nmax + 1, dend = n * dstep;
    cp_fill(A, nmax * nmax, [&](int e) { return e < dend && e % dstep == 0 ? 1.f : 0.f; });
    __syncthreads();  // fill before entries: see the head of the file
    for (int e = lane; e < cnt; e += CP_THREADS) {
        const int i = a.v.d_adj_ij[2 * (a0 + e)], j = a.v.d_adj_ij[2 * (a0 + e) + 1];
        const float w = a.v.d_adj_w[a0 + e];
        A[i * nmax + j] = i == j ? w + 1.0f : w;  // A + torch.eye(n): exact off the diagonal, one add on it
    }
    if (lane == 0) {
        a.nb[b] = n;
        a.y[b] = bad ? 0.f : a.v.d_targets[g * a.n_targets + a.task];
        if (bad && a.err) atomicOr(a.err, 1);
    }
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

extern "C" {

int hgnn_pack_ccn_chunk(const hgnn_pack_view* view, int n_targets, const int32_t* d_idx, int G, int nmax, int task,
                        float* d_X, float* d_adj, int64_t* d_n_batch, float* d_y, int32_t* d_err, void* stream) {
    if (!view || !view->d_node_off || !view->d_x || !view->d_adj_off || !view->d_adj_ij || !view->d_adj_w ||
        !view->d_targets || view->graphs <= 0 || view->graphs >= (1ll << 31) || view->f_in <= 0)
        return HGNN_ERR_ARG;
    if (!d_idx || !d_X || !d_adj || !d_n_batch || !d_y || G <= 0 || nmax <= 0 || task < 0 || task >= n_targets)
        return HGNN_ERR_ARG;
    // a slot's blocks are indexed in 32 bits (and n * (nmax + 1) with them)
    if ((long long)nmax * (nmax + 1) > 0x7fffffffll || (long long)nmax * view->f_in > 0x7fffffffll)
        return HGNN_ERR_UNSUPPORTED;
    CpArgs a{};
    a.v = *view;
    a.idx = d_idx;
    a.n_targets = n_targets;
    a.nmax = nmax;
    a.task = task;
    a.X = d_X;
    a.adj = d_adj;
    a.nb = reinterpret_cast<long long*>(d_n_batch);
    a.y = d_y;
    a.err = d_err;
    HGNN_KLAUNCH(k_ccn_pack_chunk, dim3((unsigned)G), dim3(CP_THREADS), 0, static_cast<hipStream_t>(stream), a);
    HGNN_LAUNCH_CHECK();
    return HGNN_OK;
}

}  // extern "C"
