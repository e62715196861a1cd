// Kernel probes (include/hgnn_amd.h, "Kernel probes"): the Conv1d-pair GEMMs and the weight repack behind plain
// entry points for tests.  Each probe repacks the pair with launch_repack and hands the GEMM launcher the
// operands with the leading dimensions net.hip uses (FwdWalk::half, BwdWalk::half / fork_dw), so the repack ->
// GEMM operand contract is what the executor runs.  No kernels of its own.
#include "kernels.h"

namespace hgnn {
namespace {

int pad4(int x) { return (x + 3) / 4 * 4; }
size_t up256(size_t x) { return (x + 255) / 256 * 256; }

// the repacked pair, the BN scratch and a row count inside the workspace
struct ProbeWs {
    size_t wt, wc, bc, wc3, wt3, part, acc, ticket, cnt, bytes;
};

ProbeWs probe_ws(int d, int k, int m_cap) {
    const int c2 = 2 * d, c2p = pad4(c2), kp = pad4(k);
    ProbeWs w;
    size_t o = 0;
    auto take = [&](size_t b) {
        const size_t at = o;
        o += up256(b);
        return at;
    };
    w.wt = take((size_t)k * c2p * 4);
    w.wc = take((size_t)c2 * kp * 4);
    w.bc = take((size_t)c2 * 4);
    w.wc3 = take((size_t)3 * c2 * bf3_ld(kp) * 2);
    w.wt3 = take((size_t)3 * k * bf3_ld(c2p) * 2);
    w.part = take((size_t)gemm_fwd_tiles_m(m_cap) * c2 * 3 * 4);
    w.acc = take((size_t)bn_acc_doubles(c2) * 8);
    w.ticket = take(4);
    w.cnt = take(4);
    w.bytes = o;
    return w;
}

bool probe_fits(int d, int k, int m_cap) {
    const long long lim = (1ll << 31) - 1;
    return d > 0 && k > 0 && m_cap >= 0 && 2 * d <= 1024 && (long long)pad4(2 * d) * pad4(k) * 4 <= lim &&
           (long long)m_cap * pad4(k) * 4 <= lim;
}

RepackTable pair_table(const float* wl, const float* wr, const float* bl, const float* br, int d, int k, float* wt,
                       float* wc, float* bc, __bf16* wc3, __bf16* wt3) {
    RepackTable rt{};
    rt.d = d;
    rt.n = 1;
    RepackItem& it = rt.it[0];
    it.wl = wl;
    it.wr = wr;
    it.bl = bl;
    it.br = br;
    it.wt = wt;
    it.wc = wc;
    it.bc = bc;
    it.k = k;
    it.kp = pad4(k);
    it.ldt = pad4(2 * d);
    it.wc3 = wc3;
    it.ldc3 = bf3_ld(it.kp);
    it.wt3 = wt3;
    it.ldt3 = bf3_ld(it.ldt);
    return rt;
}

int repack_into(const ProbeWs& w, char* ws, const float* wl, const float* wr, const float* bl, const float* br, int d,
                int k, hipStream_t s) {
    return launch_repack(pair_table(wl, wr, bl, br, d, k, (float*)(ws + w.wt), (float*)(ws + w.wc),
                                    (float*)(ws + w.bc), (__bf16*)(ws + w.wc3), (__bf16*)(ws + w.wt3)),
                         s);
}

bool diag_args(const hgnn_probe_diag& g, DiagIdArgs& id) {
    if (!g.x) return false;
    id.x = g.x;
    id.ldx = g.ldx;
    id.c = g.c;
    id.diag = reinterpret_cast<const float2*>(g.diag);
    id.bn.mean = g.mean;
    id.bn.std = g.std;
    id.bn.w = g.w;
    id.bn.b = g.b;
    return true;
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

extern "C" {

int hgnn_probe_repack(const float* d_wl, const float* d_wr, const float* d_bl, const float* d_br, int d, int k,
                      float* d_wt, float* d_wc, float* d_bc, void* d_wc3, void* d_wt3, void* stream) {
    if (!d_wl || !d_wr || !d_bl || !d_br || !d_wt || !d_wc || !d_bc || d <= 0 || k <= 0) return HGNN_ERR_ARG;
    if (!probe_fits(d, k, 0)) return HGNN_ERR_UNSUPPORTED;
    return launch_repack(pair_table(d_wl, d_wr, d_bl, d_br, d, k, d_wt, d_wc, d_bc, (__bf16*)d_wc3, (__bf16*)d_wt3),
                         (hipStream_t)stream);
}

size_t hgnn_probe_gemm_workspace_bytes(int d, int k, int m_cap) {
    if (m_cap <= 0 || !probe_fits(d, k, m_cap)) return 0;
    return probe_ws(d, k, m_cap).bytes;
}

int hgnn_probe_gemm_fwd(const hgnn_probe_fwd* p, void* workspace, void* stream) {
    if (!p || !workspace || !p->a || !p->wl || !p->wr || !p->bl || !p->br || !p->y || p->m_cap <= 0 || p->d <= 0 ||
        p->k <= 0 || p->kernel < 0 || p->kernel > 2 || p->bn < 0 || p->bn > 3 || (p->bn && (!p->mean || !p->std)) ||
        (!p->run_mean) != (!p->run_std))
        return HGNN_ERR_ARG;
    if (!probe_fits(p->d, p->k, p->m_cap)) return HGNN_ERR_UNSUPPORTED;
    DiagIdArgs ida{};
    const bool id = diag_args(p->diag, ida);
    // the fp32 kernels have neither the fp64 statistics nor the diagonal columns
    if (p->kernel != 0 && (p->bn > 1 || id)) return HGNN_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const ProbeWs w = probe_ws(p->d, p->k, p->m_cap);
    char* ws = (char*)workspace;
    const int c2 = 2 * p->d, kp = pad4(p->k);
    int r = repack_into(w, ws, p->wl, p->wr, p->bl, p->br, p->d, p->k, s);
    if (r) return r;
    float* part = p->bn == 1 ? (float*)(ws + w.part) : nullptr;
    double* acc = p->bn >= 2 ? (double*)(ws + w.acc) : nullptr;
    unsigned* ticket = (unsigned*)(ws + w.ticket);
    int* cnt = (int*)(ws + w.cnt);
    if (acc) {  // zero on entry: the executor's first kernel does this (BatchMeta::zero64)
        HGNN_HOST_CHECK(hipMemsetAsync(acc, 0, (size_t)bn_acc_doubles(c2) * 8, s));
        HGNN_HOST_CHECK(hipMemsetAsync(ticket, 0, 4, s));
    }
    FwdBnFin fin{};
    if (p->bn == 3) {
        fin.mean = p->mean;
        fin.std = p->std;
        fin.run_mean = p->run_mean;
        fin.run_std = p->run_std;
        fin.momentum = 0.1f;
        fin.ticket = ticket;
    }
    if (p->kernel == 0)
        r = launch_gemm_bf3_fwd(p->a, p->lda, p->m_valid, p->m_cap, kp, (const __bf16*)(ws + w.wc3),
                                (long long)c2 * bf3_ld(kp), bf3_ld(kp), c2, (const float*)(ws + w.bc), p->relu_from,
                                p->y, p->ldy, part, s, id ? &ida : nullptr, acc, p->bn == 3 ? &fin : nullptr);
    else
        r = launch_gemm3_fwd(p->a, p->lda, p->m_valid, p->m_cap, kp, (const float*)(ws + w.wc), kp, c2,
                             (const float*)(ws + w.bc), p->relu_from, p->y, p->ldy, part, s, p->kernel == 2 ? 1 : 0);
    if (r) return r;
    if (p->bn == 3) {
        if (p->ticket_out) HGNN_HOST_CHECK(hipMemcpyAsync(p->ticket_out, ticket, 4, hipMemcpyDeviceToDevice, s));
        return HGNN_OK;
    }
    if (!p->bn) return HGNN_OK;
    if (!p->m_valid) HGNN_HOST_CHECK(hipMemsetD32Async((hipDeviceptr_t)cnt, p->m_cap, 1, s));
    BnFwdArgs bf{};
    bf.acc = acc;
    bf.part = (const float*)(ws + w.part);
    bf.tiles = gemm_fwd_tiles_m(p->m_cap);
    bf.c = c2;
    bf.count = p->m_valid ? p->m_valid : cnt;
    bf.mean = p->mean;
    bf.std = p->std;
    bf.run_mean = p->run_mean;
    bf.run_std = p->run_std;
    bf.training = 1;
    bf.momentum = 0.1f;
    return launch_bn_finalize(bf, s);
}

int hgnn_probe_gemm_da(const hgnn_probe_da* p, void* workspace, void* stream) {
    if (!p || !workspace || !p->dy || !p->wl || !p->wr || !p->bl || !p->br || !p->da || p->m_cap <= 0 || p->d <= 0 ||
        p->k <= 0 || p->kernel < 0 || p->kernel > 1)
        return HGNN_ERR_ARG;
    if (!probe_fits(p->d, p->k, p->m_cap)) return HGNN_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const ProbeWs w = probe_ws(p->d, p->k, p->m_cap);
    char* ws = (char*)workspace;
    const int c2p = pad4(2 * p->d);
    if (p->lddy < c2p || p->ldda < p->k) return HGNN_ERR_ARG;
    const int r = repack_into(w, ws, p->wl, p->wr, p->bl, p->br, p->d, p->k, s);
    if (r) return r;
    if (p->kernel == 0)
        return launch_gemm_bf3_da(p->dy, p->lddy, p->m_valid, p->m_cap, c2p, (const __bf16*)(ws + w.wt3),
                                  (long long)p->k * bf3_ld(c2p), bf3_ld(c2p), p->k, p->da, p->ldda, s);
    return launch_gemm3_da(p->dy, p->lddy, p->m_valid, p->m_cap, c2p, (const float*)(ws + w.wt), c2p, p->k, p->da,
                           p->ldda, s);
}

size_t hgnn_probe_dw_workspace_bytes(int r_cap, int o, int k, int nz) {
    if (r_cap <= 0 || o <= 0 || k <= 0 || nz < 0) return 0;
    if (!nz) nz = dw3_chunks(r_cap, o, k);
    return up256((size_t)nz * o * k * 4);
}

int hgnn_probe_gemm_dw(const hgnn_probe_dw* p, void* workspace, void* stream) {
    if (!p || !workspace || !p->dy || !p->a || !p->r_valid || !p->dw0 || !p->dw1 || p->r_cap <= 0 || p->o <= 0 ||
        p->k <= 0 || p->nz < 0 || p->o_real <= 0 || p->o_real > p->o || p->split < 0 || p->split > p->o_real ||
        p->lddy < p->o || (p->dbpart && (!p->db0 || !p->db1)))
        return HGNN_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    DiagIdArgs ida{};
    const bool id = diag_args(p->diag, ida);
    const int nz = p->nz ? p->nz : dw3_chunks(p->r_cap, p->o, p->k);
    float* slabs = (float*)workspace;
    const int r = launch_gemm3_dw(p->dy, p->lddy, p->a, p->lda, p->r_valid, p->r_cap, p->o, p->k, nz, slabs, s,
                                  id ? &ida : nullptr);
    if (r) return r;
    return launch_dw_reduce2(slabs, p->r_valid, nz, p->o, p->o_real, p->k, p->split, p->dw0, p->dw1, p->dbpart, p->db0,
                             p->db1, s);
}

}  // extern "C"
