// Kernel probes of the dense side outside the GEMMs (include/hgnn_amd.h, "Kernel probes"): the BN finalize and
// backward, the readout launchers (bn.hip) and the dense operator gradient (dwdense.hip, k_dw_readout) behind plain
// entry points for tests.  Each probe fills the launcher's argument struct from its C mirror and returns the
// launcher's status unchanged.  No kernels of its own, nothing allocated, only enqueues on `stream`.
#include "kernels.h"

namespace hgnn {
namespace {

StructView list_view(const hgnn_probe_list& l) {
    return StructView{reinterpret_cast<const RowInfo*>(l.rows), l.entries, l.stride};
}

bool list_ok(const hgnn_probe_list& l) { return l.rows && l.entries && l.stride >= 4 && l.stride % 4 == 0; }

bool readout_agg_ok(const hgnn_probe_readout_agg_args* p) {
    if (!p || !p->dout || !p->fcw || p->dim_out <= 0 || p->jt <= 0 || p->bs <= 0 || p->cg < 0 || p->cp < 0 ||
        p->g_cap < 0 || p->p_cap < 0 || p->k < p->jt * p->cg + 2 * p->cp)
        return false;
    if (p->g_out && (!p->node_off || !list_ok(p->g) || p->cg <= 0)) return false;
    if (p->p_out && (!p->edge_off || !list_ok(p->p) || p->cp <= 0)) return false;
    return true;
}

ReadoutAggArgs readout_agg_args(const hgnn_probe_readout_agg_args& p) {
    ReadoutAggArgs a{};
    a.dout = p.dout;
    a.fcw = p.fcw;
    a.dim_out = p.dim_out;
    a.k = p.k;
    a.jt = p.jt;
    a.cg = p.cg;
    a.cp = p.cp;
    a.bs = p.bs;
    a.node_off = p.node_off;
    a.edge_off = p.edge_off;
    a.g = list_view(p.g);
    a.g_total = p.g_total;
    a.g_cap = p.g_cap;
    a.g_out = p.g_out;
    a.g_acc = p.g_acc;
    a.p = list_view(p.p);
    a.p_total = p.p_total;
    a.p_cap = p.p_cap;
    a.p_out = p.p_out;
    a.p_acc = p.p_acc;
    return a;
}

bool dw_dense_ok(const hgnn_probe_dw_dense_args* p, bool readout) {
    if (!p || !p->node_off || !p->dW || p->f <= 0 || p->jt <= 0 || p->bs <= 0 || p->nmax <= 0) return false;
    if (!p->xp == !p->xdense) return false;
    if (p->pmean && (!p->pstd || !p->pw || !p->pb)) return false;
    if (p->dout && (!p->fcw || p->dim_out <= 0 || p->kfc < p->jt * p->f)) return false;
    if (readout) return true;  // (launch_dw_readout refuses a null dout itself)
    return p->dA && p->lda >= p->jt * p->f;
}

DwDenseArgs dw_dense_args(const hgnn_probe_dw_dense_args& p) {
    DwDenseArgs a{};
    a.dA = p.dA;
    a.lda = p.lda;
    a.f = p.f;
    a.jt = p.jt;
    a.xp = p.xp;
    a.xdense = p.xdense;
    a.pmean = p.pmean;
    a.pstd = p.pstd;
    a.pw = p.pw;
    a.pb = p.pb;
    a.dout = p.dout;
    a.fcw = p.fcw;
    a.dim_out = p.dim_out;
    a.kfc = p.kfc;
    a.node_off = p.node_off;
    a.bs = p.bs;
    a.nmax = p.nmax;
    a.dW = p.dW;
    a.accumulate = p.accumulate;
    return a;
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

extern "C" {

int hgnn_probe_bn_finalize(const hgnn_probe_bn_finalize_args* p, void* stream) {
    if (!p || !p->mean || !p->std || p->c <= 0 || p->tiles < 0 || (!p->run_mean) != (!p->run_std)) return HGNN_ERR_ARG;
    if (p->training ? (!p->count || (!p->acc) == (!p->part)) : !p->run_mean) return HGNN_ERR_ARG;
    BnFwdArgs a{};
    a.acc = p->acc;
    a.part = p->part;
    a.tiles = p->tiles;
    a.c = p->c;
    a.count = p->count;
    a.mean = p->mean;
    a.std = p->std;
    a.run_mean = p->run_mean;
    a.run_std = p->run_std;
    a.training = p->training;
    a.momentum = 0.1f;
    return launch_bn_finalize(a, (hipStream_t)stream);
}

int hgnn_probe_bn_backward(hgnn_probe_bn_backward_args* p, void* stream) {
    if (!p || !p->y || !p->dz || !p->total_rows || !p->mean || !p->std || !p->w || !p->part || !p->sums ||
        p->c <= 0 || p->cap_rows < 0 || p->ldy < 0 || (p->apply && (!p->dy || !p->dw || !p->db)) ||
        ((reinterpret_cast<uintptr_t>(p->part) | reinterpret_cast<uintptr_t>(p->sums)) & 15))
        return HGNN_ERR_ARG;
    BnBwdArgs a{};
    a.y = p->y;
    a.dz = p->dz;
    a.total_rows = p->total_rows;
    a.cap_rows = p->cap_rows;
    a.c = p->c;
    a.mean = p->mean;
    a.std = p->std;
    a.w = p->w;
    a.relu_from = p->relu_from;
    a.training = p->training;
    a.part = p->part;
    a.sums = p->sums;
    a.dy = p->dy;
    a.ldy = p->ldy;
    a.dw = p->dw;
    a.db = p->db;
    a.dbpart = p->dbpart;
    a.acc64 = p->acc64;
    a.acc64_zero = p->acc64_zero;
    p->path = (int)bn_bwd_variant(a, p->apply);
    return launch_bn_backward(a, (hipStream_t)stream, p->apply);
}

int hgnn_probe_readout_fwd(const float* d_a, int k, const int32_t* d_node_off, int bs, int nmax, const float* d_fcw,
                           const float* d_fcb, int dim_out, float* d_colsum, float* d_out, void* stream) {
    if (!d_a || !d_node_off || !d_fcw || !d_fcb || !d_colsum || !d_out || k <= 0 || bs <= 0 || nmax <= 0 ||
        dim_out <= 0)
        return HGNN_ERR_ARG;
    return launch_readout_fwd(d_a, k, d_node_off, bs, nmax, d_fcw, d_fcb, dim_out, d_colsum, d_out,
                              (hipStream_t)stream);
}

int hgnn_probe_readout_bwd_da(const float* d_dout, const int32_t* d_node_off, int bs, int cap_rows,
                              const int32_t* d_total_rows, const float* d_fcw, int dim_out, int k, float* d_da,
                              void* stream) {
    if (!d_dout || !d_node_off || !d_fcw || !d_da || bs <= 0 || cap_rows < 0 || dim_out <= 0 || k <= 0)
        return HGNN_ERR_ARG;
    return launch_readout_bwd_da(d_dout, d_node_off, bs, cap_rows, d_total_rows, d_fcw, dim_out, k, d_da,
                                 (hipStream_t)stream);
}

size_t hgnn_probe_readout_bwd_scratch_bytes(int dim_out, int k) {
    if (dim_out <= 0 || k <= 0) return 0;
    return readout_bwd_scratch_bytes(dim_out, k);
}

int hgnn_probe_readout_bwd_params(const float* d_dout, const float* d_colsum, int bs, int nmax, int dim_out, int k,
                                  float* d_dfcw, float* d_dfcb, void* scratch, void* stream) {
    if (!d_dout || !d_colsum || !d_dfcw || !d_dfcb || !scratch || bs <= 0 || nmax <= 0 || dim_out <= 0 || k <= 0)
        return HGNN_ERR_ARG;
    return launch_readout_bwd_params(d_dout, d_colsum, bs, nmax, dim_out, k, d_dfcw, d_dfcb, scratch,
                                     (hipStream_t)stream);
}

int hgnn_probe_readout_agg_bwd(const hgnn_probe_readout_agg_args* p, void* stream) {
    if (!readout_agg_ok(p)) return HGNN_ERR_ARG;
    return launch_readout_agg_bwd(readout_agg_args(*p), (hipStream_t)stream);
}

int hgnn_probe_dw_dense(const hgnn_probe_dw_dense_args* p, void* stream) {
    if (!dw_dense_ok(p, false)) return HGNN_ERR_ARG;
    return launch_dw_dense(dw_dense_args(*p), (hipStream_t)stream);
}

int hgnn_probe_dw_readout(const hgnn_probe_dw_dense_args* p, void* stream) {
    if (!dw_dense_ok(p, true)) return HGNN_ERR_ARG;
    return launch_dw_readout(dw_dense_args(*p), (hipStream_t)stream);
}

int hgnn_probe_readout_row_fits(const hgnn_probe_readout_agg_args* ra, const hgnn_probe_dw_dense_args* dw) {
    if (!ra) return 0;
    if (!dw) return readout_row_fits(readout_agg_args(*ra), nullptr) ? 1 : 0;
    const DwDenseArgs d = dw_dense_args(*dw);
    return readout_row_fits(readout_agg_args(*ra), &d) ? 1 : 0;
}

}  // extern "C"
