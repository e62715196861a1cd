// Kernel probes of the sparse side (include/hgnn_amd.h, "Kernel probes"): the batch plan and the structure
// extraction (struct.hip), the pack / unpack kernels and the aggregation launchers (agg.hip) behind plain entry
// points for tests.  Each probe fills the launcher's argument struct from its C mirror and returns the launcher's
// status unchanged.  No kernels of its own, nothing allocated, only enqueues on `stream`.
#include "kernels.h"

namespace hgnn {
namespace {

StructView list_view(const hgnn_probe_list& l) {
    return StructView{reinterpret_cast<const RowInfo*>(l.rows), l.entries, l.stride};
}

BnView bn_view(const hgnn_probe_bn& b) { return BnView{b.mean, b.std, b.w, b.b}; }

BatchMeta offsets_meta(const int32_t* node_off, const int32_t* edge_off) {
    BatchMeta m{};
    m.node_off = const_cast<int*>(node_off);
    m.edge_off = const_cast<int*>(edge_off);
    return m;
}

AggBwdArgs bwd_args(const hgnn_probe_agg_bwd_args& p) {
    AggBwdArgs a{};
    a.total_rows = p.total_rows;
    a.cap_rows = p.cap_rows;
    a.g = list_view(p.g);
    a.ing = p.ing;
    a.ldg = p.ldg;
    a.gofs = p.gofs;
    a.jtot = p.jtot;
    a.p = list_view(p.p);
    a.inp = p.inp;
    a.ldp = p.ldp;
    a.pofs_m = p.pofs_m;
    a.pofs_d = p.pofs_d;
    a.c = p.c;
    a.out = p.out;
    a.ldo = p.ldo;
    a.accumulate = p.accumulate;
    return a;
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

extern "C" {

int hgnn_probe_extract(hgnn_probe_extract_args* p, void* stream) {
    if (!p || !p->W || !p->mask || !p->n_batch || !p->node_off || !p->edge_off || !p->totals || !p->err ||
        p->bs <= 0 || p->nmax <= 0 || (p->xo && (!p->X || p->f <= 0)))
        return HGNN_ERR_ARG;
    const int nk = p->dual ? S_COUNT : 2;
    for (int k = 0; k < nk; ++k)
        if (!p->rows[k] || !p->entries[k]) return HGNN_ERR_ARG;
    if (p->dual && (!p->WL || !p->Pm || !p->Pd || !p->mask_lg || !p->e_batch || p->emax <= 0 || (p->xlo && !p->XL)))
        return HGNN_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    ExtractArgs a{};
    a.W = p->W;
    a.WL = p->dual ? p->WL : nullptr;
    a.Pm = p->dual ? p->Pm : nullptr;
    a.Pd = p->dual ? p->Pd : nullptr;
    a.mask = p->mask;
    a.mask_lg = p->dual ? p->mask_lg : nullptr;
    a.bs = p->bs;
    a.nmax = p->nmax;
    a.emax = p->dual ? p->emax : 0;
    a.jtot = p->jtot;
    a.meta.node_off = p->node_off;
    a.meta.edge_off = p->edge_off;
    a.meta.totals = p->totals;
    a.meta.err = p->err;
    for (int k = 0; k < nk; ++k) {
        a.rows[k] = reinterpret_cast<RowInfo*>(p->rows[k]);
        a.entries[k] = p->entries[k];
    }
    a.entry_stride_w = p->jtot <= 3 ? 4 : 8;  // program.hip build_program
    a.validate = p->validate;
    a.dual = p->dual ? 1 : 0;
    a.X = p->xo ? p->X : nullptr;
    a.XL = p->dual && p->xlo ? p->XL : nullptr;
    a.f = p->f;
    a.xo = p->xo;
    a.xlo = p->dual ? p->xlo : nullptr;
    p->variant = extract_variant(a);
    const int r = launch_plan(p->n_batch, p->dual ? p->e_batch : nullptr, p->bs, a.nmax, a.emax, a.meta, s);
    if (r) return r;
    return launch_extract(a, s);
}

int hgnn_probe_pack_nodes(const float* d_X, int bs, int f, int nmax, const int32_t* d_node_off, float* d_out,
                          void* stream) {
    if (!d_X || !d_node_off || !d_out || bs <= 0 || f <= 0 || nmax <= 0) return HGNN_ERR_ARG;
    return launch_pack_nodes(d_X, bs, f, nmax, offsets_meta(d_node_off, nullptr), d_out, (hipStream_t)stream);
}

int hgnn_probe_pack_edges(const float* d_XL, int bs, int emax, const int32_t* d_edge_off, float* d_out,
                          void* stream) {
    if (!d_XL || !d_edge_off || !d_out || bs <= 0 || emax <= 0) return HGNN_ERR_ARG;
    return launch_pack_edges(d_XL, bs, emax, offsets_meta(nullptr, d_edge_off), d_out, (hipStream_t)stream);
}

int hgnn_probe_unpack_nodes(const float* d_in, int bs, int f, int nmax, const int32_t* d_node_off, float* d_X,
                            void* stream) {
    if (!d_in || !d_node_off || !d_X || bs <= 0 || f <= 0 || nmax <= 0) return HGNN_ERR_ARG;
    return launch_unpack_nodes(d_in, bs, f, nmax, offsets_meta(d_node_off, nullptr), d_X, (hipStream_t)stream);
}

int hgnn_probe_agg_fwd(const hgnn_probe_agg_fwd_args* p, void* stream) {
    if (!p || !p->total_rows || !p->out) return HGNN_ERR_ARG;
    AggFwdArgs a{};
    a.total_rows = p->total_rows;
    a.cap_rows = p->cap_rows;
    a.g = list_view(p->g);
    a.xg = p->xg;
    a.cg = p->cg;
    a.jtot = p->jtot;
    a.gbn = bn_view(p->gbn);
    a.p = list_view(p->p);
    a.xp = p->xp;
    a.cp = p->cp;
    a.pbn = bn_view(p->pbn);
    a.out = p->out;
    a.ldo = p->ldo;
    a.pad_from = p->pad_from;
    a.j0 = p->j0;
    a.diag = reinterpret_cast<float2*>(p->diag);
    a.err = p->err;
    return launch_agg_fwd(a, (hipStream_t)stream);
}

int hgnn_probe_agg_bwd(const hgnn_probe_agg_bwd_args* a, const hgnn_probe_agg_bwd_args* b, int pair, void* stream) {
    if (!a || !a->total_rows || !a->out || (pair && (!b || !b->total_rows || !b->out))) return HGNN_ERR_ARG;
    if (!pair) return launch_agg_bwd(bwd_args(*a), (hipStream_t)stream);
    return launch_agg_bwd_pair(bwd_args(*a), bwd_args(*b), (hipStream_t)stream);
}

}  // extern "C"
