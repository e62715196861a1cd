// The program of a configuration and its workspace layout (program.h).
#include "program.h"

#include <string.h>

#include <algorithm>

namespace hgnn {
namespace {

struct Bump {
    static constexpr size_t ALIGN = 256;
    size_t top = 0;
    size_t take(size_t n) {
        const size_t o = top;
        top += (n + ALIGN - 1) / ALIGN * ALIGN;
        return o;
    }
};

}  // namespace

bool valid_config(const hgnn_net_config* c) {
    if (!c) return false;
    if (c->kind != 0 && c->kind != 1) return false;
    if (c->bs <= 0 || c->nmax <= 0 || c->f_in <= 0 || c->d <= 0 || c->n_layers < 2) return false;
    if (c->dim_out <= 0) return false;
    if (c->kind == 1 && (c->emax < 0 || c->order < 1 || c->order > 3)) return false;
    if (c->j_tot < 3 || c->j_tot > 7) return false;  // entries of 8 floats: column + up to 7 slices
    if (2 * c->d > 512) return false;
    const long long capn = (long long)c->bs * c->nmax;
    const long long cape = (long long)c->bs * (c->kind == 1 ? c->emax : 0);
    if (capn * c->nmax > (1ll << 31) - 1) return false;
    if (cape * (c->emax > c->nmax ? c->emax : c->nmax) > (1ll << 31) - 1) return false;
    return true;
}

Program build_program(const hgnn_net_config* c) {
    Program P;
    const bool lg = c->kind == 1;
    P.cap_n = c->bs * c->nmax;
    P.cap_e = lg ? c->bs * c->emax : 0;
    P.jt = c->j_tot;
    P.d = c->d;
    P.c2 = 2 * c->d;
    P.c2p = (P.c2 + 3) / 4 * 4;
    P.entry_stride_w = c->j_tot <= 3 ? 4 : 8;
    const int L = c->n_layers;

    auto add_feat = [&](bool edge, int ch) {
        Feat f;
        f.edge = edge;
        f.c = ch;
        P.feats.push_back(f);
        return (int)P.feats.size() - 1;
    };
    add_feat(false, c->f_in);
    if (lg) add_feat(true, 1);
    int in_n = 0, in_e = lg ? 1 : -1;
    for (int l = 0; l < L - 1; ++l) {
        if (lg) {
            const int pb = 12 * l;
            const int out_n = add_feat(false, P.c2);
            const int out_e = add_feat(true, P.c2);
            P.feats[out_n].has_y = P.feats[out_e].has_y = true;
            Half hn{}, he{};
            hn.edge = false;
            hn.gin = in_n;
            hn.cg = P.feats[in_n].c;
            hn.out = out_n;
            hn.bn = 2 * l;
            hn.pw_relu = pb + 0;
            hn.pb_relu = pb + 1;
            hn.pw_lin = pb + 2;
            hn.pb_lin = pb + 3;
            hn.pbn_w = pb + 4;
            hn.pbn_b = pb + 5;
            hn.relu_from = c->d;
            he.edge = true;
            he.gin = in_e;
            he.cg = P.feats[in_e].c;
            he.out = out_e;
            he.bn = 2 * l + 1;
            he.pw_relu = pb + 6;
            he.pb_relu = pb + 7;
            he.pw_lin = pb + 8;
            he.pb_lin = pb + 9;
            he.pbn_w = pb + 10;
            he.pbn_b = pb + 11;
            he.relu_from = c->d;
            if (c->order == 1) {  // node first; edge half reads the BN'd node output
                hn.pin = in_e;
                he.pin = out_n;
            } else if (c->order == 2) {  // edge first; node half reads the BN'd edge output
                he.pin = in_n;
                hn.pin = out_e;
            } else {  // independent halves
                hn.pin = in_e;
                he.pin = in_n;
            }
            hn.cp = P.feats[hn.pin].c;
            he.cp = P.feats[he.pin].c;
            hn.k = P.jt * hn.cg + 2 * hn.cp;
            he.k = P.jt * he.cg + 2 * he.cp;
            if (c->order == 2) {
                P.halves.push_back(he);
                P.halves.push_back(hn);
            } else {
                P.halves.push_back(hn);
                P.halves.push_back(he);
            }
            in_n = out_n;
            in_e = out_e;
        } else {
            const int pb = 6 * l;
            const int out_n = add_feat(false, P.c2);
            P.feats[out_n].has_y = true;
            Half h{};
            h.edge = false;
            h.gin = in_n;
            h.cg = P.feats[in_n].c;
            h.pin = -1;
            h.cp = 0;
            h.k = P.jt * h.cg;
            h.out = out_n;
            h.bn = l;
            // layer_simple: cat(relu(cv2(x)), relu(cv1(x))) -> both halves ReLU (layers_mnb.py:59-65)
            h.pw_lin = pb + 2;
            h.pb_lin = pb + 3;
            h.pw_relu = pb + 0;
            h.pb_relu = pb + 1;
            h.pbn_w = pb + 4;
            h.pbn_b = pb + 5;
            h.relu_from = 0;
            P.halves.push_back(h);
            in_n = out_n;
        }
    }
    for (Half& h : P.halves) {
        bool prod = false;
        for (const Half& o : P.halves) prod = prod || o.out == h.gin;
        h.id = diag_id_on(P.c2) && prod && h.cg == P.c2 && (h.pin < 0 || h.cp == P.c2);
    }
    Stage& ro = P.readout;
    ro.edge = false;
    ro.gin = in_n;
    ro.pin = lg ? in_e : -1;
    ro.cg = P.feats[in_n].c;
    ro.cp = lg ? P.feats[in_e].c : 0;
    ro.k = P.jt * ro.cg + 2 * ro.cp;
    ro.lda = ro.k;  // not rounded up to 4 as a half's kp is
    P.p_fcw = n_params(c) - 2;
    P.p_fcb = n_params(c) - 1;

    // ---- workspace layout
    Bump B;
    P.node_off = B.take(sizeof(int) * (c->bs + 1));
    P.edge_off = B.take(sizeof(int) * (c->bs + 1));
    P.totals = B.take(sizeof(int) * 4);
    P.err = B.take(sizeof(uint32_t) * 4);
    const int nmax = c->nmax, emax = lg ? c->emax : 0;
    const size_t sw = P.entry_stride_w * sizeof(float);
    P.rows[S_W] = B.take(sizeof(RowInfo) * P.cap_n);
    P.ent[S_W] = B.take((size_t)P.cap_n * nmax * sw);
    P.rows[S_WT] = B.take(sizeof(RowInfo) * P.cap_n);
    P.ent[S_WT] = B.take((size_t)P.cap_n * nmax * sw);
    if (lg) {
        P.rows[S_WL] = B.take(sizeof(RowInfo) * P.cap_e);
        P.ent[S_WL] = B.take((size_t)P.cap_e * emax * sw);
        P.rows[S_WLT] = B.take(sizeof(RowInfo) * P.cap_e);
        P.ent[S_WLT] = B.take((size_t)P.cap_e * emax * sw);
        P.rows[S_PN] = B.take(sizeof(RowInfo) * P.cap_n);
        P.ent[S_PN] = B.take((size_t)P.cap_n * emax * 16);
        P.rows[S_PE] = B.take(sizeof(RowInfo) * P.cap_e);
        P.ent[S_PE] = B.take((size_t)P.cap_e * nmax * 16);
    }
    for (auto& f : P.feats) {
        const size_t cap = f.edge ? P.cap_e : P.cap_n;
        if (f.has_y) f.y = B.take(cap * f.c * sizeof(float));
        else f.z = B.take(cap * f.c * sizeof(float));
        f.grad = B.take(cap * f.c * sizeof(float));
    }
    size_t max_da = 0, max_slab = 0;
    int max_cap = 0;
    for (auto& h : P.halves) {
        const int cap = h.edge ? P.cap_e : P.cap_n;
        h.kp = (h.k + 3) / 4 * 4;
        h.lda = h.id ? h.kp - 2 * h.cg : h.kp;
        h.a = B.take((size_t)cap * h.lda * sizeof(float));
        h.part = B.take((size_t)gemm_fwd_tiles_m(cap) * P.c2 * 3 * sizeof(float));
        h.mean = B.take(P.c2 * sizeof(float));
        h.stdv = B.take(P.c2 * sizeof(float));
        h.wt = B.take((size_t)h.k * P.c2p * sizeof(float));
        h.wc = B.take((size_t)P.c2 * h.kp * sizeof(float));
        h.bc = B.take((size_t)P.c2 * sizeof(float));
        h.wc3 = B.take((size_t)3 * P.c2 * bf3_ld(h.kp) * 2);
        h.wt3 = B.take((size_t)3 * h.k * bf3_ld(P.c2p) * 2);
        max_da = std::max(max_da, (size_t)cap * h.kp);
        max_slab = std::max(max_slab, dw3_slab_floats(cap, P.c2, h.k));
        max_cap = std::max(max_cap, cap);
    }
    // ring slot q % nbuf for the q-th half of the backward's walk (the last half first)
    P.nbuf = std::max(1, std::min((int)P.halves.size(), BWD_NBUF));
    for (int i = 0; i < P.nbuf; ++i) {
        P.dbk[i] = B.take((size_t)bn_bwd_tiles(max_cap > 0 ? max_cap : 1) * P.c2 * sizeof(float));
        P.dyk[i] = B.take((size_t)max_cap * P.c2p * sizeof(float));
        size_t na = 0;  // the node halves of this slot (their dA is read by the side stream's dense dW)
        for (int q = i; q < (int)P.halves.size(); q += P.nbuf) {
            const Half& h = P.halves[P.halves.size() - 1 - q];
            if (!h.edge) na = std::max(na, (size_t)P.cap_n * h.kp);
        }
        if (na) P.dak[i] = B.take(na * sizeof(float));
    }
    P.diag_n = B.take((size_t)P.cap_n * sizeof(float2));
    if (lg) P.diag_e = B.take((size_t)P.cap_e * sizeof(float2));
    ro.a = B.take((size_t)P.cap_n * ro.k * sizeof(float));
    P.colsum = B.take((size_t)c->bs * ro.k * sizeof(float));
    max_da = std::max(max_da, (size_t)P.cap_n * ro.k);
    P.da = B.take(max_da * sizeof(float));  // dA of the halves the side stream does not read, and the readout's
    P.slabs = B.take(max_slab * sizeof(float));
    P.bnb_part = B.take((size_t)bn_bwd_tiles(max_cap) * P.c2 * 4 * sizeof(float));
    // the statistics accumulators, one contiguous run zeroed by the forward's first kernel: the backward's two
    // ping-pong regions, then one forward region per half
    for (int i = 0; i < 2; ++i) P.bnb_acc[i] = B.take((size_t)bn_acc_doubles(P.c2) * sizeof(double));
    for (auto& h : P.halves) h.bnf = B.take((size_t)BN_ACC_COPIES * 2 * P.c2 * sizeof(double));
    P.fwd_ticket = B.take(sizeof(unsigned));
    P.acc_end = B.top;
    P.bnb_sums = B.take((size_t)P.c2 * 4 * sizeof(float));
    P.rb_scratch = B.take(readout_bwd_scratch_bytes(c->dim_out, ro.k));
    P.bytes = B.top;
    return P;
}

const Program& program_of(const hgnn_net_config* c) {
    struct Entry {
        int key[11];
        Program P;
    };
    thread_local std::vector<Entry> cache;
    const int key[11] = {c->kind, c->order, c->bs, c->nmax, c->emax, c->f_in, c->d, c->n_layers, c->j_tot,
                         c->dim_out, c->training};
    for (const Entry& e : cache)
        if (memcmp(e.key, key, sizeof(key)) == 0) return e.P;
    if (cache.size() >= 16) cache.erase(cache.begin());
    cache.push_back(Entry{});
    memcpy(cache.back().key, key, sizeof(key));
    cache.back().P = build_program(c);
    return cache.back().P;
}

bool fits_32bit(const Program& P) {
    const long long lim = (1ll << 31) - 1;
    for (const Half& h : P.halves) {
        const long long cap = h.edge ? P.cap_e : P.cap_n;
        if (cap * h.kp * 4 > lim || cap * P.c2p * 4 > lim || (long long)P.c2p * h.kp * 4 > lim) return false;
    }
    return (long long)P.cap_n * P.readout.k * 4 <= lim;
}

const Half* producer(const Program& P, int f) {
    for (const Half& h : P.halves)
        if (h.out == f) return &h;
    return nullptr;
}

const float* feat_src(const Program& P, void* ws, int f, const float* x0, const float* xl0) {
    if (f == 0 && x0) return x0;
    if (f == 1 && xl0 && P.feats[1].edge && !P.feats[1].has_y) return xl0;
    return P.feats[f].has_y ? at<float>(ws, P.feats[f].y) : at<float>(ws, P.feats[f].z);
}

BnView feat_bn(const Program& P, void* ws, const float* const* prm, int f) {
    BnView v{};
    const Half* h = producer(P, f);
    if (!h) return v;
    v.mean = at<float>(ws, h->mean);
    v.std = at<float>(ws, h->stdv);
    v.w = prm[h->pbn_w];
    v.b = prm[h->pbn_b];
    return v;
}

DiagIdArgs diag_id_args(const Program& P, void* ws, const float* const* prm, const Half& h) {
    DiagIdArgs d{};
    if (!h.id) return d;
    d.x = feat_src(P, ws, h.gin);
    d.ldx = P.feats[h.gin].c;
    d.c = h.cg;
    d.diag = at<float2>(ws, h.edge ? P.diag_e : P.diag_n);
    d.bn = feat_bn(P, ws, prm, h.gin);
    return d;
}

BatchMeta meta_of(const Program& P, void* ws) {
    BatchMeta m;
    m.node_off = at<int>(ws, P.node_off);
    m.edge_off = at<int>(ws, P.edge_off);
    m.totals = at<int>(ws, P.totals);
    m.err = at<uint32_t>(ws, P.err);
    return m;
}

StructView view(const Program& P, void* ws, int kind) {
    StructView v;
    v.rows = at<RowInfo>(ws, P.rows[kind]);
    v.entries = at<float>(ws, P.ent[kind]);
    v.stride = (kind == S_PN || kind == S_PE) ? 4 : P.entry_stride_w;
    return v;
}

Src make_src(const Program& P, void* ws, const hgnn_csr_batch* csr) {
    Src r;
    r.m = meta_of(P, ws);
    for (int k = 0; k < S_COUNT; ++k) r.v[k] = view(P, ws, k);
    if (csr) {
        r.m.node_off = const_cast<int*>(static_cast<const int*>(csr->d_node_off));
        r.m.edge_off = const_cast<int*>(static_cast<const int*>(csr->d_edge_off));
        r.m.totals = const_cast<int*>(static_cast<const int*>(csr->d_totals));
        for (int k = 0; k < S_COUNT; ++k) {
            r.v[k].rows = static_cast<const RowInfo*>(csr->d_rows[k]);
            r.v[k].entries = csr->d_entries[k];
            r.v[k].stride = (k == S_PN || k == S_PE) ? 4 : csr->stride_w;
        }
        r.x0 = csr->d_x;
        r.xl0 = csr->d_xl;
        r.nodes = csr->nodes;
    }
    return r;
}

}  // namespace hgnn
