// Network executor: GNN_lg / GNN_simple forward and backward as one enqueue.
//
// The reference runs every layer as Python-level torch ops with per-graph
// Python loops (models/gnns/model_mnb.py:58-66 GNN_simple.forward, 124-129
// GNN_lg.forward, order switch 102-119; models/layers/layers_mnb.py).
// Here the network is a fixed "program" of half-layers derived from the
// config: each half = aggregate (agg_fwd) -> fused Conv1d pair GEMM with
// bias/ReLU/BN-partials epilogue -> BN finalize -> BN apply.  The last layer is
// aggregate -> segmented readout.  Backward walks the program in reverse.  All
// activations live in one caller-provided workspace laid out here, so a
// forward+backward is a fixed sequence of launches with no allocation and no
// host synchronisation (graph-capturable).
#include <vector>

#include "../../include/hgnn_amd.h"
#include "program.h"
#include "replay.h"
#include "timer.h"

namespace hgnn {
namespace {

// Side stream.  Backward: the weight-gradient GEMM of a half (and its slab
// reduction) only feeds the parameter grads, so it runs beside the dA -> dense dW
// -> aggregation-backward chain of the same half.  Fork after the half's BN
// backward, join before the next half's BN backward overwrites dY / the bias
// partials, and once more at the end.  One non-blocking stream and a few events
// per host thread and device, created on first use.
struct SideStream {
    int dev = -1;
    hipStream_t s = nullptr;
    hipEvent_t fork[2] = {nullptr, nullptr}, join[BWD_NBUF + 1] = {};  // join[BWD_NBUF]: the end of the backward
};

static int side_stream(hipStream_t caller, SideStream** out) {
    thread_local SideStream ss;
    // the device the caller's stream belongs to, not the thread's current device: the side
    // stream's kernels read and write the main stream's buffers
    hipDevice_t dev = 0;
    HGNN_HOST_CHECK(hipStreamGetDevice(caller, &dev));
    if (ss.dev != dev) {
        int cur = 0;
        HGNN_HOST_CHECK(hipGetDevice(&cur));
        HGNN_HOST_CHECK(hipSetDevice(dev));
        if (ss.s) {
            (void)hipStreamDestroy(ss.s);
            for (int i = 0; i < 2; ++i) (void)hipEventDestroy(ss.fork[i]);
            for (int i = 0; i <= BWD_NBUF; ++i) (void)hipEventDestroy(ss.join[i]);
        }
        ss = SideStream{};
        // (the HIP runtime maps a process's streams round-robin onto GPU_MAX_HW_QUEUES hardware queues: with an RCCL
        // process group's streams this one can land on the main stream's queue and run serialised with it -- 8 queues
        // avoid it; a high- or low-priority side stream made the host's launches slow, round 6)
        HGNN_HOST_CHECK(hipStreamCreateWithFlags(&ss.s, hipStreamNonBlocking));
        // fork / join events without the system-scope fence of a record (hipEventDisableSystemFence): the two
        // streams are on one device, so the producing kernel's end-of-kernel release and the consumer's
        // dispatch acquire already order the data, and the fence's cache writeback / invalidate only delays
        // the main stream's next kernel -- 1.163-1.169 vs 1.193-1.197 ms per step in three alternating pairs
        // (profiles/r05_ab_event_fence.txt); HGNN_EVENT_FENCE=1 restores the fenced records
        const unsigned ef = hipEventDisableTiming | (switches().event_fence ? 0u : hipEventDisableSystemFence);
        for (int i = 0; i < 2; ++i) HGNN_HOST_CHECK(hipEventCreateWithFlags(&ss.fork[i], ef));
        for (int i = 0; i < BWD_NBUF; ++i) HGNN_HOST_CHECK(hipEventCreateWithFlags(&ss.join[i], ef));
        // the end-of-backward join hands the side stream's final dW / bias gradients to the caller's stream,
        // whose next consumer may be a D2H copy (gloo DP) or a peer: that record keeps the system-scope
        // release (once per step)
        HGNN_HOST_CHECK(hipEventCreateWithFlags(&ss.join[BWD_NBUF], hipEventDisableTiming));
        ss.dev = dev;
        HGNN_HOST_CHECK(hipSetDevice(cur));
    }
    *out = &ss;
    return 0;
}

// The aggregation of a stage's inputs: a half's, or the readout's
static AggFwdArgs agg_fwd_args(const Program& P, const Src& src, void* ws, const float* const* prm, const Stage& st) {
    AggFwdArgs ag{};
    ag.total_rows = src.m.totals + (st.edge ? 1 : 0);
    ag.cap_rows = st.edge ? P.cap_e : P.cap_n;
    ag.g = src.v[st.edge ? S_WL : S_W];
    ag.xg = feat_src(P, ws, st.gin, src.x0, src.xl0);
    ag.gbn = feat_bn(P, ws, prm, st.gin);
    ag.cg = st.cg;
    ag.jtot = P.jt;
    if (st.pin >= 0) {
        ag.p = src.v[st.edge ? S_PE : S_PN];
        ag.xp = feat_src(P, ws, st.pin, src.x0, src.xl0);
        ag.pbn = feat_bn(P, ws, prm, st.pin);
        ag.cp = st.cp;
    }
    ag.out = at<float>(ws, st.a);
    ag.ldo = st.lda;
    return ag;
}

// The repack tables of the Conv1d pairs of every half: Wcat^T (forward B) and padded Wcat (dA B)
static std::vector<RepackTable> repack_tables(const Program& P, const float* const* prm, void* ws) {
    std::vector<RepackTable> tables;
    RepackTable rt{};
    rt.d = P.d;
    for (size_t hi = 0; hi < P.halves.size(); ++hi) {
        const Half& h = P.halves[hi];
        RepackItem& it = rt.it[rt.n++];
        it.wl = prm[h.pw_lin];
        it.wr = prm[h.pw_relu];
        it.bl = prm[h.pb_lin];
        it.br = prm[h.pb_relu];
        it.wt = at<float>(ws, h.wt);
        it.wc = at<float>(ws, h.wc);
        it.bc = at<float>(ws, h.bc);
        it.k = h.k;
        it.kp = h.kp;
        it.ldt = P.c2p;
        if (fwd_bf3(P)) {
            it.wc3 = at<__bf16>(ws, h.wc3);
            it.ldc3 = bf3_ld(h.kp);
        }
        if (da_bf3(P)) {
            it.wt3 = at<__bf16>(ws, h.wt3);
            it.ldt3 = bf3_ld(P.c2p);
        }
        if (rt.n == REPACK_MAX || hi + 1 == P.halves.size()) {
            tables.push_back(rt);
            rt.n = 0;
        }
    }
    return tables;
}

// One forward call: the batch structure, then the halves in program order, then the readout
struct FwdWalk {
    const hgnn_net_config* c;
    const Program& P;
    Src src;  // src.m also names the statistics accumulators the first kernel zeroes
    const float* const* prm;
    float* const* run;
    void* ws;
    hipStream_t s;
    Timer* tm;

    // Dense inputs: k_plan (offsets, totals, the error word and the accumulators zeroed; the first repack table
    // rides in its launch) and the extraction of the operators' structure and the packed inputs
    int extract(const hgnn_net_inputs* in, const RepackTable* first_table) {
        const bool lg = c->kind == 1;
        TL(HGNN_K_STRUCT, s, launch_plan(in->d_N_batch, lg ? in->d_E_batch : nullptr, c->bs, c->nmax,
                                         lg ? c->emax : 0, src.m, s, first_table));
        ExtractArgs ex{};
        ex.W = in->d_W;
        ex.WL = in->d_WL;
        ex.Pm = in->d_Pm;
        ex.Pd = in->d_Pd;
        ex.mask = in->d_mask;
        ex.mask_lg = in->d_mask_lg;
        ex.bs = c->bs;
        ex.nmax = c->nmax;
        ex.emax = lg ? c->emax : 0;
        ex.jtot = c->j_tot;
        ex.meta = src.m;
        for (int k = 0; k < S_COUNT; ++k) {
            ex.rows[k] = at<RowInfo>(ws, P.rows[k]);
            ex.entries[k] = at<float>(ws, P.ent[k]);
        }
        ex.entry_stride_w = P.entry_stride_w;
        ex.validate = 1;
        ex.dual = lg ? 1 : 0;
        ex.X = in->d_X;
        ex.f = c->f_in;
        ex.xo = at<float>(ws, P.feats[0].z);
        if (lg) {
            ex.XL = in->d_XL;
            ex.xlo = at<float>(ws, P.feats[1].z);
        }
        TL(HGNN_K_STRUCT, s, launch_extract(ex, s));
        return 0;
    }

    // One half: aggregate -> Conv1d-pair GEMM (bias, ReLU, BN partials) -> BN finalize
    int half(int hi) {
        const Half& h = P.halves[hi];
        const int cap = h.edge ? P.cap_e : P.cap_n;
        const int* tot = src.m.totals + (h.edge ? 1 : 0);
        AggFwdArgs ag = agg_fwd_args(P, src, ws, prm, h);
        if (h.id) {
            ag.j0 = 2;
            // the first diagonal-I / D half of its kind records the rows' diagonal coefficients
            bool first = true;
            for (int q = 0; q < hi; ++q) first = first && !(P.halves[q].id && P.halves[q].edge == h.edge);
            if (first) {
                ag.diag = at<float2>(ws, h.edge ? P.diag_e : P.diag_n);
                ag.err = src.m.err;
            }
        }
        TL(HGNN_K_AGG_FWD, s, launch_agg_fwd(ag, s));

        const DiagIdArgs ida = diag_id_args(P, ws, prm, h);
        // the BN statistics by fp64 atomics (split-bf16 forward GEMM, training)
        double* bnf = fwd_bf3(P) && c->training && bn_acc_on() ? at<double>(ws, h.bnf) : nullptr;
        FwdBnFin fbn{};
        const bool gfin = bnf && bn_fwd_fin_on();
        if (gfin) {
            fbn.mean = at<float>(ws, h.mean);
            fbn.std = at<float>(ws, h.stdv);
            fbn.run_mean = run ? run[2 * h.bn] : nullptr;
            fbn.run_std = run ? run[2 * h.bn + 1] : nullptr;
            fbn.momentum = 0.1f;
            fbn.ticket = at<unsigned>(ws, P.fwd_ticket);
        }
        float* y = at<float>(ws, P.feats[h.out].y);
        float* part = c->training ? at<float>(ws, h.part) : nullptr;
        if (fwd_bf3(P))
            TL(HGNN_K_GEMM_FWD, s,
               launch_gemm_bf3_fwd(at<float>(ws, h.a), h.lda, tot, cap, h.kp, at<__bf16>(ws, h.wc3),
                                   (long long)P.c2 * bf3_ld(h.kp), bf3_ld(h.kp), P.c2, at<float>(ws, h.bc),
                                   h.relu_from, y, P.c2, part, s, h.id ? &ida : nullptr, bnf, gfin ? &fbn : nullptr));
        else
            TL(HGNN_K_GEMM_FWD, s,
               launch_gemm3_fwd(at<float>(ws, h.a), h.kp, tot, cap, h.kp, at<float>(ws, h.wc), h.kp, P.c2,
                                at<float>(ws, h.bc), h.relu_from, y, P.c2, part, s, c->kind == 1 ? 1 : 0));
        if (gfin) return 0;

        BnFwdArgs bf{};
        bf.acc = bnf;
        bf.part = at<float>(ws, h.part);
        bf.tiles = gemm_fwd_tiles_m(cap);
        bf.c = P.c2;
        bf.count = tot;
        bf.w = prm[h.pbn_w];
        bf.b = prm[h.pbn_b];
        bf.mean = at<float>(ws, h.mean);
        bf.std = at<float>(ws, h.stdv);
        bf.run_mean = run ? run[2 * h.bn] : nullptr;
        bf.run_std = run ? run[2 * h.bn + 1] : nullptr;
        bf.training = c->training;
        bf.momentum = 0.1f;
        TL(HGNN_K_BN_FWD, s, launch_bn_finalize(bf, s));
        return 0;
    }

    int readout(float* out) {
        const Stage& ro = P.readout;
        TL(HGNN_K_AGG_FWD, s, launch_agg_fwd(agg_fwd_args(P, src, ws, prm, ro), s));
        TL(HGNN_K_READOUT, s, launch_readout_fwd(at<float>(ws, ro.a), ro.k, src.m.node_off, c->bs, c->nmax, prm[P.p_fcw],
                                                 prm[P.p_fcb], c->dim_out, at<float>(ws, P.colsum), out, s));
        return 0;
    }
};

int net_forward(const hgnn_net_config* c, const hgnn_net_inputs* in, const hgnn_csr_batch* csr,
                const float* const* prm, float* const* run, void* ws, float* out, hipStream_t s, Timer* tm) {
    const Program& P = program_of(c);
    if (!fits_32bit(P)) return HGNN_ERR_UNSUPPORTED;
    if (!c->training && !run) return HGNN_ERR_ARG;  // eval mode normalises with the running statistics
    FwdWalk w{c, P, make_src(P, ws, csr), prm, run, ws, s, tm};
    // The forward's first kernel zeroes the statistics accumulators, the backward's two regions and the halves'
    // (k_plan; a CSR batch: a memset beside the error word's)
    BatchMeta& m = w.src.m;
    if (bn_acc_on()) {
        m.zero64 = at<double>(ws, P.bnb_acc[0]);
        m.zero64_n = (int)((P.acc_end - P.bnb_acc[0]) / sizeof(double));
    }
    const std::vector<RepackTable> tables = repack_tables(P, prm, ws);
    // the first table rides in k_plan's launch (dense inputs), the rest (> REPACK_MAX halves, or a CSR
    // batch) are launches of their own
    size_t plan_tables = 0;
    if (csr) {  // dense inputs: k_plan zeroes both
        HGNN_HOST_CHECK(hipMemsetAsync(m.err, 0, sizeof(uint32_t), s));
        if (m.zero64) HGNN_HOST_CHECK(hipMemsetAsync(m.zero64, 0, (size_t)m.zero64_n * sizeof(double), s));
    } else {
        plan_tables = tables.empty() ? 0 : 1;
        TRY(w.extract(in, tables.empty() ? nullptr : &tables[0]));
    }
    for (size_t t = plan_tables; t < tables.size(); ++t) TL(HGNN_K_STRUCT, s, launch_repack(tables[t], s));
    for (int hi = 0; hi < (int)P.halves.size(); ++hi) TRY(w.half(hi));
    return w.readout(out);
}

// One backward call: the readout, then the halves in reverse program order, then the join and dX.  The
// weight-gradient work runs on the side stream beside the main stream's dA -> aggregation-backward chain.
struct BwdWalk {
    const hgnn_net_config* c;
    const hgnn_net_inputs* in;
    const Program& P;
    const Src src;
    const float* const* prm;
    void* ws;
    const float* dout;
    float* const* grads;
    float* dX;
    float* dW;
    void* const* ev;  // per-layer completion events (hgnn_net_backward_ex)
    int n_ev;
    Timer* tm;
    hipStream_t s;     // the caller's stream
    SideStream* side;  // nullptr with HGNN_SIDE=0
    hipStream_t rs = s;  // stream of the readout's parameter gradients and dense dW
    const bool need_dw = c->need_dw != 0;
    // HGNN_SERIAL_BWD=1 (diagnostics): all on the main stream, so a kernel trace shows each kernel's own duration
    const bool serial_bwd = switches().serial_bwd;
    // HGNN_BWD_TAIL=0: the round-4 tail (the last half forks after its dA GEMM, dX unpacked after the join)
    const bool bwd_tail = switches().bwd_tail;
    // dY, the bias partials and the side-read dA of the q-th half (of the reverse walk) live in ring slot
    // q % nbuf, so the side stream's dW of an earlier half may still read its slot while the main stream runs
    // the next halves; the main stream waits for the side stream only where a slot comes round again (more
    // than BWD_NBUF halves) and once at the end.  (Two alternating slots and a join per half before round 4:
    // each mid-backward join idles the main stream.)
    bool pending[BWD_NBUF] = {};
    int slot = 0, q = 0;
    std::vector<char> init = std::vector<char>(P.feats.size(), 0);  // per feature: its gradient buffer is written

    const int* total(bool edge) const { return src.m.totals + (edge ? 1 : 0); }
    int cap(bool edge) const { return edge ? P.cap_e : P.cap_n; }
    bool needs_grad(int f) const {
        if (f < 0) return false;
        if (f == 0) return c->need_dx != 0;
        if (c->kind == 1 && f == 1) return false;  // XL never requires grad (scripts/train_mnb.py:56-66)
        return true;
    }

    // dense dW contribution of one graph_oper(W, X_l): G block of dA (node rows) x X_l
    DwDenseArgs dw_args(int gin, const float* da, int lda, bool readout, int accumulate) const {
        DwDenseArgs a{};
        a.dA = da;
        a.lda = lda;
        a.f = P.feats[gin].c;
        a.jt = P.jt;
        if (gin == 0) {
            a.xdense = in->d_X;
        } else {
            a.xp = feat_src(P, ws, gin, src.x0, src.xl0);
            const BnView v = feat_bn(P, ws, prm, gin);
            a.pmean = v.mean;
            a.pstd = v.std;
            a.pw = v.w;
            a.pb = v.b;
        }
        if (readout) {
            a.dout = dout;
            a.fcw = prm[P.p_fcw];
            a.dim_out = c->dim_out;
            a.kfc = P.readout.k;
        }
        a.node_off = src.m.node_off;
        a.bs = c->bs;
        a.nmax = c->nmax;
        a.dW = dW;
        a.accumulate = accumulate;
        return a;
    }

    // The aggregation backward of a stage from its dA (row stride ldd) into the gradients of its G input (ng)
    // and its P input (np): one paired launch, or the one that is needed
    int agg_bwd(const Stage& st, const float* da, int ldd, bool ng, bool np) {
        AggBwdArgs gab{}, pab{};
        if (ng) {
            gab.total_rows = total(st.edge);
            gab.cap_rows = cap(st.edge);
            gab.g = src.v[st.edge ? S_WLT : S_WT];
            gab.ing = da;
            gab.ldg = ldd;
            gab.gofs = 0;
            gab.jtot = P.jt;
            gab.c = st.cg;
            gab.out = at<float>(ws, P.feats[st.gin].grad);
            gab.ldo = st.cg;
            gab.accumulate = init[st.gin];
        }
        if (np) {  // the rows of the other kind
            pab.total_rows = total(!st.edge);
            pab.cap_rows = cap(!st.edge);
            pab.p = src.v[st.edge ? S_PN : S_PE];
            pab.inp = da;
            pab.ldp = ldd;
            pab.pofs_m = P.jt * st.cg;
            pab.pofs_d = P.jt * st.cg + st.cp;
            pab.jtot = P.jt;
            pab.c = st.cp;
            pab.out = at<float>(ws, P.feats[st.pin].grad);
            pab.ldo = st.cp;
            pab.accumulate = init[st.pin];
        }
        if (ng && np) TL(HGNN_K_AGG_BWD, s, launch_agg_bwd_pair(gab, pab, s));
        else if (ng) TL(HGNN_K_AGG_BWD, s, launch_agg_bwd(gab, s));
        else if (np) TL(HGNN_K_AGG_BWD, s, launch_agg_bwd(pab, s));
        if (ng) init[st.gin] = 1;
        if (np) init[st.pin] = 1;
        return 0;
    }

    ReadoutAggArgs readout_agg_args(bool lgr, bool lpr) const {
        const Stage& ro = P.readout;
        ReadoutAggArgs ra{};
        ra.dout = dout;
        ra.fcw = prm[P.p_fcw];
        ra.dim_out = c->dim_out;
        ra.k = ro.k;
        ra.jt = P.jt;
        ra.cg = ro.cg;
        ra.cp = ro.cp;
        ra.bs = c->bs;
        ra.node_off = src.m.node_off;
        ra.edge_off = src.m.edge_off;
        ra.g = src.v[S_WT];
        ra.g_total = total(false);
        ra.g_cap = P.cap_n;
        ra.g_out = lgr ? at<float>(ws, P.feats[ro.gin].grad) : nullptr;
        ra.g_acc = init[ro.gin];
        if (lpr) {
            ra.p = src.v[S_PE];
            ra.p_total = total(true);
            ra.p_cap = P.cap_e;
            ra.p_out = at<float>(ws, P.feats[ro.pin].grad);
            ra.p_acc = init[ro.pin];
        }
        return ra;
    }

    int readout() {
        const Stage& ro = P.readout;
        // the readout's parameter gradients and its dense dW only feed gradients: on the side stream, forked
        // here, beside the main stream's readout aggregation backward and first halves
        if (side && !serial_bwd) {
            HGNN_HOST_CHECK(hipEventRecord(side->fork[1], s));
            HGNN_HOST_CHECK(hipStreamWaitEvent(side->s, side->fork[1], 0));
            rs = side->s;
        }
        TL(HGNN_K_READOUT, rs,
           launch_readout_bwd_params(dout, at<float>(ws, P.colsum), c->bs, c->nmax, c->dim_out, ro.k, grads[P.p_fcw],
                                     grads[P.p_fcb], at<void>(ws, P.rb_scratch), rs));
        const bool lgr = needs_grad(ro.gin), lpr = needs_grad(ro.pin);
        if (!lgr && !lpr && !need_dw) return 0;
        const ReadoutAggArgs ra = readout_agg_args(lgr, lpr);
        const DwDenseArgs dwr = need_dw ? dw_args(ro.gin, nullptr, 0, true, 0) : DwDenseArgs{};
        // HGNN_READOUT_ROW=0: the readout gradient materialised as a [rows][K] buffer and gathered.  The
        // readout-row kernels hold a graph's rows in LDS: configurations beyond it (wide 2d with a large
        // Nmax / Emax) take the materialised form as well.
        if (switches().readout_row && readout_row_fits(ra, need_dw ? &dwr : nullptr)) {
            if (need_dw) TL(HGNN_K_DW_DENSE, rs, launch_dw_readout(dwr, rs));
            // the readout class (k_readout_agg_bwd: R_b broadcast, no dA read), not agg_bwd: the aggregation
            // class and its HBM roofline are the k_agg_bwd gathers of the halves
            if (lgr || lpr) TL(HGNN_K_READOUT, s, launch_readout_agg_bwd(ra, s));
            if (lgr) init[ro.gin] = 1;
            if (lpr) init[ro.pin] = 1;
            return 0;
        }
        float* da = at<float>(ws, P.da);
        TL(HGNN_K_READOUT, s,
           launch_readout_bwd_da(dout, src.m.node_off, c->bs, P.cap_n, total(false), prm[P.p_fcw], c->dim_out, ro.k, da, s));
        if (need_dw) TL(HGNN_K_DW_DENSE, s, launch_dw_dense(dw_args(ro.gin, da, ro.k, true, 0), s));
        return agg_bwd(ro, da, ro.k, lgr, lpr);
    }

    // The weight-gradient GEMM of a half and its slab reduction, forked onto the side stream.
    // The side stream also takes the dense operator gradient (W.requires_grad) of a node
    // half: it only accumulates into dW, so it leaves the dA -> aggregation-backward chain.
    // (Measured alternative, not kept: the gather half of the aggregation backward on a third
    // stream, overlapping the next half -- 268K vs 286K graphs/s: the concurrent memory-bound
    // kernels only slowed each other.)
    int fork_dw(const Half& h, float* dyb, float* dbp, bool dense_dw, float* dab) {
        const int nz = dw3_chunks(cap(h.edge), P.c2, h.k);
        if (side) {
            HGNN_HOST_CHECK(hipEventRecord(side->fork[q & 1], s));
            HGNN_HOST_CHECK(hipStreamWaitEvent(side->s, side->fork[q & 1], 0));
        }
        const hipStream_t d = side && !serial_bwd ? side->s : s;
        if (dense_dw) TL(HGNN_K_DW_DENSE, d, launch_dw_dense(dw_args(h.gin, dab, h.kp, false, 1), d));
        // dY rows have stride c2p; the dW GEMM's float4 loads along the 2d outputs read the zero
        // padding of an odd 2d and store only the 2d real rows of each slab
        const DiagIdArgs ida = diag_id_args(P, ws, prm, h);
        TL(HGNN_K_GEMM_DW, d,
           launch_gemm3_dw(dyb, P.c2p, at<float>(ws, h.a), h.lda, total(h.edge), cap(h.edge), P.c2, h.k, nz,
                           at<float>(ws, P.slabs), d, h.id ? &ida : nullptr));
        TL(HGNN_K_DW_REDUCE, d,
           launch_dw_reduce2(at<float>(ws, P.slabs), total(h.edge), nz, P.c2, P.c2, h.k, P.d, grads[h.pw_lin],
                             grads[h.pw_relu], dbp, grads[h.pb_lin], grads[h.pb_relu], d));
        // a join only where the slot comes round again (the end of the backward has its own)
        pending[slot] = side && q + P.nbuf < (int)P.halves.size();
        if (pending[slot]) HGNN_HOST_CHECK(hipEventRecord(side->join[slot], d));
        return 0;
    }

    BnBwdArgs bn_bwd_args(const Half& h, float* dyb, float* dbp) const {
        BnBwdArgs bb{};
        bb.y = at<float>(ws, P.feats[h.out].y);
        bb.dz = at<float>(ws, P.feats[h.out].grad);
        bb.total_rows = total(h.edge);
        bb.cap_rows = cap(h.edge);
        bb.c = P.c2;
        bb.mean = at<float>(ws, h.mean);
        bb.std = at<float>(ws, h.stdv);
        bb.w = prm[h.pbn_w];
        bb.relu_from = h.relu_from;
        bb.training = c->training;
        bb.part = at<float>(ws, P.bnb_part);
        bb.sums = at<float>(ws, P.bnb_sums);
        bb.dy = dyb;
        bb.dw = grads[h.pbn_w];
        bb.db = grads[h.pbn_b];
        bb.dbpart = dbp;
        bb.ldy = P.c2p;
        if (bn_acc_on()) {  // ping-pong: apply4 of this half zeroes the next half's region
            bb.acc64 = at<double>(ws, P.bnb_acc[q % 2]);
            bb.acc64_zero = at<double>(ws, P.bnb_acc[(q + 1) % 2]);
        }
        return bb;
    }

    // Half hi, the q-th of the walk: BN backward -> dA GEMM -> aggregation backward, its dW forked beside them
    int half(int hi) {
        const Half& h = P.halves[hi];
        // the walk leaves region H % 2 zeroed; with an odd number of halves region 0 is not, so a second backward of
        // the same forward (retain_graph) would meet the first one's sums: zeroed here
        if (q == 0 && bn_acc_on() && P.halves.size() % 2 == 1)
            HGNN_HOST_CHECK(hipMemsetAsync(at<double>(ws, P.bnb_acc[0]), 0, (size_t)bn_acc_doubles(P.c2) * sizeof(double), s));
        float* dyb = at<float>(ws, P.dyk[slot]);
        float* dbp = at<float>(ws, P.dbk[slot]);
        if (pending[slot]) {  // the dW nbuf halves back still reads this slot
            HGNN_HOST_CHECK(hipStreamWaitEvent(s, side->join[slot], 0));
            pending[slot] = false;
        }
        if (!init[h.out]) HGNN_HOST_CHECK(hipMemsetAsync(at<float>(ws, P.feats[h.out].grad), 0,
                                                          (size_t)cap(h.edge) * P.c2 * sizeof(float), s));
        TL(HGNN_K_BN_BWD, s, launch_bn_backward(bn_bwd_args(h, dyb, dbp), s));

        const bool ng = needs_grad(h.gin), np = needs_grad(h.pin);
        const bool ndw = need_dw && !h.edge;
        if (!ng && !np && !ndw) return fork_dw(h, dyb, dbp, false, nullptr);
        // the side stream's dense dW reads a node half's dA: its own slot buffer; other halves share P.da
        float* da = at<float>(ws, ndw && side && P.dak[slot] ? P.dak[slot] : P.da);
        // the last half of the walk (no dense dW, which reads dA) forks before its dA GEMM: the side stream's
        // dW + reduce is the step's tail there, nothing on the main stream follows to overlap it
        const bool early = side && hi == 0 && !ndw && bwd_tail;
        if (early) TRY(fork_dw(h, dyb, dbp, false, nullptr));
        if (da_bf3(P))
            TL(HGNN_K_GEMM_DA, s,
               launch_gemm_bf3_da(dyb, P.c2p, total(h.edge), cap(h.edge), P.c2p, at<__bf16>(ws, h.wt3),
                                  (long long)h.k * bf3_ld(P.c2p), bf3_ld(P.c2p), h.k, da, h.kp, s));
        else
            TL(HGNN_K_GEMM_DA, s,
               launch_gemm3_da(dyb, P.c2p, total(h.edge), cap(h.edge), P.c2p, at<float>(ws, h.wt), P.c2p, h.k, da,
                               h.kp, s));
        // dW starts once dA is done: two MFMA GEMMs side by side only slow each other,
        // dW beside the latency-bound dense-dW / aggregation-backward kernels does not
        if (!early) TRY(fork_dw(h, dyb, dbp, ndw, da));
        return agg_bwd(h, da, h.kp, ng, np);
    }

    void next() { slot = ++q % P.nbuf; }

    // per-layer completion events (hgnn_net_backward_ex): recorded once the first half (in program
    // order) of a layer -- the last one the reverse walk reaches -- has been enqueued
    int mark(int hi) {
        const bool lgk = c->kind == 1;
        if (!ev || n_ev <= 0 || (lgk && hi % 2 != 0)) return 0;
        const int l = lgk ? hi / 2 : hi;
        if (2 * l + 1 >= n_ev) return 0;
        HGNN_HOST_CHECK(hipEventRecord(static_cast<hipEvent_t>(ev[2 * l]), s));
        HGNN_HOST_CHECK(hipEventRecord(static_cast<hipEvent_t>(ev[2 * l + 1]), side ? side->s : s));
        return 0;
    }

    int join_side() {  // the side stream runs in order: its last work done means all of it is
        if (side) {
            HGNN_HOST_CHECK(hipEventRecord(side->join[BWD_NBUF], side->s));
            HGNN_HOST_CHECK(hipStreamWaitEvent(s, side->join[BWD_NBUF], 0));
        }
        return 0;
    }

    int finish(bool csr) {
        // dX reads only the main stream's aggregation gradients: unpacked before the join (HGNN_BWD_TAIL=0: after)
        if (!bwd_tail) TRY(join_side());
        if (c->need_dx) {
            if (!dX) return HGNN_ERR_ARG;
            float* g0 = at<float>(ws, P.feats[0].grad);
            if (!init[0]) HGNN_HOST_CHECK(hipMemsetAsync(g0, 0, (size_t)P.cap_n * c->f_in * sizeof(float), s));
            if (csr)
                HGNN_HOST_CHECK(hipMemcpyAsync(dX, g0, (size_t)src.nodes * c->f_in * sizeof(float),
                                               hipMemcpyDeviceToDevice, s));
            else
                TL(HGNN_K_STRUCT, s, launch_unpack_nodes(g0, c->bs, c->f_in, c->nmax, src.m, dX, s));
        }
        if (bwd_tail) TRY(join_side());
        return 0;
    }
};

int net_backward(const hgnn_net_config* c, const hgnn_net_inputs* in, const hgnn_csr_batch* csr,
                 const float* const* prm, void* ws, const float* dout, float* const* grads, float* dX, float* dW,
                 hipStream_t s, Timer* tm, void* const* ev = nullptr, int n_ev = 0) {
    const Program& P = program_of(c);
    if (!fits_32bit(P)) return HGNN_ERR_UNSUPPORTED;
    if (c->need_dw && (!dW || !in || !in->d_X || csr)) return HGNN_ERR_ARG;
    SideStream* side = nullptr;
    // HGNN_SIDE=0: the weight-gradient work stays on the main stream, with no events at all (a
    // cross-stream event record / wait costs the main stream ~6-7 us of idle GPU per fork)
    if (switches().side) TRY(side_stream(s, &side));
    BwdWalk w{c, in, P, make_src(P, ws, csr), prm, ws, dout, grads, dX, dW, ev, n_ev, tm, s, side};
    TRY(w.readout());
    for (int hi = (int)P.halves.size() - 1; hi >= 0; --hi, w.next()) {
        TRY(w.half(hi));
        TRY(w.mark(hi));
    }
    return w.finish(csr != nullptr);
}

static int forward_call(const hgnn_net_config* c, const hgnn_net_inputs* in, const hgnn_csr_batch* csr,
                        const float* const* prm, float* const* run, void* ws, float* out, hipStream_t s) {
    if (!replay_eligible(c)) return net_forward(c, in, csr, prm, run, ws, out, s, nullptr);
    KeyBuilder k;
    k.add('F');
    k.cfg(c);
    k.inputs(in);
    k.csr(csr);
    k.ptrs(prm, n_params(c));
    k.ptrs(run, 2 * n_bn(c));
    k.ptr(ws);
    k.ptr(out);
    return replayed(std::move(k.k), s,
                    [&](hipStream_t st) { return net_forward(c, in, csr, prm, run, ws, out, st, nullptr); });
}

static int backward_call(const hgnn_net_config* c, const hgnn_net_inputs* in, const hgnn_csr_batch* csr,
                         const float* const* prm, void* ws, const float* dout, float* const* grads, float* dX,
                         float* dW, hipStream_t s) {
    if (!replay_eligible(c)) return net_backward(c, in, csr, prm, ws, dout, grads, dX, dW, s, nullptr);
    KeyBuilder k;
    k.add('B');
    k.cfg(c);
    k.inputs(in);
    k.csr(csr);
    k.ptrs(prm, n_params(c));
    k.ptr(ws);
    k.ptr(dout);
    k.ptrs(grads, n_params(c));
    k.ptr(dX);
    k.ptr(dW);
    return replayed(std::move(k.k), s, [&](hipStream_t st) {
        return net_backward(c, in, csr, prm, ws, dout, grads, dX, dW, st, nullptr);
    });
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

extern "C" {

int hgnn_abi_version(void) { return HGNN_ABI_VERSION; }

const char* hgnn_status_string(int status) {
    switch (status) {
        case HGNN_OK: return "ok";
        case HGNN_ERR_ARG: return "invalid argument";
        case HGNN_ERR_UNSUPPORTED: return "unsupported configuration";
        case HGNN_ERR_HIP: return "HIP runtime error";
        case HGNN_ERR_INDEX: return "index out of range";
        default: return "unknown status";
    }
}

int hgnn_net_param_count(const hgnn_net_config* cfg) {
    if (!valid_config(cfg)) return -1;
    return n_params(cfg);
}

int hgnn_net_bn_count(const hgnn_net_config* cfg) {
    if (!valid_config(cfg)) return -1;
    return n_bn(cfg);
}

size_t hgnn_net_workspace_bytes(const hgnn_net_config* cfg) {
    if (!valid_config(cfg)) return 0;
    const Program& P = program_of(cfg);
    return fits_32bit(P) ? P.bytes : 0;
}

uint32_t* hgnn_net_error_word(const hgnn_net_config* cfg, void* workspace) {
    if (!valid_config(cfg) || !workspace) return nullptr;
    return at<uint32_t>(workspace, program_of(cfg).err);
}

int hgnn_net_forward(const hgnn_net_config* cfg, const hgnn_net_inputs* in, const float* const* params,
                     float* const* bn_running, void* workspace, float* d_out, void* stream) {
    if (!valid_config(cfg) || !in || !params || !workspace || !d_out) return HGNN_ERR_ARG;
    if (!in->d_X || !in->d_W || !in->d_N_batch || !in->d_mask) return HGNN_ERR_ARG;
    if (cfg->kind == 1 && (!in->d_XL || !in->d_WL || !in->d_Pm || !in->d_Pd || !in->d_E_batch || !in->d_mask_lg))
        return HGNN_ERR_ARG;
    return forward_call(cfg, in, nullptr, params, bn_running, workspace, d_out, static_cast<hipStream_t>(stream));
}

int hgnn_net_backward(const hgnn_net_config* cfg, const hgnn_net_inputs* in, const float* const* params,
                      void* workspace, const float* d_dout, float* const* grads, float* d_dX, float* d_dW,
                      void* stream) {
    if (!valid_config(cfg) || !params || !workspace || !d_dout || !grads) return HGNN_ERR_ARG;
    return backward_call(cfg, in, nullptr, params, workspace, d_dout, grads, d_dX, d_dW,
                         static_cast<hipStream_t>(stream));
}

int hgnn_net_forward_timed(const hgnn_net_config* cfg, const hgnn_net_inputs* in, const float* const* params,
                           float* const* bn_running, void* workspace, float* d_out, void* stream, void* timer) {
    if (!valid_config(cfg) || !in || !params || !workspace || !d_out) return HGNN_ERR_ARG;
    return net_forward(cfg, in, nullptr, params, bn_running, workspace, d_out, static_cast<hipStream_t>(stream),
                       static_cast<Timer*>(timer));
}

int hgnn_net_backward_timed(const hgnn_net_config* cfg, const hgnn_net_inputs* in, const float* const* params,
                            void* workspace, const float* d_dout, float* const* grads, float* d_dX, float* d_dW,
                            void* stream, void* timer) {
    if (!valid_config(cfg) || !params || !workspace || !d_dout || !grads) return HGNN_ERR_ARG;
    return net_backward(cfg, in, nullptr, params, workspace, d_dout, grads, d_dX, d_dW,
                        static_cast<hipStream_t>(stream), static_cast<Timer*>(timer));
}

static bool csr_matches(const hgnn_net_config* cfg, const hgnn_csr_batch* b) {
    if (!b || !b->d_node_off || !b->d_totals || !b->d_x || !b->d_rows[S_W] || !b->d_rows[S_WT]) return false;
    if (cfg->kind == 1 && (!b->d_xl || !b->d_rows[S_WL] || !b->d_rows[S_WLT] || !b->d_rows[S_PN] || !b->d_rows[S_PE]))
        return false;
    return b->stride_w == (cfg->j_tot <= 3 ? 4 : 8);
}

int hgnn_csr_batch_view(const hgnn_csr_layout* L, const void* d_base, hgnn_csr_batch* out) {
    if (!L || !d_base || !out) return HGNN_ERR_ARG;
    const char* b = static_cast<const char*>(d_base);
    hgnn_csr_batch r{};
    r.d_node_off = b + L->off_node_off;
    r.d_edge_off = b + L->off_edge_off;
    r.d_totals = b + L->off_totals;
    r.d_n_batch = reinterpret_cast<const int64_t*>(b + L->off_n_batch);
    r.d_e_batch = reinterpret_cast<const int64_t*>(b + L->off_e_batch);
    r.d_x = reinterpret_cast<const float*>(b + L->off_x);
    r.d_xl = reinterpret_cast<const float*>(b + L->off_xl);
    for (int k = 0; k < S_COUNT; ++k) {
        r.d_rows[k] = b + L->off_rows[k];
        r.d_entries[k] = reinterpret_cast<const float*>(b + L->off_entries[k]);
    }
    r.stride_w = L->stride_w;
    r.nodes = L->nodes;
    r.edges = L->edges;
    *out = r;
    return HGNN_OK;
}

int hgnn_net_forward_csr(const hgnn_net_config* cfg, const hgnn_csr_batch* batch, const float* const* params,
                         float* const* bn_running, void* workspace, float* d_out, void* stream) {
    if (!valid_config(cfg) || !csr_matches(cfg, batch) || !params || !workspace || !d_out) return HGNN_ERR_ARG;
    return forward_call(cfg, nullptr, batch, params, bn_running, workspace, d_out, static_cast<hipStream_t>(stream));
}

int hgnn_net_backward_ex(const hgnn_net_config* cfg, const hgnn_net_inputs* in, const hgnn_csr_batch* csr,
                         const float* const* params, void* workspace, const float* d_dout, float* const* grads,
                         float* d_dX, float* d_dW, void* stream, void* timer, void* const* events, int n_events) {
    if (!valid_config(cfg) || !params || !workspace || !d_dout || !grads) return HGNN_ERR_ARG;
    if (csr && (!csr_matches(cfg, csr) || cfg->need_dw)) return HGNN_ERR_ARG;
    if (!csr && cfg->need_dw && (!in || !in->d_X)) return HGNN_ERR_ARG;
    if (n_events < 0 || (n_events > 0 && !events)) return HGNN_ERR_ARG;
    if (!timer && n_events == 0)
        return backward_call(cfg, in, csr, params, workspace, d_dout, grads, d_dX, d_dW, static_cast<hipStream_t>(stream));
    return net_backward(cfg, in, csr, params, workspace, d_dout, grads, d_dX, d_dW, static_cast<hipStream_t>(stream),
                        static_cast<Timer*>(timer), events, n_events);
}

int hgnn_net_backward_csr(const hgnn_net_config* cfg, const hgnn_csr_batch* batch, const float* const* params,
                          void* workspace, const float* d_dout, float* const* grads, float* d_dX, void* stream) {
    if (!valid_config(cfg) || !csr_matches(cfg, batch) || !params || !workspace || !d_dout || !grads)
        return HGNN_ERR_ARG;
    if (cfg->need_dw) return HGNN_ERR_ARG;
    return backward_call(cfg, nullptr, batch, params, workspace, d_dout, grads, d_dX, nullptr,
                         static_cast<hipStream_t>(stream));
}

}  // extern "C"
