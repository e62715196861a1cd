// The executor's program: a network configuration as a fixed list of half-layers plus the readout, and the
// layout of the one caller-provided workspace every activation lives in (program.hip builds it; net.hip
// walks it forward and in reverse).
#pragma once

#include <vector>

#include "kernels.h"

namespace hgnn {

struct Feat {
    bool edge;
    int c;
    size_t z = 0, y = 0, grad = 0;
    bool has_y = false;
};

// "Aggregate these inputs": the G input gin (cg channels, jt operator slices) and, on a line graph, the P
// input pin (cp channels, Pm and Pd) of the other kind, into k = jt cg + 2 cp columns per row.  Every half
// starts with one; the readout is a node stage without a GEMM.
struct Stage {
    bool edge;
    int gin, pin;
    int cg, cp, k;
    size_t a = 0;  // the aggregate
    int lda = 0;   // its row stride: a half's kp (kp - 2 cg with id), the readout's k itself
};

struct Half : Stage {
    int out, bn;
    int pw_lin, pb_lin, pw_relu, pb_relu, pbn_w, pbn_b;
    int relu_from;
    int kp;  // row stride of the dA buffer and logical width of the GEMM operand (k rounded up to 4: float4 k)
    bool id = false;  // diagonal I / D columns (AggFwdArgs::j0 = 2): the aggregate holds slices 2.. and P only
    size_t part = 0, mean = 0, stdv = 0;
    size_t wt = 0, wc = 0, bc = 0;  // repacked Conv1d-pair weights (repack.hip)
    size_t wc3 = 0;                 // Wcat as three bf16 planes [3][2d][bf3_ld(kp)] (split-bf16 forward GEMM)
    size_t bnf = 0;                 // the forward GEMM's BN sums by fp64 atomics [BN_ACC_COPIES][2][2d] (HGNN_BN_ACC)
    size_t wt3 = 0;                 // WT as three bf16 planes [3][k][bf3_ld(c2p)] (split-bf16 dA GEMM)
};

// Buffer ring of the backward: a dY / bias-partial buffer (and, for the node halves whose dense dW the side
// stream reads, a dA buffer) per half, up to this many halves, so the main stream never waits mid-backward
// for the side stream's dW of an earlier half before reusing a buffer (config 2: 8 halves, no such joins)
constexpr int BWD_NBUF = 16;

struct Program {
    int cap_n = 0, cap_e = 0, jt = 0, d = 0, c2 = 0;
    int c2p = 0;  // 2d rounded up to 4: row stride of dY and of the repacked WT (dA GEMM's float4 k)
    std::vector<Feat> feats;
    std::vector<Half> halves;
    Stage readout{};
    int p_fcw = 0, p_fcb = 0;
    size_t colsum = 0;
    size_t diag_n = 0, diag_e = 0;  // per row (v_0, v_1) of the diagonal operator entry (diagonal I / D mode)
    size_t node_off = 0, edge_off = 0, totals = 0, err = 0;
    size_t rows[S_COUNT] = {}, ent[S_COUNT] = {};
    int entry_stride_w = 4;
    size_t da = 0, slabs = 0, bnb_part = 0, bnb_sums = 0, rb_scratch = 0;
    size_t bnb_acc[2] = {};  // BN-backward statistics accumulators (BnBwdArgs::acc64), ping-pong over the walk
    size_t acc_end = 0;      // end of the accumulator run (bnb_acc[0] .. the halves' bnf, the forward ticket)
    size_t fwd_ticket = 0;  // the forward GEMM's last-block finalize (FwdBnFin)
    int nbuf = 0;  // ring length: min(halves, BWD_NBUF)
    size_t dyk[BWD_NBUF] = {}, dbk[BWD_NBUF] = {}, dak[BWD_NBUF] = {};
    size_t bytes = 0;
};

// Parameter tensors (per layer and kind: two Conv1d weight / bias pairs and the BN pair; then fc) and BN
// layers of a valid configuration
inline int n_params(const hgnn_net_config* c) { return (c->kind == 1 ? 12 : 6) * (c->n_layers - 1) + 2; }
inline int n_bn(const hgnn_net_config* c) { return (c->kind == 1 ? 2 : 1) * (c->n_layers - 1); }

bool valid_config(const hgnn_net_config* c);
Program build_program(const hgnn_net_config* c);
// Program of a configuration, cached per host thread: built four times per training step
// otherwise (workspace query, forward, error word, backward), vectors included.
const Program& program_of(const hgnn_net_config* c);
// The GEMMs address each operand through a 32-bit buffer resource: every operand the
// program hands them must stay under 2 GB (checked before anything is enqueued).
bool fits_32bit(const Program& P);

template <typename T>
T* at(void* ws, size_t off) {
    return reinterpret_cast<T*>(static_cast<char*>(ws) + off);
}

// A layer output is kept pre-BN (y) only; its readers apply the BN of the half
// that produced it on load (BnView).  Inputs (feature 0, XL) are stored as is.
const Half* producer(const Program& P, int f);
const float* feat_src(const Program& P, void* ws, int f, const float* x0 = nullptr, const float* xl0 = nullptr);
BnView feat_bn(const Program& P, void* ws, const float* const* prm, int f);
// The diagonal I / D operand of a half's GEMMs (DiagIdArgs): its G input (pre-BN y, BN on load) and the row
// coefficients of its kind
DiagIdArgs diag_id_args(const Program& P, void* ws, const float* const* prm, const Half& h);

// Where a call's batch structure lives: the workspace (filled by the device
// extraction from the dense inputs) or a CSR batch image built on the host.
struct Src {
    BatchMeta m;
    StructView v[S_COUNT];
    const float* x0 = nullptr;   // packed node input (CSR batch) -- else feats[0].z
    const float* xl0 = nullptr;  // packed edge input (CSR batch) -- else feats[1].z
    long long nodes = 0;         // host node count (CSR batch)
};

BatchMeta meta_of(const Program& P, void* ws);
StructView view(const Program& P, void* ws, int kind);
Src make_src(const Program& P, void* ws, const hgnn_csr_batch* csr);

// The forward Conv1d-pair GEMM on bf16 MFMA with three-way split operands (gemm_bf3.hip: fp32 accuracy,
// 2.7x fewer MFMA cycles); HGNN_FWD_BF3=0: the fp32 MFMA kernels (launch_gemm3_fwd).  Line-graph networks
// with 2d % 64 == 0 (the kernel's 64-column tiles).
inline bool fwd_bf3_c2(int c2) { return switches().fwd_bf3 && c2 % 64 == 0; }
inline bool fwd_bf3(const Program& P) { return fwd_bf3_c2(P.c2); }
// the dA GEMM on the split-bf16 kernel (k_gemm_bf3_fwd with a plain-store epilogue, B = WT's planes)
inline bool da_bf3(const Program& P) { return switches().da_bf3 && P.c2p <= 128; }
// Diagonal I / D columns (round 6; HGNN_DIAG_ID=1: on, off by default -- measured 1.110 vs 1.105 ms per step in three
// of three alternating pairs at config 2: the aggregation lost 5 us per step, the forward and dW GEMMs' staging
// gained 11 and 14): graph_operators' slices 0 and 1 are I and diag(D)
// (functions/operators.py:19-23), so the aggregate's I / D column blocks are x̂ and D_r x̂ -- two of the five
// column blocks of a line-graph half at J = 1, written by the aggregation and read by the forward and dW GEMMs.
// In this mode the aggregation stores only slices 2.. and P (plus each row's diagonal coefficients) and the two
// split-bf16 GEMMs build the I / D columns from the half's input x̂ as they stage it (DiagIdArgs), the same
// values bit for bit.  For the halves whose G input is a BN'd layer output of 2d <= 256 channels (not the
// raw inputs of layer 0), with the split-bf16 forward and dW GEMMs.
inline bool diag_id_on(int c2) { return switches().diag_id && fwd_bf3_c2(c2) && dw_bf3_enabled() && c2 <= 256; }
// BN-backward statistics by fp64 atomics into accumulator copies, no k_bn_bwd_fin (round 6; HGNN_BN_ACC=0: the
// per-tile partials and k_bn_bwd_fin).  The sums' order over the tiles is not fixed: the statistics can differ in the
// last fp64 bits from run to run (a float flip of m1 / m2 once in ~1e9 values), where the fin path is bitwise
// deterministic.  The same switch puts the split-bf16 forward GEMM's BN sums on fp64 atomics (Half::bnf), so
// with the defaults the forward BN statistics are not bitwise repeatable from run to run either; HGNN_BN_ACC=0
// fixes both orders.
inline bool bn_acc_on() { return switches().bn_acc; }
// the forward BN finalize in the forward GEMM's last block (FwdBnFin; HGNN_BN_FWD_FIN=0: k_bn_finalize): 1.093 vs
// 1.106 ms median, five of five alternating pairs
inline bool bn_fwd_fin_on() { return switches().bn_fwd_fin; }

}  // namespace hgnn
