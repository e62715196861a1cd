/*
 * hgnn_amd.h -- C ABI of the MI355X (gfx950) message-passing hot path.
 *
 * Drop-in boundary: these entry points are what the reference's nn.Module
 * forward()/backward() calls become.  The reference is pure Python/PyTorch
 * (SURVEY.md §0.1), so the Python layer in hgnn-2_amd/ (same import paths as
 * the reference: models.gnns.model_mnb, models.layers.*, functions.*) binds
 * this ABI through ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - every pointer named d_* is device memory (HBM) owned by the caller;
 *  - fp32 tensors are dense, contiguous, in the reference's layouts:
 *      X  (bs, f, Nmax)        node features, channel-major (functions/batching.py:116, 172-174)
 *      XL (bs, 1, Emax)        line-graph input = diag(WL[:, :, 1]) (functions/batching.py:119, 171)
 *      W  (bs, Nmax, Nmax, J+2)  graph operators (functions/operators.py:19-29)
 *      WL (bs, Emax, Emax, J+2)  line-graph operators (functions/operators.py:39-81)
 *      Pm, Pd (bs, Nmax, Emax)   incidence operators (functions/operators.py:43-66)
 *      mask (bs, Nmax, Nmax), mask_lg (bs, Emax, Emax)  (functions/batching.py:113-114, 182-183)
 *      N_batch, E_batch (bs,) int64  (functions/batching.py:99-103)
 *  - outputs are caller-allocated; scratch comes from a caller-allocated
 *    workspace whose size is queried first (no allocation inside any call, so
 *    every call can be captured into a hipGraph);
 *  - `stream` is a hipStream_t passed as void*; every call only enqueues work;
 *  - return value: 0 = HGNN_OK, otherwise an HGNN_ERR_* code (the Python layer
 *    raises RuntimeError, the reference's error behaviour);
 *  - device-side input validation (operator entries outside a graph's real
 *    block, mask/N_batch disagreement) ORs HGNN_DEVERR_* bits into a uint32
 *    word inside the workspace; hgnn_*_error_word() gives its device address.
 *  - no global mutable state: calls are re-entrant, one stream per call.
 *
 * Size limits (a call outside them returns HGNN_ERR_UNSUPPORTED or HGNN_ERR_ARG before anything
 * is enqueued, or -- for data-dependent bounds -- sets a device error bit; the reference has no
 * such limits, the Python layer raises RuntimeError):
 *  - networks: J + 2 in [3, 7] (J <= 5; operator values exact below 2^24 as in the reference's fp32 powers); any d with 2d <= 512 (odd 2d runs the same MFMA GEMMs over a
 *    row stride padded to 4); the GEMMs address each operand through a 32-bit buffer resource,
 *    so every per-call operand must stay under 2 GB -- about 12 K QM9-shape graphs per call at
 *    d = 64 (the 640-wide edge aggregate is the largest; split larger batches); the dense
 *    operator gradient (need_dw) keeps a graph's rows in LDS: Nmax <= ~1200 at J + 2 = 3;
 *  - CCN: receptive-field degree <= 1024 (CCN-1D) / 256 (CCN-2D), f_in and hidden <= 16
 *    (HGNN_DEVERR_CCN_DEGREE for the degree, an error status for the channel counts).
 */
#ifndef HGNN_AMD_H
#define HGNN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HGNN_ABI_VERSION 1

#define HGNN_OK 0
#define HGNN_ERR_ARG 1          /* invalid argument: null pointer, bad size   */
#define HGNN_ERR_UNSUPPORTED 2  /* configuration not compiled (e.g. J > 3)    */
#define HGNN_ERR_HIP 3          /* HIP launch / runtime failure               */
#define HGNN_ERR_INDEX 4        /* input the reference rejects with IndexError */

#define HGNN_DEVERR_PAD_NONZERO 0x1u  /* operator entry outside the real block */
#define HGNN_DEVERR_MASK 0x2u         /* mask[:, :, 0] != (n < N_batch[b])      */
#define HGNN_DEVERR_SIZES 0x4u        /* N_batch > Nmax, E_batch > Emax, < 0   */
#define HGNN_DEVERR_CCN_SELFLOOP 0x8u /* CCN adjacency lacks a self loop        */
#define HGNN_DEVERR_CCN_DEGREE 0x10u  /* CCN degree above the compiled bound    */
#define HGNN_DEVERR_CCN_ASYM 0x20u    /* CCN adjacency pattern not symmetric    */
#define HGNN_DEVERR_DIAG_ID 0x40u     /* operator slice 0 / 1 (I, D) not diagonal */
#define HGNN_DEVERR_CLASS_TARGET 0x80u /* CCN loop: class target not an integer in [0, n_out) */

int hgnn_abi_version(void);
const char* hgnn_status_string(int status);

/* The HGNN_* kernel switches as the library read them from the environment, once, at its first use of any of
 * them (INTEGRATION.md lists them).  Host-only, read-only: no GPU needed.  Flags report 0 / 1; the tri-state
 * HGNN_EXEC_GRAPH and HGNN_BN_BWD2 report -1 (unset), 0 or 1; integer switches their value after range checking. */
const char* hgnn_switch_name(int i);                 /* NULL past the last row */
int hgnn_switch_value(const char* name, int* value); /* HGNN_OK, or HGNN_ERR_ARG for an unknown name */

/* ------------------------------------------------------------------------
 * Network executor: GNN_lg.forward / GNN_simple.forward + autograd backward.
 *
 * Replaces models/gnns/model_mnb.py:58-66 (GNN_simple.forward) and
 * models/gnns/model_mnb.py:124-129 (GNN_lg.forward) with every layer
 * (models/layers/layers_mnb.py:52-69, 88-95, 189-225, 256-290, 322-358,
 * 379-388), BN (models/layers/batch_normalization.py:34-108) and the
 * aggregation ops graph_oper / P_multi (layers_mnb.py:391-434) fused into one
 * enqueue; hgnn_net_backward is the autograd backward of the same graph
 * (scripts/train_mnb.py:90).
 * ---------------------------------------------------------------------- */
typedef struct hgnn_net_config {
    int32_t kind;      /* 0 = GNN_simple, 1 = GNN_lg                              */
    int32_t order;     /* GNN_lg update order 1, 2, 3 (model_mnb.py:102-119)      */
    int32_t bs;        /* graphs in the batch                                     */
    int32_t nmax;      /* padded node count Nmax (X.shape[2])                     */
    int32_t emax;      /* padded edge-slot count Emax (XL.shape[2]); 0 for simple */
    int32_t f_in;      /* dim_input (X.shape[1])                                  */
    int32_t d;         /* n_features                                              */
    int32_t n_layers;  /* >= 2: layer0, n_layers-2 middle layers, layerlast       */
    int32_t j_tot;     /* J + 2 operator slices (W.shape[3])                      */
    int32_t dim_out;   /* dim_output                                              */
    int32_t training;  /* 1: batch BN statistics + running-stat update; 0: eval   */
    int32_t need_dx;   /* backward: write dX (bs, f_in, nmax)                     */
    int32_t need_dw;   /* backward: write dense dW (bs, nmax, nmax, j_tot)        */
    int32_t reserved;
} hgnn_net_config;

typedef struct hgnn_net_inputs {
    const float* d_X;
    const float* d_XL;       /* NULL for GNN_simple */
    const float* d_W;
    const float* d_WL;       /* NULL for GNN_simple */
    const float* d_Pm;       /* NULL for GNN_simple */
    const float* d_Pd;       /* NULL for GNN_simple */
    const int64_t* d_N_batch;
    const int64_t* d_E_batch; /* NULL for GNN_simple */
    const float* d_mask;
    const float* d_mask_lg;   /* NULL for GNN_simple */
} hgnn_net_inputs;

/* Parameter pointer order (device fp32, contiguous), per layer l = 0..n_layers-2:
 *   GNN_lg:     cv1.w cv1.b cv2.w cv2.b bn1.w bn1.b cv3.w cv3.b cv4.w cv4.b bn2.w bn2.b
 *   GNN_simple: cv1.w cv1.b cv2.w cv2.b bn1.w bn1.b
 * then layerlast.fc.w layerlast.fc.b.  BN weight/bias are 0-dim (scalar) tensors
 * (batch_normalization.py:26-27).  Count: hgnn_net_param_count(). */
int hgnn_net_param_count(const hgnn_net_config* cfg);

/* Running BN statistics, per BN module in the order above (bn1, bn2 per layer):
 * running_mean then running_std, each (2 d,).  Updated in place in training
 * mode as r = 0.9 * batch + 0.1 * r (batch_normalization.py:37-38); read in
 * eval mode (batch_normalization.py:41). */
int hgnn_net_bn_count(const hgnn_net_config* cfg);

size_t hgnn_net_workspace_bytes(const hgnn_net_config* cfg);

/* Device address of the validation word inside `workspace` (uint32). */
uint32_t* hgnn_net_error_word(const hgnn_net_config* cfg, void* workspace);

/* out: (bs, dim_out).  The workspace keeps what backward needs; it must stay
 * untouched between a forward and its backward. */
int hgnn_net_forward(const hgnn_net_config* cfg, const hgnn_net_inputs* in,
                     const float* const* params, float* const* bn_running,
                     void* workspace, float* d_out, void* stream);

/* d_dout: (bs, dim_out).  grads: same order/shapes as params; every gradient
 * buffer is OVERWRITTEN.  d_dX (bs, f_in, nmax) if cfg->need_dx, d_dW
 * (bs, nmax, nmax, j_tot) if cfg->need_dw (else may be NULL). */
int hgnn_net_backward(const hgnn_net_config* cfg, const hgnn_net_inputs* in,
                      const float* const* params, void* workspace,
                      const float* d_dout, float* const* grads,
                      float* d_dX, float* d_dW, void* stream);

struct hgnn_csr_batch;  /* defined below (native sparse batcher) */

/* Extended backward: the batch comes from `in` (dense) or `csr` (exactly one non-NULL), an
 * optional launch timer, and optional per-layer completion events for overlapping a gradient
 * all-reduce with the rest of the backward: events[2 l] is recorded on `stream`
 * and events[2 l + 1] on the executor's side stream once every gradient of layer l
 * (l = 0 .. n_layers - 2; layerlast.fc counts as layer n_layers - 2) has been enqueued on
 * that stream -- a communication stream that waits on both may reduce layer l's gradients
 * while layers < l are still being differentiated.  events: hipEvent_t handles;
 * n_events = 2 (n_layers - 1), or 0 for none. */
int hgnn_net_backward_ex(const hgnn_net_config* cfg, const hgnn_net_inputs* in,
                         const struct hgnn_csr_batch* csr, const float* const* params,
                         void* workspace, const float* d_dout, float* const* grads,
                         float* d_dX, float* d_dW, void* stream, void* timer,
                         void* const* events, int n_events);

/* Kernel classes for the optional launch timer (bench.py measures the
 * dominant kernel class and the aggregation classes inside timed regions of
 * its own steps).  A timer times every launch of a class in `class_mask`
 * (bit k = class k) in one of three modes (hgnn_timer_create_ex):
 *   HGNN_TIMER_STAMPS    the aggregation and GEMM kernels write a 100 MHz
 *                        s_memrealtime stamp per wave at entry and exit into
 *                        the timer's device buffer (2 words per wave, stamp_words
 *                        in all); a launch lasts max(exit) - min(entry).  Nothing
 *                        is added to the stream, so a timed kernel runs as in an
 *                        untimed step; classes without stamp slots are not timed;
 *   HGNN_TIMER_DISPATCH  an event pair bound to each dispatch (hipExtLaunchKernel):
 *                        every class, but the timed dispatch runs slower;
 *   HGNN_TIMER_MARKERS   event records on the stream around each launch call.
 * hgnn_timer_create: DISPATCH (MARKERS with HGNN_TIMER_MARKERS=1). */
#define HGNN_TIMER_STAMPS 0
#define HGNN_TIMER_DISPATCH 1
#define HGNN_TIMER_MARKERS 2
#define HGNN_K_STRUCT 0    /* plan, dense->list extraction, pack/unpack */
#define HGNN_K_AGG_FWD 1   /* aggregation gather (graph_oper + P_multi)  */
#define HGNN_K_GEMM_FWD 2  /* fused Conv1d pair GEMM + bias/ReLU/BN partials */
#define HGNN_K_BN_FWD 3    /* BN finalize + apply                         */
#define HGNN_K_READOUT 4   /* readout forward/backward                    */
#define HGNN_K_BN_BWD 5
#define HGNN_K_GEMM_DW 6
#define HGNN_K_GEMM_DA 7
#define HGNN_K_AGG_BWD 8
#define HGNN_K_DW_DENSE 9  /* dense operator gradient dW (W.requires_grad) */
#define HGNN_K_DW_REDUCE 10 /* dW slab + bias reductions                    */
void* hgnn_timer_create(int max_launches, unsigned class_mask);
void* hgnn_timer_create_ex(int max_launches, unsigned class_mask, int mode, long long stamp_words);
void hgnn_timer_reset(void* timer);
/* Waits for the timed work (stamp mode: a device synchronisation and one copy of
 * the stamp buffer); sums the durations of class `kernel_class`. */
int hgnn_timer_elapsed(void* timer, int kernel_class, double* total_ms, int* launches);
/* Stamp mode: every timed launch in enqueue order -- its class, its first-entry / last-exit times in us
 * from the region's earliest stamp (-1: no stamp) and (stream_idx, optional) the stream it went to, numbered
 * in order of first appearance.  Returns the number of launches (up to `max` written), or minus an
 * HGNN_ERR_* code. */
int hgnn_timer_launches(void* timer, int max, int* cls, double* t_entry_us, double* t_exit_us, int* stream_idx);
/* Stamp mode: the entry / exit times (us from the region's earliest stamp, -1: none) of every wave of timed
 * launch `launch` (enqueue order), in the kernel's wave order (linear block id x waves per block + wave).
 * Returns the launch's wave count (up to `max` written), or minus an HGNN_ERR_* code.  (Diagnostics:
 * tools/wave_stats.py.) */
long long hgnn_timer_waves(void* timer, int launch, long long max, double* entry_us, double* exit_us);
void hgnn_timer_destroy(void* timer);
int hgnn_net_forward_timed(const hgnn_net_config* cfg, const hgnn_net_inputs* in,
                           const float* const* params, float* const* bn_running,
                           void* workspace, float* d_out, void* stream, void* timer);
int hgnn_net_backward_timed(const hgnn_net_config* cfg, const hgnn_net_inputs* in,
                            const float* const* params, void* workspace,
                            const float* d_dout, float* const* grads,
                            float* d_dX, float* d_dW, void* stream, void* timer);

/* ------------------------------------------------------------------------
 * Native operator builder and sparse batcher (host C++, csrc/builder.cpp).
 *
 * hgnn_graph_operators replaces graph_operators (functions/operators.py:11-83,
 * twin preprocessing/preprocessing.py:100-170): dense per-graph W (n, n, J+2) and,
 * with dual, WL (m, m, J+2), Pm, Pd (n, m), m = hgnn_graph_edge_slots(n, A) =
 * nnz(A) incl. the diagonal.  Bit-exact, edge-slot quirk included.  Returns
 * HGNN_ERR_INDEX where the reference raises IndexError.
 *
 * hgnn_csr_batch_plan / _build replace prepare_batch (functions/batching.py:77-185)
 * for the executor: a batch of graphs (A_b (n_b, n_b), X_b (n_b, f_in) row-major,
 * host memory) goes straight into one host image holding the packed operator row
 * lists the executor walks, packed X / XL and the batch offsets.  Plan gives the
 * layout (byte offsets, sizes); build fills an image of layout.bytes bytes; the
 * caller copies it to the device and describes it with hgnn_csr_batch_view.
 * ---------------------------------------------------------------------- */
typedef struct hgnn_csr_layout {
    int32_t bs, nmax, emax, f_in, j_tot, dual, stride_w, reserved;
    int64_t nodes, edges;      /* packed node rows, packed edge-slot rows          */
    int64_t rows[6], nnz[6];   /* per list kind: W, WT, WL, WLT, PN (node->slot), PE */
    int64_t off_node_off, off_edge_off, off_totals, off_n_batch, off_e_batch, off_x, off_xl;
    int64_t off_rows[6], off_entries[6];
    int64_t bytes;
} hgnn_csr_layout;
int hgnn_graph_edge_slots(int n, const float* A);
int hgnn_graph_operators(int n, const float* A, int J, int dual, float* W, int m, float* WL,
                         float* Pm, float* Pd);
int hgnn_csr_batch_plan(int bs, const int* n_nodes, const float* const* A, int f_in, int J, int dual,
                        hgnn_csr_layout* layout);
int hgnn_csr_batch_build(int bs, const int* n_nodes, const float* const* A, const float* const* X,
                         int f_in, int J, int dual, const hgnn_csr_layout* layout, void* image);

/* Device view of a CSR batch image (d_base = its device copy). */
typedef struct hgnn_csr_batch {
    const void* d_node_off;    /* int32 (bs + 1) */
    const void* d_edge_off;    /* int32 (bs + 1) */
    const void* d_totals;      /* int32 [nodes, edges] */
    const int64_t* d_n_batch;  /* (bs,) */
    const int64_t* d_e_batch;
    const float* d_x;          /* packed [nodes][f_in] */
    const float* d_xl;         /* packed [edges] */
    const void* d_rows[6];
    const float* d_entries[6];
    int32_t stride_w, reserved;
    int64_t nodes, edges;
} hgnn_csr_batch;
int hgnn_csr_batch_view(const hgnn_csr_layout* layout, const void* d_base, hgnn_csr_batch* out);

/* The executor on a CSR batch: cfg->bs / nmax / emax / f_in / j_tot from the
 * layout; no dense operator, mask or padding is read (no plan / extraction
 * pass).  Backward: need_dw must be 0 (there is no dense W); d_dX is packed
 * [nodes][f_in]. */
int hgnn_net_forward_csr(const hgnn_net_config* cfg, const hgnn_csr_batch* batch,
                         const float* const* params, float* const* bn_running,
                         void* workspace, float* d_out, void* stream);
int hgnn_net_backward_csr(const hgnn_net_config* cfg, const hgnn_csr_batch* batch,
                          const float* const* params, void* workspace,
                          const float* d_dout, float* const* grads, float* d_dX, void* stream);

/* ------------------------------------------------------------------------
 * Device batcher (csrc/batcher.hip): the image hgnn_csr_batch_build writes on the host, built on the
 * device from a resident graph pack -- byte for byte the same image, so everything that runs on a CSR
 * batch runs on it unchanged.
 *
 * The pack is hgnn_amd.dataset.GraphPack's arrays in device memory: node_off (graphs + 1) int64, x
 * (nodes, f_in) fp32, adj_off (graphs + 1) int64, adj_ij (adj_nnz, 2) int32 local (i, j) in strictly
 * ascending row-major order per graph, adj_w (adj_nnz) fp32, targets (not read here).
 *
 * One workgroup builds one graph in LDS; J <= 3, and supported per graph: with dual, n <= 32 nodes and
 * m = nnz(A) <= 72 edge slots; without dual (the node-graph family W, WT, x alone) n <= 64 nodes, any
 * nnz(A).  hgnn_pack_count runs the builder in its counting mode over the whole pack, once
 * per (pack, J, dual), and writes one record of HGNN_PACK_COUNT_WORDS int32 per graph:
 *   {n, m (0 without dual), nnz[W, WT, WL, WLT, PN, PE], flags, 0}
 * A flagged graph's record holds no counts.  The caller reads the records back once, gathers those of a
 * batch on the host and sizes the image with hgnn_csr_layout_from_counts (no GPU call; the layout
 * hgnn_csr_batch_plan gives for the same graphs: both form the offsets in one function).
 * hgnn_csr_batch_build_device then enqueues, with no host synchronisation: the image's memset, the
 * batch-offset kernel (node_off, edge_off, totals, N_batch, E_batch and each graph's entry starts) and
 * the per-graph build.  d_counts are the records hgnn_pack_count wrote for this view, J and dual; d_idx
 * (bs) int32 the batch's graph indices (repeats allowed).  If the records of d_idx do not add up to
 * `layout`, an index is outside the pack or a record is flagged, nothing but zeros and offsets is
 * written (the kernels never write past the layout).  Without dual, a batch whose largest graph
 * (layout->nmax) has at most 32 nodes is built by the same kernel as a dual batch's node family; a
 * larger one by the 64-node instantiation.  The records do not depend on which of them counted.
 * ---------------------------------------------------------------------- */
#define HGNN_PACK_COUNT_WORDS 10
#define HGNN_PACK_FLAG_BOUNDS 1 /* the host batcher takes it.  dual: n not in [1, 32] or m > 72; else n not in [1, 64] */
#define HGNN_PACK_FLAG_INDEX 2  /* the edge-slot index error (hgnn_csr_batch_plan: HGNN_ERR_INDEX) */
#define HGNN_PACK_FLAG_COO 4    /* an index >= n, or entries not strictly ascending row-major      */
typedef struct hgnn_pack_view {
    const int64_t* d_node_off;
    const float* d_x;
    const int64_t* d_adj_off;
    const int32_t* d_adj_ij;
    const float* d_adj_w;
    const float* d_targets;
    int64_t graphs;
    int32_t f_in, reserved;
} hgnn_pack_view;
/* HGNN_ERR_ARG: null pointers, graphs <= 0, J < 1; HGNN_ERR_UNSUPPORTED: J > 3. */
int hgnn_pack_count(const hgnn_pack_view* view, int J, int dual, int32_t* d_counts, void* stream);
/* counts: host, bs x HGNN_PACK_COUNT_WORDS in batch order.  HGNN_ERR_INDEX if any record has
 * HGNN_PACK_FLAG_INDEX, else HGNN_ERR_UNSUPPORTED if any has HGNN_PACK_FLAG_BOUNDS or _COO. */
int hgnn_csr_layout_from_counts(int bs, const int32_t* counts, int f_in, int J, int dual,
                                hgnn_csr_layout* layout);
size_t hgnn_csr_batch_build_device_scratch_bytes(int bs);
/* HGNN_ERR_ARG: a null pointer, bs <= 0, scratch_bytes too small, or a layout that is not one of
 * (bs, view->f_in, J, dual); HGNN_ERR_UNSUPPORTED: J > 3. */
int hgnn_csr_batch_build_device(const hgnn_pack_view* view, const int32_t* d_counts, const int32_t* d_idx,
                                int bs, int J, int dual, const hgnn_csr_layout* layout, void* d_image,
                                void* d_scratch, size_t scratch_bytes, void* stream);

/* CCN chunk from the resident pack (csrc/ccn_pack.hip): the padded batch hgnn_ccn_forward and the CCN
 * training loops take, as hgnn_amd.train.CcnTrainStep._chunks assembles it on the host
 * (scripts/train_ccn.py:35-37 plus padding) -- bit for bit.  One enqueue, no host synchronisation.  For
 * b < G and g = d_idx[b] (any order, repeats allowed):
 *   d_X[b]       (nmax, f_in)  rows < n_g from the pack, everything else 0
 *   d_adj[b]     (nmax, nmax)  A + I in fp32: the stored weight off the diagonal, w + 1.0f on it (w = 0 where
 *                              no entry is stored), 0 at every row or column >= n_g
 *   d_n_batch[b] = n_g,  d_y[b] = targets[g * n_targets + task]   (targets: (graphs, n_targets) fp32)
 * Every element of the four outputs is written; they may be uninitialised.  Nothing else is written, whatever
 * the pack holds: a slot whose g is outside [0, graphs), whose n_g > nmax, or whose entries are not all in
 * [0, n_g)^2 and strictly ascending row-major becomes the empty slot the CCN kernels skip (all zero,
 * n_batch = 0, y = 0), and bit 1 is ORed into *d_err (int32, may be null).  Any n_g <= nmax is taken.
 * HGNN_ERR_ARG: a null pointer (view members and d_targets included), G <= 0, nmax <= 0, task outside
 * [0, n_targets); HGNN_ERR_UNSUPPORTED: nmax * (nmax + 1) or nmax * f_in >= 2^31. */
int hgnn_pack_ccn_chunk(const hgnn_pack_view* view, int n_targets, const int32_t* d_idx, int G, int nmax, int task,
                        float* d_X, float* d_adj, int64_t* d_n_batch, float* d_y, int32_t* d_err, void* stream);

/* ------------------------------------------------------------------------
 * Device-resident training step (csrc/train.hip): the loss and optimizer of
 * train_with_mnb (scripts/train_mnb.py:41-91) with no host round trip.
 *
 * hgnn_mse_loss: T' = normalize_data(T, mean, std) (functions/utils.py:84-95:
 * mean only when std < 1e-5), d_stats[0] = MSELoss(out, T'), d_stats[1] = MAE
 * (utils.evaluation, functions/utils.py:98-102), d_stats[2..3] = RunningAverage
 * (momentum 0.1, functions/utils.py:134-146) of both, updated in place (zero them
 * per epoch); d_dout (optional) = dLoss/dout = 2 (out - T') / n.
 * hgnn_adamax_step: torch.optim.Adamax(lr, (beta1, beta2), eps, weight_decay)
 * (scripts/main_gnn_qm9.py:185) on n_tensors parameter tensors in one launch per
 * 64 tensors; step = the 1-based step count of this update.
 * ---------------------------------------------------------------------- */
int hgnn_mse_loss(const float* d_out, const float* d_t, int n, float t_mean, float t_std, float* d_stats,
                  float* d_dout, void* stream);

/* Classification branch (scripts/train_mnb.py:50-51, nn.CrossEntropyLoss of
 * scripts/main_generate.py:147): d_out (n, c) logits, d_t (n,) class indices stored
 * as float (prepare_batch's T); stats[0] = mean cross entropy, stats[2] its
 * RunningAverage (stats[1], stats[3] untouched: no MAE for classes); d_dout =
 * (softmax - onehot) / n.  A target outside [0, c) or not integral sets *d_err. */
int hgnn_xent_loss(const float* d_out, const float* d_t, int n, int c, float* d_stats,
                   float* d_dout, uint32_t* d_err, void* stream);
int hgnn_adamax_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                     float* const* exp_inf, const int64_t* numel, double lr, double beta1, double beta2,
                     double eps, double weight_decay, long long step, void* stream);

/* The evaluation meters of test_with_mnb (scripts/test_mnb.py:25-92: two AverageMeters, update(value, bs) per
 * batch), accumulated on the device over the batches of a set.  d_meters: six doubles owned by the caller, zeroed
 * by the caller at the start of a set:
 *   [0] loss.sum = sum_b loss_b * rows_b    [1] error.sum = sum_b mae_b * rows_b    [2] count = sum_b rows_b
 *   [3] hits (classification)               [4] loss.val (last batch)               [5] error.val (last batch)
 * so loss.avg = [0] / [2], error.avg = [1] / [2], accuracy = [3] / [2].  One 256-thread block per call; fp64 sums
 * in a fixed order; the meters are updated by one thread with plain loads and stores (stream order serialises the
 * batches: no atomics, the same bits for the same sequence of calls).
 * hgnn_eval_loss (test_mnb.py:52, 64-70, mean != 0): d_out, d_t (rows, dim_out); the target normalised as in
 *   hgnn_mse_loss; loss = MSELoss and mae = utils.evaluation over the rows * dim_out elements -- the bits
 *   hgnn_mse_loss writes to d_stats[0..1] for the same inputs -- then, in double, [0] += loss * rows,
 *   [1] += mae * rows, [2] += rows, [4] = loss, [5] = mae.
 * hgnn_eval_xent (test_mnb.py:49-50, mean == 0, nn.CrossEntropyLoss): d_out (rows, c) logits, d_t (rows,) class
 *   indices stored as float; loss = the mean cross entropy as hgnn_xent_loss forms it; [0] += loss * rows,
 *   [2] += rows, [3] += the rows whose first maximum (torch.argmax's tie rule) is the target, [4] = loss; [1] and
 *   [5] are never written.  A target that is not an integer in [0, c) ORs 1 into *d_err and adds to neither the
 *   loss nor the hits; the divisor stays rows.
 * rows == 0 writes nothing and returns HGNN_OK.  HGNN_ERR_ARG, before any launch: a null pointer, rows < 0,
 * dim_out < 1, c < 1, rows * dim_out (rows * c) >= 2^31. */
int hgnn_eval_loss(const float* d_out, const float* d_t, int rows, int dim_out, float t_mean, float t_std,
                   double* d_meters, void* stream);
int hgnn_eval_xent(const float* d_out, const float* d_t, int rows, int c, double* d_meters, uint32_t* d_err,
                   void* stream);

/* The optimizers the reference's drivers build (--optim sgd|adamax|adam, scripts/main_ccn.py:155-162,
 * scripts/main_gnn.py:161-167): torch.optim.Adamax(params, lr), torch.optim.SGD(params, lr, momentum) and
 * torch.optim.Adam(params, lr). */
typedef enum hgnn_optimizer {
    HGNN_OPT_ADAMAX = 0,
    HGNN_OPT_SGD = 1,
    HGNN_OPT_ADAM = 2
} hgnn_optimizer;

/* hgnn_optim_step: one step of optimizer `kind` on n_tensors parameter tensors, one launch per 64 tensors, in
 * torch.optim's arithmetic (scalars combined in double, passed to the kernel as fp32):
 *   HGNN_OPT_ADAMAX  hgnn_adamax_step, bit for bit; state1 = exp_avg, state2 = exp_inf.
 *   HGNN_OPT_SGD     g += wd p; buf = momentum buf + g; p -= lr buf (dampening 0, no Nesterov; a zero buffer makes
 *                    the first step buf = g as torch's does).  state1 = momentum_buffer; state2, beta2, eps and
 *                    step are not used (state2 may be NULL); beta1_or_momentum = momentum.
 *   HGNN_OPT_ADAM    g += wd p; m = lerp(m, g, 1 - beta1); v = beta2 v + (1 - beta2) g g;
 *                    p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps) (no amsgrad).
 *                    state1 = exp_avg, state2 = exp_avg_sq.
 * step = the 1-based count of this update (>= 1).  HGNN_ERR_ARG for any other kind. */
int hgnn_optim_step(int kind, int n_tensors, float* const* params, const float* const* grads,
                    float* const* state1, float* const* state2, const int64_t* numel, double lr,
                    double beta1_or_momentum, double beta2, double eps, double weight_decay, long long step,
                    void* stream);

/* ------------------------------------------------------------------------
 * Covariant compositional networks: CCN_1D / CCN_2D forward + backward.
 *
 * Replaces models/compnets/model_ccn.py:41-64 (CCN_1D.forward) and 93-105
 * (CCN_2D.forward) with CompnetUtils' receptive fields / chi matrices
 * (functions/utils_ccn.py:66-222), promotions and updates (225-324) and
 * collapse6to3 (functions/contraction.py:106-121, evaluated in its O(n^3) closed
 * form).  A batch of graphs is padded like prepare_batch does for the GNNs:
 *   X (bs, nmax, f), adj (bs, nmax, nmax) WITH self loops (scripts/train_ccn.py:36),
 *   n_batch (bs,) int64.
 * Graphs are independent: output[b] is the reference's net(X_b, adj_b).
 * Params: w1.weight w1.bias ... wL.weight wL.bias fc.weight fc.bias (nn.Linear).
 * ---------------------------------------------------------------------- */
typedef struct hgnn_ccn_config {
    int32_t order;    /* 1: CCN_1D, 2: CCN_2D                         */
    int32_t bs, nmax, f_in;
    int32_t hidden;   /* hidden_size                                   */
    int32_t layers;   /* number of update layers (<= 15)               */
    int32_t n_out;    /* n_outputs                                     */
    int32_t reserved;
} hgnn_ccn_config;

/* Plan: receptive fields, degrees, offsets and chi position maps (device).  The
 * one synchronising call of the CCN path: it returns h_sums[4] = {sum d_i,
 * sum d_i^2, nodes, max d_i} to size the feature workspace and the kernels' LDS.
 * Pass the bound max_sum_d2 used to size plan_ws (e.g. bs * nmax^2); HGNN_ERR_ARG
 * if exceeded.  forward / backward / workspace_bytes take the same four sums. */
size_t hgnn_ccn_plan_bytes(const hgnn_ccn_config* cfg, long long max_sum_d2);
int hgnn_ccn_plan(const hgnn_ccn_config* cfg, const float* d_adj, const int64_t* d_n_batch,
                  void* plan_ws, long long max_sum_d2, long long* h_sums, void* stream);
/* Same without any host synchronisation (the per-graph drop-in path, scripts/train_ccn.py:52):
 * h_sums_bound[4] receives upper bounds {bs nmax^2, max_sum_d2, bs nmax, nmax} that size the workspace;
 * the kernels read the exact totals on the device.  max_sum_d2 >= bs nmax^3 (a bound for any
 * content; HGNN_ERR_ARG otherwise), so the sizes never depend on the data. */
int hgnn_ccn_plan_async(const hgnn_ccn_config* cfg, const float* d_adj, const int64_t* d_n_batch,
                        void* plan_ws, long long max_sum_d2, long long* h_sums_bound, void* stream);
uint32_t* hgnn_ccn_error_word(const hgnn_ccn_config* cfg, void* plan_ws, long long max_sum_d2);
size_t hgnn_ccn_workspace_bytes(const hgnn_ccn_config* cfg, const long long* sums);
int hgnn_ccn_forward(const hgnn_ccn_config* cfg, const long long* sums, const float* d_X,
                     const float* const* params, void* plan_ws, long long max_sum_d2,
                     void* workspace, float* d_out, void* stream);
/* grads overwritten (params order); d_dX (bs, nmax, f) overwritten. */
int hgnn_ccn_backward(const hgnn_ccn_config* cfg, const long long* sums, const float* const* params,
                      void* plan_ws, long long max_sum_d2, void* workspace, const float* d_dout,
                      float* const* grads, float* d_dX, void* stream);

/* CCN on small graphs -- order 1 (CCN_1D): nmax <= 64, f_in and hidden <= 8; order 2 (CCN_2D):
 * nmax <= 32, f_in <= 8, hidden <= 2 (the reference's CCN_2D hidden size).  One workgroup per graph
 * builds the receptive fields, runs every level and the readout -- no plan, no host sync, one
 * dispatch forward, one backward (+ one reduction over the graphs when bs > 1).  The per-graph
 * drop-in call of scripts/train_ccn.py:31-73 (net(X, A + I) per graph) and QM9-size batches.  Same
 * layouts and results as hgnn_ccn_forward / _backward: outputs and dX in the same fp32 order (order 2
 * at bs = 1: the weight gradients too -- a batch of several graphs reduces its per-node parameter
 * partials in another order; order 1 sums them in a different order).  d_n_batch may be NULL (every
 * graph has nmax nodes).
 * supported: 1 if cfg fits (order 1: the LDS of the backward, 4 nmax^2 (hidden L + 2 max(f_in, hidden)
 * + 2 hidden) + 8 KB, within 160 KB; order 2: 8 waves x (6.5 KB + 10 nmax^2 B) + 8 KB), else 0 (use
 * the general path).  Order 2's workspace holds each graph's levels at a bound of nmax^3 rows per
 * level: (L + 2) nmax^3 hidden floats per graph (about 4 MB per graph at nmax = 32, L = 15) -- the
 * Python layer sends batches above 512 MB of that region to the general path (hgnn_amd/ccn.py).
 * Validation (self loops, symmetric pattern, 0 <= n_b <= nmax): a graph with bits stores
 * *d_err = tag * 256 + bits (0 < tag < 2^23, a plain store; nothing is stored when the batch is valid;
 * tag only labels the store).  The caller reports any nonzero word and clears it (clear-on-report): a
 * store that lands between the caller's read and its clear is lost.  d_err may be the device alias of
 * a host-mapped word (hgnn_host_word_alloc): the check is then a host read, with no copy or event per
 * call.
 * The workspace holds the readout features between forward and backward. */
int hgnn_ccn_small_supported(const hgnn_ccn_config* cfg);
/* A 64-byte host-mapped, coherent word block (zeroed): *host_ptr for the host, *dev_ptr for kernels. */
int hgnn_host_word_alloc(void** host_ptr, void** dev_ptr);
size_t hgnn_ccn_small_workspace_bytes(const hgnn_ccn_config* cfg);
int hgnn_ccn_small_forward(const hgnn_ccn_config* cfg, const float* d_X, const float* d_adj,
                           const int64_t* d_n_batch, const float* const* params, void* workspace,
                           int32_t* d_err, int32_t tag, float* d_out, void* stream);
int hgnn_ccn_small_backward(const hgnn_ccn_config* cfg, const float* d_X, const float* d_adj,
                            const int64_t* d_n_batch, const float* const* params, void* workspace,
                            const float* d_dout, float* const* grads, float* d_dX, void* stream);

/* The per-graph training loop of scripts/train_ccn.py:31-73 (per graph: the normalised target, net(X, A + I),
 * MAE and MSE meters, backward, one Adamax step) for CCN_1D in ONE dispatch: one workgroup walks the cfg->bs
 * graphs in index order -- forward, loss, backward and the optimizer step of graph g, then graph g + 1 on the
 * weights graph g left -- with no host round trip.  The arithmetic is that of the pieces it replaces:
 * hgnn_ccn_small_forward / _backward on the one-graph slice, hgnn_mse_loss on the normalised target and
 * hgnn_adamax_step.
 *   supported: host only; 1 for order 1 within hgnn_ccn_small_supported's bounds (cfg->bs is not looked at)
 *     and n_out <= 1088, else 0.
 *   cfg->bs = the number of graphs, 1 .. 4096 (HGNN_ERR_ARG above: split the list); d_X, d_adj, d_n_batch as
 *     hgnn_ccn_small_forward (d_n_batch may be NULL); d_y (bs, n_out) raw targets, normalised as
 *     (y - (float)t_mean) / (float)(t_std + 1e-8) (train_ccn.py:42).
 *   params (updated in place), grads (left holding the last applied graph's gradients), exp_avg, exp_inf
 *     (updated in place): 2 layers + 2 device pointers each, in the parameter order above.
 *   d_clr (bs,): the step sizes (float)(lr / (1 - beta1^t)) of the steps t = step0 + 1, step0 + 2, ... this call
 *     takes, formed in double as hgnn_adamax_step forms its own; entry k belongs to the k-th applied step.
 *   d_stats[4]: loss, MAE and the RunningAverage of both, as hgnn_mse_loss updates them, once per graph.
 *   d_out (bs, n_out): the output each graph saw before its own update.
 *   A graph with validation bits (see above) gets its d_out row and *d_err = tag * 256 + bits, and nothing
 *     else: no loss, no meters, no gradients, no step; the loop goes on with the next graph. */
int hgnn_ccn_small_train_supported(const hgnn_ccn_config* cfg);
int hgnn_ccn_small_train(const hgnn_ccn_config* cfg, const float* d_X, const float* d_adj,
                         const int64_t* d_n_batch, const float* d_y, double t_mean, double t_std,
                         float* const* params, float* const* grads, float* const* exp_avg,
                         float* const* exp_inf, const float* d_clr, double beta1, double beta2, double eps,
                         double weight_decay, float* d_stats, float* d_out, int32_t* d_err, int32_t tag,
                         void* stream);
/* The same loop on the reference's classification branch (`mean == 0`, scripts/train_ccn.py:39-41, 56-57: the
 * target cast to a class index, the output viewed as (1, n_out), nn.CrossEntropyLoss; the generated-data driver
 * scripts/main_generate_ccn.py).  Arguments as hgnn_ccn_small_train without the target statistics, and:
 *   d_y (bs,): class indices stored as float; cfg->n_out >= 2 (HGNN_ERR_ARG below: one class has loss 0).
 *   The loss of a graph is hgnn_xent_loss's on its row (n = 1), bit for bit: both kernels inline one row function.
 *   d_stats[0] = the graph's cross entropy, d_stats[2] its RunningAverage; d_stats[1] and d_stats[3] are never
 *     written (no MAE on this branch).
 *   A target that is not an integer in [0, n_out) is handled like a validation bit: the graph gets its d_out
 *     row and *d_err = tag * 256 + bits with HGNN_DEVERR_CLASS_TARGET among them, and nothing else. */
int hgnn_ccn_small_train_xent(const hgnn_ccn_config* cfg, const float* d_X, const float* d_adj,
                              const int64_t* d_n_batch, const float* d_y, float* const* params,
                              float* const* grads, float* const* exp_avg, float* const* exp_inf,
                              const float* d_clr, double beta1, double beta2, double eps, double weight_decay,
                              float* d_stats, float* d_out, int32_t* d_err, int32_t tag, void* stream);
/* The same per-graph loop for CCN_2D (the drivers' other model: scripts/main_ccn_qm9.py:140,145) in ONE dispatch:
 * one 512-thread workgroup walks the cfg->bs graphs in index order.  Per graph the arithmetic is that of
 * hgnn_ccn_small_forward / _backward (order 2) on the one-graph slice, hgnn_mse_loss (or hgnn_xent_loss with
 * n = 1) and hgnn_adamax_step, bit for bit: out, every gradient, both moments and the parameters.  (The running
 * loss of the _xent entry may differ from hgnn_xent_loss's in its last bit, as for order 1.)  No dX is formed.
 *   supported: host only; 1 for order 2 with nmax <= 32, f_in <= 8, hidden <= 2, layers <= 15,
 *     f_in + layers * hidden <= 64 and n_out <= 256 (the graph's out / dout row is a 1 KB static LDS buffer), the
 *     kernel's LDS -- hgnn_ccn_small_supported's order-2 carve plus that 1 KB -- within 160 KB (nmax = 32 uses
 *     about 140 KB); cfg->bs is not looked at.  Else 0.
 *   workspace_bytes: one graph's region whatever cfg->bs is -- the (L + 2) nmax^3 hidden floats of the levels
 *     and the dp format, the per-node parameter partials and a feature row -- reused by every graph of the
 *     dispatch; 0 where unsupported.  The caller may keep it across calls; nothing in it is read before it is
 *     written.
 *   Arguments, the rejected graphs (validation bits; _xent: a class target that is no integer in [0, n_out)) and
 *     the return codes are those of hgnn_ccn_small_train / _xent, with the workspace before d_err.
 *     hgnn_ccn_small_train* itself keeps returning HGNN_ERR_UNSUPPORTED for order 2. */
int hgnn_ccn2_small_train_supported(const hgnn_ccn_config* cfg);
size_t hgnn_ccn2_small_train_workspace_bytes(const hgnn_ccn_config* cfg);
int hgnn_ccn2_small_train(const hgnn_ccn_config* cfg, const float* d_X, const float* d_adj,
                          const int64_t* d_n_batch, const float* d_y, double t_mean, double t_std,
                          float* const* params, float* const* grads, float* const* exp_avg,
                          float* const* exp_inf, const float* d_clr, double beta1, double beta2, double eps,
                          double weight_decay, float* d_stats, float* d_out, void* workspace, int32_t* d_err,
                          int32_t tag, void* stream);
int hgnn_ccn2_small_train_xent(const hgnn_ccn_config* cfg, const float* d_X, const float* d_adj,
                               const int64_t* d_n_batch, const float* d_y, float* const* params,
                               float* const* grads, float* const* exp_avg, float* const* exp_inf,
                               const float* d_clr, double beta1, double beta2, double eps, double weight_decay,
                               float* d_stats, float* d_out, void* workspace, int32_t* d_err, int32_t tag,
                               void* stream);
/* Both loops with the optimizer chosen (scripts/main_ccn.py:59-62, 155-162: --optim sgd|adamax|adam, --momentum):
 * the same kernels with their optimizer stage instantiated for `kind` (hgnn_optimizer); everything else -- the
 * validation bits, the error word, the 4096-graph bound, the return codes, supported and the workspace -- is that
 * of hgnn_ccn_small_train / hgnn_ccn2_small_train.  Per graph the update is hgnn_optim_step's, bit for bit.
 *   xent: 0 = the MSE loop (t_mean, t_std as above), nonzero = the classification loop (t_mean, t_std ignored).
 *   state1, state2: as hgnn_optim_step (SGD: state2 and its entries may be NULL and are never touched).
 *   d_steps (bs, 2): the per-step scalars, formed in double on the host; row k belongs to the k-th APPLIED step of
 *     the dispatch (a rejected graph consumes no row):
 *       ADAMAX  [lr / (1 - beta1^t), unused]     SGD  [lr, unused]
 *       ADAM    [lr / (1 - beta1^t), sqrt(1 - beta2^t)]
 *   beta1_or_momentum, beta2, eps, weight_decay: as hgnn_optim_step.  HGNN_ERR_ARG for an unknown kind. */
int hgnn_ccn_small_train_opt(const hgnn_ccn_config* cfg, int kind, int xent, const float* d_X, const float* d_adj,
                             const int64_t* d_n_batch, const float* d_y, double t_mean, double t_std,
                             float* const* params, float* const* grads, float* const* state1,
                             float* const* state2, const float* d_steps, double beta1_or_momentum, double beta2,
                             double eps, double weight_decay, float* d_stats, float* d_out, int32_t* d_err,
                             int32_t tag, void* stream);
int hgnn_ccn2_small_train_opt(const hgnn_ccn_config* cfg, int kind, int xent, const float* d_X, const float* d_adj,
                              const int64_t* d_n_batch, const float* d_y, double t_mean, double t_std,
                              float* const* params, float* const* grads, float* const* state1,
                              float* const* state2, const float* d_steps, double beta1_or_momentum, double beta2,
                              double eps, double weight_decay, float* d_stats, float* d_out, void* workspace,
                              int32_t* d_err, int32_t tag, void* stream);
/* Mini-batch training for CCN_1D: one optimizer step per mini-batch of `batch` graphs, the graphs of a mini-batch in
 * parallel (one workgroup each), everything on the device.  The cfg->bs graphs are cut into ceil(bs / batch)
 * consecutive mini-batches, the last one shorter; mini-batch k + 1 runs on the weights mini-batch k left.  Per
 * mini-batch of B graphs, all seeing the same weights: out_g = net(X_g, A_g + I); MSE: the target normalised as
 * above, nn.MSELoss over the (B, n_out) block, dout = 2 (out - y') / (B n_out); classification: nn.CrossEntropyLoss
 * on the (B, n_out) logits, dout = (softmax - onehot) / B; the parameter gradients summed over the B graphs; one
 * step of the optimizer `kind`.  Two dispatches per mini-batch, ordered by the stream alone.  The arithmetic is that
 * of the pieces on the mini-batch's slice -- hgnn_ccn_small_forward, hgnn_mse_loss on the normalised target (or
 * hgnn_xent_loss), hgnn_ccn_small_backward, hgnn_optim_step -- bit for bit: out, every gradient, the meters, the
 * optimizer state and the parameters.  (The running loss of the classification branch is formed from the same row
 * losses in the same order.)
 *   supported: host only; 1 for order 1 within hgnn_ccn_small_train_supported's bounds (cfg->bs is not looked at),
 *     else 0 (order 2: hgnn_ccn2_small_train_batch below).
 *   workspace_bytes: cfg->bs reject words (a call clears and uses the first ceil(bs / batch), one per mini-batch,
 *     with one hipMemsetAsync), then one mini-batch's per-graph regions, each 256-byte aligned: the level partials
 *     [batch][ptot], the readout features [batch][nf] and dout [batch][n_out].  It grows with `batch` and with
 *     cfg->bs, and a workspace sized for (bs, batch) serves every call with no more graphs and no larger
 *     mini-batches.  The regions are reused by the mini-batches of a call in stream order; nothing in the workspace
 *     is read before it is written, apart from the reject words.  0 where unsupported, for batch < 1 or bs outside
 *     1 .. 4096.  The caller may keep it across calls on one stream.
 *   cfg->bs = the number of graphs, 1 .. 4096; batch >= 1 (it may exceed bs: one mini-batch of bs graphs).
 *   kind, xent, d_X, d_adj, d_n_batch, d_y, t_mean, t_std, params, state1, state2, the hyper-parameters, d_err and
 *     tag: as hgnn_ccn_small_train_opt.  MSE: (float)(t_std + 1e-8) must be at least 1e-5 (HGNN_ERR_ARG below:
 *     hgnn_mse_loss, whose meters these are, stops dividing there).
 *   grads: left holding the last applied mini-batch's gradients.
 *   d_steps (ceil(bs / batch), 2): the rows of hgnn_ccn_small_train_opt, but row k belongs to mini-batch k WHETHER
 *     OR NOT it is applied: the host cannot know which mini-batches the device rejected, so a rejected mini-batch
 *     consumes its row (and its step number) without taking the step.
 *   d_stats[4]: as hgnn_mse_loss (or hgnn_xent_loss: [1] and [3] never written) updates them, once per applied
 *     mini-batch: the mini-batch's loss and MAE and the RunningAverage of both.
 *   d_out (bs, n_out): the output each graph saw before its mini-batch's update.
 *   An empty slot (n_b = 0) is a graph like any other: its output is fc.bias, and it contributes to the loss and
 *     to the fc.bias gradient.
 *   A graph with validation bits (classification: or a class target that is no integer in [0, n_out)) gets its
 *     d_out row, ORs its bits into its mini-batch's reject word and stores *d_err = tag * 256 + bits; its whole
 *     mini-batch then takes no step: no gradients, no meters, no update (the other graphs' d_out rows are
 *     written).  The call goes on with the next mini-batch.
 *   Returns HGNN_ERR_UNSUPPORTED where supported is 0, HGNN_ERR_ARG for a null pointer (d_n_batch may be NULL;
 *     SGD: state2 may be), batch < 1, bs outside 1 .. 4096, a tag outside (0, 2^23), an unknown kind, or
 *     xent with n_out < 2.  No allocation and no synchronisation inside the entry. */
int hgnn_ccn_small_train_batch_supported(const hgnn_ccn_config* cfg);
size_t hgnn_ccn_small_train_batch_workspace_bytes(const hgnn_ccn_config* cfg, int batch);
int hgnn_ccn_small_train_batch(const hgnn_ccn_config* cfg, int batch, int kind, int xent, const float* d_X,
                               const float* d_adj, const int64_t* d_n_batch, const float* d_y, double t_mean,
                               double t_std, float* const* params, float* const* grads, float* const* state1,
                               float* const* state2, const float* d_steps, double beta1_or_momentum, double beta2,
                               double eps, double weight_decay, float* d_stats, float* d_out, void* workspace,
                               int32_t* d_err, int32_t tag, void* stream);
/* CCN-1D small graphs past the LDS bound (csrc/ccn_small_spill.hip, csrc/ccn_small_batch_spill.hip): a second
 * instantiation of the kernels above whose four row-sized arrays (the L levels, dcoll, dF0, dF1) live in a
 * per-workgroup region of a caller-allocated global workspace; everything else stays in LDS (at most 37.2 KB at
 * nmax = 64).  The arithmetic and its order are those of the LDS kernels: bit for bit the same results wherever both
 * exist.  Chosen per call -- no entry above ever routes here.
 *   spill_supported: host only; 1 for order 1, 1 <= nmax <= 64, 1 <= f_in, hidden <= 8, 1 <= layers <= 15 (bs and
 *     n_out positive), with no LDS-fit term; else 0 (NULL: 0).
 *   spill_train_supported: the same with n_out <= 1088 (the training kernels' bound, as hgnn_ccn_small_train_supported); cfg->bs is not looked at.
 *   spill_workspace_bytes(cfg, regions): host only.  `regions` row regions, then the feat / ppart part of
 *     hgnn_ccn_small_workspace_bytes for cfg->bs graphs: regions * stride + align256(4 bs nf) + (bs > 1 ?
 *     4 bs ptot : 0) bytes.  A region keeps the LDS carve's order and strides -- nmax^2 hidden floats per level,
 *     nmax^2 2 max(f_in, hidden), nmax^2 hidden twice -- plus 512 floats of tail padding (the walks read rows of idle
 *     lanes past the graph's and drop them; those reads stay inside the region), rounded up to 256 bytes:
 *     stride = align256(4 (nmax^2 (hidden layers + 2 max(f_in, hidden) + 2 hidden) + 512)).
 *     regions = cfg->bs for the one-shot calls, 1 for the training loop, `batch` for a mini-batch call (the training
 *     entries use the regions only, so their cfg->bs may be 1 in the query).  0 for regions < 1, on overflow or
 *     where spill_supported is 0.  The workspace must be 256-byte aligned; a region is written and read by its
 *     workgroup only and nothing in it is read before it is written (apart from values the selects drop).
 *   The entries mirror hgnn_ccn_small_forward / _backward, hgnn_ccn_small_train_opt and hgnn_ccn_small_train_batch
 *     argument for argument, with the spill workspace added (`workspace` / `spill_workspace`; the mini-batch entry
 *     still takes hgnn_ccn_small_train_batch_workspace_bytes' workspace as well), and return the same codes:
 *     HGNN_ERR_UNSUPPORTED where the predicate is 0, HGNN_ERR_ARG for a null pointer and the other argument errors. */
int hgnn_ccn_small_spill_supported(const hgnn_ccn_config* cfg);
int hgnn_ccn_small_spill_train_supported(const hgnn_ccn_config* cfg);
size_t hgnn_ccn_small_spill_workspace_bytes(const hgnn_ccn_config* cfg, int regions);
int hgnn_ccn_small_spill_forward(const hgnn_ccn_config* cfg, const float* d_X, const float* d_adj,
                                 const int64_t* d_n_batch, const float* const* params, void* workspace,
                                 int32_t* d_err, int32_t tag, float* d_out, void* stream);
int hgnn_ccn_small_spill_backward(const hgnn_ccn_config* cfg, const float* d_X, const float* d_adj,
                                  const int64_t* d_n_batch, const float* const* params, void* workspace,
                                  const float* d_dout, float* const* grads, float* d_dX, void* stream);
int hgnn_ccn_small_spill_train(const hgnn_ccn_config* cfg, int kind, int xent, const float* d_X, const float* d_adj,
                               const int64_t* d_n_batch, const float* d_y, double t_mean, double t_std,
                               float* const* params, float* const* grads, float* const* state1,
                               float* const* state2, const float* d_steps, double beta1_or_momentum, double beta2,
                               double eps, double weight_decay, float* d_stats, float* d_out, void* workspace,
                               int32_t* d_err, int32_t tag, void* stream);
int hgnn_ccn_small_spill_train_batch(const hgnn_ccn_config* cfg, int batch, int kind, int xent, const float* d_X,
                                     const float* d_adj, const int64_t* d_n_batch, const float* d_y, double t_mean,
                                     double t_std, float* const* params, float* const* grads, float* const* state1,
                                     float* const* state2, const float* d_steps, double beta1_or_momentum,
                                     double beta2, double eps, double weight_decay, float* d_stats, float* d_out,
                                     void* workspace, void* spill_workspace, int32_t* d_err, int32_t tag,
                                     void* stream);
/* The same for CCN-2D (csrc/ccn2_small_batch.hip): mini-batches of `batch` graphs, one workgroup per graph, two
 * dispatches per mini-batch ordered by the stream alone.  The first runs plan, forward, the graph's dout row and the
 * backward (no dX, one plan for both directions) in the graph's own workspace region; the second sums the node
 * partials and the fc products over the mini-batch in the order of hgnn_ccn_small_backward's batch reduction and
 * applies the optimizer `kind` to each element.  Bit for bit the pieces on the mini-batch's slice, as above.
 *   supported: host only; 1 exactly where hgnn_ccn2_small_train_supported is (cfg->bs is not looked at), else 0.
 *   workspace_bytes: cfg->bs reject words (a call clears and uses the first ceil(bs / batch), one per mini-batch,
 *     with one hipMemsetAsync), then one mini-batch's regions, each 256-byte aligned and reused by the mini-batches
 *     of a call in stream order: the readout features [batch][nf], dout [batch][n_out], per level the node partials
 *     [batch nmax][hidden 18 c_l + hidden], and `batch` graph regions (levels, the dp format, row sums: the
 *     per-graph region of hgnn_ccn_small_workspace_bytes).  A graph region is about 0.8 MB at nmax = 29,
 *     layers = 2, hidden = 2, so batch = 256 takes about 200 MB and batch = 4096 about 3.3 GB.  It never shrinks as
 *     `batch` or cfg->bs grows; nothing in it is read before it is written, apart from the reject words.  0 where
 *     unsupported, for batch < 1 or bs outside 1 .. 4096.  The caller may keep it across calls on one stream.
 *   Every argument, d_steps' row rule, d_stats, d_out, empty slots, rejected graphs and the return values: as
 *     hgnn_ccn_small_train_batch (the refusals are made in the same order, before any pointer is read). */
int hgnn_ccn2_small_train_batch_supported(const hgnn_ccn_config* cfg);
size_t hgnn_ccn2_small_train_batch_workspace_bytes(const hgnn_ccn_config* cfg, int batch);
int hgnn_ccn2_small_train_batch(const hgnn_ccn_config* cfg, int batch, int kind, int xent, const float* d_X,
                                const float* d_adj, const int64_t* d_n_batch, const float* d_y, double t_mean,
                                double t_std, float* const* params, float* const* grads, float* const* state1,
                                float* const* state2, const float* d_steps, double beta1_or_momentum, double beta2,
                                double eps, double weight_decay, float* d_stats, float* d_out, void* workspace,
                                int32_t* d_err, int32_t tag, void* stream);
/* The evaluation meters of scripts/test_ccn.py:34-67 on the outputs of a forward over n_graphs graphs:
 * d_res[0] = mean over graphs of MSELoss(out_g, y'_g), d_res[1] = mean over graphs of the MAE, y' normalised
 * as above.  One block, fp64 sums in a fixed order: the same bits every call. */
int hgnn_ccn_eval_loss(const float* d_out, const float* d_y, int n_graphs, int n_out, double t_mean,
                       double t_std, float* d_res, void* stream);
/* The classification branch of the same meters (test_ccn.py:40-41, 52-55): d_y (n_graphs,) class indices stored
 * as float; d_res[0] = mean over graphs of the per-graph cross entropy (losses.avg), d_res[1] = 0 (error.avg,
 * never updated on this branch), d_res[2] = the fraction of graphs whose first maximum (torch.argmax's tie
 * rule) is the target.  A target that is not an integer in [0, n_out) ORs 1 into *d_err and adds to neither
 * sum; the divisor stays n_graphs.  One block, fp64 sums in the same fixed order. */
int hgnn_ccn_eval_xent(const float* d_out, const float* d_y, int n_graphs, int n_out, float* d_res,
                       uint32_t* d_err, void* stream);

/* collapse6to3 (functions/contraction.py:106-121) on a general 6-D tensor
 * F (C, n, n, n, n, n) -> (n, n, 18 C); the 18 contractions of _c6to2_111 /
 * _c6to2_12 / _c6to2_3 with their diagonal filters. */
int hgnn_collapse6to3(const float* d_F, float* d_out, int c, int n, void* stream);
int hgnn_collapse6to3_backward(const float* d_dout, float* d_dF, int c, int n, void* stream);

/* Byte offsets inside plan_ws of: node_off, deg, nbr (nmax slots per node),
 * selfpos, graph, off1 (prefix of d), off2 (prefix of d^2), pos (chi position
 * maps), error word -- for inspection / tests of the index construction. */
int hgnn_ccn_plan_offsets(const hgnn_ccn_config* cfg, long long max_sum_d2, size_t* offs);

/* ------------------------------------------------------------------------
 * Layer-level drop-ins on dense padded tensors.
 * ---------------------------------------------------------------------- */

/* graph_oper.forward (models/layers/layers_mnb.py:395-411) == graph_op
 * (functions/utils.py:24-52):  out[b, j*F+f, n] = sum_m A[b,n,m,j] X[b,f,m].
 * A (bs, N, N, J), X (bs, F, N), out (bs, J*F, N). */
int hgnn_graph_oper_forward(const float* d_A, const float* d_X, float* d_out,
                            int bs, int n, int j, int f, void* stream);
/* Backward: dX (bs, F, N) = sum_j A_j^T dOut_j (overwritten); dA (bs, N, N, J)
 * = dOut_j X^T if d_dA != NULL (overwritten). */
int hgnn_graph_oper_backward(const float* d_A, const float* d_X, const float* d_dout,
                             float* d_dX, float* d_dA, int bs, int n, int j, int f,
                             void* stream);

/* P_multi.forward (layers_mnb.py:418-434) == Pmul (functions/utils.py:55-81):
 * out[b, f, n] = sum_m P[b, n, m] X[b, f, m], P read as (bs, N, M) with strides
 * (sb, sn, sm) so a transposed view (Pm.transpose(2,1)) needs no copy. */
int hgnn_p_multi_forward(const float* d_P, long sb, long sn, long sm,
                         const float* d_X, float* d_out, int bs, int n, int m, int f,
                         void* stream);
int hgnn_p_multi_backward(const float* d_P, long sb, long sn, long sm,
                          const float* d_X, const float* d_dout, float* d_dX,
                          float* d_dP, int bs, int n, int m, int f, void* stream);

/* BN.forward (batch_normalization.py:34-43) with sb_normalization /
 * mean_with_padding / mask_embedding (65-108).  X, out (bs, C, N); mask (bs, N, N);
 * training: writes batch mean/std (C,) to d_mean/d_std; eval: reads them.
 * w, b: 0-dim device scalars. */
int hgnn_bn_forward(const float* d_X, const int64_t* d_nb, const float* d_mask,
                    const float* d_w, const float* d_b, float* d_mean, float* d_std,
                    float* d_out, int bs, int c, int n, int training, void* stream);
/* dX (bs, C, N) overwritten; dw, db (scalars) overwritten; d_scratch: 2 C floats. */
int hgnn_bn_backward(const float* d_X, const int64_t* d_nb, const float* d_mask,
                     const float* d_w, const float* d_mean, const float* d_std,
                     const float* d_dout, float* d_dX, float* d_dw, float* d_db,
                     float* d_scratch, int bs, int c, int n, int training, void* stream);

/* 1x1 Conv1d (torch.nn.Conv1d(cin, cout, 1), used by every layer_* module,
 * layers_mnb.py:36-37, 81, 172-177, 239-244, 305-310, 371) on the channel-major
 * layout: y (bs, cout, n) = W (cout, cin) . x (bs, cin, n) + b, then ReLU if relu.
 * Workspace: hgnn_conv1x1_workspace_bytes(). */
size_t hgnn_conv1x1_workspace_bytes(int bs, int cin, int cout, int n);
int hgnn_conv1x1_forward(const float* d_x, const float* d_w, const float* d_b, float* d_y,
                         int bs, int cin, int cout, int n, int relu, void* workspace, void* stream);
/* d_dy: gradient wrt the pre-ReLU output.  dW (cout, cin), db (cout) overwritten;
 * dx (bs, cin, n) overwritten when non-NULL. */
int hgnn_conv1x1_backward(const float* d_x, const float* d_w, const float* d_dy, float* d_dx,
                          float* d_dw, float* d_db, int bs, int cin, int cout, int n,
                          void* workspace, void* stream);

/* ------------------------------------------------------------------------
 * Kernel probes (tests and inspection).
 *
 * The Conv1d-pair GEMMs of the executor (csrc/gemm_bf3.hip, csrc/gemm3.hip) and the weight repack
 * (csrc/kernels.h repack_part) behind plain entry points, so a test can hand one kernel any shape
 * its launcher accepts.  A probe takes the pair as the executor holds it (wl, wr (d, k) row-major,
 * bl, br (d)), runs the repack itself and passes the GEMM the repacked operands with the executor's
 * leading dimensions: kp = k rounded up to 4, c2 = 2d, c2p = c2 rounded up to 4, bf16 plane rows of
 * ld3(x) = x rounded up to 16.  Nothing is allocated; the caller's workspace is sized by the
 * *_workspace_bytes query; every call only enqueues work on `stream`; the launcher's status comes
 * back unchanged.  No switch is added: the HGNN_* switches select kernel variants as they do in
 * the executor.
 * ---------------------------------------------------------------------- */

/* The diagonal I / D operand columns (csrc/kernels.h DiagIdArgs); x == NULL: none.  The logical
 * operand is [v_0 z | v_1 z | A] with z = fmaf(x - mean, w / std, b) and (v_0, v_1) = diag[row]. */
typedef struct hgnn_probe_diag {
    const float* x;     /* [rows][ldx] */
    const float* diag;  /* [rows][2] */
    const float* mean;  /* (c) */
    const float* std;   /* (c) */
    const float* w;     /* scalar */
    const float* b;     /* scalar */
    int32_t ldx, c;
} hgnn_probe_diag;

/* One repack item.  Outputs: wt [k][c2p] (columns >= c2 zero), wc [c2][kp] (columns >= k zero),
 * bc (c2), wc3 [3][c2][ld3(kp)], wt3 [3][k][ld3(c2p)] (bf16, the three split planes, zero padding). */
int hgnn_probe_repack(const float* d_wl, const float* d_wr, const float* d_bl, const float* d_br, int d, int k,
                      float* d_wt, float* d_wc, float* d_bc, void* d_wc3, void* d_wt3, void* stream);

/* Workspace of hgnn_probe_gemm_fwd / hgnn_probe_gemm_da for a pair (d, k) and m_cap rows. */
size_t hgnn_probe_gemm_workspace_bytes(int d, int k, int m_cap);

typedef struct hgnn_probe_fwd {
    const float* a;          /* [m_cap][lda]: the aggregate (k - 2c columns used with diag, else k) */
    const int32_t* m_valid;  /* device row count, or NULL: m_cap */
    const float* wl;
    const float* wr;
    const float* bl;
    const float* br;
    float* y;                /* [m_cap][ldy], 2d columns written */
    float* mean;             /* bn != 0: (2d) */
    float* std;
    float* run_mean;         /* optional, read and updated in place (momentum 0.1) */
    float* run_std;
    uint32_t* ticket_out;    /* bn == 3, optional: the ticket's value after the launch */
    hgnn_probe_diag diag;
    int32_t lda, m_cap, d, k, relu_from, ldy;
    int32_t kernel;          /* 0: split-bf16; 1: fp32 (mfma16 = 0); 2: fp32 (mfma16 = 1) */
    int32_t bn;              /* 0: none; 1: per-tile partials + finalize; 2: fp64 sums + finalize;
                                3: fp64 sums, the finalize in the GEMM's last block (2, 3: kernel 0 only) */
} hgnn_probe_fwd;
int hgnn_probe_gemm_fwd(const hgnn_probe_fwd* p, void* workspace, void* stream);

/* dA [m_cap][ldda] (k columns written) = dY [m_cap][lddy] (c2p columns read) . Wcat. */
typedef struct hgnn_probe_da {
    const float* dy;
    const int32_t* m_valid;
    const float* wl;
    const float* wr;
    const float* bl;
    const float* br;
    float* da;
    int32_t lddy, m_cap, d, k, ldda;
    int32_t kernel;          /* 0: split-bf16; 1: fp32 */
} hgnn_probe_da;
int hgnn_probe_gemm_da(const hgnn_probe_da* p, void* workspace, void* stream);

/* The dW GEMM and its slab reduction.  nz = 0: dw3_chunks(r_cap, o, k).  The workspace holds only
 * the nz split-K slabs [nz][o][k], from its first byte. */
size_t hgnn_probe_dw_workspace_bytes(int r_cap, int o, int k, int nz);
typedef struct hgnn_probe_dw {
    const float* dy;         /* [r_cap][lddy], o columns read */
    const float* a;          /* [r_cap][lda]: the saved operand (k - 2c columns with diag, else k) */
    const int32_t* r_valid;  /* device row count (required) */
    const float* dbpart;     /* optional [ceil(r_cap / 64)][o_real]: per-tile column sums of dY */
    float* dw0;              /* [split][k] */
    float* dw1;              /* [o_real - split][k] */
    float* db0;              /* with dbpart: (split) */
    float* db1;              /* with dbpart: (o_real - split) */
    hgnn_probe_diag diag;
    int32_t lddy, lda, r_cap, o, o_real, split, k, nz;
} hgnn_probe_dw;
int hgnn_probe_gemm_dw(const hgnn_probe_dw* p, void* workspace, void* stream);

/* ---- The sparse side (csrc/struct.hip, csrc/agg.hip): the batch plan and the structure extraction, the pack /
 * unpack kernels and the aggregation forward / backward launchers, under the same rules (csrc/probe_sparse.hip).
 * Row lists are those of csrc/kernels.h StructView: rows [R][2] int32 (start, count), entries of `stride` floats
 * (column as int bits, then the coefficients). */

/* launch_plan, then launch_extract with entry_stride_w = j_tot <= 3 ? 4 : 8 (the executor's choice).  Every output
 * is caller-allocated: node_off, edge_off (bs + 1), totals (2), err (1), rows[k] (bs nmax rows for the node kinds 0,
 * 1, 4; bs emax for the edge kinds 2, 3, 5), entries[k] (bs nmax nmax, bs emax emax entries of the stride for W / WT,
 * WL / WLT; bs nmax emax entries of 4 floats for PN / PE), xo [nodes][f] and xlo [edges] (optional, with X / XL).
 * dual = 0: only W, mask, n_batch and kinds 0, 1 are used.  variant (written on the host): the kernel
 * launch_extract chose -- 0 general, 1 LDS-staged, 2 register-staged. */
typedef struct hgnn_probe_extract_args {
    const float* W;
    const float* WL;
    const float* Pm;
    const float* Pd;
    const float* mask;
    const float* mask_lg;
    const int64_t* n_batch;
    const int64_t* e_batch;
    const float* X;          /* optional (bs, f, nmax) */
    const float* XL;         /* optional (bs, 1, emax) */
    int32_t* node_off;
    int32_t* edge_off;
    int32_t* totals;
    uint32_t* err;
    void* rows[6];
    float* entries[6];
    float* xo;
    float* xlo;
    int32_t bs, nmax, emax, jtot, dual, validate, f;
    int32_t variant;
} hgnn_probe_extract_args;
int hgnn_probe_extract(hgnn_probe_extract_args* p, void* stream);

/* launch_pack_nodes / launch_pack_edges / launch_unpack_nodes on the offsets of a plan (bs + 1 each). */
int hgnn_probe_pack_nodes(const float* d_X, int bs, int f, int nmax, const int32_t* d_node_off, float* d_out,
                          void* stream);
int hgnn_probe_pack_edges(const float* d_XL, int bs, int emax, const int32_t* d_edge_off, float* d_out, void* stream);
int hgnn_probe_unpack_nodes(const float* d_in, int bs, int f, int nmax, const int32_t* d_node_off, float* d_X,
                            void* stream);

typedef struct hgnn_probe_list {
    const void* rows;
    const float* entries;
    int32_t stride, reserved;
} hgnn_probe_list;

/* BN applied where the features are read (csrc/kernels.h BnView); mean == NULL: none. */
typedef struct hgnn_probe_bn {
    const float* mean;
    const float* std;
    const float* w;
    const float* b;
} hgnn_probe_bn;

/* csrc/kernels.h AggFwdArgs (launch_agg_fwd); diag [rows][2] and err are optional. */
typedef struct hgnn_probe_agg_fwd_args {
    const int32_t* total_rows;
    hgnn_probe_list g;
    const float* xg;
    hgnn_probe_bn gbn;
    hgnn_probe_list p;
    const float* xp;
    hgnn_probe_bn pbn;
    float* out;
    float* diag;
    uint32_t* err;
    int32_t cap_rows, cg, jtot, cp, ldo, pad_from, j0, reserved;
} hgnn_probe_agg_fwd_args;
int hgnn_probe_agg_fwd(const hgnn_probe_agg_fwd_args* p, void* stream);

/* csrc/kernels.h AggBwdArgs.  pair = 0: launch_agg_bwd on a (b unused); pair = 1: launch_agg_bwd_pair(a, b). */
typedef struct hgnn_probe_agg_bwd_args {
    const int32_t* total_rows;
    hgnn_probe_list g;
    const float* ing;
    hgnn_probe_list p;
    const float* inp;
    float* out;
    int32_t cap_rows, ldg, gofs, jtot, ldp, pofs_m, pofs_d, c, ldo, accumulate;
} hgnn_probe_agg_bwd_args;
int hgnn_probe_agg_bwd(const hgnn_probe_agg_bwd_args* a, const hgnn_probe_agg_bwd_args* b, int pair, void* stream);

/* ---- The dense side outside the GEMMs (csrc/bn.hip, csrc/dwdense.hip): the BN finalize and backward, the readout
 * launchers and the dense operator gradient, under the same rules (csrc/probe_dense.hip).  Every scratch buffer is
 * the caller's. */

/* csrc/kernels.h BnFwdArgs (launch_bn_finalize).  Exactly one of acc ([8][2][c] fp64: sum y, sum y^2 per copy) and
 * part ([ceil(count / 64)][c][3]: count, mean, M2 per 64-row tile) in training mode; eval mode (training = 0)
 * copies run_mean / run_std (required then).  momentum is 0.1, as the executor's. */
typedef struct hgnn_probe_bn_finalize_args {
    const double* acc;
    const float* part;
    const int32_t* count;    /* device: the real rows */
    float* mean;             /* (c) */
    float* std;              /* (c) */
    float* run_mean;         /* optional pair, read and updated in place */
    float* run_std;
    int32_t tiles, c, training, reserved;
} hgnn_probe_bn_finalize_args;
int hgnn_probe_bn_finalize(const hgnn_probe_bn_finalize_args* p, void* stream);

/* The launch sequence launch_bn_backward takes (csrc/kernels.h BnBwdPath, bn_bwd_variant). */
enum {
    HGNN_BN_BWD_NARROW2S = 0,  /* k_bn_bwd_part2s + apply2s */
    HGNN_BN_BWD_WIDE2 = 1,     /* k_bn_bwd_part2 + apply2 */
    HGNN_BN_BWD_PART4ACC = 2,  /* k_bn_bwd_part4 (fp64 atomics) + apply4 */
    HGNN_BN_BWD_PART4FIN = 3,  /* k_bn_bwd_part4 + fin (+ apply4) */
    HGNN_BN_BWD_SCALAR = 4     /* k_bn_bwd_part + fin (+ apply) */
};

/* csrc/kernels.h BnBwdArgs (launch_bn_backward) and `apply` (0: only the statistics into sums).  y, dz
 * [rows][c] (no kernel reads a row >= *total_rows), part: 4 c ceil(cap_rows / 64) floats, sums: 4 c floats, both
 * 16-byte aligned; dy [rows][ldy] (ldy = 0: c); dbpart optional [ceil(cap_rows / 64)][c]; acc64 / acc64_zero
 * optional, 32 c doubles each.  path (written on the host): the HGNN_BN_BWD_* sequence the launcher chose. */
typedef struct hgnn_probe_bn_backward_args {
    const float* y;
    const float* dz;
    const int32_t* total_rows;
    const float* mean;
    const float* std;
    const float* w;
    float* part;
    float* sums;
    float* dy;
    float* dw;
    float* db;
    float* dbpart;
    double* acc64;
    double* acc64_zero;
    int32_t cap_rows, c, relu_from, training, ldy, apply;
    int32_t path, reserved;
} hgnn_probe_bn_backward_args;
int hgnn_probe_bn_backward(hgnn_probe_bn_backward_args* p, void* stream);

/* launch_readout_fwd: a [rows][k], node_off (bs + 1), fcw (dim_out, k), fcb (dim_out) -> colsum (bs, k),
 * out (bs, dim_out). */
int hgnn_probe_readout_fwd(const float* d_a, int k, const int32_t* d_node_off, int bs, int nmax, const float* d_fcw,
                           const float* d_fcb, int dim_out, float* d_colsum, float* d_out, void* stream);
/* launch_readout_bwd_da: da [rows][k], row r of graph b = dout[b] . fcw. */
int hgnn_probe_readout_bwd_da(const float* d_dout, const int32_t* d_node_off, int bs, int cap_rows,
                              const int32_t* d_total_rows, const float* d_fcw, int dim_out, int k, float* d_da,
                              void* stream);
/* launch_readout_bwd_params: dfcw (dim_out, k), dfcb (dim_out); scratch of hgnn_probe_readout_bwd_scratch_bytes. */
size_t hgnn_probe_readout_bwd_scratch_bytes(int dim_out, int k);
int hgnn_probe_readout_bwd_params(const float* d_dout, const float* d_colsum, int bs, int nmax, int dim_out, int k,
                                  float* d_dfcw, float* d_dfcb, void* scratch, void* stream);

/* csrc/kernels.h ReadoutAggArgs (launch_readout_agg_bwd, readout_row_fits).  g: the S_WT list (node rows, jt
 * coefficients per entry), p: the S_PE list (edge rows, pm and pd); g_cap / p_cap: bs times the most rows a graph
 * may hold (the kernel's LDS is sized from them). */
typedef struct hgnn_probe_readout_agg_args {
    const float* dout;
    const float* fcw;
    const int32_t* node_off;
    const int32_t* edge_off;
    hgnn_probe_list g;
    const int32_t* g_total;
    float* g_out;            /* NULL: no G gather */
    hgnn_probe_list p;
    const int32_t* p_total;
    float* p_out;            /* NULL: no P gather */
    int32_t dim_out, k, jt, cg, cp, bs, g_cap, g_acc, p_cap, p_acc;
} hgnn_probe_readout_agg_args;
int hgnn_probe_readout_agg_bwd(const hgnn_probe_readout_agg_args* p, void* stream);

/* csrc/kernels.h DwDenseArgs (launch_dw_dense, launch_dw_readout).  dW (bs, nmax, nmax, jt). */
typedef struct hgnn_probe_dw_dense_args {
    const float* dA;         /* [rows][lda] (launch_dw_dense) */
    const float* xp;         /* [rows][f], or */
    const float* xdense;     /* (bs, f, nmax) */
    const float* pmean;      /* optional BN of the producer of xp: (f), (f), scalar, scalar */
    const float* pstd;
    const float* pw;
    const float* pb;
    const float* dout;       /* optional (bs, dim_out): readout mode */
    const float* fcw;        /* (dim_out, kfc) */
    const int32_t* node_off;
    float* dW;
    int32_t lda, f, jt, dim_out, kfc, bs, nmax, accumulate;
} hgnn_probe_dw_dense_args;
int hgnn_probe_dw_dense(const hgnn_probe_dw_dense_args* p, void* stream);
int hgnn_probe_dw_readout(const hgnn_probe_dw_dense_args* p, void* stream);
/* readout_row_fits(ra, dw): 1 when the readout-row backward fits its LDS (dw optional). */
int hgnn_probe_readout_row_fits(const hgnn_probe_readout_agg_args* ra, const hgnn_probe_dw_dense_args* dw);

#ifdef __cplusplus
}
#endif

#endif /* HGNN_AMD_H */
