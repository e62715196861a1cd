// The HGNN_* kernel switches: one table, read from the environment once per process by switches.cpp; every launcher
// reads a field of switches().  A row is X(type, field, variable, default, min, max, description); how its value is
// read depends on the type alone:
//   bool: unset or empty = the default; a first character '0' = off; anything else = on
//   Tri:  unset or empty = Auto; a first character '0' = Off; anything else = On
//   int:  the whole string must parse (strtol) and lie in [min, max]; otherwise the default
#pragma once

namespace hgnn {

enum class Tri : int { Auto = -1, Off = 0, On = 1 };

#define HGNN_SWITCH_TABLE(X)                                                                                         \
    X(bool, fwd_bf3, "HGNN_FWD_BF3", 1, 0, 1, "forward GEMM on split-bf16 MFMA (0: fp32 MFMA)")                      \
    X(bool, diag_id, "HGNN_DIAG_ID", 0, 0, 1, "the GEMMs build the diagonal I / D operand columns")                  \
    X(bool, event_fence, "HGNN_EVENT_FENCE", 0, 0, 1, "fork / join events keep the system-scope fence")              \
    X(bool, bn_acc, "HGNN_BN_ACC", 1, 0, 1, "BN statistics by fp64 atomics (0: per-tile partials + fin)")            \
    X(bool, bn_fwd_fin, "HGNN_BN_FWD_FIN", 1, 0, 1, "forward BN finalize in the GEMM's last block")                  \
    X(bool, da_bf3, "HGNN_DA_BF3", 1, 0, 1, "dA GEMM on split-bf16 MFMA at 2d <= 128 (0: fp32 k_gemm5)")             \
    X(bool, side, "HGNN_SIDE", 1, 0, 1, "weight-gradient work on a side stream")                                     \
    X(bool, serial_bwd, "HGNN_SERIAL_BWD", 0, 0, 1, "diagnostics: the whole backward on the main stream")            \
    X(bool, readout_row, "HGNN_READOUT_ROW", 1, 0, 1, "readout-row backward kernels (0: materialised gradient)")     \
    X(bool, bwd_tail, "HGNN_BWD_TAIL", 1, 0, 1, "the shortened backward tail (0: the round-4 tail)")                 \
    X(bool, dw_bf3, "HGNN_DW_BF3", 1, 0, 1, "dW GEMM on split-bf16 MFMA (0: fp32 k_gemm3_tn)")                       \
    X(bool, dw_xcd, "HGNN_DW_XCD", 1, 0, 1, "XCD-aware block order of the dW GEMM")                                  \
    X(bool, fwd_xcd, "HGNN_FWD_XCD", 1, 0, 1, "XCD-aware block order of the fp32 forward GEMM")                      \
    X(bool, da_xcd, "HGNN_DA_XCD", 1, 0, 1, "XCD-aware block order of the fp32 dA GEMM")                             \
    X(bool, gemm_dma, "HGNN_GEMM_DMA", 1, 0, 1, "fp32 dA GEMM with LDS-DMA staging (0: k_gemm3)")                    \
    X(bool, dw_narrow, "HGNN_DW_NARROW", 1, 0, 1, "dense dW from LDS at F <= 16 (0: the MFMA kernel)")               \
    X(bool, extract_lds, "HGNN_EXTRACT_LDS", 1, 0, 1, "LDS- / register-staged operator extraction")                  \
    X(bool, extract_reg, "HGNN_EXTRACT_REG", 1, 0, 1, "register-staged extraction (0: the LDS-staged one)")          \
    X(bool, extract_split, "HGNN_EXTRACT_SPLIT", 0, 0, 1, "diagnostics: one k_extract launch per block slot")        \
    X(bool, timer_markers, "HGNN_TIMER_MARKERS", 0, 0, 1, "hgnn_timer_create makes a marker-event timer")            \
    X(bool, ccn_small_prof, "HGNN_CCN_SMALL_PROF", 0, 0, 1, "diagnostics: phase cycles of the small CCN forward")    \
    X(Tri, exec_graph, "HGNN_EXEC_GRAPH", -1, -1, 1, "HIP-graph replay of repeated calls: by size / never / always") \
    X(Tri, bn_bwd2, "HGNN_BN_BWD2", -1, -1, 1, "two-launch BN backward: narrow widths / none / narrow and wide")     \
    X(int, dw_blocks, "HGNN_DW_BLOCKS", 256, 16, 4096, "target block count of the dW GEMM")                          \
    X(int, fwd_g5, "HGNN_FWD_G5", 3, 0, 3, "fp32 forward k_gemm5: never / 64 x 64 tiles / always / 64 x 32 tiles")   \
    X(int, dw_ring, "HGNN_DW_RING", 4, 2, 4, "load-ring depth of the split-bf16 dW GEMM")                            \
    X(int, agg_rpw, "HGNN_AGG_RPW", 2, 1, 4, "rows per wave of the forward aggregation (1, 2 or 4; 3 runs as 2)")    \
    X(int, dwd_grid, "HGNN_DWD_GRID", 256, 0, 65535, "blocks of the dense dW (0: one per graph)")                    \
    X(int, xr_dbg, "HGNN_XR_DBG", 0, 0, 2, "diagnostics: a truncated k_extract_reg launch ahead of the real one")

struct Switches {
#define X(type, field, ...) type field;
    HGNN_SWITCH_TABLE(X)
#undef X
    bool dw_blocks_given;  // HGNN_DW_BLOCKS is set: no doubling for the wide networks (gemm3.hip dw3_chunks)
};

const Switches& switches();

}  // namespace hgnn
