"""The executor's program in numbers (CPU): workspace bytes, parameter count and BN count of a spread of
configurations (csrc/program.hip build_program lays the workspace out; the three queries need no device).

RECORDED holds what the library of commit b943851 (the parent of the executor's split into program / timer /
replay / net) answered, printed by `python tests/test_program_layout.py` with HGNN_LIB_PATH pointing at that
build; a change of the layout must change these on purpose.
"""

import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kind (0 GNN_simple, 1 GNN_lg), order, bs, nmax, emax, f_in, d, n_layers, j_tot, dim_out
CONFIGS = {
    "lg_o1_d32_L3": (1, 1, 4, 9, 20, 5, 32, 3, 3, 1),
    "lg_o2_d64_L2": (1, 2, 6, 9, 24, 5, 64, 2, 3, 1),
    "lg_o3_d4_L20_j5": (1, 3, 4, 7, 12, 5, 4, 20, 5, 2),
    "lg_o2_d130_L3": (1, 2, 4, 9, 20, 5, 130, 3, 3, 1),  # 2d = 260: the padded c2p differs from c2
    "lg_o1_d32_L3_emax0": (1, 1, 4, 9, 0, 5, 32, 3, 3, 1),
    "simple_d4_L20": (0, 0, 4, 9, 0, 5, 4, 20, 3, 1),
    "simple_d64_L2_j5": (0, 0, 32, 50, 0, 5, 64, 2, 5, 13),
    "simple_d130_L3": (0, 0, 4, 9, 0, 5, 130, 3, 3, 1),
}
# (workspace bytes, parameter tensors, BN layers), recorded from commit b943851
RECORDED = {
    "lg_o1_d32_L3": (1995264, 26, 4),
    "lg_o2_d64_L2": (2021376, 14, 2),
    "lg_o3_d4_L20_j5": (1118976, 230, 38),
    "lg_o2_d130_L3": (22337024, 26, 4),
    "lg_o1_d32_L3_emax0": (1501952, 26, 4),
    "simple_d4_L20": (367872, 116, 19),
    "simple_d64_L2_j5": (17946368, 8, 1),
    "simple_d130_L3": (6044928, 14, 2),
}
INVALID = {
    "wide": (1, 1, 4, 9, 20, 5, 257, 3, 3, 1),      # 2d > 512
    "j_tot_8": (1, 1, 4, 9, 20, 5, 32, 3, 8, 1),
    "one_layer": (0, 0, 4, 9, 0, 5, 32, 1, 3, 1),
}


def _answers(cfg_tuple):
    from hgnn_amd import _lib as L
    cfg = L.NetConfig()
    (cfg.kind, cfg.order, cfg.bs, cfg.nmax, cfg.emax, cfg.f_in, cfg.d, cfg.n_layers, cfg.j_tot,
     cfg.dim_out) = cfg_tuple
    cfg.training = 1
    lib = L.lib()
    return (lib.hgnn_net_workspace_bytes(ctypes.byref(cfg)), lib.hgnn_net_param_count(ctypes.byref(cfg)),
            lib.hgnn_net_bn_count(ctypes.byref(cfg)))


def test_layout_matches_the_recorded_one():
    assert set(RECORDED) == set(CONFIGS)
    got = {name: _answers(t) for name, t in CONFIGS.items()}
    assert got == RECORDED, {k: (got[k], RECORDED[k]) for k in CONFIGS if got[k] != RECORDED[k]}


def test_counts_follow_the_network():
    """12 (GNN_lg) or 6 (GNN_simple) parameter tensors and 2 or 1 BN layers per layer but the last, plus fc."""
    for name, t in CONFIGS.items():
        kind, layers = t[0], t[7]
        assert RECORDED[name][1] == (12 if kind else 6) * (layers - 1) + 2, name
        assert RECORDED[name][2] == (2 if kind else 1) * (layers - 1), name


def test_invalid_configurations():
    for name, t in INVALID.items():
        assert _answers(t) == (0, -1, -1), name


if __name__ == "__main__":
    for p in (REPO, os.path.join(REPO, "hgnn-2_amd")):
        sys.path.insert(0, p)
    print("RECORDED = {")
    for name, t in CONFIGS.items():
        print(f"    {name!r}: {_answers(t)!r},")
    print("}")
