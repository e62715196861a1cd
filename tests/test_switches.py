"""The HGNN_* kernel switches (CPU): one table in csrc/switches.cpp, read once per process, is the only reader.

The library reads the table on first use, so every setting is looked at from a child process that loads the
library and prints hgnn_switch_value for every name.  The expected values are what each switch meant before the
table existed (the per-site parsers of net.hip, gemm3.hip, gemm_bf3.hip, struct.hip, agg.hip, bn.hip, dwdense.hip and
ccn_small.hip), written out here; they are not derived from the table.
"""

import ast
import json
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "hgnn-2_amd")
LIB = os.environ.get("HGNN_LIB_PATH") or os.path.join(PKG, "hgnn_amd", "libhgnn_amd.so")

# flags and their defaults
FLAGS = {"HGNN_FWD_BF3": 1, "HGNN_DIAG_ID": 0, "HGNN_EVENT_FENCE": 0, "HGNN_BN_ACC": 1, "HGNN_BN_FWD_FIN": 1,
         "HGNN_DA_BF3": 1, "HGNN_SIDE": 1, "HGNN_SERIAL_BWD": 0, "HGNN_READOUT_ROW": 1, "HGNN_BWD_TAIL": 1,
         "HGNN_DW_BF3": 1, "HGNN_DW_XCD": 1, "HGNN_FWD_XCD": 1, "HGNN_DA_XCD": 1, "HGNN_GEMM_DMA": 1,
         "HGNN_DW_NARROW": 1, "HGNN_EXTRACT_LDS": 1, "HGNN_EXTRACT_REG": 1, "HGNN_EXTRACT_SPLIT": 0,
         "HGNN_TIMER_MARKERS": 0, "HGNN_CCN_SMALL_PROF": 0}
TRIS = ("HGNN_EXEC_GRAPH", "HGNN_BN_BWD2")  # include/hgnn_amd.h: -1 unset, 0, 1
INTS = {"HGNN_DW_BLOCKS": 256, "HGNN_FWD_G5": 3, "HGNN_DW_RING": 4, "HGNN_AGG_RPW": 2, "HGNN_DWD_GRID": 256,
        "HGNN_XR_DBG": 0}
NAMES = set(FLAGS) | set(TRIS) | set(INTS)
DEFAULTS = {**FLAGS, **{t: -1 for t in TRIS}, **INTS}
# switches that change no result and select no kernel alternate: not in tests/test_gpu_switches.py GROUPS
DIAGNOSTICS_ONLY = {"HGNN_XR_DBG", "HGNN_CCN_SMALL_PROF", "HGNN_TIMER_MARKERS"}

CHILD_VALUES = """
import ctypes, json, sys
h = ctypes.CDLL(sys.argv[1])
h.hgnn_switch_name.restype = ctypes.c_char_p
out, i, v = {}, 0, ctypes.c_int()
while h.hgnn_switch_name(i) is not None:
    nm = h.hgnn_switch_name(i)
    assert h.hgnn_switch_value(nm, ctypes.byref(v)) == 0
    out[nm.decode()] = v.value
    i += 1
print(json.dumps(out))
"""

CHILD_ROOFLINE = """
import json, sys
sys.path[:0] = [sys.argv[1]]
from hgnn_amd import roofline as R
print(json.dumps([R.split_bf16(R.K_GEMM_FWD, 64), R.diag_id(128, 128, 64)]))
"""


def _child(code, arg, env_extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("HGNN_")}
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", code, arg], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _agg_rows_per_wave(v):
    """agg.hip agg_fwd_v: 1, 2 or 4 rows per wave; any other value runs as 2."""
    return 4 if v == 4 else (1 if v == 1 else 2)


def test_enumeration():
    from hgnn_amd import _lib
    lib = _lib.lib()
    names, i = [], 0
    while lib.hgnn_switch_name(i) is not None:
        names.append(lib.hgnn_switch_name(i).decode())
        i += 1
    assert lib.hgnn_switch_name(-1) is None
    assert len(names) == len(set(names)) == 29
    assert set(names) == NAMES
    import ctypes
    v = ctypes.c_int(77)
    assert lib.hgnn_switch_value(b"HGNN_NOPE", ctypes.byref(v)) == 1  # HGNN_ERR_ARG
    assert lib.hgnn_switch_value(None, ctypes.byref(v)) == 1
    assert v.value == 77


def test_defaults_with_nothing_set():
    assert _child(CHILD_VALUES, LIB, {}) == DEFAULTS


# batches of the values INTEGRATION.md, tests/ and tools/ use, and what each meant before the table
BATCHES = {
    # every flag at the value that is not its default; both tri-states off
    "flipped": ({**{k: str(1 - d) for k, d in FLAGS.items()}, "HGNN_EXEC_GRAPH": "0", "HGNN_BN_BWD2": "0",
                 "HGNN_DW_BLOCKS": "192", "HGNN_FWD_G5": "0", "HGNN_DW_RING": "2", "HGNN_AGG_RPW": "1",
                 "HGNN_DWD_GRID": "0", "HGNN_XR_DBG": "1"},
                {**{k: 1 - d for k, d in FLAGS.items()}, "HGNN_EXEC_GRAPH": 0, "HGNN_BN_BWD2": 0,
                 "HGNN_DW_BLOCKS": 192, "HGNN_FWD_G5": 0, "HGNN_DW_RING": 2, "HGNN_AGG_RPW": 1,
                 "HGNN_DWD_GRID": 0, "HGNN_XR_DBG": 1}),
    # every flag spelled out at its default; both tri-states on.  (HGNN_CCN_SMALL_PROF=0 is the one value here that
    # changed its meaning with the table: the profile print used to come on whenever the variable was present.)
    "explicit": ({**{k: str(d) for k, d in FLAGS.items()}, "HGNN_EXEC_GRAPH": "1", "HGNN_BN_BWD2": "1",
                  "HGNN_DW_BLOCKS": "320", "HGNN_FWD_G5": "1", "HGNN_DW_RING": "3", "HGNN_AGG_RPW": "4",
                  "HGNN_DWD_GRID": "128", "HGNN_XR_DBG": "2"},
                 {**FLAGS, "HGNN_EXEC_GRAPH": 1, "HGNN_BN_BWD2": 1, "HGNN_DW_BLOCKS": 320, "HGNN_FWD_G5": 1,
                  "HGNN_DW_RING": 3, "HGNN_AGG_RPW": 4, "HGNN_DWD_GRID": 128, "HGNN_XR_DBG": 2}),
    # out-of-range HGNN_DW_BLOCKS falls back to 256; HGNN_AGG_RPW=3 is in range and runs as 2 (checked below)
    "ints_a": ({"HGNN_DW_BLOCKS": "8", "HGNN_FWD_G5": "2", "HGNN_DW_RING": "4", "HGNN_AGG_RPW": "3",
                "HGNN_DWD_GRID": "384"},
               {**DEFAULTS, "HGNN_DW_BLOCKS": 256, "HGNN_FWD_G5": 2, "HGNN_DW_RING": 4, "HGNN_AGG_RPW": 3,
                "HGNN_DWD_GRID": 384}),
    # an empty value counts as unset; HGNN_DW_RING=0 is out of range (INTEGRATION.md listed it for a kernel that is
    # gone) and gives the default depth
    "ints_b": ({"HGNN_SIDE": "", "HGNN_DIAG_ID": "", "HGNN_EXEC_GRAPH": "", "HGNN_BN_BWD2": "", "HGNN_DW_RING": "0",
                "HGNN_FWD_G5": "3", "HGNN_AGG_RPW": "2", "HGNN_DW_BLOCKS": "4097"},
               DEFAULTS),
}


@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_documented_values_keep_their_meaning(batch):
    env, want = BATCHES[batch]
    got = _child(CHILD_VALUES, LIB, env)
    assert got == want, {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]}
    assert _agg_rows_per_wave(got["HGNN_AGG_RPW"]) == {"1": 1, "2": 2, "3": 2, "4": 4}[env.get("HGNN_AGG_RPW", "2")]


def test_tri_states_are_three_distinct_states():
    for name in TRIS:
        seen = [_child(CHILD_VALUES, LIB, env)[name] for env in ({}, {name: "0"}, {name: "1"})]
        assert seen == [-1, 0, 1], (name, seen)


def _py_files():
    d = os.path.join(PKG, "hgnn_amd")
    return [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith(".py")]


def test_single_reader():
    csrc = os.path.join(PKG, "csrc")
    readers = [f for f in sorted(os.listdir(csrc)) if "getenv(" in open(os.path.join(csrc, f)).read()]
    assert readers == ["switches.cpp"]
    for path in _py_files():
        for n, line in enumerate(open(path), 1):
            if "environ" in line or "getenv" in line:
                hit = [nm for nm in NAMES if re.search(nm + r"\b", line)]
                assert not hit, f"{path}:{n} reads {hit} itself; ask _lib.switch"


def test_documented_and_covered():
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    missing = [nm for nm in sorted(NAMES) if not re.search(nm + r"\b", doc)]
    assert not missing, f"INTEGRATION.md has no row for {missing}"
    tree = ast.parse(open(os.path.join(REPO, "tests", "test_gpu_switches.py")).read())
    groups = next(ast.literal_eval(n.value) for n in tree.body
                  if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "GROUPS")
    covered = {k for env in groups.values() for k in env}
    assert covered <= NAMES, f"GROUPS sets unknown switches {covered - NAMES}"
    assert NAMES - covered <= DIAGNOSTICS_ONLY, f"no parity group sets {sorted(NAMES - covered - DIAGNOSTICS_ONLY)}"
    assert len(DIAGNOSTICS_ONLY) <= 3


def test_roofline_follows_the_library():
    assert _child(CHILD_ROOFLINE, PKG, {"HGNN_FWD_BF3": "0", "HGNN_DIAG_ID": "1"}) == [False, False]
    assert _child(CHILD_ROOFLINE, PKG, {"HGNN_DIAG_ID": "1"}) == [True, True]
