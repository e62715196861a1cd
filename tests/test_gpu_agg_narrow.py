"""The several-rows-per-wave aggregation kernels for narrow rows (csrc/agg.hip k_agg_fwd_narrow, k_agg_bwd_narrow: a
group of 8 lanes per row, 8 rows per wave, taken for c_g <= 8 and c_p <= 8 in the forward and c <= 8 in the backward),
through hgnn_probe_agg_fwd / hgnn_probe_agg_bwd with the inputs and checks of tests/sparse_probe_util.py:

  * exact families A1 / A3 bit for bit against fp64, family AR within 2 x the naive fp32 form's error;
  * containment: the sentinel stays in rows >= total, in the columns the launch does not write, in the padding under
    pad_from = -1 and behind an explicit pad_from;
  * poison: NaN in unused entry slots, in the list rows past the total, in feature rows past the source's total and in
    the columns of ing / inp outside the blocks read.

What the table of that file does not hold and a wave of eight rows needs: rows of 0, 1, 7, 8, 9, 17 and 130 entries
next to each other in one wave (groups that finish early, the second and later 8-entry chunks, the wave's trip count
from its longest row), G and P lists of different length in every row, totals 1, 7, 8, 9 and 33 under a capacity
rounded up to 16 (a wave's last partial group, a block's last partial wave, a second block), an ldo of 1 to 3
padding columns, every J_tot with its own entry layout (3: one float4; 4 and 7: two), BN on load on either part.
Family AR runs at 300 rows (ten blocks), the small totals in the exact families: its criterion holds two roundings
of the same sums against each other by their rms and largest error, and over the 3 to 16 outputs of a one-row launch
the ratio of two largest errors is one element's luck (the one-row-per-wave kernel, unchanged here, measured 2.08 on
16 outputs at total 1); 300 rows give every width at least 300 outputs, as many as the dense probes ask before they
take the criterion without pooling (tests/dense_probe_util.py POOL_BELOW).  The exact families are the stronger
check -- bit for bit -- and cover every total.
c = 9 and c = 16 (and a narrow part beside a wider one) run on the one-row-per-wave kernels with the same data, so
the dispatch boundary is met from both sides.
"""

import numpy as np
import pytest

import sparse_probe_util as U

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 7, 8, 9, 17, 130)
COUNTS_A3 = (0, 1, 7, 8, 9, 17, 32)       # (family A3 stays exact up to 32 entries per row)
TOTALS = ((1, 16), (7, 16), (8, 16), (9, 16), (33, 48))
AR_ROWS = (300, 304)                      # family AR: see the docstring
FWD_WIDTHS = ((1, 5), (5, 1), (8, 0), (8, 8), (1, 0), (0, 5))
FWD_NEIGHBOURS = ((9, 9), (16, 16), (9, 0), (8, 9), (9, 8), (0, 16))
JTOT = (3, 4, 7)
BWD_C = (1, 5, 8)
BWD_NEIGHBOURS = (9, 16)


def mixed_counts(total, fam="A1"):
    """(G count, P count) of rows 0 .. total - 1: with seven counts and eight rows per wave every wave holds every
    count in both lists, and the two lists of a row differ."""
    cs = COUNTS_A3 if fam == "A3" else COUNTS
    n = len(cs)
    return [(cs[r % n], cs[(r + 3) % n]) for r in range(total)]


@pytest.fixture(autouse=True)
def _mixed_rows(monkeypatch):
    # fwd_data / bwd_data take their per-row entry counts from pair_counts
    monkeypatch.setattr(U, "pair_counts", mixed_counts)


def _fwd(cg, cp, jt, total, cap, fam, bn, pad, ldo_pad, seed):
    c = dict(cg=cg, cp=cp, jtot=jt, total=total, cap=cap, fam=fam, bn=bn, pad=pad, j0=0, ldo=0, seed=seed)
    if ldo_pad:
        c["ldo"] = U.fwd_geometry(c)[0] + ldo_pad
    return c


def fwd_cases(widths):
    out = []
    i = 0
    for (cg, cp) in widths:
        for jt in JTOT:
            # every total at J_tot 3; the others at the one-group, the full-wave and the two-block totals
            for (total, cap) in (TOTALS if jt == 3 else (TOTALS[0], TOTALS[3], TOTALS[4])):
                pad = (0, -1, "explicit", 0)[i % 4]
                ldo_pad = (1, 0, 0, 3, 2, 0)[i % 6] if pad == 0 else 0
                out.append(_fwd(cg, cp, jt, total, cap, ("A1", "A3")[i % 2], i % 4, pad, ldo_pad, 7000 + i))
                i += 1
            out.append(_fwd(cg, cp, jt, *AR_ROWS, "AR", i % 4, (0, -1, "explicit")[i % 3], 0, 7000 + i))
            i += 1
        # BN on load on and off on both parts: exact at the two-block total, AR at its own
        for bn in (0, 3):
            for (fam, (total, cap)) in (("A1", TOTALS[4]), ("AR", AR_ROWS)):
                out.append(_fwd(cg, cp, 3, total, cap, fam, bn, 0, 1 + i % 3, 7000 + i))
                i += 1
    return out


def bwd_cases(widths):
    out = []
    i = 0
    for c in widths:
        for kind in ("g", "p"):
            for acc in (0, 1):
                for jt in (JTOT if kind == "g" else (3,)):
                    rows = [(t, ("A1", "A3")[(i + k) % 2]) for k, t in enumerate(TOTALS if jt == 3 else TOTALS[3:])]
                    for ((total, cap), fam) in rows + [(AR_ROWS, "AR")]:
                        out.append(dict(kind=kind, c=c, jtot=jt, gofs=U.BWD_GOFS[i % 2], total=total, cap=cap, acc=acc,
                                        fam=fam, odd=i % 2, seed=8000 + i))
                        i += 1
    return out


def test_the_case_tables_hold_what_they_promise():
    for fam in ("A1", "A3"):
        pairs = mixed_counts(8, fam)
        cs = COUNTS_A3 if fam == "A3" else COUNTS
        assert {a for a, _ in pairs} == set(cs) == {b for _, b in pairs} and all(a != b for a, b in pairs)
    f = fwd_cases(FWD_WIDTHS)
    assert {(c["cg"], c["cp"]) for c in f} == set(FWD_WIDTHS)
    for w in FWD_WIDTHS:
        mine = [c for c in f if (c["cg"], c["cp"]) == w]
        assert {c["jtot"] for c in mine} == set(JTOT)
        assert {c["total"] for c in mine if c["fam"] != "AR"} == {t for t, _ in TOTALS}
        assert all(c["total"] == AR_ROWS[0] for c in mine if c["fam"] == "AR")
        assert {c["bn"] for c in mine} >= {0, 3} and {c["fam"] for c in mine} == {"A1", "A3", "AR"}
        assert {c["ldo"] - U.fwd_geometry(c)[0] for c in mine if c["ldo"]} == {1, 2, 3}
        assert {c["pad"] for c in mine} == {0, -1, "explicit"}
    b = bwd_cases(BWD_C)
    for c in BWD_C:
        for kind in ("g", "p"):
            mine = [x for x in b if x["c"] == c and x["kind"] == kind]
            assert {x["acc"] for x in mine} == {0, 1} and {x["fam"] for x in mine} == {"A1", "A3", "AR"}
            assert {x["total"] for x in mine if x["fam"] != "AR"} == {t for t, _ in TOTALS}
            assert {x["jtot"] for x in mine} == (set(JTOT) if kind == "g" else {3})


@pytest.mark.parametrize("cg,cp", FWD_WIDTHS)
def test_agg_forward_narrow(cg, cp):
    for c in fwd_cases(((cg, cp),)):
        U.check_fwd(c)


@pytest.mark.parametrize("cg,cp", FWD_NEIGHBOURS)
def test_agg_forward_beside_the_narrow_widths(cg, cp):
    for c in fwd_cases(((cg, cp),)):
        U.check_fwd(c)


@pytest.mark.parametrize("c", BWD_C)
def test_agg_backward_narrow(c):
    for x in bwd_cases((c,)):
        U.check_bwd(x)


@pytest.mark.parametrize("c", BWD_NEIGHBOURS)
def test_agg_backward_beside_the_narrow_widths(c):
    for x in bwd_cases((c,)):
        U.check_bwd(x)


def test_agg_backward_narrow_accumulates_onto_the_old_row_only():
    """An accumulating launch over rows without entries returns the old rows bit for bit, negative zeros included
    (slots past a row's own count leave its accumulator alone, whatever the wave's longest row is)."""
    for kind in ("g", "p"):
        c = dict(kind=kind, c=5, jtot=3, gofs=0, total=33, cap=48, acc=1, fam="A1", odd=0, seed=8900)
        d = U.bwd_data(c)
        l = d["list"]
        empty = [r for r in range(c["total"]) if l["cnt"][r] == 0]
        assert empty and any(l["cnt"][r // 8 * 8:r // 8 * 8 + 8].max() >= 130 for r in empty)
        d["out0"][empty, :5] = -0.0
        st, out = U.call_bwd(d)
        assert st == 0
        U.check_bwd_output("aggbwd-narrow-old-rows-" + kind, d, out)
        assert np.array_equal(out[empty].view(np.int32), d["out0"][empty].view(np.int32))
