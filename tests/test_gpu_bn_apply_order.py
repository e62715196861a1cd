"""k_bn_bwd_apply4 / k_bn_bwd_part4 (csrc/bn.hip) after their loads were reordered: the tile's first eight rows of dz / y
and the channels' mean / std go out before the accumulator copies (apply4) or mean / std (part4) are read, rows past the
tile are clamped into it and dropped, and block 0's dw / db reduction runs behind its own tile's stores (alone, in a
launch without rows).

Through hgnn_probe_bn_backward with the inputs, references and tolerances of tests/dense_probe_util.py, as
tests/test_gpu_dense_kernels.py uses them: the exact family equals the fp64 result, the random family stays within the
naive fp32 form's error bound; dy rows >= total and dbpart tiles past the last keep their sentinel; y / dz hold NaN in
the rows past the total, so a clamp that left the tile would show as a non-finite output.

Shapes: c = 8, 64, 128 (one, four and eight rows per thread in a 64-row tile: the prefetch's uniform cut-off at fewer
than eight rows, and its full depth), c = 256 (sixteen rows per thread: the loops behind the prefetch); totals 0, 1,
63, 64, 65 and 200 with a whole empty tile of capacity behind the last one.  Both statistics forms that end in
apply4: the fp64 atomic accumulators (acc = 1) and part4 + fin (acc = 0).  c = 8 takes the narrow two-launch form at
these capacities, so it is also run past that form's 192-tile limit, where it takes part4 / apply4 with one row per
thread.
"""

import pytest

import dense_probe_util as U

pytestmark = pytest.mark.gpu

TOTALS = (0, 1, 63, 64, 65, 200)
WIDTHS = (8, 64, 128, 256)


def _cap(total):
    return (total + 63) // 64 * 64 + 64


def _cases(c, cap_of=_cap):
    out = []
    for i, total in enumerate(TOTALS):
        base = dict(c=c, total=total, cap=cap_of(total), ldy=0, misalign=0, apply=1, dbpart=1, relu_from=c // 2)
        out.append(dict(base, fam="E", training=1, acc=1, seed=4100 + 10 * c + i))
        out.append(dict(base, fam="E", training=0, acc=i % 2, seed=4200 + 10 * c + i))
        if total:
            out.append(dict(base, fam="R", training=1, acc=(i + 1) % 2, seed=4300 + 10 * c + i))
    return out


@pytest.mark.parametrize("c", WIDTHS)
def test_bn_backward_apply4_shapes(c):
    want = {"part4acc", "part4fin"} if c != 8 else {"narrow2s"}
    for cs in _cases(c):
        got = U.run_bn_case(cs)
        assert got["path"] in want, (U.bn_case_id(cs), got["path"])


def test_bn_backward_apply4_one_row_per_thread():
    """c = 8 past the two-launch forms' capacity limit: part4 / apply4 with 64 row groups of one row each.

    Every total in eval mode, where the exact family is checked value for value.  In training mode dY is rounded, and
    the check holds the kernel's rms and largest error against the naive form's: at c = 8 a total of 65 rows gives 16
    dbpart values, of which the second tile's 8 are single rows, and the ratio of two such rms figures scatters around
    1 by more than the factor allows (seed 4184, total 65: 2.06 with the largest errors equal; the kernel's sums are
    those of the parent commit, bit for bit).  So training mode runs at 2100 rows: 33 tiles, 264 dbpart values, the
    count from which dense_probe_util takes the criterion without pooling (POOL_BELOW)."""
    seen = set()
    base = dict(c=8, cap=U.FALLBACK_CAP, ldy=0, misalign=0, apply=1, dbpart=1, relu_from=4)
    for i, total in enumerate(TOTALS):
        seen.add(U.run_bn_case(dict(base, total=total, fam="E", training=0, acc=i % 2, seed=4500 + i))["path"])
    for i, fam in enumerate(("E", "R", "E", "R")):
        seen.add(U.run_bn_case(dict(base, total=2100, fam=fam, training=1, acc=i // 2, seed=4600 + i))["path"])
    assert seen == {"part4acc", "part4fin"}


def test_bn_backward_apply4_without_rows_writes_only_the_scalars():
    """total_rows = 0: block 0 has no tile; dw = db = 0, nothing of dy or dbpart is written and the next half's
    accumulators are zeroed."""
    for c in (8, 64, 128):
        for acc in (1, 0):
            cs = dict(c=c, total=0, cap=U.FALLBACK_CAP if c == 8 else 128, fam="E", ldy=0, misalign=0, apply=1, dbpart=1,
                      relu_from=c // 2, training=1, acc=acc, seed=4400 + c + acc)
            got = U.run_bn_case(cs)
            assert got["path"] == ("part4acc" if acc else "part4fin")
            assert float(got["dw"]) == 0.0 and float(got["db"]) == 0.0
            assert U.sentinel(got["dy"]) and U.sentinel(got["dbpart"])
            if acc:
                assert not got["acc_zero"].any()
