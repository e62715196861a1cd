"""The dense side outside the GEMMs one launcher at a time: the five launch sequences of the BN backward,
k_bn_finalize, the readout launchers (csrc/bn.hip) and the dense operator gradient (csrc/dwdense.hip, k_dw_readout),
against plain numpy fp64 references.

Through the probes of csrc/probe_dense.hip (include/hgnn_amd.h "Kernel probes") every launcher is handed what the
whole-network tests never present: channel counts whose float4 lane count does not divide 256 (12, 20, 40, 100, 516),
one row group (1024), the scalar path past 256 channels, with a padded dY stride and with a 4-byte-offset dy, row
counts around the 64- and 256-row tiles with empty tiles of capacity behind them, the fall-back past 192 capacity
tiles, the statistics alone (apply = 0), the fp64 accumulator ping-pong, finalize over 1 .. 600 tiles, readout widths
past 1024 columns, graphs of 0 .. 17 nodes, 300 edge rows in one graph, every reachable instantiation of k_dw_dense.
tests/dense_probe_util.py holds the inputs, the case tables and the checks; tests/test_dense_probe_inputs.py checks
those on the CPU.

Every case: the exact family equals fp64 rounded once bit for bit wherever a sum is observable (the sign of a zero
aside); the random family's rms and max error against fp64 are at most 2 x those of the naive fp32 form; outputs
pre-filled with a sentinel keep it where nothing may be written; NaN in the scratch on entry, in the rows past the
total and in unused list slots reaches no output.  The BN backward asserts the launch sequence the launcher reports
(kernels.h bn_bwd_variant, which launch_bn_backward itself dispatches on) for every case.

Which k_dw_dense instantiation runs for which shape (launch_dw_dense's rule: FC from the padded node count and F,
MAXI from the items per wave, the items split over gridDim.y below 256 graphs; asserted on the table by
tests/test_dense_probe_inputs.py):
  narrow                F <= 16, no readout vector (HGNN_DW_NARROW=0: the MFMA kernel below)
  <128, 1>  nmax <= 32, F > 64              <128, 3>  the same with jt = 5 and >= 256 graphs
  <64, 1>   nmax <= 32, F <= 64             <64, 3>   the same with jt = 5 and >= 256 graphs
  <32, 1>   nmax 33 .. 64, < 256 graphs     <32, 3>   jt 2, >= 256 graphs     <32, 5>  jt 4, >= 256 graphs
  <16, 1>   nmax 65 .. 100, < 256 graphs    <16, 5>   >= 256 graphs (nmax 100, jt 3: three passes over the items)
  not covered: <128, 5>, <64, 5> (more than 12 slices), <16, 3> (a 3 x 3 tile grid has at least 18 items) and every
  <8, *> (FC = 8 needs more than 160 KB of LDS at FC = 16: nmax above ~450) cannot be reached with nmax <= 100.

Random family, measured on an MI355X (error against fp64 of the kernel / of the naive fp32 form, the case with the
worst ratio of each row; then the range of the rms ratio and the largest max ratio over the row's widths; the bound
is 2.00).  BN backward: an output of 256 values or more is held to the naive form in the stored row order; a smaller
one (a narrow layer's statistics, one tile's column sums, the scalars dw and db) to the naive form pooled over 8 row
orders (4 from 512 channels on) -- the rms over all orders' errors, the largest of their max errors; a single value
only to the latter (dense_probe_util.check_bound says why, with the case that forced it).

  kernel, output       widths             rms kernel / naive   max kernel / naive   rms ratio    max ratio
  scalar sums          1 .. 260           6.86e-06 / 6.31e-06  2.44e-05 / 2.11e-05  0.46 .. 1.09   1.16
  scalar dy            1 .. 260           1.11e-07 / 8.38e-08  3.60e-07 / 2.41e-07  0.54 .. 1.33   1.49
  scalar dbpart        1 .. 260           4.72e-06 / 3.32e-06  1.43e-05 / 1.02e-05  0.26 .. 1.42   1.40
  scalar dw            1 .. 260           9.65e-06 / 9.65e-06  (one value)          0.20 .. 1.00   1.00
  scalar db            1 .. 260           1.70e-05 / 1.70e-05  (one value)          0.30 .. 1.00   1.00
  narrow2s dy          4, 8, 16           1.31e-07 / 2.05e-07  6.91e-07 / 6.23e-07  0.46 .. 0.78   1.11
  narrow2s dbpart      4, 8, 16           3.60e-06 / 7.52e-06  7.79e-06 / 1.98e-05  0.38 .. 0.48   0.39
  narrow2s dw          4, 8, 16           2.20e-05 / 2.38e-05  (one value)          0.38 .. 0.92   0.92
  narrow2s db          4, 8, 16           1.65e-05 / 1.65e-05  (one value)          0.60 .. 1.00   1.00
  part4fin sums        12 .. 1024         6.94e-06 / 6.38e-06  2.64e-05 / 2.70e-05  0.43 .. 1.09   1.02
  part4fin dy          12 .. 1024         1.77e-07 / 1.78e-07  4.33e-06 / 3.38e-06  0.52 .. 0.99   1.28
  part4fin dbpart      12 .. 1024         4.08e-06 / 3.41e-06  1.71e-05 / 1.61e-05  0.44 .. 1.20   1.06
  part4fin dw          12 .. 1024         1.45e-04 / 8.38e-05  (one value)          0.10 .. 1.73   1.73
  part4fin db          12 .. 1024         4.99e-04 / 4.99e-04  (one value)          0.39 .. 1.00   1.00
  part4acc dy          12 .. 1024         8.38e-08 / 5.76e-07  1.86e-06 / 3.42e-06  0.13 .. 0.19   0.54
  part4acc dbpart      12 .. 1024         4.09e-06 / 2.24e-05  1.81e-05 / 7.04e-05  0.08 .. 0.18   0.26
  part4acc dw          12 .. 1024         7.74e-05 / 1.06e-04  (one value)          0.01 .. 0.73   0.73
  part4acc db          12 .. 1024         4.79e-06 / 4.79e-06  (one value)          0.00 .. 1.00   1.00
  readout_fwd out      k 1 .. 1300        3.65e-07 / 4.52e-07  7.99e-07 / 1.21e-06  0.03 .. 0.81   0.66
  readout_bwd_da       k 1 .. 1300        5.72e-08 / 6.16e-08  6.51e-07 / 6.51e-07  0.26 .. 0.93   1.00
  readout_agg_bwd G    C 5 .. 512         3.36e-07 / 3.31e-07  2.77e-06 / 1.67e-06  0.92 .. 1.01   1.66
  readout_agg_bwd P    C 5 .. 512         2.61e-07 / 2.92e-07  9.05e-06 / 5.31e-06  0.93 .. 1.01   1.70
  dw_dense narrow      F 1 .. 16          5.74e-08 / 6.38e-08  9.26e-07 / 9.02e-07  0.90 .. 0.99   1.03
  dw_dense <64, *>     F 1 .. 64          6.88e-07 / 7.06e-07  8.82e-06 / 8.07e-06  0.75 .. 1.01   1.23
  dw_dense <128, *>    F 65 .. 130        8.65e-06 / 7.69e-06  5.11e-05 / 3.88e-05  0.98 .. 1.13   1.32
  dw_dense <32, *>     F 17 .. 65         1.87e-07 / 2.09e-07  2.84e-06 / 1.98e-06  0.92 .. 0.98   1.44
  dw_dense <16, *>     F 5 .. 130         4.52e-07 / 4.23e-07  2.91e-06 / 2.97e-06  0.98 .. 1.07   1.00
  dw_readout           F 1 .. 130         8.65e-06 / 7.69e-06  5.11e-05 / 3.88e-05  0.78 .. 1.13   1.32
  (part4acc's rows are the 1030-row cases: the naive form sums 1030 terms in sequence, the kernel 64-row tiles in
  fp32 and the tiles in fp64.  wide2 runs only in the HGNN_BN_BWD2=1 child process and is asserted there, not
  tabulated.  dw / db at ratio 1.00: the kernel returned the bits of one of the naive orders.  The exact family's
  training-mode dy and dbpart, inexact through the rounded 1 / total, are held to the same rule: rms ratios 0.40 ..
  1.99 (narrow2s dbpart, c = 4, one tile: four values), max ratios at most 1.51.  colsum, dfcw, dfcb and the
  finalize's mean / std are held to 1 fp32 ulp of fp64 instead; on the partials path the finalize's reference is the
  fp64 combination of the fp32 partials as given.)

Wrong-value mutants (scratch builds, not committed), each failing the test named: k_bn_bwd_part4 skipping its last row
group -- test_bn_backward[4] (statistics, apply = 0); apply4 taking statistic 1 for m1 -- test_bn_backward[12];
apply2 summing the neighbouring dbpart tile -- test_switch_selected_variants (bn_bwd2=1); apply2s without the
wave-to-tile offset -- test_bn_backward[4]; k_bn_bwd_fin stopping at 64 tiles --
test_bn_backward_statistics_over_more_than_64_tiles; k_readout_fwd without its tail rows --
test_readout_fwd_and_bwd_da[1]; k_readout_agg_bwd without the j >= 3 coefficients of its unrolled entries --
test_readout_agg_bwd[5]; k_dw_dense<32, *> without its last F chunk -- test_dw_dense_and_dw_readout[64].

Found by these tests: launch_readout_agg_bwd and readout_row_fits accepted jt = 8.  A list entry is 8 floats, the
column and at most 7 coefficients, so at jt = 8 k_readout_agg_bwd took the next entry's column bits for the eighth
coefficient (and read one float past the list for its last entry).  The executor never builds such a list (j_tot
<= 7, program.hip), so no network result changes; both now refuse jt > 7 and a list stride below 1 + jt.
"""

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dense_probe_util as U

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- BN backward
@pytest.mark.parametrize("c", U.BN_WIDTHS)
def test_bn_backward(c):
    assert U.run_bn_cases((c,)) >= 20


def test_bn_backward_forced_to_the_scalar_path():
    for cs in U.bn_scalar_forced_cases():
        assert U.run_bn_case(cs)["path"] == "scalar"


def test_bn_backward_statistics_over_more_than_64_tiles():
    for cs in U.bn_many_tiles_cases():
        assert U.run_bn_case(cs)["path"] in ("part4fin", "scalar")


def test_bn_backward_falls_back_past_192_tiles_and_agrees_with_two_launch():
    """cap_rows past 192 x 256: part4 (+ fin) + apply4 instead of the two-launch form, the same result on the same
    data.  y / dz / dy hold `total` rows only: no kernel touches a row >= total (every row loop ends at min(total,
    r0 + tile), the two-launch forms clamp their unconditional loads to r1 - 1)."""
    for training in (0, 1):
        for acc in (0, 1):
            two = dict(c=4, total=300, cap=448, fam="E", training=training, apply=1, dbpart=1, acc=acc, relu_from=2,
                       ldy=0, misalign=0, seed=4242)
            far = dict(two, cap=U.FALLBACK_CAP, alloc=320)
            a, b = U.run_bn_case(two), U.run_bn_case(far)
            assert a["path"] == "narrow2s" and b["path"] == ("part4acc" if acc else "part4fin")
            for k in ("dw", "db"):
                assert np.array_equal(np.float32(a[k]).view(np.int32), np.float32(b[k]).view(np.int32)), k
            assert np.array_equal(a["dy"][:300].view(np.int32), b["dy"][:300].view(np.int32))
            # the column sums of a training-mode dy (inexact terms) depend on the order, which differs between
            # apply2s (wave shuffles) and apply4 (a serial walk over the row groups): each is held to the bound above
            if not training:
                assert np.array_equal(a["dbpart"][:5].view(np.int32), b["dbpart"][:5].view(np.int32))


@pytest.mark.parametrize("c", (12, 8, 5, 1024))
def test_bn_backward_accumulator_ping_pong(c):
    """acc64 = A, zero = B; then acc64 = B, zero = A; then A again: the third call equals the first bit for bit, and
    acc64_zero is all zero after every call, whether apply4 or the memset zeroed it."""
    cs = dict(c=c, total=300, cap=448, fam="E", training=1, apply=1, dbpart=1, acc=1, relu_from=c // 2, ldy=0,
              misalign=0, seed=99 + c)
    d = U.bn_data(cs)
    d2 = U.bn_data(dict(cs, seed=199 + c))
    A, B = U._full(32 * c, 0.0, torch.float64), U._full(32 * c, 0.0, torch.float64)
    r1 = U.call_bn_bwd(cs, d, A, B)
    U.check_bn_bwd(cs, d, r1)
    r2 = U.call_bn_bwd(cs, d2, B, A)
    U.check_bn_bwd(cs, d2, r2)
    r3 = U.call_bn_bwd(cs, d, A, B)
    U.check_bn_bwd(cs, d, r3)
    for k in ("dy", "dbpart"):
        assert np.array_equal(r1[k].view(np.int32), r3[k].view(np.int32)), k
    assert r1["dw"] == r3["dw"] and r1["db"] == r3["db"]


def test_bn_backward_refusals():
    L = U._L()
    cs = dict(c=8, total=65, cap=192, fam="E", training=1, apply=1, dbpart=0, acc=0, relu_from=4, ldy=0, misalign=0,
              seed=5)
    d = U.bn_data(cs)
    assert L.lib().hgnn_probe_bn_backward(None, U._stream()) == U.ERR_ARG
    a = L.ProbeBnBackward()
    assert L.lib().hgnn_probe_bn_backward(ctypes.byref(a), U._stream()) == U.ERR_ARG
    with pytest.raises(AssertionError, match="status"):       # ldy below c: launch_bn_backward's own HGNN_ERR_ARG
        U.call_bn_bwd(dict(cs, ldy=4), d)


# ---------------------------------------------------------------------------------------------- BN finalize
@pytest.mark.parametrize("c", U.FIN_C)
def test_bn_finalize(c):
    cases = [x for x in U.fin_cases() if x["c"] == c]
    assert len(cases) == 4 * len(U.FIN_TILES)
    for cs in cases:
        d = U.fin_data(cs)
        got = U.call_fin(cs, d, with_run=bool(cs["run"]))
        U.check_fin("fin c{c} t{tiles} last{last} {fam} {mode}".format(**cs), d, got, cs["mode"], cs["fam"] == "E")


def test_bn_finalize_without_rows_and_in_eval_mode():
    g = np.random.default_rng(3)
    for mode in ("part", "acc"):
        cs = dict(c=5, mode=mode)
        d = U.fin_from_y(np.zeros((0, 5), np.float32), g)
        got = U.call_fin(cs, d)
        assert not got["mean"].any() and (got["std"] == np.float32(np.sqrt(1e-5))).all()
        U.check_fin("fin rows 0 " + mode, d, got, mode, True)
        d = U.fin_data(dict(c=5, tiles=3, last=37, fam="R", seed=8))
        got = U.call_fin(cs, d, training=0)
        for k in ("mean", "std"):     # eval: the running statistics, copied; themselves unchanged
            assert np.array_equal(got[k].view(np.int32), d["run_" + k].view(np.int32))
            assert np.array_equal(got["run_" + k].view(np.int32), d["run_" + k].view(np.int32))


@pytest.mark.parametrize("v", (3.0, 0.1))
def test_bn_finalize_constant_channel_clamps_the_variance(v):
    """The atomic form's Q / N - mean^2 of a constant channel: 0, and with a sum of squares that came out low (by
    half of the 1e-5 the variance starts from, so that an unclamped difference would show in the result) negative
    before the clamp: std = sqrt(1e-5) rounded."""
    g = np.random.default_rng(4)
    Y = g.standard_normal((300, 4)).astype(np.float32)
    Y[:, 1] = np.float32(v)
    d = U.fin_from_y(Y, g)
    for nudge in (0, 1):
        d["acc"][0, 1, 1] -= nudge * 0.5e-5 * 300
        got = U.call_fin(dict(c=4, mode="acc"), d)
        assert got["std"][1] == np.float32(np.sqrt(1e-5)) and got["mean"][1] == np.float32(v), (nudge, got)
        U.check_fin(f"fin const {v} nudge {nudge}", d, got, "acc", True)


# ---------------------------------------------------------------------------------------------- readout
@pytest.mark.parametrize("k", U.RO_K)
def test_readout_fwd_and_bwd_da(k):
    for o in U.RO_DIM_OUT:
        for fam in ("E", "R"):
            d = U.ro_data(k, o, fam, seed=100 * k + o)
            name = f"readout k{k} o{o} {fam}"
            U.check_ro_fwd(name, d, U.call_ro_fwd(d))
            U.check_ro_da(name, d, U.call_ro_da(d))


@pytest.mark.parametrize("bs", U.RO_BS)
def test_readout_bwd_params(bs):
    for k in U.RO_PARAM_K:
        for o in U.RO_DIM_OUT:
            for fam in ("E", "R"):
                d = U.ro_param_data(bs, k, o, fam, seed=bs * 1000 + k + o)
                U.check_ro_params(f"readout params bs{bs} k{k} o{o} {fam}", d, U.call_ro_params(d))


@pytest.mark.parametrize("C", U.AGG_C)
def test_readout_agg_bwd(C):
    for cs in U.agg_cases(C):
        U.run_agg_case(cs)


def test_readout_agg_bwd_refuses_more_slices_than_an_entry_holds():
    """jt = 8 and 9: HGNN_ERR_UNSUPPORTED from the launcher, in agreement with readout_row_fits; nothing written.
    (cg is lowered with jt so that every column a launch would read stays inside fcw.)"""
    L = U._L()
    cs = dict(C=5, jt=7, stride=8, fam="E", g=1, p=1, g_acc=0, p_acc=0, mis=0, lds=0, seed=31)
    d = U.agg_data(cs)
    for over in (dict(jt=8, cg=4), dict(jt=9, cg=3)):
        st, fits, gg, gp = U.call_agg(cs, d, over)
        assert st == U.ERR_UNSUPPORTED and fits == 0, (over, st, fits)
        assert np.array_equal(gg[:len(d["g0"])], d["g0"]) and np.array_equal(gp[:len(d["p0"])], d["p0"])
    # a stride-4 list cannot hold 4 coefficients
    cs4 = dict(cs, jt=3, stride=4)
    d4 = U.agg_data(cs4)
    st, _, gg, _ = U.call_agg(cs4, d4, dict(jt=4, cg=3))
    assert st == U.ERR_UNSUPPORTED and np.array_equal(gg[:len(d4["g0"])], d4["g0"])
    assert L.lib().hgnn_probe_readout_agg_bwd(None, U._stream()) == U.ERR_ARG


# ---------------------------------------------------------------------------------------------- dense dW
@pytest.mark.parametrize("F", sorted({c["F"] for c in U.dw_cases()}))
def test_dw_dense_and_dw_readout(F):
    assert U.run_dw_cases(only=lambda cs: cs["F"] == F) >= 4


def test_dw_readout_lds_opt_in_and_refusal_agree_with_readout_row_fits():
    """k_dw_readout's dynamic LDS below 64 KB, between 64 KB and 160 KB (the opt-in) and past 160 KB (refused, nothing
    written): readout_row_fits(ra, dw) says the same as launch_dw_readout does."""
    L = U._L()
    acs = dict(C=5, jt=4, stride=8, fam="E", g=1, p=1, g_acc=0, p_acc=0, mis=0, lds=0, seed=41)
    keep = []
    ra = U.agg_struct(acs, U.agg_data(acs), keep)[0]
    for F, fits in ((16, 1), (170, 1), (420, 0)):
        cs = dict(F=F, nmax=100, jt=4, bs=1, fam="E", bn=1, xdense=0, dout=1, acc=0, ldx=0, seed=70 + F)
        d = U.dw_data(cs)
        lds = U.dw_readout_lds_bytes(cs)
        assert fits == int(lds <= 160 * 1024) and (F != 170 or lds > 64 * 1024), (F, lds)
        dwa = U.dw_struct(cs, d, keep)[0]
        assert L.lib().hgnn_probe_readout_row_fits(ctypes.byref(ra), ctypes.byref(dwa)) == fits, F
        st, got = U.call_dw(cs, d, readout=True)
        if fits:
            assert st == 0, (F, st)
            U.check_dw(f"dw_readout F{F} lds {lds}", cs, d, got)
        else:
            assert st == U.ERR_UNSUPPORTED and U.sentinel(got), (F, st)


def test_dw_refusals():
    L = U._L()
    cs = dict(F=4, nmax=5, jt=2, bs=3, fam="E", bn=0, xdense=0, dout=0, acc=0, ldx=0, seed=1)
    d = U.dw_data(cs)
    st, got = U.call_dw(cs, d, readout=True)           # k_dw_readout without a readout gradient
    assert st == U.ERR_UNSUPPORTED and U.sentinel(got)
    st, got = U.call_dw(cs, d, lda=4)                  # lda below jt F
    assert st == U.ERR_ARG and U.sentinel(got)
    assert L.lib().hgnn_probe_dw_dense(None, U._stream()) == U.ERR_ARG


# ---------------------------------------------------------------------------------------------- switches
def test_switch_selected_variants():
    """The variants only a switch selects, each group in a fresh child process, one after another; the first child
    that fails -- a nonzero status, a signal or the time limit -- fails the test and no further child is started."""
    for name, (extra, mode) in U.SWITCH_GROUPS.items():
        # no switch of the parent's reaches the child; HGNN_LIB_PATH names the library under test, not a switch
        env = {k: v for k, v in os.environ.items() if not k.startswith("HGNN_") or k == "HGNN_LIB_PATH"}
        env.update(extra)
        cmd = [sys.executable, os.path.join(REPO, "tests", "dense_probe_worker.py"), mode]
        try:
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"{name}: the worker ran into its time limit: {str(e.stderr)[-2000:]}")
        assert r.returncode == 0, (name, r.returncode, r.stderr[-2000:])
