"""The inputs, case tables and checks of the dense-side kernel tests (tests/dense_probe_util.py) have the properties
those tests rely on -- checked on the CPU, so a mistake in a generator or a vacuous check cannot hide a kernel bug.

* The exact families are exact: evaluated in fp32 in the generator's row order, in a permuted order and as the naive
  sequential form, the sums equal the fp64 result, at the largest case of each table.
* The case tables hold every edge the GPU tests are meant to run (row counts, widths, options, switch groups), the
  path table lists all five launch sequences of the BN backward, and the dense-dW table instantiates every reachable
  k_dw_dense<FC, MAXI>, so a later edit of a table cannot silently drop one.
* The checks are not vacuous: the reference alone passes every check, and a reference perturbed by a dropped row, a
  dropped 64-row tile of the statistics, swapped statistics, m1 over cap_rows instead of total, a dropped last entry
  of a readout row's coefficient sum, R_b shifted by one column or a dW row n != 0 left at zero fails it.
* The random family's naive form stays inside its own bound.
"""

import numpy as np
import pytest

import dense_probe_util as U

F32, F64 = np.float32, np.float64


def _bn_case(fam="E", **kw):
    cs = dict(c=16, total=300, cap=448, fam=fam, training=1, apply=1, dbpart=1, acc=1, relu_from=8, ldy=0, misalign=0,
              seed=21)
    cs.update(kw)
    return cs


# ------------------------------------------------------------------------------------------------ exactness
@pytest.mark.parametrize("c", (1024, 257))
def test_bn_exact_family_is_exact_in_any_order(c):
    cs = _bn_case(c=c, total=1030, cap=1100, training=0, relu_from=c // 2)
    d = U.bn_data(cs)
    ref = U.bn_ref64(d, cs)
    for inv in (True, False):
        nv = U.bn_naive32(d, cs, inv)
        assert np.array_equal(nv["sums"].astype(F64), ref["sums"])
        assert np.array_equal(nv["dy"].astype(F64), ref["dy"]) and np.array_equal(nv["dbpart"].astype(F64), ref["dbpart"])
    perm = np.random.default_rng(1).permutation(cs["total"])
    dp = dict(d, y=d["y"][perm], dz=d["dz"][perm])
    assert np.array_equal(U.bn_naive32(dp, cs, True)["sums"].astype(F64), ref["sums"])
    y, dz, mu, sd = (d[k].astype(F64) for k in ("y", "dz", "mean", "std"))
    assert (np.abs(float(d["w"]) * dz * (y - mu) / sd).sum(0) * 4 < 2 ** 24).all()      # in quarter units
    assert abs(dz.mean()) > 0.5 and (d["y"] == 0).any() and np.signbit(d["y"][d["y"] == 0]).any()
    # per channel the fp32 statistics are exact, so dw / db are one rounding of the exact total
    assert np.array_equal(ref["sums"].astype(F32).astype(F64), ref["sums"])


def test_finalize_exact_family_has_exact_partials():
    cs = dict(c=5, tiles=600, last=32, fam="E", mode="part", run=1, seed=7)
    d = U.fin_data(cs)
    Yd = d["Y"].astype(F64)
    for t in (0, 17, 599):
        blk = Yd[t * 64:(t + 1) * 64]
        assert np.array_equal(d["part"][t, :, 1].astype(F64), blk.mean(0))
        assert np.array_equal(d["part"][t, :, 2].astype(F64), ((blk - blk.mean(0)) ** 2).sum(0))
    assert np.allclose(d["cmean"], d["mean"], rtol=0, atol=1e-14) and np.allclose(d["cstd"], d["std"], rtol=0, atol=1e-11)
    assert np.allclose(d["acc"][:, 0].sum(0) / d["rows"], d["mean"])


def test_readout_and_dw_exact_families_are_exact():
    d = U.ro_data(1300, 3, "E", 1)
    r64, r32 = U.ro_ref(d, F64), U.ro_ref(d, F32)
    for k in ("colsum", "out", "da"):
        assert np.array_equal(r32[k].astype(F64), r64[k]), k
    for C, jt in ((512, 7), (260, 5)):
        cs = dict(C=C, jt=jt, stride=8, fam="E", g=1, p=1, g_acc=1, p_acc=1, mis=0, lds=0, seed=2)
        da = U.agg_data(cs)
        for kind in ("g", "p"):
            assert np.array_equal(U.agg_ref(cs, da, kind, F32).astype(F64), U.agg_ref(cs, da, kind, F64))
    for cs in U.dw_cases():
        if cs["fam"] == "E" and cs["F"] == 130 and cs["bs"] < 256:
            dd = U.dw_data(cs)
            r = U.dw_ref(cs, dd, F64)
            assert np.array_equal(U.dw_ref(cs, dd, F32).astype(F64), r) and np.abs(r).max() < 2 ** 24


# ------------------------------------------------------------------------------------------------ tables
def test_bn_tables_hold_every_edge_and_all_five_paths():
    cases = U.bn_cases() + U.bn_scalar_forced_cases()
    assert {t for t, _ in U.BN_TOTALS} == {0, 1, 63, 64, 65, 255, 256, 257, 300, 1030}
    for total, cap in U.BN_TOTALS:
        assert cap // 64 > -(-total // 64) or (total % 64 and cap >= total), (total, cap)   # empty tiles behind
    assert any(t % 64 and -(-cap // 64) > -(-t // 64) for t, cap in U.BN_TOTALS)
    assert set(U.BN_WIDTHS) == {1, 3, 5, 255, 257, 4, 8, 16, 12, 20, 40, 100, 516, 1024, 64, 128, 256}
    for c in U.BN_WIDTHS:
        mine = [x for x in cases if x["c"] == c and not x["ldy"] and not x["misalign"]]
        assert {x["total"] for x in mine} == {t for t, _ in U.BN_TOTALS}
        for key, vals in (("training", {0, 1}), ("apply", {0, 1}), ("dbpart", {0, 1}), ("acc", {0, 1}),
                          ("fam", {"E", "R"}), ("relu_from", {0, c // 2, c})):
            assert {x[key] for x in mine} >= vals, (c, key)
    paths = lambda env: {U.bn_expected_path(x, env) for x in cases}
    assert paths(None) == {"narrow2s", "part4acc", "part4fin", "scalar"}
    assert paths(dict(HGNN_BN_BWD2="1")) == set(U.PATHS)
    assert "narrow2s" not in paths(dict(HGNN_BN_BWD2="0"))
    by = lambda c, env=None, **kw: U.bn_expected_path(_bn_case(c=c, **kw), env)
    assert [by(c) for c in U.SCALAR_C] == ["scalar"] * 5 and [by(c) for c in U.NARROW_C] == ["narrow2s"] * 3
    assert [by(c) for c in U.PART4_C + U.WIDE_C] == ["part4acc"] * 9
    assert [by(c, dict(HGNN_BN_BWD2="1")) for c in U.WIDE_C] == ["wide2"] * 3
    assert by(8, dict(HGNN_BN_BWD2="0"), acc=0) == "part4fin" and by(8, apply=0) == "part4fin"
    assert by(8, ldy=12) == "scalar" and by(8, misalign=1) == "scalar"
    assert by(4, cap=U.FALLBACK_CAP) == "part4acc" and by(4, cap=U.FALLBACK_CAP - 1) == "narrow2s"
    many = U.bn_many_tiles_cases()
    assert all(-(-x["total"] // 64) > 64 for x in many) and {U.bn_expected_path(x) for x in many} == {"part4fin", "scalar"}
    for x in many:
        d = U.bn_data(x)
        assert np.array_equal(U.bn_naive32(d, x, True)["sums"].astype(F64), U.bn_ref64(d, x)["sums"])
    forced = U.bn_scalar_forced_cases()
    assert {(x["ldy"] > 0, x["misalign"]) for x in forced} == {(True, 0), (False, 1)}
    assert all(x["c"] % 4 == 0 and U.bn_expected_path(x) == "scalar" for x in forced)


def test_finalize_readout_tables_hold_every_edge():
    assert U.FIN_TILES == (1, 2, 63, 64, 65, 511, 512, 513, 600) and U.FIN_C == (1, 3, 4, 5)
    fc = U.fin_cases()
    assert {x["mode"] for x in fc} == {"part", "acc"} and {x["run"] for x in fc} == {0, 1}
    assert any(x["last"] < 64 for x in fc)
    assert U.RO_NB == (0, 1, 7, 8, 9, 17) and U.RO_K == (1, 63, 64, 65, 1024, 1025, 1300)
    assert U.RO_DIM_OUT == (1, 3) and U.RO_BS == (1, 15, 16, 17, 33)
    assert U.AGG_C == (5, 64, 260, 512) and U.AGG_COUNTS == (0, 3, 4, 5, 9) and U.AGG_EDGE_ROWS > 256
    for C in U.AGG_C:
        ac = U.agg_cases(C)
        assert {x["jt"] for x in ac} == {2, 3, 4, 5, 7} and {x["stride"] for x in ac} == {4, 8}
        assert {(x["g"], x["p"]) for x in ac} == {(1, 1), (1, 0), (0, 1), (0, 0)}
        assert {x["g_acc"] for x in ac} == {0, 1} == {x["p_acc"] for x in ac} and any(x["mis"] for x in ac)
    lds = {x["lds"]: U.agg_lds_bytes(x, U.agg_data(x)) for x in U.agg_cases(512)}
    assert lds[0] <= 64 * 1024 < lds[1] <= 160 * 1024 < lds[2]


def test_dw_table_instantiates_every_reachable_kernel():
    cases = U.dw_cases()
    assert {c["F"] for c in cases} == set(U.DW_F) | {20} and {c["nmax"] for c in cases} >= set(U.DW_NMAX)
    assert {c["jt"] for c in cases} >= set(U.DW_JT) and {c["bs"] for c in cases} >= {1, 3, 260}
    assert any(c["bs"] == 260 and c["nmax"] == 5 and c["F"] == 4 for c in cases)
    for key in ("bn", "xdense", "dout", "acc"):
        assert {c[key] for c in cases} == {0, 1}, key
    assert {c["ldx"] for c in cases} == {0, 3, 4}
    kern = {U.dw_kernel(c)[:3] for c in cases}
    want = {("narrow",)} | {("dense", fc, 1) for fc in (128, 64, 32, 16)} | \
           {("dense", 128, 3), ("dense", 64, 3), ("dense", 32, 3), ("dense", 32, 5), ("dense", 16, 5)}
    assert kern == want, kern ^ want
    off = {U.dw_kernel(c, dict(HGNN_DW_NARROW="0"))[:3] for c in cases}
    assert ("narrow",) not in off
    assert any(U.dw_kernel(c)[-1] > 1 for c in cases if c["bs"] < 256 and len(U.dw_kernel(c)) == 4)   # gridDim.y
    assert any(U.dw_kernel(c)[1:3] == (16, 5) and (-(-c["nmax"] // 32)) ** 2 * c["jt"] > 20 for c in cases)
    for c in cases:      # N_b of 0, 1 and nmax in one batch wherever the batch has three graphs
        if c["bs"] >= 3:
            nb = np.diff(U.dw_data(c)["off"])
            assert {0, 1, c["nmax"]} <= set(nb.tolist())
    assert set(U.SWITCH_GROUPS) == {"bn_bwd2=0", "bn_bwd2=1", "bn_acc=0", "dw_narrow=0", "dwd_grid=0", "dwd_grid=3"}


# ------------------------------------------------------------------------------------------------ the checks bite
@pytest.mark.parametrize("fam,c", [("E", 16), ("R", 16), ("E", 5), ("R", 100)])
def test_bn_check_passes_the_reference_and_fails_perturbed_ones(fam, c):
    cs = _bn_case(fam, c=c, relu_from=c // 2)
    d = U.bn_data(cs)
    U.check_bn_bwd(cs, d, U.bn_got_from_ref(cs, d))
    stats = dict(cs, apply=0)
    U.check_bn_bwd(stats, d, U.bn_got_from_ref(stats, d))

    def fails(case, got):
        with pytest.raises(AssertionError):
            U.check_bn_bwd(case, d, got)
    short = dict(d, y=d["y"][:-1], dz=d["dz"][:-1])                 # a dropped row
    g = U.bn_got_from_ref(stats, d)
    g["sums"] = U.bn_ref64(short, dict(stats, total=cs["total"] - 1))["sums"].astype(F32)
    fails(stats, g)
    keep = np.r_[0:64, 128:cs["total"]]                              # a dropped 64-row tile of the statistics
    g = U.bn_got_from_ref(stats, d)
    g["sums"] = U.bn_ref64(dict(d, y=d["y"][keep], dz=d["dz"][keep]), dict(stats, total=len(keep)))["sums"].astype(F32)
    fails(stats, g)
    for a, b in ((0, 1), (2, 3)):                                    # swapped statistics
        g = U.bn_got_from_ref(stats, d)
        g["sums"][:, [a, b]] = g["sums"][:, [b, a]]
        fails(stats, g)
    g = U.bn_got_from_ref(cs, d)                                     # m1 / m2 over cap_rows instead of total
    g["dy"][:cs["total"]] = U.bn_ref64(d, cs, n_for_mean=cs["cap"])["dy"]
    fails(cs, g)
    g = U.bn_got_from_ref(cs, d)                                     # a row of dy not written
    g["dy"][17] = U.SENT
    fails(cs, g)
    g = U.bn_got_from_ref(cs, d)                                     # dbpart written one tile late
    g["dbpart"][1:6] = g["dbpart"][0:5].copy()
    fails(cs, g)
    g = U.bn_got_from_ref(cs, d)
    g["dw"], g["db"] = g["db"], g["dw"]
    fails(cs, g)
    less = U.bn_ref64(short, dict(cs, total=cs["total"] - 1))     # dw / db of one row less (the integer family's
    full = U.bn_ref64(d, cs)                                         # last row may sum to zero over the channels)
    assert less["dw"] != full["dw"] or less["db"] != full["db"]
    for k in ("dw", "db"):
        if less[k] != full[k]:
            g = U.bn_got_from_ref(cs, d)
            g[k] = F32(less[k])
            fails(cs, g)
    g = U.bn_got_from_ref(cs, d)
    g["acc_zero"][3] = 1.0
    fails(cs, g)
    g = U.bn_got_from_ref(cs, d)
    g["path"] = "part4fin"
    fails(cs, g)


def test_bn_naive_form_stays_inside_its_own_bound():
    for c in (16, 5):
        cs = _bn_case("R", c=c, relu_from=c // 2)
        d = U.bn_data(cs)
        got = U.bn_got_from_ref(cs, d)
        nv = U.bn_naive32(d, cs, inv=c % 4 == 0)
        got["dy"][:cs["total"]], got["dbpart"][:5] = nv["dy"], nv["dbpart"]
        U.check_bn_bwd(cs, d, got)
        stats = dict(cs, apply=0)
        got = U.bn_got_from_ref(stats, d)
        got["sums"] = nv["sums"]
        U.check_bn_bwd(stats, d, got)


def test_finalize_check_bites():
    cs = dict(c=4, tiles=65, last=37, fam="R", mode="part", run=1, seed=3)
    d = U.fin_data(cs)
    ok = lambda: dict(mean=d["cmean"].astype(F32), std=d["cstd"].astype(F32),
                      run_mean=U.running_update(d["cmean"].astype(F32), d["run_mean"]),
                      run_std=U.running_update(d["cstd"].astype(F32), d["run_std"]))
    U.check_fin("ref", d, ok(), "part", False)
    drop = U.fin_from_y(d["Y"][:-64], np.random.default_rng(0))      # a dropped tile
    for k in ("mean", "std"):
        g = ok()
        g[k] = drop[k].astype(F32)
        with pytest.raises(AssertionError):
            U.check_fin("dropped tile", d, g, "part", False)
    g = ok()
    g["run_mean"] = np.nextafter(g["run_mean"], F32(9))
    with pytest.raises(AssertionError):
        U.check_fin("running", d, g, "part", False)
    g = ok()
    g["std"][2] = 0.0
    with pytest.raises(AssertionError):
        U.check_fin("negative variance", d, g, "part", False)


@pytest.mark.parametrize("fam", ("E", "R"))
def test_readout_checks_bite(fam):
    d = U.ro_data(65, 3, fam, 5)
    r = U.ro_ref(d, F64)
    got = dict(colsum=r["colsum"].astype(F32), out=r["out"].astype(F32))
    U.check_ro_fwd("ref", d, got)
    short = dict(d, A=d["A"].copy())
    short["A"][int(d["off"][-1]) - 1] = 0                            # the 17-node graph's tail row dropped
    bad = U.ro_ref(short, F64)
    for k in ("colsum", "out"):
        with pytest.raises(AssertionError):
            U.check_ro_fwd("dropped row", d, dict(got, **{k: bad[k].astype(F32)}))
    da = np.full((int(d["off"][-1]) + 9, 65), U.SENT, F32)
    da[:int(d["off"][-1])] = r["da"]
    U.check_ro_da("ref", d, da)
    bad = da.copy()
    bad[:int(d["off"][-1])] = np.roll(r["da"], 1, axis=1)            # R_b shifted by one column
    with pytest.raises(AssertionError):
        U.check_ro_da("shift", d, bad)
    bad = da.copy()
    bad[int(d["off"][-1])] = 0.0
    with pytest.raises(AssertionError):
        U.check_ro_da("row past the total", d, bad)
    p = U.ro_param_data(17, 65, 3, fam, 6)
    dfcw = np.full((4, 65), U.SENT, F32)
    dfcb = np.full(4, U.SENT, F32)
    dfcw[:3] = p["dout"].astype(F64).T @ p["colsum"].astype(F64)
    dfcb[:3] = p["nmax"] * p["dout"].astype(F64).sum(0)
    U.check_ro_params("ref", p, dict(dfcw=dfcw, dfcb=dfcb))
    bad = dfcw.copy()
    bad[:3] = p["dout"][:16].astype(F64).T @ p["colsum"][:16].astype(F64)   # the 17th graph (a second chunk) dropped
    with pytest.raises(AssertionError):
        U.check_ro_params("dropped graph", p, dict(dfcw=bad, dfcb=dfcb))


@pytest.mark.parametrize("fam", ("E", "R"))
def test_agg_check_bites(fam):
    cs = dict(C=64, jt=5, stride=8, fam=fam, g=1, p=1, g_acc=1, p_acc=0, mis=0, lds=0, seed=9)
    d = U.agg_data(cs)

    def padded(x):
        out = np.full((len(x) + 3, x.shape[1]), U.SENT, F32)
        out[:len(x)] = x
        return out
    gg, gp = padded(U.agg_ref(cs, d, "g", F64)), padded(U.agg_ref(cs, d, "p", F64))
    U.check_agg("ref", cs, d, gg, gp)
    if fam == "R":
        U.check_agg("naive", cs, d, padded(U.agg_ref(cs, d, "g", F32)), padded(U.agg_ref(cs, d, "p", F32)))
    for kw in (dict(drop_last=True), dict(shift=1)):                 # a 9-entry row cut to 8; R_b shifted
        with pytest.raises(AssertionError):
            U.check_agg("bad g", cs, d, padded(U.agg_ref(cs, d, "g", F64, **kw)), gp)
        with pytest.raises(AssertionError):
            U.check_agg("bad p", cs, d, gg, padded(U.agg_ref(cs, d, "p", F64, **kw)))
    no3 = dict(d, gl=dict(d["gl"], vals=[np.concatenate([v[:, :3], 0 * v[:, 3:]], 1) for v in d["gl"]["vals"]]))
    with pytest.raises(AssertionError):                              # the j >= 3 coefficients dropped
        U.check_agg("no j >= 3", cs, d, padded(U.agg_ref(cs, no3, "g", F64)), gp)


@pytest.mark.parametrize("fam,dout", [("E", 1), ("R", 1), ("E", 0), ("R", 0)])
def test_dw_check_bites(fam, dout):
    cs = dict(F=17, nmax=33, jt=3, bs=3, fam=fam, bn=1, xdense=0, dout=dout, acc=1, ldx=0, seed=12)
    d = U.dw_data(cs)

    def padded(x):
        out = np.full((cs["bs"] + 1,) + x.shape[1:], U.SENT, F32)
        out[:cs["bs"]] = x
        return out
    U.check_dw("ref", cs, d, padded(U.dw_ref(cs, d, F64)))
    if fam == "R":
        U.check_dw("naive", cs, d, padded(U.dw_ref(cs, d, F32)))
    with pytest.raises(AssertionError):
        U.check_dw("rows n != 0 zero", cs, d, padded(U.dw_ref(cs, d, F64, zero_rows=True)))
    if dout:
        with pytest.raises(AssertionError):
            U.check_dw("shift", cs, d, padded(U.dw_ref(cs, d, F64, shift=1)))
    nobn = dict(cs, bn=0)                                            # padded m left at 0 instead of the BN of 0
    with pytest.raises(AssertionError):
        U.check_dw("no BN of zero", cs, d, padded(U.dw_ref(nobn, dict(d, xp=_bn_applied(d)), F64)))
    bad = padded(U.dw_ref(cs, d, F64))
    bad[cs["bs"], 0, 0, 0] = 0.0
    with pytest.raises(AssertionError):
        U.check_dw("graph outside the launch", cs, d, bad)


def _bn_applied(d):
    bn = d["bn"]
    return ((d["xp"].astype(F64) - bn["mean"]) * (float(bn["w"]) / bn["std"].astype(F64)) + float(bn["b"])).astype(F32)
