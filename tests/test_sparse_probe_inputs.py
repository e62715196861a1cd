"""The inputs, case tables and checks of the sparse-side kernel tests (tests/sparse_probe_util.py) have the properties
those tests rely on -- checked on the CPU, so a mistake in a generator or a vacuous check cannot hide a kernel bug.

* The exact families are exact: the naive fp32 reference equals the fp64 one and sum |v||x| stays below 2^24 at the
  longest row each family is used with (BN on load included).
* The case tables hold every entry count, row count, width, J_tot, j0, pad_from, BN combination, extraction shape
  and switch group the GPU tests are meant to run, so a later edit of a table cannot silently drop one.
* The checks are not vacuous: the fp64 reference of a perturbed list (the last entry of a row dropped, Pm and Pd
  swapped, the slices shifted by one, the second chunk's first entry dropped) fails the check of its family.
* The numpy list builder agrees with tests/test_builder.py's emulation of k_extract on a dense batch.
"""

import copy

import numpy as np
import pytest

import sparse_probe_util as U


def _abs_bound_fwd(d):
    """max over rows and parts of sum_e |v| |z|."""
    m = 0.0
    for l, x, bn, ncs in ((d["g"], d["xg"], d["gbn"], None), (d["p"], d["xp"], d["pbn"], None)):
        if l is None:
            continue
        z = np.abs(U.bn_z(x, bn, np.float64))
        la = dict(l, vals=np.abs(l["vals"]))
        for j in range(l["nc"]):
            m = max(m, float(U.gather_sum(la, j, z, np.float64).max(initial=0.0)))
    return m


LONGEST = [dict(cg=64, cp=64, jtot=7, total=37, cap=48, fam="A1", bn=3, pad=0, j0=0, ldo=0, seed=1),
           dict(cg=64, cp=64, jtot=3, total=37, cap=48, fam="A1", bn=0, pad=0, j0=0, ldo=0, seed=2),
           dict(cg=64, cp=64, jtot=4, total=37, cap=48, fam="A3", bn=3, pad=0, j0=0, ldo=0, seed=3),
           dict(cg=64, cp=64, jtot=3, total=37, cap=48, fam="A3", bn=0, pad=0, j0=0, ldo=0, seed=4),
           dict(cg=64, cp=64, jtot=4, total=100, cap=112, fam="A1", bn=1, pad=0, j0=2, ldo=0, seed=5)]


@pytest.mark.parametrize("c", LONGEST, ids=U.case_id)
def test_exact_forward_families_are_exact(c):
    d = U.fwd_data(c)
    longest = max(int(l["cnt"].max()) for l in (d["g"], d["p"]))
    assert longest == (32 if c["fam"] == "A3" else (130 if c["j0"] == 0 else 130))
    r64, r32 = U.ref_fwd(d, np.float64), U.ref_fwd(d, np.float32)
    assert np.array_equal(r32.astype(np.float64), r64) and np.isfinite(r64).all()
    assert _abs_bound_fwd(d) < 2 ** 24
    for bn, x in ((d["gbn"], d["xg"]), (d["pbn"], d["xp"])):
        if bn is not None:   # z is an exact integer and the kernel's scale w / std is exact
            z = U.bn_z(x, bn, np.float64)
            assert np.array_equal(z, np.round(z)) and np.array_equal(U.bn_z(x, bn, np.float32).astype(np.float64), z)
            s = (bn["w"] / bn["std"]).astype(np.float32)
            assert np.array_equal(s.astype(np.float64), np.float64(bn["w"]) / bn["std"].astype(np.float64))
            assert np.array_equal(((x - bn["mean"]) * s + bn["b"]).astype(np.float64), z)


@pytest.mark.parametrize("kind,fam,jt", [("g", "A1", 7), ("p", "A1", 3), ("g", "A3", 4), ("p", "A3", 3)])
def test_exact_backward_families_are_exact(kind, fam, jt):
    c = dict(kind=kind, c=64, jtot=jt, gofs=4, total=37, cap=48, acc=1, fam=fam, odd=0, seed=11)
    d = U.bwd_data(c)
    r64, r32 = U.ref_bwd(d, np.float64), U.ref_bwd(d, np.float32)
    assert np.array_equal(r32.astype(np.float64), r64) and np.isfinite(r64).all()
    da = dict(d, src=np.abs(np.nan_to_num(d["src"])), out0=np.abs(d["out0"]), list=dict(d["list"], vals=np.abs(d["list"]["vals"])))
    assert U.ref_bwd(da, np.float64).max() < 2 ** 24
    # the poison lies outside everything the formulas read
    assert np.isnan(d["src"][:, :d["live"][0][0]]).all() and np.isnan(d["src"][(U.SRC_G if kind == "g" else U.SRC_P)[0]:]).all()


def test_a3_rows_stay_short():
    for c in U.fwd_cases() + U.diag_cases():
        if c["fam"] == "A3":
            d = U.fwd_data(c)
            assert max(int(l["cnt"].max()) for l in (d["g"], d["p"]) if l is not None) <= 32, c
    for c in U.bwd_cases():
        if c["fam"] == "A3":
            assert int(U.bwd_data(c)["list"]["cnt"].max()) <= 32, c


def test_case_tables_cover_the_listed_edges():
    assert set(U.COUNTS) == {0, 1, 3, 4, 5, 8, 9, 63, 64, 65, 130}
    pc = U.pair_counts(37)
    assert {a for a, _ in pc} >= set(U.COUNTS) and {b for _, b in pc} >= set(U.COUNTS)
    assert all(a != b for a, b in pc[:11]) and {(65, 3), (3, 65), (9, 8), (8, 9)} <= set(pc)
    assert any(a == 0 and b > 0 for a, b in pc) and any(b == 0 and a > 0 for a, b in pc)
    for t in (15, 16, 17):
        assert {a for a, _ in U.pair_counts(t)} >= set(U.COUNTS)
    f = U.fwd_cases()
    assert {(c["total"], c["cap"]) for c in f} == {(0, 48), (1, 48), (15, 48), (16, 48), (17, 48), (37, 48), (48, 48)}
    assert {(c["cg"], c["cp"]) for c in f} == {(5, 1), (64, 64), (100, 100), (128, 128), (256, 256), (512, 64), (130, 0),
                                               (0, 64)}
    assert {c["jtot"] for c in f} == {3, 4, 7} and {c["pad"] for c in f} == {0, -1, "explicit"}
    assert {c["fam"] for c in f} == {"A1", "A3", "AR"}
    for (cg, cp) in U.FWD_WIDTHS:   # each width in an exact and in the random family
        assert {c["fam"] for c in f if (c["cg"], c["cp"]) == (cg, cp)} >= {"A1", "AR"}
    for jt in (3, 4):               # G on/off x P on/off, on the rows-per-wave kernel (J_tot 3) and on k_agg_fwd
        assert {c["bn"] for c in f if c["jtot"] == jt and c["cg"] and c["cp"]} == {0, 1, 2, 3}
        assert {c["pad"] for c in f if c["jtot"] == jt} == {0, -1, "explicit"}
    dg = U.diag_cases()
    assert {c["cg"] for c in dg} == {64, 128, 256} and all(c["j0"] == 2 and c["cp"] in (0, c["cg"]) for c in dg)
    assert {c["cp"] == 0 for c in dg} == {True, False} and {c["jtot"] for c in dg} == {3, 4, 7}
    assert {c["j0"] for c in f} == {0} and {c["fam"] for c in dg} == {"A1", "A3", "AR"}
    d = U.fwd_data(next(c for c in dg if c["fam"] != "A3"))
    assert d["g"]["cnt"][80] == 70 and d["diag_rows"][80] == 65 and d["g"]["cols"][80, 65] == 80
    assert any(v is None for v in d["diag_rows"].values())
    b = U.bwd_cases()
    assert {c["c"] for c in b} == {5, 64, 100, 128, 256, 512} and {c["jtot"] for c in b} == {3, 4, 7}
    assert {c["gofs"] for c in b if c["kind"] == "g"} == {0, 4}
    assert {(c["kind"], c["acc"]) for c in b} == {("g", 0), ("g", 1), ("p", 0), ("p", 1)}
    assert {(c["total"], c["cap"]) for c in b} == set(U.ROWS)
    for c in (5, 64, 100, 128, 256, 512):
        assert {(x["kind"], x["acc"], x["fam"]) for x in b if x["c"] == c} >= {(k, a, fam) for k in "gp" for a in (0, 1)
                                                                              for fam in ("A1", "AR")}
    assert {(p["cg"], p["cp"], p["odd"]) for p in U.PAIR_CASES} >= {(64, 64, 0), (64, 128, 0), (128, 128, 1)}
    s = U.EXTRACT_SHAPES
    assert [x["variant"] for x in s] == [2, 2, 1, 1, 0]
    assert [(x["dual"], x["jtot"], x["nmax"], x["emax"]) for x in s] == [(1, 3, 9, 25), (1, 4, 32, 64), (1, 5, 6, 8),
                                                                         (0, 3, 70, 0), (1, 3, 12, 130)]
    for x in s:
        assert {0, 1, x["nmax"]} <= set(x["Nb"]) and len(set(x["Nb"])) == 5
        assert not x["dual"] or ({0, 1, x["emax"]} <= set(x["Eb"]) and len(set(x["Eb"])) == 5)
    assert 4 * 130 * 130 * 3 > 96 * 1024
    assert set(U.INVALID) == {"w_pad_row", "w_pad_col", "wl_pad", "pm_pad", "pd_pad", "mask", "sizes"}
    assert {tuple(sorted(env.items())): (mode, var) for env, mode, var in U.SWITCH_GROUPS.values()} == {
        (("HGNN_AGG_RPW", "1"),): ("agg_fwd", None),
        (("HGNN_AGG_RPW", "4"),): ("agg_fwd", None),
        (("HGNN_EXTRACT_REG", "0"),): ("extract", (1, 1, 1, 1, 0)),
        (("HGNN_EXTRACT_LDS", "0"),): ("extract", (0, 0, 0, 0, 0)),
        (("HGNN_EXTRACT_LDS", "0"), ("HGNN_EXTRACT_SPLIT", "1")): ("extract", (0, 0, 0, 0, 0)),
    }


# ---------------------------------------------------------------------------------------------- perturbations
def _perturb(d, how):
    """A copy of forward data d whose lists a subtly wrong kernel would effectively have walked."""
    p = copy.deepcopy(d)
    g, pl = p["g"], p["p"]
    long_g = int(np.argmax(g["cnt"]))
    if how == "drop_last":
        g["cnt"][long_g] -= 1
    elif how == "swap_pm_pd":
        pl["vals"] = pl["vals"][:, :, ::-1].copy()
    elif how == "slice_shift":
        g["vals"] = np.roll(g["vals"], 1, axis=2)
    elif how == "drop_chunk2_first":
        assert g["cnt"][long_g] > 64
        k = int(g["cnt"][long_g])
        g["cols"][long_g, 64:k - 1], g["vals"][long_g, 64:k - 1] = g["cols"][long_g, 65:k].copy(), g["vals"][long_g, 65:k].copy()
        g["cnt"][long_g] -= 1
    return p


@pytest.mark.parametrize("how", ["drop_last", "swap_pm_pd", "slice_shift", "drop_chunk2_first"])
@pytest.mark.parametrize("fam", ["A1", "AR"])
def test_checks_are_not_vacuous_forward(fam, how):
    c = dict(cg=64, cp=64, jtot=3, total=37, cap=48, fam=fam, bn=0, pad=0, j0=0, ldo=0, seed=21)
    d = U.fwd_data(c)
    r64, r32 = U.ref_fwd(d, np.float64), U.ref_fwd(d, np.float32)
    U.check_values("unperturbed", fam, r32, r64, r32)
    wrong = U.ref_fwd(_perturb(d, how), np.float64).astype(np.float32)
    with pytest.raises(AssertionError):
        U.check_values(how, fam, wrong, r64, r32)


@pytest.mark.parametrize("how", ["drop_last", "swap_pm_pd", "slice_shift", "drop_chunk2_first"])
@pytest.mark.parametrize("fam", ["A1", "AR"])
def test_checks_are_not_vacuous_backward(fam, how):
    kind = "p" if how == "swap_pm_pd" else "g"
    c = dict(kind=kind, c=64, jtot=3, gofs=4, total=37, cap=48, acc=1, fam=fam, odd=0, seed=22)
    d = U.bwd_data(c)
    r64, r32 = U.ref_bwd(d, np.float64), U.ref_bwd(d, np.float32)
    U.check_values("unperturbed", fam, r32, r64, r32)
    p = copy.deepcopy(d)
    fake = dict(g=p["list"], p=p["list"])
    p["list"] = _perturb(fake, how)["p" if kind == "p" else "g"]
    wrong = U.ref_bwd(p, np.float64).astype(np.float32)
    with pytest.raises(AssertionError):
        U.check_values(how, fam, wrong, r64, r32)


def test_list_checks_are_not_vacuous():
    """check_lists fails on a dropped last entry, a wrong count and a write outside the lists."""
    b = U.extract_batch(U.EXTRACT_SHAPES[0])
    want = U.dense_lists(b)
    rows, ents = [w["rows"].copy() for w in want], [w["ent"].copy() for w in want]
    U.check_lists("same", rows, ents, want)
    r = int(np.argmax(want[4]["rows"][:want[4]["total"], 1]))
    s, k = want[4]["rows"][r]
    for what in ("count", "pm_pd", "last", "stray"):
        rr, ee = [x.copy() for x in rows], [x.copy() for x in ents]
        if what == "count":
            rr[4][r, 1] -= 1
        elif what == "pm_pd":
            ee[4][s:s + k, 1:3] = ee[4][s:s + k, 2:0:-1]
        elif what == "last":
            ee[4][s + k - 1] = U.SENT
        else:
            ee[4][s + k, 0] = 0.0
        with pytest.raises(AssertionError):
            U.check_lists(what, rr, ee, want)


# ---------------------------------------------------------------------------------------------- list builder
def test_dense_list_builder_matches_the_documented_format():
    from test_builder import _extract
    for s in U.EXTRACT_SHAPES:
        b = U.extract_batch(s)
        lists = U.dense_lists(b)
        nb, eb = U.clamp_counts(b)
        assert len(lists) == (6 if s["dual"] else 2)
        n0 = 0
        for g in range(b["bs"]):
            n = int(nb[g])
            for k, blk in ((0, b["W"][g, :n, :n]), (1, b["W"][g, :n, :n].transpose(1, 0, 2))):
                l = lists[k]
                for r, items in enumerate(_extract(blk, s["jtot"])):
                    start, count = l["rows"][n0 + r]
                    assert start == g * s["nmax"] ** 2 + r * s["nmax"] and count == len(items)
                    cols = l["ent"][start:start + count, 0].view(np.int32)
                    assert cols.tolist() == [n0 + c for c, _ in items] and (np.diff(cols) > 0).all()
                    for e, (_, v) in enumerate(items):
                        assert np.array_equal(l["ent"][start + e, 1:1 + s["jtot"]], v)
            n0 += n
        # -0.0 counts as zero: some all-zero elements carry a sign bit and are not listed
        W = b["W"]
        assert (np.signbit(W) & (W == 0)).any()
        assert lists[0]["used"].sum() == sum(int(((W[g, :nb[g], :nb[g]] != 0).any(-1)).sum()) for g in range(b["bs"]))
    # the complete graph gives the two-chunk rows
    assert U.dense_lists(U.extract_batch(U.EXTRACT_SHAPES[3]))[0]["rows"][:, 1].max() == 70
    assert U.dense_lists(U.extract_batch(U.EXTRACT_SHAPES[4]))[2]["rows"][:, 1].max() == 130


def test_direct_list_poisons_what_is_not_read():
    g = np.random.default_rng(0)
    l = U.direct_list(g, "AR", [0, 3, 65], 8, 150, 3, 4)
    used = np.zeros(len(l["ent"]), bool)
    for r in range(3):
        s, k = l["rows"][r]
        used[s:s + k] = True
        assert (np.diff(l["cols"][r, :k]) > 0).all()
    assert np.isfinite(l["ent"][used]).all()
    assert np.isnan(l["ent"][~used, 1:]).all() and (l["ent"][~used, 0].view(np.int32) == 0).all()
    for r in range(3, 8):
        s, k = l["rows"][r]
        assert not used[s:s + k].any()
