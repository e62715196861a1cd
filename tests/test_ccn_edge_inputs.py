"""CPU checks of the inputs of tests/test_gpu_ccn_edges.py (tests/ccn_edge_util.py): the boundary graphs have the
degrees their table claims, the dispatch mirror selects every untested instantiation the cases are there for, family
M keeps its pre-activations 100 x above the fp32 noise, family S is exact at level 1 and fixed at the levels above,
the numpy plan restatement equals the oracle's literal one, and dropping any contraction block from the oracle is
seen by the criteria."""

import numpy as np
import pytest
import torch

import ccn_edge_util as U
from oracle import ref_ccn as RC


def test_boundary_graph_degrees():
    for g, (dmax, dmin, above) in U.DEGREES.items():
        a = U.GRAPHS[g]()
        d = U.degrees(a)
        assert torch.equal(a, a.T) and bool((a.diagonal() == 1).all()), g
        assert (int(d.max()), int(d.min()), int((d > 64).sum())) == (dmax, dmin, above), (g, d.max(), d.min())
    d = U.degrees(U.lolli(64, 2))
    assert sorted(d.tolist()) == [2, 3] + [64] * 63 + [65]
    assert sorted(U.degrees(U.star(130)).tolist()) == [2] * 129 + [130]


def test_tiny_batch():
    adjs = U.tiny()
    assert [0 if a is None else a.shape[0] for a in adjs] == [1, 4, 6, 7, 5, 0]
    for a in adjs[:-1]:
        n = a.shape[0]
        assert torch.equal(a, a.T) and bool((a.diagonal() == 1).all())
        chords = (int(a.sum().item()) - n - 2 * (n - 1)) // 2
        assert chords == min(2, (n - 1) * (n - 2) // 2), (n, chords)


def test_ro_chunks_rule():
    """ccn_readout.hip ro_chunks: rows per graph / 4096 + 1, capped at 32 -- the second chunk starts at 4096 rows"""
    assert [U.ro_chunks(r, 1) for r in (0, 4095, 4096, 4225, 8192, 10 ** 9)] == [1, 1, 2, 2, 3, 32]
    assert U.ro_chunks(3 * 4225, 3) == 2 and U.ro_chunks(4225, 2) == 1
    by = {c["graphs"][0]: U.case_mirror(c["name"]) for c in U.CASES_S if c["order"] == 1}
    assert "readout1[nch=2]" in by["clique(65)"] and "readout1[nch=2]" in by["clique(64)"]
    assert "readout1[nch=1]" in by["star(1024)"]  # 3070 rows


def test_mirror_selections():
    """The instantiations named case by case, for the shapes the issue lists."""
    m = U.mirror
    d63, d65 = [U.degrees(U.lolli(63, 1))], [U.degrees(U.lolli(64, 2))]
    # B1: max degree 64 -> no large-degree kernel under either plan (nmax = 64)
    for plan in ("async", "sync"):
        s = m(2, 5, 2, 2, d63, 1, 64, plan)
        assert "top_direct" in s and not any("big" in k for k in s), s
    # B2: one node of degree 65 -> both plans run the large-degree kernels and the broadcast top level
    for plan in ("async", "sync"):
        s = m(2, 9, 3, 2, d65, 1, 66, plan)
        assert {"k_ccn_bcast", "k_ccn2_fwd_big<16,16>", "k_c2_fwd<16,2,1,true>", "k_c2_fwd<8,2,4,false>",
                "k_c2_gather<8,1>", "k_c2_gather_big<8,1>", "k_ccn2_dx0[cin>8]"} <= s, s
    # nmax = 65 without a degree above 64: the async plan's bounds differ from the sync plan's totals
    d = [U.degrees(U.lolli(63, 2))]
    a, s = m(2, 5, 2, 2, d, 1, 65, "async"), m(2, 5, 2, 2, d, 1, 65, "sync")
    assert "c2[big kernels over zero nodes]" in a and "k_ccn_bcast" in a and "top_direct" in s
    assert U.auto_plan(2, 1, 64) == "async" and U.auto_plan(2, 1, 66) == "async" and U.auto_plan(2, 1, 130) == "sync"
    assert U.auto_plan(2, 7, 66) == "sync" and U.auto_plan(1, 1, 129) == "async" and U.auto_plan(1, 1, 1024) == "sync"
    # wide levels: the backward's instantiation differs from the forward's (ccn_general.h c2_select)
    s = m(2, 8, 16, 2, [np.array([3, 3, 3])], 1, 3, "async")
    assert {"k_c2_fwd<16,2,2,false>", "k_c2_bwd<16,1,2,false>", "k_c2_gather<16,1>", "readout[h passes>1]"} <= s
    # CCN-1D: 9 channels at degree <= 64 enter the chunked branch without a second chunk
    s = m(1, 9, 2, 2, [np.array([2, 3, 2])], 1, 3, "async")
    assert {"k_ccn1_fwd[chunked,n<=64,cin>8]", "k_ccn1_fwd[fast]", "k_ccn1_bwd_gather[chunked,n<=64,cin>8]"} <= s
    s = m(1, 2, 9, 3, [np.array([2, 3, 2])], 1, 3, "async")
    assert {"k_ccn1_bwd_node[chunked,n<=64]", "k_ccn1_fwd[fast]", "readout1[h passes>1]"} <= s


def test_coverage_set():
    """Items 1-9 of the gap list are each selected by at least one case."""
    have = U.covered()
    hit = {item for item, names in U.COVERAGE.items() if names <= have}
    assert hit == set(range(1, 10)), {i: sorted(n - have) for i, n in U.COVERAGE.items() if not n <= have}


@pytest.mark.parametrize("name", [c["name"] for c in U.CASES_A])
def test_family_m_margin(name):
    l64, l32 = U.legs(name)
    margin, same = U.margin_m(l64, l32)
    print(f"{name}: margin {margin:.0f}x, {sum(t.numel() for t in l64['taps'])} pre-activations")
    assert same and margin >= U.MARGIN_M, (name, margin, same)


@pytest.mark.parametrize("name", [c["name"] for c in U.CASES_S])
def test_family_s_exact_and_fixed(name):
    c = U.BY_NAME[name]
    adjs, xs, p, w = U.inputs(name)
    m, f, h = (18 if c["order"] == 2 else 2), c["f"], c["h"]
    w1 = p["w1.weight"]
    assert set(w1.unique().tolist()) <= {-1.0, 0.0, 1.0} and set(p["w1.bias"].abs().tolist()) == {0.5}
    assert all(bool(w1[:, q * f:(q + 1) * f].any()) for q in range(m))
    assert all(bool((x == x.round()).all()) and x.abs().max() <= 2 for x in xs if x.numel())
    bound = U.s_bound(name)
    print(f"{name}: largest level-1 intermediate {bound:.3g}")
    assert bound < 2 ** 23
    leg = {dt: U._leg(c, adjs, xs, p, w, dt, False) for dt in (torch.float64, torch.float32)}
    t64, t32 = leg[torch.float64]["taps"], leg[torch.float32]["taps"]
    # level 1: odd multiples of 1/2, the same bits in fp32
    assert torch.equal(t32[0].double(), t64[0]) and bool(((2 * t64[0]) % 2 == 1).all())
    sgn = torch.tensor([1.0 if o % 2 == 0 else -1.0 for o in range(h)], dtype=torch.float64)
    assert h == 1 or (bool((sgn > 0).any()) and bool((sgn < 0).any()))
    for l in range(1, c["layers"]):
        v = t64[l].view(-1, h) * sgn
        assert 1e-2 <= v.min().item() and v.max().item() <= 1e3, (l, v.min().item(), v.max().item())
        noise = (t32[l].double() - t64[l]).abs().max().item()
        assert v.min().item() >= U.MARGIN_M * noise, (l, v.min().item(), noise)
        assert bool(((t64[l] > 0) == (t32[l] > 0)).all())


def test_oracle_taps_change_nothing():
    adjs = U.tiny()[:-1]
    for order, fn in ((2, RC.ccn2_forward_closed), (1, RC.ccn1_forward_vec)):
        c = U._case("A", order, ("TINY",), 3, 4, 2, 2, "M", 5)
        xs, p = U.family_m(c, adjs)
        for x, a in zip(xs, adjs):
            taps = []
            assert torch.equal(fn(p, x, a, 2), fn(p, x, a, 2, taps))
            assert len(taps) == 2 and taps[0].numel() == 4 * int((U.degrees(a) ** order).sum())


def test_plan_restatement_equals_literal():
    """plan_ref (vectorised numpy) against receptive_fields / positions of oracle/ref_ccn.py"""
    for a in U.tiny()[:-1] + [U.er(20, 0.3, 1), U.lolli(5, 3), U.star(6)]:
        nbrs = RC.receptive_fields(a)
        deg, nbr, pos = U.plan_ref(a)
        assert np.array_equal(deg, [len(v) for v in nbrs])
        assert np.array_equal(nbr, np.concatenate([np.array(v) for v in nbrs]))
        lit = [q for i in range(len(nbrs)) for j in nbrs[i] for q in RC.positions(nbrs, i, j)]
        assert np.array_equal(pos, np.array(lit))
    # the multi-word batches of part C have what they are there for
    b = U.plan_batches()
    assert b["ccn2d er(130,0.5)+er(70,0.3)"][1][1].shape[0] == 70
    for nmax in (64, 65, 128, 129):
        g, k = b[f"ccn1d clique60 in {nmax}"][1]
        assert g.shape[0] == nmax and k.shape[0] == 60 and int(U.degrees(g).max()) >= 60


@pytest.mark.parametrize("name", ["A-ccn2d-TINY-f1h2L2o1-M","A-ccn2d-TINY-f16h16L3o8-M", "A-ccn1d-TINY-f8h8L2o1-M",
                                  "A-ccn1d-TINY-f17h12L2o3-M"])
def test_sensitivity_to_a_dropped_block(name):
    """The smallest and the largest case of each order: the fp64 oracle without any one of the 18 (2) blocks of any
    level misses the case's bound on some compared tensor."""
    c = U.BY_NAME[name]
    adjs, xs, p, w = U.inputs(name)
    l64, l32 = U.legs(name)
    keys = ["out", "dX"] + U.param_names(c["layers"])
    weakest = np.inf
    for l in range(c["layers"]):
        for q in range(18 if c["order"] == 2 else 2):
            d = U._leg(c, adjs, xs, p, w, torch.float64, True, drop=(l, q))
            worst = max(U.compare(d[k], l64[k], l32[k])["ratio"] for k in keys)
            weakest = min(weakest, worst)
            assert worst > U.FACTOR, (name, l, q, worst)
    print(f"{name}: the least visible dropped block measures {weakest:.3g} (bound {U.FACTOR})")
