"""Inputs, case tables, the dispatch mirror and the checks of tests/test_gpu_ccn_edges.py (the general CCN path,
csrc/ccn.hip and the files it names, at its kernel-selection and degree boundaries); tests/test_ccn_edge_inputs.py
checks all of it on the CPU.  Nothing here needs a GPU except run_gpu() and plan_maps_gpu().

Reference of every comparison: oracle/ref_ccn.py (ccn2_forward_closed / ccn1_forward_vec) in fp64, with the same
oracle in fp32 as the naive leg.  The kernel's rms and max error against fp64 may be at most FACTOR = 2 x the naive
leg's (oracle/parity.py, tests/test_gpu_gemm_kernels.py) plus one fp32 ulp of the tensor's largest magnitude.

Weight families (ReLU makes the gradient discontinuous, so the inputs keep every pre-activation away from zero):
  M  gaussian X, W = randn / (m cin), b = 0.1 randn, on the TINY batch; the seed of a case is committed in CASES_A
     and is one for which the fp64 oracle's smallest |pre-activation| is >= 100 x the level's max |pre32 - pre64|
     (the forward criterion holds the kernel to 2 x that error: a factor 50 is left);
  S  level 1 exact: X integers in [-2, 2], W1 in {-1, 0, 1} (every block non-zero), b1 = +-1/2 -- every partial sum
     in any order is a multiple of 1/2 below 2^23 (s_bound() proves it), never zero; levels >= 2 read non-negative
     inputs through channels that are alive (|randn| weights, bias +0.1 of the typical pre-activation) or dead (the
     negatives): the mask is fixed with a margin while every block's arithmetic runs on random magnitudes;
  R  M's recipe at the shapes of part B, outputs only (the forward is continuous).
"""

import functools

import numpy as np
import torch

from oracle import ref_ccn as RC

FACTOR = 2.0          # oracle/parity.py: the fp64-leg factor
MARGIN_M = 100.0      # family M: min |pre64| / max |pre32 - pre64| per level

# csrc/ccn_general.h constants the mirror restates
CCN_MAXD, CCN_BIGD, CCN1_MAXD = 64, 256, 1024
C1F = C1H = 8
C2_CMAX = C2_HMAX = 8
C2_NCAP = 64
RO_CH = 32
ASYNC_PLAN_BOUND = {1: 8 << 20, 2: 1 << 20}        # hgnn_amd/ccn.py ASYNC_PLAN_BOUND


# ---------------------------------------------------------------------------------------------- graphs
def star(n):
    """n nodes, node 0 adjacent to all: hub degree n (self loop included), leaves 2."""
    a = torch.eye(n)
    a[0, :] = 1.0
    a[:, 0] = 1.0
    return a


def clique(k):
    return torch.ones(k, k)


def lolli(k, t):
    """A k-clique with a path of t nodes hanging off node 0 (degree k + 1)."""
    a = torch.eye(k + t)
    a[:k, :k] = 1.0
    prev = 0
    for i in range(k, k + t):
        a[prev, i] = a[i, prev] = 1.0
        prev = i
    return a


def er(n, p, seed):
    r = np.random.RandomState(seed)
    u = np.triu(r.rand(n, n) < p, 1)
    return torch.from_numpy((u | u.T | np.eye(n, dtype=bool)).astype(np.float32))


def path_chords(n, seed):
    """A path of n nodes plus two random chords (fewer where the graph has no room for them)."""
    a = torch.eye(n)
    for i in range(n - 1):
        a[i, i + 1] = a[i + 1, i] = 1.0
    free = [(i, j) for i in range(n) for j in range(i + 2, n)]
    r = np.random.RandomState(seed)
    for k in r.permutation(len(free))[:2]:
        i, j = free[k]
        a[i, j] = a[j, i] = 1.0
    return a


TINY_SIZES = (1, 4, 6, 7, 5)


def tiny():
    """Five graphs of 1, 4, 6, 7 and 5 nodes and one empty slot (None)."""
    return [path_chords(n, 40 + n) for n in TINY_SIZES] + [None]


def clique_in(nmax, k=60):
    """nmax nodes on a path, k of them (evenly spread, so they straddle the 64-bit words) a clique."""
    a = torch.eye(nmax)
    for i in range(nmax - 1):
        a[i, i + 1] = a[i + 1, i] = 1.0
    m = torch.from_numpy(np.unique(np.linspace(0, nmax - 1, k).astype(np.int64)))
    a[m.view(-1, 1), m.view(1, -1)] = 1.0
    return a


GRAPHS = {
    "lolli(63,1)": lambda: lolli(63, 1), "lolli(64,2)": lambda: lolli(64, 2), "lolli(63,2)": lambda: lolli(63, 2),
    "star(130)": lambda: star(130), "star(256)": lambda: star(256), "clique(64)": lambda: clique(64),
    "clique(65)": lambda: clique(65), "star(129)": lambda: star(129), "star(1024)": lambda: star(1024),
    "star(257)": lambda: star(257), "star(1025)": lambda: star(1025),
}
# graph -> (max degree, min degree, nodes of degree above 64)
DEGREES = {
    "lolli(63,1)": (64, 2, 0), "lolli(64,2)": (65, 2, 1), "lolli(63,2)": (64, 2, 0), "star(130)": (130, 2, 1),
    "star(256)": (256, 2, 1), "clique(64)": (64, 64, 0), "clique(65)": (65, 65, 65), "star(129)": (129, 2, 1),
    "star(1024)": (1024, 2, 1), "star(257)": (257, 2, 1), "star(1025)": (1025, 2, 1),
}


def graphs_of(names):
    out = []
    for g in names:
        out += tiny() if g == "TINY" else [GRAPHS[g]()]
    return out


def degrees(adj):
    return (adj > 0).sum(1).numpy().astype(np.int64) if adj is not None else np.zeros(0, np.int64)


# ---------------------------------------------------------------------------------------------- cases
def _gname(graphs):
    return "+".join(g if graphs.count(g) == 1 else f"{graphs.count(g)}x{g}" for g in dict.fromkeys(graphs))


def _case(part, order, graphs, f, h, layers, n_out, family, seed):
    name = f"{part}-ccn{order}d-{_gname(tuple(graphs))}-f{f}h{h}L{layers}o{n_out}-{family}"
    return {"name": name, "part": part, "order": order, "graphs": tuple(graphs), "f": f, "h": h, "layers": layers,
            "n_out": n_out, "family": family, "seed": seed}


# part A: (f_in, hidden, layers, n_out) -> seed of family M (chosen by find_seed_m, asserted by the CPU test)
A_SHAPES = {
    2: {(1, 2, 2, 1): 0, (8, 3, 3, 3): 1, (9, 8, 2, 8): 0, (16, 9, 2, 3): 2, (8, 16, 2, 1): 3, (16, 16, 3, 8): 10},
    1: {(8, 8, 2, 1): 0, (9, 2, 2, 3): 0, (2, 9, 3, 8): 0, (17, 12, 2, 3): 0},
}
CASES_A = [_case("A", o, ("TINY",), *shp, "M", seed) for o in (2, 1) for shp, seed in A_SHAPES[o].items()]

B_CHANNELS_2D = ((5, 2, 2), (9, 3, 2), (5, 12, 2))
B_CHANNELS_1D = ((5, 2, 2), (9, 9, 2))
B_GRAPHS_2D = ("lolli(63,1)", "lolli(64,2)", "star(130)")
B_GRAPHS_1D = ("clique(64)", "clique(65)", "star(129)", "star(1024)")
B_NOUT = 8  # outputs per graph: bs n_out elements are the sample of the outputs' criterion


# graphs of one construction per batch (different X each).  A star's outputs hang on its hub alone: with one
# star(130), bs n_out = 8 outputs all combine the same 15 feature sums, and the fp32 oracle's error on them varied
# 1.7 .. 4 ulp rms from seed to seed (and between CPUs); (9, 3, 2) measured 2.66 on that sample, the other channel
# sets 0.25 and 0.39.  Four stars give the criterion 32 outputs from four hubs.
B_COPIES = {"star(130)": 4}


def cases_b(family):
    cs = [_case("B", 2, (g,) * B_COPIES.get(g, 1), f, h, L, B_NOUT, family, 11)
          for g in B_GRAPHS_2D for f, h, L in B_CHANNELS_2D]
    cs += [_case("B", 2, ("star(256)",), 1, 2, 2, B_NOUT, family, 12)]
    cs += [_case("B", 1, (g,), f, h, L, B_NOUT, family, 13) for g in B_GRAPHS_1D for f, h, L in B_CHANNELS_1D]
    # B8: the degree-65 graph first, then the ragged TINY graphs and the empty slot (nmax = 66)
    cs += [_case("B", 2, ("lolli(64,2)", "TINY"), 5, 2, 2, B_NOUT, family, 14)]
    # item 9: nmax = 65 without a degree above 64 (the async plan's bounds call the graph big, the sync plan does not)
    cs += [_case("B", 2, ("lolli(63,2)",), 5, 2, 2, B_NOUT, family, 15)]
    return cs


CASES_S = cases_b("S")
CASES_R = cases_b("R")
BY_NAME = {c["name"]: c for c in CASES_A + CASES_S + CASES_R}
# B7: these run under both plans
BOTH_PLANS = ("lolli(63,1)", "lolli(64,2)", "lolli(63,2)")


def param_names(layers):
    return [f"w{l + 1}.{k}" for l in range(layers) for k in ("weight", "bias")] + ["fc.weight", "fc.bias"]


def _oracle(order):
    return RC.ccn2_forward_closed if order == 2 else RC.ccn1_forward_vec


def _forward(order, p, x, adj, layers, taps=None):
    """The oracle on one graph; an empty slot has no rows: its features are zero (model_ccn.py:102-105)."""
    if adj is None or adj.shape[0] == 0:
        nf = p["fc.weight"].shape[1]
        if taps is not None:
            taps += [x.new_zeros(0)] * layers
        return p["fc.weight"] @ x.new_zeros(nf) + p["fc.bias"]
    return _oracle(order)(p, x, adj.to(x.dtype), layers, taps)


# ---------------------------------------------------------------------------------------------- families
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _sizes(adjs):
    return [0 if a is None else a.shape[0] for a in adjs]


def family_m(case, adjs, seed=None):
    """fp32 tensors: X per graph, params by name"""
    c = case
    g = _gen(1000 * (c["seed"] if seed is None else seed) + 7)
    m = 18 if c["order"] == 2 else 2
    xs = [torch.randn(n, c["f"], generator=g) for n in _sizes(adjs)]
    p = {}
    for l in range(c["layers"]):
        cin = c["f"] if l == 0 else c["h"]
        p[f"w{l + 1}.weight"] = torch.randn(c["h"], m * cin, generator=g) / (m * cin)
        p[f"w{l + 1}.bias"] = 0.1 * torch.randn(c["h"], generator=g)
    nf = c["f"] + c["layers"] * c["h"]
    p["fc.weight"] = torch.randn(c["n_out"], nf, generator=g)
    p["fc.bias"] = 0.1 * torch.randn(c["n_out"], generator=g)
    return xs, p


def family_s(case, adjs):
    c = case
    g = _gen(1000 * c["seed"] + 9)
    m = 18 if c["order"] == 2 else 2
    f, h, L = c["f"], c["h"], c["layers"]
    xs = [torch.randint(-2, 3, (n, f), generator=g).float() for n in _sizes(adjs)]
    w1 = torch.randint(-1, 2, (h, m * f), generator=g).float()
    for q in range(m):  # every block has non-zeros
        if not w1[:, q * f:(q + 1) * f].any():
            w1[q % h, q * f] = 1.0 if q % 2 else -1.0
    p = {"w1.weight": w1, "w1.bias": torch.randint(0, 2, (h,), generator=g).float() - 0.5}
    sgn = torch.tensor([1.0 if o % 2 == 0 else -1.0 for o in range(h)])
    for l in range(1, L):
        mag = torch.randn(h, m * h, generator=g).abs()
        # calibrate on the fp64 oracle: all channels alive, no bias -> this level's pre-activations
        q = {k: v.double() for k, v in p.items()}
        q[f"w{l + 1}.weight"], q[f"w{l + 1}.bias"] = mag.double(), torch.zeros(h, dtype=torch.float64)
        q["fc.weight"], q["fc.bias"] = torch.zeros(1, f + (l + 1) * h, dtype=torch.float64), torch.zeros(1).double()
        taps = []
        with torch.no_grad():
            for x, a in zip(xs, adjs):
                t = []
                _forward(c["order"], q, x.double(), a, l + 1, t)
                taps.append(t[l])
        t = torch.cat(taps)
        scale = 100.0 / max(t.max().item(), 1e-30)          # the level's largest value: 100
        typical = max(t.median().item() * scale, 0.1)       # alive bias: 0.1 of the typical value, >= 1e-2
        p[f"w{l + 1}.weight"] = (sgn.view(-1, 1) * mag * scale).float()
        p[f"w{l + 1}.bias"] = (sgn * 0.1 * typical).float()
    nf = f + L * h
    p["fc.weight"] = torch.randn(c["n_out"], nf, generator=g)
    p["fc.bias"] = torch.randn(c["n_out"], generator=g)
    return xs, p


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(adjs, xs, params, w): the case's graphs (None = empty slot), fp32 inputs and the loss weights of
    loss = sum(out * w)."""
    c = BY_NAME[name]
    adjs = graphs_of(c["graphs"])
    xs, p = family_s(c, adjs) if c["family"] == "S" else family_m(c, adjs)
    w = torch.randn(len(adjs), c["n_out"], generator=_gen(c["seed"] + 31))
    return adjs, xs, p, w


def pad(adjs, xs):
    bs, nmax, f = len(adjs), max(max(_sizes(adjs)), 1), xs[0].shape[1]
    X, A = torch.zeros(bs, nmax, f), torch.zeros(bs, nmax, nmax)
    for b, (x, a) in enumerate(zip(xs, adjs)):
        n = x.shape[0]
        X[b, :n] = x
        if n:
            A[b, :n, :n] = a
    return X, A, torch.tensor(_sizes(adjs), dtype=torch.int64)


# ---------------------------------------------------------------------------------------------- oracle legs
def _leg(c, adjs, xs, p, w, dtype, grad, drop=None):
    """One oracle leg: {'out', 'dX', grads by name, 'taps': per level the batch's pre-activations}.
    drop = (level, block): that block of the level's weight is taken out (sensitivity)."""
    p = {k: v.to(dtype).clone() for k, v in p.items()}
    if drop is not None:
        l, q = drop
        cin = c["f"] if l == 0 else c["h"]
        p[f"w{l + 1}.weight"][:, q * cin:(q + 1) * cin] = 0
    nmax = max(max(_sizes(adjs)), 1)
    res = {"out": torch.zeros(len(adjs), c["n_out"], dtype=dtype), "dX": torch.zeros(len(adjs), nmax, c["f"], dtype=dtype)}
    taps = [[] for _ in range(c["layers"])]
    if grad:
        for v in p.values():
            v.requires_grad_(True)
    with torch.set_grad_enabled(grad):
        for b, (x, a) in enumerate(zip(xs, adjs)):
            xr = x.to(dtype).clone().requires_grad_(grad)
            t = []
            o = _forward(c["order"], p, xr, a, c["layers"], t)
            for l in range(c["layers"]):
                taps[l].append(t[l])
            res["out"][b] = o.detach()
            if grad:
                (o * w[b].to(dtype)).sum().backward()
                if x.shape[0]:
                    res["dX"][b, :x.shape[0]] = xr.grad
    if grad:
        for k, v in p.items():
            res[k] = v.grad if v.grad is not None else torch.zeros_like(v)
    else:
        del res["dX"]
    res["taps"] = [torch.cat(t) for t in taps]
    return res


@functools.lru_cache(maxsize=None)
def legs(name):
    """(fp64 leg, fp32 leg) of a case; family R has outputs only.  Computed once per process."""
    c = BY_NAME[name]
    adjs, xs, p, w = inputs(name)
    grad = c["family"] != "R"
    return _leg(c, adjs, xs, p, w, torch.float64, grad), _leg(c, adjs, xs, p, w, torch.float32, grad)


def margin_m(l64, l32):
    """family M's condition: per level min |pre64| / max |pre32 - pre64|, and whether the ReLU patterns agree"""
    ratios, same = [], True
    for t64, t32 in zip(l64["taps"], l32["taps"]):
        noise = (t32.double() - t64).abs().max().item()
        ratios.append(t64.abs().min().item() / max(noise, 1e-300))
        same = same and bool(((t64 > 0) == (t32 > 0)).all())
    return min(ratios), same


def find_seed_m(case, tries=24):
    """The first seed whose margin reaches MARGIN_M (how the seeds of A_SHAPES were chosen)."""
    adjs = graphs_of(case["graphs"])
    w = torch.zeros(len(adjs), case["n_out"])
    for seed in range(tries):
        xs, p = family_m(case, adjs, seed)
        m, same = margin_m(_leg(case, adjs, xs, p, w, torch.float64, False), _leg(case, adjs, xs, p, w, torch.float32, False))
        if same and m >= MARGIN_M:
            return seed, m
    return None, 0.0


def s_bound(name):
    """Family S: the largest level-1 intermediate, from the oracle on (|X|, |W1|, |b1|) -- all non-negative, so
    its ReLU is the identity and each pre-activation is the sum of the magnitudes of every term of the signed run."""
    c = BY_NAME[name]
    adjs, xs, p, _ = inputs(name)
    q = {"w1.weight": p["w1.weight"].abs().double(), "w1.bias": p["w1.bias"].abs().double(),
         "fc.weight": torch.zeros(1, c["f"] + c["h"], dtype=torch.float64), "fc.bias": torch.zeros(1).double()}
    big = 0.0
    with torch.no_grad():
        for x, a in zip(xs, adjs):
            t = []
            _forward(c["order"], q, x.abs().double(), a, 1, t)
            if t[0].numel():
                big = max(big, t[0].max().item())
    return big


# ---------------------------------------------------------------------------------------------- criteria
def _ulp(x):
    return float(np.spacing(np.float32(x))) if x > 0 else 0.0


def compare(got, r64, r32):
    """{'rms': (kernel, naive, bound), 'max': (...), 'ratio': worst of kernel / bound, 'zeros_ok'} for one tensor.
    Elements that are exactly zero in the fp64 oracle (analytic zeros: autograd never touched them) must be
    exactly zero."""
    g, a, b = got.detach().double().cpu(), r64.double(), r32.double()
    assert g.shape == a.shape, (g.shape, a.shape)
    if g.numel() == 0:
        return {"rms": (0, 0, 0), "max": (0, 0, 0), "ratio": 0.0, "zeros_ok": True, "pass": True}
    ek, en = g - a, b - a
    ulp = _ulp(a.abs().max().item())
    rk, rn = ek.pow(2).mean().sqrt().item(), en.pow(2).mean().sqrt().item()
    mk, mn = ek.abs().max().item(), en.abs().max().item()
    br, bm = FACTOR * rn + ulp, FACTOR * mn + ulp
    zeros_ok = bool((g[a == 0] == 0).all())
    # ratio: the error over the bound, scaled so that 2.00 is the limit as in the module's table
    ratio = max(FACTOR * rk / br if br else (0.0 if rk == 0 else np.inf), FACTOR * mk / bm if bm else (0.0 if mk == 0 else np.inf))
    return {"rms": (rk, rn, br), "max": (mk, mn, bm), "ratio": ratio, "zeros_ok": zeros_ok,
            "pass": rk <= br and mk <= bm and zeros_ok}


def check(name, got, tag=""):
    """got: {'out', 'dX', grads...} from run_gpu.  Asserts the criteria on every tensor the case compares, prints the
    table row (worst tensor and its ratio) before asserting."""
    c = BY_NAME[name]
    l64, l32 = legs(name)
    keys = ["out"] if c["family"] == "R" else ["out", "dX"] + param_names(c["layers"])
    res = {k: compare(got[k], l64[k], l32[k]) for k in keys}
    worst = max(res, key=lambda k: res[k]["ratio"])
    r = res[worst]
    row = (f"  {name}{tag:<8} worst {worst:<10} ratio {r['ratio']:.2f}  rms {r['rms'][0]:.2e} / {r['rms'][1]:.2e}"
           f"  max {r['max'][0]:.2e} / {r['max'][1]:.2e}")
    print("TABLE" + row)
    bad = {k: v for k, v in res.items() if not v["pass"]}
    assert not bad, f"{name}{tag}: " + "; ".join(
        f"{k}: rms {v['rms'][0]:.3g} > {v['rms'][2]:.3g} or max {v['max'][0]:.3g} > {v['max'][2]:.3g} or zeros {v['zeros_ok']}"
        for k, v in bad.items())
    if c["family"] != "R":  # containment: dX rows at and beyond n_b are exactly zero
        adjs = inputs(name)[0]
        for b, n in enumerate(_sizes(adjs)):
            assert got["dX"][b, n:].abs().sum().item() == 0.0, f"{name}: dX rows of graph {b} beyond n_b = {n}"
    return res


# ---------------------------------------------------------------------------------------------- dispatch mirror
def auto_plan(order, bs, nmax):
    """hgnn_amd/ccn.py _plan"""
    return "async" if bs * nmax ** 3 <= ASYNC_PLAN_BOUND[order] else "sync"


def ro_chunks(rows, bs):
    """ccn_readout.hip ro_chunks"""
    per = rows // bs if bs > 0 else rows
    return min(per // 4096 + 1, RO_CH)


def mirror(order, f, h, layers, degs, bs, nmax, plan):
    """The kernels and branches hgnn_ccn_forward / hgnn_ccn_backward (ccn.hip) select for a batch whose
    graphs have the degree arrays `degs` (one per slot), as a set of names."""
    alld = np.concatenate([np.asarray(d, np.int64) for d in degs]) if degs else np.zeros(0, np.int64)
    dmax = int(alld.max()) if alld.size else 0
    if plan == "async":  # ccn_plan.hip ccn_plan: bounds from the shape
        s0, s2, s3 = bs * nmax * nmax, bs * nmax, nmax
    else:                # ccn_plan.hip ccn_plan: the device totals
        s0, s2, s3 = int(alld.sum()), int(alld.size), dmax
    names = {f"plan[{plan}]"}
    if order == 2:
        big = s3 > CCN_MAXD                                           # ccn.hip CcnRun::bigd
        for d in (64, 65, 256):
            if (alld == d).any():
                names.add(f"c2[deg={d}]")
        if big and dmax <= CCN_MAXD:
            names.add("c2[big kernels over zero nodes]")
        names.add("k_ccn_bcast" if big else "top_direct")             # ccn.hip ccn2_backward
        for l in range(layers):
            cin = f if l == 0 else h
            narrow = cin <= C2_CMAX and h <= C2_HMAX                  # ccn_general.h c2_big_select
            if l == 0:                                                # ccn_general.h c2_select, level 0
                t = "8,2,1,true" if cin <= 8 else "16,2,1,true"
                names |= {f"k_c2_fwd<{t}>", f"k_c2_bwd<{t}>", "k_ccn2_dx0[cin>8]" if cin > 8 else "k_ccn2_dx0"}
            else:                                                     # ccn_general.h c2_select, levels >= 1
                t = "2,2,8,false" if cin <= 2 else "8,2,4,false" if cin <= 8 else "16,2,2,false"
                tb = t if cin <= 8 else "16,1,2,false"
                names |= {f"k_c2_fwd<{t}>", f"k_c2_bwd<{tb}>", f"c2_level[cin={cin}]"}
                g = "2,8" if h <= 2 else "8,1" if h <= 8 else "16,1"  # ccn_general.h c2_gather_select
                names |= {f"k_c2_gather<{g}>", f"k_c2_gather<{g}>[h={h}]"}
                if s3 > C2_NCAP:                                      # ccn.hip ccn2_backward
                    names.add("k_c2_gather_big<%s>" % ("2,4" if h <= 2 else g))
            if big:                                                   # ccn.hip ccn2_forward, ccn2_backward
                t = "8,8" if narrow else "16,16"
                names |= {f"k_ccn2_fwd_big<{t}>", f"k_ccn2_bwd_node_big<{t}>", "k_c2_dp_big"}
        names.add(f"readout[nch={ro_chunks(s2, bs)}]")               # ccn.hip hgnn_ccn_forward: nodes
        if f > C2_CMAX:
            names.add("readout[f passes>1]")                          # ccn_readout.hip k_ccn_readout_part
        if h > C2_CMAX:
            names.add("readout[h passes>1]")                          # ccn_readout.hip k_ccn_readout_part
    else:
        for d in (64, 65, 1024):
            if (alld == d).any():
                names.add(f"c1[deg={d}]")
        small, large = bool((alld <= 64).any()), bool((alld > 64).any())
        for l in range(layers):
            cin = f if l == 0 else h
            if small:  # ccn1.hip: the one-chunk branch of each kernel
                names.add("k_ccn1_fwd[fast]" if cin <= C1F else "k_ccn1_fwd[chunked,n<=64,cin>8]")
                names.add("k_ccn1_bwd_node[fast]" if cin <= C1F and h <= C1H else
                          "k_ccn1_bwd_node[chunked,n<=64]")
                names.add("k_ccn1_bwd_gather[fast]" if cin <= C1F else "k_ccn1_bwd_gather[chunked,n<=64,cin>8]")
            if large:
                names |= {"k_ccn1_fwd[chunked,n>64]", "k_ccn1_bwd_node[chunked,n>64]", "k_ccn1_bwd_gather[chunked,n>64]"}
        names.add(f"readout1[nch={ro_chunks(s0, bs)}]")              # ccn.hip hgnn_ccn_forward: sum of degrees
        if h > C2_CMAX:
            names.add("readout1[h passes>1]")
        if f > C2_CMAX:
            names.add("readout1[f passes>1]")
    return names


def case_mirror(name, plan=None):
    c = BY_NAME[name]
    adjs = graphs_of(c["graphs"])
    bs, nmax = len(adjs), max(max(_sizes(adjs)), 1)
    plan = plan or auto_plan(c["order"], bs, nmax)
    return mirror(c["order"], c["f"], c["h"], c["layers"], [degrees(a) for a in adjs], bs, nmax, plan)


# the issue's items 1-9 -> names every one of which some case must select
COVERAGE = {
    1: {"k_c2_fwd<16,2,1,true>", "k_c2_bwd<16,2,1,true>", "k_ccn2_dx0[cin>8]", "readout[f passes>1]"},
    2: {"c2_level[cin=8]", "c2_level[cin=9]", "c2_level[cin=16]", "k_c2_gather<8,1>[h=8]"},
    3: {"k_ccn1_fwd[chunked,n<=64,cin>8]", "k_ccn1_bwd_node[chunked,n<=64]", "k_ccn1_bwd_gather[chunked,n<=64,cin>8]",
        "readout1[h passes>1]"},
    4: {"c2[deg=64]", "c2[deg=65]"},
    5: {"c2[deg=256]"},
    6: {"c1[deg=64]", "c1[deg=65]", "readout1[nch=2]"},
    7: {"c1[deg=1024]"},
    8: {"refuse[order=1]", "refuse[order=2]"},
    9: {"c2[big kernels over zero nodes]", "item9[async: k_ccn_bcast, sync: top_direct]"},
}
REFUSALS = ((2, "star(257)"), (1, "star(1025)"))


def covered():
    names = set()
    for c in CASES_A + CASES_S:
        names |= case_mirror(c["name"])
        if c["graphs"][0] in BOTH_PLANS and len(c["graphs"]) == 1:
            a, s = case_mirror(c["name"], "async"), case_mirror(c["name"], "sync")
            names |= a | s
            if "k_ccn_bcast" in a and "top_direct" in s:
                names.add("item9[async: k_ccn_bcast, sync: top_direct]")
    for order, g in REFUSALS:
        n = GRAPHS[g]().shape[0]
        # above the async bound: the sync plan reads the error word before any forward is enqueued
        if auto_plan(order, 1, n) == "sync" and DEGREES[g][0] > (CCN_BIGD if order == 2 else CCN1_MAXD):
            names.add(f"refuse[order={order}]")
    return names


# ---------------------------------------------------------------------------------------------- plan maps
def plan_ref(adj):
    """(deg, nbr, pos) of one graph as oracle/ref_ccn.py receptive_fields / positions define them, vectorised:
    nbr_i ascending nonzero(adj[i]); pos[i][a][x] = index of nbr_i[x] in nbr_{nbr_i[a]}, or -1."""
    m = np.asarray(adj) > 0
    n = m.shape[0]
    deg = m.sum(1).astype(np.int64)
    nbr = np.nonzero(m)[1].astype(np.int64)            # row-major: each row's columns ascending
    idx = np.where(m, np.cumsum(m, 1) - 1, -1)         # idx[j, v] = position of v in nbr_j
    off = np.concatenate([[0], np.cumsum(deg)])
    pos = [idx[np.ix_(nbr[off[i]:off[i + 1]], nbr[off[i]:off[i + 1]])].reshape(-1) for i in range(n)]
    return deg, nbr, (np.concatenate(pos) if pos else np.zeros(0)).astype(np.int64)


def plan_batches():
    """name -> (order, [adj or None]) of part C"""
    out = {}
    for c in CASES_S:
        out[f"ccn{c['order']}d " + "+".join(c["graphs"])] = (c["order"], graphs_of(c["graphs"]))
    for order in (1, 2):
        out[f"ccn{order}d er(130,0.5)+er(70,0.3)"] = (order, [er(130, 0.5, 3), er(70, 0.3, 4)])
        for nmax in (64, 65, 128, 129):
            out[f"ccn{order}d clique60 in {nmax}"] = (order, [clique_in(nmax), clique(60)])
    return out


# ---------------------------------------------------------------------------------------------- GPU
def run_gpu(name, plan=None, per_graph=False):
    """forward_batch + backward of loss = sum(out * w) on the general path; plan 'sync' forces hgnn_ccn_plan.
    Returns {'out', 'dX', grads by name} on the CPU (and 'per_graph': the drop-in forward of each graph)."""
    import hgnn_amd.ccn as HC
    from models.compnets.model_ccn import CCN_1D, CCN_2D
    c = BY_NAME[name]
    adjs, xs, p, w = inputs(name)
    net = (CCN_2D if c["order"] == 2 else CCN_1D)(c["f"], c["n_out"], c["h"], c["layers"], False)
    with torch.no_grad():
        for k, v in net.named_parameters():
            v.copy_(p[k])
    net = net.cuda()
    X, A, nb = (t.cuda() for t in pad(adjs, xs))
    old = HC.SMALL, HC.ASYNC_PLAN_BOUND
    HC.SMALL = False
    if plan == "sync":
        HC.ASYNC_PLAN_BOUND = {1: 0, 2: 0}
    elif plan == "async":
        assert auto_plan(c["order"], X.shape[0], X.shape[1]) == "async"
    try:
        Xr = X.clone().requires_grad_(True)
        out = net.forward_batch(Xr, A, nb)
        res = {"out": out.detach().cpu()}
        if c["family"] != "R":
            (out * w.cuda()).sum().backward()
            res["dX"] = Xr.grad.cpu()
            for k, v in net.named_parameters():
                res[k] = v.grad.detach().cpu()
        if per_graph:
            with torch.no_grad():
                res["per_graph"] = torch.stack([net(x.cuda(), a.cuda()).cpu() for x, a in zip(xs, adjs)])
        torch.cuda.synchronize()
    finally:
        HC.SMALL, HC.ASYNC_PLAN_BOUND = old
    return res


def plan_maps_gpu(order, adjs):
    from hgnn_amd.ccn import plan_maps
    X, A, nb = pad(adjs, [torch.zeros(0 if a is None else a.shape[0], 1) for a in adjs])
    return plan_maps(order, X.cuda(), A.cuda(), nb.cuda())
