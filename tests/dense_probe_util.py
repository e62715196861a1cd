"""Inputs, references, case tables and runners of the dense-side kernel probes outside the GEMMs (include/hgnn_amd.h,
"Kernel probes"; csrc/probe_dense.hip): the BN backward and finalize, the readout launchers (csrc/bn.hip) and the dense
operator gradient (csrc/dwdense.hip, k_dw_readout).  Shared by tests/test_dense_probe_inputs.py (CPU: the inputs and
the checks have the properties the GPU tests rely on), tests/test_gpu_dense_kernels.py and its child-process worker
tests/dense_probe_worker.py.  The counterpart of tests/gemm_probe_util.py and tests/sparse_probe_util.py.

Families.  "E" (exact): small integers and powers of two, chosen so that every product and every partial sum a
kernel can form is exact in fp32 (and in the fp64 atomics), whatever its summation order: the outputs that are sums
equal the fp64 result bit for bit.
  BN backward: y, dz integers in [-7, 7] (dz drawn from [-5, 7]: a non-zero mean), mean an integer in [-3, 3], std in
    {0.5, 1, 2, 4}, w in {+-1, +-2}: h = (y - mean) / std is a multiple of 0.25 with |h| <= 20, |g h| <= 280, and the
    sum over 1100 rows stays below 2^24 quarter units.  Exact: the four statistics, dw, db, and in eval mode dy and
    dbpart.  The training-mode dy multiplies by the rounded 1 / total, so it is held to the naive bound instead.
  readout, dense dW: integer features, gradients and fc weights, dyadic operator coefficients.
"R" (random): normals with a per-channel offset.  rms and max error against fp64 at most FACTOR x those of the
naive fp32 form of the same formula (sequential sums, every operation rounded); the float4 BN kernels' naive form
multiplies by the once-rounded 1 / std (kernels.h bn_bwd_dy_inv), the scalar kernels' divides.  Outputs that are one
fp64 sum rounded once (colsum, dfcw, dfcb, the finalize's mean / std) are held to 1 fp32 ulp of the fp64 reference.

Every runner pre-fills outputs with SENT and scratch / unread inputs with NaN; the checks assert what must keep the
sentinel and that no output is non-finite.
"""

import ctypes

import numpy as np
import torch

from gemm_probe_util import FACTOR, SENT, errs, ulp_dist, values_equal  # noqa: F401

F32, F64 = np.float32, np.float64
NAN = float("nan")
EPS = 2.0 ** -24
PATHS = ("narrow2s", "wide2", "part4acc", "part4fin", "scalar")   # hgnn_amd._lib.BN_BWD_PATHS
ERR_ARG, ERR_UNSUPPORTED = 1, 2
POOL_BELOW = 256              # check_bound: outputs of fewer values pool the naive form over several row orders


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def sentinel(a):
    """All of a float32 array still holds SENT bit for bit."""
    return bool((np.ascontiguousarray(a, F32).view(np.int32) == np.array(SENT, F32).view(np.int32)).all())


def check_finite(name, got):
    assert np.isfinite(got).all(), (name, "non-finite output: a poisoned element was read")


def check_exact(name, got, ref64):
    """Bit for bit the fp64 result rounded once (the sign of a zero aside)."""
    check_finite(name, got)
    want = np.asarray(ref64, F64).astype(F32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert values_equal(_t(got), _t(want)), (name, "not exact", errs(_t(got), _t(np.asarray(ref64, F64))))


def check_bound(name, got, ref64, naive32, report=None, kernel=None, width=None):
    """rms and max error against fp64 at most FACTOR x those of the naive fp32 form.

    naive32 may be a list: the naive form in its stored row order first, then in further row orders (it has no
    canonical one, and neither has the kernel).  An output of POOL_BELOW values or more is held to the stored order
    alone.  A smaller one -- a narrow layer's statistics, the column sums of one tile, the scalars dw and db -- is too
    small a sample of one order's error: its yardstick is the rms over all the orders' errors and the largest of
    their max errors.  (The case that forced this: scalar path, c = 5, 63 rows, training, dbpart -- five values near
    4620, where an ulp is 4.9e-4: the kernel's worst was 4.7e-4, the stored order's by chance 1.6e-5.)  For a single value rms and max coincide, and 2 x an rms estimate would refuse a correct kernel
    one time in twenty, so only the max criterion is applied to it."""
    check_finite(name, got)
    nvs = naive32 if isinstance(naive32, list) else [naive32]
    if got.size >= POOL_BELOW:
        nvs = nvs[:1]
    assert all(got.shape == ref64.shape == n.shape for n in nvs), (name, got.shape, ref64.shape, nvs[0].shape)
    kr, kx = errs(_t(got), _t(ref64))
    ne = [errs(_t(n), _t(ref64)) for n in nvs]
    nr, nx = float(np.sqrt(np.mean([e[0] ** 2 for e in ne]))), max(e[1] for e in ne)
    if got.size == 1:
        nr = nx
    if report is not None:
        report.append(dict(name=name, kernel=kernel, width=width, rms=kr, max=kx, nrms=nr, nmax=nx))
    assert kr <= FACTOR * nr and kx <= FACTOR * nx, (name, "rms", kr, nr, "max", kx, nx)


def check_ulp(name, got, ref64, ulps=1):
    """Within `ulps` fp32 ulp of the fp64 reference rounded to fp32."""
    check_finite(name, got)
    want = np.asarray(ref64, F64).astype(F32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    d = ulp_dist(_t(got) + 0.0, _t(want) + 0.0)
    assert int(d.max()) <= ulps if d.numel() else True, (name, "ulp distance", int(d.max()))


# ================================================================================================ BN backward
# (total, cap_rows): a partly filled last tile and whole empty tiles of capacity behind it
BN_TOTALS = ((0, 128), (1, 128), (63, 192), (64, 192), (65, 192), (255, 384), (256, 384), (257, 448), (300, 448),
             (1030, 1100))
BN_R_TOTALS = (65, 300, 1030)
SCALAR_C = (1, 3, 5, 255, 257)
NARROW_C = (4, 8, 16)
PART4_C = (12, 20, 40, 100, 516, 1024)
WIDE_C = (64, 128, 256)
BN_WIDTHS = SCALAR_C + NARROW_C + PART4_C + WIDE_C
BN2_MAX_TILES = 192           # bn.hip bn_bwd_variant: the two-launch forms up to 192 256-row tiles of capacity
FALLBACK_CAP = BN2_MAX_TILES * 256 + 1


def bn_switches(env=None):
    """(narrow two-launch on, wide two-launch on) under HGNN_BN_BWD2 (unset: narrow only; 0: none; 1: both)."""
    v = (env or {}).get("HGNN_BN_BWD2")
    return (v != "0", v == "1")


def bn_expected_path(cs, env=None):
    """kernels.h bn_bwd_variant, from the case alone."""
    c, ldy = cs["c"], cs.get("ldy", 0)
    narrow, wide = bn_switches(env)
    if c % 4 or c > 1024 or cs.get("misalign") or ldy not in (0, c):
        return "scalar"
    t256 = -(-cs["cap"] // 256)
    if cs["apply"] and cs["cap"] > 0 and t256 <= BN2_MAX_TILES:
        if narrow and c in NARROW_C:
            return "narrow2s"
        if wide and c in WIDE_C:
            return "wide2"
    return "part4acc" if cs.get("acc") and cs["apply"] else "part4fin"


def bn_cases(widths=BN_WIDTHS):
    out = []
    for c in widths:
        seed = 1000 * c
        for i, (total, cap) in enumerate(BN_TOTALS):
            base = dict(c=c, total=total, cap=cap, fam="E", ldy=0, misalign=0)
            out.append(dict(base, training=1, apply=1, dbpart=1, acc=1, relu_from=c // 2, seed=seed + i))
            if c < 255 or i % 2 == 0:
                out.append(dict(base, training=0, apply=1, dbpart=i % 2, acc=0, relu_from=(0, c)[(i // 2) % 2],
                                seed=seed + 20 + i))
            if total in (65, 1030):     # the statistics alone (part + fin): acc64 given, not used
                out.append(dict(base, training=1, apply=0, dbpart=0, acc=1, relu_from=0, seed=seed + 40 + i))
            if total in BN_R_TOTALS:
                out.append(dict(base, fam="R", training=1, apply=1, dbpart=1, acc=i % 2, relu_from=c // 2,
                                seed=seed + 60 + i))
    return out


def bn_scalar_forced_cases():
    """c % 4 == 0 taken to the scalar path: a padded dY stride (padding zeroed) and a 4-byte-offset dy."""
    out = []
    for c in (4, 64, 260):
        for i, (total, cap) in enumerate(((65, 192), (300, 448))):
            for fam in ("E", "R"):
                b = dict(c=c, total=total, cap=cap, fam=fam, training=1 - (i if fam == "E" else 0), apply=1, dbpart=1,
                         acc=1, relu_from=c // 2, seed=77000 + c + i)
                out.append(dict(b, ldy=c + 4, misalign=0))
                out.append(dict(b, ldy=0, misalign=1))
    return out


def bn_many_tiles_cases():
    """66 64-row tiles: k_bn_bwd_fin's lanes take a second tile each (the tables above end at 17 tiles).  Still exact:
    4200 rows of |g h| <= 280 in quarter units stay below 2^24."""
    out = []
    for c in (12, 5):
        b = dict(c=c, total=4200, cap=4288, fam="E", dbpart=1, acc=0, relu_from=c // 2, ldy=0, misalign=0)
        out += [dict(b, training=0, apply=1, seed=88000 + c), dict(b, training=1, apply=1, seed=88100 + c),
                dict(b, training=1, apply=0, seed=88200 + c)]
    return out


def bn_data(cs):
    g = np.random.default_rng(cs["seed"])
    c, total = cs["c"], cs["total"]
    if cs["fam"] == "E":
        y = g.integers(-7, 8, (total, c)).astype(F32)
        y[g.random(y.shape) < 0.05] = 0.0
        y[g.random(y.shape) < 0.05] = -0.0
        dz = g.integers(-5, 8, (total, c)).astype(F32)
        mean = g.integers(-3, 4, c).astype(F32)
        std = g.choice(np.array([0.5, 1.0, 2.0, 4.0], F32), c)
        w = F32(g.choice([-2.0, -1.0, 1.0, 2.0]))
    else:
        off = (g.uniform(0.5, 2.0, c) * g.choice([-1.0, 1.0], c))
        y = (g.standard_normal((total, c)) + off).astype(F32)
        dz = (g.standard_normal((total, c)) + g.uniform(0.5, 1.5, c)).astype(F32)
        mean = (off + 0.1 * g.standard_normal(c)).astype(F32)
        std = g.uniform(0.5, 2.0, c).astype(F32)
        w = F32(1.3)
    return dict(y=y, dz=dz, mean=mean, std=std, w=w)


def _relu_mask(cs, y):
    m = np.zeros(y.shape, bool)
    m[:, cs["relu_from"]:] = ~(y[:, cs["relu_from"]:] > 0)
    return m


def _tile_sums(dy, dtype):
    total, c = dy.shape
    t64 = -(-total // 64)
    out = np.zeros((t64, c), dtype)
    for t in range(t64):
        blk = dy[t * 64:(t + 1) * 64]
        if dtype == F64:
            out[t] = blk.sum(0)
        else:
            s = np.zeros(c, F32)
            for r in range(len(blk)):
                s = s + blk[r]
            out[t] = s
    return out


def bn_ref64(d, cs, n_for_mean=None):
    """fp64 of the formulas of kernels.h BnBwdArgs / bn_bwd_dy: sums [c][4] = {sum g, sum g h, sum dz h, sum dz},
    dy, dbpart (64-row tile column sums of dy), dw = sum_c sum dz h, db = sum_c sum dz."""
    y, dz = d["y"].astype(F64), d["dz"].astype(F64)
    mu, sd, w = d["mean"].astype(F64), d["std"].astype(F64), F64(d["w"])
    total = cs["total"]
    n = total if n_for_mean is None else n_for_mean
    h, g = (y - mu) / sd, w * dz
    S = np.stack([g.sum(0), (g * h).sum(0), (dz * h).sum(0), dz.sum(0)], 1)
    m1, m2 = (S[:, 0] / n, S[:, 1] / n) if n > 0 else (np.zeros_like(mu), np.zeros_like(mu))
    dy = (g - m1 - h * m2) / sd if cs["training"] else g / sd
    dy = np.where(_relu_mask(cs, d["y"]), 0.0, dy)
    return dict(sums=S, dy=dy, dbpart=_tile_sums(dy, F64), dw=S[:, 2].sum(), db=S[:, 3].sum())


def bn_naive_orders(d, cs, inv):
    """bn_naive32 in the stored row order and in further orders (rows permuted inside their 64-row tile, so every
    output keeps its meaning): 8 orders below 512 channels, 4 from there on.  The stored order comes first."""
    g = np.random.default_rng(cs["seed"] + 1)
    out = []
    for i in range(8 if cs["c"] < 512 else 4):
        perm = np.arange(cs["total"])
        if i:
            for t0 in range(0, cs["total"], 64):
                g.shuffle(perm[t0:t0 + 64])
        out.append(bn_naive32(d, cs, inv, perm))
    res = {k: [o[k] for o in out] for k in ("sums", "dy", "dbpart")}
    # dw / db as the kernels document them: the per-channel fp32 statistic, summed over the channels in fp64, rounded
    res["dw"] = [np.array([o["sums"][:, 2].astype(F64).sum()], F64).astype(F32) for o in out]
    res["db"] = [np.array([o["sums"][:, 3].astype(F64).sum()], F64).astype(F32) for o in out]
    return res


def bn_naive32(d, cs, inv, perm=None):
    """The same in fp32: sequential sums over the rows, every operation rounded.  inv: h and dy through the
    once-rounded 1 / std (the float4 kernels, kernels.h bn_bwd_dy_inv), else through divisions (the scalar kernels).
    perm: the order the rows are summed in (dy comes back in the stored order)."""
    if perm is not None:
        r = bn_naive32(dict(d, y=d["y"][perm], dz=d["dz"][perm]), cs, inv)
        dy = np.empty_like(r["dy"])
        dy[perm] = r["dy"]
        return dict(r, dy=dy)
    y, dz, mu, sd, w = d["y"], d["dz"], d["mean"], d["std"], F32(d["w"])
    total, c = y.shape
    isd = F32(1.0) / sd
    h = ((y - mu) * isd) if inv else ((y - mu) / sd)
    g = w * dz
    gh, dh = g * h, dz * h
    S = np.zeros((4, c), F32)
    for r in range(total):
        S[0] += g[r]
        S[1] += gh[r]
        S[2] += dh[r]
        S[3] += dz[r]
    inv_n = F32(1.0) / F32(total) if total > 0 else F32(0.0)
    m1, m2 = S[0] * inv_n, S[1] * inv_n
    if cs["training"]:
        t = (g - m1) - h * m2
        dy = t * isd if inv else t / sd
    else:
        dy = g * isd if inv else g / sd
    dy = np.where(_relu_mask(cs, y), F32(0.0), dy).astype(F32)
    return dict(sums=np.ascontiguousarray(S.T), dy=dy, dbpart=_tile_sums(dy, F32))


def check_bn_bwd(cs, d, got, report=None, env=None, ref=None):
    """got: path, sums [c][4], dy [alloc][ld], dw, db (scalars), dbpart [tiles][c] or None, acc_zero or None."""
    name = bn_case_id(cs)
    c, total, cap = cs["c"], cs["total"], cs["cap"]
    path = bn_expected_path(cs, env)
    assert got["path"] == path, (name, "path", got["path"], path)
    ref = bn_ref64(d, cs) if ref is None else ref
    exact = cs["fam"] == "E"
    naive = None if exact and not cs["training"] else bn_naive_orders(d, cs, inv=path != "scalar")
    rep = dict(report=report, width=c)
    if not cs["apply"] or path in ("part4fin", "scalar"):     # the only sequences that store the statistics
        if exact:
            check_exact(name + " sums", got["sums"], ref["sums"])
        else:
            check_bound(name + " sums", got["sums"], ref["sums"], naive["sums"], kernel=path + " sums", **rep)
    if got.get("acc_zero") is not None:
        assert not got["acc_zero"].any(), (name, "acc64_zero is not zero after the call")
    if not cs["apply"]:
        return
    for k in ("dw", "db"):
        if exact:
            check_exact(name + " " + k, np.array([got[k]], F32), np.array([ref[k]]))
        else:
            check_bound(name + " " + k, np.array([got[k]], F32), np.array([ref[k]], F64), naive[k],
                        kernel=path + " " + k, **rep)
    dy = got["dy"]
    ld = dy.shape[1]
    assert sentinel(dy[total:]), (name, "dy rows >= total written")
    if ld > c:
        assert not dy[:total, c:].any(), (name, "dy padding columns not zero")
    if exact and not cs["training"]:
        check_exact(name + " dy", dy[:total, :c], ref["dy"])
    else:
        check_bound(name + " dy", dy[:total, :c], ref["dy"], naive["dy"], kernel=path + " dy", **rep)
    if got.get("dbpart") is not None:
        t64 = -(-total // 64)
        assert sentinel(got["dbpart"][t64:]), (name, "dbpart tiles >= ceil(total / 64) written")
        if exact and not cs["training"]:
            check_exact(name + " dbpart", got["dbpart"][:t64], ref["dbpart"])
        else:
            check_bound(name + " dbpart", got["dbpart"][:t64], ref["dbpart"], naive["dbpart"],
                        kernel=path + " dbpart", **rep)
    assert cap >= total


def bn_case_id(cs):
    return "bn c{c} t{total}/{cap} {fam} tr{training} ap{apply} db{dbpart} acc{acc} relu{relu_from} ldy{ldy} mis{misalign}".format(**cs)


def bn_got_from_ref(cs, d, env=None, ref=None):
    """What a correct kernel would return, from the fp64 reference (the CPU tests perturb this)."""
    ref = bn_ref64(d, cs) if ref is None else ref
    c, total, cap = cs["c"], cs["total"], cs["cap"]
    ld = cs["ldy"] or c
    dy = np.full((cap, ld), SENT, F32)
    dy[:total, :c] = ref["dy"]
    dy[:total, c:] = 0.0
    dbp = None
    if cs["dbpart"]:
        dbp = np.full((-(-cap // 64), c), SENT, F32)
        dbp[:-(-total // 64)] = ref["dbpart"]
    return dict(path=bn_expected_path(cs, env), sums=ref["sums"].astype(F32), dy=dy, dw=F32(ref["dw"]),
                db=F32(ref["db"]), dbpart=dbp, acc_zero=np.zeros(32 * c) if cs["acc"] else None)


# ================================================================================================ BN finalize
FIN_TILES = (1, 2, 63, 64, 65, 511, 512, 513, 600)
FIN_C = (1, 3, 4, 5)
FIN_LAST = (64, 32, 1)        # rows of the last tile: powers of two, so the exact family's tile means are exact


def fin_cases():
    out = []
    for c in FIN_C:
        for i, t in enumerate(FIN_TILES):
            for fam in ("E", "R"):
                for mode in ("part", "acc"):
                    out.append(dict(c=c, tiles=t, last=FIN_LAST[i % 3] if fam == "E" else (64, 37, 1)[i % 3], fam=fam,
                                    mode=mode, run=(i + (mode == "acc")) % 2, seed=500 + 10 * i + c))
    return out


def fin_data(cs):
    g = np.random.default_rng(cs["seed"])
    c = cs["c"]
    rows = (cs["tiles"] - 1) * 64 + cs["last"] if cs["tiles"] else 0
    if cs["fam"] == "E":
        Y = (g.integers(-7, 8, (rows, c)) + g.integers(-3, 4, c)).astype(F32)
    else:
        Y = (g.standard_normal((rows, c)) + g.uniform(0.5, 3.0, c) * g.choice([-1.0, 1.0], c)).astype(F32)
    return fin_from_y(Y, g)


def fin_from_y(Y, g):
    """The (count, mean, M2) partials per 64-row tile rounded to fp32 and the fp64 sums [8][2][c] (copy = tile % 8) of
    Y, the two-pass fp64 statistics of Y, and the Chan combination in fp64 of the partials as rounded."""
    rows, c = Y.shape
    tiles = -(-rows // 64)
    Yd = Y.astype(F64)
    part = np.zeros((max(tiles, 1), c, 3), F32)
    acc = np.zeros((8, 2, c), F64)
    for t in range(tiles):
        blk = Yd[t * 64:(t + 1) * 64]
        m = blk.mean(0)
        part[t, :, 0], part[t, :, 1], part[t, :, 2] = len(blk), m, ((blk - m) ** 2).sum(0)
        acc[t % 8, 0] += blk.sum(0)
        acc[t % 8, 1] += (blk * blk).sum(0)
    if rows:
        mean = Yd.mean(0)
        var = ((Yd - mean) ** 2).mean(0)
        n, pm, pq = part[:tiles, :, 0].astype(F64), part[:tiles, :, 1].astype(F64), part[:tiles, :, 2].astype(F64)
        cmean = (n * pm).sum(0) / rows
        cvar = (pq + n * (pm - cmean) ** 2).sum(0) / rows
    else:
        mean = var = cmean = cvar = np.zeros(c)
    return dict(Y=Y, rows=rows, tiles=tiles, part=part, acc=acc, mean=mean, std=np.sqrt(1e-5 + var), cmean=cmean,
                cstd=np.sqrt(1e-5 + cvar), run_mean=g.standard_normal(c).astype(F32),
                run_std=g.uniform(0.5, 2.0, c).astype(F32))


def running_update(batch, run):
    """The three fp32 operations of k_bn_finalize: (1 - momentum) * batch + momentum * running."""
    mom = F32(0.1)
    m1 = F32(1.0) - mom
    return (m1 * batch.astype(F32)).astype(F32) + (mom * run.astype(F32)).astype(F32)


def check_fin(name, d, got, mode, exact):
    """got: mean, std (c,), and run_mean / run_std after the call or None.  1 fp32 ulp of the two-pass fp64
    statistics of Y.  The fp32-rounded partials of the random family are not those of Y but carry a rounding of their
    own, so there the reference is the fp64 (Chan) combination of the partials as given -- the operation the kernel
    is documented to do -- and the kernel's own error gets the same 1 ulp, no more."""
    for k, ck in (("mean", "cmean"), ("std", "cstd")):
        check_finite(name + " " + k, got[k])
        ref = d[k] if (exact or mode == "acc") else d[ck]
        ulp = np.spacing(np.abs(ref).astype(F32)).astype(F64)
        err = np.abs(got[k].astype(F64) - ref)
        assert (err <= ulp).all(), (name, k, float(err.max()), float(ulp.min()))
    assert (got["std"] >= F32(np.sqrt(1e-5))).all(), (name, "std below sqrt(1e-5): a negative variance")
    if got.get("run_mean") is not None:
        for k in ("mean", "std"):
            want = running_update(got[k], d["run_" + k])
            assert np.array_equal(got["run_" + k].view(np.int32), want.view(np.int32)), (name, "run_" + k)


# ================================================================================================ readout
RO_NB = (0, 1, 7, 8, 9, 17)
RO_NMAX = 17
RO_K = (1, 63, 64, 65, 1024, 1025, 1300)
RO_DIM_OUT = (1, 3)
RO_BS = (1, 15, 16, 17, 33)
RO_PARAM_K = (1, 65, 1025)


def ro_data(k, dim_out, fam, seed, nbs=RO_NB):
    g = np.random.default_rng(seed)
    nb = np.asarray(nbs)
    off = np.concatenate([[0], np.cumsum(nb)]).astype(np.int32)
    rows, bs = int(off[-1]), len(nb)
    if fam == "E":
        A = g.integers(-7, 8, (rows, k)).astype(F32)
        fcw = g.integers(-3, 4, (dim_out, k)).astype(F32)
        fcb = g.integers(-3, 4, dim_out).astype(F32)
        dout = g.integers(-3, 4, (bs, dim_out)).astype(F32)
    else:
        A = (g.standard_normal((rows, k)) + g.uniform(0.5, 1.5, k)).astype(F32)
        fcw = g.standard_normal((dim_out, k)).astype(F32)
        fcb = g.standard_normal(dim_out).astype(F32)
        dout = g.standard_normal((bs, dim_out)).astype(F32)
    return dict(A=A, fcw=fcw, fcb=fcb, dout=dout, off=off, bs=bs, k=k, dim_out=dim_out, nmax=RO_NMAX, fam=fam)


def ro_ref(d, dtype):
    """colsum (bs, k), out (bs, dim_out), da [rows][k] = R_b = dout[b] . fcw; fp32: sequential, each operation
    rounded."""
    A, fcw, fcb, dout = (d[x].astype(dtype) for x in ("A", "fcw", "fcb", "dout"))
    bs, k, o = d["bs"], d["k"], d["dim_out"]
    cs = np.zeros((bs, k), dtype)
    out = np.zeros((bs, o), dtype)
    R = np.zeros((bs, k), dtype)
    for b in range(bs):
        for r in range(d["off"][b], d["off"][b + 1]):
            cs[b] = cs[b] + A[r]
        for j in range(o):
            R[b] = R[b] + dout[b, j] * fcw[j]
    if dtype == F64:
        out = cs @ fcw.T
    else:
        prod = cs[:, None, :] * fcw[None]
        for kk in range(k):
            out = out + prod[:, :, kk]
    out = out + dtype(d["nmax"]) * fcb
    da = np.repeat(R, np.diff(d["off"]), axis=0)
    return dict(colsum=cs, out=out, da=da, R=R)


def check_ro_fwd(name, d, got, report=None):
    ref = ro_ref(d, F64)
    if d["fam"] == "E":
        check_exact(name + " colsum", got["colsum"], ref["colsum"])
        check_exact(name + " out", got["out"], ref["out"])
    else:
        check_ulp(name + " colsum", got["colsum"], ref["colsum"])
        check_bound(name + " out", got["out"], ref["out"], ro_ref(d, F32)["out"], report, "readout_fwd out", d["k"])


def check_ro_da(name, d, got, report=None):
    ref = ro_ref(d, F64)
    rows = int(d["off"][-1])
    assert sentinel(got[rows:]), (name, "da rows >= total written")
    if d["fam"] == "E" or d["dim_out"] == 1:
        check_exact(name + " da", got[:rows], ref["da"])
    else:
        check_bound(name + " da", got[:rows], ref["da"], ro_ref(d, F32)["da"], report, "readout_bwd_da", d["k"])


def ro_param_data(bs, k, dim_out, fam, seed):
    g = np.random.default_rng(seed)
    if fam == "E":
        return dict(dout=g.integers(-3, 4, (bs, dim_out)).astype(F32), colsum=g.integers(-99, 100, (bs, k)).astype(F32),
                    bs=bs, k=k, dim_out=dim_out, nmax=RO_NMAX, fam=fam)
    return dict(dout=g.standard_normal((bs, dim_out)).astype(F32),
                colsum=(3 * g.standard_normal((bs, k)) + 1).astype(F32), bs=bs, k=k, dim_out=dim_out, nmax=RO_NMAX,
                fam=fam)


def check_ro_params(name, d, got):
    """dfcw[o, k] = sum_b dout[b, o] colsum[b, k], dfcb[o] = nmax sum_b dout[b, o]: fp64 sums rounded once."""
    dfcw = d["dout"].astype(F64).T @ d["colsum"].astype(F64)
    dfcb = d["nmax"] * d["dout"].astype(F64).sum(0)
    assert sentinel(got["dfcw"][d["dim_out"]:]) and sentinel(got["dfcb"][d["dim_out"]:]), (name, "written past the end")
    f = check_exact if d["fam"] == "E" else check_ulp
    f(name + " dfcw", got["dfcw"][:d["dim_out"]], dfcw)
    f(name + " dfcb", got["dfcb"][:d["dim_out"]], dfcb)


# ------------------------------------------------------------------------------------------------ readout-row gathers
AGG_C = (5, 64, 260, 512)
AGG_JT = (2, 3, 4, 5, 7)          # 8 and 9: HGNN_ERR_UNSUPPORTED (an entry of 8 floats holds 7 coefficients)
AGG_COUNTS = (0, 3, 4, 5, 9)
AGG_EDGE_ROWS = 300               # one graph's edge rows: more than the block's 256 threads


def make_list(g, fam, counts, nc, stride):
    """rows [R][2] (start, count) and entries [slots][stride]: [column bits, v_0 .. v_{nc-1}, NaN padding]; one unused
    slot (column 0, NaN) after every row; vals[r] the row's coefficients [count][nc]."""
    assert 1 + nc <= stride
    n = int(sum(counts)) + len(counts) + 4
    ent = np.full((n, stride), NAN, F32)
    ent[:, 0] = 0.0
    rows = np.zeros((max(len(counts), 1), 2), np.int32)
    vals, s = [], 0
    for r, k in enumerate(counts):
        v = (g.integers(-8, 9, (k, nc)) / 4.0).astype(F32) if fam == "E" else g.standard_normal((k, nc)).astype(F32)
        rows[r] = (s, k)
        ent[s:s + k, 0] = np.arange(k, dtype=np.int32).view(F32)
        ent[s:s + k, 1:1 + nc] = v
        vals.append(v)
        s += k + 1
    return dict(rows=rows, ent=ent, vals=vals, nc=nc, stride=stride)


def agg_cases(C):
    out = []
    for i, jt in enumerate(AGG_JT):
        strides = (4, 8) if jt <= 3 else (8,)
        for stride in strides:
            for fam in ("E", "R"):
                out.append(dict(C=C, jt=jt, stride=stride, fam=fam, g=1, p=1, g_acc=i % 2, p_acc=(i + 1) % 2, mis=0,
                                lds=0, seed=3000 + 10 * jt + stride + C))
    out.append(dict(C=C, jt=3, stride=4, fam="E", g=1, p=0, g_acc=1, p_acc=0, mis=0, lds=0, seed=3100 + C))
    out.append(dict(C=C, jt=4, stride=8, fam="E", g=0, p=1, g_acc=0, p_acc=1, mis=0, lds=0, seed=3101 + C))
    out.append(dict(C=C, jt=3, stride=4, fam="E", g=0, p=0, g_acc=0, p_acc=0, mis=0, lds=0, seed=3102 + C))
    out.append(dict(C=C, jt=5, stride=8, fam="R", g=1, p=1, g_acc=1, p_acc=1, mis=1, lds=0, seed=3103 + C))
    if C == 512:   # dynamic LDS between 64 KB and 160 KB (the opt-in), and past 160 KB (refused)
        out.append(dict(C=C, jt=7, stride=8, fam="E", g=1, p=1, g_acc=0, p_acc=0, mis=0, lds=1, seed=3104))
        out.append(dict(C=C, jt=7, stride=8, fam="E", g=1, p=1, g_acc=0, p_acc=0, mis=0, lds=2, seed=3105))
    return out


def agg_lds_bytes(cs, d):
    """bn.hip readout_agg_bwd_lds."""
    bs = d["bs"]
    maxrows = -(-d["p_cap"] // bs) if cs["p"] else 0
    grow = -(-d["g_cap"] // bs)
    return 4 * max(cs["jt"] * cs["C"] + grow * cs["jt"], 2 * cs["C"] + maxrows * 2)


def agg_data(cs):
    g = np.random.default_rng(cs["seed"])
    C, jt, fam = cs["C"], cs["jt"], cs["fam"]
    nb = np.array([0, 1, 9, 17, 5])
    eb = np.array([0, 1, 30, AGG_EDGE_ROWS, 7])
    bs = len(nb)
    noff = np.concatenate([[0], np.cumsum(nb)]).astype(np.int32)
    eoff = np.concatenate([[0], np.cumsum(eb)]).astype(np.int32)
    cnt = lambda n: [AGG_COUNTS[i % len(AGG_COUNTS)] for i in range(n)]
    gl = make_list(g, fam, cnt(int(noff[-1])), jt, cs["stride"])
    pl = make_list(g, fam, cnt(int(eoff[-1])), 2, 4)
    k, dim_out = jt * C + 2 * C, 3
    if fam == "E":
        dout = g.integers(-3, 4, (bs, dim_out)).astype(F32)
        fcw = g.integers(-3, 4, (dim_out, k)).astype(F32)
        g0 = g.integers(-7, 8, (int(noff[-1]), C)).astype(F32)
        p0 = g.integers(-7, 8, (int(eoff[-1]), C)).astype(F32)
    else:
        dout = g.standard_normal((bs, dim_out)).astype(F32)
        fcw = g.standard_normal((dim_out, k)).astype(F32)
        g0 = g.standard_normal((int(noff[-1]), C)).astype(F32)
        p0 = g.standard_normal((int(eoff[-1]), C)).astype(F32)
    g_cap = bs * (17, 2000, 6000)[cs["lds"]]
    return dict(gl=gl, pl=pl, dout=dout, fcw=fcw, g0=g0, p0=p0, noff=noff, eoff=eoff, bs=bs, k=k, dim_out=dim_out,
                g_cap=g_cap, p_cap=bs * AGG_EDGE_ROWS)


def agg_ref(cs, d, kind, dtype, drop_last=False, shift=0):
    """kind "g": out[r, c] (+)= sum_j (sum_e v_j(e)) R_b[j C + c]; "p": (sum pm) R_b[jt C + c] + (sum pd)
    R_b[jt C + C + c].  fp32: entries summed in order, then fused over j as the kernel's fmaf chain is not -- each
    product and sum rounded."""
    C, jt = cs["C"], cs["jt"]
    l, off, old, acc = (d["gl"], d["noff"], d["g0"], cs["g_acc"]) if kind == "g" else (d["pl"], d["eoff"], d["p0"],
                                                                                    cs["p_acc"])
    ns, kb = (jt, 0) if kind == "g" else (2, jt * C)
    dout, fcw = d["dout"].astype(dtype), d["fcw"].astype(dtype)
    out = np.zeros(old.shape, dtype)
    for b in range(d["bs"]):
        R = np.zeros(d["k"], dtype)
        for o in range(d["dim_out"]):
            R = R + dout[b, o] * fcw[o]
        R = np.roll(R, shift)
        for r in range(off[b], off[b + 1]):
            v = l["vals"][r].astype(dtype)
            if drop_last and len(v) == 9:
                v = v[:-1]
            cs_ = np.zeros(ns, dtype)
            for e in range(len(v)):
                cs_ = cs_ + v[e]
            row = old[r].astype(dtype) if acc else np.zeros(C, dtype)
            for j in range(ns):
                row = row + cs_[j] * R[kb + j * C:kb + (j + 1) * C]
            out[r] = row
    return out


def check_agg(name, cs, d, got_g, got_p, report=None):
    for kind, got, on in (("g", got_g, cs["g"]), ("p", got_p, cs["p"])):
        old = d[kind + "0"]
        rows = len(old)
        if not on:
            continue
        assert sentinel(got[rows:]), (name, kind, "rows past the total written")
        ref = agg_ref(cs, d, kind, F64)
        if cs["fam"] == "E":
            check_exact(name + " " + kind, got[:rows], ref)
        else:
            check_bound(name + " " + kind, got[:rows], ref, agg_ref(cs, d, kind, F32), report,
                        "readout_agg_bwd " + kind, cs["C"])


# ================================================================================================ dense dW
DW_F = (1, 4, 5, 16, 17, 64, 65, 128, 130)
DW_NMAX = (5, 32, 33, 64, 65, 100)
DW_JT = (2, 3, 4)


def dw_cases():
    """(F, nmax, jt, bs) with the other options cycled.  bs >= 256 leaves the items of a graph in one block (MAXI 3
    / 5); fewer graphs split them over gridDim.y with MAXI 1.  jt = 5 at nmax <= 32 is the one way to MAXI 3 at
    FC 128 / 64 (the items of a 32-node graph are its slices)."""
    shapes = [
        (1, 5, 2, 3), (4, 5, 3, 3), (5, 32, 4, 3), (16, 33, 2, 1), (17, 5, 3, 3), (64, 32, 4, 3), (65, 32, 2, 3),
        (128, 32, 3, 1), (130, 5, 4, 3), (17, 33, 3, 3), (64, 64, 2, 1), (65, 64, 4, 3), (130, 65, 2, 1),
        (16, 100, 3, 1), (128, 100, 2, 1), (4, 64, 4, 3), (5, 65, 2, 3),
        (4, 5, 2, 260), (4, 5, 4, 260), (17, 33, 2, 260), (20, 40, 4, 256), (17, 65, 2, 256), (65, 5, 5, 256),
        (20, 20, 5, 256), (17, 100, 3, 256),
    ]
    out = []
    for i, (F, nmax, jt, bs) in enumerate(shapes):
        big = bs >= 256 and nmax > 40
        for v in range(1 if big else 4):
            # v: 0 packed input, 1 packed + producer BN, 2 dense layer input (every other shape with BN pointers, which a
            # dense input ignores: it is read as stored), 3 readout mode (dout, BN)
            fam = "E" if big else ("E", "R")[(i + v) % 2]
            out.append(dict(F=F, nmax=nmax, jt=jt, bs=bs, fam=fam, bn=int(v in (1, 3) or (v == 2 and i % 2)),
                            xdense=int(v == 2),
                            dout=int(v == 3), acc=(i + v) % 2, ldx=(0, 4, 3)[(i + v) % 3], seed=9000 + 10 * i + v))
    return out


def dw_kernel(cs, env=None):
    """The kernel launch_dw_dense takes (csrc/dwdense.hip): ("narrow",) or ("dense", FC, MAXI, gy)."""
    F, nmax, jt, bs = cs["F"], cs["nmax"], cs["jt"], cs["bs"]
    narrow = (env or {}).get("HGNN_DW_NARROW") != "0"
    if narrow and F <= 16 and not cs["dout"] and 4 * nmax * (jt * F + F) <= 64 * 1024:
        return ("narrow",)
    npad = (nmax + 31) // 32 * 32
    fc = (128 if F > 64 else 64) if npad <= 32 else (32 if npad <= 64 else 16)
    lds = lambda c: 4 * (npad * ((jt * c + 1) + (c + 1)) + jt * c + 3 * c)
    if lds(fc) > 160 * 1024:
        fc = 8
    nitems = (npad // 32) ** 2 * jt
    maxi, gy = -(-nitems // 4), 1
    if bs < 256 and nitems > 4:
        maxi, gy = 1, -(-nitems // 4)
    return ("dense", fc, 1 if maxi <= 1 else (3 if maxi <= 3 else 5), gy)


def dw_readout_lds_bytes(cs):
    """bn.hip dw_readout_lds: R_b [jt F], X [nmax][F + 1], u [nmax jt]."""
    return 4 * (cs["jt"] * cs["F"] + cs["nmax"] * (cs["F"] + 1) + cs["nmax"] * cs["jt"])


def dw_data(cs):
    g = np.random.default_rng(cs["seed"])
    F, nmax, jt, bs, fam = cs["F"], cs["nmax"], cs["jt"], cs["bs"], cs["fam"]
    nb = np.array([(0, 1, nmax, nmax // 2 + 1)[i % 4] for i in range(bs)])
    if bs == 1:
        nb = np.array([nmax - 1 if nmax > 1 else 1])
    off = np.concatenate([[0], np.cumsum(nb)]).astype(np.int32)
    rows = int(off[-1])
    dim_out, kfc = 3, jt * F + 6
    ints = lambda lo, hi, shape: g.integers(lo, hi + 1, shape).astype(F32)
    nrm = lambda shape: g.standard_normal(shape).astype(F32)
    E = fam == "E"
    d = dict(off=off, rows=rows, dim_out=dim_out, kfc=kfc)
    d["G"] = ints(-7, 7, (rows, jt * F)) if E else nrm((rows, jt * F))
    d["xp"] = ints(-7, 7, (rows, F)) if E else nrm((rows, F))
    d["xdense"] = ints(-7, 7, (bs, F, nmax)) if E else nrm((bs, F, nmax))
    d["dout"] = ints(-3, 3, (bs, dim_out)) if E else nrm((bs, dim_out))
    d["fcw"] = ints(-3, 3, (dim_out, kfc)) if E else nrm((dim_out, kfc))
    d["old"] = ints(-7, 7, (bs, nmax, nmax, jt)) if E else nrm((bs, nmax, nmax, jt))
    if E:
        d["bn"] = dict(mean=ints(-3, 3, F), std=g.choice(np.array([0.5, 1.0, 2.0, 4.0], F32), F),
                       w=F32(g.choice([-2.0, -1.0, 1.0, 2.0])), b=F32(g.integers(-3, 4)))
    else:
        d["bn"] = dict(mean=nrm(F), std=g.uniform(0.5, 2.0, F).astype(F32), w=F32(1.3), b=F32(-0.4))
    return d


def dw_ref(cs, d, dtype, shift=0, zero_rows=False):
    """dW[b, n, m, j] (+)= sum_f G[b, n, j F + f] X[b, m, f]: G the gradient rows (R_b at padded n in readout mode,
    else 0), X the input rows (the BN of 0 at padded m with a producer BN, else 0; the dense input as stored).  fp32:
    BN as (y - mean) * (w / std) + b with the scale rounded once (kernels.h bn_z_s), f summed in order."""
    F, nmax, jt, bs = cs["F"], cs["nmax"], cs["jt"], cs["bs"]
    off = d["off"]
    bn = d["bn"] if cs["bn"] and not cs["xdense"] else None
    Gd = np.zeros((bs, nmax, jt * F), dtype)
    X = np.zeros((bs, nmax, F), dtype)
    z = lambda y: (y.astype(dtype) - bn["mean"].astype(dtype)) * (dtype(bn["w"]) / bn["std"].astype(dtype)) + dtype(bn["b"])
    for b in range(bs):
        n = off[b + 1] - off[b]
        Gd[b, :n] = d["G"][off[b]:off[b + 1]]
        if cs["dout"]:   # readout mode: the gradient of every position, real or padded, is R_b
            R = np.zeros(d["kfc"], dtype)
            for o in range(d["dim_out"]):
                R = R + d["dout"][b, o].astype(dtype) * d["fcw"][o].astype(dtype)
            Gd[b, :] = np.roll(R, shift)[:jt * F]
        if cs["xdense"]:
            X[b] = d["xdense"][b].T
        else:
            X[b, :n] = z(d["xp"][off[b]:off[b + 1]]) if bn else d["xp"][off[b]:off[b + 1]]
            if bn:
                X[b, n:] = z(np.zeros(F, F32))
    G4 = Gd.reshape(bs, nmax, jt, F)
    if dtype == F64:
        dW = np.einsum("bnjf,bmf->bnmj", G4, X)
    else:
        dW = np.zeros((bs, nmax, nmax, jt), F32)
        for f in range(F):
            dW = dW + G4[:, :, None, :, f] * X[:, None, :, None, f]
    if zero_rows:
        dW[:, 1:] = 0
    if cs["acc"]:
        dW = d["old"].astype(dtype) + dW
    return dW


def dw_case_id(cs):
    return "dw F{F} n{nmax} j{jt} bs{bs} {fam} bn{bn} xd{xdense} ro{dout} acc{acc} ldx{ldx}".format(**cs)


def check_dw(name, cs, d, got, report=None, kernel=None):
    bs = cs["bs"]
    assert sentinel(got[bs:]), (name, "dW of a graph outside the launch written")
    ref = dw_ref(cs, d, F64)
    if cs["fam"] == "E":
        check_exact(name, got[:bs], ref)
    else:
        check_bound(name, got[:bs], ref, dw_ref(cs, d, F32), report, kernel or "dw_dense", cs["F"])


# ================================================================================================ GPU runners
def _L():
    from hgnn_amd import _lib as L
    return L


def _dev():
    return torch.device("cuda", 0)


def _up(a):
    return None if a is None else _t(a).to(_dev())


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return _L().stream_handle(_dev())


def _full(shape, v, dtype=torch.float32):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), v, dtype=dtype, device=_dev())


def _padded(x, rows):
    """x's rows followed by NaN rows up to `rows`."""
    out = np.full((max(rows, 1),) + x.shape[1:], NAN, F32)
    out[:len(x)] = x
    return _up(out)


def call_bn_bwd(cs, d, acc=None, acc_zero=None):
    """One hgnn_probe_bn_backward call.  y / dz hold NaN in rows [total, alloc); part and sums NaN on entry; dy, dw,
    db, dbpart SENT.  acc / acc_zero: device fp64 regions (ping-pong test); by default a zeroed region and one
    filled with 7.0 when the case has acc."""
    L = _L()
    c, total, cap = cs["c"], cs["total"], cs["cap"]
    alloc = cs.get("alloc", cap)
    ld = cs["ldy"] or c
    tiles = -(-cap // 64)
    y, dz = _padded(d["y"], alloc), _padded(d["dz"], alloc)
    dybuf = _full(max(alloc, 1) * ld + 4, SENT)
    dyv = dybuf[1:] if cs["misalign"] else dybuf
    part, sums = _full(4 * c * max(tiles, 1), NAN), _full(4 * c, NAN)
    dw, db = _full(1, SENT), _full(1, SENT)
    dbp = _full((max(tiles, 1), c), SENT) if cs["dbpart"] else None
    if cs["acc"] and acc is None:
        acc, acc_zero = _full(32 * c, 0.0, torch.float64), _full(32 * c, 7.0, torch.float64)
    tot = _up(np.array([total], np.int32))
    mean, std, w = _up(d["mean"]), _up(d["std"]), _up(np.array([d["w"]], F32))
    a = L.ProbeBnBackward()
    a.y, a.dz, a.total_rows, a.mean, a.std, a.w = _p(y), _p(dz), _p(tot), _p(mean), _p(std), _p(w)
    a.part, a.sums, a.dy, a.dw, a.db, a.dbpart = _p(part), _p(sums), _p(dyv), _p(dw), _p(db), _p(dbp)
    a.acc64, a.acc64_zero = _p(acc), _p(acc_zero)
    a.cap_rows, a.c, a.relu_from, a.training, a.ldy, a.apply = cap, c, cs["relu_from"], cs["training"], cs["ldy"], cs["apply"]
    a.path = -1
    st = L.lib().hgnn_probe_bn_backward(ctypes.byref(a), _stream())
    torch.cuda.synchronize()
    assert st == 0, (bn_case_id(cs), "status", st)
    return dict(path=PATHS[a.path], sums=sums.cpu().numpy().reshape(c, 4),
                dy=dyv[:max(alloc, 1) * ld].cpu().numpy().reshape(max(alloc, 1), ld)[:alloc],
                dw=dw.cpu().numpy()[0], db=db.cpu().numpy()[0], dbpart=None if dbp is None else dbp.cpu().numpy()[:tiles],
                acc_zero=None if acc_zero is None else acc_zero.cpu().numpy(), head=dybuf[:1].cpu().numpy())


def run_bn_case(cs, report=None, env=None):
    d = bn_data(cs)
    got = call_bn_bwd(cs, d)
    check_bn_bwd(cs, d, got, report, env)
    if cs["misalign"]:
        assert sentinel(got["head"]), "the float before a 4-byte-offset dy written"
    return got


def run_bn_cases(widths, env=None, report=None):
    n = 0
    for cs in bn_cases(widths):
        run_bn_case(cs, report, env)
        n += 1
    return n


def call_fin(cs, d, training=1, with_run=True):
    L = _L()
    c, mode = cs["c"], cs["mode"]
    tiles = d["tiles"]
    part = np.full((tiles + 2, c, 3), NAN, F32)
    part[:tiles] = d["part"][:tiles]
    tp, ta = (_up(part), None) if mode == "part" else (None, _up(d["acc"]))
    mean, std = _full(c + 3, SENT), _full(c + 3, SENT)
    rm, rs = (_up(d["run_mean"]), _up(d["run_std"])) if with_run else (None, None)
    cnt = _up(np.array([d["rows"]], np.int32))
    a = L.ProbeBnFinalize()
    a.acc, a.part, a.count, a.mean, a.std, a.run_mean, a.run_std = _p(ta), _p(tp), _p(cnt), _p(mean), _p(std), _p(rm), _p(rs)
    a.tiles, a.c, a.training = tiles, c, training
    st = L.lib().hgnn_probe_bn_finalize(ctypes.byref(a), _stream())
    torch.cuda.synchronize()
    assert st == 0, ("finalize status", st)
    mean, std = mean.cpu().numpy(), std.cpu().numpy()
    assert sentinel(mean[c:]) and sentinel(std[c:]), "finalize wrote past channel c"
    return dict(mean=mean[:c], std=std[:c], run_mean=None if rm is None else rm.cpu().numpy(),
                run_std=None if rs is None else rs.cpu().numpy())


def call_ro_fwd(d):
    L = _L()
    rows = int(d["off"][-1])
    A = _padded(d["A"], rows + 9)
    off, fcw, fcb = _up(d["off"]), _up(d["fcw"]), _up(d["fcb"])
    cs, out = _full((d["bs"] + 1, d["k"]), SENT), _full((d["bs"] + 1, d["dim_out"]), SENT)
    st = L.lib().hgnn_probe_readout_fwd(_p(A), d["k"], _p(off), d["bs"], d["nmax"], _p(fcw), _p(fcb), d["dim_out"],
                                        _p(cs), _p(out), _stream())
    torch.cuda.synchronize()
    assert st == 0
    cs, out = cs.cpu().numpy(), out.cpu().numpy()
    assert sentinel(cs[d["bs"]:]) and sentinel(out[d["bs"]:]), "readout_fwd wrote past the batch"
    return dict(colsum=cs[:d["bs"]], out=out[:d["bs"]])


def call_ro_da(d):
    L = _L()
    rows = int(d["off"][-1])
    da = _full((rows + 9, d["k"]), SENT)
    off, fcw, dout, tot = _up(d["off"]), _up(d["fcw"]), _up(d["dout"]), _up(np.array([rows], np.int32))
    st = L.lib().hgnn_probe_readout_bwd_da(_p(dout), _p(off), d["bs"], rows + 9, _p(tot), _p(fcw), d["dim_out"], d["k"],
                                           _p(da), _stream())
    torch.cuda.synchronize()
    assert st == 0
    return da.cpu().numpy()


def call_ro_params(d):
    L = _L()
    o, k = d["dim_out"], d["k"]
    nbytes = L.lib().hgnn_probe_readout_bwd_scratch_bytes(o, k)
    assert nbytes == 8 * 16 * o * (k + 1)
    scratch = _full(nbytes // 8, NAN, torch.float64)
    dfcw, dfcb = _full((o + 1, k), SENT), _full(o + 1, SENT)
    dout, cs = _up(d["dout"]), _up(d["colsum"])
    st = L.lib().hgnn_probe_readout_bwd_params(_p(dout), _p(cs), d["bs"], d["nmax"], o, k, _p(dfcw), _p(dfcb),
                                               _p(scratch), _stream())
    torch.cuda.synchronize()
    assert st == 0
    return dict(dfcw=dfcw.cpu().numpy(), dfcb=dfcb.cpu().numpy())


def agg_struct(cs, d, keep, overrides=None):
    """The probe arguments of an agg case and its two output tensors (SENT rows behind the totals; the old values
    in front, read when the launch accumulates)."""
    L = _L()
    C = cs["C"]

    def outbuf(old):
        buf = _full((len(old) + 3) * C + 4, SENT)
        v = buf[1:] if cs["mis"] else buf
        v[:old.size] = _up(old).reshape(-1)
        return buf, v
    gb, gv = outbuf(d["g0"])
    pb, pv = outbuf(d["p0"])
    ts = dict(dout=_up(d["dout"]), fcw=_up(d["fcw"]), noff=_up(d["noff"]), eoff=_up(d["eoff"]),
              gr=_up(d["gl"]["rows"]), ge=_up(d["gl"]["ent"]), pr=_up(d["pl"]["rows"]), pe=_up(d["pl"]["ent"]),
              gt=_up(d["noff"][-1:]), pt=_up(d["eoff"][-1:]))
    keep += list(ts.values()) + [gb, pb]
    a = L.ProbeReadoutAgg()
    a.dout, a.fcw, a.node_off, a.edge_off = _p(ts["dout"]), _p(ts["fcw"]), _p(ts["noff"]), _p(ts["eoff"])
    a.g.rows, a.g.entries, a.g.stride = _p(ts["gr"]), _p(ts["ge"]), d["gl"]["stride"]
    a.p.rows, a.p.entries, a.p.stride = _p(ts["pr"]), _p(ts["pe"]), 4
    a.g_total, a.p_total = _p(ts["gt"]), _p(ts["pt"])
    a.g_out = _p(gv) if cs["g"] else None
    a.p_out = _p(pv) if cs["p"] else None
    a.dim_out, a.k, a.jt, a.cg, a.cp, a.bs = d["dim_out"], d["k"], cs["jt"], C, C, d["bs"]
    a.g_cap, a.g_acc, a.p_cap, a.p_acc = d["g_cap"], cs["g_acc"], d["p_cap"], cs["p_acc"]
    for k, v in (overrides or {}).items():
        setattr(a, k, v)
    return a, gv, pv


def call_agg(cs, d, overrides=None):
    L = _L()
    keep = []
    a, gv, pv = agg_struct(cs, d, keep, overrides)
    C = cs["C"]
    fits = L.lib().hgnn_probe_readout_row_fits(ctypes.byref(a), None)
    st = L.lib().hgnn_probe_readout_agg_bwd(ctypes.byref(a), _stream())
    torch.cuda.synchronize()
    if cs["mis"]:      # the float in front of a 4-byte-offset output (keep ends with the two whole buffers)
        assert sentinel(keep[-2][:1].cpu().numpy()) and sentinel(keep[-1][:1].cpu().numpy()), \
            "the float before a 4-byte-offset g_out / p_out written"
    rows = lambda v, old: v[:(len(old) + 3) * C].cpu().numpy().reshape(len(old) + 3, C)
    return st, fits, rows(gv, d["g0"]), rows(pv, d["p0"])


def run_agg_case(cs, report=None):
    d = agg_data(cs)
    name = "agg C{C} j{jt} s{stride} {fam} g{g} p{p} acc{g_acc}{p_acc} mis{mis} lds{lds}".format(**cs)
    st, fits, gg, gp = call_agg(cs, d)
    lds = agg_lds_bytes(cs, d)
    if cs["g"] or cs["p"]:
        assert fits == int(lds <= 160 * 1024), (name, "readout_row_fits", fits, lds)
    if cs["lds"] == 1:
        assert 64 * 1024 < lds <= 160 * 1024, lds
    if cs["lds"] == 2:
        assert lds > 160 * 1024 and st == ERR_UNSUPPORTED, (name, st, lds)
    else:
        assert st == 0, (name, "status", st)
        check_agg(name, cs, d, gg, gp, report)
    # what the launch does not gather keeps its contents
    for on, got, old in ((cs["g"] and cs["lds"] != 2, gg, d["g0"]), (cs["p"] and cs["lds"] != 2, gp, d["p0"])):
        if not on:
            assert np.array_equal(got[:len(old)].view(np.int32), old.view(np.int32)) and sentinel(got[len(old):]), name


def dw_struct(cs, d, keep, G=None, lda=None, dW=None):
    L = _L()
    F, nmax, jt, bs = cs["F"], cs["nmax"], cs["jt"], cs["bs"]
    G = d["G"] if G is None else G
    lda = (G.shape[1] + cs["ldx"]) if lda is None else lda
    Gp = np.full((d["rows"] + 5, max(lda, G.shape[1])), NAN, F32)
    Gp[:d["rows"], :G.shape[1]] = G
    if dW is None:
        dW = _full((bs + 1, nmax, nmax, jt), SENT)
        if cs["acc"]:
            dW[:bs] = _up(d["old"])
    ts = dict(G=_up(Gp), off=_up(d["off"]), dW=dW)
    a = L.ProbeDwDense()
    if cs["xdense"]:
        ts["xd"] = _up(d["xdense"])
        a.xdense = _p(ts["xd"])
    else:
        ts["xp"] = _padded(d["xp"], d["rows"] + 5)
        a.xp = _p(ts["xp"])
    if cs["bn"]:
        bn = d["bn"]
        ts.update(m=_up(bn["mean"]), s=_up(bn["std"]), w=_up(np.array([bn["w"]], F32)), b=_up(np.array([bn["b"]], F32)))
        a.pmean, a.pstd, a.pw, a.pb = _p(ts["m"]), _p(ts["s"]), _p(ts["w"]), _p(ts["b"])
    if cs["dout"]:
        ts.update(dout=_up(d["dout"]), fcw=_up(d["fcw"]))
        a.dout, a.fcw, a.dim_out, a.kfc = _p(ts["dout"]), _p(ts["fcw"]), d["dim_out"], d["kfc"]
    a.dA, a.lda, a.node_off, a.dW = _p(ts["G"]), lda, _p(ts["off"]), _p(dW)
    a.f, a.jt, a.bs, a.nmax, a.accumulate = F, jt, bs, nmax, cs["acc"]
    keep += list(ts.values())
    return a, dW


def call_dw(cs, d, readout=False, G=None, lda=None):
    L = _L()
    keep = []
    a, dW = dw_struct(cs, d, keep, G, lda)
    f = L.lib().hgnn_probe_dw_readout if readout else L.lib().hgnn_probe_dw_dense
    st = f(ctypes.byref(a), _stream())
    torch.cuda.synchronize()
    return st, dW.cpu().numpy()


def run_dw_case(cs, report=None, env=None):
    """launch_dw_dense on the case; in readout mode (F <= 130) also k_dw_readout and launch_dw_dense fed the
    materialised readout gradient: the three must agree (exact family: bit for bit; random: each on the bound)."""
    d = dw_data(cs)
    name = dw_case_id(cs)
    kern = "/".join(str(x) for x in dw_kernel(cs, env)[:3])
    if not cs["dout"]:
        st, got = call_dw(cs, d)
        assert st == 0, (name, "status", st)
        check_dw(name, cs, d, got, report, "dw_dense " + kern)
    else:
        # readout mode: the real rows carry the materialised launch_readout_bwd_da gradient (R_b, as the padded do)
        da = call_ro_da(ro_like(cs, d))[:d["rows"]]
        st, got2 = call_dw(cs, d, G=da, lda=d["kfc"])
        assert st == 0, (name, "status", st)
        check_dw(name + " (materialised)", cs, d, got2, report, "dw_dense " + kern)
        st, got3 = call_dw(cs, d, readout=True)
        assert st == 0, (name, "dw_readout status", st)
        check_dw(name + " (k_dw_readout)", cs, d, got3, report, "dw_readout")
        if cs["fam"] == "E":
            assert np.array_equal(got2.view(np.int32), got3.view(np.int32)), (name, "dw_readout != dw_dense")
    return 1


def ro_like(cs, d):
    return dict(off=d["off"], bs=cs["bs"], k=d["kfc"], dim_out=d["dim_out"], dout=d["dout"], fcw=d["fcw"])


def run_dw_cases(env=None, only=None, report=None):
    n = 0
    for cs in dw_cases():
        if only is None or only(cs):
            n += run_dw_case(cs, report, env)
    return n


# the child-process groups of test_switch_selected_variants: (environment, worker mode).  HGNN_BN_ACC is read by the
# executor alone (it then passes no acc64, the tables' acc = 0 cases): its group shows the launchers do not read it.
# HGNN_READOUT_ROW likewise never reaches a launcher and has no group.
SWITCH_GROUPS = {
    "bn_bwd2=0": (dict(HGNN_BN_BWD2="0"), "bn_narrow_wide"),
    "bn_bwd2=1": (dict(HGNN_BN_BWD2="1"), "bn_narrow_wide"),
    "bn_acc=0": (dict(HGNN_BN_ACC="0"), "bn_narrow"),
    "dw_narrow=0": (dict(HGNN_DW_NARROW="0"), "dw_narrow"),
    "dwd_grid=0": (dict(HGNN_DWD_GRID="0"), "dw_many"),
    "dwd_grid=3": (dict(HGNN_DWD_GRID="3"), "dw_many"),
}


def run_worker_mode(mode, env):
    if mode == "bn_narrow_wide":
        return run_bn_cases(NARROW_C + WIDE_C, env)
    if mode == "bn_narrow":
        return run_bn_cases(NARROW_C, env)
    if mode == "dw_narrow":
        return run_dw_cases(env, lambda cs: cs["F"] <= 16 and not cs["dout"])
    if mode == "dw_many":
        return run_dw_cases(env, lambda cs: cs["bs"] >= 256 and cs["nmax"] <= 40)
    raise ValueError(mode)
