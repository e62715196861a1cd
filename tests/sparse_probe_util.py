"""Inputs, references, case tables and runners of the sparse-side kernel probes (include/hgnn_amd.h, "Kernel
probes"; csrc/probe_sparse.hip): shared by tests/test_sparse_probe_inputs.py (CPU: the inputs and the checks have the
properties the GPU tests rely on), tests/test_gpu_sparse_kernels.py and its child-process worker
tests/sparse_probe_worker.py.  The counterpart of tests/gemm_probe_util.py for csrc/struct.hip and csrc/agg.hip.

Row lists (csrc/kernels.h StructView): rows [R][2] int32 (start, count); an entry is `stride` floats, [column as
int bits, v_0 .. v_{NC-1}]; one row's columns ascend; a (row, col) is listed once when any of its NC slices is
nonzero (-0.0 counts as zero).  The extraction gives row r of a graph the slot start = slot0 + r * cap (k_extract's
slot bases); dense_lists() builds that format from the dense operators in numpy, direct_list() builds lists with
prescribed per-row entry counts for the aggregation tests.

Input families of the aggregation tests (coefficients v, features x):
  A1  v integers |v| <= 3, x integers |x| <= 7: with at most 130 entries per row and 7 slices every partial sum stays
      below 130 * 7 * 21 < 2^24.
  A3  x odd 19-bit integers with random sign, v in {0, +-1} with one nonzero slice per entry at most, rows of at most
      32 entries: every sub-sum (the backward's runs over entries and slices) stays below 2^24.
  AR  random normals (30 % of the coefficients exact zeros: the backward's zero-coefficient skip).
BN on load in A1 / A3: integer mean and b, w and std powers of two, so z is an exact integer in the family's range.
In A1 / A3 a correct kernel returns the fp64 result bit for bit whatever its summation order; in AR the kernel's rms
and max error against fp64 are held against FACTOR x those of the naive fp32 form (sequential in entry order, the
product rounded, then the sum rounded; BN as sub, div, mul, add).
"""

import ctypes

import numpy as np
import torch

from gemm_probe_util import FACTOR, SENT, bits_equal, errs, values_equal  # noqa: F401

EXACT = ("A1", "A3")
ERR_PAD_NONZERO, ERR_MASK, ERR_SIZES, ERR_DIAG_ID = 1, 2, 4, 0x40
ROW_SENT = -77777777          # sentinel of the int32 row infos
F32 = np.float32
NAN = float("nan")


# ================================================================================================ list builders
def _colbits(c):
    return np.asarray(c, dtype=np.int32).view(F32)


def dense_lists(b):
    """The six lists k_extract builds from the dense batch `b` (extract_batch): per kind a dict with rows [R][2]
    int32 (ROW_SENT past the total), ent [slots][stride] (SENT where nothing is written), spec (the floats of ent
    the format specifies: column and coefficients of the listed entries; the stride padding of a listed entry is
    unspecified) and used (the listed entry slots).  Kinds of a non-dual batch: 0 and 1 only."""
    bs, nmax, emax, jt, dual = b["bs"], b["nmax"], b["emax"], b["jtot"], b["dual"]
    sw = 4 if jt <= 3 else 8
    nb, eb = clamp_counts(b)
    n0 = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
    e0 = np.concatenate([[0], np.cumsum(eb)]).astype(np.int64)
    out = []
    W = b["W"]
    P = np.stack([b["Pm"], b["Pd"]], -1) if dual else None
    # (dense source [bs][R][C][NC], transpose, rows per graph, cols per graph, row base, col base, row length, cap)
    kinds = [(W, False, nb, nb, n0, n0, nmax, nmax, sw), (W, True, nb, nb, n0, n0, nmax, nmax, sw)]
    if dual:
        WL = b["WL"]
        kinds += [(WL, False, eb, eb, e0, e0, emax, emax, sw), (WL, True, eb, eb, e0, e0, emax, emax, sw),
                  (P, False, nb, eb, n0, e0, nmax, emax, 4), (P, True, eb, nb, e0, n0, emax, nmax, 4)]
    for (src, tr, rcnt, ccnt, rbase, cbase, rlen, cap, stride) in kinds:
        nc = src.shape[-1]
        rows = np.full((bs * rlen, 2), ROW_SENT, np.int32)
        ent = np.full((bs * rlen * cap, stride), SENT, F32)
        spec = np.zeros(ent.shape, bool)
        for g in range(bs):
            blk = src[g].transpose(1, 0, 2) if tr else src[g]
            slot0 = g * rlen * cap
            for r in range(int(rcnt[g])):
                v = blk[r, :int(ccnt[g])]
                cols = np.nonzero((v != 0).any(-1))[0]
                s = slot0 + r * cap
                rows[rbase[g] + r] = (s, len(cols))
                ent[s:s + len(cols), 0] = _colbits(cbase[g] + cols)
                ent[s:s + len(cols), 1:1 + nc] = v[cols]
                spec[s:s + len(cols), :1 + nc] = True
        out.append(dict(rows=rows, ent=ent, spec=spec, used=spec[:, 0].copy(), nc=nc, stride=stride,
                        total=int(rbase[-1])))
    return out


def clamp_counts(b):
    """N_batch / E_batch as k_plan clamps them."""
    nb = np.clip(b["Nb"], 0, b["nmax"])
    eb = np.clip(b["Eb"], 0, b["emax"]) if b["dual"] else np.zeros_like(nb)
    return nb, eb


def _coefs(g, fam, shape):
    if fam == "A1":
        return g.integers(-3, 4, shape).astype(F32)
    if fam == "A3":
        # one slice per entry is 0 / +-1, the others 0: the backward sums over entries and slices, and 32 terms of 19
        # bits is the most that stays below 2^24
        v = np.zeros(shape, F32)
        if shape[0]:
            v[np.arange(shape[0]), g.integers(0, shape[1], shape[0])] = g.integers(-1, 2, shape[0])
        return v
    v = g.standard_normal(shape).astype(F32)
    v[g.random(shape) < 0.3] = 0.0
    return v


def direct_list(g, fam, counts, cap_rows, ncol, nc, stride, diag_rows=None):
    """A list with counts[r] entries in row r (r < total = len(counts)), columns a sorted sample of [0, ncol).
    Unused entry slots hold column 0 and NaN coefficients; rows >= total point at three such slots.  diag_rows
    (diagonal I / D mode, square lists): {row: position of the diagonal entry, or None}: off-diagonal entries get
    v_0 = v_1 = 0, the diagonal entry nonzero v_0, v_1."""
    total = len(counts)
    M = max(max(counts, default=0), 1)
    slot = M + 3
    poison = cap_rows * slot
    ent = np.full((poison + 4, stride), NAN, F32)
    ent[:, 0] = 0.0
    rows = np.empty((cap_rows, 2), np.int32)
    rows[:, 0], rows[:, 1] = poison, 3
    cols = np.zeros((total, M), np.int64)
    vals = np.zeros((total, M, nc), F32)
    for r, k in enumerate(counts):
        v = _coefs(g, fam, (k, nc))
        if diag_rows is None:
            c = np.sort(g.choice(ncol, size=k, replace=False))
        else:
            pos = diag_rows.get(r)
            others = np.array([x for x in range(ncol) if x != r])
            if pos is None or k == 0:
                c = np.sort(g.choice(others, size=k, replace=False))
                v[:, :2] = 0.0
            else:
                lo = np.sort(g.choice(np.arange(r), size=pos, replace=False))
                hi = np.sort(g.choice(np.arange(r + 1, ncol), size=k - 1 - pos, replace=False))
                c = np.concatenate([lo, [r], hi])
                v[:, :2] = 0.0
                v[pos, :2] = (2.0, -3.0) if fam in EXACT else (0.75, -1.25)
                if fam == "A3":
                    v[pos, :2] = (1.0, -1.0)
        cols[r, :k], vals[r, :k] = c, v
        s = r * slot
        rows[r] = (s, k)
        ent[s:s + k, 0] = _colbits(c)
        ent[s:s + k, 1:1 + nc] = v
    return dict(rows=rows, ent=ent, cols=cols, vals=vals, cnt=np.asarray(counts, np.int64), nc=nc, stride=stride,
                slot=slot)


def relist(l):
    """The device arrays of a list rebuilt from its (possibly perturbed) cols / vals / cnt."""
    for r in range(len(l["cnt"])):
        k, s = int(l["cnt"][r]), r * l["slot"]
        l["rows"][r] = (s, k)
        l["ent"][s:s + l["slot"], 0], l["ent"][s:s + l["slot"], 1:] = 0.0, NAN
        l["ent"][s:s + k, 0] = _colbits(l["cols"][r, :k])
        l["ent"][s:s + k, 1:1 + l["nc"]] = l["vals"][r, :k]
    return l


# ================================================================================================ features
def gen_feat(g, fam, rows, c):
    if fam == "A1":
        return g.integers(-7, 8, (rows, c)).astype(F32)
    if fam == "A3":
        return ((2 ** 18 + 1 + 2 * g.integers(0, 2 ** 17, (rows, c))) * (1 - 2 * g.integers(0, 2, (rows, c)))).astype(F32)
    return g.standard_normal((rows, c)).astype(F32)


def gen_bn(g, fam, rows, c):
    """Pre-BN features y and the BN view (mean, std (c), w, b) whose z = w (y - mean) / std + b is in the family:
    A1: y = mean + 2 k, std 2, w 1, b 1 (z = k + 1 in [-3, 5]); A3: y odd 19-bit, mean odd, std 2, w 1, b -2 (z an
    integer below 2^18 + 8)."""
    if fam == "A1":
        mu = g.integers(-3, 4, c).astype(F32)
        y = (mu[None, :] + 2 * g.integers(-4, 5, (rows, c))).astype(F32)
        return y, dict(mean=mu, std=np.full(c, 2.0, F32), w=F32(1.0), b=F32(1.0))
    if fam == "A3":
        mu = (1 + 2 * g.integers(-3, 4, c)).astype(F32)
        return gen_feat(g, "A3", rows, c), dict(mean=mu, std=np.full(c, 2.0, F32), w=F32(1.0), b=F32(-2.0))
    mu = (0.3 * g.standard_normal(c)).astype(F32)
    return gen_feat(g, "AR", rows, c), dict(mean=mu, std=(0.5 + g.random(c)).astype(F32), w=F32(0.8), b=F32(-0.2))


def bn_z(y, bn, dtype):
    """z = w ((y - mean) / std) + b in `dtype`, the reference's operation order (sub, div, mul, add)."""
    if bn is None:
        return y.astype(dtype)
    t = y.astype(dtype) - bn["mean"].astype(dtype)[None, :]
    t = t / bn["std"].astype(dtype)[None, :]
    t = t * dtype(bn["w"])
    return t + dtype(bn["b"])


# ================================================================================================ references
def gather_sum(l, j, X, dtype, acc=None):
    """acc[r] (+)= sum_e v_j(e) X[col(e)] over row r's entries in order; in float32: product rounded, sum rounded."""
    R = len(l["cnt"])
    if acc is None:
        acc = np.zeros((R, X.shape[1]), dtype)
    X = X.astype(dtype)
    for e in range(int(l["cnt"].max()) if R else 0):
        m = l["cnt"] > e
        acc[m] = acc[m] + l["vals"][m, e, j].astype(dtype)[:, None] * X[l["cols"][m, e]]
    return acc


def ref_fwd(d, dtype):
    """The forward's three formulas (agg.hip header): [total][K] in `dtype` with the columns the launch does not
    write left NaN.  d: forward data (fwd_data)."""
    c = d["case"]
    jt, j0, cp = c["jtot"], c["j0"], c["cp"]
    cg = fwd_geometry(c)[5]
    K = (jt - j0) * cg + 2 * cp
    out = np.full((c["total"], K), NAN, dtype)
    if d["xg"] is not None:
        z = bn_z(d["xg"], d["gbn"], dtype)
        for j in range(j0, jt):
            out[:, (j - j0) * cg:(j - j0 + 1) * cg] = gather_sum(d["g"], j, z, dtype)
    if cp:
        z = bn_z(d["xp"], d["pbn"], dtype)
        base = (jt - j0) * cg
        out[:, base:base + cp] = gather_sum(d["p"], 0, z, dtype)
        out[:, base + cp:base + 2 * cp] = gather_sum(d["p"], 1, z, dtype)
    return out


def ref_bwd(d, dtype):
    """The backward formulas: out[r, c] (+)= sum_e sum_j v_j ing[col, gofs + j C + c] (G), or
    sum_e (pm inp[col, pofs_m + c] + pd inp[col, pofs_d + c]) (P); entry order, then slice order."""
    c = d["case"]
    C = c["c"]
    acc = d["out0"][:c["total"], :C].astype(dtype) if c["acc"] else np.zeros((c["total"], C), dtype)
    l = d["list"]
    src = d["src"].astype(dtype)
    offs = [c["gofs"] + j * C for j in range(c["jtot"])] if c["kind"] == "g" else [d["pofs_m"], d["pofs_d"]]
    for e in range(int(l["cnt"].max()) if len(l["cnt"]) else 0):
        m = l["cnt"] > e
        for j, o in enumerate(offs):
            acc[m] = acc[m] + l["vals"][m, e, j].astype(dtype)[:, None] * src[l["cols"][m, e], o:o + C]
    return acc


# ================================================================================================ checks
def check_values(name, fam, got, ref64, naive32, report=None, kind=None, shape=None):
    """got, naive32 float32 arrays, ref64 float64, same shape.  Exact families: values_equal; AR: rms and max error at
    most FACTOR x the naive leg's."""
    got_t, ref_t = torch.from_numpy(np.ascontiguousarray(got)), torch.from_numpy(np.ascontiguousarray(ref64))
    assert torch.isfinite(got_t).all(), (name, "non-finite output: a poisoned element was read")
    if fam in EXACT:
        assert values_equal(got_t, ref_t.float()), (name, "not exact", errs(got_t, ref_t))
        return
    (kr, kx), (nr, nx) = errs(got_t, ref_t), errs(torch.from_numpy(np.ascontiguousarray(naive32)), ref_t)
    if report is not None:
        report.append(dict(name=name, kind=kind, shape=shape, rms=kr, max=kx, nrms=nr, nmax=nx))
    assert kr <= FACTOR * nr and kx <= FACTOR * nx, (name, "rms", kr, nr, "max", kx, nx)


def sentinel(a):
    """All of a float32 array still holds SENT bit for bit."""
    return bool((np.ascontiguousarray(a).view(np.int32) == np.array(SENT, F32).view(np.int32)).all())


# ================================================================================================ case tables
COUNTS = (0, 1, 3, 4, 5, 8, 9, 63, 64, 65, 130)
COUNTS_A3 = (0, 1, 3, 4, 5, 8, 9, 32)
COUNTS_DIAG = (0, 1, 3, 4, 5, 8, 9, 63, 64, 65, 70)
ROWS = ((0, 48), (1, 48), (15, 48), (16, 48), (17, 48), (37, 48), (48, 48))
FWD_WIDTHS = ((5, 1), (64, 64), (100, 100), (128, 128), (256, 256), (512, 64), (130, 0), (0, 64))
FWD_JTOT = (3, 4, 7)
PAD_FROM = (0, -1, "explicit")
DIAG_WIDTHS = (64, 128, 256)
BWD_WIDTHS = (5, 64, 100, 128, 256, 512)
BWD_JTOT = (3, 4, 7)
BWD_GOFS = (0, 4)
SRC_G, SRC_P = (150, 160), (140, 144)     # (rows read, rows allocated) of the gathered tensors
SWITCH_GROUPS = {
    "rpw1": ({"HGNN_AGG_RPW": "1"}, "agg_fwd", None),
    "rpw4": ({"HGNN_AGG_RPW": "4"}, "agg_fwd", None),
    "extract_reg_off": ({"HGNN_EXTRACT_REG": "0"}, "extract", (1, 1, 1, 1, 0)),
    "extract_general": ({"HGNN_EXTRACT_LDS": "0"}, "extract", (0, 0, 0, 0, 0)),
    "extract_general_split": ({"HGNN_EXTRACT_LDS": "0", "HGNN_EXTRACT_SPLIT": "1"}, "extract", (0, 0, 0, 0, 0)),
}


def pair_counts(total, fam="A1"):
    """(G count, P count) of rows 0 .. total - 1: every count of the table in both lists, the two differing in
    the same row, (0, k), (k, 0), (65, 3) and (3, 65)."""
    cs = COUNTS_A3 if fam == "A3" else COUNTS
    n = len(cs)
    pairs = [(k, cs[(i + 3) % n]) for i, k in enumerate(cs)]
    big = cs[-1]
    pairs += [(0, 5), (5, 0), (0, big), (big, 0)]
    if fam != "A3":
        pairs += [(65, 3), (3, 65), (64, 64), (130, 130), (9, 8), (8, 9)]
    else:
        pairs += [(32, 3), (3, 32), (9, 8), (8, 9)]
    return [pairs[i % len(pairs)] for i in range(total)]


def fwd_cases():
    """Forward cases: every width x {A1, AR} at 37 of 48 rows with J_tot, the BN combination and pad_from rotating;
    every row count at two widths and J_tot 3 / 4; every J_tot at two widths; A3 at short rows."""
    out = []
    i = 0

    def add(cg, cp, jt, total, cap, fam, **kw):
        nonlocal i
        c = dict(cg=cg, cp=cp, jtot=jt, total=total, cap=cap, fam=fam, bn=i % 4, pad=PAD_FROM[i % 3], j0=0, ldo=0,
                 seed=100 + i)
        c.update(kw)
        out.append(c)
        i += 1

    n = 0
    for (cg, cp) in FWD_WIDTHS:
        for fam in ("A1", "AR"):
            # J_tot 3 (the rows-per-wave kernel) at every width; 4 and 7 alternate so each width meets both
            for jt in ((3, FWD_JTOT[1 + (n // 2 + n) % 2]) if cg <= 256 else (3,)):
                add(cg, cp, jt, 37, 48, fam)
            n += 1
    for (total, cap) in ROWS:
        for (cg, cp, jt) in ((128, 128, 3), (5, 1, 4), (64, 64, 3)):
            add(cg, cp, jt, total, cap, "A1")
    for jt in FWD_JTOT:
        for (cg, cp) in ((64, 64), (130, 0)):
            for fam in ("A1", "AR"):
                add(cg, cp, jt, 17, 48, fam)
    for (cg, cp, jt) in ((64, 64, 3), (128, 128, 4), (5, 1, 7), (0, 64, 3), (256, 256, 3)):
        for bn in (0, 3):
            add(cg, cp, jt, 37, 48, "A3", bn=bn)
    # every BN combination and every pad_from on the rows-per-wave kernel's width and on the scalar path
    for bn in range(4):
        for pad in PAD_FROM:
            add(128, 128, 3, 37, 48, "A1" if (bn + i) % 2 else "AR", bn=bn, pad=pad)
            add(100, 100, 4, 17, 48, "A1", bn=bn, pad=pad)
    return out


def diag_cases():
    out = []
    i = 0
    for c in DIAG_WIDTHS:
        for cp in (c, 0):
            for jt in FWD_JTOT:
                fam = ("A1", "AR", "A1", "A3")[i % 4]
                out.append(dict(cg=c, cp=cp, jtot=jt, total=100, cap=112, fam=fam, bn=i % 4, pad=PAD_FROM[i % 3], j0=2,
                                ldo=0, seed=300 + i))
                i += 1
    return out


def bwd_cases():
    out = []
    i = n = 0
    for c in BWD_WIDTHS:
        for kind in ("g", "p"):
            for acc in (0, 1):
                for fam in ("A1", "AR"):
                    jts = (3, BWD_JTOT[1 + (n // 2 + n) % 2]) if (kind == "g" and c <= 256) else (3,)
                    n += 1
                    for jt in jts:
                        out.append(dict(kind=kind, c=c, jtot=jt, gofs=BWD_GOFS[i % 2], total=37, cap=48, acc=acc, fam=fam,
                                        odd=0, seed=500 + i))
                        i += 1
    for (total, cap) in ROWS:
        for kind in ("g", "p"):
            out.append(dict(kind=kind, c=128, jtot=3, gofs=BWD_GOFS[i % 2], total=total, cap=cap, acc=i % 2, fam="A1",
                            odd=0, seed=500 + i))
            i += 1
    for kind in ("g", "p"):
        for c in (64, 256):
            out.append(dict(kind=kind, c=c, jtot=3, gofs=4, total=37, cap=48, acc=1, fam="A3", odd=0, seed=500 + i))
            i += 1
        # a misaligned leading dimension: the guarded scalar path at a vector width
        out.append(dict(kind=kind, c=128, jtot=3, gofs=0, total=37, cap=48, acc=0, fam="A1", odd=1, seed=500 + i))
        i += 1
    return out


PAIR_CASES = (dict(cg=64, cp=64, odd=0, one_grid=True), dict(cg=128, cp=128, odd=0, one_grid=True),
              dict(cg=256, cp=256, odd=0, one_grid=True), dict(cg=64, cp=128, odd=0, one_grid=False),
              dict(cg=128, cp=128, odd=1, one_grid=False))


# the extraction shapes: per-graph node / edge counts 0, 1, the maximum and two in between; graph 2 is complete
EXTRACT_SHAPES = (
    dict(name="dual_j3_reg", dual=1, jtot=3, nmax=9, emax=25, Nb=(0, 1, 9, 4, 7), Eb=(0, 1, 25, 7, 18), f=5, variant=2),
    dict(name="dual_j4_reg_limits", dual=1, jtot=4, nmax=32, emax=64, Nb=(0, 1, 32, 13, 27), Eb=(0, 1, 64, 30, 50), f=1,
         variant=2),
    dict(name="dual_j5_lds", dual=1, jtot=5, nmax=6, emax=8, Nb=(0, 1, 6, 3, 5), Eb=(0, 1, 8, 4, 7), f=3, variant=1),
    dict(name="simple_70_lds", dual=0, jtot=3, nmax=70, emax=0, Nb=(0, 1, 70, 33, 65), Eb=(0, 0, 0, 0, 0), f=5,
         variant=1),
    dict(name="dual_e130_general", dual=1, jtot=3, nmax=12, emax=130, Nb=(0, 1, 12, 5, 11), Eb=(0, 1, 130, 64, 129), f=64,
         variant=0),
)
INVALID = ("w_pad_row", "w_pad_col", "wl_pad", "pm_pad", "pd_pad", "mask", "sizes")


def case_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items() if k != "seed")


# ================================================================================================ case data (CPU)
def fwd_data(c, mutate=None):
    """Lists, features and BN views of a forward case.  BN combination bn: bit 0 the G part, bit 1 the P part."""
    g = np.random.default_rng(c["seed"])
    fam, jt, total, cap = c["fam"], c["jtot"], c["total"], c["cap"]
    sw = 4 if jt <= 3 else 8
    d = dict(case=c, xg=None, xp=None, gbn=None, pbn=None, g=None, p=None)
    if c["j0"] == 2:
        cnts = [(COUNTS_DIAG[(r + 2) % len(COUNTS_DIAG)], COUNTS[(r + 5) % len(COUNTS)] if fam != "A3" else
                 COUNTS_A3[r % len(COUNTS_A3)]) for r in range(total)]
        if fam == "A3":
            cnts = [(min(a, 32), b) for a, b in cnts]
        # the diagonal entry's position: pos columns below r and k - 1 - pos above it must exist
        dr = {r: (None if r % 3 == 0 or k == 0 else (max(0, k - (total - r)) + min(k - 1, r)) // 2) for r, (k, _) in
              enumerate(cnts)}
        if fam != "A3":
            cnts[80] = (70, cnts[80][1])
            dr[80] = 65            # a 70-entry row whose diagonal is the 66th entry (the second chunk)
        d["diag_rows"] = dr
        src_g = (total, cap)
    else:
        cnts = pair_counts(total, fam)
        src_g = SRC_G
    if c["cg"] and not c.get("p_only"):
        d["g"] = direct_list(g, fam, [a for a, _ in cnts], cap, src_g[0], jt, sw, d.get("diag_rows"))
        if c["bn"] & 1:
            d["xg"], d["gbn"] = gen_bn(g, fam, src_g[0], c["cg"])
        else:
            d["xg"] = gen_feat(g, fam, src_g[0], c["cg"])
    if c["cp"]:
        d["p"] = direct_list(g, fam, [b for _, b in cnts], cap, SRC_P[0], 2, 4)
        if c["bn"] & 2:
            d["xp"], d["pbn"] = gen_bn(g, fam, SRC_P[0], c["cp"])
        else:
            d["xp"] = gen_feat(g, fam, SRC_P[0], c["cp"])
    d["src_g_cap"] = src_g[1]
    return d


def fwd_geometry(c):
    """(K, ldo, pad_from argument, first column written, first zeroed column or None)."""
    cg_cols = c["cg"] if c["cg"] else 64          # a P-only launch: its columns still start at jtot * cg
    K = (c["jtot"] - c["j0"]) * cg_cols + 2 * c["cp"]
    ldo = c["ldo"] or (K + 3) // 4 * 4 + 8
    pad = {0: 0, -1: -1, "explicit": K + 2}[c["pad"]]
    zero_from = None if pad < 0 else (K if pad == 0 else pad)
    first = (c["jtot"] - c["j0"]) * cg_cols if not c["cg"] else 0
    return K, ldo, pad, first, zero_from, cg_cols


def bwd_data(c):
    g = np.random.default_rng(c["seed"])
    fam, jt, C, total, cap = c["fam"], c["jtot"], c["c"], c["total"], c["cap"]
    cnts = pair_counts(total, fam)
    d = dict(case=c)
    if c["kind"] == "g":
        d["list"] = direct_list(g, fam, [a for a, _ in cnts], cap, SRC_G[0], jt, 4 if jt <= 3 else 8)
        lo, width, rows = c["gofs"], jt * C, SRC_G
        d["ld"] = c["gofs"] + width + 4 + c["odd"]
        live = [(lo, lo + width)]
    else:
        d["list"] = direct_list(g, fam, [b for _, b in cnts], cap, SRC_P[0], 2, 4)
        c4 = (C + 3) // 4 * 4
        d["pofs_m"], d["pofs_d"], rows = 4, 4 + c4 + 4, SRC_P
        d["ld"] = d["pofs_d"] + c4 + 4 + c["odd"]
        live = [(d["pofs_m"], d["pofs_m"] + C), (d["pofs_d"], d["pofs_d"] + C)]
    src = np.full((rows[1], d["ld"]), NAN, F32)       # NaN: rows past the source's total, columns outside the blocks
    for (a, b) in live:
        src[:rows[0], a:b] = gen_feat(g, fam, rows[0], b - a)
    d["src"], d["live"] = src, live
    d["ldo"] = C + 4
    out0 = np.full((cap, d["ldo"]), SENT, F32)
    if c["acc"]:
        out0[:total, :C] = gen_feat(g, "A1" if fam in EXACT else "AR", total, C)
    d["out0"] = out0
    return d


def extract_batch(s, seed=7, invalid=None):
    """A dense batch of extraction shape s: random sparse symmetric patterns, graph 2 complete, random slices zeroed
    (an entry is listed when any slice is nonzero), some -0.0 (not listed); X / XL padding NaN (never read)."""
    g = np.random.default_rng(seed)
    bs, nmax, emax, jt, dual, f = 5, s["nmax"], s["emax"], s["jtot"], s["dual"], s["f"]
    Nb, Eb = np.array(s["Nb"], np.int64), np.array(s["Eb"], np.int64)

    def sym(n, complete):
        if complete:
            return np.ones((n, n), bool)
        p = g.random((n, n)) < 0.3
        return p | p.T

    def block(bs_, R, C, nc, rr, cc, square):
        out = np.zeros((bs_, R, C, nc), F32)
        for b in range(bs_):
            r, c_ = int(rr[b]), int(cc[b])
            pat = sym(r, b == 2) if square else ((g.random((r, c_)) < 0.3) | (b == 2))
            v = g.standard_normal((r, c_, nc)).astype(F32)
            keep = g.random((r, c_, nc)) < 0.6
            if b == 2:
                keep[..., nc - 1] = True               # complete: every (row, col) listed
            v = np.where(keep & pat[..., None], v, 0.0).astype(F32)
            v[(g.random((r, c_, nc)) < 0.05) & (v == 0)] = -0.0
            out[b, :r, :c_] = v
        return out

    b = dict(bs=bs, nmax=nmax, emax=emax, jtot=jt, dual=dual, f=f, Nb=Nb, Eb=Eb, shape=s)
    b["W"] = block(bs, nmax, nmax, jt, Nb, Nb, True)
    mask = np.zeros((bs, nmax, nmax), F32)
    for i in range(bs):
        mask[i, :Nb[i], :Nb[i]] = 1.0
    b["mask"] = mask
    X = np.full((bs, f, nmax), NAN, F32)
    for i in range(bs):
        X[i, :, :Nb[i]] = g.standard_normal((f, Nb[i]))
    b["X"] = X
    if dual:
        b["WL"] = block(bs, emax, emax, jt, Eb, Eb, True)
        P = block(bs, nmax, emax, 2, Nb, Eb, False)
        b["Pm"], b["Pd"] = np.ascontiguousarray(P[..., 0]), np.ascontiguousarray(P[..., 1])
        ml = np.zeros((bs, emax, emax), F32)
        XL = np.full((bs, 1, emax), NAN, F32)
        for i in range(bs):
            ml[i, :Eb[i], :Eb[i]] = 1.0
            XL[i, 0, :Eb[i]] = g.standard_normal(Eb[i])
        b["mask_lg"], b["XL"] = ml, XL
    b["want_err"] = 0
    if invalid:
        n3, e3 = int(Nb[3]), int(Eb[3])
        if invalid == "w_pad_row":
            b["W"][3, n3, 0, 0] = 1.0
        elif invalid == "w_pad_col":
            b["W"][3, 0, n3, jt - 1] = 1.0
        elif invalid == "wl_pad":
            b["WL"][3, e3, e3, 0] = 1.0
        elif invalid == "pm_pad":
            b["Pm"][3, n3, 0] = 1.0
        elif invalid == "pd_pad":
            b["Pd"][3, 0, e3] = 1.0
        elif invalid == "mask":
            b["mask"][3, n3 - 1, 0] = 0.0
        elif invalid == "sizes":
            # graph 2 holds nmax real nodes: k_plan clamps nmax + 1 back to nmax, the graph's true size, so the pad and
            # mask checks (which run on the clamped count) see a valid graph and add no bit of their own
            b["Nb"] = Nb.copy()
            b["Nb"][2] = nmax + 1
        b["want_err"] = {"mask": ERR_MASK, "sizes": ERR_SIZES}.get(invalid, ERR_PAD_NONZERO)
    return b


def invalid_kinds(s):
    return [k for k in INVALID if s["dual"] or k in ("w_pad_row", "w_pad_col", "mask", "sizes")]


# ================================================================================================ GPU runners
def _L():
    from hgnn_amd import _lib as L
    return L


def _dev():
    return torch.device("cuda", 0)


def _up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return _L().stream_handle(_dev())


def _set_list(pl, l, keep):
    if l is None:
        return
    r, e = _up(l["rows"]), _up(l["ent"])
    keep += [r, e]
    pl.rows, pl.entries, pl.stride = r.data_ptr(), e.data_ptr(), l["stride"]


def _set_bn(pb, bn, keep):
    if bn is None:
        return
    ts = [_up(bn["mean"]), _up(bn["std"]), _up(np.array([bn["w"]], F32)), _up(np.array([bn["b"]], F32))]
    keep += ts
    pb.mean, pb.std, pb.w, pb.b = [t.data_ptr() for t in ts]


def _src(x, rows_cap):
    """Feature rows past the source's total hold NaN."""
    if x is None:
        return None
    out = np.full((rows_cap, x.shape[1]), NAN, F32)
    out[:x.shape[0]] = x
    return _up(out)


def call_fwd(d, with_diag=None, with_err=True, overrides=None):
    """One forward probe call: (status, out [cap][ldo], diag [cap][2] or None, err word or None)."""
    L = _L()
    c = d["case"]
    K, ldo, pad, first, zero_from, cg_cols = fwd_geometry(c)
    keep = []
    p = L.ProbeAggFwd()
    tot = _up(np.array([c["total"]], np.int32))
    out = torch.full((c["cap"], ldo), SENT, device=_dev())
    _set_list(p.g, d["g"], keep)
    _set_list(p.p, d["p"], keep)
    xg, xp = _src(d["xg"], d["src_g_cap"]), _src(d["xp"], SRC_P[1])
    _set_bn(p.gbn, d["gbn"], keep)
    _set_bn(p.pbn, d["pbn"], keep)
    if d["g"] is None:
        p.g.stride = 4 if c["jtot"] <= 3 else 8
    diag = err = None
    if with_diag if with_diag is not None else c["j0"] == 2:
        diag = torch.full((c["cap"], 2), SENT, device=_dev())
        p.diag = diag.data_ptr()
    if with_err:
        err = torch.zeros(1, dtype=torch.int32, device=_dev())
        p.err = err.data_ptr()
    p.total_rows, p.xg, p.xp, p.out = tot.data_ptr(), _ptr(xg), _ptr(xp), out.data_ptr()
    p.cap_rows, p.cg, p.jtot, p.cp, p.ldo, p.pad_from, p.j0 = c["cap"], cg_cols, c["jtot"], c["cp"], ldo, pad, c["j0"]
    for k, v in (overrides or {}).items():
        setattr(p, k, v)
    st = L.lib().hgnn_probe_agg_fwd(ctypes.byref(p), _stream())
    torch.cuda.synchronize()
    return st, out.cpu().numpy(), None if diag is None else diag.cpu().numpy(), None if err is None else int(err.item())


def check_fwd(c, report=None):
    """Run one forward case and assert every property of it."""
    name = "aggfwd-" + case_id(c)
    d = fwd_data(c)
    st, out, diag, err = call_fwd(d)
    assert st == 0, (name, "status", st)
    K, ldo, pad, first, zero_from, _ = fwd_geometry(c)
    total = c["total"]
    assert sentinel(out[total:]), (name, "rows past the total written")
    assert sentinel(out[:total, :first]), (name, "columns before the P part written")
    if zero_from is None:
        assert sentinel(out[:total, K:]), (name, "pad_from = -1: the padding was written")
    else:
        assert sentinel(out[:total, K:zero_from]), (name, "columns before pad_from written")
        assert not out[:total, zero_from:].any() and not np.signbit(out[:total, zero_from:]).any(), (name, "padding not zero")
    ref64, nv = ref_fwd(d, np.float64), ref_fwd(d, F32)
    check_values(name, c["fam"], out[:total, first:K], ref64[:, first:], nv[:, first:], report, "fwd",
                 (c["cg"], c["cp"], c["jtot"], c["bn"]))
    if c["j0"] == 2:
        assert err == 0, (name, "err", err)
        assert sentinel(diag[total:]), (name, "diag rows past the total written")
        want = np.zeros((total, 2), F32)
        for r, pos in d["diag_rows"].items():
            if pos is not None and d["g"]["cnt"][r] > 0:
                want[r] = d["g"]["vals"][r, pos, :2]
        assert np.array_equal(diag[:total].view(np.int32), want.view(np.int32)), (name, "diag")
    return name, out


def bwd_struct(d, keep, out):
    L = _L()
    c = d["case"]
    p = L.ProbeAggBwd()
    tot, src = _up(np.array([c["total"]], np.int32)), _up(d["src"])
    keep += [tot, src, out]
    if c["kind"] == "g":
        _set_list(p.g, d["list"], keep)
        p.ing, p.ldg, p.gofs = src.data_ptr(), d["ld"], c["gofs"]
    else:
        _set_list(p.p, d["list"], keep)
        p.inp, p.ldp, p.pofs_m, p.pofs_d = src.data_ptr(), d["ld"], d["pofs_m"], d["pofs_d"]
    p.total_rows, p.out = tot.data_ptr(), out.data_ptr()
    p.cap_rows, p.jtot, p.c, p.ldo, p.accumulate = c["cap"], c["jtot"], c["c"], d["ldo"], c["acc"]
    return p


def call_bwd(d):
    L = _L()
    keep = []
    out = _up(d["out0"])
    p = bwd_struct(d, keep, out)
    st = L.lib().hgnn_probe_agg_bwd(ctypes.byref(p), None, 0, _stream())
    torch.cuda.synchronize()
    return st, out.cpu().numpy()


def check_bwd_output(name, d, out, report=None):
    c = d["case"]
    total, C = c["total"], c["c"]
    assert sentinel(out[total:]), (name, "rows past the total written")
    assert sentinel(out[:, C:]), (name, "columns past c written")
    check_values(name, c["fam"], out[:total, :C], ref_bwd(d, np.float64), ref_bwd(d, F32), report, "bwd_" + c["kind"],
                 (C, c["jtot"], c["acc"]))


def check_bwd(c, report=None):
    name = "aggbwd-" + case_id(c)
    d = bwd_data(c)
    st, out = call_bwd(d)
    assert st == 0, (name, "status", st)
    check_bwd_output(name, d, out, report)
    return name


def pair_data(pc, seed=900):
    cg = dict(kind="g", c=pc["cg"], jtot=3, gofs=4, total=37, cap=48, acc=1, fam="A1", odd=pc["odd"], seed=seed)
    cp = dict(kind="p", c=pc["cp"], jtot=3, gofs=0, total=33, cap=40, acc=0, fam="AR", odd=0, seed=seed + 1)
    return bwd_data(cg), bwd_data(cp)


def check_pair(pc):
    """The paired launch against the two single launches, bit for bit, and each against its reference."""
    L = _L()
    name = "aggbwd-pair-" + case_id(pc)
    dg, dp = pair_data(pc)
    keep = []
    og, op = _up(dg["out0"]), _up(dp["out0"])
    a, b = bwd_struct(dg, keep, og), bwd_struct(dp, keep, op)
    st = L.lib().hgnn_probe_agg_bwd(ctypes.byref(a), ctypes.byref(b), 1, _stream())
    torch.cuda.synchronize()
    assert st == 0, (name, "status", st)
    og, op = og.cpu().numpy(), op.cpu().numpy()
    check_bwd_output(name + "-g", dg, og)
    check_bwd_output(name + "-p", dp, op)
    for d, o in ((dg, og), (dp, op)):
        st1, o1 = call_bwd(d)
        assert st1 == 0 and np.array_equal(o.view(np.int32), o1.view(np.int32)), (name, "differs from the single launch")
    return name


def call_extract(b, validate=1, with_x=True):
    """The extraction probe on a dense batch: dict with the status, the variant and every output as numpy."""
    L = _L()
    bs, nmax, emax, jt, dual, f = b["bs"], b["nmax"], b["emax"], b["jtot"], b["dual"], b["f"]
    sw = 4 if jt <= 3 else 8
    dev = _dev()
    keep = {k: _up(b[k]) for k in ("W", "WL", "Pm", "Pd", "mask", "mask_lg", "X", "XL") if k in b}
    keep["Nb"], keep["Eb"] = _up(b["Nb"]), _up(b["Eb"])
    p = L.ProbeExtract()
    p.W, p.mask, p.n_batch = keep["W"].data_ptr(), keep["mask"].data_ptr(), keep["Nb"].data_ptr()
    if dual:
        p.WL, p.Pm, p.Pd = keep["WL"].data_ptr(), keep["Pm"].data_ptr(), keep["Pd"].data_ptr()
        p.mask_lg, p.e_batch = keep["mask_lg"].data_ptr(), keep["Eb"].data_ptr()
    isent = lambda n: torch.full((n,), ROW_SENT, dtype=torch.int32, device=dev)
    o = dict(node_off=isent(bs + 2), edge_off=isent(bs + 2), totals=isent(3), err=isent(1))
    p.node_off, p.edge_off, p.totals, p.err = [o[k].data_ptr() for k in ("node_off", "edge_off", "totals", "err")]
    rlen = (nmax, nmax, emax, emax, nmax, emax)
    cap = (nmax, nmax, emax, emax, emax, nmax)
    rows, ents = [], []
    for k in range(6 if dual else 2):
        rows.append(torch.full((bs * rlen[k], 2), ROW_SENT, dtype=torch.int32, device=dev))
        ents.append(torch.full((bs * rlen[k] * cap[k], sw if k < 4 else 4), SENT, device=dev))
        p.rows[k], p.entries[k] = rows[k].data_ptr(), ents[k].data_ptr()
    xo = xlo = None
    if with_x:
        xo = torch.full((bs * nmax, f), SENT, device=dev)
        p.X, p.xo = keep["X"].data_ptr(), xo.data_ptr()
        if dual:
            xlo = torch.full((bs * emax,), SENT, device=dev)
            p.XL, p.xlo = keep["XL"].data_ptr(), xlo.data_ptr()
    p.bs, p.nmax, p.emax, p.jtot, p.dual, p.validate, p.f, p.variant = bs, nmax, emax, jt, dual, validate, f, -1
    st = L.lib().hgnn_probe_extract(ctypes.byref(p), _stream())
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in o.items()}
    res.update(status=st, variant=p.variant, rows=[r.cpu().numpy() for r in rows], ents=[e.cpu().numpy() for e in ents],
               xo=None if xo is None else xo.cpu().numpy(), xlo=None if xlo is None else xlo.cpu().numpy())
    return res


def check_lists(name, got_rows, got_ents, want):
    for k, w in enumerate(want):
        r, e = got_rows[k], got_ents[k]
        assert np.array_equal(r, w["rows"]), (name, k, "row infos (counts, starts, sentinel past the total)")
        spec, used = w["spec"], w["used"]
        assert np.array_equal(e.view(np.int32)[spec], w["ent"].view(np.int32)[spec]), (name, k, "entries")
        assert sentinel(e[~used]), (name, k, "entry slots outside the lists written")


def check_extract(s, want_variant=None, invalid=None):
    """One extraction shape (valid, or with one invalid input): variant, plan, the six lists, packed inputs, err."""
    name = f"extract-{s['name']}-{invalid}"
    b = extract_batch(s, invalid=invalid)
    res = call_extract(b)
    assert res["status"] == 0, (name, "status", res["status"])
    if want_variant is not None:
        assert res["variant"] == want_variant, (name, "variant", res["variant"], want_variant)
    assert int(res["err"][0]) == b["want_err"], (name, "err", int(res["err"][0]), b["want_err"])
    bs = b["bs"]
    nb, eb = clamp_counts(b)
    n_off = np.concatenate([[0], np.cumsum(nb)]).astype(np.int32)
    e_off = np.concatenate([[0], np.cumsum(eb)]).astype(np.int32)
    assert np.array_equal(res["node_off"][:bs + 1], n_off) and res["node_off"][bs + 1] == ROW_SENT, (name, "node_off")
    assert np.array_equal(res["edge_off"][:bs + 1], e_off) and res["edge_off"][bs + 1] == ROW_SENT, (name, "edge_off")
    assert res["totals"].tolist() == [int(n_off[-1]), int(e_off[-1]), ROW_SENT], (name, "totals")
    check_lists(name, res["rows"], res["ents"], dense_lists(b))
    xo = np.full_like(res["xo"], SENT)
    for g in range(bs):
        xo[n_off[g]:n_off[g + 1]] = b["X"][g, :, :nb[g]].T
    assert np.array_equal(res["xo"].view(np.int32), xo.view(np.int32)), (name, "xo")
    if b["dual"]:
        xlo = np.full_like(res["xlo"], SENT)
        for g in range(bs):
            xlo[e_off[g]:e_off[g + 1]] = b["XL"][g, 0, :eb[g]]
        assert np.array_equal(res["xlo"].view(np.int32), xlo.view(np.int32)), (name, "xlo")
    return res["variant"]


def run_extract_cases(variants=None):
    """Every extraction shape, valid and with each invalid input; variants: the expected kernel per shape."""
    n = 0
    for i, s in enumerate(EXTRACT_SHAPES):
        want = s["variant"] if variants is None else variants[i]
        check_extract(s, want)
        n += 1
        for inv in invalid_kinds(s):
            check_extract(s, want, inv)
            n += 1
    return n


def run_fwd_cases(report=None):
    n = 0
    for c in fwd_cases() + diag_cases():
        check_fwd(c, report)
        n += 1
    return n
