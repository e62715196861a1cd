"""Inputs, references, case tables and runners of the Conv1d-GEMM kernel probes (include/hgnn_amd.h,
"Kernel probes"): shared by tests/test_gemm_probe_inputs.py (CPU: the inputs have the properties the GPU
tests rely on), tests/test_gpu_gemm_kernels.py and its child-process worker tests/gemm_probe_worker.py.

Input families (out = L . R^T, reduction along the last axis of both):
  E1  integers |i| <= 7 in both operands and the bias; any reduction length used here.
  E2  odd integers in [257, 511] with random sign in both operands, reduction <= 64: sum |l||r| <=
      511^2 * 64 < 2^24, and every value has a nonzero second bf16 part.
  E3  one operand odd 19-bit integers in [2^18, 2^19) with random sign, the other 0 / +-1 with at most 32
      nonzeros per reduction line: every sub-sum is below 2^24.  `wide` names the 19-bit side.
  R   random floats, L ~ N(0, 1) * ls, R ~ N(0, 1) * rs, fixed seeds.
In E1..E3 every product and every partial sum, in any order, is an integer below 2^24: exactly representable in
fp32, so a correct fp32-accurate kernel returns the fp64 result bit for bit.  In R the kernel's error against
fp64 is held against a naive fp32 GEMM's (sequential k, product rounded, sum rounded) times FACTOR.
"""

import ctypes

import numpy as np
import torch

FACTOR = 2.0      # oracle/parity.py's fp64-leg factor
SENT = -12345.678  # sentinel of the containment checks (compared bit for bit)
EXACT = ("E1", "E2", "E3")


def pad4(x):
    return (x + 3) // 4 * 4


def ld3(x):
    return (x + 15) // 16 * 16


def split3(x):
    """csrc/kernels.h split3 on an fp32 tensor: three bf16 tensors with x ~= x1 + x2 + x3."""
    a = x.to(torch.bfloat16)
    r = x - a.float()
    b = r.to(torch.bfloat16)
    c = (r - b.float()).to(torch.bfloat16)
    return a, b, c


def _signs(g, shape):
    return 1 - 2 * g.integers(0, 2, shape)


def _sparse_pm1(g, rows, red, nnz):
    out = np.zeros((rows, red), dtype=np.int64)
    n = min(nnz, red)
    for r in range(rows):
        pos = g.choice(red, size=n, replace=False)
        out[r, pos] = _signs(g, n)
    return out


def gen(family, rows_l, rows_r, red, seed, wide="l", ls=1.0, rs=0.1, nnz=32):
    """L [rows_l][red], R [rows_r][red] as float32 tensors (module docstring)."""
    g = np.random.default_rng(seed)
    if family == "E1":
        L = g.integers(-7, 8, (rows_l, red))
        R = g.integers(-7, 8, (rows_r, red))
    elif family == "E2":
        assert red <= 64
        L = (257 + 2 * g.integers(0, 128, (rows_l, red))) * _signs(g, (rows_l, red))
        R = (257 + 2 * g.integers(0, 128, (rows_r, red))) * _signs(g, (rows_r, red))
    elif family == "E3":
        def wide_m(rows):
            return (2 ** 18 + 1 + 2 * g.integers(0, 2 ** 17, (rows, red))) * _signs(g, (rows, red))
        if wide == "l":
            L, R = wide_m(rows_l), _sparse_pm1(g, rows_r, red, nnz)
        else:
            L, R = _sparse_pm1(g, rows_l, red, nnz), wide_m(rows_r)
    elif family == "R":
        L = g.standard_normal((rows_l, red)) * ls
        R = g.standard_normal((rows_r, red)) * rs
    else:
        raise ValueError(family)
    return torch.from_numpy(np.asarray(L, dtype=np.float32)), torch.from_numpy(np.asarray(R, dtype=np.float32))


def gen_bias(family, n, seed):
    g = np.random.default_rng(seed + 77)
    if family in ("E1", "E2"):
        b = g.integers(-7, 8, n)
    elif family == "E3":
        b = np.zeros(n)
    else:
        b = 0.1 * g.standard_normal(n)
    return torch.from_numpy(np.asarray(b, dtype=np.float32))


def gen_diag(family, rows, c, seed):
    """The diagonal I / D inputs (csrc/kernels.h DiagIdArgs): x [rows][c], mean, std (c), w, b scalars, diag
    [rows][2], and the operand columns [v_0 z | v_1 z] [rows][2c] the kernels must build, z = fmaf(x - mean,
    w / std, b), each product fmaf(v, z, 0).  Exact families: mean, b integers, w and std powers of two, so z and
    v z are exact small integers (E1: |v z| <= 6; E3: 0 / +-1, at most 8 nonzero z per row)."""
    g = np.random.default_rng(seed + 991)
    if family == "E1":
        mu = g.integers(-3, 4, c).astype(np.float32)
        x = (mu[None, :] + 2 * g.integers(-2, 3, (rows, c))).astype(np.float32)
        sd = np.full(c, 2.0, np.float32)
        w, b = np.float32(1.0), np.float32(1.0)
        v = g.integers(-2, 3, (rows, 2)).astype(np.float32)
    elif family == "E3":
        mu = g.integers(-3, 4, c).astype(np.float32)
        x = (mu[None, :] + 4 * _sparse_pm1(g, rows, c, 8)).astype(np.float32)
        sd = np.full(c, 8.0, np.float32)
        w, b = np.float32(2.0), np.float32(0.0)
        v = g.integers(-1, 2, (rows, 2)).astype(np.float32)
    elif family == "R":
        mu = (0.3 * g.standard_normal(c)).astype(np.float32)
        x = g.standard_normal((rows, c)).astype(np.float32)
        sd = (0.5 + g.random(c)).astype(np.float32)
        w, b = np.float32(0.8), np.float32(-0.2)
        v = g.standard_normal((rows, 2)).astype(np.float32)
    else:
        raise ValueError(family)
    scale = (w / sd).astype(np.float32)
    t = (x - mu[None, :]).astype(np.float32)
    # fmaf in fp64: the product of two floats is exact there, one rounding to float (a double rounding needs a
    # 29-bit tie pattern)
    z = (t.astype(np.float64) * scale[None, :].astype(np.float64) + np.float64(b)).astype(np.float32)
    op = np.concatenate([(v[:, 0:1].astype(np.float64) * z).astype(np.float32),
                         (v[:, 1:2].astype(np.float64) * z).astype(np.float32)], axis=1)
    f = torch.from_numpy
    return dict(x=f(x), mean=f(mu), std=f(sd), w=torch.tensor(float(w)), b=torch.tensor(float(b)), diag=f(v),
                op=f(op), c=c)


def naive_fp32_gemm(L, R):
    """out[i][j] = sum_k L[i][k] R[j][k] in float32: sequential k, the product rounded, then the sum rounded."""
    Ln, Rn = L.numpy().astype(np.float32), R.numpy().astype(np.float32)
    acc = np.zeros((Ln.shape[0], Rn.shape[0]), dtype=np.float32)
    for k in range(Ln.shape[1]):
        acc += Ln[:, k:k + 1] * Rn[None, :, k]
    return torch.from_numpy(acc)


def errs(got, ref64):
    e = (got.double() - ref64).abs()
    return (float(e.pow(2).mean().sqrt()) if e.numel() else 0.0), (float(e.max()) if e.numel() else 0.0)


def ulp_dist(a, b):
    """Distance in float32 ulps between two float32 tensors (finite values)."""
    def key(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (key(a) - key(b)).abs()


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def values_equal(a, b):
    """Bit for bit, the sign of a zero aside (a sum of signed zeros depends on the summation order)."""
    return bits_equal(a + 0.0, b + 0.0)


# ---------------------------------------------------------------------------------------------- case tables
FWD_K = (4, 12, 32, 36, 68, 96, 100, 640)                       # nt = 1, 1, 1, 2, 3, 3, 4, 20
FWD_M = ((1, 64), (63, 64), (64, 64), (65, 128), (130, 192), (517, 576))
FWD_N = (64, 128, 192)
DA_M = FWD_M
DA_C2_BF3 = (4, 8, 32, 36, 64, 100, 128)                         # NST = 1, 1, 1, 2, 2, 4, 4; 4 and 8: d = 1, 3
DA_C2_FP32 = (8, 128, 256)
DA_KOUT = (12, 64, 100, 640)
DW_R = ((1, 64), (15, 64), (16, 64), (17, 64), (63, 64), (64, 64), (65, 128), (200, 256), (1000, 1024))
DW_NZ = (0, 8, 16)
DW_O = ((128, 128, 64), (64, 64, 32), (8, 6, 3), (256, 256, 128))
DW_K = (12, 128, 132, 640)


def _relu_from(n, i):
    return (0, n // 2, 37, n)[i % 4]


def families_for(red):
    return ("E1", "E2", "E3") if red <= 64 else ("E1", "E3")


def fwd_cases(kernel):
    """Forward cases of one kernel selector: every K x M x N, the ReLU start and the exact family rotating; family R
    on two (M, N) per K; the BN modes on the odd stage counts and the 517-row shape."""
    out = []
    i = 0
    for k in FWD_K:
        for (m, cap) in FWD_M:
            for n in FWD_N:
                fams = families_for(k)
                fam = fams[i % len(fams)]
                bns = (0, 1, 2, 3) if kernel == 0 else (0, 1)
                bn = bns[i % len(bns)] if (k in (12, 68, 96) or m == 517) else 0
                out.append(dict(kernel=kernel, k=k, m=m, cap=cap, n=n, relu=_relu_from(n, i), fam=fam,
                                wide="lr"[i % 2], bn=bn, c=0, seed=1000 + i))
                i += 1
        for (m, cap, n) in ((130, 192, 128), (517, 576, 192)):
            out.append(dict(kernel=kernel, k=k, m=m, cap=cap, n=n, relu=n // 2, fam="R", wide="l",
                            bn=(1 if kernel else 2) if k in (12, 96) else 0, c=0, seed=2000 + i))
            i += 1
    # every BN mode on an odd stage count (K = 12: one stage; 68: three) and on the 517-row shape, exact and random
    bns = (1, 2, 3) if kernel == 0 else (1,)
    for bn in bns:
        for (k, m, cap, n) in ((12, 65, 128, 64), (68, 130, 192, 128), (96, 517, 576, 192), (640, 517, 576, 64)):
            for fam in ("E1", "R"):
                out.append(dict(kernel=kernel, k=k, m=m, cap=cap, n=n, relu=n // 2, fam=fam, wide="l", bn=bn, c=0,
                                seed=3000 + i, run=True))
                i += 1
    return out


def fwd_special_cases():
    out = [dict(kernel=0, k=36, m=130, cap=192, n=40, relu=20, fam=f, wide="l", bn=b, c=0, seed=4000 + j)
           for j, (f, b) in enumerate((("E1", 0), ("E2", 2), ("R", 1), ("E3", 3)))]
    # the diagonal I / D columns: c = 16, K = 32 + 36 (one diagonal stage, an odd remainder); c = 64, K = 128 + 64
    j = 0
    for (c, ka) in ((16, 36), (64, 64)):
        for fam in ("E1", "E3", "R"):
            for (m, cap, bn) in ((65, 128, 0), (517, 576, 3)):
                out.append(dict(kernel=0, k=2 * c + ka, m=m, cap=cap, n=128, relu=64, fam=fam, wide="r", bn=bn, c=c,
                                seed=4100 + j, run=True))
                j += 1
    return out


def da_cases(kernel):
    out = []
    i = 0
    for c2 in (DA_C2_BF3 if kernel == 0 else DA_C2_FP32):
        for kout in DA_KOUT:
            for (m, cap) in DA_M:
                fams = families_for(c2) + ("R",)
                out.append(dict(kernel=kernel, c2=c2, kout=kout, m=m, cap=cap, fam=fams[i % len(fams)],
                                wide="lr"[i % 2], ldda=pad4(kout) + (8 if kout == 100 else 0), seed=5000 + i))
                i += 1
    return out


def dw_cases():
    """dW cases: every R with every nz at one shape, every (o, k) at two row counts, families rotating."""
    out = []
    i = 0
    for (r, cap) in DW_R:
        for nz in DW_NZ:
            for (o, o_real, split), k in (((128, 128, 64), 132), ((8, 6, 3), 12)):
                fams = families_for(r) + ("R",)
                out.append(dict(r=r, cap=cap, nz=nz, o=o, o_real=o_real, split=split, k=k, fam=fams[i % len(fams)],
                                wide="lr"[i % 2], c=0, db=i % 2 == 0, seed=6000 + i))
                i += 1
    for (o, o_real, split) in DW_O:
        for k in DW_K:
            for (r, cap) in ((65, 128), (1000, 1024)):
                fams = ("E1", "E3", "R")
                out.append(dict(r=r, cap=cap, nz=(0, 8, 16)[i % 3], o=o, o_real=o_real, split=split, k=k,
                                fam=fams[i % 3], wide="lr"[i % 2], c=0, db=i % 2 == 1, seed=6500 + i))
                i += 1
    for j, (fam, r, cap) in enumerate((("E1", 200, 256), ("R", 1000, 1024), ("E1", 17, 64))):
        out.append(dict(r=r, cap=cap, nz=0, o=128, o_real=128, split=64, k=128 + 132, fam=fam, wide="l", c=64,
                        db=True, seed=6900 + j))
    return out


def case_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items() if k not in ("seed", "run"))


# ---------------------------------------------------------------------------------------------- CPU references
def fwd_inputs(c):
    """A [m][ka], W [n][k], bias [n], the diagonal inputs (or None) and the logical operand [m][k]."""
    ka = c["k"] - 2 * c["c"]
    nnz = 16 if c["c"] else 32
    A, W = gen(c["fam"], c["m"], c["n"], c["k"], c["seed"], c["wide"], nnz=nnz)
    dg = None
    if c["c"]:
        dg = gen_diag(c["fam"], c["m"], c["c"], c["seed"])
        A = A[:, 2 * c["c"]:].contiguous() if c["fam"] != "E3" else gen("E3", c["m"], 1, ka, c["seed"] + 5, "r",
                                                                       nnz=16)[0]
        op = torch.cat([dg["op"], A], dim=1)
    else:
        op = A
    return A, W, gen_bias(c["fam"], c["n"], c["seed"]), dg, op


def fwd_epilogue(acc, bias, relu_from):
    y = acc + bias[None, :].to(acc.dtype)
    y[:, relu_from:] = y[:, relu_from:].clamp_min(0)
    return y


def bn_expect(y, m):
    """k_bn_finalize's formula in fp64 from the kernel's own Y over the m real rows."""
    yd = y[:m].double()
    if m == 0:
        z = torch.zeros(y.shape[1], dtype=torch.float64)
        return z, torch.full_like(z, 1e-5).sqrt()
    mean = yd.sum(0) / m
    var = ((yd * yd).sum(0) / m - mean * mean).clamp_min(0) + 1e-5
    return mean, var.sqrt()


# ---------------------------------------------------------------------------------------------- GPU runners
def _lib():
    from hgnn_amd import _lib as L
    return L


def _dev():
    return torch.device("cuda", 0)


def _ws(nbytes):
    """A workspace of NaN bit patterns (0xFF bytes: NaN as float, bf16 and double)."""
    return torch.full((max(nbytes, 256),), 0xFF, dtype=torch.uint8, device=_dev())


def _padded(t, rows, ld, fill):
    """t [r][c] inside a [rows][ld] device tensor filled with `fill`."""
    out = torch.full((rows, ld), fill, dtype=torch.float32)
    out[:t.shape[0], :t.shape[1]] = t
    return out.to(_dev())


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return _lib().stream_handle(_dev())


def _set_pair(p, keep, wl, wr, bl, br):
    ts = [t.contiguous().to(_dev()) for t in (wl, wr, bl, br)]
    keep.extend(ts)
    p.wl, p.wr, p.bl, p.br = [t.data_ptr() for t in ts]


def _set_diag(p, keep, dg, rows_cap):
    """x, diag rows past the real ones and x's padding columns hold NaN."""
    nan = float("nan")
    c = dg["c"]
    x = _padded(dg["x"], rows_cap, c + 4, nan)
    v = _padded(dg["diag"], rows_cap, 2, nan)
    ts = [x, v] + [dg[k].reshape(-1).to(_dev()) for k in ("mean", "std", "w", "b")]
    keep.extend(ts)
    p.diag.x, p.diag.diag, p.diag.mean, p.diag.std, p.diag.w, p.diag.b = [t.data_ptr() for t in ts]
    p.diag.ldx, p.diag.c = c + 4, c


def run_repack(d, k, seed=1):
    """The repack probe on a random pair: (inputs, outputs) as CPU tensors; every output pre-filled with NaN bits."""
    L = _lib()
    g = torch.Generator().manual_seed(seed)
    wl, wr = torch.randn(d, k, generator=g), torch.randn(d, k, generator=g)
    bl, br = torch.randn(d, generator=g), torch.randn(d, generator=g)
    c2, c2p, kp = 2 * d, pad4(2 * d), pad4(k)
    dev = _dev()
    nan = float("nan")
    wt = torch.full((k, c2p), nan, device=dev)
    wc = torch.full((c2, kp), nan, device=dev)
    bc = torch.full((c2,), nan, device=dev)
    wc3 = torch.full((3, c2, ld3(kp)), nan, device=dev, dtype=torch.bfloat16)
    wt3 = torch.full((3, k, ld3(c2p)), nan, device=dev, dtype=torch.bfloat16)
    ins = [t.to(dev) for t in (wl, wr, bl, br)]
    r = L.lib().hgnn_probe_repack(*[_p(t) for t in ins], d, k, _p(wt), _p(wc), _p(bc), _p(wc3), _p(wt3), _stream())
    assert r == 0, r
    torch.cuda.synchronize()
    return (wl, wr, bl, br), tuple(t.cpu() for t in (wt, wc, bc, wc3, wt3))


def call_fwd(c, A, W, bias, dg, run=None):
    """One forward probe call with poisoned inputs and sentinel-filled outputs.  Returns (status, Y [cap][ldy],
    mean, std, run_mean, run_std, ticket) as CPU tensors."""
    L = _lib()
    dev = _dev()
    nan = float("nan")
    n, d, k, cap, m = c["n"], c["n"] // 2, c["k"], c["cap"], c["m"]
    ka = k - 2 * c["c"]
    lda = ka + 4 if c["kernel"] == 0 else pad4(ka)   # the split-bf16 kernels never read columns [k, lda)
    ldy = n + 4
    keep = []
    p = L.ProbeFwd()
    a = _padded(A, cap, lda, nan)
    y = torch.full((cap, ldy), SENT, device=dev)
    mv = torch.tensor([m], dtype=torch.int32, device=dev)
    _set_pair(p, keep, W[:d], W[d:], bias[:d], bias[d:])
    if dg is not None:
        _set_diag(p, keep, dg, cap)
    mean = torch.full((n + 1,), SENT, device=dev)
    std = torch.full((n + 1,), SENT, device=dev)
    tick = torch.full((1,), 0x7FFFFFFF, dtype=torch.int32, device=dev)
    rm = rs = None
    if run is not None:
        rm, rs = run[0].clone().to(dev), run[1].clone().to(dev)
        p.run_mean, p.run_std = rm.data_ptr(), rs.data_ptr()
    p.a, p.m_valid, p.y = a.data_ptr(), mv.data_ptr(), y.data_ptr()
    p.mean, p.std, p.ticket_out = mean.data_ptr(), std.data_ptr(), tick.data_ptr()
    p.lda, p.m_cap, p.d, p.k, p.relu_from, p.ldy, p.kernel, p.bn = lda, cap, d, k, c["relu"], ldy, c["kernel"], c["bn"]
    ws = _ws(L.lib().hgnn_probe_gemm_workspace_bytes(d, k, cap))
    r = L.lib().hgnn_probe_gemm_fwd(ctypes.byref(p), _p(ws), _stream())
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.cpu()
    return r, y.cpu(), mean.cpu(), std.cpu(), cpu(rm), cpu(rs), int(tick.item())


def check_fwd(c, report=None):
    """Run one forward case and assert every property of it; `report` collects family R's error figures."""
    name = "fwd-" + case_id(c)
    A, W, bias, dg, op = fwd_inputs(c)
    n, m, cap = c["n"], c["m"], c["cap"]
    run = None
    if c.get("run") and c["bn"]:
        g = torch.Generator().manual_seed(c["seed"])
        run = (torch.randn(n, generator=g), torch.rand(n, generator=g) + 0.5)
    r, y, mean, std, rm, rs, tick = call_fwd(c, A, W, bias, dg, run)
    assert r == 0, (name, "status", r)
    ref = fwd_epilogue(op.double() @ W.double().T, bias, c["relu"])
    got = y[:m, :n]
    sent = torch.tensor(SENT)
    assert bits_equal(y[m:], sent.expand_as(y[m:])), (name, "rows past M written")
    assert bits_equal(y[:, n:], sent.expand_as(y[:, n:])), (name, "columns past N written")
    assert torch.isfinite(got).all(), (name, "non-finite output: a poisoned element was read")
    if c["fam"] in EXACT:
        assert values_equal(got, ref.float()), (name, "not exact", errs(got, ref))
    else:
        nv = fwd_epilogue(naive_fp32_gemm(op, W), bias, c["relu"])
        (kr, kx), (nr, nx) = errs(got, ref), errs(nv, ref)
        if report is not None:
            report.append(dict(name=name, kind=f"fwd{c['kernel']}", K=c["k"], rms=kr, max=kx, nrms=nr, nmax=nx))
        assert kr <= FACTOR * nr and kx <= FACTOR * nx, (name, "rms", kr, nr, "max", kx, nx)
    if c["bn"]:
        check_bn(name, c, y, mean, std, rm, rs, run, tick)
        if c["bn"] >= 2 and c["fam"] in ("E1", "E2"):
            # exact sums whatever the atomic order (test_gemm_probe_inputs checks sum y^2 < 2^53): a second run, the
            # accumulators zeroed again by the probe, gives the same bits
            r2, y2, mean2, std2, _, _, tick2 = call_fwd(c, A, W, bias, dg, run)
            assert r2 == 0 and bits_equal(y, y2) and bits_equal(mean, mean2) and bits_equal(std, std2), \
                (name, "second run differs")
    return name


def check_bn(name, c, y, mean, std, rm, rs, run, tick):
    n, m = c["n"], c["m"]
    sent = torch.tensor(SENT)
    assert bits_equal(mean[n:], sent.expand(1)) and bits_equal(std[n:], sent.expand(1)), (name, "mean / std past N")
    em, es = bn_expect(y[:, :n], m)
    if c["bn"] >= 2:
        dm, ds = ulp_dist(mean[:n], em.float()), ulp_dist(std[:n], es.float())
        assert dm.max() <= 2 and ds.max() <= 2, (name, "BN ulps", int(dm.max()), int(ds.max()))
    else:
        # float partials (count, mean, M2 per 64-row tile): rtol 1e-5 of test_bn_train_eval_match_reference; the
        # mean's error scales with the column's magnitude |mean| + std, not with a cancelled mean
        assert ((mean[:n].double() - em).abs() <= 1e-5 * (em.abs() + es)).all(), (name, "BN mean")
        assert ((std[:n].double() - es).abs() <= 1e-5 * es).all(), (name, "BN std")
    if c["bn"] == 3:
        assert tick == 0, (name, "ticket", tick)
    if run is not None:
        for got, new, old, what in ((rm, mean[:n], run[0], "run_mean"), (rs, std[:n], run[1], "run_std")):
            want = 0.9 * new.double() + 0.1 * old.double()
            assert ((got.double() - want).abs() <= 1e-6 * (0.9 * new.double().abs() + 0.1 * old.double().abs())
                    ).all(), (name, what)


def da_width(c2):
    """The Conv1d width d behind a dA reduction width: 4 and 8 are the padded odd widths d = 1 and d = 3."""
    return {4: 1, 8: 3}.get(c2, c2 // 2)


def da_inputs(c):
    """dY [m][2d] and Wcat^T [kout][2d]: dA = dY . Wcat."""
    return gen(c["fam"], c["m"], c["kout"], 2 * da_width(c["c2"]), c["seed"], c["wide"])


def check_da(c, report=None):
    name = "da-" + case_id(c)
    L = _lib()
    dev = _dev()
    nan = float("nan")
    c2, kout, m, cap = c["c2"], c["kout"], c["m"], c["cap"]
    c2p = pad4(c2)
    dreal = da_width(c2)
    creal = 2 * dreal
    dy, wt = da_inputs(c)
    # dY's padding columns [2d, c2p) are read (times WT's zero padding): finite, arbitrary
    dyp = torch.full((m, c2p), 3.0)
    dyp[:, :creal] = dy
    W = wt.T.contiguous()                              # Wcat [2d][kout]
    keep = []
    p = L.ProbeDa()
    _set_pair(p, keep, W[:dreal], W[dreal:], torch.zeros(dreal), torch.zeros(dreal))
    dyd = _padded(dyp, cap, c2p, nan)
    ldda = c["ldda"]
    da = torch.full((cap, ldda), SENT, device=dev)
    mv = torch.tensor([m], dtype=torch.int32, device=dev)
    p.dy, p.m_valid, p.da = dyd.data_ptr(), mv.data_ptr(), da.data_ptr()
    p.lddy, p.m_cap, p.d, p.k, p.ldda, p.kernel = c2p, cap, dreal, kout, ldda, c["kernel"]
    ws = _ws(L.lib().hgnn_probe_gemm_workspace_bytes(dreal, kout, cap))
    r = L.lib().hgnn_probe_gemm_da(ctypes.byref(p), _p(ws), _stream())
    torch.cuda.synchronize()
    assert r == 0, (name, "status", r)
    out = da.cpu()
    got = out[:m, :kout]
    sent = torch.tensor(SENT)
    assert bits_equal(out[m:], sent.expand_as(out[m:])), (name, "rows past M written")
    assert bits_equal(out[:, kout:], sent.expand_as(out[:, kout:])), (name, "columns past kout written")
    assert torch.isfinite(got).all(), (name, "non-finite output: a poisoned element was read")
    ref = dy.double() @ wt.double().T
    if c["fam"] in EXACT:
        assert values_equal(got, ref.float()), (name, "not exact", errs(got, ref))
    else:
        (kr, kx), (nr, nx) = errs(got, ref), errs(naive_fp32_gemm(dy, wt), ref)
        if report is not None:
            report.append(dict(name=name, kind=f"da{c['kernel']}", K=creal, rms=kr, max=kx, nrms=nr, nmax=nx))
        assert kr <= FACTOR * nr and kx <= FACTOR * nx, (name, "rms", kr, nr, "max", kx, nx)
    return name


def dw_inputs(c):
    """dY [r][o_real] and the logical operand [r][k] (with its parts): dW = dY^T . operand."""
    r, k, cc = c["r"], c["k"], c["c"]
    dyT, opT = gen(c["fam"], c["o_real"], k, r, c["seed"], c["wide"], ls=1.0, rs=1.0)
    dy, op = dyT.T.contiguous(), opT.T.contiguous()
    dg = None
    A = op
    if cc:
        dg = gen_diag(c["fam"], r, cc, c["seed"])
        A = op[:, 2 * cc:].contiguous()
        op = torch.cat([dg["op"], A], dim=1)
    return dy, A, dg, op


def check_dw(c, report=None):
    name = "dw-" + case_id(c)
    L = _lib()
    dev = _dev()
    nan = float("nan")
    r, cap, o, o_real, split, k = c["r"], c["cap"], c["o"], c["o_real"], c["split"], c["k"]
    dy, A, dg, op = dw_inputs(c)
    dyp = torch.zeros((r, o))                          # columns [o_real, o): the zero padding of an odd 2d
    dyp[:, :o_real] = dy
    keep = []
    p = L.ProbeDw()
    lda = pad4(A.shape[1]) + 4
    dyd, ad = _padded(dyp, cap, o, nan), _padded(A, cap, lda, nan)
    if dg is not None:
        _set_diag(p, keep, dg, cap)
    rv = torch.tensor([r], dtype=torch.int32, device=dev)
    dw0 = torch.full((split + 1, k), SENT, device=dev)
    dw1 = torch.full((o_real - split + 1, k), SENT, device=dev)
    db0 = torch.full((split + 1,), SENT, device=dev)
    db1 = torch.full((o_real - split + 1,), SENT, device=dev)
    tiles, tv = (cap + 63) // 64, (r + 63) // 64
    part = None
    if c["db"]:
        # the BN backward's per-64-row-tile column sums of dY, rounded to float; tiles past the rows hold NaN
        part = torch.full((tiles, o_real), nan)
        for t in range(tv):
            part[t] = dy[64 * t:64 * t + 64].double().sum(0).float()
        partd = part.to(dev)
        p.dbpart, p.db0, p.db1 = partd.data_ptr(), db0.data_ptr(), db1.data_ptr()
    p.dy, p.a, p.r_valid, p.dw0, p.dw1 = dyd.data_ptr(), ad.data_ptr(), rv.data_ptr(), dw0.data_ptr(), dw1.data_ptr()
    p.lddy, p.lda, p.r_cap, p.o, p.o_real, p.split, p.k, p.nz = o, lda, cap, o, o_real, split, k, c["nz"]
    ws = _ws(L.lib().hgnn_probe_dw_workspace_bytes(cap, o, k, c["nz"]))   # NaN slabs: empty chunks must not be read
    st = L.lib().hgnn_probe_gemm_dw(ctypes.byref(p), _p(ws), _stream())
    torch.cuda.synchronize()
    if dg is not None and not L.switch("HGNN_DW_BF3"):
        assert st == 2, (name, "the fp32 dW GEMM has no diagonal columns: expected HGNN_ERR_UNSUPPORTED", st)
        return name
    assert st == 0, (name, "status", st)
    g0, g1 = dw0.cpu(), dw1.cpu()
    sent = torch.tensor(SENT)
    assert bits_equal(g0[split:], sent.expand(1, k)) and bits_equal(g1[o_real - split:], sent.expand(1, k)), \
        (name, "rows past the gradient written")
    got = torch.cat([g0[:split], g1[:o_real - split]], dim=0)
    assert torch.isfinite(got).all(), (name, "non-finite output: a poisoned element or an empty slab was read")
    ref = dy.double().T @ op.double()
    if c["fam"] in EXACT:
        assert values_equal(got, ref.float()), (name, "not exact", errs(got, ref))
    else:
        (kr, kx), (nr, nx) = errs(got, ref), errs(naive_fp32_gemm(dy.T.contiguous(), op.T.contiguous()), ref)
        if report is not None:
            report.append(dict(name=name, kind="dw", K=r, rms=kr, max=kx, nrms=nr, nmax=nx))
        assert kr <= FACTOR * nr and kx <= FACTOR * nx, (name, "rms", kr, nr, "max", kx, nx)
    if c["db"]:
        b0, b1 = db0.cpu(), db1.cpu()
        assert bits_equal(b0[split:], sent.expand(1)) and bits_equal(b1[o_real - split:], sent.expand(1)), \
            (name, "bias gradient past its end written")
        gb = torch.cat([b0[:split], b1[:o_real - split]])
        rb = dy.double().sum(0)
        # each tile sum carries one float rounding (2^-24 of itself), the reduction is fp64, the result one more
        tol = 2.0 ** -24 * (part[:tv].double().abs().sum(0) + rb.abs()) * 1.001
        assert ((gb.double() - rb).abs() <= tol).all(), (name, "bias gradient", errs(gb, rb))
    return name
