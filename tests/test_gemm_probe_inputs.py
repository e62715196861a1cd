"""The inputs of the GEMM kernel tests (tests/gemm_probe_util.py) have the properties those tests rely on -- checked
on the CPU, so a mistake in a generator cannot make a GPU assertion vacuous.

Exact families, each at the largest reduction length it is used with: the fp32 matmul equals the fp64 one
(torch.equal), the three-way bf16 split leaves no residual, every E2 value has a nonzero second part and at least
half the E3 values a nonzero third part.  The diagonal I / D inputs of the exact families give exact operands, and
the BN sums of the exact cases that are run twice stay below 2^53.
"""

import pytest
import torch

import gemm_probe_util as U


def _resid(x):
    a, b, c = U.split3(x)
    return x - a.float() - b.float() - c.float(), a, b, c


# (family, wide side, reduction length): the largest each family meets in the case tables (forward K = 640, dW
# R = 1000 rows; E2 up to 64)
LARGEST = [("E1", "l", 1000), ("E2", "l", 64), ("E3", "l", 1000), ("E3", "r", 1000)]


@pytest.mark.parametrize("fam,wide,red", LARGEST)
def test_exact_family_is_exact_in_fp32(fam, wide, red):
    L, R = U.gen(fam, 130, 64, red, 11, wide, ls=1.0, rs=1.0)
    y32, y64 = L @ R.T, L.double() @ R.double().T
    assert torch.equal(y32.double(), y64)
    assert y64.abs().max() < 2 ** 24
    # any order: the sum of absolute products bounds every partial sum
    assert (L.double().abs() @ R.double().abs().T).max() < 2 ** 24
    # the bias added last keeps the sum an exact integer
    b = U.gen_bias(fam, 64, 11)
    assert ((L.double().abs() @ R.double().abs().T) + b.double().abs()[None, :]).max() < 2 ** 24
    for x in (L, R):
        r, a, bb, c = _resid(x)
        assert torch.count_nonzero(r) == 0
    if fam == "E2":
        for x in (L, R):
            assert (_resid(x)[2].float() != 0).all()
    if fam == "E3":
        x = L if wide == "l" else R
        assert (_resid(x)[3].float() != 0).float().mean() >= 0.5
        s = R if wide == "l" else L
        assert (s != 0).sum(1).max() <= 32 and set(s.unique().tolist()) <= {-1.0, 0.0, 1.0}


def test_families_cover_the_case_tables():
    ks = [c["k"] for c in U.fwd_cases(0)] + [c["r"] for c in U.dw_cases()] + [c["c2"] for c in U.da_cases(0)]
    assert max(ks) <= 1000
    for c in U.fwd_cases(0) + U.fwd_cases(1) + U.fwd_special_cases():
        assert c["fam"] != "E2" or c["k"] <= 64, c
    for c in U.dw_cases():
        assert c["fam"] != "E2" or c["r"] <= 64, c
    for c in U.da_cases(0) + U.da_cases(1):
        assert c["fam"] != "E2" or c["c2"] <= 64, c
    # the shapes stay small, and every set of the case tables is met
    f = U.fwd_cases(0) + U.fwd_special_cases()
    assert {c["k"] for c in U.fwd_cases(0)} == set(U.FWD_K) and {c["n"] for c in f} == {40, 64, 128, 192}
    assert {(c["m"], c["cap"]) for c in U.fwd_cases(0)} == set(U.FWD_M)
    assert all(c["m"] <= 600 and c["n"] <= 192 and c["k"] <= 640 for c in f)
    for bn in (1, 2, 3):
        assert {c["k"] for c in f if c["bn"] == bn} >= {12, 68} and any(c["m"] == 517 for c in f if c["bn"] == bn)
    assert {c["c2"] for c in U.da_cases(0)} == set(U.DA_C2_BF3) and {c["c2"] for c in U.da_cases(1)} == set(U.DA_C2_FP32)
    assert any(c["ldda"] > U.pad4(c["kout"]) for c in U.da_cases(0))
    d = U.dw_cases()
    assert {(c["r"], c["cap"]) for c in d} == set(U.DW_R) and {c["nz"] for c in d} == set(U.DW_NZ)
    assert {(c["o"], c["o_real"], c["split"]) for c in d} == set(U.DW_O) and {c["k"] for c in d} >= set(U.DW_K)


@pytest.mark.parametrize("fam", ["E1", "E3"])
def test_diag_inputs_are_exact(fam):
    dg = U.gen_diag(fam, 130, 64, 5)
    x, mu, sd = dg["x"].double(), dg["mean"].double(), dg["std"].double()
    z = (x - mu) * (dg["w"].double() / sd) + dg["b"].double()
    want = torch.cat([dg["diag"][:, 0:1].double() * z, dg["diag"][:, 1:2].double() * z], dim=1)
    assert torch.equal(dg["op"].double(), want)
    assert torch.equal(want, want.round()) and want.abs().max() <= (6 if fam == "E1" else 1)
    assert (dg["w"] / dg["std"]).double().equal(dg["w"].double() / sd)   # the scale w / std is exact in float
    if fam == "E3":
        assert (z != 0).sum(1).max() <= 8


def test_diag_operand_of_exact_cases_stays_in_its_family():
    for c in U.fwd_special_cases():
        if not c["c"] or c["fam"] == "R":
            continue
        A, W, bias, dg, op = U.fwd_inputs(c)
        assert op.shape == (c["m"], c["k"]) and W.shape == (c["n"], c["k"])
        assert torch.equal((op @ W.T).double(), op.double() @ W.double().T)
        assert (op.double().abs() @ W.double().abs().T).max() < 2 ** 24
        if c["fam"] == "E3":
            assert (op != 0).sum(1).max() <= 32


def test_bn_sums_of_rerun_cases_are_exact_in_fp64():
    for c in U.fwd_cases(0) + U.fwd_special_cases():
        if c["bn"] >= 2 and c["fam"] in ("E1", "E2"):
            A, W, bias, dg, op = U.fwd_inputs(c)
            y = U.fwd_epilogue(op.double() @ W.double().T, bias, c["relu"])
            assert (y * y).sum(0).max() < 2 ** 53, c


def test_naive_gemm_is_sequential_fp32():
    L, R = U.gen("R", 3, 2, 37, 3)
    want = torch.zeros(3, 2)
    for i in range(3):
        for j in range(2):
            acc = torch.tensor(0.0)
            for k in range(37):
                acc = acc + L[i, k] * R[j, k]
            want[i, j] = acc
    assert torch.equal(U.naive_fp32_gemm(L, R), want)


def test_ulp_distance():
    a = torch.tensor([1.0, -1.0, 0.0, 1e-3])
    b = torch.nextafter(a, torch.tensor([2.0, -2.0, 1.0, 0.0]))
    assert U.ulp_dist(a, b).tolist() == [1, 1, 1, 1]
    assert U.ulp_dist(torch.tensor([-0.0]), torch.tensor([0.0])).item() == 0
