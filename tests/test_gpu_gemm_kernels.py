"""The Conv1d-pair GEMM kernels and the weight repack, one kernel at a time, against plain fp64 on the CPU.

Through the kernel probes (include/hgnn_amd.h "Kernel probes", csrc/probe.hip) every launcher of csrc/gemm_bf3.hip
and csrc/gemm3.hip is handed the shapes the whole-network tests never present: stage counts 1 .. 20 (odd ones
included), row counts around the 64-row tile and past eight row tiles, N = 40 .. 192, a device row count below the
capacity, the diagonal I / D operand columns.  tests/gemm_probe_util.py holds the inputs, the case tables and the
checks; tests/test_gemm_probe_inputs.py checks the inputs themselves on the CPU.

Every case:
  * exact families E1 / E2 / E3 (integers whose every partial sum fits 24 bits): the output equals the fp64
    result bit for bit -- a lost product term, bf16 plane or k-chunk changes it;
  * family R (random floats): rms and max error against fp64 at most 2 x those of a naive sequential fp32 GEMM
    of the same operands (the fp64-leg factor of oracle/parity.py);
  * containment: outputs pre-filled with a sentinel keep it in rows >= M and columns >= N;
  * poison: NaN in everything the contracts of csrc/kernels.h say is not read (operand rows past the device
    count, A's columns past k for the split-bf16 kernels, x / diag rows past M, the whole workspace with the
    dW slabs) -- no output may turn non-finite.

The odd stage counts (K = 4, 12, 32: one stage; 68, 96: three) run the forward epilogue whose LDS scratch used to
overlay the last stage's operands (fixed by pointing it at the other stage buffer); these cases cover that path,
they cannot prove a timing-dependent race absent.

Family R, measured on an MI355X (error against fp64 of the kernel / of the naive fp32 GEMM; the largest ratio
over the cases of a row decides the assertion):

  kernel                           red.  cases  rms kernel / naive   max kernel / naive   worst ratio rms, max
  forward, split-bf16 (kernel 0)      4      2  7.73e-09 / 9.48e-09  6.54e-08 / 8.02e-08  0.82, 0.82
  forward, split-bf16 (kernel 0)     12      5  1.28e-08 / 2.16e-08  1.37e-07 / 1.49e-07  0.59, 0.92
  forward, split-bf16 (kernel 0)     32      2  3.61e-08 / 5.44e-08  5.10e-07 / 5.78e-07  0.66, 0.88
  forward, split-bf16 (kernel 0)     36      3  4.04e-08 / 6.19e-08  3.36e-07 / 4.58e-07  0.65, 0.74
  forward, split-bf16 (kernel 0)     68      7  5.96e-08 / 1.12e-07  6.81e-07 / 1.16e-06  0.53, 0.59
  forward, split-bf16 (kernel 0)     96      5  7.06e-08 / 1.55e-07  6.05e-07 / 1.43e-06  0.45, 0.42
  forward, split-bf16 (kernel 0)    100      2  7.26e-08 / 1.59e-07  5.69e-07 / 1.27e-06  0.46, 0.45
  forward, split-bf16 (kernel 0)    192      2  1.12e-07 / 3.09e-07  1.20e-06 / 4.18e-06  0.36, 0.29
  forward, split-bf16 (kernel 0)    640      5  2.57e-07 / 9.97e-07  2.37e-06 / 8.65e-06  0.26, 0.27
  forward, fp32 (kernel 1)            4      2  8.53e-09 / 9.48e-09  1.57e-07 / 1.57e-07  0.90, 1.00
  forward, fp32 (kernel 1)           12      3  2.11e-08 / 2.30e-08  2.01e-07 / 2.01e-07  0.92, 1.00
  forward, fp32 (kernel 1)           32      2  5.26e-08 / 5.53e-08  7.68e-07 / 5.78e-07  0.95, 1.33
  forward, fp32 (kernel 1)           36      2  5.38e-08 / 5.99e-08  5.08e-07 / 4.58e-07  0.90, 1.11
  forward, fp32 (kernel 1)           68      3  7.80e-08 / 1.09e-07  8.72e-07 / 1.32e-06  0.71, 0.66
  forward, fp32 (kernel 1)           96      3  9.57e-08 / 1.55e-07  6.05e-07 / 1.43e-06  0.62, 0.42
  forward, fp32 (kernel 1)          100      2  9.80e-08 / 1.59e-07  7.61e-07 / 1.27e-06  0.62, 0.60
  forward, fp32 (kernel 1)          640      3  3.01e-07 / 1.01e-06  2.21e-06 / 8.65e-06  0.30, 0.26
  forward, fp32 mfma16 (kernel 2)     4      2  8.53e-09 / 9.48e-09  1.57e-07 / 1.57e-07  0.90, 1.00
  forward, fp32 mfma16 (kernel 2)    12      3  2.05e-08 / 2.16e-08  2.37e-07 / 2.01e-07  0.95, 1.18
  forward, fp32 mfma16 (kernel 2)    32      2  5.20e-08 / 5.44e-08  7.68e-07 / 5.78e-07  0.96, 1.33
  forward, fp32 mfma16 (kernel 2)    36      2  5.37e-08 / 5.99e-08  6.31e-07 / 4.58e-07  0.90, 1.38
  forward, fp32 mfma16 (kernel 2)    68      3  8.13e-08 / 1.12e-07  6.41e-07 / 8.70e-07  0.72, 0.74
  forward, fp32 mfma16 (kernel 2)    96      3  9.59e-08 / 1.55e-07  7.15e-07 / 1.43e-06  0.62, 0.50
  forward, fp32 mfma16 (kernel 2)   100      2  9.68e-08 / 1.59e-07  7.28e-07 / 1.27e-06  0.61, 0.57
  forward, fp32 mfma16 (kernel 2)   640      3  2.99e-07 / 1.01e-06  2.84e-06 / 1.05e-05  0.30, 0.27
  dA, split-bf16 (kernel 0)           2      6  6.07e-09 / 5.89e-09  6.55e-08 / 4.97e-08  1.03, 1.32
  dA, split-bf16 (kernel 0)           6      6  8.12e-09 / 1.35e-08  7.37e-08 / 9.24e-08  0.60, 0.80
  dA, split-bf16 (kernel 0)          32      6  3.99e-08 / 6.03e-08  3.97e-07 / 5.16e-07  0.66, 0.77
  dA, split-bf16 (kernel 0)          36      6  4.24e-08 / 6.70e-08  3.22e-07 / 4.41e-07  0.63, 0.73
  dA, split-bf16 (kernel 0)          64      6  6.26e-08 / 1.19e-07  4.11e-07 / 8.05e-07  0.53, 0.51
  dA, split-bf16 (kernel 0)         100      8  7.93e-08 / 1.74e-07  6.22e-07 / 1.17e-06  0.45, 0.53
  dA, split-bf16 (kernel 0)         128      8  9.06e-08 / 2.26e-07  5.28e-07 / 1.06e-06  0.40, 0.50
  dA, fp32 (kernel 1)                 6      6  1.07e-08 / 1.18e-08  2.12e-07 / 1.32e-07  0.91, 1.60
  dA, fp32 (kernel 1)               128      8  1.29e-07 / 2.24e-07  8.19e-07 / 1.35e-06  0.57, 0.61
  dA, fp32 (kernel 1)               256      8  1.88e-07 / 4.45e-07  9.62e-07 / 2.69e-06  0.42, 0.36
  dW ring + reduce                    1      1  1.59e-08 / 1.58e-08  5.57e-08 / 5.57e-08  1.01, 1.00
  dW ring + reduce                   15      2  1.47e-07 / 3.27e-07  4.73e-07 / 1.43e-06  0.45, 0.33
  dW ring + reduce                   16      1  1.19e-07 / 3.20e-07  3.50e-07 / 1.38e-06  0.37, 0.25
  dW ring + reduce                   17      2  3.58e-07 / 3.79e-07  1.06e-06 / 8.02e-07  0.94, 1.32
  dW ring + reduce                   63      1  7.57e-07 / 9.96e-07  2.10e-06 / 2.66e-06  0.76, 0.79
  dW ring + reduce                   64      2  6.94e-07 / 1.05e-06  2.95e-06 / 4.45e-06  0.66, 0.66
  dW ring + reduce                   65      7  7.91e-07 / 9.97e-07  9.95e-06 / 8.82e-06  0.79, 1.13
  dW ring + reduce                  200      2  1.81e-06 / 3.94e-06  5.37e-06 / 1.36e-05  0.46, 0.39
  dW ring + reduce                 1000      8  5.39e-06 / 1.80e-05  1.17e-05 / 5.31e-05  0.30, 0.22
  (red.: the reduction length -- K of the forward, 2d of the dA, the row count R of the dW; each row shows the
  case with the worst ratio.  The bound is 2.00; a lost product term measures 6x (K = 640) to 37x (K = 12).)
"""

import os
import subprocess
import sys

import pytest
import torch

import gemm_probe_util as U

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- repack
@pytest.mark.parametrize("d,k", [(1, 5), (3, 12), (16, 33), (32, 12), (64, 640)])
def test_repack(d, k):
    (wl, wr, bl, br), (wt, wc, bc, wc3, wt3) = U.run_repack(d, k)
    c2, c2p, kp = 2 * d, U.pad4(2 * d), U.pad4(k)
    wcat = torch.cat([wl, wr], dim=0)
    want_wc = torch.zeros(c2, kp)
    want_wc[:, :k] = wcat
    want_wt = torch.zeros(k, c2p)
    want_wt[:, :c2] = wcat.T
    assert U.bits_equal(wc, want_wc) and U.bits_equal(wt, want_wt)
    assert U.bits_equal(bc, torch.cat([bl, br]))
    want3 = torch.zeros(3, c2, U.ld3(kp), dtype=torch.bfloat16)
    wantt3 = torch.zeros(3, k, U.ld3(c2p), dtype=torch.bfloat16)
    for pl, part in enumerate(U.split3(wcat)):
        want3[pl, :, :k] = part
        wantt3[pl, :, :c2] = part.T
    for got, want in ((wc3, want3), (wt3, wantt3)):
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))


# ---------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("k", U.FWD_K)
@pytest.mark.parametrize("kernel", [0, 1, 2])
def test_forward(kernel, k):
    cases = [c for c in U.fwd_cases(kernel) if c["k"] == k]
    assert cases
    for c in cases:
        U.check_fwd(c)


def test_forward_narrow_n_and_diag_columns():
    for c in U.fwd_special_cases():
        U.check_fwd(c)


def test_forward_no_rows_finalizes_empty_statistics():
    """M = 0 under the in-GEMM finalize: mean 0, std sqrt(1e-5), the running statistics updated with them, nothing
    written to Y, the ticket left 0."""
    c = dict(kernel=0, k=36, m=0, cap=64, n=64, relu=32, fam="E1", wide="l", bn=3, c=0, seed=7)
    A, W, bias, dg, op = U.fwd_inputs(c)
    run = (torch.linspace(-1, 1, 64), torch.linspace(0.5, 1.5, 64))
    r, y, mean, std, rm, rs, tick = U.call_fwd(c, A, W, bias, dg, run)
    assert r == 0
    assert U.bits_equal(y, torch.tensor(U.SENT).expand_as(y))
    assert U.bits_equal(mean[:64], torch.zeros(64))
    assert U.ulp_dist(std[:64], torch.full((64,), 1e-5, dtype=torch.float64).sqrt().float()).max() <= 2
    U.check_bn("fwd-no-rows", c, y, mean, std, rm, rs, run, tick)


def test_forward_fp32_kernels_refuse_what_they_lack():
    c = dict(kernel=1, k=36, m=65, cap=128, n=64, relu=32, fam="E1", wide="l", bn=2, c=0, seed=8)
    A, W, bias, dg, op = U.fwd_inputs(c)
    assert U.call_fwd(c, A, W, bias, dg)[0] == 2  # HGNN_ERR_UNSUPPORTED: no fp64 statistics in the fp32 GEMMs


# ---------------------------------------------------------------------------------------------- dA
@pytest.mark.parametrize("kernel,c2", [(0, c2) for c2 in U.DA_C2_BF3] + [(1, c2) for c2 in U.DA_C2_FP32])
def test_da(kernel, c2):
    cases = [c for c in U.da_cases(kernel) if c["c2"] == c2]
    assert cases
    for c in cases:
        U.check_da(c)


# ---------------------------------------------------------------------------------------------- dW + reduce
@pytest.mark.parametrize("r", sorted({c["r"] for c in U.dw_cases()}))
def test_dw(r):
    for c in U.dw_cases():
        if c["r"] == r:
            U.check_dw(c)


# ---------------------------------------------------------------------------------------------- switches
GROUPS = {
    "ring2": {"HGNN_DW_RING": "2"},
    "ring3": {"HGNN_DW_RING": "3"},
    "fp32_dw_no_dma": {"HGNN_DW_BF3": "0", "HGNN_GEMM_DMA": "0", "HGNN_FWD_G5": "0"},
    "g5_always_linear": {"HGNN_FWD_G5": "2", "HGNN_FWD_XCD": "0", "HGNN_DA_XCD": "0", "HGNN_DW_XCD": "0"},
}


def test_switch_selected_variants():
    """The kernel variants only a switch selects, each group in a fresh child process, one after another."""
    for name, extra in GROUPS.items():
        env = {k: v for k, v in os.environ.items() if not k.startswith("HGNN_")}
        env.update(extra)
        env["HGNN_STRICT"] = "1"
        r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "gemm_probe_worker.py")], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (name, r.stderr[-2000:])
