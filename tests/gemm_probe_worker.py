"""Worker of tests/test_gpu_gemm_kernels.py::test_switch_selected_variants (a child process: the library reads its
HGNN_* switches once per process).  Runs the dW cases and the fp32-selector (kernel = 1, 2) forward and dA cases of
tests/gemm_probe_util.py's case tables under the switches of its environment; exits nonzero naming the first
failing case."""

import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "hgnn-2_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import gemm_probe_util as U
    done = 0
    try:
        for c in U.dw_cases():
            U.check_dw(c)
            done += 1
        for kernel in (1, 2):
            for c in U.fwd_cases(kernel):
                U.check_fwd(c)
                done += 1
        for c in U.da_cases(1):
            U.check_da(c)
            done += 1
    except AssertionError as e:
        print(f"FAILED after {done} cases: {e}", file=sys.stderr)
        return 1
    print(f"{done} cases ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
