"""Worker of tests/test_gpu_sparse_kernels.py::test_switch_selected_variants (a child process: the library reads its
HGNN_* switches once per process).  argv[1] = "agg_fwd": the aggregation forward cases (general and diagonal mode) of
tests/sparse_probe_util.py; "extract": the extraction cases, argv[2] the kernel launch_extract must report per shape
(comma-separated).  Exits nonzero naming the first failing case."""

import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "hgnn-2_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import sparse_probe_util as U
    mode = sys.argv[1]
    try:
        if mode == "agg_fwd":
            done = U.run_fwd_cases()
        elif mode == "extract":
            done = U.run_extract_cases(tuple(int(x) for x in sys.argv[2].split(",")))
        else:
            print(f"unknown mode {mode}", file=sys.stderr)
            return 2
    except AssertionError as e:
        print(f"FAILED: {e}", file=sys.stderr)
        return 1
    print(f"{done} cases ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
