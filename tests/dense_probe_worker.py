"""Worker of tests/test_gpu_dense_kernels.py::test_switch_selected_variants (a child process: the library reads its
HGNN_* switches once per process).  argv[1] names a mode of tests/dense_probe_util.py run_worker_mode: the BN-backward
tables of the narrow / wide widths (the expected launch sequence follows HGNN_BN_BWD2 of this process's environment)
or a part of the dense-dW table.  Exits nonzero naming the first failing case."""

import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "hgnn-2_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import dense_probe_util as U
    env = {k: v for k, v in os.environ.items() if k.startswith("HGNN_")}
    try:
        done = U.run_worker_mode(sys.argv[1], env)
    except AssertionError as e:
        print(f"FAILED: {e}", file=sys.stderr)
        return 1
    print(f"{done} cases ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
