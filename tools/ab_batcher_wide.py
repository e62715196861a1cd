"""Same-process A/B of the batcher behind the GNN epoch loops on node graphs of up to 64 nodes (tools/ab_batcher.py's
protocol: passes alternating between the paths, 10 timed passes after 2 warm-up passes, min and median ms per pass).

  config1    GNN_simple(0, 2, 20, 5, 1, 1) on 200 sbm_dataset(n=50) graphs, bs = 32: TrainStep.train_epoch and
             eval_epoch from the GraphPack (the host batcher per batch: densify A, hgnn_csr_batch_plan + _build, one
             H2D copy) against the same calls on the DevicePack(J=1, dual=False)
  generated  the same model and epochs on 200 three_collinear_points graphs (3..49 nodes), bs = 30; the label as a
             float is the one target column, so the regression step runs
  build      DevicePack.batch alone, per batch of 32 SBM-50 graphs at J = 1, 2, 3: HIP events around the builds of
             one pass over the pack
  narrow     the non-dual QM9-shape build at bs = 64 by HIP events (batches the narrow kernel builds), each run in a
             child process of its own; with --parent-lib (a libhgnn_amd.so built from the parent commit) the runs
             alternate between this tree's library and that one, --narrow-runs each
             (HGNN_LIB_PATH in the caller's environment still chooses the library of the other three sections)

One JSON line, also written to --out (default profiles/device_batcher_wide_ab.json).  The tool holds no expectation."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "hgnn-2_amd"), REPO, os.path.join(REPO, "tools")]

MEAN, STD = 0.3, 1.7
GRAPHS = 200
MODEL = (0, 2, 20, 5, 1, 1)  # BASELINE config 1; scripts/main_gnn.py's defaults: L = 20, h = 2, J = 1
NARROW_BATCHES, NARROW_BS = 16, 64


def _stat(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}


def build_alone(dev_pack, bs):
    """ms per batch: events around the builds of one pass over the pack, nothing else on the stream."""
    import torch
    parts = [list(range(b0, min(b0 + bs, len(dev_pack)))) for b0 in range(0, len(dev_pack), bs)]
    per = []
    for it in range(12):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        keep = [dev_pack.batch(p, 0) for p in parts]
        e1.record()
        host = (time.perf_counter() - t0) * 1e3
        e1.synchronize()
        if it >= 2:
            per.append((e0.elapsed_time(e1) / len(parts), host / len(parts)))
        del keep
    return {"device_ms_per_batch": _stat([p[0] for p in per]), "host_enqueue_ms_per_batch": _stat([p[1] for p in per]),
            "batches": len(parts), "bs": bs}


def narrow_only():
    """The child process: one JSON line with the narrow build's figures for whichever library HGNN_LIB_PATH names."""
    import hgnn_amd.datagen as dg
    from hgnn_amd.dataset import GraphPack
    tmp = tempfile.mkdtemp(prefix="ab_batcher_wide_")
    pack = GraphPack.write(os.path.join(tmp, "qm9"), dg.qm9_shape_dataset(NARROW_BATCHES * NARROW_BS, seed=7))
    res = build_alone(pack.to_device(J=1, dual=False), NARROW_BS)
    shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))


def narrow_runs(parent_lib, runs):
    """Fresh child processes, one at a time, alternating between the libraries."""
    out = {"tree": [], "parent": []}
    for _ in range(runs):
        for name, lib in (("tree", None), ("parent", parent_lib)):
            if name == "parent" and not lib:
                continue
            env = dict(os.environ)
            env.pop("HGNN_LIB_PATH", None)
            if lib:
                env["HGNN_LIB_PATH"] = os.path.abspath(lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-narrow"], env=env, check=True,
                               capture_output=True, text=True, timeout=300)
            out[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
    return out


def epochs(graph_pack, bs):
    """Alternating train / eval epochs from the GraphPack and from its DevicePack."""
    import torch
    from hgnn_amd.train import TrainStep
    from models.gnns.model_mnb import GNN_simple
    torch.manual_seed(0)
    dev_pack = graph_pack.to_device(J=MODEL[5], dual=False)
    flagged = int((dev_pack.counts[:, 8] != 0).sum())
    step = TrainStep(GNN_simple(*MODEL).cuda(), t_mean=MEAN, t_std=STD)
    paths = {"train_epoch_graphpack": lambda: step.train_epoch(graph_pack, 0, bs),
             "train_epoch_devicepack": lambda: step.train_epoch(dev_pack, 0, bs),
             "eval_epoch_graphpack": lambda: step.eval_epoch(graph_pack, 0, bs),
             "eval_epoch_devicepack": lambda: step.eval_epoch(dev_pack, 0, bs)}
    times = {k: [] for k in paths}
    for it in range(12):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= 2:
                times[k].append((time.perf_counter() - t0) * 1e3)
    res = {f"{k}_ms_per_pass": _stat(v) for k, v in times.items()}
    res.update(graphs=len(graph_pack), bs=bs, batches=-(-len(graph_pack) // bs), flagged_graphs=flagged,
               passes=len(times["train_epoch_graphpack"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "device_batcher_wide_ab.json"))
    ap.add_argument("--parent-lib", default=None, help="libhgnn_amd.so of the parent commit, for the narrow line")
    ap.add_argument("--narrow-runs", type=int, default=3)
    ap.add_argument("--only-narrow", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.only_narrow:
        return narrow_only()
    # the children first, one at a time, while this process has not touched the GPU
    narrow = narrow_runs(args.parent_lib, args.narrow_runs)
    import torch
    import hgnn_amd.datagen as dg
    from hgnn_amd.dataset import GraphPack
    tmp = tempfile.mkdtemp(prefix="ab_batcher_wide_")
    sbm = GraphPack.write(os.path.join(tmp, "sbm"), dg.sbm_dataset(GRAPHS, n=50, seed=7))
    gen = GraphPack.write(os.path.join(tmp, "gen"), [(x, a, y.to(torch.float32)) for x, a, y, *_ in
                                                     dg.three_collinear_points(GRAPHS, seed=7)])
    res = {"config1": epochs(sbm, 32), "generated": epochs(gen, 30),
           "build_alone_sbm50_bs32": {f"J{J}": build_alone(sbm.to_device(J=J, dual=False), 32) for J in (1, 2, 3)},
           "narrow_qm9_bs64": narrow, "model": f"GNN_simple{MODEL}"}
    shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
