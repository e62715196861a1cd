"""Same-process A/B of the batcher behind the GNN epoch loops (tools/ab_gnn_eval.py's protocol): GNN_lg(order 2,
d = 64, L = 5) on QM9-shape graphs, passes alternating between the paths, 10 timed passes after 2 warm-up passes,
min and median ms per pass.

  eval     TrainStep.eval_epoch over 16 batches of 64 from a GraphPack (the host batcher per batch: densify A,
           hgnn_csr_batch_plan + _build, one H2D copy) against the same call on a DevicePack (the pack resident,
           hgnn_csr_batch_build_device per batch), next to evaluate() over pre-built batches, dense and CSR (no
           batching at all: the floor)
  train    TrainStep.train_epoch at bs = 512 over 8 batches, from the GraphPack and from the DevicePack
  build    DevicePack.batch alone, per batch at bs = 64 and bs = 512: HIP events around 16 (8) builds in a row

One JSON line, also written to --out (default profiles/device_batcher_ab.json).  The tool holds no expectation."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "hgnn-2_amd"), REPO, os.path.join(REPO, "tools")]
import torch  # noqa: E402

MEAN, STD = 0.3, 1.7
D, LAYERS = 64, 5
EVAL_BATCHES, EVAL_BS = 16, 64
TRAIN_BATCHES, TRAIN_BS = 8, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "device_batcher_ab.json"))
    args = ap.parse_args()
    import hgnn_amd.datagen as dg
    from functions.batching import get_batches, prepare_batch
    from functions.operators import graph_operators
    from hgnn_amd.dataset import GraphPack
    from hgnn_amd.train import TrainStep
    from models.gnns.model_mnb import GNN_lg
    torch.manual_seed(0)
    tmp = tempfile.mkdtemp(prefix="ab_batcher_")
    eval_graphs = dg.qm9_shape_dataset(EVAL_BATCHES * EVAL_BS, seed=7)
    eval_pack = GraphPack.write(os.path.join(tmp, "eval"), eval_graphs)
    train_pack = GraphPack.write(os.path.join(tmp, "train"), dg.qm9_shape_dataset(TRAIN_BATCHES * TRAIN_BS, seed=8))
    eval_dev, train_dev = eval_pack.to_device(), train_pack.to_device()
    model = GNN_lg(0, D, LAYERS, 5, 1, 1, 2).cuda()
    step = TrainStep(model, t_mean=MEAN, t_std=STD)
    idx = get_batches(len(eval_graphs), EVAL_BS, eval_graphs, False, False)
    data = [[x, a, t, *graph_operators([x, a], 1, True)] for x, a, t in eval_graphs]
    dense = [[t.cuda() for t in prepare_batch([data[j] for j in b], 0, 1)] for b in idx]
    csr = list(eval_dev.batches(range(len(eval_pack)), EVAL_BS, 0))
    step(dense[0])  # one training step: running statistics off their initial zeros

    def prebuilt(batches):
        step.reset_eval()
        for b in batches:
            step.evaluate(b)
        return step.eval_result()

    paths = {"eval_prebuilt_dense": lambda: prebuilt(dense), "eval_prebuilt_csr": lambda: prebuilt(csr),
             "eval_epoch_graphpack": lambda: step.eval_epoch(eval_pack, 0, EVAL_BS),
             "eval_epoch_devicepack": lambda: step.eval_epoch(eval_dev, 0, EVAL_BS),
             "train_epoch_graphpack": lambda: step.train_epoch(train_pack, 0, TRAIN_BS),
             "train_epoch_devicepack": lambda: step.train_epoch(train_dev, 0, TRAIN_BS)}
    times = {k: [] for k in paths}
    results = {}
    for it in range(12):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results[k] = fn()
            torch.cuda.synchronize()
            if it >= 2:
                times[k].append((time.perf_counter() - t0) * 1e3)

    def build_alone(pack, bs):
        """ms per batch: events around the builds of one pass over the pack, nothing else on the stream."""
        parts = [list(range(b0, b0 + bs)) for b0 in range(0, len(pack), bs)]
        per = []
        for it in range(12):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            keep = [pack.batch(p, 0) for p in parts]
            e1.record()
            host = (time.perf_counter() - t0) * 1e3
            e1.synchronize()
            if it >= 2:
                per.append((e0.elapsed_time(e1) / len(parts), host / len(parts)))
            del keep
        return {"device_ms_per_batch": {"min": round(min(p[0] for p in per), 4),
                                        "median": round(statistics.median(p[0] for p in per), 4)},
                "host_enqueue_ms_per_batch": {"min": round(min(p[1] for p in per), 4),
                                              "median": round(statistics.median(p[1] for p in per), 4)},
                "batches": len(parts), "bs": bs}

    res = {f"{k}_ms_per_pass": {"min": round(min(v), 4), "median": round(statistics.median(v), 4)}
           for k, v in times.items()}
    res["build_alone"] = {"bs64": build_alone(eval_dev, EVAL_BS), "bs512": build_alone(train_dev, TRAIN_BS)}
    res.update(d=D, layers=LAYERS, order=2, passes=len(times["eval_prebuilt_csr"]),
               eval={"batches": EVAL_BATCHES, "bs": EVAL_BS}, train={"batches": TRAIN_BATCHES, "bs": TRAIN_BS},
               eval_results={k: v for k, v in results.items() if k.startswith("eval")})
    shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
