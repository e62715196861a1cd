"""Same-process A/B of where a CCN epoch's chunks come from (tools/ab_ccn_train.py's protocol): epochs over the
same 256 QM9-shape graphs alternate between three inputs of CcnTrainStep.train_epoch / eval_epoch,

  list         the reference's 7-tuples through CcnTrainStep._chunks: per graph six small torch operations on the
               host, then one H2D copy of the chunk's four tensors
  graph_pack   hgnn_amd.dataset.GraphPack.ccn_chunks: the chunk gathered in numpy from the mapped arrays, then the
               same H2D copy
  device_pack  hgnn_amd.dataset.DevicePack.ccn_chunks: hgnn_pack_ccn_chunk on the resident pack, no host work per
               graph

for CCN_1D(5, 1, 2, 2) on the fused path (hgnn_ccn_small_train) and CCN_2D(5, 1, 2, 2) on fused2d
(hgnn_ccn2_small_train), each input on its own copy of the model.  Per model, operation and input the min and median
ms per graph over 10 epochs (12 run, the first 2 dropped), host clock around a synchronised epoch.  The chunk build
alone: the host clock around the two host builds (up to the tensors on the device), and HIP events around
DevicePack.ccn_chunk (the index upload and the kernel).  One JSON line, also written to profiles/ccn_pack_ab.json.
The tool holds no expectation."""
import copy
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "hgnn-2_amd"), REPO, os.path.join(REPO, "tools")]
import torch  # noqa: E402

MEAN, STD, LR = 0.3, 1.7, 1e-3
GRAPHS, RUNS, DROP = 256, 12, 2


def _summary(v, per):
    return {"min": round(min(v) / per, 5), "median": round(statistics.median(v) / per, 5)}


def main():
    import hgnn_amd.datagen as dg
    from hgnn_amd.dataset import GraphPack
    from hgnn_amd.train import CcnTrainStep
    from models.compnets.model_ccn import CCN_1D, CCN_2D
    graphs = dg.qm9_shape_dataset(GRAPHS, seed=7)
    nmax = max(x.shape[0] for x, _, _ in graphs)
    res = {"graphs": GRAPHS, "nmax": nmax, "epochs": RUNS - DROP, "chunk": 1024}
    with tempfile.TemporaryDirectory() as tmp:
        pack = GraphPack.write(os.path.join(tmp, "pack"), graphs)
        inputs = {"list": [[x, a, t, None, None, None, None] for x, a, t in graphs], "graph_pack": pack,
                  "device_pack": pack.to_device(J=None)}
        torch.manual_seed(0)
        for model, net, fused in (("ccn1d", CCN_1D(5, 1, 2, 2).cuda(), True),
                                  ("ccn2d", CCN_2D(5, 1, 2, 2).cuda(), "ccn2")):
            steps = {k: CcnTrainStep(copy.deepcopy(net), lr=LR, t_mean=MEAN, t_std=STD, fused=fused) for k in inputs}
            for op in ("train_epoch", "eval_epoch"):
                times = {k: [] for k in inputs}
                for it in range(RUNS):
                    for k, data in inputs.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        getattr(steps[k], op)(data, 0)
                        torch.cuda.synchronize()
                        if it >= DROP:
                            times[k].append((time.perf_counter() - t0) * 1e3)
                res[f"{model}_{op}_ms_per_graph"] = {k: _summary(v, GRAPHS) for k, v in times.items()}
            res[f"{model}_path"] = {k: s.path for k, s in steps.items()}

        # the chunk build alone, all 256 graphs as one chunk
        st = steps["list"]
        dp = inputs["device_pack"]
        idx = list(range(GRAPHS))
        builds = {"list": lambda: list(st._chunks(inputs["list"], 0, GRAPHS)),
                  "graph_pack": lambda: list(pack.ccn_chunks(idx, GRAPHS, 0, device="cuda")),
                  "device_pack": lambda: dp.ccn_chunk(idx, 0)}
        host = {k: [] for k in builds}
        events = []
        for it in range(RUNS):
            for k, fn in builds.items():
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                if it >= DROP:
                    host[k].append((time.perf_counter() - t0) * 1e3)
                    if k == "device_pack":
                        events.append(a.elapsed_time(b))
        res["chunk_build_host_ms"] = {k: _summary(v, 1) for k, v in host.items()}
        res["chunk_build_device_pack_events_ms"] = _summary(events, 1)
        dp.check()
    print(json.dumps(res))
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "ccn_pack_ab.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
