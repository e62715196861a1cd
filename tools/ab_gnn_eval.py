"""Same-process A/B of the GNN evaluation loop (test_with_mnb, scripts/test_mnb.py:25-92): passes over the same 16
batches of 64 QM9-shape graphs with GNN_lg(order 2, d = 64, L = 5) alternate between

  reference   the drop-in model under the reference's loop: per batch the forward in eval mode, then
              criterion(output, T).item() and utils.evaluation(output, T).item() into two AverageMeters -- two host
              synchronisations per batch
  device      hgnn_amd.train.TrainStep: evaluate(batch) per batch (hgnn_eval_loss accumulates the meters on the
              device), one eval_result() at the end -- one host read per pass

in two settings: "batches" runs both on the same pre-built dense device batches, so the difference is the per-batch
synchronisation alone; "epoch" is the whole call from a list of instances, batching included -- test_with_mnb with
prepare_batch and .cuda() per batch against TrainStep.eval_epoch, once with its default native CsrBatch per batch
(the operators are rebuilt from A, the instances' stored W / WL / Pm / Pd are not read) and once with dense=True
(the same prepare_batch as the reference's loop).  Per path the min and median ms per pass over 10 timed passes
(after 2 warm-up passes), printed as one JSON line and written to profiles/gnn_eval_ab.json.  The tool holds no
expectation."""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "hgnn-2_amd"), REPO, os.path.join(REPO, "tools")]
import torch  # noqa: E402

MEAN, STD = 0.3, 1.7
BATCHES, BS, D, LAYERS = 16, 64, 64, 5


def main():
    import hgnn_amd.datagen as dg
    from functions.batching import get_batches, prepare_batch
    from functions.operators import graph_operators
    from functions.utils import AverageMeter, evaluation, normalize_data
    from hgnn_amd.train import TrainStep
    from models.gnns.model_mnb import GNN_lg
    torch.manual_seed(0)
    graphs = dg.qm9_shape_dataset(BATCHES * BS, seed=7)
    data = [[x, a, t, *graph_operators([x, a], 1, True)] for x, a, t in graphs]
    model = GNN_lg(0, D, LAYERS, 5, 1, 1, 2).cuda()
    step = TrainStep(model, t_mean=MEAN, t_std=STD)
    idx = get_batches(len(data), BS, data, False, False)
    dense = [[t.cuda() for t in prepare_batch([data[j] for j in b], 0, 1)] for b in idx]
    step(dense[0])  # one training step: running statistics off their initial zeros
    crit = torch.nn.MSELoss()

    def reference_batch(b, loss, error):
        X, W, T, XL, WL, Pm, Pd, mask, mask_lg, Nb, Eb = b
        out = model([X, XL, W, WL, Pm, Pd], Nb, mask, Eb, mask_lg)
        loss.update(crit(out, T).item(), X.shape[0])
        error.update(evaluation(out, T).item(), X.shape[0])

    def reference_batches():
        loss, error = AverageMeter(), AverageMeter()
        model.eval()
        with torch.no_grad():
            for b in dense:
                X, W, T, XL, WL, Pm, Pd, mask, mask_lg, Nb, Eb = b
                reference_batch([X, W, normalize_data(T, MEAN, STD), XL, WL, Pm, Pd, mask, mask_lg, Nb, Eb], loss,
                                error)
        return loss.avg, error.avg

    def device_batches():
        step.reset_eval()
        for b in dense:
            step.evaluate(b)
        return step.eval_result()

    def reference_epoch():
        loss, error = AverageMeter(), AverageMeter()
        model.eval()
        with torch.no_grad():
            for b in idx:
                X, W, T, XL, WL, Pm, Pd, mask, mask_lg, Nb, Eb = prepare_batch([data[j] for j in b], 0, model.J)
                T = normalize_data(T, MEAN, STD)
                reference_batch([t.cuda() for t in (X, W, T, XL, WL, Pm, Pd, mask, mask_lg, Nb, Eb)], loss, error)
        return loss.avg, error.avg

    paths = {"batches_reference": reference_batches, "batches_device": device_batches,
             "epoch_reference": reference_epoch, "epoch_device": lambda: step.eval_epoch(data, 0, BS),
             "epoch_device_dense": lambda: step.eval_epoch(data, 0, BS, dense=True)}
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
    res = {f"{k}_ms_per_pass": {"min": round(min(v), 4), "median": round(statistics.median(v), 4)}
           for k, v in times.items()}
    res.update(batches=BATCHES, bs=BS, d=D, layers=LAYERS, order=2, passes=len(times["batches_device"]),
               host_reads_per_pass={"reference": 2 * BATCHES, "device": 1},
               loss_avg={k: v[0] for k, v in results.items()}, error_avg={k: v[1] for k, v in results.items()})
    print(json.dumps(res))
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "gnn_eval_ab.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
