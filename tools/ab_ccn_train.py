"""Same-process A/B of the per-graph CCN training loop (scripts/train_ccn.py:31-73): epochs over the same 256
QM9-shape graphs alternate between three paths,

  torch     net(x, a), nn.MSELoss, torch.optim.Adamax per graph (the drop-in model under the reference's loop)
  unfused   hgnn_amd.train.CcnTrainStep(fused=False): forward_batch, hgnn_mse_loss, backward, hgnn_adamax_step
  fused     CcnTrainStep(fused=True): hgnn_ccn_small_train, one dispatch per epoch

each on its own copy of CCN_1D(5, 1, 2, 2).  Per path the min, median and max ms per graph over the epochs, printed
as one JSON line and written to profiles/ccn_train_ab.json.  The tool holds no expectation.

--loss xent: the classification branch (train_ccn.py:39-41, 56-57) on the generated driver's task
(scripts/main_generate_ccn.py): three_collinear_points(256, n_max=30, seed=0) with CCN_1D(5, 2, 2, 10),
nn.CrossEntropyLoss on out.view(1, -1), hgnn_xent_loss / hgnn_ccn_small_train_xent; written to
profiles/ccn_train_xent_ab.json.

--order 2: the same three paths for CCN_2D(5, 1, 2, 2) on the same 256 QM9-shape graphs, the fused path being
CcnTrainStep(fused="ccn2"): hgnn_ccn2_small_train; written to profiles/ccn2_train_ab.json.  With --loss xent:
CCN_2D(5, 2, 2, 2) on those graphs with the label g % 2, written to profiles/ccn2_train_xent_ab.json.

--optim sgd|adam|adamax (--momentum, default 0.9): the drivers' other optimizers (scripts/main_ccn.py:155-162) on
all three paths -- torch.optim.SGD(momentum) / Adam / Adamax, hgnn_optim_step, and the fused kernels'
hgnn_ccn_small_train_opt / hgnn_ccn2_small_train_opt (adamax: the Adamax entries).  The result is merged into
profiles/ccn_train_optim_ab.json under the key "order<N>_<loss>_<optim>"; the files above are left alone.

--batch B [B ...] (e.g. --batch 32 256): mini-batch training, CcnTrainStep(batch_size=B), on the same graphs under the
same protocol -- the per-graph fused loop (order 2: fused2d) against, per B, the pieces route (fused=False) and the
mini-batch kernels (order 1: fused=True, hgnn_ccn_small_train_batch, arm batch_fused_B<B>; order 2:
fused="ccn2_batch", hgnn_ccn2_small_train_batch, arm batch_fused2d_B<B>); no torch arm.  Median, min and max ms per
graph, merged into profiles/ccn_train_batch_ab.json under the key "order<N>_<loss>_<optim>".

--spill: the spill instantiation of the CCN-1D kernels (CcnTrainStep(fused="ccn1_spill"): the row arrays in a global
workspace) under the same protocol, two sections in one process, written to profiles/ccn_train_spill_ab.json:
  replaces   256 three_collinear_points(n_max=50) graphs, CCN_1D(5, 2, 2, 8), classification -- shapes the LDS kernels
             refuse: the spill loop against fused=False, and spill mini-batches at B = 32 and 256 against the pieces;
  lds_price  the 256 QM9-shape graphs, CCN_1D(5, 1, 2, 2), MSE -- shapes both take: the spill loop and spill
             mini-batches at B = 32 against the LDS kernels."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "hgnn-2_amd"), REPO, os.path.join(REPO, "tools")]
import torch  # noqa: E402

MEAN, STD, LR = 0.3, 1.7, 1e-3


def batch_arms(args, net, inputs, stats, optim, nmax):
    """--batch B [B ...]: an epoch over the same graphs as mini-batches (CcnTrainStep(batch_size=B)) against the
    per-graph fused loop, arms alternating in one process, 2 warm-up and 10 timed epochs each."""
    from hgnn_amd.train import CcnTrainStep
    two = args.order == 2
    kw = dict(lr=LR, optimizer=optim, momentum=args.momentum, **stats)
    arms = {"per_graph_fused2d" if two else "per_graph_fused":
            CcnTrainStep(copy.deepcopy(net), fused="ccn2" if two else True, **kw)}
    for B in args.batch:
        arms[f"batch_pieces_B{B}"] = CcnTrainStep(copy.deepcopy(net), fused=False, batch_size=B, **kw)
        if two:
            arms[f"batch_fused2d_B{B}"] = CcnTrainStep(copy.deepcopy(net), fused="ccn2_batch", batch_size=B, **kw)
        else:
            arms[f"batch_fused_B{B}"] = CcnTrainStep(copy.deepcopy(net), fused=True, batch_size=B, **kw)
    G = inputs[0].shape[0]
    times = {k: [] for k in arms}
    for it in range(12):
        for k, st in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st.step(*inputs)
            torch.cuda.synchronize()
            if it >= 2:
                times[k].append((time.perf_counter() - t0) * 1e3 / G)
    res = {f"{k}_ms_per_graph": {"min": round(min(v), 5), "median": round(statistics.median(v), 5),
                                 "max": round(max(v), 5)} for k, v in times.items()}
    res.update(paths={k: st.path for k, st in arms.items()}, loss=args.loss, order=args.order, graphs=G, nmax=nmax,
               epochs=len(next(iter(times.values()))), optim=optim, batch=list(args.batch))
    print(json.dumps(res))
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    path = os.path.join(REPO, "profiles", "ccn_train_batch_ab.json")
    merged = {}
    if os.path.exists(path):
        with open(path) as f:
            merged = json.load(f)
    merged[f"order{args.order}_{args.loss}_{optim}"] = res
    with open(path, "w") as f:
        json.dump(merged, f, indent=1, sort_keys=True)
        f.write("\n")


def _pad(graphs):
    nmax = max(x.shape[0] for x, _, _ in graphs)
    X = torch.zeros(len(graphs), nmax, graphs[0][0].shape[1])
    A = torch.zeros(len(graphs), nmax, nmax)
    for b, (x, a, _) in enumerate(graphs):
        n = x.shape[0]
        X[b, :n] = x
        A[b, :n, :n] = a + torch.eye(n)
    nb = torch.tensor([x.shape[0] for x, _, _ in graphs], dtype=torch.int64)
    Y = torch.stack([t[0] for _, _, t in graphs]).view(-1, 1)
    return (X.cuda(), A.cuda(), nb.cuda(), Y.cuda()), nmax


def _alternate(arms, inputs):
    """2 warm-up and 10 timed epochs per arm, arms alternating: {arm: min / median / max ms per graph}, paths."""
    G = inputs[0].shape[0]
    times = {k: [] for k in arms}
    for it in range(12):
        for k, st in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st.step(*inputs)
            torch.cuda.synchronize()
            if it >= 2:
                times[k].append((time.perf_counter() - t0) * 1e3 / G)
    res = {f"{k}_ms_per_graph": {"min": round(min(v), 5), "median": round(statistics.median(v), 5),
                                 "max": round(max(v), 5)} for k, v in times.items()}
    res.update(paths={k: st.path for k, st in arms.items()}, graphs=G, epochs=10)
    return res


def spill_arms():
    """--spill: see the module docstring."""
    import hgnn_amd.datagen as dg
    from hgnn_amd.train import CcnTrainStep
    from models.compnets.model_ccn import CCN_1D
    out = {}
    # the routes it replaces, on shapes the LDS kernels refuse
    graphs = [(d[0], d[1], d[2].float()) for d in dg.three_collinear_points(256, n_max=50, seed=0)]
    inputs, nmax = _pad(graphs)
    torch.manual_seed(0)
    net = CCN_1D(5, 2, 2, 8).cuda()
    kw = dict(lr=LR, classification=True)
    arms = {"loop_unfused": CcnTrainStep(copy.deepcopy(net), fused=False, **kw),
            "loop_spill": CcnTrainStep(copy.deepcopy(net), fused="ccn1_spill", **kw)}
    for B in (32, 256):
        arms[f"batch_pieces_B{B}"] = CcnTrainStep(copy.deepcopy(net), fused=False, batch_size=B, **kw)
        arms[f"batch_spill_B{B}"] = CcnTrainStep(copy.deepcopy(net), fused="ccn1_spill", batch_size=B, **kw)
    out["replaces"] = dict(_alternate(arms, inputs), model=[5, 2, 2, 8], loss="xent", nmax=nmax,
                           data="three_collinear_points(256, n_max=50, seed=0)")
    # the price of global rows, on shapes the LDS kernels take
    inputs, nmax = _pad(dg.qm9_shape_dataset(256, seed=7))
    torch.manual_seed(0)
    net = CCN_1D(5, 1, 2, 2).cuda()
    kw = dict(lr=LR, t_mean=MEAN, t_std=STD)
    arms = {"loop_lds": CcnTrainStep(copy.deepcopy(net), fused=True, **kw),
            "loop_spill": CcnTrainStep(copy.deepcopy(net), fused="ccn1_spill", **kw),
            "batch_lds_B32": CcnTrainStep(copy.deepcopy(net), fused=True, batch_size=32, **kw),
            "batch_spill_B32": CcnTrainStep(copy.deepcopy(net), fused="ccn1_spill", batch_size=32, **kw)}
    out["lds_price"] = dict(_alternate(arms, inputs), model=[5, 1, 2, 2], loss="mse", nmax=nmax,
                            data="qm9_shape_dataset(256, seed=7)")
    print(json.dumps(out))
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "ccn_train_spill_ab.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    import hgnn_amd.datagen as dg
    from hgnn_amd.train import CcnTrainStep
    from models.compnets.model_ccn import CCN_1D, CCN_2D
    ap = argparse.ArgumentParser()
    ap.add_argument("--loss", choices=("mse", "xent"), default="mse")
    ap.add_argument("--order", type=int, choices=(1, 2), default=1)
    ap.add_argument("--optim", choices=("sgd", "adam", "adamax"), default=None)
    ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--batch", type=int, nargs="+", default=None, metavar="B")
    ap.add_argument("--spill", action="store_true")
    args = ap.parse_args()
    if args.spill:
        return spill_arms()
    xent, two = args.loss == "xent", args.order == 2
    if xent and two:
        graphs = [(x, a, torch.tensor([float(g % 2)]))
                  for g, (x, a, _) in enumerate(dg.qm9_shape_dataset(256, seed=7))]
    elif xent:
        graphs = [(d[0], d[1], d[2].float()) for d in dg.three_collinear_points(256, n_max=30, seed=0)]
    else:
        graphs = dg.qm9_shape_dataset(256, seed=7)
    torch.manual_seed(0)
    if two:
        nets = {"torch": (CCN_2D(5, 2, 2, 2) if xent else CCN_2D(5, 1, 2, 2)).cuda()}
    else:
        nets = {"torch": (CCN_1D(5, 2, 2, 10) if xent else CCN_1D(5, 1, 2, 2)).cuda()}
    nets["unfused"] = copy.deepcopy(nets["torch"])
    nets["fused"] = copy.deepcopy(nets["torch"])
    optim = args.optim or "adamax"
    if optim == "sgd":
        opt = torch.optim.SGD(nets["torch"].parameters(), lr=LR, momentum=args.momentum)
    elif optim == "adam":
        opt = torch.optim.Adam(nets["torch"].parameters(), lr=LR)
    else:
        opt = torch.optim.Adamax(nets["torch"].parameters(), lr=LR)
    crit = torch.nn.CrossEntropyLoss() if xent else torch.nn.MSELoss()
    if xent:
        data = [(x.cuda(), (a + torch.eye(a.shape[0])).cuda(), t[0].view(1).long().cuda()) for x, a, t in graphs]
    else:
        data = [(x.cuda(), (a + torch.eye(a.shape[0])).cuda(), ((t[0].view(1) - MEAN) / (STD + 10 ** -8)).cuda())
                for x, a, t in graphs]
    nmax = max(x.shape[0] for x, _, _ in graphs)
    X = torch.zeros(len(graphs), nmax, 5)
    A = torch.zeros(len(graphs), nmax, nmax)
    for b, (x, a, _) in enumerate(graphs):
        n = x.shape[0]
        X[b, :n] = x
        A[b, :n, :n] = a + torch.eye(n)
    X, A = X.cuda(), A.cuda()
    nb = torch.tensor([x.shape[0] for x, _, _ in graphs], dtype=torch.int64).cuda()
    Y = torch.stack([t[0] for _, _, t in graphs]).view(-1, 1).cuda()
    stats = dict(classification=True) if xent else dict(t_mean=MEAN, t_std=STD)
    if args.batch:
        return batch_arms(args, nets["torch"], (X, A, nb, Y), stats, optim, nmax)
    steps = {k: CcnTrainStep(nets[k], lr=LR, fused=(k == "fused") and ("ccn2" if two else True), optimizer=optim,
                             momentum=args.momentum, **stats) for k in ("unfused", "fused")}

    def torch_epoch():
        net = nets["torch"]
        for x, a, y in data:
            opt.zero_grad()
            out = net(x, a)
            loss = crit(out.view(1, -1) if xent else out, y)
            loss.backward()
            opt.step()

    paths = {"torch": torch_epoch, "unfused": lambda: steps["unfused"].step(X, A, nb, Y),
             "fused": lambda: steps["fused"].step(X, A, nb, Y)}
    times = {k: [] for k in paths}
    for it in range(12):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= 2:
                times[k].append((time.perf_counter() - t0) * 1e3 / len(graphs))
    res = {f"{k}_ms_per_graph": {"min": round(min(v), 5), "median": round(statistics.median(v), 5),
                                 "max": round(max(v), 5)} for k, v in times.items()}
    res["loss"] = "xent" if xent else "mse"
    res["order"] = args.order
    res["fused_path"] = steps["fused"].path
    res["graphs"] = len(graphs)
    res["nmax"] = nmax
    res["epochs"] = len(times["fused"])
    res["optim"] = optim
    print(json.dumps(res))
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    if args.optim:
        path = os.path.join(REPO, "profiles", "ccn_train_optim_ab.json")
        merged = {}
        if os.path.exists(path):
            with open(path) as f:
                merged = json.load(f)
        merged[f"order{args.order}_{res['loss']}_{optim}"] = res
        with open(path, "w") as f:
            json.dump(merged, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    name = ("ccn2_train" if two else "ccn_train") + ("_xent_ab.json" if xent else "_ab.json")
    with open(os.path.join(REPO, "profiles", name), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
