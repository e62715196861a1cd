"""Device-resident evaluation of the GNNs: hgnn_eval_loss / hgnn_eval_xent and TrainStep.evaluate / eval_result /
eval_epoch / train_epoch against the reference's test_with_mnb (scripts/test_mnb.py:25-92: per batch a forward in
eval mode, criterion(...).item() and utils.evaluation(...).item() into two AverageMeters).

Tolerances: a loss or MAE average against torch's fp32 reductions, or against the fp64 oracle, within
1e-5 * max(1, |v|) -- the bound tests/test_gpu_train.py holds the training loss to.  Everything that compares the
kernels with themselves, with hgnn_mse_loss or with integer data is bit for bit.
"""

import copy
import os

import numpy as np
import pytest
import torch

import fixture_util as fu

pytestmark = pytest.mark.gpu

MEAN, STD = 0.3, 1.7


def _close(got, want):
    return abs(got - want) <= 1e-5 * max(1.0, abs(want))


def _capture(step):
    """Warm-up on a side stream, then capture (the helper of tests/test_gpu_graph.py)."""
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    return g


def _instances(graphs):
    from functions.operators import graph_operators
    return [[X, A, t, *graph_operators([X, A], 1, True)] for X, A, t in graphs]


def _batch(graphs, task=0):
    from functions.batching import prepare_batch
    return [t.cuda() for t in prepare_batch(_instances(graphs), task, 1)]


def _csr(graphs, dual=True, task=0):
    from hgnn_amd.csr import CsrBatch
    return CsrBatch([(x, a) for x, a, _ in graphs], J=1, dual=dual,
                    targets=torch.tensor([float(t[task]) for _, _, t in graphs]))


def _meters():
    return torch.zeros(6, dtype=torch.float64, device="cuda")


def _eval_loss(out, t, rows, dim, mean, std, m):
    from hgnn_amd import _lib as L
    L.check(L.lib().hgnn_eval_loss(L.ptr(out), L.ptr(t), rows, dim, mean, std, L.ptr(m), L.stream_handle(m.device)),
            "hgnn_eval_loss")


def _eval_xent(out, t, rows, c, m, err):
    from hgnn_amd import _lib as L
    L.check(L.lib().hgnn_eval_xent(L.ptr(out), L.ptr(t), rows, c, L.ptr(m), L.ptr(err), L.stream_handle(m.device)),
            "hgnn_eval_xent")


def _ints(rows, dim, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-7, 8, (rows, dim), generator=g).float(),
            torch.randint(-7, 8, (rows, dim), generator=g).float())


def _exact(out, t, mean=0.0, scale=1.0):
    """(loss, mae) of integer data as the kernel must form them: exact fp64 sums, one division, one rounding to
    fp32.  The normalised target (t - mean) * scale is an integer too."""
    d = out.double().numpy() - (t.double().numpy() - mean) * scale
    n = d.size
    S, A = np.float64((d * d).sum()), np.float64(np.abs(d).sum())
    return float(np.float32(S / n)), float(np.float32(A / n))


# ---------------------------------------------------------------- the kernels alone
@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257, 1000])
def test_eval_loss_exact_on_integers(rows, dim):
    out, t = _ints(rows, dim, 1000 * dim + rows)
    m = _meters()
    _eval_loss(out.cuda(), t.cuda(), rows, dim, 0.0, 1.0, m)
    loss, mae = _exact(out, t)
    assert m.tolist() == [loss * rows, mae * rows, float(rows), 0.0, loss, mae]


@pytest.mark.parametrize("dim", [1, 3])
def test_eval_loss_accumulates_like_average_meter(dim):
    """Batches of 24, 24 and 7 rows, an empty one in between: loss.sum, error.sum and count are the three
    AverageMeter.update(value, rows) calls in Python doubles, bit for bit ((double)loss * rows is exact -- 24 + 5
    bits -- so only the additions round)."""
    m = _meters()
    s0 = s1 = cnt = 0.0
    for k, rows in enumerate([24, 24, 0, 7]):
        if rows == 0:
            before = m.tolist()
            _eval_loss(m, m, 0, dim, 0.0, 1.0, m)  # valid pointers, nothing launched
            assert m.tolist() == before
            continue
        out, t = _ints(rows, dim, 50 + 10 * dim + k)
        _eval_loss(out.cuda(), t.cuda(), rows, dim, 0.0, 1.0, m)
        loss, mae = _exact(out, t)
        s0 += loss * rows
        s1 += mae * rows
        cnt += rows
        assert m.tolist() == [s0, s1, cnt, 0.0, loss, mae], k


@pytest.mark.parametrize("mean,std,scale", [(2.0, 1e-6, 1.0), (2.0, 0.5, 2.0)])
def test_eval_loss_normalises_the_target(mean, std, scale):
    """std < 1e-5: the mean only (functions/utils.py:84-95); (T - 2) / 0.5 is exact in fp32."""
    rows, dim = 65, 3
    out, t = _ints(rows, dim, 7)
    m = _meters()
    _eval_loss(out.cuda(), t.cuda(), rows, dim, mean, std, m)
    loss, mae = _exact(out, t, mean, scale)
    assert m.tolist() == [loss * rows, mae * rows, float(rows), 0.0, loss, mae]


def test_eval_loss_is_mse_loss_bit_for_bit():
    from hgnn_amd import _lib as L
    g = torch.Generator().manual_seed(5)
    rows, dim = 257, 3
    out = torch.randn(rows, dim, generator=g).cuda()
    t = (3.0 * torch.randn(rows, dim, generator=g)).cuda()
    stats = torch.zeros(4, device="cuda")
    L.check(L.lib().hgnn_mse_loss(L.ptr(out), L.ptr(t), rows * dim, MEAN, STD, L.ptr(stats), None,
                                  L.stream_handle(out.device)), "mse loss")
    m = _meters()
    _eval_loss(out, t, rows, dim, MEAN, STD, m)
    got, s = m.tolist(), stats.tolist()
    assert got[4] == s[0] and got[5] == s[1]
    assert s[0] > 0 and s[1] > 0
    assert got[:3] == [s[0] * rows, s[1] * rows, float(rows)]


@pytest.mark.parametrize("c", [2, 5])
@pytest.mark.parametrize("rows", [1, 65, 300])
def test_eval_xent_loss_and_hits(rows, c):
    g = torch.Generator().manual_seed(100 * c + rows)
    out = torch.randn(rows, c, generator=g)
    t = torch.randint(0, c, (rows,), generator=g)
    # ties at the maximum: the first maximum wins (torch.argmax) -- a hit for target 0, a miss for target 1
    out[0, :2] = 4.0
    t[0] = 0
    if rows > 1:
        out[1, :2] = 4.0
        t[1] = 1
    want = torch.nn.CrossEntropyLoss()(out.double(), t).item()
    hits = float((np.argmax(out.numpy(), axis=1) == t.numpy()).sum())  # numpy: the first maximum
    m = _meters()
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    _eval_xent(out.cuda(), t.float().cuda(), rows, c, m, err)
    got = m.tolist()
    assert _close(got[4], want), (got[4], want)
    assert got[0] == got[4] * rows and got[2] == float(rows)
    assert got[3] == hits
    assert got[1] == 0.0 and got[5] == 0.0
    assert err.item() == 0
    # a second batch adds to the sums
    _eval_xent(out.cuda(), t.float().cuda(), rows, c, m, err)
    again = m.tolist()
    assert again[0] == got[0] + got[0] and again[2] == 2.0 * rows and again[3] == 2 * hits and again[4] == got[4]


def test_eval_xent_rejects_bad_targets():
    """A target outside [0, c) and a fractional one: reported, and left out of the loss and of the hits; the
    divisor stays the number of rows."""
    g = torch.Generator().manual_seed(9)
    out = torch.randn(7, 3, generator=g)
    t = torch.tensor([0.0, 5.0, 1.0, 1.5, 2.0, 1.0, 0.0])
    good = torch.tensor([0, 2, 4, 5, 6])
    rows_loss = torch.nn.CrossEntropyLoss(reduction="sum")(out[good].double(), t[good].long()).item()
    hits = float((np.argmax(out[good].numpy(), axis=1) == t[good].long().numpy()).sum())
    m = _meters()
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    _eval_xent(out.cuda(), t.cuda(), 7, 3, m, err)
    got = m.tolist()
    assert err.item() == 1
    assert _close(got[4], rows_loss / 7), (got[4], rows_loss / 7)
    assert got[0] == got[4] * 7 and got[2] == 7.0 and got[3] == hits
    assert got[1] == 0.0 and got[5] == 0.0


# ---------------------------------------------------------------- TrainStep.evaluate
SIZES = (24, 24, 7)


@pytest.fixture(scope="module")
def lg():
    """GNN_lg(0, 16, 4, 5, 1, 1, 2) after two training steps (running statistics off their initial values), its
    TrainStep, and 55 QM9-shape graphs as three dense batches.  The tests that share it only evaluate."""
    import hgnn_amd.datagen as dg
    from hgnn_amd.train import TrainStep
    from models.gnns.model_mnb import GNN_lg
    torch.manual_seed(41)
    model = GNN_lg(0, 16, 4, 5, 1, 1, 2).cuda()
    step = TrainStep(model, lr=1e-3, t_mean=MEAN, t_std=STD)
    for i in range(2):
        step(_batch(dg.qm9_shape_dataset(24, seed=300 + i)))
    graphs = dg.qm9_shape_dataset(sum(SIZES), seed=310)
    parts, g0 = [], 0
    for n in SIZES:
        parts.append(graphs[g0:g0 + n])
        g0 += n
    torch.cuda.synchronize()
    return {"model": model, "step": step, "graphs": graphs, "parts": parts, "dense": [_batch(p) for p in parts]}


def _reference_pass(ref, batches, mean=MEAN, std=STD):
    """test_with_mnb's loop on dense batches: .item() twice per batch, two AverageMeters."""
    from functions.utils import AverageMeter, evaluation, normalize_data
    loss, error = AverageMeter(), AverageMeter()
    crit = torch.nn.MSELoss()
    ref.eval()
    with torch.no_grad():
        for X, W, T, XL, WL, Pm, Pd, mask, mask_lg, Nb, Eb in batches:
            Tn = normalize_data(T, mean, std)
            out = ref([X, XL, W, WL, Pm, Pd], Nb, mask, Eb, mask_lg) if ref.dual else ref([X, W], Nb, mask)
            loss.update(crit(out, Tn).item(), X.shape[0])
            error.update(evaluation(out, Tn).item(), X.shape[0])
    return loss.avg, error.avg


def _state(model, step):
    from hgnn_amd.dp import running_stats
    return {"params": [p.detach().clone() for p in model.parameters()],
            "grads": [None if p.grad is None else p.grad.clone() for p in model.parameters()],
            "running": [t.clone() for t in running_stats(model)],
            "moments": [t.clone() for t in step.exp_avg + step.exp_inf],
            "stats": step.stats.clone(), "step_count": step.step_count}


def _assert_state(model, step, want):
    got = _state(model, step)
    for k in ("params", "running", "moments"):
        assert all(torch.equal(a, b) for a, b in zip(got[k], want[k])), k
    for a, b in zip(got["grads"], want["grads"]):
        assert (a is None and b is None) or torch.equal(a, b)
    assert torch.equal(got["stats"], want["stats"]) and got["step_count"] == want["step_count"]


def test_evaluate_matches_test_with_mnb(lg):
    model, step = lg["model"], lg["step"]
    want_loss, want_err = _reference_pass(copy.deepcopy(model), lg["dense"])
    assert all(p.grad is not None for p in model.parameters())
    before = _state(model, step)
    passes = []
    for training in (True, False):
        model.train(training)
        step.reset_eval()
        for b in lg["dense"]:
            r = step.evaluate(b)
            assert r is step.eval_meters
            assert model.training == training
        loss, err = step.eval_result()
        assert _close(loss, want_loss), (loss, want_loss)
        assert _close(err, want_err), (err, want_err)
        passes.append(step.eval_meters.tolist())
        assert passes[-1][2] == float(sum(SIZES))
        _assert_state(model, step, before)
    assert passes[0] == passes[1]  # a second reset_eval() + pass: the same bits
    # the same batches as CsrBatches
    model.train()
    step.reset_eval()
    for part in lg["parts"]:
        step.evaluate(_csr(part))
    assert step.eval_meters.tolist() == passes[0]
    _assert_state(model, step, before)


def test_evaluate_gnn_simple_dense_and_csr():
    import hgnn_amd.datagen as dg
    from hgnn_amd.train import TrainStep
    from models.gnns.model_mnb import GNN_simple
    torch.manual_seed(43)
    model = GNN_simple(0, 8, 3, 5, 1, 1).cuda()
    step = TrainStep(model, lr=1e-3, t_mean=MEAN, t_std=STD)
    for i in range(2):
        step(_batch(dg.sbm_dataset(4, n=30, seed=320 + i)))
    graphs = dg.sbm_dataset(7, n=30, seed=330)
    parts = [graphs[:4], graphs[4:]]
    dense = [_batch(p) for p in parts]
    want_loss, want_err = _reference_pass(copy.deepcopy(model), dense)
    before = _state(model, step)
    for batches in (dense, [_csr(p, dual=False) for p in parts]):
        step.reset_eval()
        for b in batches:
            step.evaluate(b)
        loss, err = step.eval_result()
        assert step.eval_meters[2].item() == 7.0
        assert _close(loss, want_loss), (loss, want_loss)
        assert _close(err, want_err), (err, want_err)
    _assert_state(model, step, before)
    assert model.training


def test_evaluate_vs_fp64_oracle(lg):
    """The fp64 oracle (oracle/ref_mnb.py) in eval mode with the model's running statistics, MSE and MAE in
    float64, the AverageMeters in Python doubles."""
    from functions.utils import AverageMeter
    from oracle import ref_mnb as R
    model, step = lg["model"], lg["step"]
    L, order = 4, 2
    p64 = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    st = R.bn_states(L, 2 * model.n_features, dtype=torch.float64)
    for l in range(L - 1):
        layer = model.layer0 if l == 0 else getattr(model, f"layer{l}")
        for nm in ("bn1", "bn2"):
            bn = getattr(layer, nm)
            st[f"layer{l}.{nm}"] = {"running_mean": bn.running_mean.detach().cpu().double(),
                                    "running_std": bn.running_std.detach().cpu().double()}
    loss, error = AverageMeter(), AverageMeter()
    with torch.no_grad():
        for b in lg["dense"]:
            X, W, T, XL, WL, Pm, Pd, mask, mask_lg, Nb, Eb = [t.cpu() for t in b]
            out = R.gnn_lg(p64, [X.double(), XL.double(), W.double(), WL.double(), Pm.double(), Pd.double()], Nb,
                           mask.double(), Eb, mask_lg.double(), L, order, st, False)
            d = out - (T.double() - MEAN) / STD
            loss.update((d * d).mean().item(), X.shape[0])
            error.update(d.abs().mean().item(), X.shape[0])
    step.reset_eval()
    for b in lg["dense"]:
        step.evaluate(b)
    got_loss, got_err = step.eval_result()
    assert _close(got_loss, loss.avg), (got_loss, loss.avg)
    assert _close(got_err, error.avg), (got_err, error.avg)


def test_evaluate_vs_reference_fixture(golden):
    """The reference's own eval-mode outputs after the fixture's one training-mode pass.  The bound is the
    project's forward tolerance eps = 1e-5 * max(1, |out_eval|) per element carried through the loss:
    |(d + e)^2 - d^2| <= 2 |d| eps + eps^2 and ||d + e| - |d|| <= eps, plus one fp32 rounding of the result."""
    from hgnn_amd.csr import CsrBatch
    from hgnn_amd.train import TrainStep
    from models.gnns.model_mnb import GNN_lg
    z = golden("lg_d16_o2")
    graphs = fu.unpack_graphs(z)
    d, L, order, bs, wseed = [int(v) for v in z["cfg"]]
    model = GNN_lg(0, d, L, 5, 1, 1, order).cuda()
    fu.det_init(model, wseed)
    model.train()
    b = CsrBatch([(x, a) for x, a, _ in graphs], dual=True, targets=torch.stack([t[0] for _, _, t in graphs]))
    model.forward_csr(b)  # the training-mode pass: sets the running statistics
    step = TrainStep(model, t_mean=MEAN, t_std=STD)
    step.evaluate(b)
    loss, mae = step.eval_result()
    oe = z["out_eval"].astype(np.float64)
    T = np.stack([t[0].numpy() for _, _, t in graphs]).reshape(oe.shape).astype(np.float32)
    Tn = ((T - np.float32(MEAN)) / np.float32(STD)).astype(np.float64)  # the kernel's fp32 normalisation
    diff = oe - Tn
    eps = 1e-5 * np.maximum(1.0, np.abs(oe))
    ref_loss, ref_mae = float((diff * diff).mean()), float(np.abs(diff).mean())
    loss_bound = float((2 * np.abs(diff) * eps + eps * eps).mean()) + 2.0 ** -23 * ref_loss
    mae_bound = float(eps.mean()) + 2.0 ** -23 * ref_mae
    assert abs(loss - ref_loss) <= loss_bound, (loss, ref_loss, loss_bound)
    assert abs(mae - ref_mae) <= mae_bound, (mae, ref_mae, mae_bound)
    assert step.eval_meters[2].item() == float(len(graphs))


def test_evaluate_classification_end_to_end():
    """mean == 0 (scripts/test_mnb.py:49-50): class targets, nn.CrossEntropyLoss; error.avg stays 0."""
    import hgnn_amd.datagen as dg
    from functions.utils import AverageMeter
    from hgnn_amd.train import TrainStep
    from models.gnns.model_mnb import GNN_lg
    torch.manual_seed(47)
    model = GNN_lg(0, 16, 4, 5, 3, 1, 2).cuda()
    step = TrainStep(model, lr=1e-3, t_mean=0.0)
    assert step.classification
    gen = torch.Generator().manual_seed(3)

    def batch(n, seed):
        b = _batch(dg.qm9_shape_dataset(n, seed=seed))
        b[2] = torch.randint(0, 3, (n, 1), generator=gen).float().cuda()
        return b

    for i in range(2):
        step(batch(24, 340 + i))
    step.check_targets()
    batches = [batch(24, 350), batch(7, 351)]
    ref = copy.deepcopy(model).eval()
    meter, hits = AverageMeter(), 0
    crit = torch.nn.CrossEntropyLoss()
    with torch.no_grad():
        for X, W, T, XL, WL, Pm, Pd, mask, mask_lg, Nb, Eb in batches:
            out = ref([X, XL, W, WL, Pm, Pd], Nb, mask, Eb, mask_lg)
            t = T.squeeze().long()
            meter.update(crit(out, t).item(), X.shape[0])
            hits += int((np.argmax(out.cpu().numpy(), axis=1) == t.cpu().numpy()).sum())
    before = _state(model, step)
    step.reset_eval()
    for b in batches:
        step.evaluate(b)
    res = step.eval_result(accuracy=True)
    assert len(res) == 3 and res[1] == 0.0
    assert _close(res[0], meter.avg), (res[0], meter.avg)
    assert res[2] == hits / 31.0
    assert step.eval_result() == (res[0], 0.0)
    assert step.eval_meters[1].item() == 0.0 and step.eval_meters[5].item() == 0.0
    _assert_state(model, step, before)
    bad = batch(4, 352)
    bad[2] = torch.tensor([[0.0], [5.0], [1.0], [2.0]]).cuda()
    # HGNN_STRICT=1 (conftest): evaluate raises at once
    with pytest.raises(RuntimeError, match="class target"):
        step.evaluate(bad)
    os.environ["HGNN_STRICT"] = "0"
    try:
        step.evaluate(bad)
        with pytest.raises(RuntimeError, match="class target"):
            step.check_targets()
        step.check_targets()  # the error word was consumed
    finally:
        os.environ["HGNN_STRICT"] = "1"
    with pytest.raises(RuntimeError, match="classification"):
        TrainStep(GNN_lg(0, 8, 3, 5, 1, 1, 2).cuda(), t_mean=MEAN).eval_result(accuracy=True)


# ---------------------------------------------------------------- the epoch loops
@pytest.mark.parametrize("source", ["list", "pack"])
def test_eval_epoch_is_the_manual_loop(lg, source, tmp_path):
    from hgnn_amd.dataset import GraphPack
    step = lg["step"]
    data = [[x, a, t] for x, a, t in lg["graphs"]]
    if source == "pack":
        data = GraphPack.write(str(tmp_path / "pack"), data)
        batches = list(data.batches(range(len(data)), 24, 0, J=1, dual=True))
    else:
        batches = [_csr(p) for p in lg["parts"]]
    assert [b.bs for b in batches] == list(SIZES)
    step.reset_eval()
    for b in batches:
        step.evaluate(b)
    want, meters = step.eval_result(), step.eval_meters.tolist()
    step.eval_meters.fill_(7.0)  # eval_epoch starts a new set
    assert step.eval_epoch(data, 0, 24) == want
    assert step.eval_meters.tolist() == meters
    assert want[0] > 0 and want[1] > 0


def test_eval_epoch_dense_list(lg):
    """dense=True: full 7-tuples through prepare_batch; the same meters as the CSR batches (the executor computes
    the same numbers on both layouts)."""
    step = lg["step"]
    want = step.eval_epoch([[x, a, t] for x, a, t in lg["graphs"]], 0, 24)
    assert step.eval_epoch(_instances(lg["graphs"]), 0, 24, dense=True) == want


def test_train_epoch_is_two_manual_steps():
    """31 instances at bs 24: the steps of batches [0, 24) and [24, 31).  Training-mode BN statistics are fp64
    atomics, so the parameters are held to the per-step bounds of tests/test_gpu_train.py, once per step taken:
    elements whose gradient is above the noise floor (1e-4 max|g|) in both steps within 2 * 1e-5 * max(1, |p|),
    the others within 2 lr per step."""
    import hgnn_amd.datagen as dg
    from hgnn_amd.train import TrainStep
    from models.gnns.model_mnb import GNN_lg
    torch.manual_seed(53)
    lr = 1e-3
    model = GNN_lg(0, 16, 4, 5, 1, 1, 2).cuda()
    twin = copy.deepcopy(model)
    graphs = dg.qm9_shape_dataset(31, seed=360)
    step = TrainStep(model, lr=lr, t_mean=MEAN, t_std=STD)
    manual = TrainStep(twin, lr=lr, t_mean=MEAN, t_std=STD)
    step.stats.fill_(3.0)  # train_epoch starts new RunningAverages
    res = step.train_epoch([[x, a, t] for x, a, t in graphs], 0, 24)
    assert step.step_count == 2
    s = step.stats.tolist()
    assert res == (s[2], s[3]) and s[2] > 0 and s[3] > 0
    noisy = [torch.zeros_like(p, dtype=torch.bool) for p in twin.parameters()]
    for part in (graphs[:24], graphs[24:]):
        manual(_csr(part))
        gmax = max(p.grad.abs().max().item() for p in twin.parameters())
        for k, p in enumerate(twin.parameters()):
            noisy[k] |= p.grad.abs() <= 1e-4 * gmax
    ms = manual.stats.tolist()
    assert _close(s[2], ms[2]) and _close(s[3], ms[3]) and _close(s[0], ms[0])
    for (n, p), q, nz in zip(model.named_parameters(), twin.parameters(), noisy):
        err = (p.detach() - q.detach()).abs()
        tight = err[~nz]
        assert tight.numel() == 0 or tight.max().item() <= 2 * 1e-5 * max(1.0, q.abs().max().item()), \
            (n, tight.max().item())
        assert err.max().item() <= 2 * (2 * lr), (n, err.max().item())


# ---------------------------------------------------------------- HIP-graph replay
def test_evaluate_graph_replay_equals_eager(lg):
    """evaluate() has no host synchronisation and no host-side state: a captured call, replayed three times on
    zeroed meters, leaves the bits of three eager calls."""
    step, b = lg["step"], lg["dense"][0]
    step.reset_eval()
    for _ in range(3):
        step.evaluate(b)
    torch.cuda.synchronize()
    want = step.eval_meters.tolist()
    assert want[2] == 72.0
    step.reset_eval()
    g = _capture(lambda: step.evaluate(b))
    step.reset_eval()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert step.eval_meters.tolist() == want
