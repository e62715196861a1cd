"""The classification branch of the device-resident CCN training loop (hgnn_amd.train.CcnTrainStep with
classification=True: hgnn_ccn_small_train_xent, hgnn_ccn_eval_xent) against the library's own pieces (bitwise)
and the fp64 oracle.

The loop is scripts/train_ccn.py:31-73 on its `mean == 0` branch: the target cast to a class index, net(X, A + I),
the output viewed as (1, n_outputs), nn.CrossEntropyLoss, backward, one Adamax step; no MAE meter.

Shapes are those of tests/test_gpu_ccn_train.py with at least two outputs (lr 1e-3, weights from
fixture_util.det_init, the label of graph g of a list is g % n_outputs):
  A  CCN_1D(5, 2, 2, 2) on qm9_shape_dataset(6, seed=700): 8 and 16 lanes per node
  B  CCN_1D(7, 3, 5, 3) on qm9_shape_dataset(6, seed=701, n_min=6, n_max=16), features widened to 7
  C  CCN_1D(3, 2, 8, 1) on B's graphs with X[:, :3]
  D  model A on sbm_dataset(1, n=40, seed=3, p_in=0.6) + two graphs of A: 32 lanes per node
  G  CCN_1D(5, 2, 2, 10), the generated driver's model, on three_collinear_points(6, n_max=16, seed=11) + I: dense
     patterns, real-valued features, diagonal entries of 2

Tolerances against the oracle are those of tests/test_gpu_ccn_train.py: values within 1e-5 max(1, |ref|);
parameters after K Adamax steps within the same bound where the oracle's gradient was above the noise floor
(1e-4 max|g| of its tensor) at every step or exactly 0, else within 2 lr K -- and that second class may hold at
most 5 % of the elements.  Three classes (B) saturate softmax rows within a few steps, which puts 15 % of the
oracle's own elements into the loose class over six steps, so B is compared after one step instead: out and the
loss within 1e-5 max(1, |ref|), every gradient within 1e-5 max(1, max|g| of its tensor).
"""

import ctypes

import pytest
import torch

import fixture_util as fu

pytestmark = pytest.mark.gpu

LR = 1e-3


def _self_loops(graphs):
    return [(X, A + torch.eye(A.shape[0]), t) for X, A, t in graphs]


def _graphs(shape):
    import hgnn_amd.datagen as dg
    if shape == "A":
        return _self_loops(dg.qm9_shape_dataset(6, seed=700))
    if shape in ("B", "C"):
        gen = torch.Generator().manual_seed(701)
        gs = _self_loops(dg.qm9_shape_dataset(6, seed=701, n_min=6, n_max=16))
        if shape == "B":
            return [(torch.cat([X, torch.rand(X.shape[0], 2, generator=gen)], 1), A, t) for X, A, t in gs]
        return [(X[:, :3].contiguous(), A, t) for X, A, t in gs]
    if shape == "D":
        return _self_loops(dg.sbm_dataset(1, n=40, seed=3, p_in=0.6)) + _graphs("A")[:2]
    if shape == "G":
        return _self_loops([(d[0], d[1], None) for d in dg.three_collinear_points(6, n_max=16, seed=11)])
    raise KeyError(shape)


MODELS = {"A": (5, 2, 2, 2), "B": (7, 3, 5, 3), "C": (3, 2, 8, 1), "D": (5, 2, 2, 2), "G": (5, 2, 2, 10)}


def _model(shape, seed, cls=None):
    from models.compnets.model_ccn import CCN_1D
    net = (cls or CCN_1D)(*(MODELS[shape] if isinstance(shape, str) else shape))
    fu.det_init(net, seed)
    return net


def _labels(count, n_out):
    return [g % n_out for g in range(count)]


def _pad(graphs, labels, nmax=None):
    bs = len(graphs)
    nmax = nmax or max(g[0].shape[0] for g in graphs)
    X = torch.zeros(bs, nmax, graphs[0][0].shape[1])
    A = torch.zeros(bs, nmax, nmax)
    for b, g in enumerate(graphs):
        n = g[0].shape[0]
        X[b, :n] = g[0]
        A[b, :n, :n] = g[1]
    nb = torch.tensor([g[0].shape[0] for g in graphs], dtype=torch.int64)
    y = torch.tensor(labels)
    return X.cuda(), A.cuda(), nb.cuda(), y.cuda()


def _assert_fused(net, nmax):
    from hgnn_amd import _lib
    cfg = net._spec().config(1, nmax)
    assert _lib.lib().hgnn_ccn_small_train_supported(ctypes.byref(cfg)) == 1


def _step(net, fused=True):
    from hgnn_amd.train import CcnTrainStep
    return CcnTrainStep(net, lr=LR, classification=True, fused=fused)


def _state(st):
    return [p.detach().clone() for p in st.params] + [t.clone() for t in st.exp_avg + st.exp_inf]


def _same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"{what}: tensor {i} differs by {(x - y).abs().max().item():.3g}"


def test_generated_graphs_are_dense_with_a_doubled_diagonal():
    """What shape G is there for: receptive fields well above the QM9 shapes' and a diagonal entry of 2."""
    gs = _graphs("G")
    assert max(int((a > 0).sum(1).max()) for _, a, _ in gs) > 8
    assert any(bool((a.diagonal() == 2).any()) for _, a, _ in gs)
    assert max(x.shape[0] for x, _, _ in gs) <= 15


@pytest.mark.parametrize("shape", ["A", "B", "C", "D", "G"])
def test_one_fused_step_equals_the_librarys_own_pieces(shape):
    """Graph by graph, from equal parameters and optimizer state (the state the previous graphs left):
    CcnTrainStep(classification=True, fused=True).step on the one-graph slice against forward_batch,
    hgnn_xent_loss with n = 1, backward and hgnn_adamax_step.  Bitwise: out, every p.grad, stats[0], exp_inf,
    exp_avg and the parameters (the loss kernels inline one row function, xent_row, the optimizer kernels
    adamax_elem); stats[1] and stats[3] stay 0.  The running loss 0.9 v + 0.1 r of positive terms is formed by
    each kernel's own instructions (one contracts the sum into an fma, the other rounds both products): each is
    within 2 * 2^-24 of the exact sum, so the two are within 2^-22 of each other, relative."""
    from hgnn_amd import _lib as L
    lib = L.lib()
    graphs = _graphs(shape)
    n_out = MODELS[shape][1]
    X, A, nb, y = _pad(graphs, _labels(len(graphs), n_out))
    yf = y.float()
    _assert_fused(_model(shape, 33), X.shape[1])
    fused = _step(_model(shape, 33).cuda())
    net = _model(shape, 33).cuda()
    ps = net._params()
    m = [torch.zeros_like(p) for p in ps]
    u = [torch.zeros_like(p) for p in ps]
    numel = (ctypes.c_int64 * len(ps))(*[p.numel() for p in ps])
    stats = torch.zeros(4, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = L.stream_handle(X.device)
    for g in range(len(graphs)):
        st = fused.step(X[g:g + 1], A[g:g + 1], nb[g:g + 1], y[g:g + 1])
        for p in ps:
            p.grad = None
        out = net.forward_batch(X[g:g + 1], A[g:g + 1], nb[g:g + 1])
        dout = torch.empty_like(out)
        L.check(lib.hgnn_xent_loss(L.ptr(out.detach()), L.ptr(yf[g:g + 1]), 1, n_out, L.ptr(stats), L.ptr(dout),
                                   L.ptr(err), stream), "xent")
        torch.autograd.backward(out, dout)
        grads = [p.grad for p in ps]
        L.check(lib.hgnn_adamax_step(len(ps), L.ptr_array(ps), L.ptr_array(grads), L.ptr_array(m), L.ptr_array(u),
                                     numel, LR, 0.9, 0.999, 1e-8, 0.0, g + 1, stream), "adamax")
        assert torch.equal(fused.out, out.detach()), (g, fused.out, out)
        assert torch.equal(st[0], stats[0]), (g, st.tolist(), stats.tolist())
        assert st[0].item() >= 0 and st[1].item() == 0 and st[3].item() == 0, st  # a saturated row's loss is 0
        assert abs(st[2].item() - stats[2].item()) <= 2.0 ** -22 * stats[2].item(), (g, st.tolist(), stats.tolist())
        _same([p.grad for p in fused.params], grads, f"graph {g} gradients")
        _same(fused.exp_inf, u, f"graph {g} exp_inf")
        _same(fused.exp_avg, m, f"graph {g} exp_avg")
        _same([p.detach() for p in fused.params], [p.detach() for p in ps], f"graph {g} parameters")
    assert int(err.item()) == 0


@pytest.mark.parametrize("shape", ["A", "D"])
def test_k_steps_in_one_dispatch_equal_k_one_graph_dispatches(shape):
    """step on all graphs at once against step called per graph (both the fused kernel): parameters, optimizer
    state, out, stats and step_count are bitwise equal."""
    graphs = _graphs(shape)
    X, A, nb, y = _pad(graphs, _labels(len(graphs), 2))
    _assert_fused(_model(shape, 21), X.shape[1])
    many = _step(_model(shape, 21).cuda())
    many.step(X, A, nb, y)
    one = _step(_model(shape, 21).cuda())
    outs = []
    for g in range(len(graphs)):
        one.step(X[g:g + 1], A[g:g + 1], nb[g:g + 1], y[g:g + 1])
        outs.append(one.out.clone())
    _same(_state(many), _state(one), f"shape {shape}")
    assert torch.equal(many.out, torch.cat(outs)), (many.out, torch.cat(outs))
    assert torch.equal(many.stats, one.stats), (many.stats, one.stats)
    assert many.step_count == one.step_count == len(graphs)
    _same([p.grad for p in many.params], [p.grad for p in one.params], "last graph's gradients")
    moved = (many.params[0].detach() - _model(shape, 21).w1.weight.cuda()).abs().max().item()
    assert moved > 0, moved  # the steps were taken (alternating labels pull back and forth: no lr K drift)


class _Oracle:
    """scripts/train_ccn.py:31-73 on the `mean == 0` branch in fp64: oracle.ref_ccn.ccn_forward,
    nn.CrossEntropyLoss on out.view(1, -1) and torch.optim.Adamax stepping per graph; the loss meter by
    RunningAverage's rule (functions/utils.py:142-146): a meter that is 0.0 takes the value as it is, else
    0.9 v + 0.1 r.  That rule is discontinuous at 0, and a saturated row's cross entropy (1e-13 in fp64) is
    exactly 0.0 in the reference's fp32 run, so the meter's `== 0.0` looks at the loss such a run reports:
    nn.CrossEntropyLoss in fp32 on the oracle's output.  The values stay fp64."""

    def __init__(self, net, order):
        self.order, self.layers = order, net.layers
        self.p = {n: v.detach().cpu().double().clone().requires_grad_(True) for n, v in net.named_parameters()}
        self.names = [n for n, _ in net.named_parameters()]
        self.opt = torch.optim.Adamax([self.p[n] for n in self.names], lr=LR)
        self.noisy = {n: torch.zeros_like(self.p[n], dtype=torch.bool) for n in self.names}
        self.outs, self.loss, self.run, self.run_is_zero = [], None, 0.0, True
        self.steps = 0

    def step(self, x, a, label):
        from oracle import ref_ccn as RC
        self.opt.zero_grad()
        out = RC.ccn_forward(self.p, x.double(), a.double(), self.order, self.layers)
        loss = torch.nn.CrossEntropyLoss()(out.view(1, -1), torch.tensor([label]))
        loss.backward()
        for n in self.names:
            g = self.p[n].grad.abs()
            self.noisy[n] |= (g > 0) & (g <= 1e-4 * g.max())
        self.opt.step()
        self.steps += 1
        self.outs.append(out.detach().view(-1))
        self.loss = loss.item()
        loss32 = torch.nn.CrossEntropyLoss()(out.detach().float().view(1, -1), torch.tensor([label])).item()
        self.run = self.loss if self.run_is_zero else 0.9 * self.loss + 0.1 * self.run
        self.run_is_zero = loss32 == 0.0 if self.run_is_zero else False

    def compare(self, st, what):
        outs = torch.stack(self.outs)
        err = (st.out.double().cpu() - outs).abs()
        print(f"{what}: max out error {(err / outs.abs().clamp(min=1.0)).max().item():.3g}")
        assert (err <= 1e-5 * outs.abs().clamp(min=1.0)).all(), f"{what}: out differs by {err.max().item():.3g}"
        got = st.stats.double().cpu().tolist()
        for v, r in zip(got, [self.loss, 0.0, self.run, 0.0]):
            assert abs(v - r) <= 1e-5 * max(1.0, abs(r)), (what, got, self.loss, self.run)
        assert got[1] == 0.0 and got[3] == 0.0
        loose = total = 0
        for n, p in st.model.named_parameters():
            q = self.p[n].detach()
            e = (p.detach().double().cpu() - q).abs()
            tight = ~self.noisy[n]
            assert (e[tight] <= 1e-5 * q[tight].abs().clamp(min=1.0)).all(), (what, n, e[tight].max().item())
            assert e.max().item() <= 2 * LR * self.steps, (what, n, e.max().item())
            loose += int(self.noisy[n].sum())
            total += q.numel()
        print(f"{what}: {loose} of {total} elements on the loose bound")
        assert loose <= 0.05 * total, f"{what}: {loose} of {total} elements on the loose bound"
        assert st.step_count == self.steps


def _against_oracle(net, order, graphs, labels, fused, what):
    orc = _Oracle(net, order)
    for (x, a, _), lb in zip(graphs, labels):
        orc.step(x, a, lb)
    st = _step(net.cuda(), fused=fused)
    st.step(*_pad(graphs, labels))
    orc.compare(st, what)
    return st


def test_fused_loop_against_the_fp64_oracle():
    """All graphs of A, then all of D (nine sequential steps, padded to D's 40 nodes) in one step call."""
    graphs = _graphs("A") + _graphs("D")
    net = _model("A", 47)
    _assert_fused(net, 40)
    _against_oracle(net, 1, graphs, _labels(9, 2), True, "fused A + D")


def test_fused_loop_against_the_fp64_oracle_wide_hidden():
    """Shape C: 8 hidden channels, one level, six steps."""
    graphs = _graphs("C")
    net = _model("C", 47)
    _assert_fused(net, max(g[0].shape[0] for g in graphs))
    _against_oracle(net, 1, graphs, _labels(6, 2), True, "fused C")


def test_fused_loop_against_the_fp64_oracle_at_the_drivers_depth():
    """CCN_1D(5, 2, 2, 10), the generated driver's model, on A's graphs: six steps through ten levels."""
    graphs = _graphs("A")
    net = _model("G", 47)
    _assert_fused(net, max(g[0].shape[0] for g in graphs))
    _against_oracle(net, 1, graphs, _labels(6, 2), True, "fused A, 10 levels")


def test_unfused_loop_against_the_fp64_oracle():
    """fused=False (forward_batch, hgnn_xent_loss, backward, hgnn_adamax_step per graph) on shape A."""
    _against_oracle(_model("A", 47), 1, _graphs("A"), _labels(6, 2), False, "unfused A")


def test_ccn2d_takes_the_unfused_loop():
    """CCN_2D(5, 2, 2, 2) on three graphs of 6-8 nodes against ccn_forward(order=2); fused=True raises."""
    import hgnn_amd.datagen as dg
    from hgnn_amd.train import CcnTrainStep
    from models.compnets.model_ccn import CCN_2D
    graphs = _self_loops(dg.qm9_shape_dataset(3, seed=702, n_min=6, n_max=8))
    net = _model("A", 52, CCN_2D)
    st = _against_oracle(net, 2, graphs, [0, 1, 0], None, "CCN-2D")
    assert not st._supported(8)
    with pytest.raises(RuntimeError, match="fused=True"):
        CcnTrainStep(net, lr=LR, classification=True, fused=True)


def test_three_classes_one_step_against_fp64():
    """Shape B (three classes): one fused step per graph from the initial weights against fp64 autograd -- out
    and the loss within 1e-5 max(1, |ref|), every gradient within 1e-5 max(1, max|g| of its tensor)."""
    from oracle import ref_ccn as RC
    graphs = _graphs("B")
    labels = _labels(6, 3)
    X, A, nb, y = _pad(graphs, labels)
    _assert_fused(_model("B", 33), X.shape[1])
    worst = 0.0
    for g, ((x, a, _), lb) in enumerate(zip(graphs, labels)):
        net = _model("B", 33)
        p64 = {n: v.detach().double().clone().requires_grad_(True) for n, v in net.named_parameters()}
        ref = RC.ccn_forward(p64, x.double(), a.double(), 1, net.layers)
        loss = torch.nn.CrossEntropyLoss()(ref.view(1, -1), torch.tensor([lb]))
        loss.backward()
        st = _step(net.cuda())
        stats = st.step(X[g:g + 1], A[g:g + 1], nb[g:g + 1], y[g:g + 1]).double().cpu()
        r = ref.detach().view(-1)
        e = (st.out[0].double().cpu() - r).abs()
        assert (e <= 1e-5 * r.abs().clamp(min=1.0)).all(), (g, e.max().item())
        assert abs(stats[0].item() - loss.item()) <= 1e-5 * max(1.0, abs(loss.item())), (g, stats, loss.item())
        for n, p in net.named_parameters():
            gr = p64[n].grad
            scale = max(1.0, gr.abs().max().item())
            ge = (p.grad.double().cpu() - gr).abs().max().item()
            worst = max(worst, ge / scale)
            assert ge <= 1e-5 * scale, (g, n, ge, scale)
    print(f"B one step: worst gradient error {worst:.3g} of its scale")


def test_bad_targets_fused():
    """Five slots on model A with targets [0, 1, 2 (out of range), 0.5 (not an integer), 1]: the two graphs take
    no step -- state, stats and the other out rows are bitwise those of the three-graph list; the next check
    raises the class-target message, and a following clean call raises nothing."""
    from hgnn_amd.net import check_errors
    ga = _graphs("A")[:5]
    nmax = max(g[0].shape[0] for g in ga)
    _assert_fused(_model("A", 61), nmax)
    check_errors()
    full = _step(_model("A", 61).cuda())
    with pytest.raises(RuntimeError, match="class target"):
        full.step(*_pad(ga, [0.0, 1.0, 2.0, 0.5, 1.0], nmax))  # HGNN_STRICT=1 reports here, after the call
        check_errors()
    check_errors()  # the word was consumed
    clean = _step(_model("A", 61).cuda())
    clean.step(*_pad([ga[0], ga[1], ga[4]], [0.0, 1.0, 1.0], nmax))
    check_errors()
    _same(_state(full), _state(clean), "rejected slots skipped")
    assert torch.equal(full.stats, clean.stats)
    assert torch.equal(full.out[[0, 1, 4]], clean.out)
    _same([p.grad for p in full.params], [p.grad for p in clean.params], "last graph's gradients")
    # the rejected graphs still got their out rows: finite, and not what an untouched buffer would hold twice
    assert torch.isfinite(full.out[2:4]).all() and not torch.equal(full.out[2], full.out[3])


def test_bad_targets_unfused():
    """The unfused path reports the same list (its rows get a zero dout; the steps are still taken)."""
    ga = _graphs("A")[:5]
    st = _step(_model("A", 61).cuda(), fused=False)
    with pytest.raises(RuntimeError, match="class target"):
        st.step(*_pad(ga, [0.0, 1.0, 2.0, 0.5, 1.0]))
        st.check_targets()
    st.check_targets()  # consumed
    st.step(*_pad(ga[:2], [0, 1]))
    st.check_targets()


def test_evaluation_and_epochs():
    """evaluate against the oracle's per-graph cross entropy (1e-5 relative) and argmax (exact); two calls bitwise
    equal; eval_epoch in chunks of 4 equals evaluate on all six (the count-weighted combination) and returns the
    reference's (losses.avg, 0.0) unless asked for the accuracy; train_epoch in chunks of 4 leaves the state
    bitwise equal to one step over all six and returns (stats[2], 0.0)."""
    from oracle import ref_ccn as RC
    graphs = _graphs("A")
    labels = _labels(6, 2)
    net = _model("A", 73)
    p64 = {n: v.detach().double() for n, v in net.named_parameters()}
    xent, hits = [], 0
    for (x, a, _), lb in zip(graphs, labels):
        o = RC.ccn_forward(p64, x.double(), a.double(), 1, net.layers).view(1, -1)
        xent.append(torch.nn.CrossEntropyLoss()(o, torch.tensor([lb])).item())
        hits += int(torch.argmax(o[0]).item() == lb)
    ref = sum(xent) / len(xent)
    st = _step(net.cuda())
    X, A, nb, y = _pad(graphs, labels)
    r1 = st.evaluate(X, A, nb, y)
    r2 = st.evaluate(X, A, nb, y)
    assert r1.shape == (3,) and torch.equal(r1, r2)
    assert abs(r1[0].item() - ref) <= 1e-5 * abs(ref), (r1, ref)
    assert r1[1].item() == 0.0
    assert r1[2].item() == torch.tensor(hits / 6, dtype=torch.float32).item(), (r1, hits)
    # the reference's data: [X, A without self loops, LongTensor([label]), ...] 7-tuples
    data = [[x, a - torch.eye(a.shape[0]), torch.tensor([lb]), None, None, None, None]
            for (x, a, _), lb in zip(graphs, labels)]
    ev = st.eval_epoch(data, 0, chunk=4)
    assert len(ev) == 2 and ev[1] == 0.0
    ev3 = st.eval_epoch(data, 0, chunk=4, accuracy=True)
    assert len(ev3) == 3 and ev3[:2] == ev
    for v, r in zip(ev3, r1.tolist()):
        assert abs(v - r) <= 1e-6 * max(1.0, abs(r)), (ev3, r1)
    loss, err = st.train_epoch(data, 0, chunk=4)
    whole = _step(_model("A", 73).cuda())
    s = whole.step(X, A, nb, y).tolist()
    _same(_state(st), _state(whole), "train_epoch in chunks")
    assert (loss, err) == (s[2], 0.0)
    assert st.step_count == whole.step_count == 6
    st.check_targets()
