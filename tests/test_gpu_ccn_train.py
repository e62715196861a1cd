"""The device-resident CCN training loop (hgnn_amd.train.CcnTrainStep, hgnn_ccn_small_train) and the evaluation
meters (hgnn_ccn_eval_loss) against the library's own pieces (bitwise) and the fp64 oracle.

The loop is scripts/train_ccn.py:31-73 per graph: y' = (y - mean) / (std + 1e-8), net(X, A + I), MSE and MAE,
backward, one Adamax step; graph g + 1 sees the weights graph g left.

Shapes (targets t[:n_out], t_mean 0.3, t_std 1.7, lr 1e-3, weights from fixture_util.det_init):
  A  CCN_1D(5, 1, 2, 2) on qm9_shape_dataset(6, seed=700): 13-22 nodes, receptive fields of up to 6-10 nodes,
     so graphs of 8 and of 16 lanes per node both occur
  B  CCN_1D(7, 2, 5, 3) on qm9_shape_dataset(6, seed=701, n_min=6, n_max=16), features widened to 7
  C  CCN_1D(3, 1, 8, 1) on B's graphs with X[:, :3]
  D  model A on sbm_dataset(1, n=40, seed=3, p_in=0.6) + two graphs of A: the 40-node graph has receptive
     fields above 16 nodes (32 lanes per node, three passes of the 8 waves)

Tolerances against the oracle are those of tests/test_gpu_train.py and tests/test_gpu_ccn.py: values within
1e-5 max(1, |ref|); parameters after K Adamax steps within 1e-5 max(1, |p|) where the oracle's gradient was
above the noise floor (1e-4 max|g|) at every step, else within 2 lr K (Adamax turns the sign of a noise-level
gradient into an lr-sized step) -- and that second class may hold at most 5 % of the elements.
Two points of that rule, both on the strict side.  max|g| is taken per parameter tensor: the fc weights'
gradients are sums over every node and 100-1000 times those of the level weights, so a maximum over all
tensors would call most level weights noise, which they are not.  And a gradient that is exactly 0 in the
oracle is not noise either (one-hot feature columns no node of the graph has, a ReLU channel dead on every
row: about a fifth of the elements at each step): both sides leave such an element where it was, and it stays
on the tight bound.
"""

import ctypes

import pytest
import torch

import fixture_util as fu

pytestmark = pytest.mark.gpu

MEAN, STD, LR = 0.3, 1.7, 1e-3


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
    raise KeyError(shape)


MODELS = {"A": (5, 1, 2, 2), "B": (7, 2, 5, 3), "C": (3, 1, 8, 1), "D": (5, 1, 2, 2)}


def _model(shape, seed, cls=None):
    from models.compnets.model_ccn import CCN_1D
    net = (cls or CCN_1D)(*MODELS[shape])
    fu.det_init(net, seed)
    return net


def _pad(graphs, n_out, nmax=None):
    bs = len(graphs)
    nmax = nmax or max(X.shape[0] for X, _, _ in graphs)
    X = torch.zeros(bs, nmax, graphs[0][0].shape[1])
    A = torch.zeros(bs, nmax, nmax)
    for b, (x, a, _) in enumerate(graphs):
        n = x.shape[0]
        X[b, :n] = x
        A[b, :n, :n] = a
    nb = torch.tensor([g[0].shape[0] for g in graphs], dtype=torch.int64)
    y = torch.stack([t[:n_out] for _, _, t in graphs]).float()
    return X.cuda(), A.cuda(), nb.cuda(), y.cuda()


def _max_field(a):
    return int((a > 0).sum(1).max())


def _assert_fused(net, nmax):
    from hgnn_amd import _lib
    cfg = net._spec().config(1, nmax)
    assert _lib.lib().hgnn_ccn_small_train_supported(ctypes.byref(cfg)) == 1


def _step(net, fused=True):
    from hgnn_amd.train import CcnTrainStep
    return CcnTrainStep(net, lr=LR, t_mean=MEAN, t_std=STD, fused=fused)


def _state(st):
    return [p.detach().clone() for p in st.params] + [t.clone() for t in st.exp_avg + st.exp_inf]


def _same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"{what}: tensor {i} differs by {(x - y).abs().max().item():.3g}"


def test_shapes_cover_every_lane_layout():
    """The generators give what the tests rely on: 8 and 16 lanes per node in A, 32 in D's first graph."""
    fields = [_max_field(a) for _, a, _ in _graphs("A")]
    assert min(fields) <= 8 < max(fields) <= 16, fields
    x, a, _ = _graphs("D")[0]
    assert x.shape[0] > 32 and _max_field(a) > 16, (x.shape, _max_field(a))


@pytest.mark.parametrize("shape", ["A", "D"])
def test_k_steps_in_one_dispatch_equal_k_one_graph_dispatches(shape):
    """The loop's re-staging and fence: step on all graphs at once against step called per graph (both the
    fused kernel).  The multi-graph call runs first, on parameters no other kernel has read yet.  Parameters,
    optimizer state, out, stats and step_count are bitwise equal."""
    graphs = _graphs(shape)
    X, A, nb, y = _pad(graphs, 1)
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
    # the weights moved at every step: Adamax's first steps are ~lr each
    moved = (many.params[0].detach() - _model(shape, 21).w1.weight.cuda()).abs().max().item()
    assert moved > 0.5 * LR * len(graphs), moved


@pytest.mark.parametrize("shape", ["A", "B", "C", "D"])
def test_one_fused_step_equals_the_librarys_own_pieces(shape):
    """Graph by graph, from equal parameters and optimizer state (the state the previous graphs left, so the
    moments and the step count are not trivial): CcnTrainStep(fused=True).step on the one-graph slice against
    forward_batch, hgnn_mse_loss on the CPU-normalised target with (0, 1), backward and hgnn_adamax_step.
    Bitwise: out, every p.grad, stats[0:2], exp_inf, exp_avg and the parameters (both kernels inline the one
    update function, adamax_elem)."""
    from hgnn_amd import _lib as L
    lib = L.lib()
    graphs = _graphs(shape)
    n_out = MODELS[shape][1]
    X, A, nb, y = _pad(graphs, n_out)
    _assert_fused(_model(shape, 33), X.shape[1])
    fused = _step(_model(shape, 33).cuda())
    net = _model(shape, 33).cuda()
    ps = net._params()
    m = [torch.zeros_like(p) for p in ps]
    u = [torch.zeros_like(p) for p in ps]
    numel = (ctypes.c_int64 * len(ps))(*[p.numel() for p in ps])
    stats = torch.zeros(4, device="cuda")
    stream = L.stream_handle(X.device)
    for g in range(len(graphs)):
        st = fused.step(X[g:g + 1], A[g:g + 1], nb[g:g + 1], y[g:g + 1])
        for p in ps:
            p.grad = None
        out = net.forward_batch(X[g:g + 1], A[g:g + 1], nb[g:g + 1])
        yn = ((y[g].cpu() - MEAN) / (STD + 10 ** -8)).cuda()  # train_ccn.py:42, before .cuda()
        dout = torch.empty_like(out)
        L.check(lib.hgnn_mse_loss(L.ptr(out.detach()), L.ptr(yn), n_out, 0.0, 1.0, L.ptr(stats), L.ptr(dout),
                                  stream), "mse")
        torch.autograd.backward(out, dout)
        grads = [p.grad for p in ps]
        L.check(lib.hgnn_adamax_step(len(ps), L.ptr_array(ps), L.ptr_array(grads), L.ptr_array(m), L.ptr_array(u),
                                     numel, LR, 0.9, 0.999, 1e-8, 0.0, g + 1, stream), "adamax")
        assert torch.equal(fused.out, out.detach()), (g, fused.out, out)
        assert torch.equal(st[:2], stats[:2]), (g, st, stats)
        _same([p.grad for p in fused.params], grads, f"graph {g} gradients")
        _same(fused.exp_inf, u, f"graph {g} exp_inf")
        _same(fused.exp_avg, m, f"graph {g} exp_avg")
        _same([p.detach() for p in fused.params], [p.detach() for p in ps], f"graph {g} parameters")


class _Oracle:
    """scripts/train_ccn.py:31-73 in fp64: oracle.ref_ccn.ccn_forward, the normalised target, nn.MSELoss and
    torch.optim.Adamax stepping per graph; the meters by RunningAverage's rule."""

    def __init__(self, net, order):
        self.order, self.layers = order, net.layers
        self.p = {n: v.detach().cpu().double().clone().requires_grad_(True) for n, v in net.named_parameters()}
        self.names = [n for n, _ in net.named_parameters()]
        self.opt = torch.optim.Adamax([self.p[n] for n in self.names], lr=LR)
        self.noisy = {n: torch.zeros_like(self.p[n], dtype=torch.bool) for n in self.names}
        self.outs, self.loss, self.mae, self.run = [], None, None, [None, None]
        self.steps = 0

    def step(self, x, a, y):
        from oracle import ref_ccn as RC
        self.opt.zero_grad()
        out = RC.ccn_forward(self.p, x.double(), a.double(), self.order, self.layers)
        yn = (y.double() - MEAN) / (STD + 10 ** -8)
        loss = torch.nn.MSELoss()(out, yn)
        loss.backward()
        for n in self.names:
            g = self.p[n].grad.abs()
            self.noisy[n] |= (g > 0) & (g <= 1e-4 * g.max())
        self.opt.step()
        self.steps += 1
        self.outs.append(out.detach())
        self.loss, self.mae = loss.item(), (out.detach() - yn).abs().mean().item()
        for i, v in enumerate((self.loss, self.mae)):
            self.run[i] = v if self.run[i] is None else 0.9 * v + 0.1 * self.run[i]

    def compare(self, st, what):
        outs = torch.stack(self.outs)
        err = (st.out.double().cpu() - outs).abs()
        assert (err <= 1e-5 * outs.abs().clamp(min=1.0)).all(), f"{what}: out differs by {err.max().item():.3g}"
        got = st.stats.double().cpu().tolist()
        for v, r in zip(got, [self.loss, self.mae, *self.run]):
            assert abs(v - r) <= 1e-5 * max(1.0, abs(r)), (what, got, self.loss, self.mae, self.run)
        loose = total = 0
        for n, p in self.model_params(st):
            q = self.p[n].detach()
            e = (p.detach().double().cpu() - q).abs()
            tight = ~self.noisy[n]
            assert (e[tight] <= 1e-5 * q[tight].abs().clamp(min=1.0)).all(), (what, n, e[tight].max().item())
            assert e.max().item() <= 2 * LR * self.steps, (what, n, e.max().item())
            loose += int(self.noisy[n].sum())
            total += q.numel()
        assert loose <= 0.05 * total, f"{what}: {loose} of {total} elements on the loose bound"
        assert st.step_count == self.steps

    def model_params(self, st):
        return list(st.model.named_parameters())


def _against_oracle(net, order, graphs, fused, what):
    n_out = net.n_outputs
    orc = _Oracle(net, order)
    for x, a, t in graphs:
        orc.step(x, a, t[:n_out])
    st = _step(net.cuda(), fused=fused)
    X, A, nb, y = _pad(graphs, n_out)
    st.step(X, A, nb, y)
    orc.compare(st, what)
    return st


def test_fused_loop_against_the_fp64_oracle():
    """All graphs of A, then all of D (nine sequential steps, padded to D's 40 nodes) in one step call against
    the fp64 oracle stepping per graph, no re-synchronisation: every out[g], the final stats and every
    parameter element (the rule in the module docstring)."""
    graphs = _graphs("A") + _graphs("D")
    net = _model("A", 47)
    _assert_fused(net, 40)
    _against_oracle(net, 1, graphs, True, "fused A + D")


def test_unfused_loop_against_the_fp64_oracle():
    """fused=False (forward_batch, hgnn_mse_loss, backward, hgnn_adamax_step per graph) on shape A."""
    _against_oracle(_model("A", 47), 1, _graphs("A"), False, "unfused A")


def test_ccn2d_takes_the_unfused_loop():
    """CCN_2D(5, 1, 2, 2) on three graphs of 6-8 nodes against ccn_forward(order=2); fused=True raises."""
    import hgnn_amd.datagen as dg
    from hgnn_amd.train import CcnTrainStep
    from models.compnets.model_ccn import CCN_2D
    graphs = _self_loops(dg.qm9_shape_dataset(3, seed=702, n_min=6, n_max=8))
    net = _model("A", 52, CCN_2D)
    st = _against_oracle(net, 2, graphs, None, "CCN-2D")
    assert not st._supported(8)
    with pytest.raises(RuntimeError, match="fused=True"):
        CcnTrainStep(net, lr=LR, t_mean=MEAN, t_std=STD, fused=True)


def test_ragged_and_rejected_graphs():
    """Slots: a one-node graph, an empty slot (n_b = 0), a QM9-shape graph, a graph with a self loop removed, a
    QM9-shape graph.  The rejected graph takes no step: the final state is bitwise that of the list without
    it; the empty slot's out is fc.bias as it stood before that slot's own step; the next check raises the
    self-loop message, and a following clean call raises nothing."""
    from hgnn_amd.net import check_errors
    ga = _graphs("A")
    broken = ga[1][1].clone()
    broken[2, 2] = 0.0
    t = ga[0][2]
    slots = [(ga[0][0][:1], torch.ones(1, 1), t), (torch.zeros(0, 5), torch.zeros(0, 0), t), ga[0],
             (ga[1][0], broken, ga[1][2]), ga[2]]
    nmax = max(g[0].shape[0] for g in slots)
    _assert_fused(_model("A", 61), nmax)
    check_errors()
    full = _step(_model("A", 61).cuda())
    with pytest.raises(RuntimeError, match="self loop"):
        full.step(*_pad(slots, 1, nmax))  # HGNN_STRICT=1 (the suite's setting) reports here, after the call
        check_errors()
    clean = _step(_model("A", 61).cuda())
    clean.step(*_pad(slots[:3] + slots[4:], 1, nmax))
    check_errors()
    _same(_state(full), _state(clean), "rejected slot skipped")
    assert torch.equal(full.stats, clean.stats)
    assert torch.equal(full.out[[0, 1, 2, 4]], clean.out)
    _same([p.grad for p in full.params], [p.grad for p in clean.params], "last graph's gradients")
    first = _step(_model("A", 61).cuda())
    first.step(*_pad(slots[:1], 1, nmax))
    assert torch.equal(full.out[1], first.model.fc.bias.detach()), (full.out[1], first.model.fc.bias)
    assert not torch.equal(full.out[1], _model("A", 61).fc.bias.cuda())  # the one-node graph's step moved it


def test_evaluation_and_epochs():
    """evaluate against scripts/test_ccn.py's arithmetic on the oracle's outputs (per-graph MSE and MAE, plain
    means); two calls bitwise equal; eval_epoch in chunks of 4 equals evaluate on all six (the count-weighted
    combination); train_epoch in chunks of 4 leaves the parameters bitwise equal to one step over all six
    (the arithmetic does not depend on the padding)."""
    from oracle import ref_ccn as RC
    graphs = _graphs("A")
    net = _model("A", 73)
    p64 = {n: v.detach().double() for n, v in net.named_parameters()}
    mse, mae = [], []
    for x, a, t in graphs:
        d = RC.ccn_forward(p64, x.double(), a.double(), 1, net.layers) - (t[:1].double() - MEAN) / (STD + 10 ** -8)
        mse.append((d * d).mean().item())
        mae.append(d.abs().mean().item())
    ref = [sum(mse) / len(mse), sum(mae) / len(mae)]
    st = _step(net.cuda())
    X, A, nb, y = _pad(graphs, 1)
    r1 = st.evaluate(X, A, nb, y)
    r2 = st.evaluate(X, A, nb, y)
    assert torch.equal(r1, r2)
    for v, r in zip(r1.tolist(), ref):
        assert abs(v - r) <= 1e-5 * max(1.0, abs(r)), (r1, ref)
    # the reference's data: (X, A without self loops, targets, ...) 7-tuples
    data = [(x, a - torch.eye(a.shape[0]), t, None, None, None, None) for x, a, t in graphs]
    ev = st.eval_epoch(data, 0, chunk=4)
    for v, r in zip(ev, r1.tolist()):
        assert abs(v - r) <= 1e-6 * max(1.0, abs(r)), (ev, r1)
    loss, err = st.train_epoch(data, 0, chunk=4)
    whole = _step(_model("A", 73).cuda())
    s = whole.step(X, A, nb, y).tolist()
    _same(_state(st), _state(whole), "train_epoch in chunks")
    assert (loss, err) == (s[2], s[3])
    assert st.step_count == whole.step_count == 6
