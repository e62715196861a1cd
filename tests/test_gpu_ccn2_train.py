"""The device-resident CCN-2D training loop (hgnn_amd.train.CcnTrainStep on a CCN_2D model, hgnn_ccn2_small_train
and hgnn_ccn2_small_train_xent) against the library's own pieces (bitwise) and the fp64 oracle.

The loop is scripts/train_ccn.py:31-73 per graph: the target, net(X, A + I), the loss and its meters, backward, one
Adamax step; graph g + 1 sees the weights graph g left.  One workgroup runs it for a whole list in one dispatch,
on ONE graph's workspace region, so what the tests look for is a stale weight, a stale workspace row and a wrong
row index from the second graph on.

Shapes, all CCN_2D (targets t[:n_out], t_mean 0.3, t_std 1.7, lr 1e-3, weights from fixture_util.det_init, self
loops added; on the cross-entropy branch the label of graph g is g % n_out):
  P  (5, 1, 2, 2) on qm9_shape_dataset(6, seed=700): 14, 22, 13, 14, 22, 19 nodes, so sizes go up and down
  Q  (7, 2, 2, 3) on qm9_shape_dataset(6, seed=701, n_min=6, n_max=16), features widened to 7: two outputs,
     three levels
  R  (3, 1, 1, 1) on Q's graphs with X[:, :3]: hidden 1, one level
  S  (5, 1, 2, 2) at det_init(scale=0.02) on a complete 32-node graph with random one-hot features, then P[0] and
     P[1]: nmax at the bound, degree 32, a large graph before small ones.  Two levels of a 32-clique sum over
     32^2 entries twice, hence the small scale; the tests assert first that every output and gradient is finite.
  X  (5, 2, 2, 2) at det_init(scale=0.03) on qm9_shape_dataset(6, seed=702, n_min=6, n_max=8): logits O(1), so
     expf / logf run unsaturated (at scale 0.1 the fp64 oracle's logits reach +-75 on these graphs and half the
     losses are exactly 0)
  XQ Q's model and graphs at scale 0.03; XP model X on P's graphs at scale 0.02

Bitwise tests need no tolerance: at bs = 1 and nmax <= 32 forward_batch and its backward run k_ccn2_small_fwd and
k_ccn2_small_bwd, whose node functions the training kernel inlines; the loss and the optimizer kernels inline the
same row / element functions.  The one exception is the running cross entropy 0.9 v + 0.1 r, which each kernel
forms with its own instructions (one fma against two rounded products): each is within 2 * 2^-24 of the exact
sum, so the two are within 2^-22 of each other, relative (tests/test_gpu_ccn_xent.py).

Tolerances against the oracle are those of tests/test_gpu_ccn_train.py, copied: values within 1e-5 max(1, |ref|);
parameters after K Adamax steps within 1e-5 max(1, |p|) where the oracle's gradient was above the noise floor
(1e-4 max|g| of its tensor) at every step or exactly 0, else within 2 lr K -- and that second class may hold at
most 5 % of the elements.
"""

import ctypes

import pytest
import torch

import fixture_util as fu

pytestmark = pytest.mark.gpu

MEAN, STD, LR = 0.3, 1.7, 1e-3

# shape -> (model arguments, det_init scale)
SHAPES = {"P": ((5, 1, 2, 2), 0.1), "Q": ((7, 2, 2, 3), 0.1), "R": ((3, 1, 1, 1), 0.1), "S": ((5, 1, 2, 2), 0.02),
          "X": ((5, 2, 2, 2), 0.03), "XQ": ((7, 2, 2, 3), 0.03), "XP": ((5, 2, 2, 2), 0.02)}
_cache = {}


def _self_loops(graphs):
    return [(X, A + torch.eye(A.shape[0]), t) for X, A, t in graphs]


def _graphs(shape):
    import hgnn_amd.datagen as dg
    if shape in _cache:
        return _cache[shape]
    if shape in ("P", "XP"):
        gs = _self_loops(dg.qm9_shape_dataset(6, seed=700))
    elif shape in ("Q", "XQ", "R"):
        gen = torch.Generator().manual_seed(701)
        gs = _self_loops(dg.qm9_shape_dataset(6, seed=701, n_min=6, n_max=16))
        if shape == "R":
            gs = [(X[:, :3].contiguous(), A, t) for X, A, t in gs]
        else:
            gs = [(torch.cat([X, torch.rand(X.shape[0], 2, generator=gen)], 1), A, t) for X, A, t in gs]
    elif shape == "S":
        gen = torch.Generator().manual_seed(32)
        p = _graphs("P")
        x = torch.nn.functional.one_hot(torch.randint(0, 5, (32,), generator=gen), 5).float()
        gs = [(x, torch.ones(32, 32), p[0][2])] + p[:2]
    elif shape == "X":
        gs = _self_loops(dg.qm9_shape_dataset(6, seed=702, n_min=6, n_max=8))
    else:
        raise KeyError(shape)
    _cache[shape] = gs
    return gs


def _model(shape, seed):
    from models.compnets.model_ccn import CCN_2D
    args, scale = SHAPES[shape]
    net = CCN_2D(*args)
    fu.det_init(net, seed, scale)
    return net


def _pad(graphs, n_out, nmax=None, labels=None):
    bs = len(graphs)
    nmax = nmax or max(g[0].shape[0] for g in graphs)
    X = torch.zeros(bs, nmax, graphs[0][0].shape[1])
    A = torch.zeros(bs, nmax, nmax)
    for b, g in enumerate(graphs):
        n = g[0].shape[0]
        X[b, :n] = g[0]
        A[b, :n, :n] = g[1]
    nb = torch.tensor([g[0].shape[0] for g in graphs], dtype=torch.int64)
    if labels is not None:
        y = torch.tensor(labels)
    else:
        y = torch.stack([t[:n_out] for _, _, t in graphs]).float()
    return X.cuda(), A.cuda(), nb.cuda(), y.cuda()


def _labels(count, n_out):
    return [g % n_out for g in range(count)]


def _batch(shape, xent):
    graphs = _graphs(shape)
    n_out = SHAPES[shape][0][1]
    return _pad(graphs, n_out, labels=_labels(len(graphs), n_out) if xent else None)


def _step(net, fused="ccn2", xent=False):
    from hgnn_amd.train import CcnTrainStep
    if xent:
        return CcnTrainStep(net, lr=LR, classification=True, fused=fused)
    return CcnTrainStep(net, lr=LR, t_mean=MEAN, t_std=STD, fused=fused)


def _state(st):
    return [p.detach().clone() for p in st.params] + [t.clone() for t in st.exp_avg + st.exp_inf]


def _same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"{what}: tensor {i} differs by {(x - y).abs().max().item():.3g}"


def _assert_supported(shape, nmax):
    from hgnn_amd import _lib
    cfg = _model(shape, 1)._spec().config(1, nmax)
    assert _lib.lib().hgnn_ccn2_small_train_supported(ctypes.byref(cfg)) == 1


def test_shapes_are_what_the_tests_rely_on():
    p = [x.shape[0] for x, _, _ in _graphs("P")]
    assert p == [14, 22, 13, 14, 22, 19], p
    s = _graphs("S")
    assert s[0][0].shape[0] == 32 and int((s[0][1] > 0).sum(1).min()) == 32
    assert [x.shape[0] for x, _, _ in s[1:]] == p[:2]
    assert max(x.shape[0] for x, _, _ in _graphs("Q")) <= 16 and _graphs("Q")[0][0].shape[1] == 7
    assert all(6 <= x.shape[0] <= 8 for x, _, _ in _graphs("X"))


def _k_steps(shape, xent):
    graphs = _graphs(shape)
    X, A, nb, y = _batch(shape, xent)
    _assert_supported(shape, X.shape[1])
    many = _step(_model(shape, 21).cuda(), xent=xent)
    many.step(X, A, nb, y)
    assert many.path == "fused2d"
    if shape == "S":
        assert torch.isfinite(many.out).all(), many.out
        assert all(torch.isfinite(p.grad).all() for p in many.params)
    one = _step(_model(shape, 21).cuda(), xent=xent)
    outs = []
    for g in range(len(graphs)):
        one.step(X[g:g + 1], A[g:g + 1], nb[g:g + 1], y[g:g + 1])
        outs.append(one.out.clone())
    assert torch.equal(many.out, torch.cat(outs)), (many.out, torch.cat(outs))
    _same(_state(many), _state(one), f"shape {shape}")
    assert torch.equal(many.stats, one.stats), (many.stats, one.stats)
    assert many.step_count == one.step_count == len(graphs)
    _same([p.grad for p in many.params], [p.grad for p in one.params], "last graph's gradients")
    return (many.params[0].detach() - _model(shape, 21).w1.weight.cuda()).abs().max().item()


@pytest.mark.parametrize("shape", ["P", "S"])
def test_k_steps_in_one_dispatch_equal_k_one_graph_dispatches(shape):
    """The fences, the re-reading of the weights and the reused workspace: step on all graphs at once against
    step called per graph (both the fused kernel).  The multi-graph call runs first, on parameters no other
    kernel has read yet.  Parameters, optimizer state, out, stats, step_count and the last graph's gradients
    are bitwise equal, and the weights moved at every step (Adamax's first steps are ~lr each)."""
    moved = _k_steps(shape, False)
    assert moved > 0.5 * LR * len(_graphs(shape)), moved


@pytest.mark.parametrize("shape", ["X", "XQ", "XP"])
def test_k_steps_in_one_dispatch_equal_k_one_graph_dispatches_xent(shape):
    """The same on the cross-entropy branch.  The steps were taken; alternating labels pull the weights back and
    forth, so there is no lr K drift to assert (as in tests/test_gpu_ccn_xent.py)."""
    assert _k_steps(shape, True) > 0


def _pieces(shape, xent):
    from hgnn_amd import _lib as L
    lib = L.lib()
    graphs = _graphs(shape)
    n_out = SHAPES[shape][0][1]
    X, A, nb, y = _batch(shape, xent)
    yf = y.float()
    _assert_supported(shape, X.shape[1])
    fused = _step(_model(shape, 33).cuda(), xent=xent)
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
        assert fused.path == "fused2d"
        for p in ps:
            p.grad = None
        out = net.forward_batch(X[g:g + 1], A[g:g + 1], nb[g:g + 1])
        dout = torch.empty_like(out)
        if xent:
            L.check(lib.hgnn_xent_loss(L.ptr(out.detach()), L.ptr(yf[g:g + 1]), 1, n_out, L.ptr(stats), L.ptr(dout),
                                       L.ptr(err), stream), "xent")
        else:
            yn = ((y[g].cpu() - MEAN) / (STD + 10 ** -8)).cuda()  # train_ccn.py:42, before .cuda()
            L.check(lib.hgnn_mse_loss(L.ptr(out.detach()), L.ptr(yn), n_out, 0.0, 1.0, L.ptr(stats), L.ptr(dout),
                                      stream), "mse")
        torch.autograd.backward(out, dout)
        grads = [p.grad for p in ps]
        L.check(lib.hgnn_adamax_step(len(ps), L.ptr_array(ps), L.ptr_array(grads), L.ptr_array(m), L.ptr_array(u),
                                     numel, LR, 0.9, 0.999, 1e-8, 0.0, g + 1, stream), "adamax")
        if shape == "S":
            assert torch.isfinite(out).all() and all(torch.isfinite(gr).all() for gr in grads), (g, out)
        assert torch.equal(fused.out, out.detach()), (g, fused.out, out)
        if xent:
            assert torch.equal(st[0], stats[0]), (g, st.tolist(), stats.tolist())
            assert st[0].item() >= 0 and st[1].item() == 0 and st[3].item() == 0, st
            assert abs(st[2].item() - stats[2].item()) <= 2.0 ** -22 * stats[2].item(), (g, st.tolist(),
                                                                                         stats.tolist())
        else:
            assert torch.equal(st[:2], stats[:2]), (g, st, stats)
        _same([p.grad for p in fused.params], grads, f"graph {g} gradients")
        _same(fused.exp_inf, u, f"graph {g} exp_inf")
        _same(fused.exp_avg, m, f"graph {g} exp_avg")
        _same([p.detach() for p in fused.params], [p.detach() for p in ps], f"graph {g} parameters")
    assert int(err.item()) == 0


@pytest.mark.parametrize("shape", ["P", "Q", "R", "S"])
def test_one_fused_step_equals_the_librarys_own_pieces(shape):
    """Graph by graph, from the state the previous graphs left (so the moments and the step count are not
    trivial): CcnTrainStep(fused="ccn2").step on the one-graph slice against forward_batch, hgnn_mse_loss on the
    CPU-normalised target with (0, 1), autograd backward and hgnn_adamax_step.  Bitwise: out, every p.grad,
    stats[0:2], both moments and the parameters."""
    _pieces(shape, False)


@pytest.mark.parametrize("shape", ["X", "XQ", "XP"])
def test_one_fused_step_equals_the_librarys_own_pieces_xent(shape):
    """The same against hgnn_xent_loss with n = 1: stats[0] exactly, stats[2] within 2^-22 relative (module
    docstring), stats[1] and stats[3] stay 0."""
    _pieces(shape, True)


class _Oracle:
    """scripts/train_ccn.py:31-73 in fp64 (tests/test_gpu_ccn_train.py's and tests/test_gpu_ccn_xent.py's _Oracle
    in one): oracle.ref_ccn.ccn_forward(order=2), the loss and torch.optim.Adamax stepping per graph; the meters by
    RunningAverage's rule.  xent False: MSE on the normalised target; True: nn.CrossEntropyLoss on out.view(1, -1)."""

    def __init__(self, net, xent):
        self.layers, self.xent = net.layers, xent
        self.p = {n: v.detach().cpu().double().clone().requires_grad_(True) for n, v in net.named_parameters()}
        self.names = [n for n, _ in net.named_parameters()]
        self.opt = torch.optim.Adamax([self.p[n] for n in self.names], lr=LR)
        self.noisy = {n: torch.zeros_like(self.p[n], dtype=torch.bool) for n in self.names}
        self.outs, self.loss, self.mae, self.run, self.losses = [], None, 0.0, [None, None], []
        self.steps = 0

    def step(self, x, a, y, label):
        from oracle import ref_ccn as RC
        self.opt.zero_grad()
        out = RC.ccn_forward(self.p, x.double(), a.double(), 2, self.layers)
        if self.xent:
            loss = torch.nn.CrossEntropyLoss()(out.view(1, -1), torch.tensor([label]))
        else:
            yn = (y.double() - MEAN) / (STD + 10 ** -8)
            loss = torch.nn.MSELoss()(out, yn)
        loss.backward()
        for n in self.names:
            g = self.p[n].grad.abs()
            self.noisy[n] |= (g > 0) & (g <= 1e-4 * g.max())
        self.opt.step()
        self.steps += 1
        self.outs.append(out.detach().view(-1))
        self.loss = loss.item()
        self.losses.append(self.loss)
        vals = [self.loss] if self.xent else [self.loss, (out.detach() - yn).abs().mean().item()]
        self.mae = 0.0 if self.xent else vals[1]
        for i, v in enumerate(vals):
            self.run[i] = v if self.run[i] is None else 0.9 * v + 0.1 * self.run[i]

    def loose(self):
        return sum(int(v.sum()) for v in self.noisy.values()), sum(v.numel() for v in self.noisy.values())

    def compare(self, st, what):
        outs = torch.stack(self.outs)
        err = (st.out.double().cpu() - outs).abs()
        print(f"{what}: max out error {(err / outs.abs().clamp(min=1.0)).max().item():.3g}")
        assert (err <= 1e-5 * outs.abs().clamp(min=1.0)).all(), f"{what}: out differs by {err.max().item():.3g}"
        got = st.stats.double().cpu().tolist()
        ref = [self.loss, self.mae, self.run[0], 0.0 if self.xent else self.run[1]]
        for v, r in zip(got, ref):
            assert abs(v - r) <= 1e-5 * max(1.0, abs(r)), (what, got, ref)
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


def _oracle(xent):
    """The oracle's six steps, computed once and left unchanged: (oracle, graphs, labels)."""
    key = ("oracle", xent)
    if key not in _cache:
        graphs = _graphs("X")
        labels = _labels(6, 2) if xent else [None] * 6
        net = _model("X" if xent else "P", 52)  # X: (5, 2, 2, 2) at 0.03; P: (5, 1, 2, 2) at 0.1
        orc = _Oracle(net, xent)
        for (x, a, t), lb in zip(graphs, labels):
            orc.step(x, a, t[:1], lb)
        _cache[key] = (orc, graphs, labels)
    return _cache[key]


@pytest.mark.parametrize("fused", ["ccn2", False], ids=["fused2d", "unfused"])
def test_mse_loop_against_the_fp64_oracle(fused):
    """CCN_2D(5, 1, 2, 2), det_init(net, 52), the six graphs of qm9_shape_dataset(6, seed=702, n_min=6, n_max=8)
    (the first three are tests/test_gpu_ccn_train.py's CCN-2D graphs) in one step call, against the fp64 oracle
    stepping per graph.  The oracle itself puts 0 of 266 elements in the loose class."""
    orc, graphs, _ = _oracle(False)
    assert orc.loose() == (0, 266), orc.loose()
    st = _step(_model("P", 52).cuda(), fused=fused)
    st.step(*_pad(graphs, 1))
    assert st.path == ("fused2d" if fused else "unfused")
    orc.compare(st, f"CCN-2D mse fused={fused}")


@pytest.mark.parametrize("fused", ["ccn2", False], ids=["fused2d", "unfused"])
def test_xent_loop_against_the_fp64_oracle(fused):
    """CCN_2D(5, 2, 2, 2), det_init(net, 52, 0.03), the same graphs, labels g % 2.  The oracle puts 3 of 276
    elements in the loose class, and its losses run from 0.0026 to 4.2: no row is saturated."""
    orc, graphs, labels = _oracle(True)
    assert orc.loose() == (3, 276), orc.loose()
    assert 0.002 < min(orc.losses) < 0.003 and 4.0 < max(orc.losses) < 4.4, orc.losses
    st = _step(_model("X", 52).cuda(), fused=fused, xent=True)
    st.step(*_pad(graphs, 2, labels=labels))
    assert st.path == ("fused2d" if fused else "unfused")
    orc.compare(st, f"CCN-2D xent fused={fused}")


def test_ragged_and_rejected_graphs():
    """Slots: a one-node graph, an empty slot (n_b = 0), a P graph, a P graph with one self loop removed, a P
    graph.  The rejected graph takes no step: the final state is bitwise that of the list without it; the empty
    slot's out is fc.bias as the previous step left it; the next check raises the self-loop message, and a
    following clean call raises nothing."""
    from hgnn_amd.net import check_errors
    gp = _graphs("P")
    broken = gp[1][1].clone()
    broken[2, 2] = 0.0
    t = gp[0][2]
    slots = [(gp[0][0][:1], torch.ones(1, 1), t), (torch.zeros(0, 5), torch.zeros(0, 0), t), gp[0],
             (gp[1][0], broken, gp[1][2]), gp[2]]
    nmax = max(g[0].shape[0] for g in slots)
    check_errors()
    full = _step(_model("P", 61).cuda())
    with pytest.raises(RuntimeError, match="self loop"):
        full.step(*_pad(slots, 1, nmax))  # HGNN_STRICT=1 (the suite's setting) reports here, after the call
        check_errors()
    clean = _step(_model("P", 61).cuda())
    clean.step(*_pad(slots[:3] + slots[4:], 1, nmax))
    check_errors()
    assert full.path == clean.path == "fused2d"
    _same(_state(full), _state(clean), "rejected slot skipped")
    assert torch.equal(full.stats, clean.stats)
    assert torch.equal(full.out[[0, 1, 2, 4]], clean.out)
    assert full.step_count == 5 and clean.step_count == 4  # step_count counts the rejected graph too
    _same([p.grad for p in full.params], [p.grad for p in clean.params], "last graph's gradients")
    first = _step(_model("P", 61).cuda())
    first.step(*_pad(slots[:1], 1, nmax))
    assert torch.equal(full.out[1], first.model.fc.bias.detach()), (full.out[1], first.model.fc.bias)
    assert not torch.equal(full.out[1], _model("P", 61).fc.bias.cuda())  # the one-node graph's step moved it


def test_bad_class_targets_are_skipped_like_rejected_graphs():
    """Five slots of X's graphs with targets [0, 1, 2 (out of range), 0.5 (not an integer), 1]: the two graphs
    take no step -- state, stats and the other out rows are bitwise those of the three-graph list; the next check
    raises the class-target message, and a following clean call raises nothing."""
    from hgnn_amd.net import check_errors
    gx = _graphs("X")[:5]
    nmax = max(g[0].shape[0] for g in gx)
    check_errors()
    full = _step(_model("X", 61).cuda(), xent=True)
    with pytest.raises(RuntimeError, match="class target"):
        full.step(*_pad(gx, 2, nmax, labels=[0.0, 1.0, 2.0, 0.5, 1.0]))
        check_errors()
    check_errors()  # the word was consumed
    clean = _step(_model("X", 61).cuda(), xent=True)
    clean.step(*_pad([gx[0], gx[1], gx[4]], 2, nmax, labels=[0.0, 1.0, 1.0]))
    check_errors()
    assert full.path == clean.path == "fused2d"
    _same(_state(full), _state(clean), "rejected slots skipped")
    assert torch.equal(full.stats, clean.stats)
    assert torch.equal(full.out[[0, 1, 4]], clean.out)
    _same([p.grad for p in full.params], [p.grad for p in clean.params], "last graph's gradients")
    assert torch.isfinite(full.out[2:4]).all() and not torch.equal(full.out[2], full.out[3])


def test_routing():
    """Which path runs: fused="ccn2" -> "fused2d", and it raises on a CCN_1D model and at nmax = 33;
    fused=False -> "unfused"; fused=None takes the kernel where it is supported (the measured default: its median
    per graph is below the unfused loop's in tools/ab_ccn_train.py --order 2) and runs a chunk padded to 33
    nodes unfused, with parameters bitwise those of the fused=False run; train_epoch in chunks of 4 equals one
    step over all six graphs."""
    from hgnn_amd.train import CcnTrainStep
    from models.compnets.model_ccn import CCN_1D
    graphs = _graphs("P")
    X, A, nb, y = _pad(graphs, 1)
    st = _step(_model("P", 73).cuda())
    st.step(X, A, nb, y)
    assert st.path == "fused2d"
    assert st._supported2d(32) and not st._supported2d(33) and not st._supported(22)
    net1 = CCN_1D(5, 1, 2, 2)
    fu.det_init(net1, 73)
    with pytest.raises(RuntimeError, match="ccn2"):
        CcnTrainStep(net1.cuda(), lr=LR, t_mean=MEAN, t_std=STD, fused="ccn2")
    X33, A33, nb33, y33 = _pad(graphs, 1, nmax=33)
    with pytest.raises(RuntimeError, match="ccn2"):
        _step(_model("P", 73).cuda()).step(X33, A33, nb33, y33)
    off = _step(_model("P", 73).cuda(), fused=False)
    off.step(X33, A33, nb33, y33)
    assert off.path == "unfused"
    auto = _step(_model("P", 73).cuda(), fused=None)
    auto.step(X33, A33, nb33, y33)
    assert auto.path == "unfused"
    _same(_state(auto), _state(off), "a chunk padded to 33 nodes")
    auto.step(X, A, nb, y)
    assert auto.path == "fused2d"
    # the reference's data: (X, A without self loops, targets, ...) 7-tuples
    data = [(x, a - torch.eye(a.shape[0]), t, None, None, None, None) for x, a, t in graphs]
    ep = _step(_model("P", 73).cuda())
    loss, err = ep.train_epoch(data, 0, chunk=4)
    s = st.stats.tolist()
    _same(_state(ep), _state(st), "train_epoch in chunks")
    assert (loss, err) == (s[2], s[3])
    assert ep.step_count == st.step_count == 6
    assert list(ep._ws2d) == [22]  # both chunks are padded to 22 nodes: one workspace, allocated once and kept
