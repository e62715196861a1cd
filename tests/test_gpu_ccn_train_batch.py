"""CCN mini-batch training (hgnn_amd.train.CcnTrainStep(batch_size=B), hgnn_ccn_small_train_batch) against the
library's own pieces (bitwise) and the fp64 oracle.

A mini-batch is B consecutive graphs on the same weights: out_g = net(X_g, A_g + I), yn = (y - mean) / (std + 1e-8),
nn.MSELoss over the (B, n_out) block, the parameter gradients summed over the graphs, one optimizer step; the last
mini-batch of a list is shorter and divides by its own size.  Classification: nn.CrossEntropyLoss on the (B, n_out)
logits.  Inputs, MEAN, STD, LR, det_init seeds and shape names are those of tests/test_gpu_ccn_train.py:
  A   CCN_1D(5, 1, 2, 2) on qm9_shape_dataset(6, seed=700): B = 4 gives mini-batches of 4 and 2
  B   CCN_1D(7, 2, 5, 3) on its widened graphs
  DA  model A on D (a 40-node SBM graph + two of A's) followed by A: nine graphs padded to 40 nodes, so graphs of
      8, 16 and 32 lanes per node all occur and B = 4 leaves a last mini-batch of one graph
The bitwise results follow from the shared device functions (csrc/ccn_small.h, csrc/kernels.h) and the shared
summation order (k_ccn1_small_reduce's).  Tolerances against the oracle are those of tests/test_gpu_ccn_train.py
(its module docstring); tests/test_ccn_train_batch_cpu.py checks on the CPU that the inputs meet the 5 % cap."""

import ctypes

import pytest
import torch

import ccn_batch_util as U
from test_gpu_ccn_train import LR, MEAN, MODELS, STD, _assert_fused, _graphs, _model, _pad, _same

pytestmark = pytest.mark.gpu


def _case_graphs(shape):
    return _graphs("D") + _graphs("A") if shape == "DA" else _graphs(shape)


def _case_model(shape, seed, cls=None):
    return _model("A" if shape == "DA" else shape, seed, cls)


def _step(net, B, fused=True, **kw):
    from hgnn_amd.train import CcnTrainStep
    kw.setdefault("t_mean", MEAN)
    kw.setdefault("t_std", STD)
    return CcnTrainStep(net, lr=LR, fused=fused, batch_size=B, **kw)


def _states(st):
    if st.optimizer == "sgd":
        return list(st.momentum_buffer)
    return list(st.exp_avg) + list(st.exp_avg_sq if st.optimizer == "adam" else st.exp_inf)


def _state(st):
    return [p.detach().clone() for p in st.params] + [t.clone() for t in _states(st)]


class _Pieces:
    """The library's pieces run by hand on one mini-batch at a time: forward_batch, hgnn_mse_loss on the CPU-normalised
    target with (0, 1) (or hgnn_xent_loss), autograd backward, hgnn_optim_step."""

    def __init__(self, net, optimizer="adamax", cls=False):
        from hgnn_amd import _lib as L
        self.L, self.lib = L, L.lib()
        self.net, self.ps = net, net._params()
        self.kind = L.OPT_KIND[optimizer]
        self.s1 = [torch.zeros_like(p) for p in self.ps]
        self.s2 = None if optimizer == "sgd" else [torch.zeros_like(p) for p in self.ps]
        self.numel = (ctypes.c_int64 * len(self.ps))(*[p.numel() for p in self.ps])
        self.stats = torch.zeros(4, device="cuda")
        self.err = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.cls, self.t = cls, 0

    def step(self, X, A, nb, y):
        L, lib = self.L, self.lib
        stream = L.stream_handle(X.device)
        for p in self.ps:
            p.grad = None
        out = self.net.forward_batch(X, A, nb)
        dout = torch.empty_like(out)
        if self.cls:
            L.check(lib.hgnn_xent_loss(L.ptr(out.detach()), L.ptr(y), out.shape[0], out.shape[1], L.ptr(self.stats),
                                       L.ptr(dout), L.ptr(self.err), stream), "xent")
        else:
            yn = ((y.cpu() - MEAN) / (STD + 10 ** -8)).cuda()  # train_ccn.py:42, before .cuda()
            L.check(lib.hgnn_mse_loss(L.ptr(out.detach()), L.ptr(yn), out.numel(), 0.0, 1.0, L.ptr(self.stats),
                                      L.ptr(dout), stream), "mse")
        torch.autograd.backward(out, dout)
        self.grads = [p.grad for p in self.ps]
        self.t += 1
        L.check(lib.hgnn_optim_step(self.kind, len(self.ps), L.ptr_array(self.ps), L.ptr_array(self.grads),
                                    L.ptr_array(self.s1), None if self.s2 is None else L.ptr_array(self.s2),
                                    self.numel, LR, 0.9, 0.999, 1e-8, 0.0, self.t, stream), "optimizer")
        return out.detach()

    def state(self):
        return [p.detach() for p in self.ps] + self.s1 + (self.s2 or [])


def _fused_against_pieces(fused, pieces, X, A, nb, y, B, what, stats=slice(0, 2)):
    """Per mini-batch, each side from the state its own previous mini-batches left."""
    for g0 in range(0, X.shape[0], B):
        sl = slice(g0, g0 + B)
        st = fused.step(X[sl], A[sl], nb[sl], y[sl])
        out = pieces.step(X[sl], A[sl], nb[sl], y[sl])
        assert torch.equal(fused.out, out), (what, g0, fused.out, out)
        _same([p.grad for p in fused.params], pieces.grads, f"{what}: mini-batch at {g0}, gradients")
        if stats is not None:
            assert torch.equal(st[stats], pieces.stats[stats]), (what, g0, st, pieces.stats)
        _same(_state(fused), pieces.state(), f"{what}: mini-batch at {g0}, parameters and optimizer state")
    assert fused.step_count == pieces.t


@pytest.mark.parametrize("shape,optimizer", [("A", "adamax"), ("B", "adamax"), ("DA", "adamax"), ("A", "sgd"),
                                             ("A", "adam")])
def test_fused_step_equals_the_librarys_pieces(shape, optimizer):
    """Test 1.  B = 4: out, every p.grad, stats[0:2], both optimizer states and the parameters, bitwise, after every
    mini-batch (the moments and the step count are not trivial from the second one on)."""
    graphs = _case_graphs(shape)
    n_out = _case_model(shape, 33).n_outputs
    X, A, nb, y = _pad(graphs, n_out)
    _assert_fused(_case_model(shape, 33), X.shape[1])
    fused = _step(_case_model(shape, 33).cuda(), 4, optimizer=optimizer)
    pieces = _Pieces(_case_model(shape, 33).cuda(), optimizer)
    _fused_against_pieces(fused, pieces, X, A, nb, y, 4, f"{shape} {optimizer}")
    assert fused.path == "batch_fused"
    assert fused.step_count == -(-len(graphs) // 4)


@pytest.mark.parametrize("shape", ["A", "DA"])
def test_k_minibatches_in_one_call_equal_k_calls(shape):
    """Test 2.  The workspace regions reused in stream order, one reject word and one d_steps row per mini-batch:
    parameters, states, out, stats and step_count, bitwise."""
    graphs = _case_graphs(shape)
    X, A, nb, y = _pad(graphs, 1)
    many = _step(_case_model(shape, 21).cuda(), 4)
    many.step(X, A, nb, y)
    one = _step(_case_model(shape, 21).cuda(), 4)
    outs = []
    for g0 in range(0, len(graphs), 4):
        one.step(X[g0:g0 + 4], A[g0:g0 + 4], nb[g0:g0 + 4], y[g0:g0 + 4])
        outs.append(one.out.clone())
    _same(_state(many), _state(one), f"shape {shape}")
    assert torch.equal(many.out, torch.cat(outs))
    assert torch.equal(many.stats, one.stats), (many.stats, one.stats)
    assert many.step_count == one.step_count == -(-len(graphs) // 4)
    _same([p.grad for p in many.params], [p.grad for p in one.params], "last mini-batch's gradients")
    moved = (many.params[0].detach() - _case_model(shape, 21).w1.weight.cuda()).abs().max().item()
    assert moved > 0.5 * LR * many.step_count, moved


def test_batch_size_one_equals_the_per_graph_fused_loop():
    """Test 3.  batch_size=1 against batch_size=None, fused=True on shape A: out, parameters, states, stats[0:2]."""
    from hgnn_amd.train import CcnTrainStep
    X, A, nb, y = _pad(_graphs("A"), 1)
    mini = _step(_model("A", 21).cuda(), 1)
    mini.step(X, A, nb, y)
    loop = CcnTrainStep(_model("A", 21).cuda(), lr=LR, t_mean=MEAN, t_std=STD, fused=True)
    loop.step(X, A, nb, y)
    assert (mini.path, loop.path) == ("batch_fused", "fused")
    assert torch.equal(mini.out, loop.out)
    _same(_state(mini), _state(loop), "batch_size=1 against the per-graph loop")
    assert torch.equal(mini.stats[:2], loop.stats[:2]), (mini.stats, loop.stats)
    assert mini.step_count == loop.step_count == 6


def test_ccn2d_takes_the_pieces_route():
    """Test 4.  CCN_2D(5, 1, 2, 2), B = 2 (mini-batches of 2, 2 and 1): .path == "batch", bitwise the pieces run
    by hand; fused=True and fused="ccn2" raise."""
    from hgnn_amd.train import CcnTrainStep
    graphs = U.graphs_2d()
    X, A, nb, y = _pad(graphs, 1)
    st = _step(U.model_2d(52).cuda(), 2, fused=None)
    pieces = _Pieces(U.model_2d(52).cuda())
    _fused_against_pieces(st, pieces, X, A, nb, y, 2, "CCN-2D")
    assert st.path == "batch"
    assert st.step_count == 3
    with pytest.raises(RuntimeError, match="fused=True"):
        _step(U.model_2d(52).cuda(), 2, fused=True)
    with pytest.raises(RuntimeError, match="ccn2"):
        CcnTrainStep(U.model_2d(52).cuda(), lr=LR, t_mean=MEAN, t_std=STD, fused="ccn2", batch_size=2)


@pytest.mark.parametrize("case,fused,path", [("A-b4", True, "batch_fused"), ("DA-b4", True, "batch_fused"),
                                             ("B-b4", True, "batch_fused"), ("B-b2", True, "batch_fused"),
                                             ("2D-b2", None, "batch"), ("2D-b5", None, "batch"),
                                             ("A-b4", False, "batch")])
def test_against_the_fp64_oracle(case, fused, path):
    """Test 5.  One step call over the whole list against the fp64 oracle stepping per mini-batch: every out row and
    the meters within 1e-5 max(1, |ref|); parameters within 1e-5 max(1, |p|) where the oracle's gradient stayed
    above 1e-4 max|g| of its tensor at every step, else within 2 lr K, and that class at most 5 % of the elements."""
    net, graphs, B, orc = U.run_oracle(case)
    st = _step(net.cuda(), B, fused=fused)
    st.step(*_pad(graphs, net.n_outputs))
    assert st.path == path
    orc.compare(st, f"{case} {path}")


def _slots():
    ga = _graphs("A")
    broken = ga[1][1].clone()
    broken[2, 2] = 0.0
    t = ga[0][2]
    return [(ga[0][0][:1], torch.ones(1, 1), t), (torch.zeros(0, 5), torch.zeros(0, 0), t), ga[0],
            (ga[1][0], broken, ga[1][2]), ga[2]]


def test_ragged_and_rejected_graphs():
    """Test 6.  Slots: a one-node graph, an empty slot | a QM9-shape graph, a graph with a self loop removed | a
    QM9-shape graph, B = 2.  The middle mini-batch takes no step: parameters, states and stats are bitwise those of a
    run over the other two alone -- with the rejected mini-batch's step number left out, since row k of the step
    scalars belongs to mini-batch k whether or not it is applied; its other graph's out row is written; the next
    check raises the self-loop message and a following clean call raises nothing."""
    from hgnn_amd.net import check_errors
    slots = _slots()
    nmax = max(g[0].shape[0] for g in slots)
    _assert_fused(_model("A", 61), nmax)
    check_errors()
    X, A, nb, y = _pad(slots, 1, nmax)
    full = _step(_model("A", 61).cuda(), 2)
    full.out = None
    with pytest.raises(RuntimeError, match="self loop"):
        full.step(X, A, nb, y)  # HGNN_STRICT=1 (the suite's setting) reports here, after the call
        check_errors()
    assert full.step_count == 3
    clean = _step(_model("A", 61).cuda(), 2)
    clean.step(X[:2], A[:2], nb[:2], y[:2])
    out01 = clean.out.clone()
    with torch.no_grad():  # what graph 2 saw: the weights the first mini-batch left
        out2 = clean.model.forward_batch(X[2:3], A[2:3], nb[2:3])
    clean.step_count += 1  # the rejected mini-batch's number
    clean.step(X[4:], A[4:], nb[4:], y[4:])
    check_errors()
    _same(_state(full), _state(clean), "rejected mini-batch skipped")
    assert torch.equal(full.stats, clean.stats), (full.stats, clean.stats)
    assert torch.equal(full.out[[0, 1, 4]], torch.cat([out01, clean.out]))
    assert torch.equal(full.out[2], out2[0]), (full.out[2], out2)
    _same([p.grad for p in full.params], [p.grad for p in clean.params], "last mini-batch's gradients")
    # the empty slot's output is fc.bias as the mini-batch saw it
    assert torch.equal(full.out[1], _model("A", 61).fc.bias.cuda())


def test_the_empty_slots_minibatch_equals_the_pieces_route():
    """Test 6, last point: [one-node graph, empty slot] through the kernels and through fused=False."""
    slots = _slots()
    nmax = max(g[0].shape[0] for g in slots)
    X, A, nb, y = _pad(slots[:2], 1, nmax)
    a = _step(_model("A", 61).cuda(), 2, fused=True)
    b = _step(_model("A", 61).cuda(), 2, fused=False)
    sa, sb = a.step(X, A, nb, y), b.step(X, A, nb, y)
    assert (a.path, b.path) == ("batch_fused", "batch")
    assert torch.equal(a.out, b.out)
    assert torch.equal(sa, sb), (sa, sb)
    _same(_state(a), _state(b), "empty slot's mini-batch")
    _same([p.grad for p in a.params], [p.grad for p in b.params], "gradients")
    # the empty slot contributes to the loss and to fc.bias's gradient: dout of its row is 2 (bias - yn) / 2
    assert a.params[-1].grad.abs().max().item() > 0


def _cls_inputs(targets):
    graphs = _graphs("A")
    X, A, nb, _ = _pad(graphs, 1)
    return X, A, nb, torch.tensor(targets, dtype=torch.float32).cuda()


def _cls_model(seed):
    import fixture_util as fu
    from models.compnets.model_ccn import CCN_1D
    net = CCN_1D(5, 3, 2, 2)
    fu.det_init(net, seed)
    return net


def test_classification_equals_the_pieces():
    """Test 7.  CCN_1D(5, 3, 2, 2) on shape A, class g % 3, B = 4, against the pieces with hgnn_xent_loss: out,
    gradients, states and parameters bitwise; stats[0] within 1e-6 relative."""
    X, A, nb, y = _cls_inputs([g % 3 for g in range(6)])
    fused = _step(_cls_model(33).cuda(), 4, classification=True, t_mean=None)
    pieces = _Pieces(_cls_model(33).cuda(), cls=True)
    for g0 in (0, 4):
        sl = slice(g0, g0 + 4)
        st = fused.step(X[sl], A[sl], nb[sl], y[sl])
        out = pieces.step(X[sl], A[sl], nb[sl], y[sl])
        assert torch.equal(fused.out, out)
        _same([p.grad for p in fused.params], pieces.grads, f"mini-batch at {g0}, gradients")
        _same(_state(fused), pieces.state(), f"mini-batch at {g0}, parameters and optimizer state")
        got, ref = st[0].item(), pieces.stats[0].item()
        assert abs(got - ref) <= 1e-6 * abs(ref), (got, ref)
        assert st[1].item() == 0.0 and st[3].item() == 0.0  # no MAE on this branch
    assert fused.path == "batch_fused"
    assert int(pieces.err.item()) == 0


def test_classification_rejects_a_bad_target():
    """Test 7, second part.  A target of 3 in the second mini-batch rejects that mini-batch (state and stats are
    those of the first alone) and raises the class-target message at check_targets(); a clean call follows."""
    X, A, nb, y = _cls_inputs([0, 1, 2, 0, 3, 2])
    st = _step(_cls_model(33).cuda(), 4, classification=True, t_mean=None)
    with pytest.raises(RuntimeError, match="class target"):
        st.step(X, A, nb, y)  # HGNN_STRICT=1 reports here, after the call
        st.check_targets()
    first = _step(_cls_model(33).cuda(), 4, classification=True, t_mean=None)
    first.step(X[:4], A[:4], nb[:4], y[:4])
    first.check_targets()
    _same(_state(st), _state(first), "rejected mini-batch skipped")
    assert torch.equal(st.stats, first.stats)
    assert torch.equal(st.out[:4], first.out)
    assert st.step_count == 2 and first.step_count == 1


def test_epochs(tmp_path):
    """Test 8.  train_epoch with batch_size=4 and chunk=5 (rounded down to 4) over shape A as a list, a GraphPack and
    a DevicePack: the same returned values, parameters and states, bitwise those of one step over all six graphs."""
    import hgnn_amd.datagen as dg
    from hgnn_amd.dataset import GraphPack
    raw = dg.qm9_shape_dataset(6, seed=700)
    pack = GraphPack.write(str(tmp_path / "p"), raw)
    sets = {"list": [[x, a, t, None, None, None, None] for x, a, t in raw], "graph pack": pack,
            "device pack": pack.to_device(J=None)}
    whole = _step(_model("A", 73).cuda(), 4)
    s = whole.step(*_pad(_graphs("A"), 1)).tolist()
    for name, data in sets.items():
        st = _step(_model("A", 73).cuda(), 4)
        seen = []
        step = st.step
        st.step = lambda X, A, nb, y: (seen.append(X.shape[0]), step(X, A, nb, y))[1]
        res = st.train_epoch(data, 0, chunk=5)
        assert seen == [4, 2], (name, seen)
        assert res == (s[2], s[3]), (name, res, s)
        _same(_state(st), _state(whole), name)
        assert st.step_count == whole.step_count == 2
        assert st.path == "batch_fused"


def test_nothing_outside_the_documented_extents_is_written():
    """Test 9.  hgnn_ccn_small_train_batch called directly on shape A (six graphs, B = 4): `out` rows past G and 256
    guard bytes on both sides of a workspace of exactly workspace_bytes keep their NaN fill, and a workspace that
    was all NaN bits before the call (nothing in it is read before it is written, apart from the reject words, which
    the entry clears) gives the bits of CcnTrainStep's own call."""
    from hgnn_amd import _lib as L
    from hgnn_amd.ccn import _word
    from hgnn_amd.net import check_errors
    lib = L.lib()
    check_errors()
    X, A, nb, y = _pad(_graphs("A"), 1)
    G, B = X.shape[0], 4
    ref = _step(_model("A", 21).cuda(), B)
    ref.step(X, A, nb, y)
    net = _model("A", 21).cuda()
    ps = net._params()
    grads, m, u = ([torch.zeros_like(p) for p in ps] for _ in range(3))
    cfg = net._spec().config(G, X.shape[1])
    nbytes = lib.hgnn_ccn_small_train_batch_workspace_bytes(ctypes.byref(cfg), B)
    assert nbytes > 0 and nbytes % 256 == 0
    buf = torch.full(((nbytes + 512) // 4,), float("nan"), device="cuda")
    fill = buf.view(torch.int32).clone()
    ws = buf.data_ptr() + 256
    out = torch.full((G + 3, 1), float("nan"), device="cuda")
    stats = torch.zeros(4, device="cuda")
    steps = torch.tensor([(LR / (1.0 - 0.9 ** t), 0.0) for t in (1, 2)], dtype=torch.float32).cuda()
    err, tag = _word.next(X.device)
    L.check(lib.hgnn_ccn_small_train_batch(ctypes.byref(cfg), B, L.OPT_KIND["adamax"], 0, L.ptr(X), L.ptr(A),
                                           L.ptr(nb), L.ptr(y), MEAN, STD, L.ptr_array(ps), L.ptr_array(grads),
                                           L.ptr_array(m), L.ptr_array(u), L.ptr(steps), 0.9, 0.999, 1e-8, 0.0,
                                           L.ptr(stats), L.ptr(out), ctypes.c_void_p(ws), err, tag,
                                           L.stream_handle(X.device)), "hgnn_ccn_small_train_batch")
    torch.cuda.synchronize()
    check_errors()
    assert torch.isnan(out[G:]).all(), out
    assert torch.equal(out[:G], ref.out)
    after = buf.view(torch.int32)
    assert torch.equal(after[:64], fill[:64]), "guard bytes before the workspace"
    assert torch.equal(after[-64:], fill[-64:]), "guard bytes after the workspace"
    assert int(after[64:64 + 2].abs().sum()) == 0, "the two mini-batches' reject words"
    _same([p.detach() for p in ps] + m + u, _state(ref), "direct call against CcnTrainStep")
    assert torch.equal(stats, ref.stats)
    _same(grads, [p.grad for p in ref.params], "last mini-batch's gradients")
