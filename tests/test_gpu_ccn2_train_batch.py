"""The CCN-2D mini-batch kernels (hgnn_amd.train.CcnTrainStep(fused="ccn2_batch", batch_size=B),
hgnn_ccn2_small_train_batch) against the library's own pieces (bitwise) and the fp64 oracle.

A mini-batch is B consecutive graphs on the same weights (tests/test_gpu_ccn_train_batch.py's module docstring).  The
kernels run it in two dispatches: one workgroup per graph (plan, forward, the graph's dout row, backward without dX,
in the graph's own workspace region), then the sums over the mini-batch's packed nodes and graphs with the optimizer's
element update behind each.  Shapes P, Q, R, S and X, MEAN, STD, LR and the det_init seeds are those of
tests/test_gpu_ccn2_train.py; the pieces runner is tests/test_gpu_ccn_train_batch.py's.

Bitwise tests need no tolerance: the node functions are those of k_ccn2_small_fwd / k_ccn2_small_bwd, which
forward_batch and its backward run on these shapes, the sums run in k_ccn2_small_reduce's order, and the loss rows and
the optimizer elements are the shared functions of csrc/kernels.h.  The one exception is the running cross entropy
0.9 v + 0.1 r, which each kernel forms with its own instructions: within 2^-22 relative
(tests/test_gpu_ccn_xent.py).  Tolerances against the oracle are the project's (tests/test_gpu_ccn2_train.py)."""

import ctypes

import pytest
import torch

import ccn_batch_util as U
import test_gpu_ccn_train as T1
from test_gpu_ccn2_train import LR, MEAN, SHAPES, STD, _assert_supported, _graphs, _labels, _model, _pad, _same
from test_gpu_ccn_train_batch import _Pieces, _fused_against_pieces, _state

pytestmark = pytest.mark.gpu

assert (T1.MEAN, T1.STD, T1.LR) == (MEAN, STD, LR)  # _Pieces normalises and steps with the CCN-1D module's


def _step(net, B, fused="ccn2_batch", **kw):
    from hgnn_amd.train import CcnTrainStep
    kw.setdefault("t_mean", MEAN)
    kw.setdefault("t_std", STD)
    return CcnTrainStep(net, lr=LR, fused=fused, batch_size=B, **kw)


def _finite(st, what):
    assert torch.isfinite(st.out).all(), (what, st.out)
    assert all(torch.isfinite(p.grad).all() for p in st.params), what


@pytest.mark.parametrize("shape,optimizer,B", [("P", "adamax", 4), ("P", "sgd", 4), ("P", "adam", 4),
                                               ("Q", "adamax", 4), ("R", "adamax", 4), ("S", "adamax", 2)])
def test_fused_step_equals_the_librarys_pieces(shape, optimizer, B):
    """Test 1.  out, every p.grad, stats[0:2], both optimizer states and the parameters, bitwise, after every
    mini-batch.  P: mini-batches of 4 and 2; Q: f = 7, two outputs, three levels; R: hidden 1, one level; S: the
    32-clique at the nmax bound shares a mini-batch with a 14-node graph, then a one-graph mini-batch."""
    graphs = _graphs(shape)
    n_out = SHAPES[shape][0][1]
    X, A, nb, y = _pad(graphs, n_out)
    _assert_supported(shape, X.shape[1])
    fused = _step(_model(shape, 33).cuda(), B, optimizer=optimizer)
    pieces = _Pieces(_model(shape, 33).cuda(), optimizer)
    step = fused.step

    def checked(*a):  # every output and gradient is finite, before anything is compared
        st = step(*a)
        _finite(fused, shape)
        return st

    fused.step = checked
    _fused_against_pieces(fused, pieces, X, A, nb, y, B, f"{shape} {optimizer}")
    assert fused.path == "batch_fused2d"
    assert fused.step_count == -(-len(graphs) // B)


@pytest.mark.parametrize("shape,B", [("P", 4), ("S", 2)])
def test_k_minibatches_in_one_call_equal_k_calls(shape, B):
    """Test 2.  The workspace regions reused in stream order, one reject word and one d_steps row per mini-batch.  S:
    the second mini-batch's 22 packed rows and its graph region were written by the clique before, so a stale row
    shows here."""
    graphs = _graphs(shape)
    X, A, nb, y = _pad(graphs, 1)
    many = _step(_model(shape, 21).cuda(), B)
    many.step(X, A, nb, y)
    _finite(many, shape)
    one = _step(_model(shape, 21).cuda(), B)
    outs = []
    for g0 in range(0, len(graphs), B):
        one.step(X[g0:g0 + B], A[g0:g0 + B], nb[g0:g0 + B], y[g0:g0 + B])
        outs.append(one.out.clone())
    assert many.path == one.path == "batch_fused2d"
    _same(_state(many), _state(one), f"shape {shape}")
    assert torch.equal(many.out, torch.cat(outs))
    assert torch.equal(many.stats, one.stats), (many.stats, one.stats)
    assert many.step_count == one.step_count == -(-len(graphs) // B)
    _same([p.grad for p in many.params], [p.grad for p in one.params], "last mini-batch's gradients")
    moved = (many.params[0].detach() - _model(shape, 21).w1.weight.cuda()).abs().max().item()
    assert moved > 0.5 * LR * many.step_count, moved


def test_batch_size_one_equals_the_per_graph_fused_loop():
    """Test 3.  batch_size=1 against batch_size=None, fused="ccn2" on shape P: out, parameters, states, stats[0:2]."""
    from hgnn_amd.train import CcnTrainStep
    X, A, nb, y = _pad(_graphs("P"), 1)
    mini = _step(_model("P", 21).cuda(), 1)
    mini.step(X, A, nb, y)
    loop = CcnTrainStep(_model("P", 21).cuda(), lr=LR, t_mean=MEAN, t_std=STD, fused="ccn2")
    loop.step(X, A, nb, y)
    assert (mini.path, loop.path) == ("batch_fused2d", "fused2d")
    assert torch.equal(mini.out, loop.out)
    _same(_state(mini), _state(loop), "batch_size=1 against the per-graph loop")
    assert torch.equal(mini.stats[:2], loop.stats[:2]), (mini.stats, loop.stats)
    assert mini.step_count == loop.step_count == 6


@pytest.mark.parametrize("case", ["2D-b2", "2D-b5"])
def test_against_the_fp64_oracle(case):
    """Test 4.  One step call over the whole list against the fp64 oracle stepping per mini-batch: every out row and
    the meters within 1e-5 max(1, |ref|); parameters within 1e-5 max(1, |p|) where the oracle's gradient stayed
    above 1e-4 max|g| of its tensor at every step, else within 2 lr K, and that class at most 5 % of the elements
    (the oracle alone: 0 of 266, tests/test_ccn_train_batch_cpu.py)."""
    net, graphs, B, orc = U.run_oracle(case)
    st = _step(net.cuda(), B)
    st.step(*_pad(graphs, net.n_outputs))
    assert st.path == "batch_fused2d"
    orc.compare(st, f"{case} batch_fused2d")


def _slots():
    gp = _graphs("P")
    broken = gp[1][1].clone()
    broken[2, 2] = 0.0
    t = gp[0][2]
    return [(gp[0][0][:1], torch.ones(1, 1), t), (torch.zeros(0, 5), torch.zeros(0, 0), t), gp[0],
            (gp[1][0], broken, gp[1][2]), gp[2], gp[3]]


def test_ragged_and_rejected_graphs():
    """Test 5.  B = 2, three mini-batches: [a one-node graph, an empty slot], [a QM9-shape graph, a graph with one
    self loop removed], [a QM9-shape graph, n_b = nmax + 1].  Each rejected mini-batch leaves parameters, states and
    stats exactly as its predecessor left them; the valid graph's out row is written (what the weights of the first
    mini-batch give); the check raises; step_count counts all three."""
    from hgnn_amd.net import check_errors
    slots = _slots()
    nmax = max(g[0].shape[0] for g in slots)
    _assert_supported("P", nmax)
    check_errors()
    X, A, nb, y = _pad(slots, 1, nmax)
    nb = nb.clone()
    nb[5] = nmax + 1
    first = _step(_model("P", 61).cuda(), 2)
    first.step(X[:2], A[:2], nb[:2], y[:2])
    check_errors()
    with torch.no_grad():  # what graphs 2 and 4 saw: the weights the first mini-batch left
        seen = first.model.forward_batch(X[[2, 4]], A[[2, 4]], nb[[2, 4]])
    for k, message in ((2, "self loop"), (3, None)):
        full = _step(_model("P", 61).cuda(), 2)
        full.out = None
        with pytest.raises(RuntimeError, match=message):
            full.step(X[:2 * k], A[:2 * k], nb[:2 * k], y[:2 * k])  # HGNN_STRICT=1 reports here, after the call
            check_errors()
        check_errors()  # the word was consumed
        assert full.path == "batch_fused2d" and full.step_count == k
        _same(_state(full), _state(first), f"{k - 1} rejected mini-batches skipped")
        assert torch.equal(full.stats, first.stats), (full.stats, first.stats)
        assert torch.equal(full.out[:2], first.out)
        assert torch.equal(full.out[2], seen[0]), (full.out[2], seen[0])
        if k == 3:
            assert torch.equal(full.out[4], seen[1]), (full.out[4], seen[1])
        _same([p.grad for p in full.params], [p.grad for p in first.params], "the last applied gradients")
    # the empty slot's output is fc.bias as the mini-batch saw it
    assert torch.equal(full.out[1], _model("P", 61).fc.bias.cuda())


def test_the_empty_slots_minibatch_equals_the_pieces_route():
    """Test 5, last point: [one-node graph, empty slot] through the kernels and through fused=False."""
    slots = _slots()
    nmax = max(g[0].shape[0] for g in slots)
    X, A, nb, y = _pad(slots[:2], 1, nmax)
    a = _step(_model("P", 61).cuda(), 2)
    b = _step(_model("P", 61).cuda(), 2, fused=False)
    sa, sb = a.step(X, A, nb, y), b.step(X, A, nb, y)
    assert (a.path, b.path) == ("batch_fused2d", "batch")
    assert torch.equal(a.out, b.out)
    assert torch.equal(sa, sb), (sa, sb)
    _same(_state(a), _state(b), "empty slot's mini-batch")
    _same([p.grad for p in a.params], [p.grad for p in b.params], "gradients")
    assert a.params[-1].grad.abs().max().item() > 0


def test_classification_equals_the_pieces():
    """Test 6.  CCN_2D(5, 2, 2, 2) at scale 0.03 on X's graphs, labels g % 2, B = 4, against the pieces with
    hgnn_xent_loss: out, gradients, stats[0], states and parameters bitwise; the running loss within 2^-22 relative;
    stats[1] and stats[3] are never written."""
    graphs = _graphs("X")
    X, A, nb, y = _pad(graphs, 2, labels=_labels(len(graphs), 2))
    y = y.float()
    fused = _step(_model("X", 33).cuda(), 4, classification=True, t_mean=None)
    pieces = _Pieces(_model("X", 33).cuda(), cls=True)
    for g0 in (0, 4):
        sl = slice(g0, g0 + 4)
        st = fused.step(X[sl], A[sl], nb[sl], y[sl])
        out = pieces.step(X[sl], A[sl], nb[sl], y[sl])
        assert torch.equal(fused.out, out)
        _same([p.grad for p in fused.params], pieces.grads, f"mini-batch at {g0}, gradients")
        _same(_state(fused), pieces.state(), f"mini-batch at {g0}, parameters and optimizer state")
        print(f"mini-batch at {g0}: stats {st.tolist()} against {pieces.stats.tolist()}")
        assert torch.equal(st[0], pieces.stats[0]), (st, pieces.stats)
        got, ref = st[2].item(), pieces.stats[2].item()
        assert abs(got - ref) <= 2.0 ** -22 * abs(ref), (got, ref)
        assert st[0].item() > 0 and st[1].item() == 0.0 and st[3].item() == 0.0  # no MAE on this branch
    assert fused.path == "batch_fused2d"
    assert int(pieces.err.item()) == 0


def test_classification_rejects_a_bad_target():
    """Test 6, second part.  A target of 2 in the second mini-batch rejects that mini-batch alone (state and stats are
    those of the first) and raises the class-target message at the next check; a clean call follows."""
    graphs = _graphs("X")
    X, A, nb, _ = _pad(graphs, 2, labels=_labels(len(graphs), 2))
    y = torch.tensor([0, 1, 0, 1, 2, 1], dtype=torch.float32).cuda()
    st = _step(_model("X", 33).cuda(), 4, classification=True, t_mean=None)
    with pytest.raises(RuntimeError, match="class target"):
        st.step(X, A, nb, y)  # HGNN_STRICT=1 reports here, after the call
        st.check_targets()
    first = _step(_model("X", 33).cuda(), 4, classification=True, t_mean=None)
    first.step(X[:4], A[:4], nb[:4], y[:4])
    first.check_targets()
    _same(_state(st), _state(first), "rejected mini-batch skipped")
    assert torch.equal(st.stats, first.stats)
    assert torch.equal(st.out[:4], first.out)
    assert torch.isfinite(st.out[4:]).all()
    assert st.step_count == 2 and first.step_count == 1


def test_epochs(tmp_path):
    """Test 7.  train_epoch with batch_size=4 and chunk=5 (rounded down to 4) over shape P as a list, a GraphPack and
    a DevicePack: the same returned values, stats, parameters and states, bitwise those of one step over all six
    graphs."""
    import hgnn_amd.datagen as dg
    from hgnn_amd.dataset import GraphPack
    raw = dg.qm9_shape_dataset(6, seed=700)
    pack = GraphPack.write(str(tmp_path / "p"), raw)
    sets = {"list": [[x, a, t, None, None, None, None] for x, a, t in raw], "graph pack": pack,
            "device pack": pack.to_device(J=None)}
    whole = _step(_model("P", 73).cuda(), 4)
    s = whole.step(*_pad(_graphs("P"), 1)).tolist()
    for name, data in sets.items():
        st = _step(_model("P", 73).cuda(), 4)
        seen = []
        step = st.step
        st.step = lambda X, A, nb, y: (seen.append(X.shape[0]), step(X, A, nb, y))[1]
        res = st.train_epoch(data, 0, chunk=5)
        assert seen == [4, 2], (name, seen)
        assert res == (s[2], s[3]), (name, res, s)
        assert torch.equal(st.stats, whole.stats), (name, st.stats, whole.stats)
        _same(_state(st), _state(whole), name)
        assert st.step_count == whole.step_count == 2
        assert st.path == "batch_fused2d"
        assert list(st._ws_batch2d) == [22]  # both chunks are padded to 22 nodes: one workspace, kept


def test_nothing_outside_the_documented_extents_is_written():
    """Test 8.  hgnn_ccn2_small_train_batch called directly on shape P (six graphs, B = 4): `out` rows past G, a
    sentinel after `stats` and 256 guard bytes on both sides of a workspace of exactly workspace_bytes keep their NaN
    fill, every out row inside G is written, and a workspace that was all NaN bits before the call (nothing in it is
    read before it is written, apart from the reject words, which the entry clears) gives the bits of CcnTrainStep's
    own call."""
    from hgnn_amd import _lib as L
    from hgnn_amd.ccn import _word
    from hgnn_amd.net import check_errors
    lib = L.lib()
    check_errors()
    X, A, nb, y = _pad(_graphs("P"), 1)
    G, B = X.shape[0], 4
    ref = _step(_model("P", 21).cuda(), B)
    ref.step(X, A, nb, y)
    net = _model("P", 21).cuda()
    ps = net._params()
    grads, m, u = ([torch.zeros_like(p) for p in ps] for _ in range(3))
    cfg = net._spec().config(G, X.shape[1])
    nbytes = lib.hgnn_ccn2_small_train_batch_workspace_bytes(ctypes.byref(cfg), B)
    assert nbytes > 0 and nbytes % 256 == 0
    buf = torch.full(((nbytes + 512) // 4,), float("nan"), device="cuda")
    fill = buf.view(torch.int32).clone()
    ws = buf.data_ptr() + 256
    out = torch.full((G + 3, 1), float("nan"), device="cuda")
    stats = torch.zeros(8, device="cuda")
    stats[4:] = float("nan")
    steps = torch.tensor([(LR / (1.0 - 0.9 ** t), 0.0) for t in (1, 2)], dtype=torch.float32).cuda()
    err, tag = _word.next(X.device)
    L.check(lib.hgnn_ccn2_small_train_batch(ctypes.byref(cfg), B, L.OPT_KIND["adamax"], 0, L.ptr(X), L.ptr(A),
                                            L.ptr(nb), L.ptr(y), MEAN, STD, L.ptr_array(ps), L.ptr_array(grads),
                                            L.ptr_array(m), L.ptr_array(u), L.ptr(steps), 0.9, 0.999, 1e-8, 0.0,
                                            L.ptr(stats), L.ptr(out), ctypes.c_void_p(ws), err, tag,
                                            L.stream_handle(X.device)), "hgnn_ccn2_small_train_batch")
    torch.cuda.synchronize()
    check_errors()
    assert torch.isnan(out[G:]).all(), out
    assert torch.isfinite(out[:G]).all(), out
    assert torch.equal(out[:G], ref.out)
    assert torch.isnan(stats[4:]).all(), stats
    assert torch.equal(stats[:4], ref.stats)
    after = buf.view(torch.int32)
    assert torch.equal(after[:64], fill[:64]), "guard bytes before the workspace"
    assert torch.equal(after[-64:], fill[-64:]), "guard bytes after the workspace"
    assert int(after[64:64 + 2].abs().sum()) == 0, "the two mini-batches' reject words"
    _same([p.detach() for p in ps] + m + u, _state(ref), "direct call against CcnTrainStep")
    _same(grads, [p.grad for p in ref.params], "last mini-batch's gradients")


def test_routing():
    """Test 9.  On a CCN_2D model with batch_size: fused=None and False give "batch", "ccn2_batch" gives
    "batch_fused2d" and raises in step at nmax = 33; the default is off."""
    from hgnn_amd import train
    graphs = _graphs("P")
    X, A, nb, y = _pad(graphs, 1)
    for fused, path in ((None, "batch"), (False, "batch"), ("ccn2_batch", "batch_fused2d")):
        st = _step(_model("P", 73).cuda(), 4, fused=fused)
        st.step(X, A, nb, y)
        assert st.path == path, (fused, st.path)
    assert st._supported_batch(32, True) and not st._supported_batch(33, True) and not st._supported_batch(22)
    X33, A33, nb33, y33 = _pad(graphs, 1, nmax=33)
    with pytest.raises(RuntimeError, match="ccn2_batch"):
        _step(_model("P", 73).cuda(), 4).step(X33, A33, nb33, y33)
    assert train.CCN2_TRAIN_BATCH_FUSED_DEFAULT is False
