"""The spill instantiation of the CCN-1D small-graph kernels (csrc/ccn_small_spill.hip, csrc/ccn_small_batch_spill.hip;
forward_batch(small="spill"), CcnTrainStep(fused="ccn1_spill")): the row-sized arrays of a graph -- the L levels, dcoll,
dF0, dF1 -- live in a per-workgroup region of a global workspace instead of LDS, so the depth no longer bounds the graph
size.  The arithmetic and its order are the LDS kernels', so

  * where both exist the results are the same bits (shapes A-D of tests/test_gpu_ccn_train.py and a batch padded to
    64 nodes), whatever the padding;
  * on shapes only the spill kernels take (W27, W64, DA6 of tests/ccn_spill_util.py) outputs and dX are the general
    path's bits, the weight gradients are on test_ccn1_small_graph_path_at_its_bounds' gradient bound, and the
    training loops meet the fp64 oracle on _Oracle.compare's rule (tests/test_gpu_ccn_train.py's docstring).

Generators, MEAN, STD, LR, det_init seeds, targets t[:n_out] and the oracles are imported, not restated."""

import copy
import ctypes

import pytest
import torch

import ccn_edge_util as EU
import ccn_spill_util as U
import fixture_util as fu
from test_gpu_ccn_train import LR, MEAN, MODELS, STD, _graphs, _model, _pad, _same
from test_gpu_ccn_train_batch import _slots

pytestmark = pytest.mark.gpu


def _step(net, fused, B=None, **kw):
    from hgnn_amd.train import CcnTrainStep
    if not kw.get("classification"):
        kw.setdefault("t_mean", MEAN)
        kw.setdefault("t_std", STD)
    kw.setdefault("lr", LR)
    return CcnTrainStep(net, fused=fused, batch_size=B, **kw)


def _states(st):
    if st.optimizer == "sgd":
        return list(st.momentum_buffer)
    return list(st.exp_avg) + list(st.exp_avg_sq if st.optimizer == "adam" else st.exp_inf)


def _state(st):
    return [p.detach().clone() for p in st.params] + [t.clone() for t in _states(st)]


def _assert_same_step(a, b, what):
    assert all(bool(torch.isfinite(t).all()) for t in [a.out, *_state(a), *[p.grad for p in a.params]]), what
    assert torch.equal(a.out, b.out), f"{what}: out differs by {(a.out - b.out).abs().max().item():.3g}"
    assert torch.equal(a.stats, b.stats), (what, a.stats, b.stats)
    _same([p.grad for p in a.params], [p.grad for p in b.params], f"{what}: gradients")
    _same(_state(a), _state(b), f"{what}: parameters and optimizer state")
    assert a.step_count == b.step_count


# ------------------------------------------------------------------ 1. the LDS kernels' bits where both exist
def _k64_graphs():
    """Padded to 64 nodes: a clique (rows = nmax^2, 64 lanes per node), a star and a sparse graph."""
    gen = torch.Generator().manual_seed(64)
    return [(torch.randn(a.shape[0], 2, generator=gen), a, torch.randn(2, generator=gen))
            for a in (EU.clique(64), EU.star(64), EU.er(20, 0.2, 7))]


def _both_graphs(shape):
    if shape == "K64":
        return _k64_graphs()
    return _graphs("D") + _graphs("A") if shape == "DA" else _graphs(shape)


def _both_model(shape, seed, n_out=None):
    """The shape's model of tests/test_gpu_ccn_train.py (K64: CCN_1D(2, 2, 1, 2)); n_out overrides its outputs."""
    from models.compnets.model_ccn import CCN_1D
    f, o, h, layers = (2, 2, 1, 2) if shape == "K64" else MODELS["A" if shape == "DA" else shape]
    net = CCN_1D(f, n_out or o, h, layers)
    fu.det_init(net, seed)
    return net


MODES = {"adamax": dict(), "sgd": dict(optimizer="sgd"), "adam": dict(optimizer="adam"),
         "xent": dict(classification=True), "b4": dict(B=4), "b4-adam-xent": dict(B=4, optimizer="adam",
                                                                                 classification=True)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", ["A", "B", "C", "D", "DA", "K64"])
def test_spill_steps_are_the_lds_kernels_bits(shape, mode):
    """CcnTrainStep(fused="ccn1_spill") against fused=True from equal initial states, two step calls each (so the
    second starts from moments and a step count that are not trivial): out, stats, every p.grad, the parameters and
    every optimizer state.  DA at B = 4 ends in a one-graph mini-batch.  SGD has no normalisation and the 64-clique's
    gradients are of the order 1e8 (4096 rows a level), so on K64 it steps with lr = 1e-12 to stay finite; every
    compared value is checked to be finite, since NaN equals nothing."""
    kw = dict(MODES[mode])
    if shape == "K64" and kw.get("optimizer") == "sgd":
        kw["lr"] = 1e-12
    graphs = _both_graphs(shape)
    cls = kw.get("classification", False)
    net = _both_model(shape, 21, 2 if cls else None)
    X, A, nb, y = _pad(graphs, net.n_outputs)
    if cls:
        y = (torch.arange(len(graphs)) % 2).float().cuda()
    lds, spill = _step(copy.deepcopy(net).cuda(), True, **kw), _step(copy.deepcopy(net).cuda(), "ccn1_spill", **kw)
    for call in range(2):
        lds.step(X, A, nb, y)
        spill.step(X, A, nb, y)
        want = ("fused", "fused_spill") if "B" not in kw else ("batch_fused", "batch_fused_spill")
        assert (lds.path, spill.path) == want
        _assert_same_step(spill, lds, f"{shape} {mode} call {call}")
    assert lds.step_count == 2 * (len(graphs) if "B" not in kw else -(-len(graphs) // 4))


def _fwd_bwd(net, X, A, nb, w, small):
    net.zero_grad(set_to_none=True)
    Xr = X.clone().requires_grad_(True)
    out = net.forward_batch(Xr, A, nb, small=small)
    (out * w).sum().backward()
    return out.detach(), Xr.grad, [p.grad.detach().clone() for p in net._params()]


@pytest.mark.parametrize("shape", ["A", "B", "C", "D", "K64"])
def test_spill_forward_and_backward_are_the_lds_kernels_bits(shape):
    """forward_batch(small="spill") against the default small path on the whole batch and on its first graph alone
    (the one-graph backward writes its gradients directly): out, dX and every weight gradient."""
    graphs = _both_graphs(shape)
    net = _both_model(shape, 33).cuda()
    X, A, nb, _ = _pad(graphs, net.n_outputs)
    assert net._spec().small(X.shape[0], X.shape[1]) is not None
    w = torch.randn(X.shape[0], net.n_outputs, generator=torch.Generator().manual_seed(5)).cuda()
    for sl in (slice(None), slice(0, 1)):
        o1, dx1, g1 = _fwd_bwd(net, X[sl], A[sl], nb[sl], w[sl], None)
        o2, dx2, g2 = _fwd_bwd(net, X[sl], A[sl], nb[sl], w[sl], "spill")
        assert torch.equal(o1, o2) and torch.equal(dx1, dx2), shape
        _same(g2, g1, f"{shape} weight gradients")
    # n_batch = None: every graph has nmax nodes
    n = int(nb[0])
    X0, A0 = X[:1, :n].contiguous(), A[:1, :n, :n].contiguous()
    o1, dx1, g1 = _fwd_bwd(net, X0, A0, None, w[:1], None)
    o2, dx2, g2 = _fwd_bwd(net, X0, A0, None, w[:1], "spill")
    assert torch.equal(o1, o2) and torch.equal(dx1, dx2)
    _same(g2, g1, f"{shape} weight gradients, n_batch None")


# ------------------------------------------------------------------ 2. padding does not change the bits
@pytest.mark.parametrize("B", [None, 4])
def test_padding_does_not_change_the_bits(B):
    """The LDS route on DA padded to 40 and to 42 nodes (its bound for CCN_1D(5, 1, 2, 2)) ends in the same bits --
    the assumption -- and so does the spill route padded to 43, which the LDS kernels refuse."""
    graphs = _both_graphs("DA")
    runs = {}
    for name, fused, nmax in (("lds 40", True, 40), ("lds 42", True, 42), ("spill 43", "ccn1_spill", 43)):
        st = _step(_model("A", 21).cuda(), fused, B)
        st.step(*_pad(graphs, 1, nmax))
        runs[name] = st
    assert not runs["lds 40"]._supported(43)
    with pytest.raises(RuntimeError, match="fused=True"):
        _step(_model("A", 21).cuda(), True, B).step(*_pad(graphs, 1, 43))
    assert runs["spill 43"].path == ("fused_spill" if B is None else "batch_fused_spill")
    _assert_same_step(runs["lds 42"], runs["lds 40"], "LDS route, 42 against 40")
    _assert_same_step(runs["spill 43"], runs["lds 40"], "spill route at 43 against the LDS route at 40")


# ------------------------------------------------------------------ 3. spill-only shapes against the general path
def _grad_close(got, ref, what):
    """tests/test_gpu_ccn.py test_ccn1_small_graph_path_at_its_bounds' rule for weight gradients summed in another
    order (_grad_close there): 1e-4 of the tensor's largest gradient + 1e-5 |ref| + 1e-7."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    tol = 1e-4 * ref.abs().max().item() + 1e-5 * ref.abs() + 1e-7
    assert not ((got - ref).abs() > tol).any(), f"{what}: max err {(got - ref).abs().max().item():.3g}"


@pytest.mark.parametrize("case", list(U.CASES))
def test_spill_only_shapes_against_the_general_path(case):
    graphs = U.graphs(case)
    net = U.model(case).cuda()
    X, A, nb, _ = _pad(graphs, net.n_outputs)
    assert net._spec().small(X.shape[0], X.shape[1]) is None and net._spec().small(1, X.shape[1]) is None
    w = torch.randn(X.shape[0], net.n_outputs, generator=torch.Generator().manual_seed(9)).cuda()
    og, dxg, gg = _fwd_bwd(net, X, A, nb, w, None)
    os_, dxs, gs = _fwd_bwd(net, X, A, nb, w, "spill")
    assert torch.equal(os_, og), f"outputs differ: {(os_ - og).abs().max().item():.3g}"
    assert torch.equal(dxs, dxg), f"dX differs: {(dxs - dxg).abs().max().item():.3g}"
    assert all(dxs[b, n:].abs().max().item() == 0.0 for b, n in enumerate(nb.tolist()) if n < X.shape[1])
    for i, (a, b) in enumerate(zip(gs, gg)):
        _grad_close(a, b, f"{case}: spill against general, parameter {i}")


# ------------------------------------------------------------------ 4. loop structure
def test_k_graphs_in_one_dispatch_equal_k_dispatches():
    X, A, nb, y = _pad(U.graphs("W27"), 2)
    many = _step(U.model("W27").cuda(), "ccn1_spill")
    many.step(X, A, nb, y)
    one = _step(U.model("W27").cuda(), "ccn1_spill")
    outs = []
    for g in range(X.shape[0]):
        one.step(X[g:g + 1], A[g:g + 1], nb[g:g + 1], y[g:g + 1])
        outs.append(one.out.clone())
    one.out = torch.cat(outs)
    _assert_same_step(many, one, "one dispatch against one per graph")
    moved = (many.params[0].detach() - U.model("W27").w1.weight.cuda()).abs().max().item()
    assert moved > 0.5 * LR * X.shape[0], moved


def test_k_minibatches_in_one_call_equal_k_calls():
    X, A, nb, y = _pad(U.graphs("W27"), 2)
    many = _step(U.model("W27").cuda(), "ccn1_spill", 2)
    many.step(X, A, nb, y)
    one = _step(U.model("W27").cuda(), "ccn1_spill", 2)
    outs = []
    for g in range(0, X.shape[0], 2):
        one.step(X[g:g + 2], A[g:g + 2], nb[g:g + 2], y[g:g + 2])
        outs.append(one.out.clone())
    one.out = torch.cat(outs)
    _assert_same_step(many, one, "one call against one per mini-batch")
    assert many.step_count == 3


def test_batch_size_one_is_the_per_graph_loop():
    X, A, nb, y = _pad(U.graphs("W27"), 2)
    loop = _step(U.model("W27").cuda(), "ccn1_spill")
    b1 = _step(U.model("W27").cuda(), "ccn1_spill", 1)
    loop.step(X, A, nb, y)
    b1.step(X, A, nb, y)
    assert (loop.path, b1.path) == ("fused_spill", "batch_fused_spill")
    _assert_same_step(b1, loop, "batch_size=1 against the loop")


# ------------------------------------------------------------------ 5. the fp64 oracle on spill-only shapes
@pytest.mark.parametrize("case,B", list(U.LOOSE), ids=str)
def test_spill_training_against_the_fp64_oracle(case, B):
    orc = U.run_oracle(case, B)
    net = U.model(case)
    st = _step(net.cuda(), "ccn1_spill", B)
    st.step(*_pad(U.graphs(case), net.n_outputs))
    assert st.path == ("fused_spill" if B is None else "batch_fused_spill")
    orc.compare(st, f"{case}, B = {B}")


# ------------------------------------------------------------------ 6. rejection and ragged slots
def test_a_rejected_minibatch_takes_no_step():
    """tests/test_gpu_ccn_train_batch.py's slots (a one-node graph, an empty slot | a graph, a graph with a self loop
    removed | a graph; B = 2) padded to 43 nodes: the middle mini-batch takes no step, its other graph's out row is
    written, the error surfaces at the next check and a following clean call raises nothing."""
    from hgnn_amd.net import check_errors
    X, A, nb, y = _pad(_slots(), 1, 43)
    check_errors()
    full = _step(_model("A", 61).cuda(), "ccn1_spill", 2)
    with pytest.raises(RuntimeError, match="self loop"):
        full.step(X, A, nb, y)  # HGNN_STRICT=1 (the suite's setting) reports here, after the call
        check_errors()
    assert full.step_count == 3
    clean = _step(_model("A", 61).cuda(), "ccn1_spill", 2)
    clean.step(X[:2], A[:2], nb[:2], y[:2])
    out01 = clean.out.clone()
    with torch.no_grad():  # what graph 2 saw: the weights the first mini-batch left
        out2 = clean.model.forward_batch(X[2:3], A[2:3], nb[2:3], small="spill")
    clean.step_count += 1  # the rejected mini-batch's number
    clean.step(X[4:], A[4:], nb[4:], y[4:])
    check_errors()
    _same(_state(full), _state(clean), "rejected mini-batch skipped")
    assert torch.equal(full.stats, clean.stats), (full.stats, clean.stats)
    assert torch.equal(full.out[[0, 1, 4]], torch.cat([out01, clean.out]))
    assert torch.equal(full.out[2], out2[0]), (full.out[2], out2)
    assert torch.equal(full.out[1], _model("A", 61).fc.bias.cuda())  # the empty slot: fc.bias as its mini-batch saw it


def test_a_rejected_graph_takes_no_step_in_the_loop():
    """The same slots through the per-graph loop: the graph with a removed self loop takes no step and updates no
    meter; the final state is bitwise that of the list without it."""
    from hgnn_amd.net import check_errors
    slots = _slots()
    check_errors()
    full = _step(_model("A", 61).cuda(), "ccn1_spill")
    with pytest.raises(RuntimeError, match="self loop"):
        full.step(*_pad(slots, 1, 43))
        check_errors()
    clean = _step(_model("A", 61).cuda(), "ccn1_spill")
    clean.step(*_pad(slots[:3] + slots[4:], 1, 43))
    check_errors()
    _same(_state(full), _state(clean), "rejected slot skipped")
    assert torch.equal(full.stats, clean.stats)
    assert torch.equal(full.out[[0, 1, 2, 4]], clean.out)
    _same([p.grad for p in full.params], [p.grad for p in clean.params], "last graph's gradients")


# ------------------------------------------------------------------ 7. workspace bounds
GUARD = 4096


class _Carved:
    """A workspace of exactly `nbytes` at a 256-byte aligned base inside a larger buffer whose every byte is 0xFF
    (as floats: NaN), with at least GUARD bytes on either side."""

    def __init__(self, nbytes):
        self.buf = torch.full((nbytes + 2 * GUARD + 256,), 0xFF, dtype=torch.uint8, device="cuda")
        self.lo = GUARD + (-(self.buf.data_ptr() + GUARD)) % 256
        self.hi = self.lo + nbytes
        self.ws = self.buf[self.lo:self.hi]
        assert self.ws.data_ptr() % 256 == 0 and self.ws.numel() == nbytes

    def guards_intact(self):
        return bool((self.buf[:self.lo] == 0xFF).all()) and bool((self.buf[self.hi:] == 0xFF).all())


def test_nothing_outside_the_queried_workspace_is_written():
    """Forward, backward, the training loop and a mini-batch call on W64 (graphs of 64, 33 and 7 nodes: full and
    nearly empty regions) with workspaces of exactly the queried size: the guards on both sides keep their fill, and
    the results are those of a fresh workspace -- nothing depends on what a region held before."""
    from hgnn_amd import _lib as L
    from hgnn_amd.ccn import _CcnSpillFn
    graphs = U.graphs("W64")
    net = U.model("W64").cuda()
    X, A, nb, y = _pad(graphs, 2)
    bs, nmax = X.shape[0], X.shape[1]
    spec = net._spec()
    cfg, nbytes = spec.spill(bs, nmax)
    w = torch.randn(bs, 2, generator=torch.Generator().manual_seed(9)).cuda()
    want = _fwd_bwd(net, X, A, nb, w, "spill")
    one = _Carved(nbytes)
    net.zero_grad(set_to_none=True)
    Xr = X.clone().requires_grad_(True)
    out = _CcnSpillFn.apply(spec, (cfg, nbytes, one.ws), Xr, A, nb, *net._params())
    torch.cuda.synchronize()
    assert one.guards_intact(), "forward"
    (out * w).sum().backward()
    torch.cuda.synchronize()
    assert one.guards_intact(), "backward"
    assert torch.equal(out.detach(), want[0]) and torch.equal(Xr.grad, want[1])
    _same([p.grad for p in net._params()], want[2], "carved workspace: weight gradients")
    for B in (None, 2):
        regions = 1 if B is None else B
        c1 = spec.config(1, nmax)
        carved = _Carved(L.lib().hgnn_ccn_small_spill_workspace_bytes(ctypes.byref(c1), regions))
        a, b = _step(U.model("W64").cuda(), "ccn1_spill", B), _step(U.model("W64").cuda(), "ccn1_spill", B)
        a._ws_spill[(nmax, regions)] = carved.ws
        a.step(X, A, nb, y)
        b.step(X, A, nb, y)
        torch.cuda.synchronize()
        assert carved.guards_intact(), f"training, B = {B}"
        assert b._ws_spill[(nmax, regions)].numel() == carved.ws.numel()
        _assert_same_step(a, b, f"carved workspace, B = {B}")


# ------------------------------------------------------------------ 8. routing
def test_routing():
    from hgnn_amd.train import CcnTrainStep
    from models.compnets.model_ccn import CCN_1D, CCN_2D
    X, A, nb, y = _pad(U.graphs("W27"), 2)
    for B, default, spill in ((None, "unfused", "fused_spill"), (2, "batch", "batch_fused_spill")):
        st = _step(U.model("W27").cuda(), None, B)  # unchanged: the chunk is outside the LDS kernels' bound
        st.step(X, A, nb, y)
        assert st.path == default
        sp = _step(U.model("W27").cuda(), "ccn1_spill", B)
        sp.step(X, A, nb, y)
        assert sp.path == spill
        # the two routes run the same arithmetic but for the weight gradients' summation order
        assert torch.equal(sp.out[:1 if B is None else 2], st.out[:1 if B is None else 2])
        with pytest.raises(RuntimeError, match="hgnn_ccn_small_spill_train_supported"):
            _step(fu_model(CCN_2D, (5, 1, 2, 2)), "ccn1_spill", B)
        with pytest.raises(RuntimeError, match="hgnn_ccn_small_spill_train_supported"):
            _step(fu_model(CCN_1D, (9, 1, 2, 2)), "ccn1_spill", B)
        wide = _step(_model("A", 3).cuda(), "ccn1_spill", B)
        with pytest.raises(RuntimeError, match="hgnn_ccn_small_spill_train_supported"):
            wide.step(*_pad(_graphs("A"), 1, 65))
        wide.step(*_pad(_graphs("A"), 1, 64))
        assert wide.path == spill
    with pytest.raises(RuntimeError, match="ccn1_spill"):
        CcnTrainStep(_model("A", 3).cuda(), t_mean=MEAN, t_std=STD, fused="ccn1_spil")
    with pytest.raises(RuntimeError, match="hgnn_ccn_small_spill_supported"):
        _model("A", 3).cuda().forward_batch(*_pad(_graphs("A"), 1, 65)[:3], small="spill")
    with pytest.raises(RuntimeError, match="small="):
        _model("A", 3).cuda().forward_batch(*_pad(_graphs("A"), 1)[:3], small="lds")


def fu_model(cls, args):
    net = cls(*args)
    fu.det_init(net, 3)
    return net.cuda()


@pytest.mark.parametrize("B", [None, 4])
def test_epochs_from_a_list_and_from_packs(tmp_path, B):
    """train_epoch and eval_epoch on DA6 from the reference's list, a GraphPack and a DevicePack, chunk 5 (mini-batch
    mode: rounded down to 4): the same returned values, parameters and states from all three -- bitwise those of
    steps over the same chunks -- and evaluation (forward_batch(small="spill")) equal to the default route's, whose
    outputs are the same bits."""
    import hgnn_amd.datagen as dg
    from hgnn_amd.dataset import GraphPack
    qm9 = dg.qm9_shape_dataset(6, seed=700)
    raw = dg.sbm_dataset(1, n=40, seed=3, p_in=0.6) + qm9[:2] + qm9  # shapes D + A without their self loops
    graphs = U.graphs("DA6")
    assert all(torch.equal(a + torch.eye(a.shape[0]), g[1]) for (_, a, _), g in zip(raw, graphs))
    pack = GraphPack.write(str(tmp_path / "p"), raw)
    legs = {"list": [[x, a, t, None, None, None, None] for x, a, t in raw], "graph pack": pack,
            "device pack": pack.to_device(J=None)}
    chunk = 5 if B is None else 4
    whole = _step(U.model("DA6").cuda(), "ccn1_spill", B)
    whole.reset_running()
    for g0 in range(0, len(graphs), chunk):
        s = whole.step(*_pad(graphs[g0:g0 + chunk], 1)).tolist()
    ev_default = _step(copy.deepcopy(whole.model), None, B).eval_epoch(legs["list"], 0, chunk=5)
    for name, data in legs.items():
        st = _step(U.model("DA6").cuda(), "ccn1_spill", B)
        res = st.train_epoch(data, 0, chunk=5)
        assert st.path == ("fused_spill" if B is None else "batch_fused_spill")
        assert res == (s[2], s[3]), (name, res, s)
        _same(_state(st), _state(whole), name)
        assert st.step_count == whole.step_count
        assert st.eval_epoch(data, 0, chunk=5) == ev_default, name
