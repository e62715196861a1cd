"""The CCN training loops with SGD-momentum and Adam (CcnTrainStep(optimizer=...), hgnn_ccn_small_train_opt,
hgnn_ccn2_small_train_opt) against the library's own pieces (bitwise) and the fp64 oracle with torch's optimizer.

Cases (graphs, models, padding and labels are those of the existing test modules, imported):
  1d-mse   CCN_1D(5, 1, 2, 2), shape A of tests/test_gpu_ccn_train.py: qm9_shape_dataset(6, seed=700), 13-22 nodes
  1d-xent  CCN_1D(5, 2, 2, 2), shape A of tests/test_gpu_ccn_xent.py: the same graphs, label g % 2
  2d-mse   CCN_2D(5, 2, 2, 2), shape X of tests/test_gpu_ccn2_train.py (its smallest graphs, 6-8 nodes, and the one
  2d-xent  small shape that has two outputs, which cross entropy needs), regression targets t[:2] / label g % 2

Bitwise tests need no tolerance: the fused kernels and hgnn_optim_step inline one element function per optimizer
(sgd_elem / adam_elem, csrc/kernels.h), and both sides take their per-step scalars from the same double
arithmetic.  The running cross entropy is the one exception, as in tests/test_gpu_ccn_xent.py (within 2^-22).

Against the oracle (shape A, six steps, no re-synchronisation):
  adam  the rule of tests/test_gpu_ccn_train.py unchanged (its _Oracle.compare): 1e-5 max(1, |p|) where the
        oracle's gradient was above the noise floor at every step or exactly 0, else 2 lr K, the second class at
        most 5 % of the elements.  With torch.optim.Adam the oracle alone puts none of the 42 elements into the
        second class on these graphs at seed 47 (nor at 48 or 49; run on the CPU).
  sgd   the step is proportional to the gradient, so there is no noise class: every element within
        lr K (1e-4 max|g| + 1e-5 |g|) / (1 - mu) + 1e-5 max(1, |p|), with max|g| per tensor and |g| per element,
        both the largest over the K steps (the gradient bound of the forward / backward tests, through K steps of
        a momentum sum that weighs a gradient by at most 1 / (1 - mu)).
"""

import ctypes

import pytest
import torch

import test_gpu_ccn2_train as T2
import test_gpu_ccn_train as T1
import test_gpu_ccn_xent as TX

pytestmark = pytest.mark.gpu

MEAN, STD, LR, MU = T1.MEAN, T1.STD, T1.LR, 0.9
KIND = {"adamax": 0, "sgd": 1, "adam": 2}
CASES = ["1d-mse", "1d-xent", "2d-mse", "2d-xent"]
OPTS = ["sgd", "adam"]
_batches = {}


def _case(case):
    """(model factory by seed, the padded batch -- built once and shared, never modified --, xent, fused flag)."""
    xent = case.endswith("xent")
    if case not in _batches:
        if case == "1d-mse":
            _batches[case] = T1._pad(T1._graphs("A"), 1)
        elif case == "1d-xent":
            _batches[case] = TX._pad(TX._graphs("A"), TX._labels(6, 2))
        else:
            _batches[case] = T2._batch("X", xent)
    make = {"1d-mse": lambda s: T1._model("A", s), "1d-xent": lambda s: TX._model("A", s),
            "2d-mse": lambda s: T2._model("X", s), "2d-xent": lambda s: T2._model("X", s)}[case]
    return make, _batches[case], xent, ("ccn2" if case.startswith("2d") else True)


def _step(net, opt, xent, fused, **kw):
    from hgnn_amd.train import CcnTrainStep
    stats = dict(classification=True) if xent else dict(t_mean=MEAN, t_std=STD)
    return CcnTrainStep(net, lr=LR, fused=fused, optimizer=opt, momentum=MU, **stats, **kw)


def _states(st):
    if st.optimizer == "sgd":
        return list(st.momentum_buffer)
    return list(st.exp_avg) + list(st.exp_avg_sq)


def _state(st):
    return [p.detach().clone() for p in st.params] + [t.clone() for t in _states(st)]


_same = T1._same


def test_state_attributes_follow_the_optimizer():
    make, _, _, fused = _case("1d-mse")
    sgd = _step(make(1).cuda(), "sgd", False, fused)
    assert hasattr(sgd, "momentum_buffer") and not hasattr(sgd, "exp_avg") and not hasattr(sgd, "exp_inf")
    adam = _step(make(1).cuda(), "adam", False, fused)
    assert hasattr(adam, "exp_avg") and hasattr(adam, "exp_avg_sq") and not hasattr(adam, "exp_inf")
    amax = _step(make(1).cuda(), "adamax", False, fused)
    assert hasattr(amax, "exp_avg") and hasattr(amax, "exp_inf") and not hasattr(amax, "exp_avg_sq")
    from hgnn_amd.train import CcnTrainStep
    with pytest.raises(RuntimeError, match="rmsprop"):
        CcnTrainStep(make(1).cuda(), t_mean=MEAN, t_std=STD, optimizer="rmsprop")


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("case", CASES)
def test_one_fused_step_equals_the_librarys_own_pieces(case, opt):
    """Graph by graph, from the state the previous graphs left: the fused step on the one-graph slice against
    forward_batch, the loss kernel, backward and hgnn_optim_step.  Bitwise: out, every p.grad, both states, the
    parameters and the loss and MAE of stats (the running averages within 2^-22, see the module docstring)."""
    from hgnn_amd import _lib as L
    lib = L.lib()
    make, (X, A, nb, y), xent, flag = _case(case)
    yf = y.float()
    fused = _step(make(33).cuda(), opt, xent, flag)
    net = make(33).cuda()
    n_out = net.n_outputs
    ps = net._params()
    s1 = [torch.zeros_like(p) for p in ps]
    s2 = [torch.zeros_like(p) for p in ps]
    numel = (ctypes.c_int64 * len(ps))(*[p.numel() for p in ps])
    stats = torch.zeros(4, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = L.stream_handle(X.device)
    start = [p.detach().clone() for p in ps]
    for g in range(X.shape[0]):
        st = fused.step(X[g:g + 1], A[g:g + 1], nb[g:g + 1], y[g:g + 1])
        assert fused.path == ("fused2d" if flag == "ccn2" else "fused")
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
        L.check(lib.hgnn_optim_step(KIND[opt], len(ps), L.ptr_array(ps), L.ptr_array(grads), L.ptr_array(s1),
                                    None if opt == "sgd" else L.ptr_array(s2), numel, LR, MU if opt == "sgd" else 0.9,
                                    0.999, 1e-8, 0.0, g + 1, stream), "optim")
        assert torch.equal(fused.out, out.detach()), (g, fused.out, out)
        if xent:
            assert torch.equal(st[0], stats[0]), (g, st.tolist(), stats.tolist())
            assert st[1].item() == 0 and st[3].item() == 0, st
            assert abs(st[2].item() - stats[2].item()) <= 2.0 ** -22 * stats[2].item(), (g, st.tolist(),
                                                                                         stats.tolist())
        else:
            assert torch.equal(st[:2], stats[:2]), (g, st, stats)
            for k in (2, 3):  # the running averages: each kernel's own instructions, as for the cross entropy
                assert abs(st[k].item() - stats[k].item()) <= 2.0 ** -22 * stats[k].item(), (g, st, stats)
        _same([p.grad for p in fused.params], grads, f"graph {g} gradients")
        _same(_states(fused), s1 if opt == "sgd" else s1 + s2, f"graph {g} optimizer state")
        _same([p.detach() for p in fused.params], [p.detach() for p in ps], f"graph {g} parameters")
    assert int(err.item()) == 0
    assert all(not t.any() for t in s2) or opt == "adam"
    assert any(not torch.equal(a, b.detach()) for a, b in zip(start, ps))  # the steps were taken


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("case", CASES)
def test_k_steps_in_one_dispatch_equal_k_one_graph_dispatches(case, opt):
    """step on all graphs at once against step called per graph (both the fused kernel); the multi-graph call runs
    first.  Parameters, optimizer state, out, stats, step_count and the last graph's gradients are bitwise equal:
    the per-step scalars of the dispatch are those of the single steps, and each graph read the weights the one
    before it wrote."""
    make, (X, A, nb, y), xent, flag = _case(case)
    many = _step(make(21).cuda(), opt, xent, flag)
    many.step(X, A, nb, y)
    one = _step(make(21).cuda(), opt, xent, flag)
    outs = []
    for g in range(X.shape[0]):
        one.step(X[g:g + 1], A[g:g + 1], nb[g:g + 1], y[g:g + 1])
        outs.append(one.out.clone())
    assert torch.equal(many.out, torch.cat(outs)), (many.out, torch.cat(outs))
    _same(_state(many), _state(one), case)
    assert torch.equal(many.stats, one.stats), (many.stats, one.stats)
    assert many.step_count == one.step_count == X.shape[0]
    _same([p.grad for p in many.params], [p.grad for p in one.params], "last graph's gradients")
    moved = (many.params[0].detach() - make(21).w1.weight.cuda()).abs().max().item()
    assert moved > 0, moved
    if opt == "adam" and not xent:  # Adam's first steps are ~lr each
        assert moved > 0.5 * LR * X.shape[0], moved


def test_a_rejected_graph_in_the_middle_consumes_no_step_scalars():
    """Adam on shape A with the self loop of node 2 of graph 2 of 6 removed: the error word reports it, and the
    other five graphs end bitwise equal to a run on those five alone -- their per-step scalars (lr / (1 - b1^t),
    sqrt(1 - b2^t)) were those of steps 1 .. 5, indexed by applied step and not by graph."""
    from hgnn_amd.net import check_errors
    graphs = T1._graphs("A")
    broken = graphs[2][1].clone()
    broken[2, 2] = 0.0
    slots = graphs[:2] + [(graphs[2][0], broken, graphs[2][2])] + graphs[3:]
    nmax = max(g[0].shape[0] for g in slots)
    check_errors()
    full = _step(T1._model("A", 61).cuda(), "adam", False, True)
    with pytest.raises(RuntimeError, match="self loop"):
        full.step(*T1._pad(slots, 1, nmax))  # HGNN_STRICT=1 (the suite's setting) reports here, after the call
        check_errors()
    clean = _step(T1._model("A", 61).cuda(), "adam", False, True)
    clean.step(*T1._pad(slots[:2] + slots[3:], 1, nmax))
    check_errors()
    _same(_state(full), _state(clean), "rejected graph skipped")
    assert torch.equal(full.stats, clean.stats)
    assert torch.equal(full.out[[0, 1, 3, 4, 5]], clean.out)
    _same([p.grad for p in full.params], [p.grad for p in clean.params], "last graph's gradients")
    # the scalars do differ from step to step, so an index by graph would have shown: graphs 3 .. 5 on the rows of
    # steps 4 .. 6 end elsewhere
    shifted = _step(T1._model("A", 61).cuda(), "adam", False, True)
    X, A, nb, y = T1._pad(slots[:2] + slots[3:], 1, nmax)
    shifted.step(X[:2], A[:2], nb[:2], y[:2])
    shifted.step_count += 1
    shifted.step(X[2:], A[2:], nb[2:], y[2:])
    assert not torch.equal(shifted.params[0].detach(), clean.params[0].detach())


class _Oracle(T1._Oracle):
    """T1._Oracle with torch.optim.Adam or torch.optim.SGD(momentum) on the fp64 parameters; it also keeps, per
    tensor, the largest max|g| and per element the largest |g| over the steps (the SGD bound)."""

    def __init__(self, net, opt):
        super().__init__(net, 1)
        ps = [self.p[n] for n in self.names]
        self.opt = torch.optim.Adam(ps, lr=LR) if opt == "adam" else torch.optim.SGD(ps, lr=LR, momentum=MU)
        self.gmax = {n: 0.0 for n in self.names}
        self.gabs = {n: torch.zeros_like(self.p[n]) for n in self.names}

    def step(self, x, a, y):
        super().step(x, a, y)
        for n in self.names:  # the gradients of this step: opt.step() leaves them
            g = self.p[n].grad.abs()
            self.gmax[n] = max(self.gmax[n], g.max().item())
            self.gabs[n] = torch.maximum(self.gabs[n], g)

    def compare_sgd(self, st, what):
        outs = torch.stack(self.outs)
        err = (st.out.double().cpu() - outs).abs()
        assert (err <= 1e-5 * outs.abs().clamp(min=1.0)).all(), f"{what}: out differs by {err.max().item():.3g}"
        got = st.stats.double().cpu().tolist()
        for v, r in zip(got, [self.loss, self.mae, *self.run]):
            assert abs(v - r) <= 1e-5 * max(1.0, abs(r)), (what, got, self.loss, self.mae, self.run)
        moved = False
        for n, p in self.model_params(st):
            q = self.p[n].detach()
            e = (p.detach().double().cpu() - q).abs()
            bound = LR * self.steps * (1e-4 * self.gmax[n] + 1e-5 * self.gabs[n]) / (1.0 - MU) \
                + 1e-5 * q.abs().clamp(min=1.0)
            print(f"{what} {n}: worst error / bound = {(e / bound).max().item():.3g}")
            assert (e <= bound).all(), (what, n, (e / bound).max().item())
            moved |= self.gmax[n] > 0
        assert moved and st.step_count == self.steps


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("opt", OPTS)
def test_loop_against_the_fp64_oracle_with_torchs_optimizer(opt, fused):
    """Six sequential steps on shape A in one step call against the fp64 oracle stepping per graph with
    torch.optim.Adam / torch.optim.SGD(momentum=0.9): every out[g], the final stats and every parameter element
    (the rules in the module docstring)."""
    graphs = T1._graphs("A")
    net = T1._model("A", 47)
    orc = _Oracle(net, opt)
    for x, a, t in graphs:
        orc.step(x, a, t[:1])
    st = _step(net.cuda(), opt, False, fused)
    st.step(*_case("1d-mse")[1])
    assert st.path == ("fused" if fused else "unfused")
    if opt == "adam":
        orc.compare(st, f"adam {st.path}")
    else:
        orc.compare_sgd(st, f"sgd {st.path}")


@pytest.mark.parametrize("opt", OPTS)
def test_default_routing_follows_the_measured_table(opt):
    """fused=None takes the kernel the table names (hgnn_amd.train.CCN_TRAIN_FUSED_OPTIM), and the explicit flags
    keep their meaning."""
    from hgnn_amd.train import CCN_TRAIN_FUSED_OPTIM
    for case, order, path in (("1d-mse", 1, "fused"), ("2d-mse", 2, "fused2d")):
        make, (X, A, nb, y), xent, flag = _case(case)
        st = _step(make(5).cuda(), opt, xent, None)
        st.step(X[:1], A[:1], nb[:1], y[:1])
        assert st.path == (path if CCN_TRAIN_FUSED_OPTIM[(order, opt)] else "unfused")
        st = _step(make(5).cuda(), opt, xent, False)
        st.step(X[:1], A[:1], nb[:1], y[:1])
        assert st.path == "unfused"
