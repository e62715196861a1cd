"""The optimizer kernels (hgnn_optim_step: SGD with momentum, Adam, Adamax) against torch.optim on fixed
gradients, and TrainStep(optimizer=...) against torch's loop.

Kernel against torch.  Both sides take the same fp32 gradients for five steps.  After step t, per element, with q
torch's value and q_prev its value before the step,

    |p - q| <= t (2^-23 |q| + 1e-5 |q - q_prev|)

-- one rounding of the result per step, plus the project's 1e-5 relative bound applied to the step itself; the
optimizer states are held to the same form.  Bitwise agreement with torch is not asked: its foreach and
single-tensor paths differ from each other.  kind = HGNN_OPT_ADAMAX equals hgnn_adamax_step bitwise.

TrainStep.  The rule of tests/test_gpu_train.py: from equal states, parameters within 1e-5 max(1, max|p|) after
the step.  For adam (as for Adamax there) an element whose reference gradient is below the noise floor
(1e-4 max|g|) has no defined sign and moves by an lr-sized step on both sides: only |d| <= 2 lr holds for those.
SGD's step is proportional to the gradient, so it has no such class: every element is on the tight bound.
"""

import copy
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

ADAMAX, SGD, ADAM = 0, 1, 2
LR = 3e-4
# the tensor shapes of test_adamax_kernel_matches_torch_exactly_on_fixed_grads, and 67 tensors of 1 .. 67 elements:
# more than the 64 entries of one launch's table
SHAPES = {"five": [(64, 271, 1), (64,), (), (1, 640, 1), (5000,)], "sixty-seven": [(n,) for n in range(1, 68)]}


def _close(got, ref, prev, t, what):
    bound = t * (2.0 ** -23 * ref.abs().double() + 1e-5 * (ref.double() - prev.double()).abs())
    err = (got.double() - ref.double()).abs()
    over = err > bound
    assert not over.any(), f"{what}: {int(over.sum())} elements over the bound, worst {err[over].max().item():.3g}"


def _run(kind, shapes, make_opt, state_names, wd, b1, steps=5):
    """hgnn_optim_step against make_opt(params) on the same gradients; state_names: torch's state keys in the
    order (state1, state2)."""
    from hgnn_amd import _lib as L
    gen = torch.Generator(device="cpu").manual_seed(3)
    ps = [torch.randn(s, generator=gen).cuda() for s in shapes]
    qs = [p.clone().requires_grad_(True) for p in ps]
    opt = make_opt(qs)
    s1 = [torch.zeros_like(p) for p in ps]
    s2 = [torch.zeros_like(p) for p in ps]
    numel = (ctypes.c_int64 * len(ps))(*[p.numel() for p in ps])
    prev_state = {n: [torch.zeros_like(p) for p in ps] for n in state_names}
    for t in range(1, steps + 1):
        grads = [torch.randn(s, generator=gen).cuda() for s in shapes]
        q_prev = [q.detach().clone() for q in qs]
        for q, gr in zip(qs, grads):
            q.grad = gr.clone()
        opt.step()
        L.check(L.lib().hgnn_optim_step(kind, len(ps), L.ptr_array(ps), L.ptr_array(grads), L.ptr_array(s1),
                                        None if kind == SGD else L.ptr_array(s2), numel, LR, b1, 0.999, 1e-8, wd,
                                        t, L.stream_handle(ps[0].device)), "optim step")
        for i, (p, q) in enumerate(zip(ps, qs)):
            _close(p, q.detach(), q_prev[i], t, f"step {t} tensor {i} parameter")
            for n, mine in zip(state_names, (s1, s2)):
                ref = opt.state[q].get(n)
                if ref is None:  # torch keeps no buffer at momentum 0: ours then holds the gradient
                    assert n == "momentum_buffer" and b1 == 0.0
                    continue
                _close(mine[i], ref, prev_state[n][i], t, f"step {t} tensor {i} {n}")
                prev_state[n][i] = ref.clone()
    assert all(torch.isfinite(p).all() for p in ps)
    # the steps were taken
    assert (ps[0] - torch.randn(shapes[0], generator=torch.Generator().manual_seed(3)).cuda()).abs().max() > 0
    return ps, s1, s2


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("mu", [0.9, 0.0])
@pytest.mark.parametrize("shapes", list(SHAPES))
def test_sgd_kernel_against_torch_on_fixed_grads(shapes, mu, wd):
    _, buf, s2 = _run(SGD, SHAPES[shapes], lambda qs: torch.optim.SGD(qs, lr=LR, momentum=mu, weight_decay=wd),
                      ["momentum_buffer"], wd, mu)
    assert all(not t.any() for t in s2)  # SGD never touches the second state
    assert all(t.abs().max() > 0 for t in buf)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("shapes", list(SHAPES))
def test_adam_kernel_against_torch_on_fixed_grads(shapes, wd):
    _run(ADAM, SHAPES[shapes], lambda qs: torch.optim.Adam(qs, lr=LR, weight_decay=wd), ["exp_avg", "exp_avg_sq"],
         wd, 0.9)


@pytest.mark.parametrize("shapes", list(SHAPES))
def test_adamax_through_the_new_entry_is_hgnn_adamax_step_bitwise(shapes):
    from hgnn_amd import _lib as L
    shp = SHAPES[shapes]
    gen = torch.Generator(device="cpu").manual_seed(5)
    init = [torch.randn(s, generator=gen) for s in shp]
    sides = []
    for _ in range(2):
        ps = [p.clone().cuda() for p in init]
        sides.append((ps, [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]))
    numel = (ctypes.c_int64 * len(shp))(*[p.numel() for p in init])
    stream = L.stream_handle(sides[0][0][0].device)
    for t in range(1, 6):
        grads = [torch.randn(s, generator=gen).cuda() for s in shp]
        ps, m, u = sides[0]
        L.check(L.lib().hgnn_adamax_step(len(ps), L.ptr_array(ps), L.ptr_array(grads), L.ptr_array(m), L.ptr_array(u),
                                         numel, LR, 0.9, 0.999, 1e-8, 0.01, t, stream), "adamax")
        ps, m, u = sides[1]
        L.check(L.lib().hgnn_optim_step(ADAMAX, len(ps), L.ptr_array(ps), L.ptr_array(grads), L.ptr_array(m),
                                        L.ptr_array(u), numel, LR, 0.9, 0.999, 1e-8, 0.01, t, stream), "optim")
        for k in range(3):
            for i, (a, b) in enumerate(zip(sides[0][k], sides[1][k])):
                assert torch.equal(a, b), (t, k, i)
    assert not torch.equal(sides[0][0][0].cpu(), init[0])


def _batch(graphs):
    from functions.batching import prepare_batch
    from functions.operators import graph_operators
    data = [[X, A, t, *graph_operators([X, A], 1, True)] for X, A, t in graphs]
    return [t.cuda() for t in prepare_batch(data, 0, 1)]


def _torch_opt(name, params, lr):
    if name == "sgd":
        return torch.optim.SGD(params, lr=lr, momentum=0.9)
    if name == "adam":
        return torch.optim.Adam(params, lr=lr)
    return torch.optim.Adamax(params, lr=lr)


_batches = {}


def _qm9_batch(seed):
    """One batch of 64 QM9-shape graphs, built once per seed and shared (never modified)."""
    import hgnn_amd.datagen as dg
    if seed not in _batches:
        _batches[seed] = _batch(dg.qm9_shape_dataset(64, seed=seed))
    return _batches[seed]


def _compare(model, ref, name, lr, steps):
    """Parameters after `steps` steps from equal states: the module docstring's rule."""
    gmax = max(q.grad.abs().max().item() for q in ref.parameters())
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        err = (p.detach() - q.detach()).abs()
        if name == "sgd":
            tight = err
        else:
            tight = err[q.grad.abs() > 1e-4 * gmax]
            assert err.max().item() <= 2 * lr * steps, (n, err.max().item())
        assert tight.numel() == 0 or tight.max().item() <= 1e-5 * max(1.0, q.abs().max().item()), \
            (n, tight.max().item())


@pytest.mark.parametrize("name", ["adamax", "sgd", "adam"])
def test_train_step_matches_torch_loop_per_optimizer(name):
    """One GNN_lg(0, 16, 4, 5, 1, 1, 2) batch of 64 QM9-shape graphs from equal states."""
    from functions.utils import normalize_data
    from hgnn_amd.train import TrainStep
    from models.gnns.model_mnb import GNN_lg
    torch.manual_seed(11)
    model = GNN_lg(0, 16, 4, 5, 1, 1, 2).cuda()
    ref = copy.deepcopy(model)
    mean, std, lr = 0.3, 1.7, 1e-3
    opt = _torch_opt(name, ref.parameters(), lr)
    step = TrainStep(model, lr=lr, t_mean=mean, t_std=std, optimizer=name, momentum=0.9)
    before = [p.detach().clone() for p in model.parameters()]
    X, W, T, XL, WL, Pm, Pd, mask, mask_lg, Nb, Eb = _qm9_batch(500)
    opt.zero_grad()
    loss = torch.nn.MSELoss()(ref([X, XL, W, WL, Pm, Pd], Nb, mask, Eb, mask_lg), normalize_data(T, mean, std))
    loss.backward()
    opt.step()
    s = step([X, W, T, XL, WL, Pm, Pd, mask, mask_lg, Nb, Eb]).cpu()
    assert abs(s[0].item() - loss.item()) <= 1e-5 * max(1.0, abs(loss.item())), (s[0].item(), loss.item())
    assert step.step_count == 1
    _compare(model, ref, name, lr, 1)
    assert any(not torch.equal(p.detach(), b) for p, b in zip(model.parameters(), before))
    # the state attributes the optimizer has, and reset_optimizer
    states = {"adamax": ("exp_avg", "exp_inf"), "adam": ("exp_avg", "exp_avg_sq"), "sgd": ("momentum_buffer",)}[name]
    for a in states:
        assert any(t.abs().max().item() > 0 for t in getattr(step, a)), a
    step.reset_optimizer()
    assert step.step_count == 0
    for a in states:
        assert all(not t.any() for t in getattr(step, a)), a


@pytest.mark.parametrize("name", ["sgd", "adam"])
def test_lr_damping_between_steps(name):
    """Two steps with .lr multiplied by 0.9 in between, against torch with param_group['lr'] changed
    (scripts/main_ccn.py:183-186); compared after each step, re-synchronised (parameters and state) in between,
    so the second step is compared from equal states and with a non-trivial state."""
    from functions.utils import normalize_data
    from hgnn_amd.train import TrainStep
    from models.gnns.model_mnb import GNN_lg
    torch.manual_seed(12)
    model = GNN_lg(0, 16, 4, 5, 1, 1, 2).cuda()
    ref = copy.deepcopy(model)
    mean, std, lr = 0.3, 1.7, 1e-3
    opt = _torch_opt(name, ref.parameters(), lr)
    step = TrainStep(model, lr=lr, t_mean=mean, t_std=std, optimizer=name, momentum=0.9)
    for i, seed in enumerate((500, 501)):
        X, W, T, XL, WL, Pm, Pd, mask, mask_lg, Nb, Eb = _qm9_batch(seed)
        opt.zero_grad()
        loss = torch.nn.MSELoss()(ref([X, XL, W, WL, Pm, Pd], Nb, mask, Eb, mask_lg), normalize_data(T, mean, std))
        loss.backward()
        opt.step()
        s = step([X, W, T, XL, WL, Pm, Pd, mask, mask_lg, Nb, Eb]).cpu()
        assert abs(s[0].item() - loss.item()) <= 1e-5 * max(1.0, abs(loss.item())), (i, s[0].item(), loss.item())
        _compare(model, ref, name, step.lr, 1)
        with torch.no_grad():
            for k, (p, q) in enumerate(zip(model.parameters(), ref.parameters())):
                p.copy_(q)
                st = opt.state[q]
                if name == "sgd":
                    step.momentum_buffer[k].copy_(st["momentum_buffer"])
                else:
                    step.exp_avg[k].copy_(st["exp_avg"])
                    step.exp_avg_sq[k].copy_(st["exp_avg_sq"])
        step.lr *= 0.9
        for gr in opt.param_groups:
            gr["lr"] *= 0.9
    assert step.step_count == 2 and abs(step.lr - lr * 0.81) < 1e-12
