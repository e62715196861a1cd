"""Host-only checks of the optimizer entry points (hgnn_optim_step, hgnn_ccn_small_train_opt,
hgnn_ccn2_small_train_opt) and of the optimizer argument of TrainStep / CcnTrainStep.  No GPU: every call here
returns from its argument checks, before any launch."""

import ctypes

import pytest

ARG, UNSUPPORTED = 1, 2
ADAMAX, SGD, ADAM = 0, 1, 2


def _lib():
    from hgnn_amd import _lib
    return _lib.lib()


def _cfg(order=1, nmax=29, f=5, h=2, layers=2, n_out=1, bs=4):
    from hgnn_amd import _lib
    return _lib.CcnConfig(order, bs, nmax, f, h, layers, n_out, 0)


class _Args:
    """Non-null arguments that are never dereferenced by a call the host refuses: `word` stands for every device
    pointer, `tensors` for the four pointer arrays (2 layers + 2 entries each, all non-null)."""

    def __init__(self, layers=2):
        self.buf = (ctypes.c_float * 16)()
        self.word = ctypes.cast(self.buf, ctypes.c_void_p)
        n = 2 * layers + 2
        self.tensors = (ctypes.c_void_p * n)(*[self.word.value] * n)

    def train(self, two, **null):
        """The arguments after (cfg, kind, xent); null: names set to NULL."""
        a = dict(X=self.word, adj=self.word, nb=None, y=self.word, params=self.tensors, grads=self.tensors,
                 s1=self.tensors, s2=self.tensors, steps=self.word, stats=self.word, out=self.word, ws=self.word,
                 err=self.word)
        for k in null:
            assert k in a
            a[k] = None
        ws = [a["ws"]] if two else []
        return [a["X"], a["adj"], a["nb"], a["y"], 0.3, 1.7, a["params"], a["grads"], a["s1"], a["s2"], a["steps"],
                0.9, 0.999, 1e-8, 0.0, a["stats"], a["out"], *ws, a["err"], 1, None]


ENTRIES = [("hgnn_ccn_small_train_opt", 1), ("hgnn_ccn2_small_train_opt", 2)]


def test_enum_values_are_the_headers():
    import os
    import re
    from hgnn_amd import _lib
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(here, "..", "include", "hgnn_amd.h")).read()
    got = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"HGNN_OPT_([A-Z]+) = (\d+)", src)}
    assert got == {"adamax": 0, "sgd": 1, "adam": 2} == _lib.OPT_KIND


def test_new_entries_are_bound():
    from hgnn_amd import _lib
    for name in ("hgnn_optim_step", "hgnn_ccn_small_train_opt", "hgnn_ccn2_small_train_opt"):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name)


def test_optim_step_argument_checks():
    lib = _lib()
    a = _Args()
    numel = (ctypes.c_int64 * 4)(4, 4, 4, 4)
    tail = (3e-4, 0.9, 0.999, 1e-8, 0.0)

    def call(kind, n, p, g, s1, s2, nm, step=1):
        return lib.hgnn_optim_step(kind, n, p, g, s1, s2, nm, *tail, step, None)

    t = a.tensors
    for kind in (ADAMAX, SGD, ADAM):
        assert call(kind, 0, None, None, None, None, None) == 0  # nothing to do
        assert call(kind, 4, None, t, t, t, numel) == ARG
        assert call(kind, 4, t, None, t, t, numel) == ARG
        assert call(kind, 4, t, t, None, t, numel) == ARG
        assert call(kind, 4, t, t, t, t, None) == ARG
        assert call(kind, 4, t, t, t, t, numel, step=0) == ARG
        assert call(kind, -1, t, t, t, t, numel) == ARG
    # the second state: required by adamax and adam, not looked at by sgd (checked on an empty list, so that the
    # accepted call launches nothing)
    assert call(ADAMAX, 4, t, t, t, None, numel) == ARG
    assert call(ADAM, 4, t, t, t, None, numel) == ARG
    zero = (ctypes.c_int64 * 4)(0, 0, 0, 0)
    assert call(SGD, 4, t, t, t, None, zero) == 0
    # a null tensor, a size outside [0, 2^30]
    holed = (ctypes.c_void_p * 4)(a.word.value, None, a.word.value, a.word.value)
    assert call(ADAM, 4, holed, t, t, t, numel) == ARG
    assert call(SGD, 4, t, t, holed, None, numel) == ARG
    assert call(SGD, 4, t, t, t, None, (ctypes.c_int64 * 4)(4, -1, 4, 4)) == ARG
    assert call(SGD, 4, t, t, t, None, (ctypes.c_int64 * 4)(4, (1 << 30) + 1, 4, 4)) == ARG


@pytest.mark.parametrize("kind", [-1, 3, 17])
def test_unknown_kind_is_refused(kind):
    lib = _lib()
    a = _Args()
    zero = (ctypes.c_int64 * 4)(0, 0, 0, 0)
    assert lib.hgnn_optim_step(kind, 4, a.tensors, a.tensors, a.tensors, a.tensors, zero, 3e-4, 0.9, 0.999, 1e-8,
                               0.0, 1, None) == ARG
    for name, order in ENTRIES:
        assert getattr(lib, name)(ctypes.byref(_cfg(order=order)), kind, 0, *a.train(order == 2)) == ARG


@pytest.mark.parametrize("name,order", ENTRIES)
@pytest.mark.parametrize("kind", [ADAMAX, SGD, ADAM])
def test_train_opt_null_pointers(name, order, kind):
    fn = getattr(_lib(), name)
    a = _Args()
    two = order == 2
    names = ["X", "adj", "y", "params", "grads", "s1", "steps", "stats", "out", "err"] + (["ws"] if two else [])
    if kind != SGD:
        names.append("s2")
    for n in names:
        for xent in (0, 1):
            cfg = _cfg(order=order, n_out=2)
            assert fn(ctypes.byref(cfg), kind, xent, *a.train(two, **{n: None})) == ARG, (n, xent)
    assert fn(None, kind, 0, *a.train(two)) == UNSUPPORTED
    # a null entry of a pointer array
    holed = (ctypes.c_void_p * 6)(*[a.word.value] * 6)
    holed[3] = None
    args = a.train(two)
    args[8] = holed  # state1
    assert fn(ctypes.byref(_cfg(order=order)), kind, 0, *args) == ARG
    # the tag and cross entropy over one class
    args = a.train(two)
    args[-2] = 0
    assert fn(ctypes.byref(_cfg(order=order)), kind, 0, *args) == ARG
    assert fn(ctypes.byref(_cfg(order=order, n_out=1)), kind, 1, *a.train(two)) == ARG


@pytest.mark.parametrize("name,order", ENTRIES)
@pytest.mark.parametrize("kind", [ADAMAX, SGD, ADAM])
def test_more_than_4096_graphs_are_refused(name, order, kind):
    """Every pointer is non-null, so the graph count is the one reason."""
    fn = getattr(_lib(), name)
    a = _Args()
    assert fn(ctypes.byref(_cfg(order=order, bs=4097)), kind, 0, *a.train(order == 2)) == ARG
    assert fn(ctypes.byref(_cfg(order=order, bs=0)), kind, 0, *a.train(order == 2)) == ARG


ONE_D = [dict(nmax=65), dict(h=9), dict(f=9), dict(order=2), dict(nmax=0), dict(layers=16)]
TWO_D = [dict(nmax=33), dict(h=3), dict(f=9), dict(layers=16), dict(order=1), dict(n_out=257), dict(nmax=0)]


@pytest.mark.parametrize("kind", [ADAMAX, SGD, ADAM])
def test_new_entries_are_unsupported_wherever_the_existing_ones_are(kind):
    lib = _lib()
    a = _Args()
    for kw in ONE_D + [dict()]:
        cfg = _cfg(**{"order": 1, **kw})
        sup = lib.hgnn_ccn_small_train_supported(ctypes.byref(cfg))
        got = lib.hgnn_ccn_small_train_opt(ctypes.byref(cfg), kind, 0, *a.train(False, X=None))
        assert got == (ARG if sup else UNSUPPORTED), (kw, sup, got)
    for kw in TWO_D + [dict()]:
        cfg = _cfg(**{"order": 2, **kw})
        sup = lib.hgnn_ccn2_small_train_supported(ctypes.byref(cfg))
        got = lib.hgnn_ccn2_small_train_opt(ctypes.byref(cfg), kind, 0, *a.train(True, X=None))
        assert got == (ARG if sup else UNSUPPORTED), (kw, sup, got)
    # both ways round: the lists above hold supported and unsupported shapes
    assert lib.hgnn_ccn_small_train_supported(ctypes.byref(_cfg())) == 1
    assert lib.hgnn_ccn_small_train_supported(ctypes.byref(_cfg(nmax=65))) == 0
    assert lib.hgnn_ccn2_small_train_supported(ctypes.byref(_cfg(order=2))) == 1
    assert lib.hgnn_ccn2_small_train_supported(ctypes.byref(_cfg(order=2, nmax=33))) == 0


def test_step_scalars_are_indexed_by_step():
    """_Optimizer._step_scalars: the (n, 2) rows the fused entries take, in double."""
    import math
    from hgnn_amd.train import _Optimizer
    o = _Optimizer()
    o.lr, o.betas = 1e-3, (0.9, 0.999)
    o.optimizer = "adam"
    rows = o._step_scalars(3, 2)
    assert rows == [(1e-3 / (1 - 0.9 ** 4), math.sqrt(1 - 0.999 ** 4)), (1e-3 / (1 - 0.9 ** 5), math.sqrt(1 - 0.999 ** 5))]
    o.optimizer = "sgd"
    assert o._step_scalars(3, 2) == [(1e-3, 0.0)] * 2
    o.optimizer = "adamax"
    assert o._step_scalars(0, 1) == [(1e-3 / (1 - 0.9), 0.0)]


def test_unknown_optimizer_name_raises():
    """The name is checked before anything touches the device."""
    from hgnn_amd.train import _Optimizer
    o = _Optimizer()
    o.params = []
    with pytest.raises(RuntimeError, match="rmsprop"):
        o._init_optimizer("rmsprop", 0.9)
    for name, attrs in (("adamax", ("exp_avg", "exp_inf")), ("adam", ("exp_avg", "exp_avg_sq")),
                        ("sgd", ("momentum_buffer",))):
        o = _Optimizer()
        o.params = []
        o._init_optimizer(name, 0.5)
        assert o.optimizer == name and o.step_count == 0 and o.momentum == 0.5
        for a in attrs:
            assert getattr(o, a) == []
        assert not hasattr(o, "exp_inf") or name == "adamax"
        assert not hasattr(o, "momentum_buffer") or name == "sgd"


def test_train_steps_refuse_an_unknown_optimizer():
    """optimizer="rmsprop" raises from both steps, before the device is looked at."""
    from hgnn_amd.train import CcnTrainStep, TrainStep
    from models.compnets.model_ccn import CCN_1D
    from models.gnns.model_mnb import GNN_lg
    with pytest.raises(RuntimeError, match="rmsprop"):
        TrainStep(GNN_lg(0, 8, 3, 5, 1, 1, 2), optimizer="rmsprop")
    with pytest.raises(RuntimeError, match="rmsprop"):
        CcnTrainStep(CCN_1D(5, 1, 2, 2), t_mean=0.3, t_std=1.7, optimizer="rmsprop")
