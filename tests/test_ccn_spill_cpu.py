"""Host-only checks of the spill instantiation of the CCN-1D small-graph kernels (csrc/ccn_small_spill.hip,
csrc/ccn_small_batch_spill.hip: the row arrays in a global workspace): which shapes it takes, that the LDS kernels'
predicates answer what they answered, the workspace query, the entries' refusals, the constructor's, and the fp64
oracle's own condition on the inputs tests/test_gpu_ccn_spill.py uses.  No GPU."""

import ctypes

import pytest

import ccn_spill_util as U

CS_OMAX = 8 * (8 * 2 * 8 + 8)  # csrc/ccn_small_kernels.h: n_out bound of the training kernels
CS_SPILL_PAD = 64 * 8          # csrc/ccn_small.h: floats of tail padding of a row region


def _cfg(order=1, nmax=29, f=5, h=2, layers=2, n_out=1, bs=1):
    from hgnn_amd import _lib
    return _lib.CcnConfig(order, bs, nmax, f, h, layers, n_out, 0)


def _lib():
    from hgnn_amd import _lib
    return _lib.lib()


# (nmax, f, h, L) -> what the LDS kernels' predicates answer (the formula of csrc/ccn_small.h cs_lds_bytes: on the
# parent commit as here)
TAKEN = {(43, 5, 2, 2): 0, (49, 5, 2, 10): 0, (27, 8, 8, 2): 0, (64, 8, 8, 4): 0, (64, 8, 8, 15): 0, (29, 5, 2, 2): 1}
REFUSED = [dict(nmax=65), dict(f=9), dict(h=9), dict(layers=16), dict(order=2, nmax=8)]


@pytest.mark.parametrize("shape", list(TAKEN), ids=str)
def test_spill_takes_every_shape_within_the_advertised_bounds(shape):
    lib = _lib()
    nmax, f, h, L = shape
    for bs in (1, 7, 100000):
        cfg = _cfg(nmax=nmax, f=f, h=h, layers=L, bs=bs)
        assert lib.hgnn_ccn_small_spill_supported(ctypes.byref(cfg)) == 1
        assert lib.hgnn_ccn_small_spill_train_supported(ctypes.byref(cfg)) == 1
        # the existing predicates keep their answers
        assert lib.hgnn_ccn_small_supported(ctypes.byref(cfg)) == TAKEN[shape]
        assert lib.hgnn_ccn_small_train_supported(ctypes.byref(cfg)) == TAKEN[shape]
        assert lib.hgnn_ccn_small_train_batch_supported(ctypes.byref(cfg)) == TAKEN[shape]
        assert (lib.hgnn_ccn_small_workspace_bytes(ctypes.byref(cfg)) > 0) == bool(TAKEN[shape])


@pytest.mark.parametrize("kw", REFUSED, ids=str)
def test_spill_refuses_outside_the_bounds(kw):
    lib = _lib()
    cfg = _cfg(**kw)
    assert lib.hgnn_ccn_small_spill_supported(ctypes.byref(cfg)) == 0
    assert lib.hgnn_ccn_small_spill_train_supported(ctypes.byref(cfg)) == 0
    assert lib.hgnn_ccn_small_spill_workspace_bytes(ctypes.byref(cfg), 1) == 0
    if kw.get("order") != 2:  # order 2 belongs to the CCN-2D kernels' own rule
        assert lib.hgnn_ccn_small_supported(ctypes.byref(cfg)) == 0
    assert lib.hgnn_ccn_small_train_supported(ctypes.byref(cfg)) == 0


def test_spill_refuses_null_and_degenerate_configs():
    lib = _lib()
    assert lib.hgnn_ccn_small_spill_supported(None) == 0
    assert lib.hgnn_ccn_small_spill_train_supported(None) == 0
    assert lib.hgnn_ccn_small_spill_workspace_bytes(None, 1) == 0
    for kw in (dict(nmax=0), dict(layers=0), dict(f=0), dict(h=0)):
        assert lib.hgnn_ccn_small_spill_supported(ctypes.byref(_cfg(**kw))) == 0, kw
    assert lib.hgnn_ccn_small_spill_supported(ctypes.byref(_cfg(nmax=1))) == 1
    assert lib.hgnn_ccn_small_spill_supported(ctypes.byref(_cfg(nmax=64, layers=15, f=8, h=8))) == 1


def test_training_predicate_stops_one_past_the_output_bound():
    lib = _lib()
    at, past = _cfg(nmax=49, layers=10, n_out=CS_OMAX), _cfg(nmax=49, layers=10, n_out=CS_OMAX + 1)
    assert lib.hgnn_ccn_small_spill_train_supported(ctypes.byref(at)) == 1
    assert lib.hgnn_ccn_small_spill_train_supported(ctypes.byref(past)) == 0
    assert lib.hgnn_ccn_small_spill_supported(ctypes.byref(past)) == 1  # the one-shot calls have no such bound
    # independent of bs, like hgnn_ccn_small_train_supported
    assert lib.hgnn_ccn_small_spill_train_supported(ctypes.byref(_cfg(nmax=49, layers=10, bs=0))) == 1
    assert lib.hgnn_ccn_small_train_supported(ctypes.byref(_cfg(bs=0))) == 1


def _formula(nmax, f, h, L, bs, regions):
    """include/hgnn_amd.h: `regions` row regions, then the feat / ppart part of hgnn_ccn_small_workspace_bytes."""
    align = lambda n: (n + 255) // 256 * 256  # noqa: E731
    stride = align(4 * (nmax * nmax * (h * L + 2 * max(f, h) + 2 * h) + CS_SPILL_PAD))
    ptot = h * 2 * f + h + (L - 1) * (h * 2 * h + h)
    return stride, regions * stride + align(4 * bs * (f + L * h)) + (4 * bs * ptot if bs > 1 else 0)


@pytest.mark.parametrize("shape", [(49, 5, 2, 10), (27, 8, 8, 2), (64, 8, 8, 15)], ids=str)
def test_workspace_query_is_the_documented_formula(shape):
    lib = _lib()
    nmax, f, h, L = shape
    ws = lib.hgnn_ccn_small_spill_workspace_bytes
    for bs in (1, 5):
        cfg = _cfg(nmax=nmax, f=f, h=h, layers=L, bs=bs, n_out=2)
        sizes = {r: ws(ctypes.byref(cfg), r) for r in (1, 2, 3, 32, 4096)}
        for r, got in sizes.items():
            stride, want = _formula(nmax, f, h, L, bs, r)
            assert got == want, (bs, r, got, want)
        stride = sizes[2] - sizes[1]
        assert stride % 256 == 0
        assert stride >= 4 * (nmax * nmax * (h * L + 2 * max(f, h) + 2 * h) + 8)
        # linear in regions
        assert sizes[3] - sizes[2] == stride and sizes[4096] - sizes[32] == (4096 - 32) * stride
        for r in (0, -1):
            assert ws(ctypes.byref(cfg), r) == 0
    # where the LDS kernels exist, the rest is their workspace
    cfg = _cfg(bs=5)
    assert ws(ctypes.byref(cfg), 5) - 5 * _formula(29, 5, 2, 2, 5, 5)[0] == \
        lib.hgnn_ccn_small_workspace_bytes(ctypes.byref(cfg))


def test_entries_reject_bad_arguments():
    """HGNN_ERR_UNSUPPORTED (2) where the predicate refuses, HGNN_ERR_ARG (1) for a null pointer, a bad tag, batch or
    kind -- before any pointer is read, so the dummy pointers are never touched."""
    lib = _lib()
    nt = 6
    dummy = (ctypes.c_float * 64)()
    p = ctypes.cast(dummy, ctypes.c_void_p)
    arr = (ctypes.c_void_p * nt)(*[p.value] * nt)
    good, wide, two = _cfg(nmax=43, bs=6), _cfg(nmax=65, bs=6), _cfg(order=2, nmax=8, bs=6)

    def fwd(cfg, ws=p, tag=1):
        return lib.hgnn_ccn_small_spill_forward(ctypes.byref(cfg), p, p, p, arr, ws, p, tag, p, None)

    def bwd(cfg, ws=p):
        return lib.hgnn_ccn_small_spill_backward(ctypes.byref(cfg), p, p, p, arr, ws, p, arr, p, None)

    def train(cfg, ws=p, kind=0, xent=0, tag=1):
        return lib.hgnn_ccn_small_spill_train(ctypes.byref(cfg), kind, xent, p, p, p, p, 0.3, 1.7, arr, arr, arr, arr, p,
                                              0.9, 0.999, 1e-8, 0.0, p, p, ws, p, tag, None)

    def batch(cfg, ws=p, rows=p, B=4, kind=0, xent=0):
        return lib.hgnn_ccn_small_spill_train_batch(ctypes.byref(cfg), B, kind, xent, p, p, p, p, 0.3, 1.7, arr, arr,
                                                    arr, arr, p, 0.9, 0.999, 1e-8, 0.0, p, p, ws, rows, p, 1, None)

    for fn in (fwd, bwd, train, batch):
        assert fn(wide) == 2 and fn(two) == 2, fn.__name__
        assert fn(good, ws=None) == 1, fn.__name__
    assert fwd(good, tag=0) == 1 and train(good, tag=0) == 1
    assert train(good, kind=3) == 1 and batch(good, kind=-1) == 1
    assert train(good, xent=1) == 1 and batch(good, xent=1) == 1  # one class
    assert train(_cfg(nmax=43, bs=4097)) == 1 and batch(_cfg(nmax=43, bs=4097)) == 1
    assert batch(good, rows=None) == 1 and batch(good, B=0) == 1
    assert train(_cfg(nmax=43, n_out=CS_OMAX + 1, bs=6)) == 2


def test_constructor_and_one_shot_refusals_name_the_predicate():
    from hgnn_amd.ccn import CcnSpec
    from hgnn_amd.train import CcnTrainStep
    from models.compnets.model_ccn import CCN_1D, CCN_2D
    for net in (CCN_2D(5, 1, 2, 2), CCN_1D(9, 1, 2, 2), CCN_1D(5, 1, 9, 2), CCN_1D(5, 1, 2, 16)):
        for bs in (None, 4):
            with pytest.raises(RuntimeError, match="hgnn_ccn_small_spill_train_supported"):
                CcnTrainStep(net, t_mean=0.3, t_std=1.7, fused="ccn1_spill", batch_size=bs)
    for bs in (None, 4):  # a model it takes gets as far as the device check
        with pytest.raises(RuntimeError, match="GPU only"):
            CcnTrainStep(CCN_1D(5, 2, 2, 10), t_mean=0.3, t_std=1.7, fused="ccn1_spill", batch_size=bs)
    with pytest.raises(RuntimeError, match="hgnn_ccn_small_spill_supported"):
        CcnSpec(1, 5, 2, 2, 1).spill(3, 65)
    with pytest.raises(RuntimeError, match="hgnn_ccn_small_spill_supported"):
        CcnSpec(2, 5, 2, 2, 1).spill(3, 8)
    with pytest.raises(RuntimeError, match="SPILL_WS_CAP"):
        CcnSpec(1, 8, 8, 15, 1).spill(4096, 64)
    cfg, nbytes = CcnSpec(1, 5, 2, 10, 2).spill(3, 49)
    assert nbytes == _lib().hgnn_ccn_small_spill_workspace_bytes(ctypes.byref(cfg), 3) > 0


def test_the_spill_default_is_off():
    import hgnn_amd.train as T
    assert T.CCN1_TRAIN_SPILL_DEFAULT is False


@pytest.mark.parametrize("case,B", list(U.LOOSE), ids=str)
def test_oracle_inputs_meet_the_loose_bound_cap(case, B):
    """The GPU test's condition on its own inputs, recomputed here: the elements whose oracle gradient fell to the
    noise floor (<= 1e-4 max|g| of their tensor at some step) -- compared within 2 lr K instead of 1e-5 -- are at
    most 5 % of the parameters, and as many as measured: W27 0 of 322 (per graph and B = 2), W64 11 and 9 of 626,
    DA6 1 and 4 of 90.  (L = 10 on DA gives 7 and 8 of 138, over the cap: hence six layers.)"""
    orc = U.run_oracle(case, B)
    got = U.loose(orc)
    print(f"{case}, B = {B}: {got[0]} of {got[1]} elements on the loose bound")
    n = len(U.graphs(case))
    assert orc.steps == (n if B is None else -(-n // B)) and len(orc.outs) == n
    assert got[0] <= 0.05 * got[1], got
    assert got == U.LOOSE[(case, B)], got
