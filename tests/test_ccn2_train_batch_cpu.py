"""Host-only checks of the CCN-2D mini-batch kernels (hgnn_amd.train.CcnTrainStep(fused="ccn2_batch", batch_size=B),
hgnn_ccn2_small_train_batch*): which shapes they take, the workspace size, the entry's refusals and the constructor's.
No GPU."""

import ctypes

import pytest

NAMES = ("hgnn_ccn2_small_train_batch_supported", "hgnn_ccn2_small_train_batch_workspace_bytes",
         "hgnn_ccn2_small_train_batch")


def _cfg(order=2, nmax=29, f=5, h=2, layers=2, n_out=1, bs=1):
    from hgnn_amd import _lib
    return _lib.CcnConfig(order, bs, nmax, f, h, layers, n_out, 0)


SHAPES = [dict(nmax=29), dict(nmax=32), dict(nmax=33), dict(f=8), dict(f=9), dict(h=2), dict(h=3), dict(n_out=256),
          dict(n_out=257), dict(layers=15), dict(bs=100000)]


@pytest.mark.parametrize("kw", SHAPES, ids=[str(i) for i in range(len(SHAPES))])
def test_supported_is_the_per_graph_kernels_rule(kw):
    from hgnn_amd import _lib
    lib = _lib.lib()
    cfg = _cfg(**kw)
    assert lib.hgnn_ccn2_small_train_batch_supported(ctypes.byref(cfg)) == \
        lib.hgnn_ccn2_small_train_supported(ctypes.byref(cfg))


def test_supported_takes_the_bounds_and_refuses_order_1_and_null():
    from hgnn_amd import _lib
    sup = _lib.lib().hgnn_ccn2_small_train_batch_supported
    assert sup(ctypes.byref(_cfg())) == 1
    assert sup(ctypes.byref(_cfg(nmax=32, f=8, n_out=256))) == 1
    for kw in (dict(nmax=33), dict(f=9), dict(h=3), dict(n_out=257), dict(order=1)):
        assert sup(ctypes.byref(_cfg(**kw))) == 0, kw
    assert sup(None) == 0


def _gstride(nmax, f, h, layers):
    """csrc/ccn2_small.h q_gstride: the floats of one graph's region."""
    r1, r2 = nmax * nmax, nmax ** 3
    fl = layers * r2 * h + 2 * r2 * h + r1 * h + nmax * h + r1 * f
    return (fl + 63) // 64 * 64


def test_workspace_grows_with_the_batch():
    from hgnn_amd import _lib
    ws = _lib.lib().hgnn_ccn2_small_train_batch_workspace_bytes
    for kw in (dict(bs=6), dict(bs=4096), dict(bs=256, nmax=32, f=8, layers=3, n_out=3), dict(bs=4096, nmax=1, f=1,
                                                                                               h=1, layers=1)):
        cfg = _cfg(**kw)
        batches = (1, 2, 3, 4, 32, 33, 256, 4096)
        sizes = [ws(ctypes.byref(cfg), b) for b in batches]
        assert sizes[0] > 0 and all(s % 256 == 0 for s in sizes)
        # never smaller for a larger batch, and larger: every graph region is a whole number of 256-byte lines
        assert all(x < y for x, y in zip(sizes, sizes[1:])), sizes
        gs = _gstride(cfg.nmax, cfg.f_in, cfg.hidden, cfg.layers)
        for b, s in zip(batches, sizes):
            assert s >= 4 * b * gs, (b, s, gs)
    # the docstring's figure: a graph region at nmax = 29, L = 2, h = 2 is about 0.8 MB
    assert 0.75e6 < 4 * _gstride(29, 5, 2, 2) < 0.85e6
    # more graphs in the call: more reject words, never fewer bytes
    assert ws(ctypes.byref(_cfg(bs=4096)), 4) >= ws(ctypes.byref(_cfg(bs=6)), 4)
    assert ws(ctypes.byref(_cfg(order=1, bs=6)), 4) == 0
    assert ws(ctypes.byref(_cfg(nmax=33, bs=6)), 4) == 0
    assert ws(ctypes.byref(_cfg(bs=6)), 0) == 0
    assert ws(ctypes.byref(_cfg(bs=4097)), 4) == 0
    assert ws(ctypes.byref(_cfg(bs=0)), 4) == 0
    assert ws(None, 4) == 0


def test_entry_rejects_bad_arguments():
    """tests/test_ccn_train_batch_cpu.py's list for the CCN-2D entry: null pointers, batch < 1, bs outside 1 .. 4096,
    an unknown kind, tag = 0 and xent with one output: HGNN_ERR_ARG (1); order 1, nmax 33 and a null config:
    HGNN_ERR_UNSUPPORTED (2).  Every refusal comes before any pointer is read, so the dummy pointers are never
    touched."""
    from hgnn_amd import _lib
    lib = _lib.lib()
    nt = 6  # CCN_2D(5, 1, 2, 2): 2 layers + fc, weights and biases
    dummy = (ctypes.c_float * 64)()
    p = ctypes.cast(dummy, ctypes.c_void_p)
    arr = (ctypes.c_void_p * nt)(*[p.value] * nt)

    def call(cfg, batch=4, kind=0, xent=0, null=None, tag=1, t_std=1.7):
        ptrs = dict(X=p, adj=p, nb=p, y=p, params=arr, grads=arr, s1=arr, s2=arr, steps=p, stats=p, out=p, ws=p,
                    err=p)
        if null:
            ptrs[null] = None
        return lib.hgnn_ccn2_small_train_batch(ctypes.byref(cfg), batch, kind, xent, ptrs["X"], ptrs["adj"],
                                               ptrs["nb"], ptrs["y"], 0.3, t_std, ptrs["params"], ptrs["grads"],
                                               ptrs["s1"], ptrs["s2"], ptrs["steps"], 0.9, 0.999, 1e-8, 0.0,
                                               ptrs["stats"], ptrs["out"], ptrs["ws"], ptrs["err"], tag, None)

    good = _cfg(bs=6)
    for name in ("X", "adj", "y", "params", "grads", "s1", "s2", "steps", "stats", "out", "ws", "err"):
        assert call(good, null=name) == 1, name
    assert call(good, batch=0) == 1
    assert call(good, batch=-3) == 1
    assert call(_cfg(bs=4097)) == 1
    assert call(_cfg(bs=0)) == 1
    assert call(good, kind=3) == 1
    assert call(good, kind=-1) == 1
    assert call(good, tag=0) == 1
    assert call(good, xent=1) == 1  # one class: cross-entropy is identically 0
    assert call(good, t_std=1e-6) == 1  # regression: (float)(t_std + 1e-8) < 1e-5f
    assert call(_cfg(order=1, bs=6)) == 2
    assert call(_cfg(nmax=33, bs=6)) == 2
    assert lib.hgnn_ccn2_small_train_batch(None, 4, 0, 0, *[None] * 4, 0.3, 1.7, *[None] * 5, 0.9, 0.999, 1e-8,
                                           0.0, *[None] * 4, 1, None) == 2


def test_the_names_are_bound_and_exported():
    from hgnn_amd import _lib
    lib = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    # the argument list is hgnn_ccn_small_train_batch's
    assert _lib.SIGNATURES["hgnn_ccn2_small_train_batch"] == _lib.SIGNATURES["hgnn_ccn_small_train_batch"]
    assert _lib.SIGNATURES["hgnn_ccn2_small_train_batch_workspace_bytes"][1] is ctypes.c_size_t


def test_the_constructor_refuses_what_the_kernels_do_not_take():
    from hgnn_amd import train
    from models.compnets.model_ccn import CCN_1D, CCN_2D
    kw = dict(t_mean=0.3, t_std=1.7, fused="ccn2_batch")
    with pytest.raises(RuntimeError, match="needs batch_size"):
        train.CcnTrainStep(CCN_2D(5, 1, 2, 2), **kw)
    with pytest.raises(RuntimeError, match="ccn2_batch.*needs CCN_2D"):
        train.CcnTrainStep(CCN_1D(5, 1, 2, 2), batch_size=4, **kw)
    with pytest.raises(RuntimeError, match="ccn2_batch.*needs CCN_2D"):
        train.CcnTrainStep(CCN_2D(5, 1, 3, 2), batch_size=4, **kw)  # hidden 3
    with pytest.raises(RuntimeError, match="ccn2_batch.*needs CCN_2D"):
        train.CcnTrainStep(CCN_2D(9, 1, 2, 2), batch_size=4, **kw)  # nine input features
    # a model the kernels take passes every host-side check and stops at the device's
    with pytest.raises(RuntimeError, match="GPU only"):
        train.CcnTrainStep(CCN_2D(5, 1, 2, 2), batch_size=4, **kw)
    # "ccn2" with batch_size still raises, and now names the selector that exists
    with pytest.raises(RuntimeError, match="ccn2_batch"):
        train.CcnTrainStep(CCN_2D(5, 1, 2, 2), t_mean=0.3, t_std=1.7, batch_size=4, fused="ccn2")
    assert train.CCN2_TRAIN_BATCH_FUSED_DEFAULT is False
