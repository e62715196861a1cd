"""Host-only checks of the CCN-2D training kernel's entry points (hgnn_ccn2_small_train*): which shapes it takes,
the workspace query and the argument checks.  No GPU."""

import ctypes

import pytest


def _cfg(order=2, nmax=29, f=5, h=2, layers=2, n_out=1, bs=1):
    from hgnn_amd import _lib
    return _lib.CcnConfig(order, bs, nmax, f, h, layers, n_out, 0)


def _supported(**kw):
    from hgnn_amd import _lib
    return _lib.lib().hgnn_ccn2_small_train_supported(ctypes.byref(_cfg(**kw)))


def _ws(**kw):
    from hgnn_amd import _lib
    return _lib.lib().hgnn_ccn2_small_train_workspace_bytes(ctypes.byref(_cfg(**kw)))


def test_train_kernel_takes_the_qm9_shape():
    assert _supported() == 1
    # a property of the model and nmax, not of the number of graphs in the call
    assert _supported(bs=100000) == 1
    # the bound the one-shot forward and backward take today
    assert _supported(nmax=32) == 1
    assert _supported(nmax=32, f=8, h=2, layers=15, n_out=256) == 1


@pytest.mark.parametrize("kw", [dict(nmax=33), dict(h=3), dict(f=9), dict(layers=16), dict(order=1),
                                dict(n_out=257), dict(nmax=0)],
                         ids=["nmax33", "hidden3", "f_in9", "layers16", "order1", "n_out257", "nmax0"])
def test_train_kernel_refuses_shapes_outside_its_bounds(kw):
    assert _supported(**kw) == 0
    assert _ws(**kw) == 0


def test_null_config():
    from hgnn_amd import _lib
    lib = _lib.lib()
    assert lib.hgnn_ccn2_small_train_supported(None) == 0
    assert lib.hgnn_ccn2_small_train_workspace_bytes(None) == 0


def test_workspace_is_one_graphs_region_whatever_the_batch():
    one = _ws()
    assert one > 0
    assert _ws(bs=4096) == one
    # the levels and the dp format: (L + 2) nmax^3 hidden floats, and the per-node parameter partials on top
    assert one >= 4 * (2 + 2) * 29 ** 3 * 2
    assert one < 2 * 4 * (2 + 2) * 29 ** 3 * 2
    assert _ws(nmax=32) > one


def test_train_entry_points_reject_unsupported_null_and_oversized_calls():
    from hgnn_amd import _lib
    lib = _lib.lib()
    mse = [None] * 4 + [0.3, 1.7] + [None] * 5 + [0.9, 0.999, 1e-8, 0.0] + [None] * 4 + [1, None]
    xent = [None] * 4 + [None] * 5 + [0.9, 0.999, 1e-8, 0.0] + [None] * 4 + [1, None]
    # unsupported comes first: CCN-1D belongs to hgnn_ccn_small_train
    assert lib.hgnn_ccn2_small_train(ctypes.byref(_cfg(order=1, bs=4)), *mse) == 2
    assert lib.hgnn_ccn2_small_train_xent(ctypes.byref(_cfg(order=1, bs=4, n_out=2)), *xent) == 2
    assert lib.hgnn_ccn2_small_train(ctypes.byref(_cfg(nmax=33, bs=4)), *mse) == 2
    # null pointers; more than 4096 graphs
    assert lib.hgnn_ccn2_small_train(ctypes.byref(_cfg(bs=4)), *mse) == 1
    assert lib.hgnn_ccn2_small_train(ctypes.byref(_cfg(bs=4097)), *mse) == 1
    assert lib.hgnn_ccn2_small_train_xent(ctypes.byref(_cfg(bs=4, n_out=2)), *xent) == 1
    # cross-entropy over one class
    assert lib.hgnn_ccn2_small_train_xent(ctypes.byref(_cfg(bs=4, n_out=1)), *xent) == 1
    # the CCN-1D entries keep refusing order 2
    old = [None] * 4 + [0.3, 1.7] + [None] * 5 + [0.9, 0.999, 1e-8, 0.0] + [None] * 3 + [1, None]
    assert lib.hgnn_ccn_small_train(ctypes.byref(_cfg(bs=4)), *old) == 2
    assert lib.hgnn_ccn_small_train_supported(ctypes.byref(_cfg())) == 0
