"""Host-only checks of the CCN training step (hgnn_amd.train.CcnTrainStep, hgnn_ccn_small_train_supported):
which shapes the one-dispatch training kernel takes, and the constructor's refusals.  No GPU."""

import ctypes

import pytest


def _supported(order=1, nmax=29, f=5, h=2, layers=2, n_out=1, bs=1):
    from hgnn_amd import _lib
    cfg = _lib.CcnConfig(order, bs, nmax, f, h, layers, n_out, 0)
    return _lib.lib().hgnn_ccn_small_train_supported(ctypes.byref(cfg))


def test_train_kernel_takes_the_qm9_shape():
    assert _supported() == 1
    # a property of the model and nmax, not of the number of graphs in the call
    assert _supported(bs=100000) == 1
    # the widest channels, at a size whose backward fits the LDS cap (4 * 400 * 48 B of levels + 20 KB fixed)
    assert _supported(nmax=20, f=8, h=8, layers=2) == 1
    # the QM9 model up to 42 nodes: 4 nmax^2 (h L + 2 max(f, h) + 2 h) = 72 nmax^2 bytes of levels
    assert _supported(nmax=42) == 1
    assert _supported(nmax=43) == 0


@pytest.mark.parametrize("kw", [dict(order=2), dict(nmax=65), dict(f=9), dict(h=9)],
                         ids=["order2", "nmax65", "f_in9", "hidden9"])
def test_train_kernel_refuses_shapes_outside_the_small_graph_bounds(kw):
    assert _supported(**kw) == 0


def test_train_kernel_refuses_a_backward_lds_request_above_the_cap():
    # 4 nmax^2 (h L + 2 max(f, h) + 2 h) = 4 * 4096 * 64 bytes = 1 MB of levels alone
    assert _supported(nmax=64, f=8, h=8, layers=4) == 0


def test_train_entry_points_reject_null_and_oversized_calls():
    from hgnn_amd import _lib
    lib = _lib.lib()
    assert lib.hgnn_ccn_small_train_supported(None) == 0
    cfg = _lib.CcnConfig(2, 4, 8, 5, 2, 2, 1, 0)
    args = [None] * 4 + [0.3, 1.7] + [None] * 5 + [0.9, 0.999, 1e-8, 0.0] + [None] * 3 + [1, None]
    assert lib.hgnn_ccn_small_train(ctypes.byref(cfg), *args) == 2  # unsupported: CCN-2D
    cfg = _lib.CcnConfig(1, 4097, 29, 5, 2, 2, 1, 0)
    assert lib.hgnn_ccn_small_train(ctypes.byref(cfg), *args) == 1  # null pointers / more than 4096 graphs
    assert lib.hgnn_ccn_eval_loss(None, None, 4, 1, 0.3, 1.7, None, None) == 1


def test_ccn_train_step_refuses_a_cpu_model():
    from hgnn_amd.train import CcnTrainStep
    from models.compnets.model_ccn import CCN_1D
    with pytest.raises(RuntimeError, match="GPU only"):
        CcnTrainStep(CCN_1D(5, 1, 2, 2), t_mean=0.3, t_std=1.7)


def test_ccn_train_step_refuses_the_classification_branch():
    from hgnn_amd.train import CcnTrainStep
    from models.compnets.model_ccn import CCN_1D
    net = CCN_1D(5, 1, 2, 2)
    with pytest.raises(RuntimeError, match="classification"):
        CcnTrainStep(net, t_mean=0.0, t_std=1.0)
    with pytest.raises(RuntimeError, match="classification"):
        CcnTrainStep(net, t_mean=0.3, t_std=1.7, classification=True)
    # regression on targets of mean 0, said explicitly, gets as far as the device check
    with pytest.raises(RuntimeError, match="GPU only"):
        CcnTrainStep(net, t_mean=0.0, t_std=1.0, classification=False)
