"""Host-only checks of the CCN classification loop: CcnTrainStep's constructor rules for the reference's
`mean == 0` branch (scripts/train_ccn.py:39-41), the argument checks of hgnn_ccn_small_train_xent and
hgnn_ccn_eval_xent, and the generated data set hgnn_amd.datagen.three_collinear_points
(functions/data_generator.py:45-87).  No GPU."""

import ctypes
import itertools

import pytest
import torch


def test_classification_needs_two_outputs_and_is_refused_before_the_device_check():
    from hgnn_amd.train import CcnTrainStep
    from models.compnets.model_ccn import CCN_1D
    one = CCN_1D(5, 1, 2, 2)  # a CPU model: the refusal below is not the device check's
    with pytest.raises(RuntimeError, match="classification"):
        CcnTrainStep(one, classification=True)
    with pytest.raises(RuntimeError, match="classification"):
        CcnTrainStep(one, t_mean=0.0, t_std=1.0)  # inferred from mean == 0, as TrainStep does


def test_classification_needs_no_target_statistics():
    from hgnn_amd.train import CcnTrainStep
    from models.compnets.model_ccn import CCN_1D
    two = CCN_1D(5, 2, 2, 2)
    # gets as far as the device check: neither the statistics nor the class count stop it
    with pytest.raises(RuntimeError, match="GPU only"):
        CcnTrainStep(two, classification=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        CcnTrainStep(two, t_mean=0.0, t_std=1.0)
    # regression still needs them
    with pytest.raises(RuntimeError, match="t_mean"):
        CcnTrainStep(two)


def test_xent_entry_points_reject_unsupported_null_and_oversized_calls():
    from hgnn_amd import _lib
    lib = _lib.lib()
    args = [None] * 9 + [0.9, 0.999, 1e-8, 0.0] + [None] * 3 + [1, None]
    cfg = _lib.CcnConfig(2, 4, 8, 5, 2, 2, 2, 0)
    assert lib.hgnn_ccn_small_train_xent(ctypes.byref(cfg), *args) == 2  # unsupported: CCN-2D
    cfg = _lib.CcnConfig(1, 4, 29, 5, 2, 2, 2, 0)
    assert lib.hgnn_ccn_small_train_xent(ctypes.byref(cfg), *args) == 1  # null pointers
    cfg = _lib.CcnConfig(1, 4097, 29, 5, 2, 2, 2, 0)
    assert lib.hgnn_ccn_small_train_xent(ctypes.byref(cfg), *args) == 1  # more than 4096 graphs
    # one class: every argument but n_out is valid (the pointers are never followed: the call returns first)
    buf = (ctypes.c_float * 64)()
    tab = (ctypes.c_void_p * 6)(*[ctypes.addressof(buf)] * 6)
    p, t = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(tab, ctypes.c_void_p)
    real = [p, p, None, p, t, t, t, t, p, 0.9, 0.999, 1e-8, 0.0, p, p, p, 1, None]
    cfg = _lib.CcnConfig(1, 4, 29, 5, 2, 2, 1, 0)
    assert lib.hgnn_ccn_small_train_xent(ctypes.byref(cfg), *real) == 1
    assert lib.hgnn_ccn_eval_xent(None, None, 4, 2, None, None, None) == 1


def _triples_rank_one(X):
    """Whether some three rows of X span a rank-1 subspace: second singular value <= 1e-4 of the first."""
    idx = torch.tensor(list(itertools.combinations(range(X.shape[0]), 3)))
    s = torch.linalg.svdvals(X.double()[idx])  # (triples, 3)
    return bool((s[:, 1] <= 1e-4 * s[:, 0]).any())


def test_three_collinear_points_properties():
    from hgnn_amd.datagen import three_collinear_points
    data = three_collinear_points(40, n_max=20, seed=5)
    assert len(data) == 40
    labels = set()
    for X, A, y, W, WL, Pm, Pd in data:
        n = X.shape[0]
        assert 3 <= n <= 19 and X.shape == (n, 5) and A.shape == (n, n)
        assert X.dtype == torch.float32 and A.dtype == torch.float32
        assert torch.equal(A, A.t()) and bool(((A == 0) | (A == 1)).all()) and A[0, 1] == 1
        assert y.dtype == torch.int64 and y.shape == (1,) and int(y) in (0, 1)
        assert W is None and WL is None and Pm is None and Pd is None
        assert _triples_rank_one(X) == (int(y) == 1), (n, int(y))
        labels.add(int(y))
    assert labels == {0, 1}
    sizes = {d[0].shape[0] for d in data}
    assert len(sizes) > 5, sizes  # random sizes, not one
    again = three_collinear_points(40, n_max=20, seed=5)
    for a, b in zip(data, again):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    other = three_collinear_points(40, n_max=20, seed=6)
    assert any(a[0].shape != b[0].shape or not torch.equal(a[0], b[0]) for a, b in zip(data, other))


def test_three_collinear_points_operators():
    from functions.operators import graph_operators
    from hgnn_amd.datagen import three_collinear_points
    data = three_collinear_points(3, n_max=8, seed=2, operators=True)
    bare = three_collinear_points(3, n_max=8, seed=2)
    for (X, A, y, W, WL, Pm, Pd), b in zip(data, bare):
        assert torch.equal(X, b[0]) and torch.equal(A, b[1]) and torch.equal(y, b[2])
        ref = graph_operators([X, A], dual=True)
        for got, want in zip((W, WL, Pm, Pd), ref):
            assert got.shape == want.shape and torch.equal(got, want)
        n, m = X.shape[0], int((A != 0).sum())
        assert W.shape == (n, n, 3) and WL.shape == (m, m, 3) and Pm.shape == (n, m) and Pd.shape == (n, m)
