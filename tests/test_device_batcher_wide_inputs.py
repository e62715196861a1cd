"""The wide pack (tests/device_batcher_wide_util.py) is what its docstrings say it is, for the committed generators:
the shapes the GPU tests of the n <= 64 node-family builder rely on.  Needs no GPU: the entry counts are the host
plan's (hgnn_csr_batch_plan at bs = 1, dual = 0)."""

import ctypes

import numpy as np
import torch

import device_batcher_wide_util as U


def _plan(graph, J):
    from hgnn_amd import _lib as L
    x, a, _ = graph
    a = a.contiguous().float()
    lay = L.CsrLayout()
    L.check(L.lib().hgnn_csr_batch_plan(1, (ctypes.c_int * 1)(a.shape[0]), (ctypes.c_void_p * 1)(a.data_ptr()),
                                        x.shape[1], J, 0, ctypes.byref(lay)), "plan")
    return lay


def _nnz(a):
    return int((a != 0).sum())


def test_node_counts_and_nnz():
    gs = U.wide_graphs()
    n = [x.shape[0] for x, _, _ in gs]
    assert n == [50, 50, 50] + U.COLLINEAR_N + [64, 33, 40, 64, 1] + n[14:]
    assert all(9 <= k <= 29 for k in n[14:])  # QM9 shapes: the narrow kernel's graphs
    assert U.small_indices(gs) == [4, 5, 8, 13, 14, 15, 16, 17]
    assert [_nnz(gs[i][1]) for i in U.INDEX["sbm"]] == U.SBM_NNZ
    for x, a, t in gs:
        assert x.shape[1] == 5 and t.shape == (13,) and a.shape == (x.shape[0],) * 2
        assert torch.equal(a, a.T)
    k64, k33, path, single = (gs[U.INDEX[k]][1] for k in ("k64", "k33", "path64", "single"))
    assert _nnz(k64) == 64 * 64  # n^2: the COO cap and the node cap at once
    assert _nnz(k33) == 33 * 32 and not torch.diagonal(k33).any()
    assert _nnz(path) == 2 * 62 and not path[63].any() and not path[:, 63].any()
    assert _nnz(single) == 0


def test_collinear_graphs_are_dense_with_self_loops():
    gs = U.wide_graphs()
    for i in U.INDEX["collinear"]:
        a = gs[i][1]
        n = a.shape[0]
        if n > 3:  # min(A + A^T, 1) of a half-filled A: 3 / 4 of the pairs, 1 / 2 of the diagonal
            assert _nnz(a) > 0.6 * n * n
            loops = int((torch.diagonal(a) != 0).sum())
            assert 0.25 * n < loops < 0.75 * n


def test_union_patterns():
    gs = U.wide_graphs()
    sbm0 = gs[0]
    assert _plan(sbm0, 1).nnz[0] == U.SBM_NNZ[0] + 50  # A has no self loops: the diagonal is added
    assert _plan(sbm0, 2).nnz[0] == 1948  # of 2500: partly filled
    assert _plan(sbm0, 3).nnz[0] == 2500  # full
    for J, nbytes in ((1, 136960), (2, 268032), (3, 268032)):
        lay = _plan(gs[U.INDEX["k64"]], J)
        assert lay.nnz[0] == lay.nnz[1] == 4096 and lay.bytes == nbytes


def test_high40_cancellation():
    """Bonds only among nodes >= 32; two fp64 sums of A^2 cancel to exactly 0.0 and the host stores no entry."""
    x, a, _ = U.high40()
    assert not a[:32].any() and not a[:, :32].any()
    a2 = a.double() @ a.double()
    assert a2[34, 36] == 0.0 and a2[35, 37] == 0.0 and a[34, 35] * a[35, 36] != 0
    structural = ((a != 0) | ((a != 0).double() @ (a != 0).double() > 0) | torch.eye(40, dtype=torch.bool))
    assert int(structural.sum()) == 58
    lay = _plan((x, a, None), 2)
    assert lay.nnz[0] == 54
    from hgnn_amd.csr import CsrBatch
    b = CsrBatch([(x, a)], J=2, dual=False, targets=torch.zeros(1), device="cpu")
    rows, ent = b.lists()[0]
    start, count = int(rows[34][0]), int(rows[34][1])
    cols = ent[start:start + count, 0].copy().view(np.int32).tolist()
    assert cols == [34, 35, 37]  # 36 is missing: (A^2)[34][36] == 0.0


def test_real_weights_keep_the_patterns():
    gs = U.wide_graphs()
    rw = U.real_weights(gs)
    for (_, a, _), (_, w, _) in zip(gs, rw):
        assert torch.equal(a != 0, w != 0) and torch.equal(w, w.T)
        if w.any():
            assert 0.5 <= float(w[w != 0].min()) and float(w.max()) <= 2.5


def test_every_graph_round_trips_through_a_pack(tmp_path):
    from hgnn_amd.dataset import GraphPack, check_coo
    for name, gs in (("plain", U.wide_graphs()), ("real", U.real_weights(U.wide_graphs()))):
        pack = GraphPack.write(str(tmp_path / name), gs)
        assert len(pack) == U.N_GRAPHS
        check_coo(pack)
        for i, (x, a, t) in enumerate(gs):
            px, pa, pt = pack.graph(i)
            assert torch.equal(px, x) and torch.equal(pa, a) and torch.equal(pt, t), i
        cnt = np.diff(np.asarray(pack.adj_off))
        assert int(cnt[U.INDEX["k64"]]) == 4096
