"""The host side of the device batcher (csrc/batcher.hip, hgnn_amd.dataset.DevicePack), on the CPU.

hgnn_csr_layout_from_counts sizes a batch image from per-graph records {n, m, nnz[6], flags, 0} (the records
hgnn_pack_count writes on the device).  It must give the very hgnn_csr_layout that hgnn_csr_batch_plan gives for
the same graphs -- both form the offsets in one function -- compared here as raw struct bytes, with the records
taken from the host plan at bs = 1.
"""

import ctypes

import numpy as np
import pytest
import torch

ERR_UNSUPPORTED, ERR_INDEX = 2, 4


def _graphs(n_qm9=12, n_sbm=2, seed=5):
    """tests/test_builder.py's graphs: QM9 shapes, SBM-24, a self loop, an isolated last node, a single node."""
    import hgnn_amd.datagen as dg
    gs = dg.qm9_shape_dataset(n_qm9, seed=seed) + dg.sbm_dataset(n_sbm, n=24, seed=seed)
    X, A, t = gs[0]
    A = A.clone()
    A[0, 0] = 1.0
    gs[0] = (X, A, t)
    X, A, t = gs[1]
    A = A.clone()
    A[-1, :] = 0
    A[:, -1] = 0
    gs[1] = (X, A, t)
    gs.append((torch.eye(1, 5), torch.zeros(1, 1), torch.randn(13)))
    return gs


def _plan(graphs, J, dual):
    from hgnn_amd import _lib as L
    As = [A.contiguous().float() for _, A, _ in graphs]
    bs = len(As)
    n_nodes = (ctypes.c_int * bs)(*[a.shape[0] for a in As])
    ptrs = (ctypes.c_void_p * bs)(*[a.data_ptr() for a in As])
    lay = L.CsrLayout()
    L.check(L.lib().hgnn_csr_batch_plan(bs, n_nodes, ptrs, graphs[0][0].shape[1], J, dual, ctypes.byref(lay)), "plan")
    return lay


def _records(graphs, J, dual):
    rec = np.zeros((len(graphs), 10), dtype=np.int32)
    for g, inst in enumerate(graphs):
        lay = _plan([inst], J, dual)
        rec[g, 0], rec[g, 1] = lay.nodes, lay.edges
        rec[g, 2:8] = list(lay.nnz)
    return rec


def _from_counts(rec, f_in, J, dual):
    from hgnn_amd import _lib as L
    rec = np.ascontiguousarray(rec, dtype=np.int32)
    lay = L.CsrLayout()
    st = L.lib().hgnn_csr_layout_from_counts(len(rec), ctypes.c_void_p(rec.ctypes.data), f_in, J, dual,
                                             ctypes.byref(lay))
    return st, lay


@pytest.mark.parametrize("dual", [0, 1])
@pytest.mark.parametrize("J", [1, 2, 3])
def test_layout_from_counts_equals_plan(J, dual):
    gs = _graphs()
    rec = _records(gs, J, dual)
    rng = np.random.default_rng(3)
    batches = [list(range(len(gs))), list(rng.permutation(len(gs))), [3, 3, 0, 14, 7, 3, 14], [5], [14]]
    for idx in batches:
        want = _plan([gs[i] for i in idx], J, dual)
        st, got = _from_counts(rec[idx], gs[0][0].shape[1], J, dual)
        assert st == 0
        assert bytes(got) == bytes(want), (J, dual, idx)


def test_layout_from_counts_flags():
    gs = _graphs()
    rec = _records(gs, 1, 1)
    f_in = gs[0][0].shape[1]
    bad = rec.copy()
    bad[4, 8] = 1  # outside the device builder's bounds
    assert _from_counts(bad, f_in, 1, 1)[0] == ERR_UNSUPPORTED
    bad[4, 8] = 4  # malformed COO
    assert _from_counts(bad, f_in, 1, 1)[0] == ERR_UNSUPPORTED
    bad[9, 8] = 2  # the edge-slot index error wins over the others
    assert _from_counts(bad, f_in, 1, 1)[0] == ERR_INDEX
    bad = rec.copy()
    bad[0, 8] = 2
    assert _from_counts(bad, f_in, 1, 1)[0] == ERR_INDEX
    assert _from_counts(rec, f_in, 1, 1)[0] == 0
