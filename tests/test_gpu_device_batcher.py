"""The device batcher (csrc/batcher.hip, hgnn_amd.dataset.DevicePack) against the host batcher (csrc/builder.cpp).

DevicePack.batch builds the executor's CSR batch image on the GPU from the resident pack.  It must be the image
hgnn_csr_batch_build writes on the host, byte for byte -- operator values, row lists, offsets, alignment gaps --
so every comparison here is torch.equal on the raw bytes or on what the executor computes from them.
"""

import copy
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLAG_BOUNDS, FLAG_INDEX = 1, 2


def _edge_cases(gs):
    """tests/test_builder.py's edge cases on the first two graphs, plus a single node without bonds (m = 0)."""
    X, A, t = gs[0]
    A = A.clone()
    A[0, 0] = 1.0  # a self loop: an edge slot that no bond fills (Q2)
    gs[0] = (X, A, t)
    X, A, t = gs[1]
    A = A.clone()
    A[-1, :] = 0  # the last node isolated
    A[:, -1] = 0
    gs[1] = (X, A, t)
    gs.append((torch.eye(1, 5), torch.zeros(1, 1), torch.randn(13, generator=torch.Generator().manual_seed(1))))
    return gs


def _hand_graph(n, bonds):
    A = torch.zeros(n, n)
    for i, j in bonds:
        A[i, j] = A[j, i] = 1.0
    X = torch.zeros(n, 5)
    X[torch.arange(n), torch.arange(n) % 5] = 1.0
    return X, A, torch.arange(13, dtype=torch.float32) * 0.25 - float(n)


def _graphs():
    import hgnn_amd.datagen as dg
    gs = _edge_cases(dg.qm9_shape_dataset(48, seed=5))
    gs += dg.sbm_dataset(2, n=16, seed=5)  # dense squares: sums over many terms, wide union patterns
    assert [int((a != 0).sum()) for _, a, _ in gs[-2:]] == [44, 48]
    gs.append(_hand_graph(2, [(0, 1)]))  # B = 1: slot 1 is the last reverse
    full = _hand_graph(32, [(i, i + 1) for i in range(31)] + [(0, 5), (3, 9), (10, 20), (15, 30), (2, 31)])
    assert full[1].shape[0] == 32 and int((full[1] != 0).sum()) == 72  # exactly the device builder's bounds
    gs.append(full)
    return gs


def _real_weights(gs, seed=11):
    """The same graphs with every bond weight (and self loop) a seeded uniform(0.5, 2.5) value, symmetric."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for X, A, t in gs:
        R = torch.rand(A.shape, generator=g) * 2.0 + 0.5
        W = torch.triu(R, 1)
        W = W + W.T + torch.diag(torch.diagonal(R))
        out.append((X, torch.where(A != 0, W, torch.zeros_like(W)), t))
    return out


@pytest.fixture(scope="module")
def packs(tmp_path_factory):
    from hgnn_amd.dataset import GraphPack
    root = tmp_path_factory.mktemp("device_batcher")
    gs = _graphs()
    return {"plain": GraphPack.write(str(root / "plain"), gs),
            "real": GraphPack.write(str(root / "real"), _real_weights(gs))}


def _host_batch(pack, idx, J, dual, task=0, device="cpu"):
    from hgnn_amd.csr import CsrBatch
    graphs = [pack.graph(i) for i in idx]
    targets = torch.tensor([float(t[task]) for _, _, t in graphs])
    return CsrBatch([(x, a) for x, a, _ in graphs], J=J, dual=dual, targets=targets, device=device)


def _index_lists(n):
    rng = np.random.default_rng(7)
    return [list(range(n)), list(range(n))[::-1], [3, 3, 0, n - 1, 7, 3, n - 1, n - 2, 50], [n - 1], [50],
            [int(i) for i in rng.integers(0, n, 64)]]


def _assert_same_batch(dev_batch, host_batch):
    assert bytes(dev_batch.layout) == bytes(host_batch.layout)
    got = dev_batch.image.cpu()
    want = host_batch.host if host_batch.image.device.type == "cpu" else host_batch.image.cpu()
    if not torch.equal(got, want):
        diff = torch.nonzero(got != want).flatten()
        raise AssertionError(f"{diff.numel()} image bytes differ, first at {int(diff[0])} of {got.numel()}")
    assert torch.equal(dev_batch.T.cpu(), host_batch.T.cpu())


@pytest.mark.parametrize("dual", [True, False])
@pytest.mark.parametrize("J", [1, 2, 3])
def test_image_equals_host_image(packs, J, dual):
    pack = packs["plain"]
    dp = pack.to_device(J=J, dual=dual)
    assert not dp.counts[:, 8].any()
    for idx in _index_lists(len(pack)):
        b = dp.batch(idx, 2)
        _assert_same_batch(b, _host_batch(pack, idx, J, dual, task=2))
        assert b.image.is_cuda and b.bs == len(idx)


@pytest.mark.parametrize("dual", [True, False])
def test_image_equals_host_image_real_weights(packs, dual):
    """Weights that are not dyadic: every fp64 sum must be formed in the host's order, multiply and add apart."""
    pack = packs["real"]
    dp = pack.to_device(J=3, dual=dual)
    for idx in _index_lists(len(pack)):
        _assert_same_batch(dp.batch(idx, 0), _host_batch(pack, idx, 3, dual))


def test_from_image_lists_and_views(packs):
    """CsrBatch.from_image fills what the constructor fills; lists() reads the lazily copied host image."""
    pack = packs["plain"]
    idx = list(range(len(pack)))
    b = pack.to_device().batch(idx, 0)
    h = _host_batch(pack, idx, 1, True)
    for name in ("bs", "nmax", "emax", "f_in", "j_tot", "dual", "nodes", "edges"):
        assert getattr(b, name) == getattr(h, name), name
    assert torch.equal(b.x.cpu(), h.x) and torch.equal(b.N_batch.cpu(), h.N_batch)
    assert torch.equal(b.E_batch.cpu(), h.E_batch)
    for (r1, e1), (r2, e2) in zip(b.lists(), h.lists()):
        assert np.array_equal(r1, r2) and np.array_equal(e1.view(np.int32), e2.view(np.int32))


@pytest.mark.parametrize("dual", [1, 0])
@pytest.mark.parametrize("J", [1, 2, 3])
def test_counts_equal_host_plan(packs, J, dual):
    from hgnn_amd import _lib as L
    pack = packs["plain"]
    rec = pack.to_device(J=J, dual=bool(dual)).counts
    assert rec.shape == (len(pack), 10) and rec.dtype == np.int32
    for g in range(len(pack)):
        x, a, _ = pack.graph(g)
        lay = L.CsrLayout()
        L.check(L.lib().hgnn_csr_batch_plan(1, (ctypes.c_int * 1)(a.shape[0]), (ctypes.c_void_p * 1)(a.data_ptr()),
                                            x.shape[1], J, dual, ctypes.byref(lay)), "plan")
        assert rec[g].tolist() == [lay.nodes, lay.edges, *lay.nnz, 0, 0], g


def test_large_graphs_fall_back_to_the_host_batcher(tmp_path):
    import hgnn_amd.datagen as dg
    from hgnn_amd.dataset import GraphPack
    big = dg.sbm_dataset(2, n=24, seed=5)
    assert all(int((a != 0).sum()) > 72 for _, a, _ in big)
    pack = GraphPack.write(str(tmp_path / "p"), dg.qm9_shape_dataset(6, seed=9) + big)
    dp = pack.to_device()
    assert (dp.counts[:, 8] == [0] * 6 + [FLAG_BOUNDS] * 2).all()
    for idx in ([0, 6, 3], [7], list(range(8))):
        _assert_same_batch(dp.batch(idx, 1), _host_batch(pack, idx, 1, True, task=1))
    _assert_same_batch(dp.batch([0, 1, 2, 5], 1), _host_batch(pack, [0, 1, 2, 5], 1, True, task=1))


def test_index_error_graph_raises_when_its_batch_is_asked_for(tmp_path):
    import hgnn_amd.datagen as dg
    from hgnn_amd.dataset import GraphPack
    A = torch.zeros(3, 3)
    A[0, 1] = 1.0  # one bond, one edge slot: the reverse slot is column 1 of 1
    bad = (torch.eye(3, 5), A, torch.zeros(13))
    pack = GraphPack.write(str(tmp_path / "p"), dg.qm9_shape_dataset(5, seed=2) + [bad])
    with pytest.raises(IndexError):
        _host_batch(pack, [1, 5], 1, True)
    dp = pack.to_device()
    assert dp.counts[5, 8] == FLAG_INDEX and not dp.counts[:5, 8].any()
    with pytest.raises(IndexError):
        dp.batch([1, 5], 0)
    _assert_same_batch(dp.batch([4, 0, 1], 0), _host_batch(pack, [4, 0, 1], 1, True))
    # without the line graph there are no edge slots: the host builds it, so does the device
    _assert_same_batch(pack.to_device(dual=False).batch([1, 5], 0), _host_batch(pack, [1, 5], 1, False))


def test_j4_takes_the_host_path(packs):
    pack = packs["plain"]
    dp = pack.to_device(J=4)
    assert dp.counts is None
    idx = [0, 1, 50, 2]
    _assert_same_batch(dp.batch(idx, 0), _host_batch(pack, idx, 4, True))


def test_malformed_coo_raises_at_construction(tmp_path):
    import os

    import hgnn_amd.datagen as dg
    from hgnn_amd.dataset import DevicePack, GraphPack
    path = str(tmp_path / "p")
    pack = GraphPack.write(path, dg.qm9_shape_dataset(3, seed=4))
    ij = np.load(os.path.join(path, "adj_ij.npy"))
    a0 = int(pack.adj_off[1])
    ij[[a0, a0 + 1]] = ij[[a0 + 1, a0]]  # graph 1: two entries out of order
    np.save(os.path.join(path, "adj_ij.npy"), ij)
    with pytest.raises(RuntimeError, match="graph 1"):
        DevicePack(GraphPack(path))


@pytest.mark.parametrize("kind", ["lg", "simple"])
def test_network_on_device_built_batch_is_bitwise_the_host_built_one(packs, kind):
    from models.gnns.model_mnb import GNN_lg, GNN_simple
    pack = packs["plain"]
    idx = list(range(24))
    torch.manual_seed(5)
    model = (GNN_lg(0, 16, 2, 5, 1, 1, 2) if kind == "lg" else GNN_simple(0, 16, 2, 5, 1, 1)).cuda()
    twin = copy.deepcopy(model)
    res = []
    for net, b in ((model, _host_batch(pack, idx, 1, kind == "lg", device="cuda")),
                   (twin, pack.to_device(J=1, dual=kind == "lg").batch(idx, 0))):
        b.x.requires_grad_(True)
        out = net.forward_csr(b)
        (out * torch.linspace(-1, 1, out.numel(), device="cuda").view_as(out)).sum().backward()
        res.append((out.detach(), b.x.grad))
    torch.cuda.synchronize()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        assert torch.equal(p.grad, q.grad), n


def test_epochs_from_device_pack_equal_epochs_from_graph_pack(tmp_path):
    import hgnn_amd.datagen as dg
    from hgnn_amd.dataset import GraphPack
    from hgnn_amd.train import TrainStep
    from models.gnns.model_mnb import GNN_lg, GNN_simple
    pack = GraphPack.write(str(tmp_path / "p"), dg.qm9_shape_dataset(64, seed=21))
    dp = pack.to_device()
    torch.manual_seed(9)
    model = GNN_lg(0, 16, 2, 5, 1, 1, 2).cuda()
    twin = copy.deepcopy(model)
    a = TrainStep(model, lr=1e-3, t_mean=0.25, t_std=1.5)
    b = TrainStep(twin, lr=1e-3, t_mean=0.25, t_std=1.5)
    for _ in range(2):
        assert a.train_epoch(dp, 0, 16) == b.train_epoch(pack, 0, 16)
    assert a.step_count == b.step_count == 8
    for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        assert torch.equal(p, q), n
    for s, t in zip(a.exp_avg + a.exp_inf, b.exp_avg + b.exp_inf):
        assert torch.equal(s, t)
    assert a.eval_epoch(dp, 0, 16) == b.eval_epoch(pack, 0, 16)
    # what does not fit is refused
    with pytest.raises(RuntimeError, match="dense"):
        a.eval_epoch(dp, 0, 16, dense=True)
    with pytest.raises(RuntimeError, match="does not match"):
        a.eval_epoch(pack.to_device(J=2), 0, 16)
    with pytest.raises(RuntimeError, match="does not match"):
        TrainStep(GNN_simple(0, 8, 2, 5, 1, 1).cuda(), t_mean=0.25).eval_epoch(dp, 0, 16)


def test_batch_does_not_wait_for_the_stream(packs):
    """batch() only enqueues: with the stream kept busy by earlier work (200 passes over 1 GiB, tens of
    milliseconds), eight builds return and the event recorded after them has not completed; a host
    synchronisation anywhere in batch() would have drained the stream first.  No timing is asserted."""
    pack = packs["plain"]
    dp = pack.to_device()
    idx = list(range(len(pack)))
    want = dp.batch(idx, 0).image.clone()  # also warms the allocators
    busy = torch.zeros(1 << 28, device="cuda")
    torch.cuda.synchronize()
    for _ in range(200):
        busy.add_(1.0)
    built = [dp.batch(idx, 0) for _ in range(8)]
    end = torch.cuda.Event()
    end.record()
    assert not end.query()
    end.synchronize()
    assert end.query()
    for b in built:
        assert torch.equal(b.image, want)
