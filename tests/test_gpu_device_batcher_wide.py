"""The device batcher on node-graph batches of up to 64 nodes (csrc/batcher.hip, the BtWide instantiation;
hgnn_amd.dataset.DevicePack with dual=False) against the host batcher (csrc/builder.cpp), byte for byte, on the wide
pack of tests/device_batcher_wide_util.py.  No tolerance anywhere: torch.equal on the raw image bytes or on what
the executor computes from them."""

import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import device_batcher_wide_util as U

pytestmark = pytest.mark.gpu

FLAG_BOUNDS = 1


@pytest.fixture(scope="module")
def packs(tmp_path_factory):
    from hgnn_amd.dataset import GraphPack
    root = tmp_path_factory.mktemp("device_batcher_wide")
    gs = U.wide_graphs()
    return {"plain": GraphPack.write(str(root / "plain"), gs),
            "real": GraphPack.write(str(root / "real"), U.real_weights(gs)),
            "small": GraphPack.write(str(root / "small"), [gs[i] for i in U.small_indices(gs)]),
            "graphs": gs, "root": root}


def _no_host_batches(monkeypatch, pack):
    def refuse(*a, **k):
        raise AssertionError("the host batcher was asked for a batch the device should build")
    monkeypatch.setattr(pack, "batches", refuse)


def _check_all_lists(pack, J, monkeypatch, task):
    dp = pack.to_device(J=J, dual=False)
    assert not dp.counts[:, 8].any()  # on the parent commit every graph past 32 nodes is flagged here
    want = {tuple(idx): U.host_batch(pack, idx, J, task=task) for idx in U.index_lists(len(pack))}
    _no_host_batches(monkeypatch, pack)
    for idx, host in want.items():
        b = dp.batch(list(idx), task)
        U.assert_same_batch(b, host)
        assert b.image.is_cuda and b.bs == len(idx)


@pytest.mark.parametrize("J", [1, 2, 3])
def test_no_flags_and_image_equals_host_image(packs, J, monkeypatch):
    _check_all_lists(packs["plain"], J, monkeypatch, task=2)


def test_image_equals_host_image_real_weights(packs, monkeypatch):
    """Weights that are not dyadic, 64-term fp64 sums: the order of summation, the separate multiply and add and the
    one rounding per squaring all show in the bits."""
    _check_all_lists(packs["real"], 3, monkeypatch, task=0)


@pytest.mark.parametrize("J", [1, 2, 3])
def test_counts_equal_host_plan(packs, J):
    from hgnn_amd import _lib as L
    pack = packs["plain"]
    rec = pack.to_device(J=J, dual=False).counts
    assert rec.shape == (len(pack), 10) and rec.dtype == np.int32
    for g in range(len(pack)):
        x, a, _ = pack.graph(g)
        lay = L.CsrLayout()
        L.check(L.lib().hgnn_csr_batch_plan(1, (ctypes.c_int * 1)(a.shape[0]), (ctypes.c_void_p * 1)(a.data_ptr()),
                                            x.shape[1], J, 0, ctypes.byref(lay)), "plan")
        assert rec[g].tolist() == [lay.nodes, 0, lay.nnz[0], lay.nnz[1], 0, 0, 0, 0, 0, 0], g
        assert lay.edges == 0 and list(lay.nnz[2:]) == [0, 0, 0, 0]


@pytest.mark.parametrize("J", [1, 3])
def test_small_only_batches_take_the_narrow_kernel(packs, J, monkeypatch):
    """nmax <= 32: the narrow kernel builds from records the wide count pass wrote.  The image is the host's, and the
    one a DevicePack of only those graphs builds."""
    pack, small_pack = packs["plain"], packs["small"]
    small = U.small_indices(packs["graphs"])
    dp, dps = pack.to_device(J=J, dual=False), small_pack.to_device(J=J, dual=False)
    assert np.array_equal(dp.counts[small], dps.counts)
    lists = [list(range(len(small))), list(range(len(small)))[::-1], [2, 2, 3, 0, 7, 2], [3]]
    want = [U.host_batch(small_pack, loc, J, task=1) for loc in lists]
    _no_host_batches(monkeypatch, pack)
    _no_host_batches(monkeypatch, small_pack)
    for loc, host in zip(lists, want):
        b = dp.batch([small[i] for i in loc], 1)
        assert b.nmax <= 32
        U.assert_same_batch(b, host)
        s = dps.batch(loc, 1)
        assert bytes(s.layout) == bytes(b.layout) and torch.equal(s.image, b.image)


def test_bounds(packs, tmp_path, monkeypatch):
    from hgnn_amd.dataset import GraphPack
    gs = packs["graphs"]
    big = U.hand_graph(65, [(i, i + 1) for i in range(64)])
    part = [gs[U.INDEX["sbm"][0]], big, gs[U.INDEX["k33"]], gs[U.INDEX["qm9"][0]], gs[U.INDEX["k64"]]]
    pack = GraphPack.write(str(tmp_path / "p"), part)
    dp = pack.to_device(J=2, dual=False)
    assert dp.counts[:, 8].tolist() == [0, FLAG_BOUNDS, 0, 0, 0]
    assert dp.counts[1, :8].tolist() == [65, 0, 0, 0, 0, 0, 0, 0]
    for idx in ([0, 1, 2], [1], list(range(5))):  # through the host path
        U.assert_same_batch(dp.batch(idx, 1), U.host_batch(pack, idx, 2, task=1))
    # with the line graph the bounds are what they were: n <= 32 and m <= 72
    dual = pack.to_device(J=1, dual=True)
    assert dual.counts[:, 8].tolist() == [FLAG_BOUNDS] * 3 + [0, FLAG_BOUNDS]
    wide_dual = packs["plain"].to_device(J=1, dual=True)
    n = np.array([x.shape[0] for x, _, _ in gs])
    assert (wide_dual.counts[n > 32, 8] == FLAG_BOUNDS).all()
    want = U.host_batch(pack, [0, 2, 3, 4], 2, task=1)
    _no_host_batches(monkeypatch, pack)
    U.assert_same_batch(dp.batch([0, 2, 3, 4], 1), want)


@pytest.mark.parametrize("kind", ["index", "order"])
def test_malformed_coo_at_50_nodes_raises_at_construction(tmp_path, kind):
    import hgnn_amd.datagen as dg
    from hgnn_amd.dataset import DevicePack, GraphPack
    path = str(tmp_path / "p")
    pack = GraphPack.write(path, dg.sbm_dataset(3, n=50, seed=5))
    ij = np.load(os.path.join(path, "adj_ij.npy"))
    a0 = int(pack.adj_off[1])
    if kind == "index":
        ij[a0 + 200, 1] = 50  # graph 1: a column index == n
    else:
        ij[[a0 + 200, a0 + 201]] = ij[[a0 + 201, a0 + 200]]  # graph 1: two entries out of order
    np.save(os.path.join(path, "adj_ij.npy"), ij)
    with pytest.raises(RuntimeError, match="graph 1"):
        DevicePack(GraphPack(path), J=1, dual=False)


def _build_into(dp, rec_idx, d_idx_list, J, pad=4096, fill=0xA5):
    """hgnn_csr_batch_build_device with the layout of the graphs `rec_idx` and the indices `d_idx_list`, into an
    image in the middle of a buffer of sentinel bytes.  Returns (layout, the whole buffer on the host, pad)."""
    from hgnn_amd import _lib as L
    lib = L.lib()
    bs = len(rec_idx)
    rec = np.ascontiguousarray(dp.counts[np.asarray(rec_idx, dtype=np.int64)])
    lay = L.CsrLayout()
    L.check(lib.hgnn_csr_layout_from_counts(bs, ctypes.c_void_p(rec.ctypes.data), dp.f_in, J, 0, ctypes.byref(lay)),
            "layout")
    nbytes = int(lay.bytes)
    buf = torch.full((pad + nbytes + pad,), fill, dtype=torch.uint8, device="cuda")
    d_idx = torch.tensor(d_idx_list, dtype=torch.int32, device="cuda")
    scratch = torch.empty(lib.hgnn_csr_batch_build_device_scratch_bytes(bs), dtype=torch.uint8, device="cuda")
    L.check(lib.hgnn_csr_batch_build_device(ctypes.byref(dp._view), L.ptr(dp._counts), L.ptr(d_idx), bs, J, 0,
                                            ctypes.byref(lay), ctypes.c_void_p(buf.data_ptr() + pad), L.ptr(scratch),
                                            scratch.numel(), L.stream_handle(dp.device)), "build")
    torch.cuda.synchronize()
    return lay, buf.cpu(), pad


def test_nothing_is_written_outside_the_image(packs):
    pack = packs["plain"]
    dp = pack.to_device(J=3, dual=False)
    idx = [U.INDEX["k64"], U.INDEX["sbm"][0], U.INDEX["single"]]
    lay, buf, pad = _build_into(dp, idx, idx, 3)
    nbytes = int(lay.bytes)
    host = U.host_batch(pack, idx, 3)
    assert bytes(lay) == bytes(host.layout)
    assert torch.equal(buf[pad:pad + nbytes], host.host)
    assert (buf[:pad] == 0xA5).all() and (buf[pad + nbytes:] == 0xA5).all()
    # indices whose records do not add up to the layout: zeros and the offset fields only
    other = [U.INDEX["k33"], U.INDEX["sbm"][1], U.INDEX["path64"]]
    lay2, buf, pad = _build_into(dp, idx, other, 3)
    assert bytes(lay2) == bytes(lay)
    assert (buf[:pad] == 0xA5).all() and (buf[pad + nbytes:] == 0xA5).all()
    img = buf[pad:pad + nbytes]
    assert not img[int(lay.off_x):].any()  # x, rows and entries: nothing but the memset
    node_off = img[int(lay.off_node_off):int(lay.off_node_off) + 16].numpy().view(np.int32)
    assert node_off.tolist() == [0, 33, 83, 147]  # the offsets of the graphs d_idx names


def _small_and_sbm(packs):
    return U.INDEX["sbm"] + U.small_indices(packs["graphs"])


@pytest.mark.parametrize("args", [(0, 16, 2, 5, 1, 1), (0, 2, 3, 5, 2, 1)])  # the second: two output columns
def test_network_on_device_built_batch_is_bitwise_the_host_built_one(packs, args):
    from models.gnns.model_mnb import GNN_simple
    pack = packs["plain"]
    idx = _small_and_sbm(packs)
    torch.manual_seed(5)
    model = GNN_simple(*args).cuda()
    J = model.J
    twin = copy.deepcopy(model)
    res = []
    for net, b in ((model, U.host_batch(pack, idx, J, device="cuda")),
                   (twin, pack.to_device(J=J, dual=False).batch(idx, 0))):
        b.x.requires_grad_(True)
        out = net.forward_csr(b)
        (out * torch.linspace(-1, 1, out.numel(), device="cuda").view_as(out)).sum().backward()
        res.append((out.detach(), b.x.grad))
    torch.cuda.synchronize()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        assert torch.equal(p.grad, q.grad), n


def test_epochs_from_device_pack_equal_epochs_from_graph_pack(tmp_path, monkeypatch):
    import hgnn_amd.datagen as dg
    from hgnn_amd.dataset import GraphPack
    from hgnn_amd.train import TrainStep
    from models.gnns.model_mnb import GNN_simple
    pack = GraphPack.write(str(tmp_path / "p"), dg.sbm_dataset(24, n=50, seed=21))
    dp = pack.to_device(J=1, dual=False)
    assert not dp.counts[:, 8].any()
    torch.manual_seed(9)
    model = GNN_simple(0, 2, 3, 5, 1, 1).cuda()
    twin = copy.deepcopy(model)
    a = TrainStep(model, lr=1e-3, t_mean=0.25, t_std=1.5)
    b = TrainStep(twin, lr=1e-3, t_mean=0.25, t_std=1.5)
    host = [b.train_epoch(pack, 0, 8) for _ in range(2)] + [b.eval_epoch(pack, 0, 8)]
    _no_host_batches(monkeypatch, pack)
    assert [a.train_epoch(dp, 0, 8) for _ in range(2)] == host[:2]
    assert a.step_count == b.step_count == 6
    for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        assert torch.equal(p, q), n
    for s, t in zip(a.exp_avg + a.exp_inf, b.exp_avg + b.exp_inf):
        assert torch.equal(s, t)
    assert a.eval_epoch(dp, 0, 8) == host[2]
