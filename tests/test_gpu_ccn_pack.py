"""CCN chunks and epochs from a graph pack (csrc/ccn_pack.hip, hgnn_amd.dataset.DevicePack.ccn_chunk,
GraphPack.ccn_chunks, CcnTrainStep.train_epoch / eval_epoch on a pack).

The chunk is data movement plus one exact `+ 1.0f` on the diagonal, so the device-built chunk must be the host-built
one bit for bit, and epochs that run the same kernels on the same bytes must end in the same bits: every comparison
here is torch.equal or == on Python floats."""

import copy
import ctypes

import pytest
import torch

import ccn_pack_util as U
import fixture_util as fu

pytestmark = pytest.mark.gpu

MEAN, STD, LR = 0.3, 1.7, 1e-3
GUARD = 64          # elements behind each output (and one in front of the float outputs: the base is not
SENTINEL = 12345.0  # 16-byte aligned, so the blocks' heads are ragged whatever nmax is)


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    from hgnn_amd.dataset import GraphPack
    root = tmp_path_factory.mktemp("ccn_pack")
    out = {}
    for name, graphs in (("wide", U.graph_set()), ("narrow", U.narrow_set())):
        pack = GraphPack.write(str(root / name), graphs)
        out[name] = {"graphs": graphs, "list": U.instances(graphs), "pack": pack,
                     "ccn": pack.to_device(J=None), "j1": pack.to_device(J=1)}
    return out


def _model(args, seed, two=False):
    from models.compnets.model_ccn import CCN_1D, CCN_2D
    net = (CCN_2D if two else CCN_1D)(*args)
    fu.det_init(net, seed)
    return net.cuda()


def _step(net, **kw):
    from hgnn_amd.train import CcnTrainStep
    if kw.get("classification"):
        return CcnTrainStep(net, lr=LR, **kw)
    return CcnTrainStep(net, lr=LR, t_mean=MEAN, t_std=STD, **kw)


# ------------------------------------------------------------------ 1. the chunk
INDEX_LISTS = {
    "in order": list(range(15)),
    "permuted": [13, 2, 9, 0, 11, 8, 5, 14, 12, 1, 10, 3, 7, 6, 4],
    "with a repeat": [4, 8, 4, 12, 10, 4],
    "without the largest graphs": [0, 8, 10, 3, 9],  # nmax below the pack's 72
    "one node only": [8],
}


@pytest.mark.parametrize("task", U.TASKS)
@pytest.mark.parametrize("which", list(INDEX_LISTS))
def test_chunk_equals_the_host_chunks(sets, which, task):
    s = sets["wide"]
    idx = INDEX_LISTS[which]
    st = _step(_model((5, 1, 2, 2), 3))
    (want,) = [tuple(t.cpu() for t in c) for c in st._chunks([s["list"][i] for i in idx], task, len(idx))]
    U.assert_same_chunk(want, U.reference_chunk([s["graphs"][i] for i in idx], task), "_chunks")
    if which == "without the largest graphs":
        assert want[0].shape[1] <= 29
    (host,) = s["pack"].ccn_chunks(idx, len(idx), task)
    U.assert_same_chunk(host, want, "GraphPack")
    (dev,) = s["pack"].ccn_chunks(idx, len(idx), task, device="cuda")
    assert dev[0].is_cuda
    U.assert_same_chunk(dev, want, "GraphPack on the device")
    for name in ("ccn", "j1"):
        got = s[name].ccn_chunk(idx, task)
        assert all(t.is_cuda and t.is_contiguous() for t in got)
        U.assert_same_chunk(got, want, name)
        s[name].check()


def test_chunk_with_three_features(sets):
    s = sets["narrow"]
    idx = [4, 0, 3, 1, 2]
    st = _step(_model((3, 1, 2, 2), 3))
    (want,) = [tuple(t.cpu() for t in c) for c in st._chunks([s["list"][i] for i in idx], 7, len(idx))]
    for name in ("ccn", "j1"):
        U.assert_same_chunk(s[name].ccn_chunk(idx, 7), want, name)
    (host,) = s["pack"].ccn_chunks(idx, len(idx), 7)
    U.assert_same_chunk(host, want, "GraphPack")


@pytest.mark.parametrize("nmax", [30, 32, 41])
def test_chunk_padded_further(sets, nmax):
    s = sets["wide"]
    idx = [0, 8, 10, 3, 9, 12]
    want = U.reference_chunk([s["graphs"][i] for i in idx], 7, nmax=nmax)
    U.assert_same_chunk(s["ccn"].ccn_chunk(idx, 7, nmax=nmax), want)
    with pytest.raises(RuntimeError, match="nmax"):
        s["ccn"].ccn_chunk(idx, 7, nmax=want[2].max().item() - 1)


def test_chunks_in_pieces(sets):
    s = sets["wide"]
    got = list(s["ccn"].ccn_chunks(range(15), 4, 0))
    want = list(s["pack"].ccn_chunks(range(15), 4, 0))
    assert [c[0].shape[0] for c in got] == [4, 4, 4, 3] and [c[0].shape[1] for c in got][-1] == 72
    for g, w in zip(got, want):
        U.assert_same_chunk(g, w)


# ------------------------------------------------------------------ 2. the ABI's contract
class _Guarded:
    """One output of `count` elements filled with `fill`, a sentinel element in front (float outputs) and GUARD
    behind."""

    def __init__(self, count, dtype, fill):
        self.front = 1 if dtype == torch.float32 else 0
        self.count = count
        self.buf = torch.full((self.front + count + GUARD,), SENTINEL, dtype=dtype, device="cuda")
        self.body = self.buf[self.front:self.front + count]
        self.body.fill_(fill)

    def ptr(self):
        return ctypes.c_void_p(self.body.data_ptr())

    def guards_intact(self):
        g = torch.cat([self.buf[:self.front], self.buf[self.front + self.count:]])
        return bool((g == SENTINEL).all())


def _raw_chunk(dp, view, idx, nmax, task, err):
    """hgnn_pack_ccn_chunk through ctypes into NaN / -1 filled, guarded outputs."""
    from hgnn_amd import _lib as L
    G, f = len(idx), dp.f_in
    out = [_Guarded(G * nmax * f, torch.float32, float("nan")), _Guarded(G * nmax * nmax, torch.float32, float("nan")),
           _Guarded(G, torch.int64, -1), _Guarded(G, torch.float32, float("nan"))]
    d_idx = torch.tensor(idx, dtype=torch.int32, device="cuda")
    st = L.lib().hgnn_pack_ccn_chunk(ctypes.byref(view), dp.n_targets, L.ptr(d_idx), G, nmax, task,
                                     *[o.ptr() for o in out], L.ptr(err), L.stream_handle(dp.device))
    assert st == 0
    torch.cuda.synchronize()
    for o, name in zip(out, ("X", "adj", "n_batch", "y")):
        assert o.guards_intact(), f"{name}: written outside the output"
    X, A, nb, y = [o.body.cpu() for o in out]
    assert not torch.isnan(X).any() and not torch.isnan(A).any() and not torch.isnan(y).any()
    assert (nb >= 0).all()
    return X.view(G, nmax, f), A.view(G, nmax, nmax), nb, y.view(G, 1)


def _assert_slots(got, want, empty):
    """The slots in `empty` are all zero with n_batch = 0 and y = 0; every other slot is the reference's."""
    for b in range(got[0].shape[0]):
        for g, w in zip(got, want):
            if b in empty:
                assert not g[b].any(), f"slot {b} is not empty"
            else:
                assert torch.equal(g[b], w[b]), f"slot {b} differs"


@pytest.mark.parametrize("name,nmax", [("wide", 29), ("wide", 40), ("wide", 75), ("narrow", 0)])
def test_every_element_is_written_and_nothing_else(sets, name, nmax):
    s = sets[name]
    dp = s["ccn"]
    idx = [i for i in range(len(dp)) if nmax == 0 or s["graphs"][i][0].shape[0] <= nmax]
    nmax = nmax or max(s["graphs"][i][0].shape[0] for i in idx)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = _raw_chunk(dp, dp._view, idx, nmax, 7, err)
    U.assert_same_chunk(got, U.reference_chunk([s["graphs"][i] for i in idx], 7, nmax=nmax))
    assert err.item() == 0


def test_bad_index_gives_an_empty_slot(sets):
    s = sets["wide"]
    dp = s["ccn"]
    idx = [3, len(dp), 8, -1, 10, 1 << 30]
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = _raw_chunk(dp, dp._view, idx, 29, 0, err)
    want = U.reference_chunk([s["graphs"][i if 0 <= i < len(dp) else 0] for i in idx], 0, nmax=29)
    _assert_slots(got, want, {1, 3, 5})
    assert err.item() == 1


def test_graph_above_nmax_gives_an_empty_slot(sets):
    s = sets["wide"]
    dp = s["ccn"]
    idx = [8, 13, 0, 10, 14]
    n0 = s["graphs"][0][0].shape[0]
    nmax = max(n0, s["graphs"][10][0].shape[0])
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = _raw_chunk(dp, dp._view, idx, nmax, 7, err)
    want = U.reference_chunk([s["graphs"][i if i < 13 else 8] for i in idx], 7, nmax=nmax)
    _assert_slots(got, want, {1, 4})
    assert err.item() == 1
    # the error word may be null
    assert _raw_chunk(dp, dp._view, idx, nmax, 7, None)[2].tolist() == got[2].tolist()


def test_coo_corrupted_on_the_device_gives_empty_slots(sets):
    from hgnn_amd import _lib as L
    from hgnn_amd.dataset import GraphPack
    s = sets["wide"]
    pack, dp = s["pack"], s["ccn"]
    ij = dp._arrays["adj_ij"].clone()
    a2, a5, a9 = (int(pack.adj_off[g]) for g in (2, 5, 9))
    ij[a2 + 4, 1] = s["graphs"][2][0].shape[0]  # graph 2: a column index == n (inside the padded row, outside the graph)
    ij[a5 + 1], ij[a5 + 2] = ij[a5 + 2].clone(), ij[a5 + 1].clone()  # graph 5: two entries swapped
    ij[a9, 0] = -3  # graph 9: a negative row
    ptrs = {k: dp._arrays[k].data_ptr() for k in GraphPack.FILES}
    ptrs["adj_ij"] = ij.data_ptr()
    view = L.PackView(*[ptrs[k] for k in GraphPack.FILES], len(pack), dp.f_in, 0)
    idx = list(range(13))
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = _raw_chunk(dp, view, idx, 29, 0, err)
    _assert_slots(got, U.reference_chunk(s["graphs"][:13], 0, nmax=29), {2, 5, 9})
    assert err.item() == 1


def test_check_raises_after_an_empty_slot(tmp_path):
    from hgnn_amd.dataset import GraphPack
    graphs = U.graph_set()[:4]
    dp = GraphPack.write(str(tmp_path / "p"), graphs).to_device(J=None)
    dp.ccn_chunk([0, 1, 2, 3], 0)
    dp.check()
    keep = dp._arrays["adj_ij"].clone()
    dp._arrays["adj_ij"][int(dp.pack.adj_off[1]), 0] = 1000  # the device copy goes bad after construction
    got = dp.ccn_chunk([0, 1, 2, 3], 0)
    _assert_slots([t.cpu() for t in got], U.reference_chunk(graphs, 0), {1})
    with pytest.raises(RuntimeError, match="left a graph out"):
        dp.check()
    dp._arrays["adj_ij"].copy_(keep)
    U.assert_same_chunk(dp.ccn_chunk([0, 1, 2, 3], 0), U.reference_chunk(graphs, 0))
    dp.check()  # the word was cleared by the check that raised


def test_host_detectable_misuse_is_an_argument_error(sets):
    from hgnn_amd import _lib as L
    dp = sets["wide"]["ccn"]
    G, nmax = 2, 29
    X = torch.zeros(G, nmax, 5, device="cuda")
    A = torch.zeros(G, nmax, nmax, device="cuda")
    nb = torch.zeros(G, dtype=torch.int64, device="cuda")
    y = torch.zeros(G, 1, device="cuda")
    idx = torch.zeros(G, dtype=torch.int32, device="cuda")
    stream = L.stream_handle(dp.device)
    fn = L.lib().hgnn_pack_ccn_chunk
    good = [ctypes.byref(dp._view), dp.n_targets, L.ptr(idx), G, nmax, 0, L.ptr(X), L.ptr(A), L.ptr(nb), L.ptr(y),
            None, stream]
    assert fn(*good) == 0
    for pos, value in [(0, None), (2, None), (6, None), (7, None), (8, None), (9, None), (3, 0), (3, -1), (4, 0),
                       (4, -5), (5, -1), (5, dp.n_targets), (1, 0)]:
        args = list(good)
        args[pos] = value
        assert fn(*args) == 1, (pos, value)
    for member in ("d_node_off", "d_x", "d_adj_off", "d_adj_ij", "d_adj_w", "d_targets"):
        view = L.PackView.from_buffer_copy(dp._view)
        setattr(view, member, None)
        assert fn(ctypes.byref(view), *good[1:]) == 1, member
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 3. epochs
def _state(st):
    return [p.detach().clone() for p in st.params] + [t.clone() for t in st.exp_avg + st.exp_inf]


def _epochs(make_step, data, chunk, paths=None):
    """Two training epochs and one evaluation from a fresh copy of the model; with `paths`, the route of every
    chunk of the first epoch."""
    st = make_step()
    if paths is not None:
        step = st.step

        def recording(*a):
            r = step(*a)
            paths.append(st.path)
            return r
        st.step = recording
    res = [st.train_epoch(data, 0, chunk=chunk)]
    if paths is not None:
        st.step = step
    res.append(st.train_epoch(data, 0, chunk=chunk))
    stats = st.stats.clone()
    res.append(st.eval_epoch(data, 0, chunk=chunk))
    return res, stats, _state(st), st.step_count


def _assert_epochs_agree(make_step, legs, chunk, want_paths):
    runs = {}
    for name, data in legs.items():
        paths = []
        runs[name] = _epochs(make_step, data, chunk, paths)
        assert paths == want_paths, (name, paths)
    res, stats, state, count = runs["list"]
    assert count == 2 * len(legs["list"])
    for name in ("device pack", "graph pack"):
        r, s, t, c = runs[name]
        assert r == res, (name, r, res)
        assert torch.equal(s, stats), name
        assert c == count and len(t) == len(state)
        for i, (x, y) in enumerate(zip(t, state)):
            assert torch.equal(x, y), f"{name}: parameter / optimizer tensor {i} differs"
    return res


def _legs(s):
    return {"list": s["list"], "device pack": s["ccn"], "graph pack": s["pack"]}


@pytest.fixture(scope="module")
def qm9(sets, tmp_path_factory):
    """The eight QM9-shape graphs as a list and as packs of their own."""
    from hgnn_amd.dataset import GraphPack
    graphs = sets["wide"]["graphs"][:8]
    pack = GraphPack.write(str(tmp_path_factory.mktemp("ccn_pack_qm9") / "p"), graphs)
    return {"list": U.instances(graphs), "device pack": pack.to_device(J=None), "graph pack": pack}


def test_epochs_ccn1d_fused(qm9):
    net = _model((5, 1, 2, 2), 11)
    res = _assert_epochs_agree(lambda: _step(copy.deepcopy(net), fused=True), qm9, 1024, ["fused"])
    assert all(v == v and v != 0.0 for pair in res for v in pair)


def test_epochs_ccn2d_fused2d(qm9):
    net = _model((5, 1, 2, 2), 12, two=True)
    _assert_epochs_agree(lambda: _step(copy.deepcopy(net), fused="ccn2"), qm9, 1024, ["fused2d"])


def test_epochs_whole_set_in_chunks_of_four(sets):
    """Chunks of 4 over the 15 graphs: the last chunk holds the 40-node and the 72-node graph; padded to 72 nodes
    it is above the fused kernel's bound and takes the unfused route."""
    net = _model((5, 1, 2, 2), 13)
    _assert_epochs_agree(lambda: _step(copy.deepcopy(net)), _legs(sets["wide"]), 4,
                         ["fused", "fused", "fused", "unfused"])


def test_epochs_from_a_pack_built_for_the_gnns(sets):
    """A DevicePack with a J offers the same CCN epochs."""
    s = sets["wide"]
    net = _model((5, 1, 2, 2), 13)
    a = _epochs(lambda: _step(copy.deepcopy(net)), s["ccn"], 4)
    b = _epochs(lambda: _step(copy.deepcopy(net)), s["j1"], 4)
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def test_epochs_classification(tmp_path):
    import hgnn_amd.datagen as dg
    from hgnn_amd.dataset import GraphPack
    data = dg.three_collinear_points(12, n_max=16, seed=11)
    assert {int(d[2][0]) for d in data} == {0, 1}
    pack = GraphPack.write(str(tmp_path / "p"), data)
    legs = {"list": data, "device pack": pack.to_device(J=None), "graph pack": pack}
    net = _model((5, 2, 2, 2), 14)
    res = _assert_epochs_agree(lambda: _step(copy.deepcopy(net), classification=True), legs, 5,
                               ["fused", "fused", "fused"])
    assert res[0][1] == 0.0 and res[1][1] == 0.0  # error.val as the reference's untouched meter leaves it


# ------------------------------------------------------------------ 4. misuse
def test_device_pack_on_another_device_is_refused(sets):
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible device")
    dp = sets["wide"]["pack"].to_device(J=None, device="cuda:1")
    st = _step(_model((5, 1, 2, 2), 3))
    with pytest.raises(RuntimeError, match="DevicePack on cuda:1"):
        st.train_epoch(dp, 0)
    with pytest.raises(RuntimeError, match="DevicePack on cuda:1"):
        st.eval_epoch(dp, 0)


def test_ccn_only_pack_builds_no_csr_batches(sets):
    dp = sets["wide"]["ccn"]
    assert dp.J is None and dp.counts is None
    with pytest.raises(RuntimeError, match="CCN only"):
        dp.batch([0, 1], 0)
    with pytest.raises(RuntimeError, match="CCN only"):
        next(dp.batches([0, 1], 2, 0))
    with pytest.raises(IndexError):
        dp.ccn_chunk([0, 15], 0)
    with pytest.raises(RuntimeError):
        dp.ccn_chunk([0, 1], 13)  # task outside the 13 targets


def test_malformed_coo_raises_at_construction_without_a_count(tmp_path):
    import os

    import numpy as np

    from hgnn_amd.dataset import DevicePack, GraphPack
    path = str(tmp_path / "p")
    pack = GraphPack.write(path, U.graph_set()[:3])
    ij = np.load(os.path.join(path, "adj_ij.npy"))
    a0 = int(pack.adj_off[1])
    ij[[a0, a0 + 1]] = ij[[a0 + 1, a0]]
    np.save(os.path.join(path, "adj_ij.npy"), ij)
    msgs = []
    for J in (None, 1):
        with pytest.raises(RuntimeError, match="graph 1") as e:
            DevicePack(GraphPack(path), J=J)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]


def test_packs_do_not_go_through_the_list_path(sets, monkeypatch):
    """_chunks indexes a list of 7-tuples; a pack handed to it fails there (as every pack did before packs were
    taken).  Packs are routed past it, lists still go through it."""
    from hgnn_amd.train import CcnTrainStep
    s = sets["wide"]
    st = _step(_model((5, 1, 2, 2), 3))
    with pytest.raises(Exception):
        next(st._chunks(s["pack"], 0, 4))
    calls = []
    inner = CcnTrainStep._chunks

    def counted(self, data, task, chunk):
        calls.append(type(data).__name__)
        return inner(self, data, task, chunk)
    monkeypatch.setattr(CcnTrainStep, "_chunks", counted)
    st.train_epoch(s["pack"], 0, chunk=4)
    st.eval_epoch(s["ccn"], 0, chunk=4)
    assert calls == []
    st.eval_epoch(s["list"], 0, chunk=4)
    assert calls == ["list"]
