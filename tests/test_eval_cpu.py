"""Host-only checks of the GNN evaluation path: the entry points hgnn_eval_loss / hgnn_eval_xent (every call here
returns from its argument checks, before any launch), TrainStep.eval_result's arithmetic, the batch order of
eval_epoch / train_epoch (test_with_mnb / train_with_mnb, scripts/test_mnb.py:36, scripts/train_mnb.py:38:
get_batches(n, bs, data, False, False)) and hgnn_amd.dp.sum_meters over gloo."""

import ctypes
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 1


def _lib():
    from hgnn_amd import _lib
    return _lib.lib()


def _word():
    """A non-null pointer that a refused call never dereferences."""
    buf = (ctypes.c_double * 8)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_entries_are_bound_and_exported():
    from hgnn_amd import _lib
    for name in ("hgnn_eval_loss", "hgnn_eval_xent"):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().hgnn_abi_version() == 1


def test_eval_loss_argument_checks():
    lib = _lib()
    _, w = _word()
    assert lib.hgnn_eval_loss(None, w, 4, 1, 0.3, 1.7, w, None) == ARG
    assert lib.hgnn_eval_loss(w, None, 4, 1, 0.3, 1.7, w, None) == ARG
    assert lib.hgnn_eval_loss(w, w, 4, 1, 0.3, 1.7, None, None) == ARG
    assert lib.hgnn_eval_loss(w, w, -1, 1, 0.3, 1.7, w, None) == ARG
    assert lib.hgnn_eval_loss(w, w, 4, 0, 0.3, 1.7, w, None) == ARG
    assert lib.hgnn_eval_loss(w, w, 4, -3, 0.3, 1.7, w, None) == ARG
    # rows * dim_out >= 2^31
    assert lib.hgnn_eval_loss(w, w, 1 << 30, 2, 0.3, 1.7, w, None) == ARG
    assert lib.hgnn_eval_loss(w, w, 65536, 32768, 0.3, 1.7, w, None) == ARG
    # the argument checks come before the empty-batch return
    assert lib.hgnn_eval_loss(None, w, 0, 1, 0.3, 1.7, w, None) == ARG
    assert lib.hgnn_eval_loss(w, w, 0, 0, 0.3, 1.7, w, None) == ARG


def test_eval_xent_argument_checks():
    lib = _lib()
    _, w = _word()
    assert lib.hgnn_eval_xent(None, w, 4, 3, w, w, None) == ARG
    assert lib.hgnn_eval_xent(w, None, 4, 3, w, w, None) == ARG
    assert lib.hgnn_eval_xent(w, w, 4, 3, None, w, None) == ARG
    assert lib.hgnn_eval_xent(w, w, 4, 3, w, None, None) == ARG
    assert lib.hgnn_eval_xent(w, w, -1, 3, w, w, None) == ARG
    assert lib.hgnn_eval_xent(w, w, 4, 0, w, w, None) == ARG
    assert lib.hgnn_eval_xent(w, w, 1 << 30, 2, w, w, None) == ARG
    assert lib.hgnn_eval_xent(w, w, 0, 0, w, w, None) == ARG


def test_rows_zero_is_ok_and_writes_nothing():
    lib = _lib()
    buf, w = _word()
    for i in range(8):
        buf[i] = 1.5 + i
    assert lib.hgnn_eval_loss(w, w, 0, 1, 0.3, 1.7, w, None) == 0
    assert lib.hgnn_eval_loss(w, w, 0, 1 << 30, 0.3, 1.7, w, None) == 0
    assert lib.hgnn_eval_xent(w, w, 0, 3, w, w, None) == 0
    assert [buf[i] for i in range(8)] == [1.5 + i for i in range(8)]


def _bare_step(model=None, classification=False):
    """A TrainStep without a device: only what eval_result and the epoch loops read."""
    from hgnn_amd.train import TrainStep
    s = TrainStep.__new__(TrainStep)
    s.model = model
    s.params = [] if model is None else list(model.parameters())
    s.classification = classification
    s.eval_meters = torch.zeros(6, dtype=torch.float64)
    s.stats = torch.zeros(4)
    return s


def test_eval_result_arithmetic():
    s = _bare_step()
    assert s.eval_result() == (0.0, 0.0)  # zero count: AverageMeter's initial state
    s.eval_meters.copy_(torch.tensor([0.1 * 24 + 0.7 * 7, 3.5, 31.0, 0.0, 0.7, 0.2], dtype=torch.float64))
    loss, err = s.eval_result()
    assert loss == (0.1 * 24 + 0.7 * 7) / 31.0 and err == 3.5 / 31.0  # Python doubles, sum / count
    with pytest.raises(RuntimeError, match="classification"):
        s.eval_result(accuracy=True)
    c = _bare_step(classification=True)
    assert c.eval_result() == (0.0, 0.0)
    assert c.eval_result(accuracy=True) == (0.0, 0.0, 0.0)
    c.eval_meters.copy_(torch.tensor([20.5, 99.0, 31.0, 17.0, 0.4, 99.0], dtype=torch.float64))
    assert c.eval_result() == (20.5 / 31.0, 0.0)  # error.avg is never updated on this branch
    assert c.eval_result(accuracy=True) == (20.5 / 31.0, 0.0, 17.0 / 31.0)
    assert c.eval_meters.tolist() == [20.5, 99.0, 31.0, 17.0, 0.4, 99.0]  # a read, not a reset


@pytest.mark.parametrize("source", ["list", "pack"])
def test_epoch_loops_take_batches_in_list_order(source, tmp_path, monkeypatch):
    """55 instances at bs 24: batches of 24, 24, 7 holding the instances in list order, for evaluate and for the
    training step."""
    import hgnn_amd.datagen as dg
    from hgnn_amd.dataset import GraphPack
    from hgnn_amd.train import TrainStep
    from models.gnns.model_mnb import GNN_lg
    graphs = dg.qm9_shape_dataset(55, seed=77)
    data = [[x, a, t] for x, a, t in graphs]
    if source == "pack":
        data = GraphPack.write(str(tmp_path / "pack"), data)
    s = _bare_step(GNN_lg(0, 8, 3, 5, 1, 1, 2))
    seen = []

    def record(self, batch):
        seen.append((batch.bs, batch.dual, batch.N_batch.tolist(), batch.T.view(-1).tolist()))
        return self.eval_meters

    monkeypatch.setattr(TrainStep, "evaluate", record)
    monkeypatch.setattr(TrainStep, "__call__", record)
    nodes = [int(x.shape[0]) for x, _, _ in graphs]
    targets = [float(t[3]) for _, _, t in graphs]
    for run in (lambda: s.eval_epoch(data, 3, 24), lambda: s.train_epoch(data, 3, 24)):
        del seen[:]
        res = run()
        assert res == (0.0, 0.0)  # nothing was accumulated by the stub
        assert [b[0] for b in seen] == [24, 24, 7]
        assert all(b[1] for b in seen)
        assert sum((b[2] for b in seen), []) == nodes
        assert sum((b[3] for b in seen), []) == targets


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_meters(rank):
    return torch.tensor([3.0 + rank, 10.0 * (rank + 1), 31.0 + 24 * rank, 5.0 + 2 * rank, 0.25 + rank, 0.5 + rank],
                        dtype=torch.float64)


def _meters_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys
    sys.path.insert(0, os.path.join(REPO, "hgnn-2_amd"))
    from hgnn_amd.dp import sum_meters
    m = _rank_meters(rank)
    out = sum_meters(m)
    q.put((rank, out.numpy().copy(), m.numpy().copy()))  # numpy copies: pickled by value
    dist.barrier()
    dist.destroy_process_group()


def test_sum_meters_gloo_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_meters_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    got = [q.get(timeout=300) for _ in range(2)]
    for pr in procs:
        pr.join(timeout=120)
        assert pr.exitcode == 0
    want = (_rank_meters(0) + _rank_meters(1))[:4].tolist()
    assert sorted(g[0] for g in got) == [0, 1]
    for rank, out, own in got:
        assert out[:4].tolist() == want  # integers: exact sums
        assert out[4:].tolist() == _rank_meters(rank)[4:].tolist()  # the last batch's values stay the rank's own
        assert own.tolist() == _rank_meters(rank).tolist()  # the argument is not written


def test_sum_meters_without_a_group_is_the_identity():
    from hgnn_amd.dp import sum_meters
    assert not dist.is_initialized()
    m = _rank_meters(1)
    out = sum_meters(m)
    assert out.dtype == torch.float64 and out.tolist() == m.tolist()
    assert out.data_ptr() != m.data_ptr()
