"""The executor's launch sequence and the kernel timer (csrc/net.hip walks, csrc/timer.h).

One training step under a KernelTimer in stamp mode gives every stamped launch's class and stream in enqueue
order; in dispatch mode, the launch count of every class.  Both are deterministic for a configuration (the
streams are numbered by first appearance), so they are compared with literals.

The literals are what the library of commit b943851 (the parent of the executor's split into program / timer /
replay / net) produced, printed by `python tests/test_gpu_launch_order.py` with HGNN_LIB_PATH pointing at that
build.  A change of the launch sequence must change them on purpose.
"""

import os
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# graphs of 5-9 nodes.  A: 2d = 64, the split-bf16 GEMMs, 4 halves; X and W require grad: the side stream's dense
# dW with its own dA slots, the readout-row path with its dW on the side stream, the early fork of the last half.
# B: no input gradients: layer 0's node half has nothing to propagate and only forks its dW.  C: 19 halves >
# BWD_NBUF = 16: the ring comes round and its joins are waited on; fp32 GEMMs, the narrow BN backward.
CASES = {
    "A": dict(net="lg", order=2, d=32, layers=3, graphs=5, seed=11, grads=True),
    "B": dict(net="lg", order=1, d=32, layers=3, graphs=4, seed=12, grads=False),
    "C": dict(net="simple", order=0, d=4, layers=20, graphs=6, seed=13, grads=True),
}

# [(class, stream)] of the stamped launches, recorded from commit b943851
STAMPED = {
    "A": [
        (0, 0), (0, 0), (1, 0), (2, 0), (1, 0), (2, 0), (1, 0), (2, 0), (1, 0), (2, 0), (1, 0), (4, 0), (4, 1),
        (4, 1), (9, 1), (4, 0), (5, 0), (5, 0), (7, 0), (9, 1), (6, 1), (10, 1), (8, 0), (5, 0), (5, 0), (7, 0),
        (6, 1), (10, 1), (8, 0), (5, 0), (5, 0), (7, 0), (9, 1), (6, 1), (10, 1), (8, 0), (8, 0), (5, 0), (5, 0),
        (6, 1), (10, 1), (7, 0), (8, 0), (0, 0)],
    "B": [
        (0, 0), (0, 0), (1, 0), (2, 0), (1, 0), (2, 0), (1, 0), (2, 0), (1, 0), (2, 0), (1, 0), (4, 0), (4, 1),
        (4, 1), (4, 0), (5, 0), (5, 0), (7, 0), (6, 1), (10, 1), (8, 0), (5, 0), (5, 0), (7, 0), (6, 1), (10, 1),
        (8, 0), (5, 0), (5, 0), (7, 0), (6, 1), (10, 1), (8, 0), (5, 0), (5, 0), (6, 1), (10, 1)],
    "C": [
        (0, 0), (0, 0), (1, 0), (3, 0), (1, 0), (3, 0), (1, 0), (3, 0), (1, 0), (3, 0), (1, 0), (3, 0), (1, 0),
        (3, 0), (1, 0), (3, 0), (1, 0), (3, 0), (1, 0), (3, 0), (1, 0), (3, 0), (1, 0), (3, 0), (1, 0), (3, 0),
        (1, 0), (3, 0), (1, 0), (3, 0), (1, 0), (3, 0), (1, 0), (3, 0), (1, 0), (3, 0), (1, 0), (3, 0), (1, 0),
        (3, 0), (1, 0), (4, 0), (4, 1), (4, 1), (9, 1), (4, 0), (7, 0), (9, 1), (6, 1), (10, 1), (8, 0), (7, 0),
        (9, 1), (6, 1), (10, 1), (8, 0), (7, 0), (9, 1), (6, 1), (10, 1), (8, 0), (7, 0), (9, 1), (6, 1), (10, 1),
        (8, 0), (7, 0), (9, 1), (6, 1), (10, 1), (8, 0), (7, 0), (9, 1), (6, 1), (10, 1), (8, 0), (7, 0), (9, 1),
        (6, 1), (10, 1), (8, 0), (7, 0), (9, 1), (6, 1), (10, 1), (8, 0), (7, 0), (9, 1), (6, 1), (10, 1), (8, 0),
        (7, 0), (9, 1), (6, 1), (10, 1), (8, 0), (7, 0), (9, 1), (6, 1), (10, 1), (8, 0), (7, 0), (9, 1), (6, 1),
        (10, 1), (8, 0), (7, 0), (9, 1), (6, 1), (10, 1), (8, 0), (7, 0), (9, 1), (6, 1), (10, 1), (8, 0), (7, 0),
        (9, 1), (6, 1), (10, 1), (8, 0), (7, 0), (9, 1), (6, 1), (10, 1), (8, 0), (7, 0), (9, 1), (6, 1), (10, 1),
        (8, 0), (7, 0), (9, 1), (6, 1), (10, 1), (8, 0), (7, 0), (9, 1), (6, 1), (10, 1), (8, 0), (0, 0)],
}
# launches per class (hgnn_amd.roofline.NAMES order) of case A in dispatch mode, recorded from commit b943851
CENSUS_A = [3, 5, 4, 0, 4, 8, 4, 4, 5, 3, 4]

_steps = {}


def _step_fn(name):
    """A closure running one forward + backward of the case (model and batch built once per process)."""
    if name in _steps:
        return _steps[name]
    import torch

    import hgnn_amd.datagen as dg
    from functions.batching import prepare_batch
    from functions.operators import graph_operators
    from models.gnns.model_mnb import GNN_lg, GNN_simple
    cs = CASES[name]
    torch.manual_seed(cs["seed"])
    graphs = dg.qm9_shape_dataset(cs["graphs"], seed=cs["seed"], n_min=5, n_max=9)
    data = [[X, A, t, *graph_operators([X, A], 1, True)] for X, A, t in graphs]
    X, W, T, XL, WL, Pm, Pd, mask, mask_lg, Nb, Eb = [t.cuda() for t in prepare_batch(data, 0, 1)]
    if cs["net"] == "lg":
        model = GNN_lg(0, cs["d"], cs["layers"], 5, 1, 1, cs["order"]).cuda()
    else:
        model = GNN_simple(0, cs["d"], cs["layers"], 5, 1, 1).cuda()
    X.requires_grad_(cs["grads"])
    W.requires_grad_(cs["grads"])
    T = T[:, :1].contiguous()

    def step():
        for p in model.parameters():
            p.grad = None
        X.grad = W.grad = None
        if cs["net"] == "lg":
            out = model([X, XL, W, WL, Pm, Pd], Nb, mask, Eb, mask_lg)
        else:
            out = model([X, W], Nb, mask)
        torch.nn.MSELoss()(out, T).backward()
        torch.cuda.synchronize()

    _steps[name] = step
    return step


def _stamp_timer():
    from hgnn_amd import roofline as RF
    from hgnn_amd.net import TIMER_STAMPS, KernelTimer
    return KernelTimer(4096, range(RF.N_CLASSES), mode=TIMER_STAMPS, stamp_words=1 << 20)


def _stamped(name, steps=1):
    """[(class, stream)] of one step; with steps > 1, of each step after a reset()."""
    step = _step_fn(name)
    tm = _stamp_timer()
    seqs = []
    try:
        for _ in range(steps):
            tm.reset()
            with tm:
                step()
            seqs.append([(cls, stream) for cls, _, _, stream in tm.launches()])
    finally:
        tm.close()
    return seqs


def _census(name):
    from hgnn_amd import roofline as RF
    from hgnn_amd.net import KernelTimer
    step = _step_fn(name)
    tm = KernelTimer(4096, range(RF.N_CLASSES))
    try:
        with tm:
            step()
        return [tm.elapsed(k) for k in range(RF.N_CLASSES)]
    finally:
        tm.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_stamped_launch_sequence(name):
    got = _stamped(name)[0]
    print(name, got)
    assert got == [tuple(x) for x in STAMPED[name]]


def test_dispatch_census():
    from hgnn_amd import roofline as RF
    got = _census("A")
    print(got)
    assert len(CENSUS_A) == RF.N_CLASSES == 11
    assert [n for _, n in got] == CENSUS_A
    for k, (ms, n) in enumerate(got):
        assert n == 0 or ms > 0.0, (RF.NAMES[k], ms, n)


def test_reset_gives_the_same_sequence_again():
    first, second = _stamped("A", steps=2)
    assert first == second == [tuple(x) for x in STAMPED["A"]]


def test_dispatch_timer_has_no_launch_list():
    import ctypes

    from hgnn_amd import _lib as L
    from hgnn_amd import roofline as RF
    from hgnn_amd.net import KernelTimer
    tm = KernelTimer(64, range(RF.N_CLASSES))
    try:
        cls = (ctypes.c_int * 4)()
        t0, t1 = (ctypes.c_double * 4)(), (ctypes.c_double * 4)()
        assert L.lib().hgnn_timer_launches(tm.handle, 4, cls, t0, t1, None) == -2  # -HGNN_ERR_UNSUPPORTED
        with pytest.raises(RuntimeError, match="unsupported"):
            tm.launches()
    finally:
        tm.close()


if __name__ == "__main__":
    for p in (REPO, os.path.join(REPO, "hgnn-2_amd")):
        sys.path.insert(0, p)
    print("STAMPED = {")
    for nm in sorted(CASES):
        print(f"    {nm!r}: {_stamped(nm)[0]!r},")
    print("}")
    print(f"CENSUS_A = {[n for _, n in _census('A')]!r}")
