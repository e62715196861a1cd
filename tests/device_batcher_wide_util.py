"""The "wide pack": the graphs the node-family device builder (csrc/batcher.hip, n <= 64, dual=False) is tested on,
shared by tests/test_device_batcher_wide_inputs.py (CPU: the properties claimed here hold for the committed
generators) and tests/test_gpu_device_batcher_wide.py (GPU: the device image against the host's).

Every case is the smallest shape at which one thing can go wrong; INDEX names where each sits in the list."""

import numpy as np
import torch

SBM_NNZ = [466, 388, 390]
COLLINEAR_N = [44, 29, 20, 46, 48, 3]
COLLINEAR_PICK = [0, 1, 2, 3, 4, 7]  # of three_collinear_points(12, seed=3)
INDEX = {"sbm": [0, 1, 2], "collinear": [3, 4, 5, 6, 7, 8], "k64": 9, "k33": 10, "high40": 11, "path64": 12,
         "single": 13, "qm9": [14, 15, 16, 17]}
N_GRAPHS = 18


def hand_features(n):
    X = torch.zeros(n, 5)
    X[torch.arange(n), torch.arange(n) % 5] = 1.0
    return X, torch.arange(13, dtype=torch.float32) * 0.25 - float(n)


def hand_graph(n, bonds, loops=()):
    """bonds: (i, j) or (i, j, w), stored both ways; loops: nodes with a self loop of weight 1."""
    A = torch.zeros(n, n)
    for b in bonds:
        i, j, w = b if len(b) == 3 else (*b, 1.0)
        A[i, j] = A[j, i] = w
    for i in loops:
        A[i, i] = 1.0
    X, t = hand_features(n)
    return X, A, t


def high40():
    """40 nodes, bonds only among nodes >= 32: word 0 of every row pattern is empty.  (A^2)[34][36] =
    1 * 1 + 1 * (-1) and (A^2)[35][37] = 1 * 1 + 1 * (-1) cancel to exactly 0.0: no entry there."""
    return hand_graph(40, [(34, 35, 1.0), (35, 36, 1.0), (34, 37, 1.0), (37, 36, -1.0), (32, 39, 2.0), (38, 39, 1.0)])


def collinear_graphs():
    """Six graphs of the generated data set as (x, A, t): t is 13 wide like every graph of the pack, the label in
    front."""
    import hgnn_amd.datagen as dg
    data = dg.three_collinear_points(12, seed=3)
    out = []
    for k in COLLINEAR_PICK:
        X, A, y = data[k][:3]
        t = torch.arange(13, dtype=torch.float32) * 0.5
        t[0] = float(y[0])
        out.append((X, A, t))
    return out


def wide_graphs():
    import hgnn_amd.datagen as dg
    gs = list(dg.sbm_dataset(3, n=50, seed=5))
    gs += collinear_graphs()
    gs.append(hand_graph(64, [(i, j) for i in range(64) for j in range(i + 1, 64)], loops=range(64)))  # K64 + loops
    gs.append(hand_graph(33, [(i, j) for i in range(33) for j in range(i + 1, 33)]))  # K33
    gs.append(high40())
    gs.append(hand_graph(64, [(i, i + 1) for i in range(62)]))  # a path; node 63 isolated
    gs.append(hand_graph(1, []))
    gs += dg.qm9_shape_dataset(4, seed=5)
    assert len(gs) == N_GRAPHS
    return gs


def real_weights(gs, seed=11):
    """The same graphs with every bond weight (and self loop) a seeded uniform(0.5, 2.5) value, symmetric."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for X, A, t in gs:
        R = torch.rand(A.shape, generator=g) * 2.0 + 0.5
        W = torch.triu(R, 1)
        W = W + W.T + torch.diag(torch.diagonal(R))
        out.append((X, torch.where(A != 0, W, torch.zeros_like(W)), t))
    return out


def small_indices(gs):
    """The pack's graphs the narrow kernel (n <= 32) builds."""
    return [i for i, (x, _, _) in enumerate(gs) if x.shape[0] <= 32]


def index_lists(n):
    rng = np.random.default_rng(7)
    return [list(range(n)), list(range(n))[::-1], [3, 3, 0, n - 1, 9, 3, n - 1, n - 2, 11, 9], [INDEX["k64"]],
            [INDEX["single"]], [int(i) for i in rng.integers(0, n, 64)]]


def host_batch(pack, idx, J, dual=False, task=0, device="cpu"):
    from hgnn_amd.csr import CsrBatch
    graphs = [pack.graph(i) for i in idx]
    targets = torch.tensor([float(t[task]) for _, _, t in graphs])
    return CsrBatch([(x, a) for x, a, _ in graphs], J=J, dual=dual, targets=targets, device=device)


def assert_same_batch(dev_batch, host_batch):
    assert bytes(dev_batch.layout) == bytes(host_batch.layout)
    got = dev_batch.image.cpu()
    want = host_batch.host if host_batch.image.device.type == "cpu" else host_batch.image.cpu()
    if not torch.equal(got, want):
        diff = torch.nonzero(got != want).flatten()
        raise AssertionError(f"{diff.numel()} image bytes differ, first at {int(diff[0])} of {got.numel()}")
    assert torch.equal(dev_batch.T.cpu(), host_batch.T.cpu())
