"""The graph set and the host reference shared by tests/test_ccn_pack_host.py and tests/test_gpu_ccn_pack.py."""

import torch

TASKS = (0, 7)


def real_weights(graph, seed):
    """The same graph with every stored weight (a self loop included) a seeded uniform(0.5, 2.5) value, symmetric."""
    X, A, t = graph
    R = torch.rand(A.shape, generator=torch.Generator().manual_seed(seed)) * 2.0 + 0.5
    W = torch.triu(R, 1)
    W = W + W.T + torch.diag(torch.diagonal(R))
    return X, torch.where(A != 0, W, torch.zeros_like(W)), t


def graph_set():
    """15 graphs (x (n, 5), A (n, n), t (13,)): 0-7 QM9-shape, 8 one node without bonds, 9 last node isolated,
    10 a stored self loop, 11 / 12 real-valued copies of 3 and 10, 13 an SBM graph of 40 nodes (rows of 40 floats
    are 16-byte multiples, QM9's 29 are not; still inside the fused CCN-1D kernel's bound), 14 an SBM graph of 72
    nodes (above every small-graph bound: its chunk takes the unfused route)."""
    import hgnn_amd.datagen as dg
    gs = dg.qm9_shape_dataset(11, seed=31)
    qm9, (Xi, Ai, ti), (Xs, As, ts) = gs[:8], gs[8], gs[9]
    one = (torch.eye(1, 5), torch.zeros(1, 1), torch.randn(13, generator=torch.Generator().manual_seed(1)))
    Ai = Ai.clone()
    Ai[-1, :] = 0
    Ai[:, -1] = 0
    As = As.clone()
    As[2, 2] = 1.0  # as the generated data stores it: A + I puts 2.0 there
    loop = (Xs, As, ts)
    out = qm9 + [one, (Xi, Ai, ti), loop, real_weights(qm9[3], 5), real_weights(loop, 6)]
    out += dg.sbm_dataset(1, n=40, seed=4) + dg.sbm_dataset(1, n=72, seed=5, p_in=0.12, p_out=0.03)
    assert len(out) == 15 and [g[0].shape[0] for g in out[13:]] == [40, 72]
    assert max(g[0].shape[0] for g in out[:13]) <= 29
    assert out[12][1][2, 2] not in (0.0, 1.0)
    return out


def narrow_set():
    """The first five graphs with f_in = 3."""
    return [(X[:, :3].contiguous(), A, t) for X, A, t in graph_set()[:5]]


def instances(graphs):
    """The reference's 7-tuples; the CCN drivers read only the first three members."""
    return [[X, A, t, None, None, None, None] for X, A, t in graphs]


def reference_chunk(graphs, task, nmax=None):
    """scripts/train_ccn.py:35-37 per graph -- X, adj = A + torch.eye(n), targets[task].view(1) -- padded to the
    chunk's largest graph (or nmax) as hgnn_amd.train.CcnTrainStep._chunks pads."""
    nmax = nmax or max(int(X.shape[0]) for X, _, _ in graphs)
    G, f = len(graphs), graphs[0][0].shape[1]
    Xp, Ap = torch.zeros(G, nmax, f), torch.zeros(G, nmax, nmax)
    nb, y = torch.empty(G, dtype=torch.int64), torch.empty(G, 1)
    for b, (X, A, t) in enumerate(graphs):
        n = X.size(0)
        adj = A + torch.eye(n)
        Xp[b, :n] = X
        Ap[b, :n, :n] = adj
        nb[b] = n
        y[b] = t[task].view(1)
    return Xp, Ap, nb, y


def assert_same_chunk(got, want, what=""):
    names = ("X", "A + I", "n_batch", "y")
    assert len(got) == 4
    for name, g, w in zip(names, got, want):
        g = g.cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what} {name}: {g.dtype} {tuple(g.shape)}"
        assert torch.equal(g, w), f"{what} {name}: {int((g != w).sum())} elements differ"
