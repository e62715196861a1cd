"""Seeded synthetic graph generators for the benchmark configurations.

The reference ships no SBM generator and its QM9 pipeline needs rdkit
(SURVEY.md §2, §8 d), so the build defines both generators here, with the
statistics SURVEY.md §8 d fixes:

* QM9-shape: N ~ U{9..29}, a random recursive tree with bond orders drawn from
  {1, 1, 1, 1.5, 2, 3}, round(0.25 N) extra unit bonds, one-hot atom type over 5
  types, 13 regression targets (task 0 is used).
* SBM: two equal blocks (z = i mod 2), p_in / p_out, symmetric, no self loops,
  one-hot(min(deg, 4)) node features (5 features).

* Three collinear points: the reference's own generated data set
  (`functions/data_generator.py:45-87`), the classification task of
  `scripts/main_generate_ccn.py`; it returns the reference's 7-tuples.

The first two generators return a list of ``(X (N, f), A (N, N), t (13,))`` float32
tensors -- the first three members of the reference's 7-tuple instances
(`functions/data_generator.py:85`, `preprocessing/preprocessing.py:95-97`).
The operator members are produced by ``functions.operators.graph_operators``.

This module imports nothing but torch/random at load time (three_collinear_points
imports functions.operators only when asked for the operators) so the golden-fixture script can
load it next to the reference without a package-name clash.
"""

import random

import torch

BOND_ORDERS = (1.0, 1.0, 1.0, 1.5, 2.0, 3.0)


def qm9_shape_graph(rng, gen, n_types=5, n_targets=13, n_min=9, n_max=29):
    """One QM9-shaped molecule graph (SURVEY.md §8 d, 'QM9-shape generator')."""
    n = rng.randint(n_min, n_max)
    A = torch.zeros(n, n)
    for v in range(1, n):
        p = rng.randrange(v)
        w = rng.choice(BOND_ORDERS)
        A[p, v] = w
        A[v, p] = w
    extra = int(round(0.25 * n))
    added = 0
    tries = 0
    while added < extra and tries < 100:
        tries += 1
        i = rng.randrange(n)
        j = rng.randrange(n)
        if i == j or A[i, j] != 0:
            continue
        A[i, j] = 1.0
        A[j, i] = 1.0
        added += 1
    X = torch.zeros(n, n_types)
    for v in range(n):
        X[v, rng.randrange(n_types)] = 1.0
    t = torch.randn(n_targets, generator=gen)
    return X, A, t


def qm9_shape_dataset(n_graphs, seed=0, **kw):
    rng = random.Random(seed)
    gen = torch.Generator().manual_seed(seed)
    return [qm9_shape_graph(rng, gen, **kw) for _ in range(n_graphs)]


def sbm_graph(gen, n=50, p_in=0.3, p_out=0.05, n_feat=5, n_targets=13):
    """Two-block stochastic block model graph (SURVEY.md §8 d, 'SBM generator')."""
    z = torch.arange(n) % 2
    same = z.view(-1, 1) == z.view(1, -1)
    prob = torch.where(same, torch.tensor(p_in), torch.tensor(p_out))
    u = torch.rand(n, n, generator=gen) < prob
    upper = torch.triu(u, diagonal=1).float()
    A = upper + upper.t()
    deg = A.sum(dim=1).long()
    X = torch.zeros(n, n_feat)
    X[torch.arange(n), torch.clamp(deg, max=n_feat - 1)] = 1.0
    t = torch.randn(n_targets, generator=gen)
    return X, A, t


def sbm_dataset(n_graphs, n=50, seed=0, **kw):
    gen = torch.Generator().manual_seed(seed)
    return [sbm_graph(gen, n=n, **kw) for _ in range(n_graphs)]


def three_collinear_points(n, n_max=50, d=5, p=0.5, c=0.5, seed=0, operators=False):
    """The generated data set of functions/data_generator.py:45-87: n random graphs of 3 + randint(0, n_max - 3)
    nodes (3 .. n_max - 1) with d random normal features per node.  With probability p a graph has label 1: three
    of its rows are multiples 10 * randn(1) * x of one direction x = randn(1, d), placed among the random rows at
    shuffled positions.  A = (rand > c), A[0, 1] = 1, symmetrised with min(A + A^T, 1); the diagonal may be 1
    (and 2 once the driver adds I: the CCN drop-in goes by the pattern A > 0).

    Returns the reference's instances [X, A, LongTensor([label]), W, WL, Pm, Pd]; the operators are
    functions.operators.graph_operators([X, A], dual=True) when operators=True, else None (the CCN drivers
    ignore them).  Everything is drawn from one torch.Generator seeded with `seed`; the reference draws from the
    global RNG and random.shuffle, so its data is matched in distribution, not bit for bit."""
    gen = torch.Generator().manual_seed(seed)
    y = torch.rand(n, generator=gen) < p
    extra = torch.randint(0, n_max - 3, (n,), generator=gen)
    if operators:
        from functions.operators import graph_operators
    data = []
    for i in range(n):
        ni = int(extra[i])
        if bool(y[i]):
            x = torch.randn(1, d, generator=gen)
            pts = [10 * torch.randn(1, generator=gen) * x for _ in range(3)]
            rows = torch.cat([torch.randn(ni, d, generator=gen)] + pts, dim=0)
            X = rows[torch.randperm(ni + 3, generator=gen)].contiguous()
        else:
            X = torch.randn(3 + ni, d, generator=gen)
        A = (torch.rand(3 + ni, 3 + ni, generator=gen) > c).float()
        A[0, 1] = 1.0
        A = torch.clamp(A + A.t(), max=1.0)
        ops = graph_operators([X, A], dual=True) if operators else (None, None, None, None)
        data.append([X, A, torch.tensor([int(y[i])], dtype=torch.int64), *ops])
    return data
