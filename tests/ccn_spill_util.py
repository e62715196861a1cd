"""Shared by tests/test_ccn_spill_cpu.py and tests/test_gpu_ccn_spill.py: the spill-only cases (shapes the LDS
kernels of csrc/ccn_small.hip refuse and the spill instantiation takes) and their fp64 oracles.  Generators, MEAN,
STD, LR, targets t[:n_out] and the oracle are those of tests/test_gpu_ccn_train.py and tests/ccn_batch_util.py
(imported, not restated).

  W27  CCN_1D(8, 2, 8, 2), det_init 71, on er(27, .15, 270), er(14, .3, 271), er(5, .5, 272), er(20, .2, 273),
       er(9, .4, 274): hidden 8 stops the LDS kernels at 26 nodes
  W64  CCN_1D(8, 2, 8, 4), det_init 73, on er(64, .1, 640), er(33, .2, 641), er(7, .5, 642): the node bound
  DA6  CCN_1D(5, 1, 2, 6), det_init 47, on shapes D + A of test_gpu_ccn_train.py (padded to 40 nodes; six layers
       stop the LDS kernels at 35)
Both W cases: X = randn(n, 8), then the target randn(2), per graph in that order from one
torch.Generator().manual_seed(270) (W27) / manual_seed(640) (W64)."""

import torch

import ccn_edge_util as EU
import fixture_util as fu
from ccn_batch_util import BatchOracle
from test_gpu_ccn_train import _graphs, _Oracle

W_ADJ = {
    "W27": lambda: [EU.er(27, .15, 270), EU.er(14, .3, 271), EU.er(5, .5, 272), EU.er(20, .2, 273), EU.er(9, .4, 274)],
    "W64": lambda: [EU.er(64, .1, 640), EU.er(33, .2, 641), EU.er(7, .5, 642)],
}
W_SEED = {"W27": 270, "W64": 640}
# case -> (model arguments, det_init seed, mini-batch size of the oracle's second run)
CASES = {"W27": ((8, 2, 8, 2), 71, 2), "W64": ((8, 2, 8, 4), 73, 2), "DA6": ((5, 1, 2, 6), 47, 4)}
# elements on _Oracle.compare's loose bound, measured with the fp64 oracle: (case, batch size or None) -> (loose, all)
LOOSE = {("W27", None): (0, 322), ("W27", 2): (0, 322), ("W64", None): (11, 626), ("W64", 2): (9, 626),
         ("DA6", None): (1, 90), ("DA6", 4): (4, 90)}


def graphs(case):
    """(X, adj with self loops, targets) per graph."""
    if case == "DA6":
        return _graphs("D") + _graphs("A")
    gen = torch.Generator().manual_seed(W_SEED[case])
    out = []
    for a in W_ADJ[case]():
        x = torch.randn(a.shape[0], 8, generator=gen)
        out.append((x, a, torch.randn(2, generator=gen)))
    return out


def model(case):
    from models.compnets.model_ccn import CCN_1D
    args, seed, _ = CASES[case]
    net = CCN_1D(*args)
    fu.det_init(net, seed)
    return net


_ORACLES = {}


def run_oracle(case, B):
    """The fp64 oracle after the whole list, stepping per graph (B None) or per mini-batch of B; once per process."""
    if (case, B) not in _ORACLES:
        net, gs = model(case), graphs(case)
        n_out = net.n_outputs
        if B is None:
            orc = _Oracle(net, 1)
            for x, a, t in gs:
                orc.step(x, a, t[:n_out])
        else:
            orc = BatchOracle(net, 1)
            for g0 in range(0, len(gs), B):
                orc.step_batch(gs[g0:g0 + B], n_out)
        _ORACLES[(case, B)] = orc
    return _ORACLES[(case, B)]


def loose(orc):
    return (sum(int(orc.noisy[n].sum()) for n in orc.names), sum(orc.p[n].numel() for n in orc.names))
