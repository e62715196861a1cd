"""Shared by tests/test_ccn_train_batch_cpu.py and tests/test_gpu_ccn_train_batch.py: the mini-batch cases and the
fp64 oracle of CcnTrainStep(batch_size=B).  Generators, MEAN, STD, LR, det_init seeds, targets t[:n_out] and the shape
names are those of tests/test_gpu_ccn_train.py (imported, not restated)."""

import torch

from test_gpu_ccn_train import LR, MEAN, MODELS, STD, _graphs, _model, _Oracle, _self_loops  # noqa: F401


def graphs_2d():
    import hgnn_amd.datagen as dg
    return _self_loops(dg.qm9_shape_dataset(5, seed=702, n_min=6, n_max=8))


def model_2d(seed):
    from models.compnets.model_ccn import CCN_2D
    return _model("A", seed, CCN_2D)  # CCN_2D(5, 1, 2, 2)


# name -> (order, model builder, graphs builder, batch size): the oracle cases of the issue, in its order
ORACLE_CASES = {
    "A-b4": (1, lambda: _model("A", 47), lambda: _graphs("A"), 4),
    "DA-b4": (1, lambda: _model("A", 47), lambda: _graphs("D") + _graphs("A"), 4),
    "B-b4": (1, lambda: _model("B", 33), lambda: _graphs("B"), 4),
    "B-b2": (1, lambda: _model("B", 33), lambda: _graphs("B"), 2),
    "2D-b2": (2, lambda: model_2d(52), graphs_2d, 2),
    "2D-b5": (2, lambda: model_2d(52), graphs_2d, 5),
}


class BatchOracle(_Oracle):
    """The mini-batch definition in fp64: per mini-batch of B consecutive graphs, all on the same weights,
    oracle.ref_ccn.ccn_forward per graph, yn = (y - mean) / (std + 1e-8), nn.MSELoss over the (B, n_out) block,
    backward (the gradients sum over the graphs) and one torch.optim.Adamax step; the last mini-batch may be shorter
    and divides by its own size.  Meters by RunningAverage's rule, once per mini-batch.  compare() is the per-graph
    oracle's: `steps` counts mini-batches."""

    def step_batch(self, graphs, n_out):
        from oracle import ref_ccn as RC
        self.opt.zero_grad()
        out = torch.stack([RC.ccn_forward(self.p, x.double(), a.double(), self.order, self.layers)
                           for x, a, _ in graphs])
        yn = (torch.stack([t[:n_out] for _, _, t in graphs]).double() - MEAN) / (STD + 10 ** -8)
        loss = torch.nn.MSELoss()(out, yn)
        loss.backward()
        for n in self.names:
            g = self.p[n].grad.abs()
            self.noisy[n] |= (g > 0) & (g <= 1e-4 * g.max())
        self.opt.step()
        self.steps += 1
        self.outs += list(out.detach())
        self.loss, self.mae = loss.item(), (out.detach() - yn).abs().mean().item()
        for i, v in enumerate((self.loss, self.mae)):
            self.run[i] = v if self.run[i] is None else 0.9 * v + 0.1 * self.run[i]

    def loose(self):
        """(elements on the loose bound, all elements)."""
        return (sum(int(self.noisy[n].sum()) for n in self.names), sum(self.p[n].numel() for n in self.names))


_ORACLES = {}


def run_oracle(case):
    """(net as initialised, graphs, batch size, the oracle after every mini-batch); computed once per process."""
    if case not in _ORACLES:
        order, model, graphs, B = ORACLE_CASES[case]
        net, gs = model(), graphs()
        orc = BatchOracle(net, order)
        for g0 in range(0, len(gs), B):
            orc.step_batch(gs[g0:g0 + B], net.n_outputs)
        _ORACLES[case] = (order, gs, B, orc)
    order, gs, B, orc = _ORACLES[case]
    return ORACLE_CASES[case][1](), gs, B, orc
