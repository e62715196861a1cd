"""Device-resident training step.

The reference's step (scripts/train_mnb.py:41-91) runs, per batch: prepare_batch
on the host, normalize_data(T), forward, nn.MSELoss, .item() twice for the
RunningAverage logs (two host syncs), backward and torch.optim.Adamax -- with
the optimizer re-created every epoch (scripts/main_gnn_qm9.py:185), which
resets its state.  TrainStep does the same arithmetic with every piece on the
device and no host synchronisation:

  forward      the network executor (dense inputs or a CsrBatch)
  loss         hgnn_mse_loss: normalised targets, MSE, MAE, the dloss seed and
               both RunningAverages, in one kernel
  backward     the executor's backward (autograd seeded with dloss)
  all-reduce   optional gradient bucket all-reduce (hgnn_amd.dp.GradAllReduce)
  optimizer    hgnn_optim_step: Adamax (the default; SGD with momentum or Adam, the drivers'
               --optim) over every parameter in one launch

Classification (the reference's `mean == 0` branch, scripts/train_mnb.py:50-51: T cast to
class indices, the drivers' nn.CrossEntropyLoss, scripts/main_generate.py:147) uses
hgnn_xent_loss instead; the MAE meters stay untouched as in the reference.

The other loop of the drivers, test_with_mnb (scripts/test_mnb.py:25-92: per batch a forward in eval mode, the
criterion's .item() and utils.evaluation(...).item() into two AverageMeters), is TrainStep.evaluate: hgnn_eval_loss /
hgnn_eval_xent accumulate the meters on the device over the batches of a set, and eval_result reads them once.
train_epoch and eval_epoch are train_with_mnb and test_with_mnb over a data set.
"""

import ctypes
import math
import os
import struct

import torch

from . import _lib as L
from .dp import sum_meters


class _TargetWord:
    """The error word of the cross-entropy kernels (a class target outside [0, dim_output) or not an integer ORs 1
    into it), checked without synchronising the stream: watch() copies it to pinned memory behind an event, poll()
    at the next step reads the copy once the event has completed.  HGNN_STRICT=1: watch() reads the word at once
    (a host sync).  Shared by TrainStep and CcnTrainStep."""

    MESSAGE = "hgnn_amd: class target outside [0, dim_output) or not an integer"

    def __init__(self, dev):
        self.dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.host = torch.zeros(1, dtype=torch.int32, pin_memory=True)
        self.ev = None

    def watch(self):
        """After the kernels that may have set the word."""
        if os.environ.get("HGNN_STRICT", "0") == "1":
            self.ev = None
            if int(self.dev.item()):
                self.dev.zero_()
                raise RuntimeError(self.MESSAGE)
        elif not torch.cuda.is_current_stream_capturing():
            self.host.copy_(self.dev, non_blocking=True)
            self.ev = torch.cuda.Event()
            self.ev.record()

    def poll(self, block):
        ev = self.ev
        if ev is None:
            return
        if block:
            ev.synchronize()
        elif not ev.query():
            return
        self.ev = None
        if int(self.host[0]):
            self.dev.zero_()
            self.host.zero_()
            raise RuntimeError(self.MESSAGE + " (the rows were left out of the loss and gradients)")

    def check(self):
        """Raise if a watched kernel saw a bad target (host sync)."""
        self.poll(block=True)
        if int(self.dev.item()):
            self.dev.zero_()
            raise RuntimeError(self.MESSAGE)


class _Optimizer:
    """The optimizer of a training step, shared by TrainStep and CcnTrainStep: the drivers' --optim
    sgd|adamax|adam and --momentum (scripts/main_ccn.py:59-62, 155-162, scripts/main_gnn.py:161-167), i.e.
    torch.optim.Adamax(params, lr), torch.optim.SGD(params, lr, momentum=momentum) or torch.optim.Adam(params, lr),
    with betas, eps and weight_decay where the optimizer has them.  State: adamax exp_avg and exp_inf, adam exp_avg
    and exp_avg_sq, sgd momentum_buffer.  .lr is read at every step, so the drivers' damping between epochs
    (main_ccn.py:183-186) is `step.lr *= damping`."""

    @staticmethod
    def _check_optimizer(optimizer):
        if optimizer not in L.OPT_KIND:
            raise RuntimeError(f"hgnn_amd: optimizer={optimizer!r}: expected \"adamax\", \"sgd\" or \"adam\"")

    def _init_optimizer(self, optimizer, momentum):
        self._check_optimizer(optimizer)
        self.optimizer = optimizer
        self.momentum = float(momentum)
        self._kind = L.OPT_KIND[optimizer]
        self.reset_optimizer()

    def reset_optimizer(self):
        """The drivers build a new optimizer every epoch (scripts/main_gnn_qm9.py:185, scripts/main_ccn.py:155-162):
        zero state, step 0."""
        zeros = lambda: [torch.zeros_like(p) for p in self.params]  # noqa: E731
        if self.optimizer == "sgd":
            self.momentum_buffer = zeros()
        elif self.optimizer == "adam":
            self.exp_avg, self.exp_avg_sq = zeros(), zeros()
        else:
            self.exp_avg, self.exp_inf = zeros(), zeros()
        self.step_count = 0

    def _states(self):
        """hgnn_optim_step's (state1, state2) as pointer arrays; sgd has no second state."""
        if self.optimizer == "sgd":
            return L.ptr_array(self.momentum_buffer), None
        return L.ptr_array(self.exp_avg), L.ptr_array(self.exp_avg_sq if self.optimizer == "adam" else self.exp_inf)

    def _b1(self):
        """hgnn_optim_step's beta1_or_momentum."""
        return self.momentum if self.optimizer == "sgd" else self.betas[0]

    def _optim_step(self, lib, grads, stream):
        """One step on `grads` (hgnn_optim_step); counts it."""
        self.step_count += 1
        s1, s2 = self._states()
        L.check(lib.hgnn_optim_step(self._kind, len(self.params), L.ptr_array(self.params), L.ptr_array(grads),
                                    s1, s2, self._numel, self.lr,
                                    self._b1(), self.betas[1], self.eps, self.weight_decay, self.step_count, stream),
                f"{self.optimizer} step")

    def _step_scalars(self, t0, n):
        """The (n, 2) per-step scalars of steps t0 + 1 .. t0 + n for the fused kernels' _opt entries, formed in
        double as hgnn_optim_step forms its own."""
        b1, b2 = self.betas
        if self.optimizer == "sgd":
            return [(self.lr, 0.0)] * n
        if self.optimizer == "adam":
            return [(self.lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)) for t in range(t0 + 1, t0 + 1 + n)]
        return [(self.lr / (1.0 - b1 ** t), 0.0) for t in range(t0 + 1, t0 + 1 + n)]


class TrainStep(_Optimizer):
    """One train_with_mnb minibatch step for a GNN_lg / GNN_simple drop-in model.

    step(batch) with batch = the 11-tuple of prepare_batch (on the model's device)
    or a hgnn_amd.csr.CsrBatch with targets.  Returns the device tensor `stats`:
    [loss, mae, running loss, running mae] (read it when you log, not per step).
    optimizer="adamax" (default) | "sgd" | "adam" and momentum: see _Optimizer.

    Evaluation (test_with_mnb): reset_eval(), evaluate(batch) per batch, eval_result() -- or eval_epoch(data, task,
    bs) for all three; train_epoch(data, task, bs) is train_with_mnb.
    """

    def __init__(self, model, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, t_mean=None, t_std=1.0,
                 grad_allreduce=None, classification=None, optimizer="adamax", momentum=0.9):
        self._check_optimizer(optimizer)
        self.model = model
        # the reference's rule (train_mnb.py:50-51): mean == 0 marks generated (classification) data --
        # inferred only from an explicitly passed t_mean; TrainStep(model) is the regression step
        if classification is None:
            classification = t_mean is not None and float(t_mean) == 0.0
        self.classification = bool(classification)
        t_mean = 0.0 if t_mean is None else t_mean
        self.params = [p for p in model.parameters()]
        self.lr = float(lr)
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = float(eps)
        self.weight_decay = float(weight_decay)
        self.t_mean = float(t_mean)
        self.t_std = float(t_std)
        self.allreduce = grad_allreduce
        dev = self.params[0].device
        if dev.type != "cuda":
            raise RuntimeError("hgnn_amd: TrainStep runs on the GPU only (call model.cuda() first)")
        for p in self.params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("hgnn_amd: TrainStep needs contiguous float32 parameters")
        self.stats = torch.zeros(4, dtype=torch.float32, device=dev)
        # the evaluation meters (hgnn_eval_loss / hgnn_eval_xent): loss.sum, error.sum, count, hits, loss.val,
        # error.val
        self.eval_meters = torch.zeros(6, dtype=torch.float64, device=dev)
        # the class-target error word, checked at the next step without synchronising the stream
        # (HGNN_STRICT=1: checked at once)
        self._targets = _TargetWord(dev)
        self._numel = (ctypes.c_int64 * len(self.params))(*[p.numel() for p in self.params])
        self._init_optimizer(optimizer, momentum)

    def reset_running(self):
        """New RunningAverage meters (one pair per train_with_mnb call, scripts/train_mnb.py:34-35)."""
        self.stats.zero_()

    def reset_eval(self):
        """New AverageMeters (one pair per test_with_mnb call, scripts/test_mnb.py:32-33)."""
        self.eval_meters.zero_()

    def _forward(self, batch):
        from .csr import CsrBatch
        m = self.model
        if isinstance(batch, CsrBatch):
            if batch.T is None:
                raise RuntimeError("hgnn_amd: TrainStep needs a CsrBatch built with targets")
            return m.forward_csr(batch), batch.T
        X, W, T, XL, WL, Pm, Pd, mask, mask_lg, Nb, Eb = batch
        if m.dual:
            out = m([X, XL, W, WL, Pm, Pd], Nb, mask, Eb, mask_lg)
        else:
            out = m([X, W], Nb, mask)
        return out, T

    def _check_target_shape(self, out, T):
        if self.classification:
            if out.shape[1] < 2:
                raise RuntimeError("hgnn_amd: classification needs dim_output >= 2 (cross-entropy over one "
                                   "class is identically 0); pass t_mean != 0 or classification=False")
            if T.numel() != out.shape[0]:
                raise RuntimeError(f"hgnn_amd: class targets {tuple(T.shape)} do not match {out.shape[0]} rows")
        elif T.numel() != out.numel():
            raise RuntimeError(f"hgnn_amd: targets {tuple(T.shape)} do not match the output {tuple(out.shape)}")

    def __call__(self, batch):
        lib = L.lib()
        self._targets.poll(block=False)
        self.model.train()
        for p in self.params:
            p.grad = None
        out, T = self._forward(batch)
        T = T.to(torch.float32).contiguous()
        stream = L.stream_handle(out.device)
        dout = torch.empty_like(out)
        self._check_target_shape(out, T)
        if self.classification:
            L.check(lib.hgnn_xent_loss(L.ptr(out.detach()), L.ptr(T), out.shape[0], out.shape[1], L.ptr(self.stats),
                                       L.ptr(dout), L.ptr(self._targets.dev), stream), "cross-entropy loss")
            self._targets.watch()
        else:
            L.check(lib.hgnn_mse_loss(L.ptr(out.detach()), L.ptr(T), out.numel(), self.t_mean, self.t_std,
                                      L.ptr(self.stats), L.ptr(dout), stream), "mse loss")
        torch.autograd.backward(out, dout)
        if self.allreduce is not None:
            self.allreduce()
        grads = [p.grad for p in self.params]
        if any(g is None for g in grads):
            raise RuntimeError("hgnn_amd: a parameter received no gradient")
        self._optim_step(lib, grads, stream)
        return self.stats

    def check_targets(self):
        """Raise if a classification step or evaluation saw a target outside [0, dim_output) (host sync)."""
        self._targets.check()

    def evaluate(self, batch):
        """One batch of test_with_mnb (scripts/test_mnb.py:42-70): the forward in eval mode under no_grad (the
        model's mode is restored afterwards), then hgnn_eval_loss -- or hgnn_eval_xent on the classification branch
        -- adds the batch to the device tensor `eval_meters` = [loss.sum, error.sum, count, hits, loss.val,
        error.val], which is returned.  batch as for __call__.  No host synchronisation; parameters, gradients, BN
        running statistics, the optimizer state, step_count and stats are not touched.  reset_eval() starts a set,
        eval_result() reads it."""
        lib = L.lib()
        m = self.model
        if self.classification:
            self._targets.poll(block=False)
        was_training = m.training
        m.eval()
        try:
            with torch.no_grad():
                out, T = self._forward(batch)
        finally:
            m.train(was_training)
        out = out.detach().contiguous()
        T = T.to(torch.float32).contiguous()
        self._check_target_shape(out, T)
        stream = L.stream_handle(out.device)
        if self.classification:
            L.check(lib.hgnn_eval_xent(L.ptr(out), L.ptr(T), out.shape[0], out.shape[1], L.ptr(self.eval_meters),
                                       L.ptr(self._targets.dev), stream), "hgnn_eval_xent")
            self._targets.watch()
        else:
            L.check(lib.hgnn_eval_loss(L.ptr(out), L.ptr(T), out.shape[0], out.shape[1], self.t_mean, self.t_std,
                                       L.ptr(self.eval_meters), stream), "hgnn_eval_loss")
        return self.eval_meters

    def eval_result(self, accuracy=False, group=None):
        """(loss.avg, error.avg) of the set evaluated since reset_eval(): the one host read.  The averages are
        formed in Python doubles, sum / count as AverageMeter does; a zero count gives zeros (AverageMeter's
        initial state).  Classification: (loss.avg, 0.0) as the reference returns (error is never updated there);
        accuracy=True adds hits / count as a third value.  group: the sums and counts are first summed over the
        process group (hgnn_amd.dp.sum_meters), so every rank gets the average over all ranks' shards.  A bad class
        target shows at check_targets() (or at once under HGNN_STRICT=1), as for a training step."""
        if accuracy and not self.classification:
            raise RuntimeError("hgnn_amd: eval_result(accuracy=True) needs a classification step")
        m = sum_meters(self.eval_meters, group).tolist()
        count = m[2]
        loss = m[0] / count if count else 0.0
        if self.classification:
            return (loss, 0.0, m[3] / count if count else 0.0) if accuracy else (loss, 0.0)
        return loss, (m[1] / count if count else 0.0)

    def _batches(self, data, task, bs, dense):
        """The batches of one epoch in the order of functions.batching.get_batches(n, bs, data, False, False), on
        the model's device.  data: a list of reference instances [x, A, t, ...] -- CsrBatch(J=model.J,
        dual=model.dual), so GNN_simple gets its node-graph-only batch; dense=True: full 7-tuples through
        prepare_batch -- or a hgnn_amd.dataset.GraphPack (pack.batches), or a hgnn_amd.dataset.DevicePack built
        for the model's J and dual (its batches are built on the device; there is no dense form of them)."""
        from functions.batching import get_batches, prepare_batch
        from .csr import CsrBatch
        from .dataset import DevicePack, GraphPack
        m = self.model
        dev = self.params[0].device
        pack = isinstance(data, GraphPack)
        if isinstance(data, DevicePack):
            if dense:
                raise RuntimeError("hgnn_amd: a DevicePack builds CSR batches only (dense=True needs a GraphPack)")
            if data.J != m.J or data.dual != bool(m.dual):
                raise RuntimeError(f"hgnn_amd: DevicePack(J={data.J}, dual={data.dual}) does not match the model "
                                   f"(J={m.J}, dual={bool(m.dual)})")
            if data.device != dev:
                raise RuntimeError(f"hgnn_amd: DevicePack on {data.device}, model on {dev}")
            for idx in get_batches(len(data), bs, data, False, False):
                yield from data.batches(idx, len(idx), task)
            return
        for idx in get_batches(len(data), bs, data, False, False):
            if pack:
                # dense: prepare_batch reads all seven members, whatever the model uses of them
                for b in data.batches(idx, len(idx), task, J=m.J, dual=m.dual or dense, device=dev, dense=dense):
                    yield [t.to(dev) for t in b] if dense else b
                continue
            part = [data[i] for i in idx]
            if dense:
                yield [t.to(dev) for t in prepare_batch(part, task, m.J)]
            else:
                targets = torch.tensor([float(d[2][task]) for d in part], dtype=torch.float32)
                yield CsrBatch([(d[0], d[1]) for d in part], J=m.J, dual=m.dual, targets=targets, device=dev)

    def eval_epoch(self, data, task, bs, accuracy=False, dense=False, group=None):
        """test_with_mnb(model, data, task, criterion, cuda, bs, mean, std, logger) (scripts/test_mnb.py:25-92): new
        meters, evaluate per batch, then eval_result(accuracy, group) -- one host read for the whole set."""
        self.reset_eval()
        for batch in self._batches(data, task, bs, dense):
            self.evaluate(batch)
        return self.eval_result(accuracy, group)

    def train_epoch(self, data, task, bs, dense=False):
        """train_with_mnb (scripts/train_mnb.py:25-94): new RunningAverages, one step per batch in list order (the
        reference's shuffle is off in its own call too); returns (losses.val, error.val), read once at the end.
        The optimizer is not reset: the drivers build a new one per epoch themselves (reset_optimizer())."""
        self.reset_running()
        for batch in self._batches(data, task, bs, dense):
            self(batch)
        s = self.stats.tolist()
        return s[2], s[3]


# graphs per hgnn_ccn_small_train / hgnn_ccn2_small_train dispatch (csrc/ccn_small.hip CS_TRAIN_GMAX,
# csrc/ccn2_small.hip Q_TRAIN_GMAX)
CCN_TRAIN_MAX_GRAPHS = 4096
# Whether fused=None takes hgnn_ccn2_small_train for CCN_2D.  Decided by the same-process A/B of
# tools/ab_ccn_train.py --order 2 ("The CCN-2D loop without the host"): the kernel's median per graph
# against the unfused loop's.
CCN2_TRAIN_FUSED_DEFAULT = True
# The same decision per optimizer for the kernels' sgd / adam instantiations (hgnn_ccn_small_train_opt,
# hgnn_ccn2_small_train_opt): (order, optimizer) -> whether fused=None takes the fused kernel.  From
# profiles/ccn_train_optim_ab.json (tools/ab_ccn_train.py --optim ...): fused where the fused median is at or below
# the unfused median.
CCN_TRAIN_FUSED_OPTIM = {(1, "sgd"): True, (1, "adam"): True, (2, "sgd"): True, (2, "adam"): True}
# Mini-batch mode (batch_size=B): whether fused=None takes hgnn_ccn_small_train_batch where it is supported.  From
# profiles/ccn_train_batch_ab.json (tools/ab_ccn_train.py --batch 32 256): fused only if the fused median is at or
# below the pieces route's at both batch sizes; otherwise the pieces route is the default and the kernels stay
# reachable with fused=True.
CCN_TRAIN_BATCH_FUSED_DEFAULT = True
# The same question for CCN_2D and hgnn_ccn2_small_train_batch (fused="ccn2_batch").  Off: fused=None keeps CCN_2D
# mini-batches on the pieces route, which tests/test_gpu_ccn_train_batch.py pins.  The measured A/B
# (tools/ab_ccn_train.py --order 2 --batch 32 256, profiles/ccn_train_batch_ab.json, DESIGN.md "CCN-2D mini-batch
# kernels"), median (min, max) ms per graph of one run: kernels 0.0094 (0.0092, 0.0095) against pieces 0.0115
# (0.0103, 0.0137) at B = 32, 0.0016 (0.0016, 0.0017) against 0.0018 (0.0018, 0.0019) at B = 256 -- below the pieces
# at both sizes, by 1.23 and 1.09 times (1.09 and 1.08 in a repeat of the run).  Switching the default is a later
# change, and one that must also change tests/test_gpu_ccn_train_batch.py.
CCN2_TRAIN_BATCH_FUSED_DEFAULT = False
# Whether fused=None takes the spill instantiation of the CCN-1D kernels (fused="ccn1_spill": hgnn_ccn_small_spill_train
# and hgnn_ccn_small_spill_train_batch, the row arrays in a global workspace) on chunks the LDS kernels refuse.  Off:
# fused=None keeps such chunks on "unfused" / "batch", which tests/test_gpu_ccn_train.py and
# tests/test_gpu_ccn_train_batch.py pin.  The measured A/B (tools/ab_ccn_train.py --spill,
# profiles/ccn_train_spill_ab.json, DESIGN.md "CCN-1D small graphs past the LDS bound"), median (min, max) ms per graph:
# (a) the routes it replaces, 256 three_collinear_points(n_max=50) graphs, CCN_1D(5, 2, 2, 8), classification: the loop
# 0.5868 (0.5857, 0.5876) against unfused 0.3651 (0.3613, 0.4875); B = 32: 0.0565 (0.0562, 0.0567) against the pieces'
# 0.0206 (0.0181, 0.0225); B = 256: 0.0078 (0.0077, 0.0081) against 0.0059 (0.0055, 0.0071) -- the spill route LOSES at
# every setting (1.6, 2.7 and 1.3 times: dense 49-node graphs, eight levels of dependent L2 round trips in one
# workgroup per graph).  Recommendation: leave it off; take it where one dispatch per chunk matters more than the time
# (a captured epoch).  (b) its price on shapes the LDS kernels take, the 256 QM9-shape graphs, CCN_1D(5, 1, 2, 2): the
# loop 0.0310 (0.0308, 0.0311) against 0.0287 (0.0287, 0.0288), B = 32: 0.0015 (0.0015, 0.0016) against 0.0017
# (0.0017, 0.0019).
# Switching the default is a later change, and one that must also change those tests.
CCN1_TRAIN_SPILL_DEFAULT = False


class CcnTrainStep(_Optimizer):
    """The per-graph training loop of scripts/train_ccn.py:31-73 for a CCN_1D / CCN_2D drop-in model, and
    the evaluation loop of scripts/test_ccn.py:23-67, without host round trips.

    The reference runs, per graph: the normalised target, net(X, A + I), the MAE and MSE meters (.item()
    twice), backward and one Adamax step.  step(X, adj, n_batch, y) runs exactly that sequence over the
    graphs of a padded batch in index order -- graph g + 1 sees the weights graph g left:

      fused    hgnn_ccn_small_train: one dispatch for the whole list (CCN_1D within the small-graph bounds:
               graphs of <= 64 nodes, input_feats and hidden_size <= 8)
      fused2d  hgnn_ccn2_small_train: the same for CCN_2D (graphs of <= 32 nodes, input_feats <= 8,
               hidden_size <= 2, n_outputs <= 256); its one-graph workspace is allocated once per nmax and kept
      fused_spill  hgnn_ccn_small_spill_train: the CCN_1D kernel with its row-sized arrays (the levels, dcoll, dF) in a
               global workspace region instead of LDS -- fused="ccn1_spill", every CCN_1D chunk within
               hgnn_ccn_small_spill_train_supported (graphs of <= 64 nodes, input_feats and hidden_size <= 8, <= 15
               layers, whatever the depth).  The LDS kernel's arithmetic in its order: the same bits where both
               exist.  Its one row region is allocated once per nmax and kept
      unfused  per graph forward_batch on the one-graph slice, hgnn_mse_loss, autograd backward and
               hgnn_optim_step: the same arithmetic from the separate entry points (larger graphs, wider
               channels)

    fused=None takes a fused kernel wherever hgnn_ccn_small_train_supported or hgnn_ccn2_small_train_supported
    allows it (the latter by CCN2_TRAIN_FUSED_DEFAULT, the measured default), fused=False never; fused=True means
    the CCN_1D kernel and raises where that is not supported (so for every CCN_2D model), fused="ccn2" means the
    CCN_2D kernel and raises likewise; fused="ccn1_spill" means the spill instantiation, whatever nmax (also where
    the LDS kernel would fit): it raises in the constructor on a model it cannot take (CCN_2D, wider channels, more
    layers) and in step() on a chunk padded beyond 64 nodes, and its evaluate / eval_epoch go through
    forward_batch(small="spill").  After each step, .path says which ran.  No path synchronises with the host.

    A graph the fused kernel rejects (missing self loop, asymmetric pattern, n_b outside [0, nmax]) takes no
    step and updates no meter; the error shows at the next check (hgnn_amd.net.check_errors(), or at once
    under HGNN_STRICT=1).  step_count still counts it, so later step sizes then differ from a run without it.

    Classification (the reference's `mean == 0` branch, train_ccn.py:39-41, 56-57, the generated-data driver
    scripts/main_generate_ccn.py): classification=True, or classification=None with t_mean == 0.0 as in
    TrainStep.  y then holds one class index per graph, the loss is nn.CrossEntropyLoss on the graph's output
    viewed as (1, n_outputs), and the MAE meters stats[1] and stats[3] are never written.  The fused paths are
    hgnn_ccn_small_train_xent and hgnn_ccn2_small_train_xent, the unfused path uses hgnn_xent_loss with n = 1.  A target that is not an
    integer in [0, n_outputs) raises the class-target error at the next check (the next step,
    check_targets(), or at once under HGNN_STRICT=1) on both paths, which otherwise differ on such a graph:
    a fused kernel skips it like a rejected graph (no step), the unfused path does what TrainStep does (the
    row's dout is zero and the Adamax step is still taken, on zero gradients).

    Limit of fused=None / True: the LDS kernels' backward layout bounds the graph size by the depth (42 nodes at
    CCN_1D(5, 2, 2, 2), 31 at the generated driver's CCN_1D(5, 2, 2, 10), 22 at hidden 8 with 4 layers), and a chunk is
    padded to its largest graph, so one larger graph sends the whole chunk to "unfused" (mini-batch mode: "batch").
    fused="ccn1_spill" has no such term: it takes those chunks in one dispatch (mini-batch mode: two per
    mini-batch) at the price of global-memory rows.  It is opt-in (CCN1_TRAIN_SPILL_DEFAULT, the measured A/B beside
    it).

    optimizer="adamax" (default) | "sgd" | "adam" and momentum (see _Optimizer; scripts/main_ccn.py:155-162): the
    fused paths are then hgnn_ccn_small_train_opt / hgnn_ccn2_small_train_opt, the same kernels with their optimizer
    stage instantiated for it, and the unfused path calls hgnn_optim_step.  Routing is the same; fused=None takes
    a fused kernel for sgd / adam by CCN_TRAIN_FUSED_OPTIM, the measured default.

    Mini-batches: batch_size=B (an integer >= 1; None, the default, is everything above, unchanged).  step() then
    cuts the G graphs into consecutive mini-batches of B, the last one shorter, and takes ONE optimizer step per
    mini-batch, its graphs in parallel and all seeing the same weights: regression -- nn.MSELoss over the (B, n_out)
    block of outputs and normalised targets, dout = 2 (out - yn) / (B n_out), meters as TrainStep's (stats[0:2] the
    mini-batch's MSE and MAE, stats[2:4] their RunningAverages, updated once per mini-batch); classification --
    nn.CrossEntropyLoss on the (B, n_out) logits, dout = (softmax - onehot) / B.  The parameter gradients are summed
    over the mini-batch's graphs; step_count grows by one per mini-batch (the bias corrections use it); a shorter last
    mini-batch divides by its own size; an empty slot (n_b = 0) is a graph like any other (its output is fc.bias).
    .path:

      batch_fused  hgnn_ccn_small_train_batch: two dispatches per mini-batch (one workgroup per graph: forward, its
                   dout row, backward; then one wave per parameter element: the sum over the graphs, the gradient, the
                   optimizer update, the meters) -- CCN_1D within hgnn_ccn_small_train_batch_supported, B <= 4096
      batch_fused2d  hgnn_ccn2_small_train_batch: the same two dispatches for CCN_2D (one workgroup per graph: one
                   plan, forward, its dout row, backward without dX, in the graph's own workspace region; then the
                   sums over the mini-batch's nodes and graphs, the gradient, the optimizer update, the meters) --
                   fused="ccn2_batch", CCN_2D within hgnn_ccn2_small_train_batch_supported (graphs of <= 32 nodes,
                   input_feats <= 8, hidden_size <= 2, n_outputs <= 256), B <= 4096.  Its workspace holds batch_size
                   graph regions (about 0.8 MB each at 29 nodes, two layers, hidden 2: about 200 MB at B = 256),
                   allocated once per nmax and kept
      batch_fused_spill  hgnn_ccn_small_spill_train_batch: batch_fused's two dispatches with the row arrays of each
                   workgroup in its own global region -- fused="ccn1_spill" with batch_size, bounds as fused_spill.
                   The workspace holds batch_size row regions (nmax^2 (hidden layers + 2 max(input_feats, hidden) +
                   2 hidden) floats each: 0.25 MB at 50 nodes, CCN_1D(5, 2, 2, 8)), allocated once per nmax and kept
      batch        the library's pieces per mini-batch: forward_batch, hgnn_mse_loss on the device-normalised target
                   with (0, 1) (or hgnn_xent_loss), autograd backward, hgnn_optim_step -- CCN_2D, larger graphs, wider
                   channels.  The same arithmetic bit for bit where both routes exist.

    fused=None takes batch_fused where it is supported and CCN_TRAIN_BATCH_FUSED_DEFAULT (the measured default) says
    so, fused=False never, fused=True raises where it is not supported (so for every CCN_2D model), fused="ccn2" (the
    per-graph kernel) raises.  fused="ccn2_batch" means the CCN-2D mini-batch kernels: it needs batch_size, raises in
    the constructor on a model they do not take and in step() on a chunk padded beyond their bound; fused=None keeps
    CCN_2D on the pieces (CCN2_TRAIN_BATCH_FUSED_DEFAULT, the measured A/B beside it).  No route synchronises with
    the host.  A graph the fused kernels reject (validation
    bits, or a class target that is no index) makes its whole mini-batch take no step and update no meter; the other
    graphs' out rows are written, the error shows at the next check, and step_count still counts the mini-batch (its
    step number is consumed: the device decides, the host cannot know).
    """

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, t_mean=None, t_std=1.0,
                 fused=None, classification=None, optimizer="adamax", momentum=0.9, batch_size=None):
        from models.compnets.model_ccn import _CCN
        self._check_optimizer(optimizer)
        if batch_size is not None and (isinstance(batch_size, bool) or not isinstance(batch_size, int)
                                       or batch_size < 1):
            raise RuntimeError(f"hgnn_amd: batch_size={batch_size!r}: expected None (the per-graph loop) or an "
                               "integer >= 1")
        if batch_size is not None and isinstance(fused, str) and fused == "ccn2":
            raise RuntimeError("hgnn_amd: fused=\"ccn2\" with batch_size: \"ccn2\" is the per-graph CCN-2D kernel; "
                               "the CCN-2D mini-batch kernels are fused=\"ccn2_batch\" (fused=None or False runs "
                               "CCN_2D mini-batches from the library's pieces)")
        if batch_size is None and isinstance(fused, str) and fused == "ccn2_batch":
            raise RuntimeError("hgnn_amd: fused=\"ccn2_batch\" needs batch_size (the per-graph CCN-2D kernel is "
                               "fused=\"ccn2\")")
        self.batch_size = batch_size
        if not isinstance(model, _CCN):
            raise RuntimeError("hgnn_amd: CcnTrainStep needs a CCN_1D / CCN_2D model (TrainStep is the GNN step)")
        if isinstance(fused, str) and fused == "ccn1_spill":  # host-only, like the next
            cfg = model._spec().config(1, 1)
            if not L.lib().hgnn_ccn_small_spill_train_supported(ctypes.byref(cfg)):
                raise RuntimeError("hgnn_amd: fused=\"ccn1_spill\" needs CCN_1D with input_feats and hidden_size <= 8, "
                                   "<= 15 layers and n_outputs <= 1088 (hgnn_ccn_small_spill_train_supported)")
        if isinstance(fused, str) and fused == "ccn2_batch":  # a host-only question: asked before the device's
            cfg = model._spec().config(1, 1)
            if not L.lib().hgnn_ccn2_small_train_batch_supported(ctypes.byref(cfg)):
                raise RuntimeError("hgnn_amd: fused=\"ccn2_batch\" needs CCN_2D with input_feats <= 8, hidden_size "
                                   "<= 2 and n_outputs <= 256 (hgnn_ccn2_small_train_batch_supported)")
        # the reference's rule (train_ccn.py:39): mean == 0 marks generated (classification) data
        if classification is None:
            classification = t_mean is not None and float(t_mean) == 0.0
        self.classification = bool(classification)
        if self.classification and model.n_outputs < 2:
            raise RuntimeError("hgnn_amd: classification needs n_outputs >= 2 (cross-entropy over one class is "
                               "identically 0); pass t_mean != 0 or classification=False for regression")
        if t_mean is None:
            if not self.classification:
                raise RuntimeError("hgnn_amd: CcnTrainStep needs the target statistics t_mean and t_std")
            t_mean = 0.0
        self.model = model
        self.params = model._params()
        dev = self.params[0].device
        if dev.type != "cuda":
            raise RuntimeError("hgnn_amd: CcnTrainStep runs on the GPU only (call model.cuda() first)")
        for p in self.params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("hgnn_amd: CcnTrainStep needs contiguous float32 parameters")
        self.lr = float(lr)
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = float(eps)
        self.weight_decay = float(weight_decay)
        self.t_mean = float(t_mean)
        self.t_std = float(t_std)
        self.spec = model._spec()
        self.fused = fused
        if isinstance(fused, str):
            if fused not in ("ccn2", "ccn2_batch", "ccn1_spill"):
                raise RuntimeError(f"hgnn_amd: fused={fused!r}: expected None, False, True, \"ccn2\", "
                                   "\"ccn2_batch\" or \"ccn1_spill\"")
            if fused == "ccn2" and not self._supported2d(1):
                raise RuntimeError("hgnn_amd: fused=\"ccn2\" needs CCN_2D with input_feats <= 8, hidden_size <= 2 "
                                   "and n_outputs <= 256 (hgnn_ccn2_small_train_supported)")
        elif fused and not self._supported(1):
            raise RuntimeError("hgnn_amd: fused=True needs CCN_1D with input_feats and hidden_size <= 8 "
                               "(hgnn_ccn_small_train_supported)")
        self.stats = torch.zeros(4, dtype=torch.float32, device=dev)
        self.out = None
        # "fused", "fused2d", "fused_spill" or "unfused" (mini-batch mode: "batch_fused", "batch_fused2d",
        # "batch_fused_spill" or "batch"): the last step
        self.path = None
        self._ws2d = {}   # nmax -> the CCN-2D kernel's one-graph workspace
        self._ws_batch = None  # hgnn_ccn_small_train_batch's workspace (sized once: it does not depend on nmax)
        self._ws_batch2d = {}  # nmax -> hgnn_ccn2_small_train_batch's workspace (batch_size graph regions)
        self._ws_spill = {}    # (nmax, regions) -> the spill kernels' row regions (1: the loop, batch_size: mini-batches)
        self._grads = [torch.zeros_like(p) for p in self.params]
        self._numel = (ctypes.c_int64 * len(self.params))(*[p.numel() for p in self.params])
        # the target's shift and divisor as fp32 device scalars: (y - mean) / (std + 1e-8), a true division
        self._mean = torch.tensor(self.t_mean, dtype=torch.float32, device=dev)
        self._div = torch.tensor(self.t_std + 1e-8, dtype=torch.float32, device=dev)
        self._targets = _TargetWord(dev)  # the unfused classification path's and evaluate's error word
        self._init_optimizer(optimizer, momentum)

    def reset_running(self):
        """New RunningAverage meters (one pair per train_ccn call, scripts/train_ccn.py:28-29)."""
        self.stats.zero_()

    def _supported(self, nmax):
        cfg = self.spec.config(1, nmax)
        return bool(L.lib().hgnn_ccn_small_train_supported(ctypes.byref(cfg)))

    def _supported2d(self, nmax):
        cfg = self.spec.config(1, nmax)
        return bool(L.lib().hgnn_ccn2_small_train_supported(ctypes.byref(cfg)))

    def _supported_batch(self, nmax, two=False):
        """Whether hgnn_ccn_small_train_batch (two: hgnn_ccn2_small_train_batch) takes mini-batches of this step
        padded to nmax nodes."""
        cfg = self.spec.config(1, nmax)
        name = "hgnn_ccn2_small_train_batch_supported" if two else "hgnn_ccn_small_train_batch_supported"
        return bool(getattr(L.lib(), name)(ctypes.byref(cfg))) and self._batch_host_ok()

    def _batch_host_ok(self):
        """The mini-batch entries' two host-side conditions: a mini-batch is one call's at most; the entries' MSE
        meters are hgnn_mse_loss's, which stops dividing below (float)1e-5 where the CCN rule always divides (the
        entries' own fp32 comparison)."""
        f32 = lambda v: struct.unpack("f", struct.pack("f", v))[0]  # noqa: E731
        return self.batch_size <= CCN_TRAIN_MAX_GRAPHS and (self.classification
                                                            or f32(self.t_std + 1e-8) >= f32(1e-5))

    def _supported_spill(self, nmax):
        """Whether the spill kernels take chunks of this step padded to nmax nodes (mini-batch mode: with
        _batch_host_ok)."""
        cfg = self.spec.config(1, nmax)
        if not L.lib().hgnn_ccn_small_spill_train_supported(ctypes.byref(cfg)):
            return False
        return self.batch_size is None or self._batch_host_ok()

    def _route_spill(self, nmax):
        if not self._supported_spill(nmax):
            what = "" if self.batch_size is None else f"batch_size = {self.batch_size} at "
            raise RuntimeError(f"hgnn_amd: fused=\"ccn1_spill\", but {what}nmax = {nmax} is outside the spill kernels' "
                               "bounds (hgnn_ccn_small_spill_train_supported: graphs of <= 64 nodes)")
        return "fused_spill" if self.batch_size is None else "batch_fused_spill"

    def _route_batch(self, nmax):
        """The path of a chunk padded to nmax nodes in mini-batch mode."""
        fused = self.fused
        if fused == "ccn1_spill":
            return self._route_spill(nmax)
        if fused is None:
            if CCN_TRAIN_BATCH_FUSED_DEFAULT and self._supported_batch(nmax):
                return "batch_fused"
            return "batch_fused2d" if CCN2_TRAIN_BATCH_FUSED_DEFAULT and self._supported_batch(nmax, True) else "batch"
        if fused == "ccn2_batch":
            if not self._supported_batch(nmax, True):
                raise RuntimeError(f"hgnn_amd: fused=\"ccn2_batch\", but batch_size = {self.batch_size} at nmax = "
                                   f"{nmax} is outside the CCN-2D mini-batch kernels' bounds "
                                   "(hgnn_ccn2_small_train_batch_supported)")
            return "batch_fused2d"
        if fused:
            if not self._supported_batch(nmax):
                raise RuntimeError(f"hgnn_amd: fused=True, but batch_size = {self.batch_size} at nmax = {nmax} is "
                                   "outside the mini-batch kernels' bounds (hgnn_ccn_small_train_batch_supported)")
            return "batch_fused"
        return "batch"

    def _route(self, nmax):
        """The path of a chunk padded to nmax nodes."""
        if self.batch_size is not None:
            return self._route_batch(nmax)
        fused = self.fused
        if fused == "ccn1_spill":
            return self._route_spill(nmax)
        if fused is None:
            one = CCN_TRAIN_FUSED_OPTIM.get((1, self.optimizer), True)
            two = CCN_TRAIN_FUSED_OPTIM.get((2, self.optimizer), CCN2_TRAIN_FUSED_DEFAULT)
            if one and self._supported(nmax):
                return "fused"
            return "fused2d" if two and self._supported2d(nmax) else "unfused"
        if fused == "ccn2":
            if not self._supported2d(nmax):
                raise RuntimeError(f"hgnn_amd: fused=\"ccn2\", but nmax = {nmax} is outside the CCN-2D kernel's "
                                   "bounds (hgnn_ccn2_small_train_supported)")
            return "fused2d"
        if fused:
            if not self._supported(nmax):
                raise RuntimeError(f"hgnn_amd: fused=True, but nmax = {nmax} is outside the fused kernel's bounds "
                                   "(hgnn_ccn_small_train_supported)")
            return "fused"
        return "unfused"

    def _inputs(self, X, adj, n_batch, y):
        from .ccn import _check_shapes
        from .net import _f32, _i64, _require_cuda
        _require_cuda([X, adj, n_batch, y, *self.params], "CCN training step")
        X, adj = _f32(X), _f32(adj)
        n_batch = None if n_batch is None else _i64(n_batch)
        _check_shapes(self.spec, self.params, X, adj, n_batch)
        G, n_out = X.shape[0], self.spec.n_out
        if self.classification:
            if y.numel() != G:
                raise RuntimeError(f"hgnn_amd: class targets {tuple(y.shape)} do not match {G} graphs")
            return X, adj, n_batch, y.to(torch.float32).reshape(G).contiguous()
        if y.numel() != G * n_out:
            raise RuntimeError(f"hgnn_amd: targets {tuple(y.shape)} do not match {G} graphs x {n_out} outputs")
        return X, adj, n_batch, y.to(torch.float32).reshape(G, n_out).contiguous()

    def step(self, X, adj, n_batch, y):
        """One reference step per graph of the padded batch (forward_batch's layout: adj with self loops),
        in index order; y: raw targets (G,) or (G, n_out) -- classification: G class indices of any dtype.
        Returns the device tensor `stats` = [loss, mae, running loss, running mae] after the last graph; leaves
        .out (G, n_out), the output each graph saw before its own update, and p.grad = the last graph's
        gradients.
        Mini-batch mode (batch_size=B): one step per mini-batch of B consecutive graphs, the last one shorter;
        `stats` after the last mini-batch, .out the output each graph saw before its mini-batch's update, p.grad
        the last mini-batch's gradients."""
        self._targets.poll(block=False)
        X, adj, n_batch, y = self._inputs(X, adj, n_batch, y)
        G, nmax = X.shape[0], X.shape[1]
        self.path = path = self._route(nmax)  # before the work: a strict check inside it may raise
        self.out = torch.empty(G, self.spec.n_out, dtype=torch.float32, device=X.device)
        if path in ("batch_fused", "batch_fused2d", "batch_fused_spill"):
            self._step_batch_fused(X, adj, n_batch, y, two=path == "batch_fused2d",
                                   spill=path == "batch_fused_spill")
        elif path in ("batch", "unfused"):
            self._step_pieces(X, adj, n_batch, y, self.batch_size if path == "batch" else 1)
        else:
            self._step_fused(X, adj, n_batch, y, two=path == "fused2d", spill=path == "fused_spill")
        return self.stats

    def _workspace2d(self, nmax, dev):
        ws = self._ws2d.get(nmax)
        if ws is None:
            cfg = self.spec.config(1, nmax)
            ws = torch.empty(L.lib().hgnn_ccn2_small_train_workspace_bytes(ctypes.byref(cfg)), dtype=torch.uint8,
                             device=dev)
            self._ws2d[nmax] = ws
        return ws

    def _workspace_spill(self, nmax, regions, dev):
        """The spill kernels' row regions for chunks padded to nmax nodes (hgnn_ccn_small_spill_workspace_bytes with
        bs = 1: the training entries use the regions only), allocated once per (nmax, regions) and kept, like
        _ws_batch2d."""
        ws = self._ws_spill.get((nmax, regions))
        if ws is None:
            cfg = self.spec.config(1, nmax)
            ws = torch.empty(L.lib().hgnn_ccn_small_spill_workspace_bytes(ctypes.byref(cfg), regions),
                             dtype=torch.uint8, device=dev)
            self._ws_spill[(nmax, regions)] = ws
        return ws

    def _step_fused(self, X, adj, n_batch, y, two=False, spill=False):
        from .ccn import _word
        from .net import _capturing, check_errors, strict
        lib = L.lib()
        check_errors(block=False)
        dev = X.device
        stream = L.stream_handle(dev)
        b1, b2 = self.betas
        # order 2: the kernel's one-graph workspace goes before the error word
        ws = (L.ptr(self._workspace2d(X.shape[1], dev)),) if two else ()
        adamax = self.optimizer == "adamax" and not spill
        name = "hgnn_ccn2_small_train" if two else "hgnn_ccn_small_train"
        name += ("_xent" if self.classification else "") if adamax else "_opt"
        if spill:  # one entry for every optimizer and loss (the _opt form); its one row region before the error word
            name = "hgnn_ccn_small_spill_train"
            ws = (L.ptr(self._workspace_spill(X.shape[1], 1, dev)),)
        entry = getattr(lib, name)
        for g0 in range(0, X.shape[0], CCN_TRAIN_MAX_GRAPHS):
            g1 = min(g0 + CCN_TRAIN_MAX_GRAPHS, X.shape[0])
            cfg = self.spec.config(g1 - g0, X.shape[1])
            if not adamax:
                # the per-step scalars in double on the host, as hgnn_optim_step forms its own; pinned
                sc = torch.tensor(self._step_scalars(self.step_count, g1 - g0),
                                  dtype=torch.float32).pin_memory().to(dev, non_blocking=True)
                err, tag = _word.next(dev)
                s1, s2 = self._states()
                L.check(entry(ctypes.byref(cfg), self._kind, int(self.classification), L.ptr(X[g0:g1]),
                              L.ptr(adj[g0:g1]), L.ptr(None if n_batch is None else n_batch[g0:g1]), L.ptr(y[g0:g1]),
                              self.t_mean, self.t_std, L.ptr_array(self.params), L.ptr_array(self._grads), s1, s2,
                              L.ptr(sc), self._b1(), b2, self.eps, self.weight_decay, L.ptr(self.stats),
                              L.ptr(self.out[g0:g1]), *ws, err, tag, stream), name)
                self.step_count += g1 - g0
                continue
            # the step sizes in double on the host, as hgnn_adamax_step forms its own; pinned, so the copy
            # does not wait for the stream
            clr = torch.tensor([self.lr / (1.0 - b1 ** t) for t in range(self.step_count + 1,
                                                                         self.step_count + 1 + g1 - g0)],
                               dtype=torch.float32).pin_memory().to(dev, non_blocking=True)
            err, tag = _word.next(dev)
            head = (ctypes.byref(cfg), L.ptr(X[g0:g1]), L.ptr(adj[g0:g1]),
                    L.ptr(None if n_batch is None else n_batch[g0:g1]), L.ptr(y[g0:g1]))
            tail = (L.ptr_array(self.params), L.ptr_array(self._grads), L.ptr_array(self.exp_avg),
                    L.ptr_array(self.exp_inf), L.ptr(clr), b1, b2, self.eps, self.weight_decay, L.ptr(self.stats),
                    L.ptr(self.out[g0:g1]), *ws, err, tag, stream)
            if self.classification:
                L.check(entry(*head, *tail), name)
            else:
                L.check(entry(*head, self.t_mean, self.t_std, *tail), name)
            self.step_count += g1 - g0
        for p, g in zip(self.params, self._grads):
            p.grad = g
        if strict() and not _capturing():
            _word.check(True)

    def _workspace_batch2d(self, nmax, dev):
        """hgnn_ccn2_small_train_batch's workspace for chunks padded to nmax nodes: batch_size graph regions of about
        0.8 MB each at nmax = 29, layers = 2, hidden = 2 (so about 200 MB at batch_size = 256), allocated once per
        nmax and kept, like the per-graph kernel's _ws2d."""
        ws = self._ws_batch2d.get(nmax)
        if ws is None:
            cfg = self.spec.config(CCN_TRAIN_MAX_GRAPHS, nmax)
            ws = torch.empty(L.lib().hgnn_ccn2_small_train_batch_workspace_bytes(ctypes.byref(cfg), self.batch_size),
                             dtype=torch.uint8, device=dev)
            self._ws_batch2d[nmax] = ws
        return ws

    def _step_batch_fused(self, X, adj, n_batch, y, two=False, spill=False):
        """Mini-batch mode, hgnn_ccn_small_train_batch (two: hgnn_ccn2_small_train_batch, spill:
        hgnn_ccn_small_spill_train_batch): one call per run of whole mini-batches within the entry's 4096-graph
        bound."""
        from .ccn import _word
        from .net import _capturing, check_errors, strict
        lib = L.lib()
        check_errors(block=False)
        dev = X.device
        stream = L.stream_handle(dev)
        B, G = self.batch_size, X.shape[0]
        name = "hgnn_ccn2_small_train_batch" if two else "hgnn_ccn_small_train_batch"
        if spill:
            name = "hgnn_ccn_small_spill_train_batch"
        entry = getattr(lib, name)
        if two:
            ws = self._workspace_batch2d(X.shape[1], dev)
        else:
            if self._ws_batch is None:
                # the layout does not depend on nmax; spill: asked at nmax = 1, where the LDS predicate of this
                # query holds for every model the spill kernels take
                cfg = self.spec.config(CCN_TRAIN_MAX_GRAPHS, 1 if spill else X.shape[1])
                self._ws_batch = torch.empty(lib.hgnn_ccn_small_train_batch_workspace_bytes(ctypes.byref(cfg), B),
                                             dtype=torch.uint8, device=dev)
            ws = self._ws_batch
        # spill: the mini-batch's row regions go after the workspace
        rows = (L.ptr(self._workspace_spill(X.shape[1], B, dev)),) if spill else ()
        span = CCN_TRAIN_MAX_GRAPHS // B * B
        s1, s2 = self._states()
        for g0 in range(0, G, span):
            g1 = min(g0 + span, G)
            k = -(-(g1 - g0) // B)  # mini-batches of this call: one step number each, applied or not
            cfg = self.spec.config(g1 - g0, X.shape[1])
            # the per-step scalars in double on the host, as hgnn_optim_step forms its own; pinned
            sc = torch.tensor(self._step_scalars(self.step_count, k),
                              dtype=torch.float32).pin_memory().to(dev, non_blocking=True)
            err, tag = _word.next(dev)
            L.check(entry(
                ctypes.byref(cfg), B, self._kind, int(self.classification), L.ptr(X[g0:g1]), L.ptr(adj[g0:g1]),
                L.ptr(None if n_batch is None else n_batch[g0:g1]), L.ptr(y[g0:g1]), self.t_mean, self.t_std,
                L.ptr_array(self.params), L.ptr_array(self._grads), s1, s2, L.ptr(sc), self._b1(), self.betas[1],
                self.eps, self.weight_decay, L.ptr(self.stats), L.ptr(self.out[g0:g1]), L.ptr(ws), *rows, err,
                tag, stream), name)
            self.step_count += k
        for p, g in zip(self.params, self._grads):
            p.grad = g
        if strict() and not _capturing():
            _word.check(True)

    def _step_pieces(self, X, adj, n_batch, y, B):
        """One step per B consecutive graphs from the library's own pieces: forward_batch, hgnn_mse_loss on the
        device-normalised target with (0, 1) -- n = B n_out -- or hgnn_xent_loss with n = B rows of n_out classes
        (B = 1: the output viewed as (1, n_out), train_ccn.py:57), autograd backward, hgnn_optim_step.  B = 1 is
        the per-graph loop (path "unfused"), B = batch_size the mini-batch mode (path "batch")."""
        lib = L.lib()
        m = self.model
        stream = L.stream_handle(X.device)
        cls = self.classification
        if not cls:
            yn = (y - self._mean) / self._div  # train_ccn.py:42, on the device: no per-graph host work
        n_out = self.spec.n_out
        for g0 in range(0, X.shape[0], B):
            g1 = min(g0 + B, X.shape[0])
            for p in self.params:
                p.grad = None
            out = m.forward_batch(X[g0:g1], adj[g0:g1], None if n_batch is None else n_batch[g0:g1])
            dout = torch.empty_like(out)
            if cls:
                L.check(lib.hgnn_xent_loss(L.ptr(out.detach()), L.ptr(y[g0:g1]), g1 - g0, n_out, L.ptr(self.stats),
                                           L.ptr(dout), L.ptr(self._targets.dev), stream), "cross-entropy loss")
            else:
                L.check(lib.hgnn_mse_loss(L.ptr(out.detach()), L.ptr(yn[g0:g1]), (g1 - g0) * n_out, 0.0, 1.0,
                                          L.ptr(self.stats), L.ptr(dout), stream), "mse loss")
            torch.autograd.backward(out, dout)
            grads = [p.grad for p in self.params]
            if any(gr is None for gr in grads):
                raise RuntimeError("hgnn_amd: a parameter received no gradient")
            self._optim_step(lib, grads, stream)
            self.out[g0:g1].copy_(out.detach())
        if cls:  # the word is sticky: one look after the list (HGNN_STRICT=1: a host sync here, none per graph)
            self._targets.watch()

    def check_targets(self):
        """Raise if a classification step or evaluation saw a target outside [0, n_outputs) (host sync): the
        unfused path's and evaluate's error word, then the fused kernel's (hgnn_amd.net.check_errors())."""
        from .net import check_errors
        self._targets.check()
        check_errors()

    def evaluate(self, X, adj, n_batch, y):
        """scripts/test_ccn.py:34-67 on a padded batch: one forward_batch, then the device tensor
        [losses.avg, error.avg] (the plain means over the graphs of the per-graph MSE and MAE).
        Classification: [losses.avg, 0, accuracy] -- the mean per-graph cross entropy, error.avg as the
        reference leaves it, and the fraction of graphs whose argmax is the target (hgnn_ccn_eval_xent)."""
        X, adj, n_batch, y = self._inputs(X, adj, n_batch, y)
        with torch.no_grad():
            if self.fused == "ccn1_spill":
                # one row region per graph of a call: slices that stay below the one-shot workspace cap
                m = self.spec.spill_max_batch(X.shape[1])
                out = torch.cat([self.model.forward_batch(X[g:g + m], adj[g:g + m],
                                                          None if n_batch is None else n_batch[g:g + m], small="spill")
                                 for g in range(0, X.shape[0], m)]).contiguous()
            else:
                out = self.model.forward_batch(X, adj, n_batch).contiguous()
        if self.classification:
            self._targets.poll(block=False)
            res = torch.empty(3, dtype=torch.float32, device=X.device)
            L.check(L.lib().hgnn_ccn_eval_xent(L.ptr(out), L.ptr(y), X.shape[0], self.spec.n_out, L.ptr(res),
                                               L.ptr(self._targets.dev), L.stream_handle(X.device)),
                    "hgnn_ccn_eval_xent")
            self._targets.watch()
            return res
        res = torch.empty(2, dtype=torch.float32, device=X.device)
        L.check(L.lib().hgnn_ccn_eval_loss(L.ptr(out), L.ptr(y), X.shape[0], self.spec.n_out, self.t_mean,
                                           self.t_std, L.ptr(res), L.stream_handle(X.device)), "hgnn_ccn_eval_loss")
        return res

    def _chunks(self, data, task, chunk):
        """The reference's list of 7-tuples (X, A, targets, ...) as padded device chunks: A + I
        (train_ccn.py:36), each chunk padded to its largest graph."""
        dev = self.params[0].device
        f = self.spec.f_in
        for c0 in range(0, len(data), chunk):
            part = data[c0:c0 + chunk]
            nmax = max(int(d[0].shape[0]) for d in part)
            X = torch.zeros(len(part), nmax, f)
            A = torch.zeros(len(part), nmax, nmax)
            nb = torch.empty(len(part), dtype=torch.int64)
            y = torch.empty(len(part), 1)  # one value per graph: targets[task].view(1)
            for b, d in enumerate(part):
                n = int(d[0].shape[0])
                X[b, :n] = d[0].detach().cpu()
                A[b, :n, :n] = d[1].detach().cpu() + torch.eye(n)
                nb[b] = n
                y[b, 0] = d[2][task]
            yield X.to(dev), A.to(dev), nb.to(dev), y.to(dev)

    def _epoch_chunks(self, data, task, chunk):
        """The padded device chunks of one epoch, graphs in order 0 .. len - 1 (train_ccn.py's for i in range(n)).
        data: the reference's list of 7-tuples (_chunks), a hgnn_amd.dataset.GraphPack (gathered on the host,
        vectorised) or a hgnn_amd.dataset.DevicePack on the model's device (built there by hgnn_pack_ccn_chunk,
        no host work per graph) -- the same bytes from all three."""
        from .dataset import DevicePack, GraphPack
        dev = self.params[0].device
        if isinstance(data, DevicePack):
            if data.device != dev:
                raise RuntimeError(f"hgnn_amd: DevicePack on {data.device}, model on {dev}")
            return data.ccn_chunks(range(len(data)), chunk, task)
        if isinstance(data, GraphPack):
            return data.ccn_chunks(range(len(data)), chunk, task, device=dev)
        return self._chunks(data, task, chunk)

    @staticmethod
    def _check_pack(data):
        # after the read that ends the epoch: the stream is drained, the error word costs no extra wait
        from .dataset import DevicePack
        if isinstance(data, DevicePack):
            data.check()

    def train_epoch(self, data, task, chunk=1024):
        """train_ccn(net, data, task, ...) (scripts/train_ccn.py:24-73): one step per graph in list order, new
        meters; returns (losses.val, error.val), read once at the end.  Classification: targets[task] is the
        class index, n_outputs >= 2, and error.val is the 0.0 the reference's untouched meter returns.
        data: a list of instances, a GraphPack or a DevicePack (_epoch_chunks).
        Mini-batch mode: one step per mini-batch; chunk is rounded down to a multiple of batch_size (and at least
        to batch_size), so the mini-batches are runs of batch_size consecutive graphs of the data order whatever
        the chunking."""
        if self.spec.n_out != 1 and not self.classification:
            raise RuntimeError("hgnn_amd: train_epoch takes one target per graph (targets[task].view(1))")
        if self.batch_size is not None:
            chunk = max(self.batch_size, chunk // self.batch_size * self.batch_size)
        self.reset_running()
        for X, A, nb, y in self._epoch_chunks(data, task, chunk):
            self.step(X, A, nb, y)
        s = self.stats.tolist()
        self._check_pack(data)
        return (s[2], 0.0) if self.classification else (s[2], s[3])

    def eval_epoch(self, data, task, chunk=1024, accuracy=False):
        """test_ccn(ccn, data, task, ...) (scripts/test_ccn.py:23-67): (losses.avg, error.avg) over the list;
        the chunks' means weighted by their graph counts, as AverageMeter.update(v, 1) per graph does.
        Classification: (losses.avg, 0.0) as the reference returns; accuracy=True adds the accuracy as a third
        value.  data: as train_epoch takes it."""
        if accuracy and not self.classification:
            raise RuntimeError("hgnn_amd: eval_epoch(accuracy=True) needs a classification step")
        if self.spec.n_out != 1 and not self.classification:
            raise RuntimeError("hgnn_amd: eval_epoch takes one target per graph (targets[task].view(1))")
        acc = None
        for X, A, nb, y in self._epoch_chunks(data, task, chunk):
            r = self.evaluate(X, A, nb, y).double() * X.shape[0]
            acc = r if acc is None else acc + r
        if acc is None:
            return (0.0, 0.0, 0.0) if accuracy else (0.0, 0.0)
        s = (acc / len(data)).tolist()
        self._check_pack(data)
        return (s[0], s[1], s[2]) if accuracy else (s[0], s[1])
