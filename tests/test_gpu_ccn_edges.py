"""The general CCN path (csrc/ccn.hip and the files it names: plan kernels, CCN-1D, the k_c2_* templates, the _big
kernels, the readout) at its kernel-selection and degree boundaries, against the fp64 oracle (oracle/ref_ccn.py)
with the same oracle in fp32 as the naive leg.  tests/ccn_edge_util.py holds the graphs, the case tables, the weight
families, the mirror of the dispatch and the checks; tests/test_ccn_edge_inputs.py checks all of those on the CPU.

Everything runs through forward_batch with hgnn_amd.ccn.SMALL = False.  Every case:
  * outputs, dX and each parameter gradient: the kernel's rms and max error against fp64 are each at most 2 x those
    of the fp32 oracle, plus one fp32 ulp of the tensor's largest magnitude (the factor of oracle/parity.py and
    tests/test_gpu_gemm_kernels.py); elements that are exactly zero in the fp64 oracle (dead channels, padding)
    must be exactly zero;
  * dX rows at and beyond n_b are exactly zero (the autograd binding allocates dX itself, so it cannot be handed in
    pre-filled; k_ccn_unpack_dx writes every row of it);
  * part A (TINY: graphs of 1, 4, 6, 7, 5 nodes and an empty slot; family M): every channel selection of the
    CCN-2D templates and of CCN-1D's one-chunk / chunked branches; the empty slot's output is fc.bias bit for bit and
    its dX rows are zero (of the parameters it reaches fc.bias alone, through out = fc.bias, as in the oracle);
  * part B (family S: outputs and all gradients; family R: outputs): degrees 64 / 65 / 130 / 256 for CCN-2D, 64 / 65 /
    129 / 1024 for CCN-1D; the 64 / 65 graphs under both plans (hgnn_ccn_plan_async and, with ASYNC_PLAN_BOUND
    set to zero, hgnn_ccn_plan); the degree-65 graph in a ragged batch with TINY; the per-graph drop-in forward equal
    to the batched one within 1e-6; the refusals above 256 / 1024;
  * part C: plan_maps bit-exact against a numpy restatement of receptive_fields / positions at multi-word rows.

Measured on an MI355X (one row per case: the tensor with the worst ratio; ratio = error over bound, scaled so that
2.00 is the limit; rms and max as kernel / fp32 oracle; "both": under the async and the sync plan, whose results
agreed bit for bit in every case, so one row stands for both):

  order graphs            channels    fam plan  worst      ratio  rms kernel / naive   max kernel / naive
  ccn2d TINY              f1h2L2o1    M       w1.weight   0.92  1.82e-05 / 1.61e-05  3.60e-05 / 3.60e-05
  ccn2d TINY              f8h3L3o3    M       w2.bias     1.33  8.26e-06 / 2.10e-06  1.42e-05 / 3.07e-06
  ccn2d TINY              f9h8L2o8    M       dX          0.78  1.72e-06 / 1.67e-06  1.08e-05 / 1.01e-05
  ccn2d TINY              f16h9L2o3   M       fc.bias     0.50  3.85e-08 / 3.94e-08  5.96e-08 / 5.96e-08
  ccn2d TINY              f8h16L2o1   M       dX          1.01  2.60e-07 / 1.80e-07  1.76e-06 / 1.26e-06
  ccn2d TINY              f16h16L3o8  M       w2.weight   0.68  2.67e-05 / 4.39e-05  1.94e-04 / 2.23e-04
  ccn1d TINY              f8h8L2o1    M       w1.weight   0.73  8.73e-07 / 9.79e-07  5.27e-06 / 5.27e-06
  ccn1d TINY              f9h2L2o3    M       w2.weight   0.67  1.65e-06 / 2.11e-06  3.80e-06 / 3.80e-06
  ccn1d TINY              f2h9L3o8    M       dX          1.16  1.83e-06 / 1.21e-06  8.84e-06 / 3.83e-06
  ccn1d TINY              f17h12L2o3  M       w2.weight   0.99  2.15e-06 / 2.20e-06  1.11e-05 / 7.33e-06
  ccn2d lolli(63,1)       f5h2L2o8    S both  dX          0.59  2.23e+01 / 4.08e+01  9.48e+01 / 1.45e+02
  ccn2d lolli(63,1)       f5h2L2o8    R both  out         0.25  4.95e+03 / 2.08e+04  1.03e+04 / 3.90e+04
  ccn2d lolli(63,1)       f9h3L2o8    S both  dX          0.72  2.36e+01 / 2.47e+01  7.08e+01 / 1.00e+02
  ccn2d lolli(63,1)       f9h3L2o8    R both  out         0.17  1.14e+03 / 6.08e+03  2.93e+03 / 1.52e+04
  ccn2d lolli(63,1)       f5h12L2o8   S both  dX          0.61  3.86e+01 / 3.12e+01  1.23e+02 / 1.87e+02
  ccn2d lolli(63,1)       f5h12L2o8   R both  out         1.09  2.64e+03 / 2.20e+03  6.57e+03 / 3.99e+03
  ccn2d lolli(64,2)       f5h2L2o8    S both  w1.bias     0.22  2.71e-02 / 1.17e-01  3.58e-02 / 1.45e-01
  ccn2d lolli(64,2)       f5h2L2o8    R both  out         0.27  9.66e+03 / 3.53e+04  2.19e+04 / 7.64e+04
  ccn2d lolli(64,2)       f9h3L2o8    S both  dX          0.39  3.08e+01 / 4.65e+01  9.26e+01 / 2.47e+02
  ccn2d lolli(64,2)       f9h3L2o8    R both  out         0.25  2.95e+03 / 1.19e+04  5.51e+03 / 2.01e+04
  ccn2d lolli(64,2)       f5h12L2o8   S both  dX          0.54  4.12e+01 / 4.39e+01  1.35e+02 / 2.21e+02
  ccn2d lolli(64,2)       f5h12L2o8   R both  out         0.17  3.54e+03 / 1.66e+04  5.66e+03 / 2.87e+04
  ccn2d 4xstar(130)       f5h2L2o8    S       dX          0.89  9.64e-02 / 1.06e-01  3.63e+00 / 3.10e+00
  ccn2d 4xstar(130)       f5h2L2o8    R       out         0.77  5.71e-01 / 5.79e-01  1.69e+00 / 1.96e+00
  ccn2d 4xstar(130)       f9h3L2o8    S       dX          0.66  2.01e-01 / 3.27e-01  8.12e+00 / 8.25e+00
  ccn2d 4xstar(130)       f9h3L2o8    R       out         0.50  3.33e-01 / 6.32e-01  1.03e+00 / 1.82e+00
  ccn2d 4xstar(130)       f5h12L2o8   S       dX          0.87  3.01e-01 / 3.59e-01  1.04e+01 / 9.99e+00
  ccn2d 4xstar(130)       f5h12L2o8   R       out         0.49  6.50e-01 / 1.32e+00  2.05e+00 / 3.72e+00
  ccn2d star(256)         f1h2L2o8    S       w2.bias     0.23  2.57e-03 / 8.48e-03  3.64e-03 / 1.20e-02
  ccn2d star(256)         f1h2L2o8    R       out         0.14  1.24e-01 / 9.86e-01  2.77e-01 / 1.72e+00
  ccn1d clique(64)        f5h2L2o8    S       dX          1.00  3.47e-03 / 3.29e-03  6.65e-03 / 5.67e-03
  ccn1d clique(64)        f5h2L2o8    R       out         0.93  3.05e-02 / 3.69e-02  7.25e-02 / 7.38e-02
  ccn1d clique(64)        f9h9L2o8    S       dX          0.72  2.92e-03 / 3.13e-03  1.11e-02 / 1.34e-02
  ccn1d clique(64)        f9h9L2o8    R       out         0.21  5.20e-02 / 2.15e-01  9.13e-02 / 4.34e-01
  ccn1d clique(65)        f5h2L2o8    S       dX          0.89  3.34e-03 / 3.70e-03  7.96e-03 / 7.96e-03
  ccn1d clique(65)        f5h2L2o8    R       out         0.17  3.36e-02 / 1.64e-01  5.79e-02 / 3.70e-01
  ccn1d clique(65)        f9h9L2o8    S       dX          1.10  4.74e-03 / 4.54e-03  2.20e-02 / 1.81e-02
  ccn1d clique(65)        f9h9L2o8    R       out         0.13  1.01e-01 / 7.31e-01  1.87e-01 / 1.69e+00
  ccn1d star(129)         f5h2L2o8    S       dX          0.89  5.14e-04 / 5.25e-04  7.65e-03 / 8.14e-03
  ccn1d star(129)         f5h2L2o8    R       out         0.16  6.13e-05 / 3.49e-04  9.91e-05 / 5.69e-04
  ccn1d star(129)         f9h9L2o8    S       w1.weight   1.00  1.68e-03 / 1.64e-03  1.05e-02 / 9.96e-03
  ccn1d star(129)         f9h9L2o8    R       out         0.32  9.52e-05 / 2.86e-04  1.65e-04 / 4.61e-04
  ccn1d star(1024)        f5h2L2o8    S       dX          1.00  9.48e-03 / 9.44e-03  5.49e-01 / 5.46e-01
  ccn1d star(1024)        f5h2L2o8    R       out         0.31  1.09e-02 / 3.86e-02  2.42e-02 / 7.10e-02
  ccn1d star(1024)        f9h9L2o8    S       dX          0.96  1.13e-03 / 1.14e-03  5.97e-02 / 6.02e-02
  ccn1d star(1024)        f9h9L2o8    R       out         0.39  6.43e-03 / 1.47e-02  1.15e-02 / 2.92e-02
  ccn2d lolli(64,2)+TINY  f5h2L2o8    S       dX          0.39  5.97e+00 / 1.13e+01  3.56e+01 / 7.54e+01
  ccn2d lolli(64,2)+TINY  f5h2L2o8    R       out         0.12  6.55e+02 / 5.27e+03  3.17e+03 / 2.21e+04
  ccn2d lolli(63,2)       f5h2L2o8    S both  w2.bias     0.52  1.04e-02 / 1.73e-02  1.47e-02 / 2.44e-02
  ccn2d lolli(63,2)       f5h2L2o8    R both  out         0.33  2.76e+03 / 7.58e+03  5.42e+03 / 1.46e+04

What the star cases found.  Before k_ccn2_bwd_node_big summed its row sums, trace, bias partial and level-0 G[a] in
fp64, one star(130) measured dX 16.60 / 1.15 / 4.24 for the three channel sets and star(256) dX 8.53, w1.bias 5.68,
w2.bias 2.72: the hub's dX row was 34 ulp off (184 at star(256); the fp32 oracle 1.6 ulp), w1.bias 3-6 ulp.  No term was
wrong (a dropped block measures far above that, tests/test_ccn_edge_inputs.py): fp32 sums of n^2 / 256 terms a thread
and n-term LDS float atomics whose one result multiplies a whole row or the whole matrix.  The atomics also made
the large-degree backward depend on scheduling: the async and sync plans of lolli(64,2) differed in bits then.
One star(130) at (9, 3, 2), family R, measured 2.66 on its 8 outputs, which all hang on one hub (ccn_edge_util.py
B_COPIES); the batch now holds four stars.
"""

import numpy as np
import pytest
import torch

import ccn_edge_util as U

pytestmark = pytest.mark.gpu


def _plans(name):
    c = U.BY_NAME[name]
    return ("async", "sync") if c["graphs"] == (c["graphs"][0],) and c["graphs"][0] in U.BOTH_PLANS else (None,)


def _empty_slots(name, got):
    adjs, _, p, _ = U.inputs(name)
    for b, a in enumerate(adjs):
        if a is None:
            assert torch.equal(got["out"][b], p["fc.bias"]), f"{name}: empty slot {b} is not fc.bias"
            if "dX" in got:
                assert got["dX"][b].abs().sum().item() == 0.0


# ------------------------------------------------------------------------------------------ A: channel selections
@pytest.mark.parametrize("name", [c["name"] for c in U.CASES_A])
def test_channel_selections_on_tiny(name):
    got = U.run_gpu(name)
    U.check(name, got)
    _empty_slots(name, got)


# ------------------------------------------------------------------------------------------ B: degree selections
@pytest.mark.parametrize("name", [c["name"] for c in U.CASES_S])
def test_degree_selections(name):
    """Family S (outputs, dX, parameter gradients) and family R (outputs) of one graph and channel set; the 64 / 65
    graphs under both plans, and their per-graph drop-in forward against the batched one."""
    c = U.BY_NAME[name]
    single = len(c["graphs"]) == 1
    runs, failed = {}, []
    for fam in ("S", "R"):  # every leg is measured (and its table row printed) before anything fails
        nm = name[:-1] + fam
        for plan in _plans(name):
            got = U.run_gpu(nm, plan, per_graph=single and fam == "S")
            runs[fam, plan] = got
            try:
                U.check(nm, got, f" {plan}" if plan else "")
            except AssertionError as e:
                failed.append(str(e))
            _empty_slots(nm, got)
            if "per_graph" in got:
                ref = got["out"]
                err = (got["per_graph"] - ref).abs().max().item()
                assert err <= 1e-6 * max(1.0, ref.abs().max().item()), f"{nm}: per-graph forward differs by {err:.3g}"
    if len(_plans(name)) == 2:  # reported, not required: the two plans size and select differently
        a, s = runs["S", "async"], runs["S", "sync"]
        same = all(torch.equal(a[k], s[k]) for k in a if k != "per_graph")
        print(f"TABLE  {name} async vs sync plan: bits {'equal' if same else 'differ'}")
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("order,graph", U.REFUSALS)
def test_degree_above_the_bound_is_refused(order, graph):
    """star(257) through CCN-2D and star(1025) through CCN-1D: both shapes are above ASYNC_PLAN_BOUND, so the plan
    is the synchronous one, which reads the error word and raises before hgnn_ccn_forward is enqueued."""
    import hgnn_amd.ccn as HC
    from hgnn_amd.net import check_errors
    from models.compnets.model_ccn import CCN_1D, CCN_2D
    a = U.GRAPHS[graph]()
    n = a.shape[0]
    assert U.auto_plan(order, 1, n) == "sync" and n ** 3 > HC.ASYNC_PLAN_BOUND[order]
    assert U.DEGREES[graph][0] == HC.CCN_MAX_DEGREE[order] + 1
    net = (CCN_2D if order == 2 else CCN_1D)(2, 1, 2, 2, False).cuda()
    old = HC.SMALL
    HC.SMALL = False
    try:
        with pytest.raises(RuntimeError, match="degree above the compiled bound"):
            net.forward_batch(torch.randn(1, n, 2).cuda(), a.unsqueeze(0).cuda(), torch.tensor([n]).cuda())
        check_errors()  # nothing pending: the refusal was complete
        # one below the bound passes
        b = U.star(n - 1)
        out = net.forward_batch(torch.randn(1, n - 1, 2).cuda(), b.unsqueeze(0).cuda(), torch.tensor([n - 1]).cuda())
        assert bool(torch.isfinite(out).all())
    finally:
        HC.SMALL = old


# ------------------------------------------------------------------------------------------ C: plan maps
@pytest.mark.parametrize("batch", list(U.plan_batches()))
def test_plan_maps_bit_exact_at_multiword_rows(batch):
    order, adjs = U.plan_batches()[batch]
    maps = U.plan_maps_gpu(order, adjs)
    assert len(maps) == len(adjs)
    for k, (a, (deg, nbr, pos)) in enumerate(zip(adjs, maps)):
        if a is None:
            assert deg.size == 0 and nbr.size == 0 and pos.size == 0
            continue
        rdeg, rnbr, rpos = U.plan_ref(a)
        assert np.array_equal(deg, rdeg), (batch, k)
        assert np.array_equal(nbr, rnbr), (batch, k)
        assert np.array_equal(pos, rpos), (batch, k)
