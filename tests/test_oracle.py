"""Pin the oracle (oracle/ref_mnb.py) to the reference's golden fixtures (CPU only)."""

import numpy as np
import pytest
import torch

import fixture_util as fu
from oracle import ref_mnb as R


def _op_graphs(z):
    return fu.unpack_graphs(z), z["J"]


def test_oracle_graph_operators_bit_exact(golden):
    z = golden("operators")
    graphs, js = _op_graphs(z)
    for k, ((X, A, _), J) in enumerate(zip(graphs, js)):
        if A.shape[0] > 30:  # the O(M^2) loop restatement is for small graphs only
            continue
        W, WL, Pm, Pd = R.graph_operators([X, A], int(J), True)
        for nm, v in (("W", W), ("WL", WL), ("Pm", Pm), ("Pd", Pd)):
            ref = z[f"{nm}_{k}"]
            assert v.shape == ref.shape, (k, nm)
            assert np.array_equal(v.numpy(), ref), (k, nm)


def test_oracle_prepare_batch_bit_exact(golden):
    z = golden("batch")
    graphs = fu.unpack_graphs(z)
    data = []
    for X, A, t in graphs:
        W, WL, Pm, Pd = R.graph_operators([X, A], 1, True)
        data.append([X, A, t, W, WL, Pm, Pd])
    out = R.prepare_batch(data, 0, 1)
    names = ["X", "W", "T", "XL", "WL", "Pm", "Pd", "mask", "mask_lg", "N_batch", "E_batch"]
    for nm, v in zip(names, out):
        assert np.array_equal(v.numpy(), z[nm]), nm


def lg_inputs(z, J=1, dtype=torch.float32, builder=None):
    from functions.operators import graph_operators as prod_ops
    from functions.batching import prepare_batch as prod_batch
    graphs = fu.unpack_graphs(z)
    build = builder or prod_ops
    data = []
    for X, A, t in graphs:
        W, WL, Pm, Pd = build([X, A], J, True)
        data.append([X, A, t, W, WL, Pm, Pd])
    b = list(prod_batch(data, 0, J))
    for i in range(9):
        b[i] = b[i].to(dtype)
    return b


def oracle_params(model_cls_args, seed, dtype=torch.float32, kind="lg"):
    from models.gnns.model_mnb import GNN_lg, GNN_simple
    m = GNN_lg(*model_cls_args) if kind == "lg" else GNN_simple(*model_cls_args)
    fu.det_init(m, seed)
    return {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in m.state_dict().items()}


LG_CASES = ["lg_d16_o1", "lg_d16_o2", "lg_d16_o3", "lg_d8_o2_L2", "lg_d16_o2_L3", "lg_d64_o2"]


@pytest.mark.parametrize("name", LG_CASES)
def test_oracle_gnn_lg_matches_reference(golden, name):
    z = golden(name)
    d, L, order, bs, wseed = [int(v) for v in z["cfg"]]
    X, W, T, XL, WL, Pm, Pd, mask, mask_lg, Nb, Eb = lg_inputs(z)
    p = oracle_params((0, d, L, 5, 1, 1, order), wseed)
    st = R.bn_states(L, 2 * d)
    X.requires_grad_(True)
    W.requires_grad_(True)
    out = R.gnn_lg(p, [X, XL, W, WL, Pm, Pd], Nb, mask, Eb, mask_lg, L, order, st, True)
    loss = torch.nn.MSELoss()(out, T)
    loss.backward()
    ref = z["out"]
    assert np.max(np.abs(out.detach().numpy() - ref)) <= 1e-5 * max(1.0, np.abs(ref).max())
    gmax = max(np.abs(z[k]).max() for k in z.files if k.startswith("grad."))
    for k in z.files:
        if k.startswith("grad."):
            g = p[k[5:]].grad.numpy()
            assert np.all(np.abs(g - z[k]) <= 1e-4 * gmax + 1e-5 * np.abs(z[k])), k
    dxg = X.grad.numpy()
    assert np.max(np.abs(dxg - z["dX"])) <= 1e-4 * max(1.0, np.abs(z["dX"]).max())
    assert np.max(np.abs(W.grad.numpy() - z["dW"])) <= 1e-4 * max(1.0, np.abs(z["dW"]).max())
    for l in range(L - 1):
        for nm in ("bn1", "bn2"):
            s = st[f"layer{l}.{nm}"]
            np.testing.assert_allclose(s["running_mean"].numpy(), z[f"rmean.layer{l}.{nm}"], rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(s["running_std"].numpy(), z[f"rstd.layer{l}.{nm}"], rtol=1e-5, atol=1e-5)


def test_oracle_gnn_simple_matches_reference(golden):
    z = golden("gnn_simple")
    X, W, T, XL, WL, Pm, Pd, mask, mask_lg, Nb, Eb = lg_inputs(z)
    p = oracle_params((0, 2, 20, 5, 1, 1), 201, kind="simple")
    st = R.bn_states(20, 4, kind="simple")
    X.requires_grad_(True)
    out = R.gnn_simple(p, [X, W], Nb, mask, 20, st, True)
    loss = torch.nn.MSELoss()(out, T)
    loss.backward()
    assert np.max(np.abs(out.detach().numpy() - z["out32"])) <= 1e-5 * max(1.0, np.abs(z["out32"]).max())
    gmax = max(np.abs(z[k]).max() for k in z.files if k.startswith("grad32."))
    for k in z.files:
        if k.startswith("grad32."):
            g = p[k[7:]].grad.numpy()
            assert np.all(np.abs(g - z[k]) <= 1e-4 * gmax + 1e-5 * np.abs(z[k])), k


@pytest.mark.parametrize("order,J", [(1, 1), (2, 1), (3, 1), (2, 2)])
def test_oracle_fast_leg_equals_loop_leg(order, J):
    """The batched leg (graph_oper_fast / p_multi_fast), which the full-size GPU parity tests use
    as their fp64 anchor, computes the same function as the reference-order loop leg."""
    import hgnn_amd.datagen as dg
    from functions.batching import prepare_batch
    from functions.operators import graph_operators
    graphs = dg.qm9_shape_dataset(12, seed=70 + order)
    data = [[X, A, t, *graph_operators([X, A], J, True)] for X, A, t in graphs]
    b = prepare_batch(data, 0, J)
    res = []
    for fast in (False, True):
        X, W, T, XL, WL, Pm, Pd, mask, mask_lg, Nb, Eb = [t.double() if t.is_floating_point() else t for t in b]
        p = oracle_params((0, 8, 4, 5, 1, J, order), 31, dtype=torch.float64)
        st = R.bn_states(4, 16, dtype=torch.float64)
        X.requires_grad_(True)
        out = R.gnn_lg(p, [X, XL, W, WL, Pm, Pd], Nb, mask, Eb, mask_lg, 4, order, st, True, fast=fast)
        torch.nn.MSELoss()(out, T).backward()
        res.append((out.detach(), {k: v.grad for k, v in p.items()}, X.grad))
    (o0, g0, x0), (o1, g1, x1) = res
    assert torch.allclose(o0, o1, rtol=1e-12, atol=1e-12)
    for k in g0:
        assert torch.allclose(g0[k], g1[k], rtol=1e-10, atol=1e-12), k
    assert torch.allclose(x0, x1, rtol=1e-10, atol=1e-12)
    s0 = R.bn_states(4, 4, kind="simple", dtype=torch.float64)
    s1 = R.bn_states(4, 4, kind="simple", dtype=torch.float64)
    ps = oracle_params((0, 2, 4, 5, 1, J), 32, kind="simple", dtype=torch.float64)
    X = b[0].double()
    W = b[1].double()
    a = R.gnn_simple(ps, [X, W], b[9], b[7].double(), 4, s0, True)
    c = R.gnn_simple(ps, [X, W], b[9], b[7].double(), 4, s1, True, fast=True)
    assert torch.allclose(a, c, rtol=1e-12, atol=1e-12)


# --------------------------------------------------------------------------- CCN
def ccn_params(kind, k, dtype=torch.float32):
    """Fixture weights: det_init(net, 300 + k) on a CCN of the fixtures' shape (5 -> 1, h=2, L=2)."""
    from models.compnets.model_ccn import CCN_1D, CCN_2D
    net = (CCN_1D if kind == "1d" else CCN_2D)(5, 1, 2, 2, False)
    fu.det_init(net, 300 + k)
    return net, {n: v.detach().to(dtype).clone() for n, v in net.named_parameters()}


def ccn_graphs(z):
    return [(X, A + torch.eye(A.shape[0]), t) for X, A, t in fu.unpack_graphs(z)]


def test_oracle_collapse6to3_matches_reference(golden):
    from oracle import ref_ccn as RC
    z = golden("ccn")
    for d in range(1, 7):
        T = torch.from_numpy(z[f"c6_T_{d}"]).double()
        H = T.permute(3, 0, 1, 2).unsqueeze(4).unsqueeze(5) * torch.eye(d, dtype=torch.float64)
        got = RC.collapse6to3(H)
        ref = torch.from_numpy(z[f"c6_out_{d}"]).double()
        assert torch.allclose(got, ref, rtol=1e-5, atol=1e-5), d


def test_oracle_ccn_receptive_fields_bit_exact(golden):
    from oracle import ref_ccn as RC
    z = golden("ccn")
    for k, (X, adj, _) in enumerate(ccn_graphs(z)):
        nbrs = RC.receptive_fields(adj)
        assert np.array_equal(np.array([len(v) for v in nbrs]), z[f"deg_{k}"]), k
        assert np.array_equal(np.concatenate([np.array(v) for v in nbrs]), z[f"nbr_{k}"]), k
        pos = [q for i in range(len(nbrs)) for j in nbrs[i] for q in RC.positions(nbrs, i, j)]
        assert np.array_equal(np.array(pos), z[f"pos_{k}"]), k


@pytest.mark.parametrize("kind", ["1d", "2d"])
def test_oracle_ccn_matches_reference(golden, kind):
    from oracle import ref_ccn as RC
    z = golden("ccn")
    order = 1 if kind == "1d" else 2
    for k, (X, adj, t) in enumerate(ccn_graphs(z)):
        if f"{kind}_out_{k}" not in z:
            continue
        _, p = ccn_params(kind, k)
        p = {n: v.requires_grad_(True) for n, v in p.items()}
        Xr = X.clone().requires_grad_(True)
        out = RC.ccn_forward(p, Xr, adj, order, 2)
        loss = torch.nn.MSELoss()(out, t[0].view(1))
        loss.backward()
        ref = torch.from_numpy(z[f"{kind}_out_{k}"])
        assert torch.allclose(out.detach(), ref, rtol=1e-5, atol=1e-5), (k, out, ref)
        assert torch.allclose(Xr.grad, torch.from_numpy(z[f"{kind}_dX_{k}"]), rtol=1e-4, atol=1e-5), k
        for n, v in p.items():
            g = torch.from_numpy(z[f"{kind}_grad_{k}.{n}"])
            assert torch.allclose(v.grad, g, rtol=1e-4, atol=1e-5 * max(1.0, g.abs().max().item())), (k, n)


def test_oracle_ccn2_closed_form_matches_literal(golden):
    """The closed-form CCN-2D oracle (used at SBM-200 size, config 5, where the literal d^5 one and
    the reference cannot run) equals the literal restatement -- outputs and every gradient -- on the
    reference fixture graphs and on random SBM graphs (fp64)."""
    from oracle import ref_ccn as RC
    import hgnn_amd.datagen as dg
    z = golden("ccn")
    graphs = ccn_graphs(z)[:6] + [(X, A + torch.eye(A.shape[0]), t) for X, A, t in dg.sbm_dataset(2, n=12, seed=9)]
    for k, (X, A, _) in enumerate(graphs):
        _, p = ccn_params("2d", k, torch.float64)
        pa = {n: v.clone().requires_grad_(True) for n, v in p.items()}
        pb = {n: v.clone().requires_grad_(True) for n, v in p.items()}
        xa = X.double().requires_grad_(True)
        xb = X.double().requires_grad_(True)
        a = RC.ccn_forward(pa, xa, A.double(), 2, 2)
        b = RC.ccn2_forward_closed(pb, xb, A.double(), 2)
        assert torch.equal(RC.ccn2_forward_closed(pb, xb, A.double(), 2, taps=[]), b)  # taps change nothing
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-10), (k, a, b)
        a.sum().backward()
        b.sum().backward()
        assert torch.allclose(xa.grad, xb.grad, rtol=1e-10, atol=1e-10)
        for n in p:
            assert torch.allclose(pa[n].grad, pb[n].grad, rtol=1e-10, atol=1e-10), n


def test_oracle_ccn1_vectorised_matches_literal(golden):
    """The vectorised CCN-1D oracle (used at SBM-400..1000 size, degrees above 64) equals the literal
    restatement -- outputs and every gradient -- on the reference fixture graphs and SBM graphs."""
    from oracle import ref_ccn as RC
    import hgnn_amd.datagen as dg
    z = golden("ccn")
    graphs = ccn_graphs(z)[:6] + [(X, A + torch.eye(A.shape[0]), t) for X, A, t in dg.sbm_dataset(2, n=16, seed=19)]
    for k, (X, A, _) in enumerate(graphs):
        _, p = ccn_params("1d", k, torch.float64)
        pa = {n: v.clone().requires_grad_(True) for n, v in p.items()}
        pb = {n: v.clone().requires_grad_(True) for n, v in p.items()}
        xa = X.double().requires_grad_(True)
        xb = X.double().requires_grad_(True)
        a = RC.ccn_forward(pa, xa, A.double(), 1, 2)
        b = RC.ccn1_forward_vec(pb, xb, A.double(), 2)
        assert torch.equal(RC.ccn1_forward_vec(pb, xb, A.double(), 2, taps=[]), b)  # taps change nothing
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-10), (k, a, b)
        a.sum().backward()
        b.sum().backward()
        assert torch.allclose(xa.grad, xb.grad, rtol=1e-10, atol=1e-10)
        for n in p:
            assert torch.allclose(pa[n].grad, pb[n].grad, rtol=1e-10, atol=1e-10), n
