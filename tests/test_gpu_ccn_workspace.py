"""The bounds of the general CCN path's two workspaces: hgnn_ccn_plan*, hgnn_ccn_forward and hgnn_ccn_backward driven
through ctypes with every buffer they write -- the plan workspace, the feature workspace, out, dX and each parameter
gradient -- a slice of a larger tensor, 256-aligned, between two 4096-byte zones of 0xA5.  After a synchronise every
zone is intact, and out, dX and the gradients are torch.equal to the same batch through forward_batch (the autograd
binding of hgnn_amd/ccn.py, which sizes both workspaces from hgnn_ccn_plan_bytes / hgnn_ccn_workspace_bytes itself).

Cases (graphs of tests/ccn_edge_util.py; path(3) is lolli(1, 2)):
  * CCN-2D, [star(65), path(3), empty slot], nmax 65, f = h = 9, 2 layers, 2 outputs, under hgnn_ccn_plan and
    hgnn_ccn_plan_async: the C2Save / C2Grad regions and the wide kernels;
  * CCN-2D, [star(6), path(3)], nmax 6, f 5, h 2, 2 layers, hgnn_ccn_plan_async: no large-degree regions;
  * CCN-1D, [star(65), path(3), empty slot], f = h = 9, 2 layers, both plans.
The buffers start as 0xA5 bytes too (-2.9e-16 as a float), as torch.empty might hand them out.  Both runs use the same
library and the general path has no order-dependent sums (tests/test_gpu_ccn_edges.py: the two plans agree bit for
bit), so the comparison is exact.
"""

import ctypes

import pytest
import torch

import ccn_edge_util as U

pytestmark = pytest.mark.gpu

ZONE = 4096
FILL = 0xA5

CASES = {
    "ccn2d-star65-f9h9-sync": (2, ("star", 65), True, 9, 9, "sync"),
    "ccn2d-star65-f9h9-async": (2, ("star", 65), True, 9, 9, "async"),
    "ccn2d-star6-f5h2-async": (2, ("star", 6), False, 5, 2, "async"),
    "ccn1d-star65-f9h9-sync": (1, ("star", 65), True, 9, 9, "sync"),
    "ccn1d-star65-f9h9-async": (1, ("star", 65), True, 9, 9, "async"),
}
LAYERS, N_OUT = 2, 2


class Guarded:
    """nbytes at a 256-aligned address inside a tensor of 0xA5 bytes, a zone on either side."""

    def __init__(self, nbytes, dev):
        self.nbytes = nbytes
        self.whole = torch.full((ZONE + 256 + nbytes + ZONE,), FILL, dtype=torch.uint8, device=dev)
        self.start = ZONE + (-(self.whole.data_ptr() + ZONE)) % 256
        assert (self.whole.data_ptr() + self.start) % 256 == 0

    @property
    def ptr(self):
        return ctypes.c_void_p(self.whole.data_ptr() + self.start)

    def data(self, dtype, shape):
        return self.whole[self.start:self.start + self.nbytes].view(dtype).view(shape)

    def intact(self):
        lo = self.whole[self.start - ZONE:self.start]
        hi = self.whole[self.start + self.nbytes:self.start + self.nbytes + ZONE]
        return bool((lo == FILL).all()) and bool((hi == FILL).all())


def _batch(order, graph, empty_slot, f, h):
    adjs = [getattr(U, graph[0])(graph[1]), U.lolli(1, 2)] + ([None] if empty_slot else [])
    g = torch.Generator().manual_seed(65 * order + f)
    xs = [torch.randn(0 if a is None else a.shape[0], f, generator=g) for a in adjs]
    m = 18 if order == 2 else 2
    params = []
    for l in range(LAYERS):
        cin = f if l == 0 else h
        params += [torch.randn(h, m * cin, generator=g) / (m * cin), 0.1 * torch.randn(h, generator=g)]
    params += [torch.randn(N_OUT, f + LAYERS * h, generator=g), 0.1 * torch.randn(N_OUT, generator=g)]
    dout = torch.randn(len(adjs), N_OUT, generator=g)
    X, A, nb = U.pad(adjs, xs)
    return X.cuda(), A.cuda(), nb.cuda(), [p.cuda() for p in params], dout.cuda()


def _through_ctypes(order, X, A, nb, params, dout, plan):
    from hgnn_amd import _lib as L
    lib = L.lib()
    dev = X.device
    bs, nmax, f = X.shape
    h = params[0].shape[0]
    cfg = L.CcnConfig(order, bs, nmax, f, h, LAYERS, N_OUT, 0)
    s = L.stream_handle(dev)
    sums = (ctypes.c_longlong * 4)()
    if plan == "async":
        max_d2 = bs * nmax ** 3
        fn = lib.hgnn_ccn_plan_async
    else:
        deg = (A > 0).sum(-1)
        max_d2 = int((deg * deg).sum().item())
        fn = lib.hgnn_ccn_plan
    bufs = {"plan_ws": Guarded(lib.hgnn_ccn_plan_bytes(ctypes.byref(cfg), max_d2), dev)}
    L.check(fn(ctypes.byref(cfg), L.ptr(A), L.ptr(nb), bufs["plan_ws"].ptr, max_d2, sums, s), "plan")
    if plan == "sync":
        assert list(sums) == [int(deg.sum()), max_d2, int(nb.sum()), int(deg.max())]
    else:
        assert list(sums) == [bs * nmax * nmax, max_d2, bs * nmax, nmax]
    bufs["workspace"] = Guarded(lib.hgnn_ccn_workspace_bytes(ctypes.byref(cfg), sums), dev)
    bufs["out"] = Guarded(4 * bs * N_OUT, dev)
    bufs["dX"] = Guarded(4 * X.numel(), dev)
    for i, p in enumerate(params):
        bufs[f"grad{i}"] = Guarded(4 * p.numel(), dev)
    pa = L.ptr_array(params)
    L.check(lib.hgnn_ccn_forward(ctypes.byref(cfg), sums, L.ptr(X), pa, bufs["plan_ws"].ptr, max_d2,
                                 bufs["workspace"].ptr, bufs["out"].ptr, s), "hgnn_ccn_forward")
    ga = (ctypes.c_void_p * len(params))(*[bufs[f"grad{i}"].ptr.value for i in range(len(params))])
    L.check(lib.hgnn_ccn_backward(ctypes.byref(cfg), sums, pa, bufs["plan_ws"].ptr, max_d2, bufs["workspace"].ptr,
                                  L.ptr(dout), ga, bufs["dX"].ptr, s), "hgnn_ccn_backward")
    torch.cuda.synchronize()
    base = bufs["plan_ws"].ptr.value
    err = int(lib.hgnn_ccn_error_word(ctypes.byref(cfg), ctypes.c_void_p(base), max_d2)) - base
    assert int(bufs["plan_ws"].data(torch.uint8, (-1,))[err:err + 4].view(torch.int32).item()) == 0
    res = {"out": bufs["out"].data(torch.float32, (bs, N_OUT)), "dX": bufs["dX"].data(torch.float32, X.shape)}
    for i, p in enumerate(params):
        res[f"grad{i}"] = bufs[f"grad{i}"].data(torch.float32, p.shape)
    return bufs, res


def _through_forward_batch(order, X, A, nb, params, dout, plan):
    import hgnn_amd.ccn as HC
    spec = HC.CcnSpec(order, X.shape[2], params[0].shape[0], LAYERS, N_OUT)
    ps = [p.clone().requires_grad_(True) for p in params]
    Xr = X.clone().requires_grad_(True)
    old = HC.SMALL, HC.ASYNC_PLAN_BOUND
    HC.SMALL = False
    if plan == "sync":
        HC.ASYNC_PLAN_BOUND = {1: 0, 2: 0}
    else:
        assert U.auto_plan(order, X.shape[0], X.shape[1]) == "async"
    try:
        out = HC.run_ccn(spec, ps, Xr, A, nb)
        out.backward(dout)
        torch.cuda.synchronize()
    finally:
        HC.SMALL, HC.ASYNC_PLAN_BOUND = old
    res = {"out": out.detach(), "dX": Xr.grad}
    for i, p in enumerate(ps):
        res[f"grad{i}"] = p.grad
    return res


@pytest.mark.parametrize("name", list(CASES))
def test_workspaces_stay_inside_their_bounds(name):
    order, graph, empty_slot, f, h, plan = CASES[name]
    batch = _batch(order, graph, empty_slot, f, h)
    bufs, got = _through_ctypes(order, *batch, plan)
    broken = [k for k, b in bufs.items() if not b.intact()]
    assert not broken, f"{name}: bytes written outside {broken}"
    ref = _through_forward_batch(order, *batch, plan)
    assert set(got) == set(ref)
    differ = [k for k in ref if not torch.equal(got[k], ref[k])]
    assert not differ, f"{name}: {differ} differ from forward_batch"
    assert bool(torch.isfinite(ref["out"]).all()) and float(ref["dX"].abs().sum()) > 0.0
