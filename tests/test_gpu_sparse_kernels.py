"""The sparse side one kernel at a time: the batch plan, the three structure-extraction kernels, the pack / unpack
kernels (csrc/struct.hip) and the aggregation forward and backward (csrc/agg.hip), against plain numpy references.

Through the probes of csrc/probe_sparse.hip (include/hgnn_amd.h "Kernel probes") every launcher is handed what the
whole-network tests never present: operator rows of 63 .. 130 entries (the second iteration of the 64-entry chunk
loops, which in k_agg_fwd_rpw is separate code from the prefetched first chunk), G and P lists of different length
in one row, empty rows, row counts around one block, every lane layout (CPL 1, 2, 4, 8; vector and guarded scalar),
J_tot 3 / 4 / 7, the diagonal I / D mode, dense blocks at the register kernel's limits and past the LDS kernel's.
tests/sparse_probe_util.py holds the inputs, the case tables and the checks; tests/test_sparse_probe_inputs.py
checks those on the CPU (the exact families are exact, the tables hold every listed edge, the checks fail on a
dropped entry, swapped Pm / Pd, a shifted slice).

Every aggregation case:
  * exact families A1 / A3: the output equals the fp64 result bit for bit (the sign of a zero aside);
  * family AR: rms and max error against fp64 at most 2 x those of the naive fp32 form (sequential in entry order,
    product rounded, then the sum; BN on load as sub, div, mul, add) -- the fp64-leg factor of oracle/parity.py;
  * containment: outputs pre-filled with a sentinel keep it in rows >= total, in the columns the launch does not
    write and in the padding under pad_from = -1;
  * poison: NaN in the feature rows past the source's total, in the columns of ing / inp outside the blocks read, in
    unused entry slots (column 0, NaN coefficients) and in the list rows >= total -- no output may turn non-finite.
Every extraction case: the kernel launch_extract reports (extract_variant, which launch_extract itself dispatches
on), node_off / edge_off / totals, all six lists against the numpy builder (counts, starts, entries bit for bit,
the sentinel everywhere else), the packed inputs, and the validation word -- 0, or exactly the bit of the one
invalid input.  N_b = nmax + 1 is put on the graph that holds nmax real nodes: k_plan sets ERR_SIZES and clamps the
count to nmax, the graph's true size, so the pad and mask checks, which run on the clamped count, add no bit.

Which extraction kernel ran for which shape (asserted; default switches | HGNN_EXTRACT_REG=0 | HGNN_EXTRACT_LDS=0):
  dual J_tot 3, nmax 9, emax 25            register-staged (2) | LDS-staged (1) | general (0)
  dual J_tot 4, nmax 32, emax 64           register-staged (2) | LDS-staged (1) | general (0)
  dual J_tot 5, nmax 6, emax 8             LDS-staged (1)      | LDS-staged (1) | general (0)
  GNN_simple J_tot 3, nmax 70 (complete)   LDS-staged (1)      | LDS-staged (1) | general (0)
  dual J_tot 3, nmax 12, emax 130          general (0)         | general (0)    | general (0)

No case failed when the file first ran, under the default switches or under the five switch groups: no kernel
fault was found, so no kernel changed here.  (Mutants of the kernels -- Pm / Pd swapped in k_agg_fwd_rpw's second
chunk, the last entry of a second chunk dropped in k_agg_fwd, 9-entry rows cut to 8 in agg_bwd_g, swapped
coefficients in agg_bwd_p's second chunk, swapped Pm / Pd in k_extract_reg's transposed list, a dropped last
dense row in extract_cols and a dropped first entry of lds_rows' second chunk -- each fail their tests here.)

Family AR, measured on an MI355X (error against fp64 of the kernel / of the naive fp32 form; the largest ratio
over the cases of a row decides the assertion; the bound is 2.00):

  kernel      width            cases  rms kernel / naive   max kernel / naive   worst ratio rms, max
  forward     cg 5, cp 1           2  6.27e-07 / 6.21e-07  4.25e-06 / 3.68e-06  1.01, 1.15
  forward     cg 64, cp 64         6  7.28e-07 / 6.97e-07  9.78e-06 / 6.58e-06  1.04, 1.49
  forward     cg 100, cp 100       2  7.49e-07 / 7.65e-07  1.49e-05 / 1.22e-05  0.98, 1.22
  forward     cg 128, cp 128       8  7.68e-07 / 7.78e-07  1.72e-05 / 1.34e-05  0.99, 1.29
  forward     cg 256, cp 256       3  6.07e-07 / 6.32e-07  1.18e-05 / 1.22e-05  0.96, 0.97
  forward     cg 512, cp 64        1  7.46e-07 / 7.73e-07  1.73e-05 / 1.35e-05  0.97, 1.28
  forward     cg 130, cp 0         5  7.67e-07 / 7.90e-07  1.52e-05 / 1.23e-05  0.98, 1.23
  forward     cg 0, cp 64          2  6.61e-07 / 6.75e-07  7.84e-06 / 7.84e-06  0.98, 1.00
  forward     cg 64, cp 0 (j0 2)   1  5.31e-07 / 5.46e-07  7.50e-06 / 6.89e-06  0.97, 1.09
  forward     cg 128, cp 0 (j0 2)  1  5.77e-07 / 6.20e-07  6.73e-06 / 9.83e-06  0.93, 0.68
  forward     cg 256, cp 0 (j0 2)  1  5.23e-07 / 5.44e-07  1.35e-05 / 9.64e-06  0.96, 1.40
  backward G  c 5                  4  2.89e-06 / 2.60e-06  2.11e-05 / 1.73e-05  1.11, 1.22
  backward G  c 64                 4  5.25e-06 / 5.27e-06  6.30e-05 / 5.92e-05  1.00, 1.06
  backward G  c 100                4  2.15e-06 / 2.11e-06  3.97e-05 / 3.20e-05  1.02, 1.24
  backward G  c 128                4  2.19e-06 / 2.26e-06  3.59e-05 / 2.70e-05  1.00, 1.33
  backward G  c 256                4  5.01e-06 / 5.00e-06  7.18e-05 / 7.03e-05  1.00, 1.02
  backward G  c 512                2  2.21e-06 / 2.22e-06  3.97e-05 / 3.58e-05  1.00, 1.11
  backward P  c 5                  2  1.65e-06 / 1.67e-06  1.20e-05 / 1.39e-05  0.99, 0.86
  backward P  c 64                 2  1.47e-06 / 1.46e-06  1.88e-05 / 1.88e-05  1.01, 1.00
  backward P  c 100                2  1.51e-06 / 1.51e-06  1.72e-05 / 1.72e-05  1.00, 1.00
  backward P  c 128                2  1.31e-06 / 1.31e-06  1.53e-05 / 1.34e-05  1.00, 1.14
  backward P  c 256                2  1.47e-06 / 1.48e-06  1.86e-05 / 1.80e-05  0.99, 1.03
  backward P  c 512                2  1.55e-06 / 1.57e-06  3.46e-05 / 2.70e-05  0.99, 1.28
  (each row shows the case with the worst ratio; rows of J_tot 3, 4 and 7, with and without BN on load, are
  merged per width.  The kernels sum in entry order like the naive form, with a fused multiply-add, so the ratios
  sit near 1; the max ratio is one element's error and scatters.  A dropped entry of one 130-entry row measures
  above 10^4 x.)
"""

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sparse_probe_util as U

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- aggregation forward
@pytest.mark.parametrize("cg,cp", U.FWD_WIDTHS)
def test_agg_forward(cg, cp):
    cases = [c for c in U.fwd_cases() if (c["cg"], c["cp"]) == (cg, cp)]
    assert cases
    for c in cases:
        U.check_fwd(c)


def test_agg_forward_odd_ldo_takes_the_scalar_path_with_equal_output():
    for fam, jt in (("A1", 3), ("AR", 3), ("AR", 4)):
        c = dict(cg=128, cp=128, jtot=jt, total=37, cap=48, fam=fam, bn=3, pad=0, j0=0, ldo=0, seed=77)
        K = U.fwd_geometry(c)[0]
        _, vec = U.check_fwd(c)
        _, sca = U.check_fwd(dict(c, ldo=K + 5))
        assert np.array_equal(vec[:37, :K].view(np.int32), sca[:37, :K].view(np.int32))


def test_agg_forward_refusals():
    c = dict(cg=128, cp=128, jtot=3, total=37, cap=48, fam="A1", bn=0, pad=0, j0=0, ldo=0, seed=78)
    d = U.fwd_data(c)
    for over in (dict(cg=513), dict(cp=513), dict(jtot=8), dict(jtot=2)):
        st, out, _, _ = U.call_fwd(d, overrides=over)
        assert st == 2 and U.sentinel(out), over      # HGNN_ERR_UNSUPPORTED, nothing launched
    st, out, _, _ = U.call_fwd(d, overrides=dict(cap_rows=0))
    assert st == 0 and U.sentinel(out)


@pytest.mark.parametrize("c", U.DIAG_WIDTHS)
def test_agg_forward_diagonal_mode(c):
    cases = [x for x in U.diag_cases() if x["cg"] == c]
    assert cases
    for x in cases:
        U.check_fwd(x)


def test_agg_forward_diagonal_mode_error_word_and_refusals():
    c = dict(cg=64, cp=64, jtot=4, total=100, cap=112, fam="A1", bn=0, pad=0, j0=2, ldo=0, seed=79)
    d = U.fwd_data(c)
    st, base, dbase, err = U.call_fwd(d)
    assert st == 0 and err == 0
    g = d["g"]
    assert g["cnt"][80] == 70 and g["cols"][80, 65] == 80
    # one off-diagonal entry with a nonzero v_0 (v_1): in the second chunk of the 70-entry row, and in a first chunk
    r1 = next(r for r in range(100) if 2 <= g["cnt"][r] <= 60 and g["cols"][r, 0] != r)
    for (r, e, j) in ((80, 67, 0), (80, 3, 1), (r1, 0, 1)):
        assert g["cols"][r, e] != r
        keep = g["vals"][r, e, j]
        g["vals"][r, e, j] = 1.0
        U.relist(g)
        st, out, dg, err = U.call_fwd(d)
        assert st == 0 and err == U.ERR_DIAG_ID, (r, e, j, err)
        # slices 0 and 1 are not aggregated: the outputs are the valid operator's
        assert np.array_equal(out.view(np.int32), base.view(np.int32)) and np.array_equal(dg.view(np.int32), dbase.view(np.int32))
        g["vals"][r, e, j] = keep
    U.relist(g)
    assert U.call_fwd(d)[3] == 0
    assert U.call_fwd(d, with_err=False)[0] == 1                   # diag without err: HGNN_ERR_ARG
    st, out, _, _ = U.call_fwd(d, overrides=dict(cg=512))          # wider than the diagonal form is built for
    assert st == 2 and U.sentinel(out)
    st, out, _, _ = U.call_fwd(d, overrides=dict(cp=128))          # P of another width
    assert st == 2 and U.sentinel(out)
    assert U.call_fwd(d, overrides=dict(j0=1))[0] == 1


# ---------------------------------------------------------------------------------------------- aggregation backward
@pytest.mark.parametrize("c", U.BWD_WIDTHS)
def test_agg_backward(c):
    cases = [x for x in U.bwd_cases() if x["c"] == c]
    assert cases
    for x in cases:
        U.check_bwd(x)


@pytest.mark.parametrize("pc", U.PAIR_CASES, ids=U.case_id)
def test_agg_backward_pair(pc):
    U.check_pair(pc)


def test_agg_backward_refusals():
    L = U._L()
    dg, dp = U.pair_data(U.PAIR_CASES[0])
    keep = []
    og, op = U._up(dg["out0"]), U._up(dp["out0"])
    a, b = U.bwd_struct(dg, keep, og), U.bwd_struct(dp, keep, op)
    both = U.bwd_struct(dg, keep, og)
    both.inp, both.p, both.ldp, both.pofs_m, both.pofs_d = b.inp, b.p, b.ldp, b.pofs_m, b.pofs_d
    neither = U.bwd_struct(dg, keep, og)
    neither.ing = None
    for p in (both, neither):
        assert L.lib().hgnn_probe_agg_bwd(ctypes.byref(p), None, 0, U._stream()) == 1
    a.jtot = 8
    assert L.lib().hgnn_probe_agg_bwd(ctypes.byref(a), None, 0, U._stream()) == 2
    a.jtot, a.c = 3, 513
    assert L.lib().hgnn_probe_agg_bwd(ctypes.byref(a), None, 0, U._stream()) == 2
    torch.cuda.synchronize()
    assert np.array_equal(og.cpu().numpy().view(np.int32), dg["out0"].view(np.int32))


# ---------------------------------------------------------------------------------------------- extraction
@pytest.mark.parametrize("s", U.EXTRACT_SHAPES, ids=lambda s: s["name"])
def test_extract(s):
    U.check_extract(s, s["variant"])


@pytest.mark.parametrize("s", U.EXTRACT_SHAPES, ids=lambda s: s["name"])
def test_extract_flags_exactly_the_invalid_input(s):
    for inv in U.invalid_kinds(s):
        U.check_extract(s, s["variant"], inv)


def test_extract_without_validation_or_packing():
    """validate = 0 leaves the word 0 on an invalid batch; without X / XL nothing is packed."""
    s = U.EXTRACT_SHAPES[0]
    b = U.extract_batch(s, invalid="pm_pad")
    res = U.call_extract(b, validate=0, with_x=False)
    assert res["status"] == 0 and int(res["err"][0]) == 0
    U.check_lists("novalidate", res["rows"], res["ents"], U.dense_lists(b))


def test_extract_equals_host_builder():
    """The device extraction of prepare_batch's dense batch against the hgnn_csr_batch_build image of the same
    graphs: the same rows, columns and values (the image's lists are compact, so `start` is dropped)."""
    from test_builder import _graphs
    from functions.batching import prepare_batch
    from functions.operators import graph_operators
    from hgnn_amd.csr import CsrBatch
    gs = _graphs(n_qm9=6, n_sbm=1)
    data = [[X, A, t, *graph_operators([X, A], 1, True)] for X, A, t in gs]
    X, W, T, XL, WL, Pm, Pd, mask, mask_lg, Nb, Eb = [t.numpy() for t in prepare_batch(data, 0, 1)]
    b = dict(bs=len(gs), nmax=W.shape[1], emax=WL.shape[1], jtot=3, dual=1, f=X.shape[1], W=W, WL=WL, Pm=Pm, Pd=Pd,
             mask=mask, mask_lg=mask_lg, X=X, XL=XL, Nb=Nb, Eb=Eb)
    res = U.call_extract(b)
    assert res["status"] == 0 and int(res["err"][0]) == 0
    host = CsrBatch([(X_, A_) for X_, A_, _ in gs], J=1, dual=True, device="cpu")
    assert res["totals"][:2].tolist() == [host.nodes, host.edges]
    assert np.array_equal(res["xo"][:host.nodes].view(np.int32), host.x.numpy().view(np.int32))
    for k, (hrows, hent) in enumerate(host.lists()):
        drows, dent = res["rows"][k], res["ents"][k]
        nc = 2 if k >= 4 else 3
        assert np.array_equal(drows[:len(hrows), 1], hrows[:, 1]), (k, "counts")
        for r in range(len(hrows)):
            (hs, n), ds = hrows[r], drows[r, 0]
            assert np.array_equal(dent[ds:ds + n, :1 + nc].view(np.int32), hent[hs:hs + n, :1 + nc].view(np.int32)), (k, r)


@pytest.mark.parametrize("f", [1, 5, 64])
def test_pack_unpack(f):
    L = U._L()
    g = np.random.default_rng(f)
    bs, nmax, emax = 5, 9, 25
    nb, eb = np.array([0, 1, 9, 4, 7]), np.array([0, 1, 25, 7, 18])
    n_off = np.concatenate([[0], np.cumsum(nb)]).astype(np.int32)
    e_off = np.concatenate([[0], np.cumsum(eb)]).astype(np.int32)
    X = np.full((bs, f, nmax), U.NAN, np.float32)
    XL = np.full((bs, 1, emax), U.NAN, np.float32)
    for i in range(bs):
        X[i, :, :nb[i]] = g.standard_normal((f, nb[i]))
        XL[i, 0, :eb[i]] = g.standard_normal(eb[i])
    dn, de, dX, dXL = U._up(n_off), U._up(e_off), U._up(X), U._up(XL)
    xo = torch.full((bs * nmax, f), U.SENT, device=U._dev())
    xlo = torch.full((bs * emax,), U.SENT, device=U._dev())
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert L.lib().hgnn_probe_pack_nodes(p(dX), bs, f, nmax, p(dn), p(xo), U._stream()) == 0
    assert L.lib().hgnn_probe_pack_edges(p(dXL), bs, emax, p(de), p(xlo), U._stream()) == 0
    back = torch.full((bs + 1, f, nmax), U.SENT, device=U._dev())
    packed = torch.full((bs * nmax, f), U.NAN, device=U._dev())    # rows past the total: never read
    want = np.full((bs * nmax, f), U.SENT, np.float32)
    wantl = np.full(bs * emax, U.SENT, np.float32)
    dense = np.zeros((bs, f, nmax), np.float32)
    for i in range(bs):
        want[n_off[i]:n_off[i + 1]] = X[i, :, :nb[i]].T
        wantl[e_off[i]:e_off[i + 1]] = XL[i, 0, :eb[i]]
        dense[i, :, :nb[i]] = X[i, :, :nb[i]]
    packed[:n_off[-1]] = torch.from_numpy(want[:n_off[-1]]).to(U._dev())
    assert L.lib().hgnn_probe_unpack_nodes(p(packed), bs, f, nmax, p(dn), p(back), U._stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(xo.cpu().numpy().view(np.int32), want.view(np.int32))
    assert np.array_equal(xlo.cpu().numpy().view(np.int32), wantl.view(np.int32))
    back = back.cpu().numpy()
    # the padding is +0.0, the values bit for bit, the block past the batch untouched
    assert np.array_equal(back[:bs].view(np.int32), dense.view(np.int32)) and U.sentinel(back[bs])


# ---------------------------------------------------------------------------------------------- switches
def test_switch_selected_variants():
    """The kernel variants only a switch selects (the default process covers HGNN_AGG_RPW=2 and the default
    extraction dispatch), each group in a fresh child process, one after another; the first child that fails -- a
    nonzero status, a signal or the time limit -- fails the test and no further child is started."""
    for name, (extra, mode, variants) in U.SWITCH_GROUPS.items():
        env = {k: v for k, v in os.environ.items() if not k.startswith("HGNN_")}
        env.update(extra)
        env["HGNN_STRICT"] = "1"
        cmd = [sys.executable, os.path.join(REPO, "tests", "sparse_probe_worker.py"), mode]
        if variants is not None:
            cmd.append(",".join(str(v) for v in variants))
        try:
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"{name}: the worker ran into its time limit: {str(e.stderr)[-2000:]}")
        assert r.returncode == 0, (name, r.returncode, r.stderr[-2000:])
