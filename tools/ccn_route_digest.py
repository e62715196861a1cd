"""One SHA-256 per CCN-1D training route, for comparing two builds of the library bit for bit (run once per library
through HGNN_LIB_PATH and diff the output).

The GPU tests compare routes of one library with each other, so an error shared by both sides of a pair passes them;
this compares a route with itself across libraries.  Each route trains two epochs of CcnTrainStep on 12 seeded
hgnn_amd.datagen graphs of at most 16 nodes and hashes the parameters, the optimizer state, `stats` and `.out`.
Models CCN_1D(5, 1, 2, 2) (MSE) / CCN_1D(5, 2, 2, 2) (cross-entropy) and CCN_1D(7, 2, 5, 3) (both); routes: the fused
loop with each optimizer, fused mini-batches, the spill kernels per graph and in mini-batches, and the pieces
(fused=False: the one-shot forward, backward and reduction) per graph and in mini-batches.  One line per route:
`<model> <loss> <route> <sha256>`.  The tool holds no expectation."""
import hashlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "hgnn-2_amd"), REPO]
import torch  # noqa: E402

ROUTES = [("fused_adamax", dict(fused=True)), ("fused_sgd", dict(fused=True, optimizer="sgd")),
          ("fused_adam", dict(fused=True, optimizer="adam")), ("fused_B4", dict(fused=True, batch_size=4)),
          ("spill", dict(fused="ccn1_spill")), ("spill_B4", dict(fused="ccn1_spill", batch_size=4)),
          ("pieces", dict(fused=False)), ("pieces_B4", dict(fused=False, batch_size=4))]


def inputs(f, n_out, xent):
    import hgnn_amd.datagen as dg
    if xent:
        graphs = [(d[0], d[1], d[2].float()) for d in dg.three_collinear_points(12, n_max=16, d=f, seed=3)]
    else:
        graphs = dg.qm9_shape_dataset(12, seed=5, n_types=f, n_min=5, n_max=16)
    nmax = max(x.shape[0] for x, _, _ in graphs)
    X = torch.zeros(len(graphs), nmax, f)
    A = torch.zeros(len(graphs), nmax, nmax)
    for b, (x, a, _) in enumerate(graphs):
        n = x.shape[0]
        X[b, :n] = x
        A[b, :n, :n] = a + torch.eye(n)
    nb = torch.tensor([x.shape[0] for x, _, _ in graphs], dtype=torch.int64)
    Y = torch.stack([t[:1 if xent else n_out] for _, _, t in graphs])  # a class index, or n_out regression targets
    return X.cuda(), A.cuda(), nb.cuda(), Y.cuda()


def digest(step):
    state = {"sgd": ["momentum_buffer"], "adam": ["exp_avg", "exp_avg_sq"], "adamax": ["exp_avg", "exp_inf"]}
    h = hashlib.sha256()
    tensors = list(step.params) + [t for name in state[step.optimizer] for t in getattr(step, name)]
    for t in tensors + [step.stats, step.out]:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def main():
    from hgnn_amd.train import CcnTrainStep
    from models.compnets.model_ccn import CCN_1D
    for xent in (False, True):
        for shape in ((5, 2 if xent else 1, 2, 2), (7, 2, 5, 3)):
            data = inputs(shape[0], shape[1], xent)
            stats = dict(classification=True) if xent else dict(t_mean=0.3, t_std=1.7)
            for name, kw in ROUTES:
                torch.manual_seed(0)
                step = CcnTrainStep(CCN_1D(*shape).cuda(), lr=1e-2, **stats, **kw)
                for _ in range(2):
                    step.step(*data)
                torch.cuda.synchronize()
                print("CCN_1D" + str(shape), "xent" if xent else "mse", name, step.path, digest(step), flush=True)


if __name__ == "__main__":
    main()
