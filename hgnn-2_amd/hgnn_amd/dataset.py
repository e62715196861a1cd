"""On-disk dataset format and ingestion.

The reference keeps datasets as pickled lists of 7-tuples (x, A, t, W, WL, Pm, Pd)
(preprocessing/preprocessing.py:97, functions/data_generator.py:85), splits them
80/10/10 (preprocessing/loading.py:19-37) and builds them from the QM9 `.xyz`
files through rdkit (preprocessing/preprocessing.py:174-275).  Here:

* GraphPack -- a directory of flat `.npy` arrays plus `meta.json`, opened with
  `numpy.load(mmap_mode="r")` (never pickle): packed node features, the
  adjacency as per-graph COO (local i, j, bond order) and the target vectors.
  Only (x, A, t) are stored; the operators W / WL / Pm / Pd are a pure function
  of A and are rebuilt by the native builder when a batch is made, so a pack is
  ~1 % of the pickled 7-tuples (no dense N x N x 3 / M x M x 3 tensors).
* GraphPack.batches -- hgnn_amd.csr.CsrBatch per batch straight from the
  memory-mapped arrays (the executor's layout, csrc/builder.cpp), or the
  reference's dense 11-tuple through functions.batching.prepare_batch.
* DevicePack (GraphPack.to_device) -- the pack resident on the GPU; the same CsrBatch images built there
  by the device batcher (csrc/batcher.hip), with no host work per graph.
* GraphPack.ccn_chunks / DevicePack.ccn_chunk -- the CCN drivers' padded (X, A + I, n_batch, y) chunks, gathered
  in numpy or built on the GPU (csrc/ccn_pack.hip).
* prepare_experiment_sets -- the reference split, same sizes and order.
* read_xyz / molecule_targets / atom_one_hot -- the QM9 `.xyz` reader: header
  properties, atoms (with the `*^` exponent form), frequencies and SMILES; the
  13-target vector in molecule_to_instance's order (preprocessing.py:44-57);
  the 5-way atom one-hot (60-77).  The bond graph is NOT derived: the
  reference takes bonds and the atom order from rdkit (AddHs, aromaticity,
  `GetBondTypeAsDouble`, preprocessing.py:238-275), which is absent here, so
  `molecule_instance` takes the bonds as an argument (parity of the rdkit part
  is unpinned).
"""

import ctypes
import json
import os
import random

import numpy as np
import torch

FORMAT = "hgnn-graphpack"
VERSION = 1


def prepare_experiment_sets(data, shuf=False):
    """80/10/10 split of a list, as preprocessing/loading.py:19-37 (in-place random.shuffle when shuf)."""
    n = len(data)
    n_train = int(0.8 * n)
    n_valid = int(0.1 * n)
    if shuf:
        random.shuffle(data)
    return data[:n_train], data[n_train:n_train + n_valid], data[n_train + n_valid:]


class GraphPack:
    """A memory-mapped graph dataset: graphs i = 0 .. len-1 with (x (n_i, f), A (n_i, n_i), t (n_t,))."""

    FILES = ("node_off", "x", "adj_off", "adj_ij", "adj_w", "targets")

    def __init__(self, path):
        with open(os.path.join(path, "meta.json")) as fh:
            meta = json.load(fh)
        if meta.get("format") != FORMAT or meta.get("version") != VERSION:
            raise RuntimeError(f"hgnn_amd: {path} is not a {FORMAT} v{VERSION} directory")
        self.path = path
        self.meta = meta
        arr = {k: np.load(os.path.join(path, k + ".npy"), mmap_mode="r", allow_pickle=False) for k in self.FILES}
        self.node_off = arr["node_off"]
        self.x = arr["x"]
        self.adj_off = arr["adj_off"]
        self.adj_ij = arr["adj_ij"]
        self.adj_w = arr["adj_w"]
        self.targets = arr["targets"]
        g = len(self.node_off) - 1
        if g < 0 or len(self.adj_off) != g + 1 or self.targets.shape[0] != g:
            raise RuntimeError(f"hgnn_amd: inconsistent graph pack {path}")

    @staticmethod
    def write(path, graphs):
        """Write graphs = iterable of (x (n, f), A (n, n), t (n_t,)) -- or the reference's 7-tuples,
        of which only the first three members are kept -- as a pack directory."""
        xs, offs, ij, w, aoff, ts = [], [0], [], [], [0], []
        f = n_t = None
        for inst in graphs:
            x = torch.as_tensor(inst[0]).detach().to("cpu", torch.float32)
            a = torch.as_tensor(inst[1]).detach().to("cpu", torch.float32)
            t = torch.as_tensor(inst[2]).detach().to("cpu", torch.float32).reshape(-1)
            n = x.shape[0]
            if x.dim() != 2 or tuple(a.shape) != (n, n):
                raise RuntimeError(f"hgnn_amd: graph shapes x {tuple(x.shape)}, A {tuple(a.shape)}")
            if f is None:
                f, n_t = x.shape[1], t.numel()
            if x.shape[1] != f or t.numel() != n_t:
                raise RuntimeError("hgnn_amd: every graph needs the same feature and target widths")
            nz = a.nonzero()  # row-major, as A's own order
            xs.append(x.numpy())
            offs.append(offs[-1] + n)
            ij.append(nz.to(torch.int32).numpy().reshape(-1, 2))
            w.append(a[nz[:, 0], nz[:, 1]].numpy())
            aoff.append(aoff[-1] + nz.shape[0])
            ts.append(t.numpy())
        if f is None:
            raise RuntimeError("hgnn_amd: no graphs to write")
        os.makedirs(path, exist_ok=True)
        data = {
            "node_off": np.asarray(offs, dtype=np.int64),
            "x": np.concatenate(xs).astype(np.float32),
            "adj_off": np.asarray(aoff, dtype=np.int64),
            "adj_ij": np.concatenate(ij).astype(np.int32) if ij else np.zeros((0, 2), np.int32),
            "adj_w": np.concatenate(w).astype(np.float32),
            "targets": np.stack(ts).astype(np.float32),
        }
        for k, v in data.items():
            np.save(os.path.join(path, k + ".npy"), v, allow_pickle=False)
        meta = {"format": FORMAT, "version": VERSION, "graphs": len(ts), "features": int(f), "targets": int(n_t),
                "nodes": int(offs[-1]), "adj_nnz": int(aoff[-1])}
        with open(os.path.join(path, "meta.json"), "w") as fh:
            json.dump(meta, fh, indent=1)
        return GraphPack(path)

    def __len__(self):
        return len(self.node_off) - 1

    def graph(self, i):
        """(x (n, f), A (n, n), t (n_t,)) CPU float32 tensors of graph i."""
        n0, n1 = int(self.node_off[i]), int(self.node_off[i + 1])
        a0, a1 = int(self.adj_off[i]), int(self.adj_off[i + 1])
        x = torch.from_numpy(np.array(self.x[n0:n1]))
        a = torch.zeros(n1 - n0, n1 - n0)
        if a1 > a0:
            ij = torch.from_numpy(np.array(self.adj_ij[a0:a1], dtype=np.int64))
            a[ij[:, 0], ij[:, 1]] = torch.from_numpy(np.array(self.adj_w[a0:a1]))
        t = torch.from_numpy(np.array(self.targets[i]))
        return x, a, t

    def instances(self, idx, J=1, dual=True):
        """Reference 7-tuples (x, A, t, W, WL, Pm, Pd) -- or (x, A, t, W) with dual=False -- for the
        indices, operators from the native builder (functions.operators.graph_operators)."""
        from functions.operators import graph_operators
        out = []
        for i in idx:
            x, a, t = self.graph(i)
            ops = graph_operators([x, a], J, dual)
            out.append([x, a, t, *(ops if dual else [ops])])
        return out

    def batches(self, idx, batch_size, task, J=1, dual=True, device="cuda", dense=False):
        """Yield one batch per `batch_size` consecutive indices of `idx`: a CsrBatch (the executor's
        layout, built natively from the mapped arrays) or, with dense=True, the reference's
        prepare_batch 11-tuple."""
        from functions.batching import prepare_batch
        from .csr import CsrBatch
        idx = list(idx)
        for b0 in range(0, len(idx), batch_size):
            part = idx[b0:b0 + batch_size]
            if dense:
                yield prepare_batch(self.instances(part, J, dual), task, J)
                continue
            graphs = [self.graph(i) for i in part]
            targets = torch.tensor([float(t[task]) for _, _, t in graphs], dtype=torch.float32)
            yield CsrBatch([(x, a) for x, a, _ in graphs], J=J, dual=dual, targets=targets, device=device)

    def ccn_chunks(self, idx, chunk, task, device="cpu"):
        """Yield (X (G, nmax, f), A + I (G, nmax, nmax), n_batch (G,) int64, y (G, 1)) per `chunk` consecutive
        indices of `idx`, each chunk padded to its own largest graph: what CcnTrainStep._chunks makes of the
        reference's 7-tuples (scripts/train_ccn.py:35-37), gathered from the mapped arrays with no loop over
        graphs or entries."""
        idx = np.asarray(list(idx), dtype=np.int64)
        if len(idx) and (idx.min() < 0 or idx.max() >= len(self)):
            raise IndexError(f"hgnn_amd: graph index outside the pack of {len(self)}")
        node_off, adj_off = np.asarray(self.node_off), np.asarray(self.adj_off)
        f = int(self.x.shape[1])
        for c0 in range(0, len(idx), chunk):
            part = idx[c0:c0 + chunk]
            G = len(part)
            n = node_off[part + 1] - node_off[part]
            cnt = adj_off[part + 1] - adj_off[part]
            nmax = int(n.max())
            # per node / per entry: its slot in the chunk and its place in the pack
            slot_n = np.repeat(np.arange(G), n)
            local = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
            slot_e = np.repeat(np.arange(G), cnt)
            src_e = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(adj_off[part], cnt)
            X = np.zeros((G, nmax, f), np.float32)
            X[slot_n, local] = self.x[np.repeat(node_off[part], n) + local]
            A = np.zeros((G, nmax, nmax), np.float32)
            ij = self.adj_ij[src_e]
            A[slot_e, ij[:, 0], ij[:, 1]] = self.adj_w[src_e]
            A[slot_n, local, local] += np.float32(1.0)  # + torch.eye(n)
            y = np.asarray(self.targets[part, task], dtype=np.float32).reshape(G, 1)
            yield tuple(torch.from_numpy(t).to(device) for t in (X, A, n.astype(np.int64), y))

    def to_device(self, J=1, dual=True, device="cuda"):
        """DevicePack(self, J, dual, device): the pack resident on the GPU, batches built there.  J=None: a pack
        for the CCN only (ccn_chunk; no CSR batches)."""
        return DevicePack(self, J=J, dual=dual, device=device)


def coo_first_bad_graph(node_off, adj_off, adj_ij):
    """The first graph whose adjacency entries are not all in [0, n)^2 and strictly ascending row-major, or
    -1: hgnn_pack_count's HGNN_PACK_FLAG_COO, on the host over the whole pack at once."""
    node_off, adj_off = np.asarray(node_off, dtype=np.int64), np.asarray(adj_off, dtype=np.int64)
    ij = np.asarray(adj_ij, dtype=np.int64).reshape(-1, 2)
    n, cnt = np.diff(node_off), np.diff(adj_off)
    gid = np.repeat(np.arange(len(n)), cnt)
    ne = n[gid]
    i, j = ij[:, 0], ij[:, 1]
    bad = (i < 0) | (i >= ne) | (j < 0) | (j >= ne)
    key = i * ne + j  # row-major rank within the graph (where in range)
    if len(key) > 1:
        bad[1:] |= (gid[1:] == gid[:-1]) & (key[1:] <= key[:-1])
    hit = np.nonzero(bad)[0]
    return int(gid[hit[0]]) if len(hit) else -1


def _coo_error(pack, g):
    return RuntimeError(f"hgnn_amd: graph {g} of {pack.path}: adjacency entries out of range "
                        "or not in strictly ascending row-major order")


def check_coo(pack):
    """Raise the RuntimeError DevicePack raises for a malformed adjacency; needs no GPU."""
    g = coo_first_bad_graph(pack.node_off, pack.adj_off, pack.adj_ij)
    if g >= 0:
        raise _coo_error(pack, g)


class DevicePack:
    """A GraphPack resident on one GPU, with the batcher on the device (csrc/batcher.hip).

    Construction uploads the pack's six arrays once, counts every graph's rows and entries on the device
    (hgnn_pack_count, once for this J and dual) and reads the records back: the one host synchronisation.
    batch(idx, task) then sizes the image on the host from the records (hgnn_csr_layout_from_counts) and
    enqueues hgnn_csr_batch_build_device on the current stream -- the image hgnn_csr_batch_build writes on the
    host, byte for byte, with no host work per graph and no synchronisation.

    The device builder takes J <= 3 and, with dual=True, graphs of at most 32 nodes and 72 edge slots; with
    dual=False (the node-graph family alone: GNN_simple) graphs of at most 64 nodes with any number of bonds, so
    SBM-50 and the generated data set (datagen.three_collinear_points, 3 to 49 nodes) are built on the device.
    A batch with a larger graph, and every batch at J > 3, is built by the host batcher (pack.batches): the
    records' HGNN_PACK_FLAG_BOUNDS decides, per batch.  A batch with a graph whose
    edge-slot construction fails raises IndexError as CsrBatch does, when that batch is asked for.

    ccn_chunk(idx, task) enqueues hgnn_pack_ccn_chunk (csrc/ccn_pack.hip): the padded (X, A + I, n_batch, y) chunk
    of the CCN drivers, for graphs of any size.  J=None makes a pack for the CCN only: nothing is counted on the
    device, the adjacency entries are validated on the host instead (check_coo), and batch() raises.  The kernel
    reports a graph it had to leave out (an empty slot) in one device error word; check() reads it.
    """

    def __init__(self, pack, J=1, dual=True, device="cuda"):
        from . import _lib as L
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("hgnn_amd: DevicePack lives on a GPU (device=\"cuda\")")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if len(pack) == 0:
            raise RuntimeError("hgnn_amd: DevicePack: the pack holds no graphs")
        self.pack, self.J, self.dual, self.device = pack, None if J is None else int(J), bool(dual), dev
        self.f_in = int(pack.x.shape[1])
        host = {k: np.ascontiguousarray(getattr(pack, k)) for k in GraphPack.FILES}
        for off, total in ((host["node_off"], len(host["x"])), (host["adj_off"], len(host["adj_w"]))):
            if off[0] != 0 or off[-1] != total or (np.diff(off) < 0).any():
                raise RuntimeError(f"hgnn_amd: inconsistent graph pack {pack.path}")
        if host["adj_ij"].shape != (len(host["adj_w"]), 2):
            raise RuntimeError(f"hgnn_amd: inconsistent graph pack {pack.path}")
        dtypes = {"node_off": np.int64, "x": np.float32, "adj_off": np.int64, "adj_ij": np.int32,
                  "adj_w": np.float32, "targets": np.float32}
        self._arrays = {k: torch.from_numpy(np.array(v, dtype=dtypes[k])).to(dev) for k, v in host.items()}
        self.targets = self._arrays["targets"]
        a = self._arrays
        self._view = L.PackView(*[a[k].data_ptr() for k in GraphPack.FILES], len(pack), self.f_in, 0)
        self.n_targets = int(host["targets"].shape[1])
        self._n = np.diff(host["node_off"])  # nodes per graph: sizes a CCN chunk on the host
        self._err = torch.zeros(1, dtype=torch.int32, device=dev)  # hgnn_pack_ccn_chunk's error word
        self.counts = None  # (graphs, 10) int32 records on the host; None at J > 3 (the host batcher builds all)
        if self.J is None:
            g = coo_first_bad_graph(host["node_off"], host["adj_off"], host["adj_ij"])
            if g >= 0:
                raise _coo_error(pack, g)
        elif self.J <= 3:
            self._counts = torch.empty(len(pack), L.PACK_COUNT_WORDS, dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                L.check(L.lib().hgnn_pack_count(ctypes.byref(self._view), self.J, int(self.dual),
                                                L.ptr(self._counts), L.stream_handle(dev)), "hgnn_pack_count")
            self.counts = self._counts.cpu().numpy()
            bad = np.nonzero(self.counts[:, 8] & L.PACK_FLAG_COO)[0]
            if len(bad):
                raise RuntimeError(f"hgnn_amd: graph {int(bad[0])} of {pack.path}: adjacency entries out of range "
                                   "or not in strictly ascending row-major order")

    def __len__(self):
        return len(self.pack)

    def batch(self, idx, task):
        """The CsrBatch of the graphs `idx` (in that order; repeats allowed) with targets[idx, task], built on
        the device on the current stream."""
        from . import _lib as L
        from .csr import CsrBatch
        if self.J is None:
            raise RuntimeError("hgnn_amd: DevicePack(J=None) is a pack for the CCN only (ccn_chunk); CSR batches "
                               "need the J of the model")
        idx = [int(i) for i in idx]
        bs = len(idx)
        if bs == 0:
            raise RuntimeError("hgnn_amd: empty batch")
        if min(idx) < 0 or max(idx) >= len(self.pack):
            raise IndexError(f"hgnn_amd: graph index outside the pack of {len(self.pack)}")
        host_path = self.counts is None
        if not host_path:
            rec = np.ascontiguousarray(self.counts[np.asarray(idx, dtype=np.int64)])
            host_path = bool((rec[:, 8] & L.PACK_FLAG_BOUNDS).any())
        if host_path:
            return next(self.pack.batches(idx, bs, task, J=self.J, dual=self.dual, device=self.device))
        lib = L.lib()
        lay = L.CsrLayout()
        st = lib.hgnn_csr_layout_from_counts(bs, ctypes.c_void_p(rec.ctypes.data), self.f_in, self.J, int(self.dual),
                                             ctypes.byref(lay))
        if st == 4:
            raise IndexError("hgnn_amd: a graph's edge-slot construction writes past nnz(A) "
                             "(the reference's graph_operators raises IndexError)")
        L.check(st, "csr layout from counts")
        dev = self.device
        with torch.cuda.device(dev):
            image = torch.empty(int(lay.bytes), dtype=torch.uint8, device=dev)
            d_idx = torch.tensor(idx, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
            scratch = torch.empty(lib.hgnn_csr_batch_build_device_scratch_bytes(bs), dtype=torch.uint8, device=dev)
            L.check(lib.hgnn_csr_batch_build_device(ctypes.byref(self._view), L.ptr(self._counts), L.ptr(d_idx), bs,
                                                    self.J, int(self.dual), ctypes.byref(lay), L.ptr(image),
                                                    L.ptr(scratch), scratch.numel(), L.stream_handle(dev)),
                    "csr batch build on the device")
            targets = self.targets[d_idx.long(), task]
        return CsrBatch.from_image(lay, image, targets)

    def batches(self, idx, batch_size, task):
        """One batch per `batch_size` consecutive indices of `idx`, as GraphPack.batches yields them."""
        idx = list(idx)
        for b0 in range(0, len(idx), batch_size):
            yield self.batch(idx[b0:b0 + batch_size], task)

    def ccn_chunk(self, idx, task, nmax=None):
        """(X (G, nmax, f), A + I (G, nmax, nmax), n_batch (G,) int64, y (G, 1)) of the graphs `idx` (in that
        order; repeats allowed) with targets[idx, task], built on the device on the current stream: the chunk
        GraphPack.ccn_chunks and CcnTrainStep._chunks build on the host, bit for bit.  nmax: the chunk's largest
        graph, or a larger padding."""
        from . import _lib as L
        idx = [int(i) for i in idx]
        G = len(idx)
        if G == 0:
            raise RuntimeError("hgnn_amd: empty chunk")
        if min(idx) < 0 or max(idx) >= len(self.pack):
            raise IndexError(f"hgnn_amd: graph index outside the pack of {len(self.pack)}")
        big = int(self._n[np.asarray(idx, dtype=np.int64)].max())
        if nmax is None:
            nmax = big
        elif int(nmax) < big:
            raise RuntimeError(f"hgnn_amd: nmax = {nmax}, but the chunk holds a graph of {big} nodes")
        nmax = int(nmax)
        dev = self.device
        with torch.cuda.device(dev):
            X = torch.empty(G, nmax, self.f_in, dtype=torch.float32, device=dev)
            A = torch.empty(G, nmax, nmax, dtype=torch.float32, device=dev)
            nb = torch.empty(G, dtype=torch.int64, device=dev)
            y = torch.empty(G, 1, dtype=torch.float32, device=dev)
            d_idx = torch.tensor(idx, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
            L.check(L.lib().hgnn_pack_ccn_chunk(ctypes.byref(self._view), self.n_targets, L.ptr(d_idx), G, nmax,
                                                int(task), L.ptr(X), L.ptr(A), L.ptr(nb), L.ptr(y),
                                                L.ptr(self._err), L.stream_handle(dev)), "hgnn_pack_ccn_chunk")
        return X, A, nb, y

    def ccn_chunks(self, idx, chunk, task):
        """One ccn_chunk per `chunk` consecutive indices of `idx`, as GraphPack.ccn_chunks yields them."""
        idx = list(idx)
        for c0 in range(0, len(idx), chunk):
            yield self.ccn_chunk(idx[c0:c0 + chunk], task)

    def check(self):
        """Raise if a ccn_chunk since the last check left a graph out as an empty slot (one host read)."""
        bits = int(self._err.item())
        if bits:
            self._err.zero_()
            raise RuntimeError("hgnn_amd: DevicePack.ccn_chunk left a graph out (index outside the pack, more nodes "
                               "than nmax, or adjacency entries out of range or out of order): the device copy of "
                               f"{self.pack.path} is corrupt")


# ---------------------------------------------------------------- QM9 .xyz
XYZ_PROPS = ("tag", "ident", "A", "B", "C", "mu", "alpha", "homo", "lumo", "gap", "r2", "zpve", "U0", "U", "H", "G",
             "Cv")
# molecule_to_instance's task order (preprocessing/preprocessing.py:44-57); task 8 is the last frequency
TARGETS = ("alpha", "Cv", "G", "gap", "H", "homo", "lumo", "mu", "freq_last", "r2", "U", "U0", "zpve")


def _num(s):
    # QM9 writes some exponents as '*^' (and '.*^'), preprocessing.py:189-190
    return float(s.replace(".*^", "e").replace("*^", "e"))


def read_xyz(path_or_text):
    """Parse one QM9 `.xyz` file (preprocessing/preprocessing.py:174-236, minus the rdkit part):
    dict with Na, the 17 header properties, atoms [(symbol, (x, y, z), partial charge)], freq
    and smiles."""
    text = path_or_text
    if "\n" not in path_or_text and os.path.exists(path_or_text):
        with open(path_or_text) as fh:
            text = fh.read()
    lines = text.splitlines()
    na = int(lines[0])
    prop = lines[1].split()
    mol = {"Na": na, "tag": prop[0], "ident": int(prop[1])}
    for k, v in zip(XYZ_PROPS[2:], prop[2:]):
        mol[k] = _num(v)
    atoms = []
    for i in range(na):
        p = lines[2 + i].split()
        atoms.append((p[0], tuple(_num(c) for c in p[1:4]), _num(p[4])))
    mol["atoms"] = atoms
    mol["freq"] = [_num(v) for v in lines[2 + na].split()]
    mol["smiles"] = lines[3 + na].split()[0]
    return mol


def molecule_targets(mol):
    """The 13-vector `task` of molecule_to_instance (preprocessing/preprocessing.py:44-57)."""
    t = torch.zeros(13)
    for k, name in enumerate(TARGETS):
        t[k] = float(mol["freq"][-1]) if name == "freq_last" else mol[name]
    return t


def atom_one_hot(symbols):
    """(n, 5) one-hot over H, C, N, O, other (preprocessing/preprocessing.py:60-77)."""
    col = {"H": 0, "C": 1, "N": 2, "O": 3}
    x = torch.zeros(len(symbols), 5)
    for i, s in enumerate(symbols):
        x[i, col.get(s, 4)] = 1.0
    return x


def molecule_instance(mol, bonds, spatial=False, charge=False):
    """(x, A, t) of molecule_to_instance (preprocessing/preprocessing.py:25-94) for atoms in the
    file's order and bonds = [(i, j, order)] supplied by the caller (the reference gets them, and
    its atom order, from rdkit).  Keeps the reference's indentation quirk: the spatial / charge
    columns are written for the LAST atom only (preprocessing.py:79-86)."""
    width = 5 + (3 if spatial else 0) + (1 if charge else 0)
    x = torch.zeros(mol["Na"], width)
    x[:, :5] = atom_one_hot([a[0] for a in mol["atoms"]])
    i = mol["Na"] - 1
    if spatial:
        x[i, 5:8] = torch.tensor(mol["atoms"][i][1])
        if charge:
            x[i, 8] = mol["atoms"][i][2]
    elif charge:
        x[i, 5] = mol["atoms"][i][2]
    a = torch.zeros(mol["Na"], mol["Na"])
    for u, v, order in bonds:
        a[u, v] = order
        a[v, u] = order
    return x, a, molecule_targets(mol)
