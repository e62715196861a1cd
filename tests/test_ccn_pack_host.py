"""GraphPack.ccn_chunks and the host validator of a pack's adjacency entries (hgnn_amd.dataset), without a GPU.

ccn_chunks gathers the CCN drivers' padded chunks from the mapped arrays in numpy; it must give what
scripts/train_ccn.py:35-37 plus padding gives from the graphs themselves, bit for bit (data movement and one exact
`+ 1.0`), so every comparison is torch.equal."""

import os

import numpy as np
import pytest

import ccn_pack_util as U


@pytest.fixture(scope="module")
def packs(tmp_path_factory):
    from hgnn_amd.dataset import GraphPack
    root = tmp_path_factory.mktemp("ccn_pack_host")
    return {"wide": (GraphPack.write(str(root / "wide"), U.graph_set()), U.graph_set()),
            "narrow": (GraphPack.write(str(root / "narrow"), U.narrow_set()), U.narrow_set())}


@pytest.mark.parametrize("task", U.TASKS)
@pytest.mark.parametrize("chunk", [1, 4, None])
@pytest.mark.parametrize("name", ["wide", "narrow"])
def test_chunks_equal_the_reference_loop(packs, name, chunk, task):
    pack, graphs = packs[name]
    chunk = chunk or len(pack)
    got = list(pack.ccn_chunks(range(len(pack)), chunk, task))
    assert len(got) == -(-len(pack) // chunk)
    for k, c in enumerate(got):
        part = graphs[k * chunk:(k + 1) * chunk]
        assert c[0].shape[1] == max(g[0].shape[0] for g in part)  # padded to its own largest graph
        U.assert_same_chunk(c, U.reference_chunk(part, task), f"{name} chunk {k}")


def test_chunks_take_any_order_and_repeats(packs):
    pack, graphs = packs["wide"]
    idx = [5, 13, 5, 0, 8, 12, 14]
    (c,) = pack.ccn_chunks(idx, len(idx), 7)
    U.assert_same_chunk(c, U.reference_chunk([graphs[i] for i in idx], 7))
    with pytest.raises(IndexError):
        next(pack.ccn_chunks([0, len(pack)], 2, 0))


def test_the_stored_self_loop_becomes_two(packs):
    pack, _ = packs["wide"]
    (c,) = pack.ccn_chunks([10], 1, 0)
    assert c[1][0, 2, 2].item() == 2.0 and c[1][0, 0, 0].item() == 1.0


def _rewritten(tmp_path, change):
    from hgnn_amd.dataset import GraphPack
    path = str(tmp_path / "p")
    pack = GraphPack.write(path, U.graph_set()[:4])
    ij = np.load(os.path.join(path, "adj_ij.npy"))
    change(ij, int(pack.adj_off[2]), int(pack.node_off[3] - pack.node_off[2]))  # graph 2: first entry, node count
    np.save(os.path.join(path, "adj_ij.npy"), ij)
    return GraphPack(path)


def test_validator_accepts_what_write_wrote(packs):
    from hgnn_amd.dataset import check_coo, coo_first_bad_graph
    for pack, _ in packs.values():
        assert coo_first_bad_graph(pack.node_off, pack.adj_off, pack.adj_ij) == -1
        check_coo(pack)


def test_validator_rejects_an_index_outside_the_graph(tmp_path):
    from hgnn_amd.dataset import check_coo

    def change(ij, a0, n):
        ij[a0 + 3, 1] = n  # the first index past the graph
    with pytest.raises(RuntimeError, match="graph 2 .*out of range or not in strictly ascending"):
        check_coo(_rewritten(tmp_path, change))


def test_validator_rejects_a_negative_index(tmp_path):
    from hgnn_amd.dataset import check_coo

    def change(ij, a0, n):
        ij[a0, 0] = -1
    with pytest.raises(RuntimeError, match="graph 2 "):
        check_coo(_rewritten(tmp_path, change))


def test_validator_rejects_two_swapped_entries(tmp_path):
    from hgnn_amd.dataset import check_coo

    def change(ij, a0, n):
        ij[[a0 + 1, a0 + 2]] = ij[[a0 + 2, a0 + 1]]
    with pytest.raises(RuntimeError, match="graph 2 "):
        check_coo(_rewritten(tmp_path, change))


def test_validator_rejects_a_repeated_entry(tmp_path):
    from hgnn_amd.dataset import check_coo

    def change(ij, a0, n):
        ij[a0 + 1] = ij[a0]
    with pytest.raises(RuntimeError, match="graph 2 "):
        check_coo(_rewritten(tmp_path, change))


def test_validator_keeps_graphs_apart():
    """The last entry of one graph and the first of the next are not compared."""
    from hgnn_amd.dataset import coo_first_bad_graph
    node_off, adj_off = np.array([0, 3, 5]), np.array([0, 2, 4])
    ij = np.array([[1, 2], [2, 1], [0, 1], [1, 0]], np.int32)
    assert coo_first_bad_graph(node_off, adj_off, ij) == -1
    ij[3] = [1, 2]  # column 2 of a two-node graph
    assert coo_first_bad_graph(node_off, adj_off, ij) == 1
