"""The host half of the LRP / DMPLRP training path (harness.LRPPairs): closed-form permutation counts against the
enumeration (``PermIndex.from_graphs`` on the CPU), the self-loop refusal and the capacity levels.  All integers: exact."""
import numpy as np
import pytest
import torch as th


def _random_graph(rng, n, e, reversed_edges, parallel):
    if n == 0:
        z = np.zeros(0, np.int64)
        return {"src": z, "dst": z, "num_nodes": 0, "rev": np.zeros(0, bool)}
    src, dst = [], []
    while len(src) < e and n > 1:
        a, b = int(rng.integers(0, n)), int(rng.integers(0, n))
        if a != b:
            src.append(a)
            dst.append(b)
    if parallel and src:                              # the same pair again, later
        src += src[:2]
        dst += dst[:2]
    src, dst = np.array(src, np.int64), np.array(dst, np.int64)
    rev = np.zeros(len(src), bool)
    if reversed_edges:                                # the stored form: [forward | reversed]
        src, dst, rev = np.concatenate([src, dst]), np.concatenate([dst, src]), np.concatenate([rev, ~rev])
    return {"src": src, "dst": dst, "num_nodes": n, "rev": rev}


def _dataset(seed=0):
    """A dozen samples: an empty graph, one node, a node of degree 0 among others, degrees below L - 1, parallel edges,
    reversed edges, a hub."""
    from dualmessagepassing_amd.harness import PairDataset
    rng = np.random.default_rng(seed)
    shapes = [(0, 0), (1, 0), (2, 1), (3, 2), (4, 3), (5, 4), (5, 12), (6, 9), (7, 20), (8, 5), (9, 30), (6, 2)]
    samples = []
    for i, (n, e) in enumerate(shapes):
        p = _random_graph(rng, max(1, n // 2), e // 2, reversed_edges=i % 2 == 0, parallel=i % 3 == 0)
        g = _random_graph(rng, n, e, reversed_edges=i % 2 == 1, parallel=i % 3 != 1)
        for x in (p, g):
            x["vlabel"], x["elabel"], x["eid"] = np.zeros(x["num_nodes"], np.int64), np.zeros(len(x["src"]), np.int64), np.arange(len(x["src"]))
        samples.append({"pattern": p, "graph": g, "counts": i, "subisomorphisms": np.zeros((0, p["num_nodes"]), np.int64)})
    hub = samples[8]["graph"]                          # a node with 6 distinct neighbours, one of them twice
    hub["src"] = np.concatenate([np.zeros(7, np.int64), hub["src"]])
    hub["dst"] = np.concatenate([np.array([1, 2, 3, 4, 5, 6, 3], np.int64), hub["dst"]])
    hub["rev"] = np.concatenate([np.zeros(7, bool), hub["rev"]])
    return PairDataset(samples, dict(p_nodes=4, p_edges=15, g_nodes=9, g_edges=40, n_vlabels=1, n_elabels=1))


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5])
def test_closed_form_counts_equal_the_enumeration(L):
    from dualmessagepassing_amd.lrp import PermIndex
    ds = _dataset()
    view = ds.lrp(L)
    assert view is ds.lrp(L) and view.seq_len == L and len(view) == len(ds)
    degs = []
    for i, x in enumerate(ds.samples):
        for side, key in enumerate(("pattern", "graph")):
            g = x[key]
            perm = PermIndex.from_graphs([(g["src"], g["dst"], g["num_nodes"], g["rev"])], "cpu", L)
            assert int(perm.sizes.sum()) == int(view.perm_counts[i, side]) == perm.num_perms, (i, key)
            keep = ~g["rev"]
            per_node = [len(set(g["dst"][keep][g["src"][keep] == v].tolist())) for v in range(g["num_nodes"])]
            degs.append(max(per_node, default=0))
            want = th.tensor([int(np.prod([d - k for k in range(min(L - 1, d))], dtype=np.int64)) for d in per_node], dtype=th.int64)
            assert th.equal(perm.sizes, want), (i, key)
    assert view.max_degree == max(degs) >= 6
    assert min(degs) == 0


def test_self_loop_is_refused():
    from dualmessagepassing_amd.harness import PairDataset
    ds = _dataset()
    g = ds.samples[5]["graph"]
    g["src"], g["dst"], g["rev"] = np.append(g["src"], 2), np.append(g["dst"], 2), np.append(g["rev"], False)
    with pytest.raises(ValueError, match="self-loop"):
        PairDataset(ds.samples, ds.shape).lrp()
    g["rev"][-1] = True                                # the same loop as a reversed edge is no neighbour
    assert PairDataset(ds.samples, ds.shape).lrp().perm_counts.shape == (len(ds), 2)


@pytest.mark.parametrize("batch", [1, 3, 5])
def test_capacity_levels_are_monotone_and_the_top_bounds_every_batch(batch):
    view = _dataset().lrp(4)
    for levels in (1, 3, 4):
        caps = view.perm_capacity(batch, levels)
        assert len(caps) == levels
        for lo, hi in zip(caps, caps[1:]):
            assert lo[0] <= hi[0] and lo[1] <= hi[1]
        rng = np.random.default_rng(batch)
        worst = np.sort(view.perm_counts, axis=0)[::-1][:batch].sum(axis=0)
        assert tuple(int(w) for w in worst) == caps[-1]
        for _ in range(50):
            idx = rng.choice(len(view), size=batch, replace=False)
            tot = view.perm_counts[idx].sum(axis=0)
            assert tot[0] <= caps[-1][0] and tot[1] <= caps[-1][1]


def test_view_keeps_the_pair_interface():
    ds = _dataset()
    view = ds.lrp(3)
    assert view.samples is ds.samples and view.shape is ds.shape
    assert view.lrp(3) is view and view.lrp(4).seq_len == 4
    sub = view.subset([8, 3])
    assert sub.seq_len == 3 and [tuple(r) for r in sub.perm_counts] == [tuple(view.perm_counts[8]), tuple(view.perm_counts[3])]
    cfg = view.model_config(hid_dim=8, layers=1)
    assert cfg["rep_net"] == "DMPLRP" and cfg["lrp_seq_len"] == 3
    assert view.model_config(rep_net="LRP", lrp_seq_len=5)["lrp_seq_len"] == 5
