"""Shared by tests/test_resident_cpu.py and tests/test_gpu_resident.py: the two datasets, the case list, and a numpy
restatement of what ``dmp_collate_resident`` does with a plan (slot by slot, nothing shared with the kernel's code)."""
import functools

import numpy as np

SIDES = ("pattern", "graph")


@functools.lru_cache(maxsize=None)
def ragged_pairs():
    """``SmallLikePairs(48, seed=7)`` with every sample's subisomorphism rows enumerated (the class itself keeps the counts
    only): ragged on both sides, rows of 0 .. a few thousand elements per sample."""
    from dualmessagepassing_amd.harness import PairDataset, SmallLikePairs, enumerate_subisomorphisms
    base = SmallLikePairs(48, seed=7, threads=4)
    samples = []
    for x in base.samples:
        p, g = x["pattern"], x["graph"]
        pe, ge = len(p["src"]) // 2, len(g["src"]) // 2
        rows = enumerate_subisomorphisms(p["src"][:pe], p["dst"][:pe], p["vlabel"], p["elabel"][:pe],
                                         g["src"][:ge], g["dst"][:ge], g["vlabel"], g["elabel"][:ge])
        assert len(rows) == x["counts"]
        samples.append(dict(x, subisomorphisms=rows))
    return PairDataset(samples, base.shape)


@functools.lru_cache(maxsize=None)
def tiny_pairs():
    """Four hand-made pairs over a ONE-label vocabulary (the inert labels are 0): a one-node pattern without edges on a graph
    without edges, a pair with ``counts == 0`` and no rows, and two small ones."""
    from dualmessagepassing_amd.harness import PairDataset, validate_samples
    i64 = lambda *a: np.array(a, np.int64)
    shape = dict(p_nodes=3, p_edges=2, g_nodes=5, g_edges=6, n_vlabels=1, n_elabels=1)

    def graph(n, u, v, max_ne):
        return PairDataset._with_rev(i64(*u), i64(*v), np.zeros(n, np.int64), np.zeros(len(u), np.int64), max_ne, 1)

    samples = [
        {"pattern": graph(1, (), (), 2), "graph": graph(3, (), (), 6), "counts": 3, "subisomorphisms": i64(0, 1, 2).reshape(3, 1)},
        {"pattern": graph(2, (0,), (1,), 2), "graph": graph(2, (1,), (0,), 6), "counts": 0, "subisomorphisms": np.zeros((0, 2), np.int64)},
        {"pattern": graph(2, (0,), (1,), 2), "graph": graph(4, (0, 2, 3), (1, 3, 0), 6), "counts": 3,
         "subisomorphisms": i64(0, 1, 2, 3, 3, 0).reshape(3, 2)},
        {"pattern": graph(3, (0, 1), (1, 2), 2), "graph": graph(5, (0, 1, 2, 3, 4, 0), (1, 2, 3, 4, 0, 2), 6), "counts": 6,
         "subisomorphisms": i64(0, 1, 2, 1, 2, 3, 2, 3, 4, 3, 4, 0, 4, 0, 1, 4, 0, 2).reshape(6, 3)},
    ]
    ds = PairDataset(samples, shape)
    assert validate_samples(ds) == 4
    return ds


def level_of(meta, pad):
    """The capacity level a padded batch landed on, from its pattern node total (``batch_arrays``' own formula)."""
    B, K = pad["batch"], pad["levels"]
    return next(k for k in range(1, K + 1) if -(-B * pad["pattern"][0] * k // K) + B == meta[0][0])


def by_size(ds):
    """Sample indices, the smallest pairs first (by graph edges, then pattern nodes)."""
    return sorted(range(len(ds)), key=lambda i: (len(ds.samples[i]["graph"]["src"]), ds.samples[i]["pattern"]["num_nodes"], i))


def cases(name):
    """The case list: ``(dataset, [(case id, indices, pad, subs)])`` for ``"ragged"``, ``"tiny"`` and ``"subset"`` (a subset
    of the ragged pairs: a dataset of its own)."""
    if name == "tiny":
        ds = tiny_pairs()
        pad, cap = ds.pad_buckets(2, levels=4), ds.sub_capacity(2)
        return ds, [("one", [0], None, None), ("all", [0, 1, 2, 3], None, None), ("all+subs", [0, 1, 2, 3], None, ds.sub_capacity(4)),
                    ("pad-edgeless", [0], pad, None), ("pad-full+subs", [1, 2], pad, cap), ("pad-no-rows+subs", [1], pad, cap),
                    ("pad-repeat+subs", [2, 2], pad, cap),
                    ("subs-zero", [1], None, 0), ("pad+subs-zero", [1], pad, 0)]       # a capacity of 0: an empty ``sub_flat``
    ds = ragged_pairs()
    if name == "subset":
        ds = ds.subset(range(10, 30))
        return ds, [("all", list(range(20)), None, None), ("pad+subs", list(range(16)), ds.pad_buckets(16, levels=4), ds.sub_capacity(16))]
    pad, cap = ds.pad_buckets(16, levels=4), ds.sub_capacity(16)
    order = by_size(ds)
    exact = sum(ds.samples[i]["subisomorphisms"].size for i in range(16, 32))      # a capacity with no zero behind the rows
    rowless = [i for i, x in enumerate(ds.samples) if x["subisomorphisms"].size == 0][:3]      # a batch a capacity of 0 holds
    assert rowless
    return ds, [
        ("subs-zero", rowless, None, 0), ("pad+subs-zero", rowless, pad, 0),
        ("subs-exact", list(range(16, 32)), None, exact), ("subs-wide", list(range(16)), pad, 3 * 4096 + 5),
        ("one", [5], None, None), ("sixteen", list(range(16)), None, None), ("all", list(range(48)), None, None),
        ("pad-full", list(range(16)), pad, None), ("pad-short", [45, 46, 47], pad, None),
        ("pad-level1", order[:3], pad, None), ("pad-level4", order[-16:], pad, None),
        ("subs", list(range(16, 32)), None, cap), ("pad+subs", list(range(16, 32)), pad, cap), ("pad-short+subs", [45, 46, 47], pad, cap),
        ("descending", list(range(15, -1, -1)), pad, cap), ("repeated", [3, 3, 7, 1, 3], None, cap), ("pad-repeated", [40, 2, 40, 2, 9], pad, cap),
    ]


def run_plan(store, plan, info, padded, subs=None):
    """What one launch makes of ``plan``, as numpy arrays in ``batch_arrays``' order: ``store`` is ``resident_store``'s."""
    P, R = info["slots"], info["real"]
    sample, prefix = plan[4:4 + P], plan[4 + P:].reshape(5, P + 1)
    out = []
    for side, key in enumerate(SIDES):
        S, noff, eoff = store[key], prefix[2 * side], prefix[2 * side + 1]
        node = {k: np.full(noff[-1], -7, np.int64) for k in ("nid", "vlabel")}
        edge = {k: np.full(eoff[-1], -7, np.int64) for k in ("src", "dst", "eid", "elabel", "rev")}
        for b in range(P):
            n, e = int(noff[b + 1] - noff[b]), int(eoff[b + 1] - eoff[b])
            ns, es = slice(noff[b], noff[b + 1]), slice(eoff[b], eoff[b + 1])
            node["nid"][ns] = np.arange(n)
            if b < R:
                a, c = S["node_ptr"][sample[b]], S["edge_ptr"][sample[b]]
                assert S["node_ptr"][sample[b] + 1] - a == n and S["edge_ptr"][sample[b] + 1] - c == e
                node["vlabel"][ns] = S["vlabel"][a:a + n]
                for k in edge:
                    edge[k][es] = S[k][c:c + e]
            else:
                j = np.arange(e)
                node["vlabel"][ns] = plan[2 * side]
                edge["src"][es], edge["dst"][es], edge["eid"][es], edge["elabel"][es], edge["rev"][es] = j % n, (j % n + 1) % n, j, plan[2 * side + 1], 0
        assert all((v != -7).all() for v in list(node.values()) + list(edge.values()))
        out += [edge["src"], edge["dst"], np.diff(noff), np.diff(eoff), node["nid"], node["vlabel"], edge["eid"], edge["elabel"],
                edge["rev"].astype(bool)]
    counts = np.zeros((P, 1), np.float32)
    counts[:R, 0] = store["counts"][sample[:R]]
    out.append(counts)
    if padded:
        out.append((np.arange(P) < R).astype(np.float32).reshape(P, 1))
    if subs is not None:
        flat = np.zeros(int(subs), np.int64)
        for b in range(R):
            a = store["sub_ptr"][sample[b]]
            flat[prefix[4, b]:prefix[4, b + 1]] = store["subs"][a:a + prefix[4, b + 1] - prefix[4, b]]
        out += [flat, prefix[4].copy()]
    return out
