"""The device labeller on the GPU (``subiso.label_pairs`` -> ``dmp_subiso_label_dev``, csrc/dmp_subiso_dev.hip) against the
plain-Python restatement of tests/util_subiso.py: counts, trials, node and edge weights as integers, over a sentinel-filled
output, on the smallest shapes at which the kernel can go wrong; the budget; the host fallback; ``SmallLikePairs``."""
import functools

import numpy as np
import pytest

import util_subiso as U

pytestmark = pytest.mark.gpu
SENTINEL = -0x0123456789ABCDEF
BOTH = ("node", "edge")


@functools.lru_cache(maxsize=None)
def _cases():
    cs = U.cases()
    return cs, {k: U.expected(p) for k, p in cs.items()}


@functools.lru_cache(maxsize=None)
def _batch(size):
    pairs = U.batch(size)
    return pairs, [U.expected(p) for p in pairs]


def _label(pairs, gpu, weights=BOTH, **kw):
    from dualmessagepassing_amd import subiso
    return subiso.label_pairs(pairs, gpu, weights=weights, fill=SENTINEL, **kw)


def _check(pairs, ex, res):
    """Assertions 1, 2 and 6a: the inputs alone stay below the default budget, so nothing may lean on the fallback; then every
    output equals the restatement as integers and the node weights of a pair sum to counts * pn."""
    from dualmessagepassing_amd import subiso
    assert max(e["per_root"] for e in ex) < subiso.DEFAULT_BUDGET
    assert res["complete"].all() and res["fallback"] == 0
    assert res["counts"].dtype == res["trials"].dtype == np.int64
    assert res["counts"].tolist() == [e["count"] for e in ex]
    assert res["trials"].tolist() == [e["trials"] for e in ex]
    for i, (p, e) in enumerate(zip(pairs, ex)):
        assert np.array_equal(res["node_weights"][i], e["node"]), i
        assert np.array_equal(res["edge_weights"][i], e["edge"]), i
        assert int(res["node_weights"][i].sum()) == e["count"] * len(p[2]), i


@pytest.mark.parametrize("name", list(U.cases()))
def test_each_case_alone_equals_the_restatement(gpu, name):
    cs, ex = _cases()
    _check([cs[name]], [ex[name]], _label([cs[name]], gpu))


def test_all_cases_in_one_batch_equal_the_restatement(gpu):
    cs, ex = _cases()
    names = list(cs)
    _check([cs[k] for k in names], [ex[k] for k in names], _label([cs[k] for k in names], gpu))


@pytest.mark.parametrize("size", [1, 2, 64, 257])
def test_batches_of_mixed_sizes_equal_the_restatement(gpu, size):
    pairs, ex = _batch(size)
    assert len(pairs) == size and len(pairs[size // 2][6]) == 0        # the empty graph in the middle
    if size >= 64:
        sizes = [len(p[6]) for p in pairs]
        assert max(sizes) >= 130 and min(sizes) == 0
    _check(pairs, ex, _label(pairs, gpu))


def test_closed_forms(gpu):
    cs, _ = _cases()
    res = _label([cs["complete_digraph_4path"], cs["pn4_gn4_no_edges"], cs["pn3_gn5_no_edges_labels"], cs["pn0"],
                  cs["pn2_gn1_pn_above_gn"], cs["node_label_absent"]], gpu)
    assert res["counts"].tolist() == [9 * 8 * 7 * 6, 24, 12, 1, 0, 0] and res["complete"].all()
    assert res["trials"][0] == 9 * (1 + 8 + 56 + 336)
    assert res["edge_weights"][0].tolist() == [3 * 7 * 6] * 72         # every edge: 3 path positions x the other two nodes


def test_two_runs_are_equal_bit_for_bit_and_weights_do_not_change_counts(gpu):
    pairs, ex = _batch(64)
    a, b = _label(pairs, gpu), _label(pairs, gpu)
    for k in ("counts", "trials", "complete"):
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in ("node_weights", "edge_weights"):
        assert np.concatenate(a[k]).tobytes() == np.concatenate(b[k]).tobytes(), k
    for w in ((), ("node", ), ("edge", )):
        c = _label(pairs, gpu, weights=w)
        assert c["counts"].tobytes() == a["counts"].tobytes() and c["trials"].tobytes() == a["trials"].tobytes(), w
        assert (c["node_weights"] is None) == ("node" not in w) and (c["edge_weights"] is None) == ("edge" not in w)
        for k in ("node_weights", "edge_weights"):
            if c[k] is not None:
                assert np.concatenate(c[k]).tobytes() == np.concatenate(a[k]).tobytes(), (w, k)
    from dualmessagepassing_amd import subiso
    assert np.array_equal(subiso.count_subisomorphisms_device(pairs, gpu), a["counts"])


def test_small_like_raw_pairs_equal_the_host_pool(gpu):
    from dualmessagepassing_amd import harness, subiso
    raw = U.raw_pairs(harness.SmallLikePairs(256, seed=1, threads=4))
    want = harness.count_subisomorphisms_batch(raw, threads=4)
    got = subiso.label_pairs(raw, gpu, threads=4, fill=SENTINEL)
    assert np.array_equal(got["counts"], want)
    assert got["fallback"] == int((~got["complete"]).sum())


def test_an_item_out_of_budget_clears_its_pair_and_the_host_finishes_it(gpu):
    cs, ex = _cases()
    names = ["pattern_duplicate_edge", "complete_digraph_4path", "graph_parallel_equal_label"]
    assert ex[names[0]]["per_root"] <= 8 and ex[names[2]]["per_root"] <= 8 < ex[names[1]]["per_root"]
    res = _label([cs[k] for k in names], gpu, budget=8, threads=2)
    assert res["complete"].tolist() == [True, False, True] and res["fallback"] == 1
    assert res["counts"].tolist() == [ex[k]["count"] for k in names] and res["counts"][1] == 3024
    assert res["trials"][0] == ex[names[0]]["trials"] and res["trials"][2] == ex[names[2]]["trials"]
    for i, k in enumerate(names):
        assert np.array_equal(res["node_weights"][i], ex[k]["node"]) and np.array_equal(res["edge_weights"][i], ex[k]["edge"]), k


def test_a_pair_outside_the_limits_is_finished_on_the_host_and_its_neighbours_are_unaffected(gpu):
    cs, ex = _cases()
    p17 = U.mixed_pn17_pair()
    e17 = U.expected(p17)
    assert len(p17[2]) == 17 and e17["count"] >= 1
    pairs = [cs["pn3"], cs["pn8"], p17, cs["pn4"]]
    want = [ex["pn3"], ex["pn8"], e17, ex["pn4"]]
    res = _label(pairs, gpu, threads=2)
    assert res["complete"].tolist() == [True, True, False, True] and res["fallback"] == 1
    assert res["counts"].tolist() == [e["count"] for e in want]
    for i, e in enumerate(want):
        assert np.array_equal(res["node_weights"][i], e["node"]) and np.array_equal(res["edge_weights"][i], e["edge"]), i
        if i != 2:
            assert res["trials"][i] == e["trials"]


def test_small_like_pairs_built_on_the_device_has_the_host_samples(gpu):
    from dualmessagepassing_amd import harness
    a = harness.SmallLikePairs(64, seed=2, threads=4)
    b = harness.SmallLikePairs(64, seed=2, threads=4, device=gpu)
    assert a.shape == b.shape and len(a) == len(b) == 64
    for x, y in zip(a.samples, b.samples):
        assert x["counts"] == y["counts"]
        for side in ("pattern", "graph"):
            for k in x[side]:
                assert np.array_equal(x[side][k], y[side][k]), (side, k)
