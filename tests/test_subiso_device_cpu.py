"""The device labeller without a GPU (dualmessagepassing_amd/subiso.py, csrc/dmp_subiso_dev.hip): its entries in the header,
the binding and the built library; the tests' plain-Python restatement of the search against the project's two host searches;
the weight definitions by hand; the host road of ``label_pairs``; the range checks; the batch image the kernel is handed,
walked in plain Python; ``SmallLikePairs`` unchanged."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import util_subiso as U
from conftest import ROOT


@functools.lru_cache(maxsize=None)
def _cases():
    cs = U.cases()
    return cs, {k: U.expected(p) for k, p in cs.items()}


def test_new_entries_are_declared_bound_and_built_and_the_abi_number_stays():
    from dualmessagepassing_amd import _abi, _build, _lib
    hdr = open(os.path.join(ROOT, "include", "dmp_hip.h")).read()
    assert re.search(r"\bint\s+dmp_subiso_label_dev\s*\(", hdr) and "dmp_subiso_image;" in hdr
    assert "dmp_subiso_label_dev" in _abi.SIGNATURES and issubclass(_abi.dmp_subiso_image, ctypes.Structure)
    assert "dmp_subiso_dev.hip" in _build.SOURCES
    assert hasattr(ctypes.CDLL(_build.build_lib()), "dmp_subiso_label_dev")
    assert int(re.search(r"#define\s+DMP_ABI_VERSION\s+(\d+)", hdr).group(1)) == 97 == _abi.ABI_VERSION == _lib.load().dmp_abi_version()
    assert (_abi.DMP_SUBISO_MAX_PN, _abi.DMP_SUBISO_MAX_PM) == (16, 64)
    assert _abi.DMP_SUBISO_MAX_GN >= 512 and _abi.DMP_SUBISO_MAX_GM >= 2048       # the reference's "large" setting fits


def test_restatement_equals_both_host_searches_on_the_case_list():
    from dualmessagepassing_amd import harness
    cs, ex = _cases()
    counts = harness.count_subisomorphisms_batch(list(cs.values()), threads=2)
    for (name, pair), c in zip(cs.items(), counts):
        assert ex[name]["count"] == c, name
        if len(pair[2]) == 0:                 # an empty pattern: the host enumerations cannot shape its one empty row
            assert ex[name]["count"] == 1 and ex[name]["rows"].shape == (1, 0)
            continue
        assert np.array_equal(ex[name]["rows"], harness.enumerate_subisomorphisms(*pair)), name
        if name != "roots_gn512":             # (512 x 512 candidate visits in the slowest of the three searches)
            assert np.array_equal(ex[name]["rows"], harness.enumerate_subisomorphisms_py(*pair)), name
    assert ex["complete_digraph_4path"]["count"] == 9 * 8 * 7 * 6 and ex["complete_digraph_4path"]["per_root"] == 1 + 8 + 56 + 336
    assert ex["pn4_gn4_no_edges"]["count"] == 24 and ex["pn3_gn5_no_edges_labels"]["count"] == 3 * 2 * 2


def test_weights_from_rows_by_hand():
    """Pattern 0 -a-> 1 given twice; graph 0 -a-> 1 (twice), 1 -a-> 2, 2 -b-> 0, one node label.  Matches: (0, 1) and (1, 2).
    Node 0 and 2 lie in one match, node 1 in both.  Each match pays 2 (the duplicated pattern edge) to every parallel image
    edge with label a: the two 0 -> 1 edges get 2 each, 1 -> 2 gets 2, 2 -> 0 (label b) gets 0."""
    from dualmessagepassing_amd import subiso
    cs, ex = _cases()
    e = ex["pattern_duplicate_edge"]
    assert e["rows"].tolist() == [[0, 1], [1, 2]]
    assert e["node"].tolist() == [1, 2, 1] and e["edge"].tolist() == [2, 2, 2, 0]
    nw, ew = subiso.weights_from_rows(cs["pattern_duplicate_edge"], e["rows"])
    assert nw.tolist() == [1, 2, 1] and ew.tolist() == [2, 2, 2, 0]
    # parallel graph edges of one label: the count is that of a simple graph, every parallel edge gets the weight
    g = ex["graph_parallel_equal_label"]
    assert g["count"] == 2 and g["edge"].tolist() == [1, 1, 1, 1] and ex["graph_parallel_other_labels"]["edge"].tolist() == [1, 0, 0, 0]


def test_label_pairs_on_a_cpu_device_equals_the_restatement():
    from dualmessagepassing_amd import subiso
    cs, ex = _cases()
    names = list(cs)
    res = subiso.label_pairs([cs[k] for k in names], "cpu", weights=("node", "edge"), threads=2)
    assert res["fallback"] == len(names) and not res["complete"].any() and res["counts"].dtype == np.int64
    for i, k in enumerate(names):
        assert res["counts"][i] == ex[k]["count"], k
        assert np.array_equal(res["node_weights"][i], ex[k]["node"]) and np.array_equal(res["edge_weights"][i], ex[k]["edge"]), k
    only = subiso.label_pairs([cs[k] for k in names], "cpu")
    assert only["node_weights"] is None and only["edge_weights"] is None and np.array_equal(only["counts"], res["counts"])
    assert np.array_equal(subiso.count_subisomorphisms_device([cs[k] for k in names], "cpu"), res["counts"])
    empty = subiso.label_pairs([], "cpu", weights=("node",))
    assert empty["counts"].shape == (0,) and empty["node_weights"] == [] and empty["fallback"] == 0


def test_range_checks_raise_before_any_library_call(monkeypatch):
    from dualmessagepassing_amd import _lib, subiso

    def no_library(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)
    good = U.cases()["pn3"]
    bad = {
        "pattern src above pn": lambda p: (U.A(0, 3), ) + p[1:2] + p[2:3] + p[3:],
        "graph dst negative": lambda p: p[:5] + (np.where(np.arange(len(p[5])) == 2, -1, p[5]), ) + p[6:],
        "graph src equal to gn": lambda p: p[:4] + (np.where(np.arange(len(p[4])) == 0, len(p[6]), p[4]), ) + p[5:],
        "ragged pattern": lambda p: p[:3] + (p[3][:-1], ) + p[4:],
        "ragged graph": lambda p: p[:5] + (p[5][:-1], ) + p[6:],
        "seven arrays": lambda p: p[:7],
        "two-dimensional": lambda p: p[:6] + (p[6].reshape(1, -1), ) + p[7:],
    }
    small = (U.A(0, 1), U.A(1, 2), U.A(0, 0, 0), U.A(1, 1), U.A(0, 1), U.A(1, 2), U.A(0, 0, 0), U.A(1, 1))
    for what, make in bad.items():
        pair = make(small if what == "pattern src above pn" else good)
        for device in ("cpu", "cuda:0"):
            with pytest.raises(ValueError, match="pair 1"):
                subiso.label_pairs([good, pair, good], device)
    with pytest.raises(ValueError, match="weights"):
        subiso.label_pairs([good], "cpu", weights=("rows",))
    with pytest.raises(ValueError, match="budget"):
        subiso.label_pairs([good], "cpu", budget=0)


@pytest.mark.parametrize("weights", [True, False])
def test_the_batch_image_walked_in_python_equals_the_restatement(weights):
    """What the kernel is handed (``subiso.build_image``: candidate ranges, pattern edges by later endpoint, the distinct graph
    edges as a CSR, the chunk list), walked item by item the way the kernel walks it."""
    from dualmessagepassing_amd import subiso
    cs, ex = _cases()
    names = list(cs)
    pairs = [cs[k] for k in names] + [U.mixed_pn17_pair()]
    got = U.walk_image(subiso.build_image(*subiso._flatten(pairs)), subiso.DEFAULT_BUDGET, weights)
    assert got["complete"].tolist() == [True] * len(names) + [False]
    assert got["counts"][:-1].tolist() == [ex[k]["count"] for k in names]
    assert got["trials"][:-1].tolist() == [ex[k]["trials"] for k in names]
    if weights:
        gn, gm = sum(len(p[6]) for p in pairs[:-1]), sum(len(p[4]) for p in pairs[:-1])
        assert np.array_equal(got["node_weights"][:gn], np.concatenate([ex[k]["node"] for k in names]))
        assert np.array_equal(got["edge_weights"][:gm], np.concatenate([ex[k]["edge"] for k in names]))
    tight = U.walk_image(subiso.build_image(*subiso._flatten([cs["pattern_duplicate_edge"], cs["complete_digraph_4path"]])), 8, False)
    assert tight["complete"].tolist() == [True, False] and tight["counts"][0] == 2


def test_small_like_pairs_is_unchanged():
    from dualmessagepassing_amd import harness
    a = harness.SmallLikePairs(32, seed=3, threads=2)
    b = harness.SmallLikePairs(32, seed=3, threads=2, device="cpu")
    assert a.shape == b.shape and len(a) == len(b) == 32
    for x, y in zip(a.samples, b.samples):
        assert x["counts"] == y["counts"] and x["subisomorphisms"].shape == y["subisomorphisms"].shape
        for side in ("pattern", "graph"):
            assert sorted(x[side]) == sorted(y[side])
            for k in x[side]:
                assert np.array_equal(x[side][k], y[side][k]), (side, k)
    assert [x["counts"] for x in a.samples] == harness.count_subisomorphisms_batch(U.raw_pairs(a), threads=2).tolist()
    assert sum(x["counts"] > 0 for x in a.samples) > 8
