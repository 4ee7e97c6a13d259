"""unc_eval on the CPU: the tensor-op form of the rank counts against the definition written as Python loops, the tie
policies and metrics on a hand example, the known-candidate filter against a dict of sets, and the chunking."""
import math

import numpy as np
import pytest
import torch as th


def _loops(query, table, target, ptr=None, idx=None):
    """The definition, one candidate at a time.  Integer-valued inputs: every product and sum is exact in any order."""
    Q, N, H = len(query), len(table), len(query[0])
    greater, equal = [], []
    for i in range(Q):
        t = sum(float(query[i][h]) * float(table[target[i]][h]) for h in range(H))
        gone = set() if ptr is None else {int(c) for c in idx[ptr[i]:ptr[i + 1]]}
        g = e = 0
        for c in range(N):
            if c == target[i] or c in gone:
                continue
            s = sum(float(query[i][h]) * float(table[c][h]) for h in range(H))
            g += s > t
            e += s == t
        greater.append(g)
        equal.append(e)
    return greater, equal


def _case(seed, Q=5, N=9, H=3):
    rng = np.random.default_rng(seed)
    query = rng.integers(-2, 3, (Q, H)).astype(np.float32)
    table = rng.integers(-2, 3, (N, H)).astype(np.float32)
    target = rng.integers(0, N, Q)
    return query, table, target


def _csr(lists):
    ptr = np.cumsum([0] + [len(l) for l in lists])
    return ptr.astype(np.int64), np.asarray([c for l in lists for c in l], dtype=np.int64)


def _run(query, table, target, ptr=None, idx=None, **kw):
    from dualmessagepassing_amd.unc_eval import rank_counts_tensor
    f = (None, None) if ptr is None else (th.from_numpy(ptr), th.from_numpy(idx))
    g, e = rank_counts_tensor(th.from_numpy(query), th.from_numpy(table), th.from_numpy(target), *f, **kw)
    assert g.dtype == th.int32 and e.dtype == th.int32
    return g.tolist(), e.tolist()


def test_tensor_form_equals_the_definition_without_a_filter():
    query, table, target = _case(0)
    want = _loops(query, table, target)
    assert sum(want[1]) > 0                       # the integer inputs do tie
    assert _run(query, table, target) == want


def test_tensor_form_equals_the_definition_with_filters():
    query, table, target = _case(1)
    N = len(table)
    lists = [sorted({int(target[0]), 0, 4}),      # holds the target: the target stays out either way, counted once
             [],                                  # empty
             list(range(N)),                      # removes every candidate
             [c for c in range(N) if c != target[3]],     # every candidate but the target
             [8]]
    ptr, idx = _csr(lists)
    want = _loops(query, table, target, ptr, idx)
    assert want[0][2] == 0 and want[1][2] == 0 and want[0][3] == 0 and want[1][3] == 0
    assert _run(query, table, target, ptr, idx) == want
    assert want != _loops(query, table, target)   # the filter changes something in this case


def test_a_single_candidate_counts_nothing():
    query, table, target = _case(2, N=1)
    assert _run(query, table, target) == ([0] * 5, [0] * 5)
    ptr, idx = _csr([[0], [], [0], [], []])
    assert _run(query, table, target, ptr, idx) == ([0] * 5, [0] * 5)


def test_rank_counts_on_the_cpu_is_the_tensor_form():
    from dualmessagepassing_amd.unc_eval import rank_counts
    query, table, target = _case(3)
    g, e = rank_counts(th.from_numpy(query), th.from_numpy(table), th.from_numpy(target))
    assert (g.tolist(), e.tolist()) == _loops(query, table, target)
    g, e = rank_counts(th.from_numpy(query).double(), th.from_numpy(table).double(), th.from_numpy(target))
    assert (g.tolist(), e.tolist()) == _loops(query, table, target)


def test_chunked_tensor_form_equals_the_unchunked_one():
    from dualmessagepassing_amd.unc_eval import rows_per_chunk
    query, table, target = _case(4)
    lists = [[1, 2], [], [0, 3, 8], [5], list(range(9))]
    ptr, idx = _csr(lists)
    budget = 2 * 9 * 4                            # two fp32 rows of nine scores
    assert math.ceil(5 / rows_per_chunk(9, 4, budget)) == 3
    assert rows_per_chunk(9, 4, 1) == 1           # never less than a row
    for f in ((), (ptr, idx)):
        assert _run(query, table, target, *f, budget_bytes=budget) == _run(query, table, target, *f)
        assert _run(query, table, target, *f, budget_bytes=budget) == _loops(query, table, target, *f)


def test_tie_policies_and_metrics_on_a_hand_example():
    from dualmessagepassing_amd.unc_eval import link_metrics, link_ranks, ranks_of
    # four nodes on a line, one relation of weight 1: score(s, o) = emb[s] * emb[o]
    emb = th.tensor([[1.0], [2.0], [2.0], [3.0]])
    w = th.tensor([[1.0]])
    trip = th.tensor([[0, 0, 1], [3, 0, 0]])
    # (0, r, 1): object side scores 1, 2, 2, 3 against t = 2 -> one greater (node 3), one equal (node 2; node 1 is the target)
    #            subject side: emb[1] * emb = 2, 4, 4, 6 against t = 2 (node 0) -> three greater, none equal
    # (3, r, 0): object side 3, 6, 6, 9 against t = 3 -> three greater;  subject side emb[0] * emb = 1, 2, 2, 3 against t = 3 -> none
    want = {"optimistic": [[2.0, 4.0], [4.0, 1.0]], "mean": [[2.5, 4.0], [4.0, 1.0]], "pessimistic": [[3.0, 4.0], [4.0, 1.0]]}
    for ties, ranks in want.items():
        assert link_ranks(w, emb, trip, ties=ties).tolist() == ranks
    assert link_ranks(w, emb, trip).tolist() == want["mean"]
    assert link_ranks(w, emb, trip, sides=("subject",)).tolist() == [[4.0], [1.0]]
    # filtered: (0, r, 3) is known, so node 3 leaves the object-side candidates of (0, r, 1); the target itself stays
    known = th.tensor([[0, 0, 1], [0, 0, 3], [3, 0, 0]])
    assert link_ranks(w, emb, trip, known=known).tolist() == [[1.5, 4.0], [4.0, 1.0]]
    with pytest.raises(ValueError):
        ranks_of(th.zeros(1), th.zeros(1), ties="best")
    m = link_metrics(th.tensor(want["mean"], dtype=th.float64))
    both = [2.5, 4.0, 4.0, 1.0]
    assert m["MRR"] == pytest.approx(sum(1 / r for r in both) / 4) and m["MR"] == pytest.approx(sum(both) / 4)
    assert m["Hits@1"] == 0.25 and m["Hits@3"] == 0.5 and m["Hits@10"] == 1.0
    assert m["object/MRR"] == pytest.approx((1 / 2.5 + 1 / 4) / 2) and m["object/MR"] == pytest.approx(3.25)
    assert m["subject/MRR"] == pytest.approx((1 / 4 + 1) / 2) and m["subject/Hits@1"] == 0.5 and m["object/Hits@3"] == 0.5
    assert link_metrics(th.tensor([[2.0], [3.0]]), ks=(2,), sides=("object",)) == {
        "MRR": pytest.approx(5 / 12), "MR": 2.5, "Hits@2": 0.5, "object/MRR": pytest.approx(5 / 12), "object/MR": 2.5, "object/Hits@2": 0.5}


@pytest.mark.parametrize("side", ["object", "subject"])
def test_known_filter_equals_a_dict_of_sets(side):
    from dualmessagepassing_amd.unc_eval import known_filter
    rng = np.random.default_rng(5)
    n, rels = 6, 2
    known = np.stack([rng.integers(0, n, 40), rng.integers(0, rels, 40), rng.integers(0, n, 40)], 1)
    fixed_col, cand_col = (0, 2) if side == "object" else (2, 0)
    table = {}
    for row in known:
        table.setdefault((int(row[fixed_col]), int(row[1])), set()).add(int(row[cand_col]))
    assert max(len(v) for v in table.values()) >= 3 and len(table) < 40       # (entity, relation) pairs repeat
    queries = np.asarray([(e, r) for e in range(n) for r in range(rels)] + [(0, 0), (n + 3, 1)])     # all pairs, a repeat, an unknown entity
    ptr, idx = known_filter(th.from_numpy(known), th.from_numpy(queries), rels, side)
    assert ptr.dtype == th.int64 and idx.dtype == th.int64 and ptr.shape == (len(queries) + 1,) and int(ptr[0]) == 0
    ptr, idx = ptr.tolist(), idx.tolist()
    assert ptr[-1] == len(idx)
    for i, (e, r) in enumerate(queries.tolist()):
        assert idx[ptr[i]:ptr[i + 1]] == sorted(table.get((e, r), ())), (i, e, r)
    assert ptr[-1] == ptr[-2]                     # the unknown entity's list is empty
    with pytest.raises(ValueError):
        known_filter(th.from_numpy(known), th.from_numpy(queries), rels, "both")


def test_split_links_is_seeded_and_disjoint():
    from dualmessagepassing_amd.unc_harness import split_links
    trip = th.stack([th.arange(50), th.zeros(50, dtype=th.int64), th.arange(50) + 100], 1)
    train, test = split_links(trip, 0.1, seed=3)
    assert test.shape == (5, 3) and train.shape == (45, 3)
    assert sorted(train[:, 0].tolist() + test[:, 0].tolist()) == list(range(50))
    again = split_links(trip, 0.1, seed=3)
    assert th.equal(again[0], train) and th.equal(again[1], test)
    assert not th.equal(split_links(trip, 0.1, seed=4)[1], test)
    assert split_links(trip[:2], 0.01, seed=0)[1].shape == (1, 3)
    with pytest.raises(ValueError):
        split_links(trip, 1.0, seed=0)


def test_evaluate_links_refuses_a_model_without_the_decoder():
    from dualmessagepassing_amd.unc import TrainModel
    from dualmessagepassing_amd.unc_harness import evaluate_links
    model = TrainModel(None, 8, 4, 1, 3)
    trip = th.tensor([[0, 0, 1], [1, 0, 2]])
    with pytest.raises(ValueError, match="w_relation"):
        evaluate_links(model, None, trip, trip)


def test_library_is_at_abi_97_with_the_rank_entries():
    import ctypes
    from dualmessagepassing_amd import _abi, _build
    lib = ctypes.CDLL(_build.build_lib())
    assert lib.dmp_abi_version() == 97 == _abi.ABI_VERSION
    assert [lib.dmp_rank_supported(h) for h in (0, 1, 50, 256, 257)] == [0, 1, 1, 1, 0]
    res, args = _abi.SIGNATURES["dmp_rank_counts"]
    fn = lib.dmp_rank_counts
    fn.restype, fn.argtypes = res, args
    # refused before any launch: a width outside 1 .. 256, a table without rows
    assert fn(None, None, None, None, None, 0, 4, 8, 257, None, None, None) == -2
    assert fn(None, None, None, None, None, 0, 4, 0, 16, None, None, None) == -1
    assert fn(None, None, None, None, None, 0, 4, 1 << 31, 16, None, None, None) == -2
