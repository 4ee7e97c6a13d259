"""The type-constrained link evaluation without a GPU: ``rank_counts_typed_tensor`` against its definition in Python loops,
the relation masks, ``link_ranks(node_type=...)``, the adjusted mean rank index, the per-relation block, ``load_nodes`` and
the new entries of the library."""
import math

import numpy as np
import pytest
import torch as th


def _typed_case(seed, Q=23, N=61, H=9, T=5):
    """Integers in [-2, 2] as fp32 (every score exact), types 0 .. T - 1 (type T - 1 on no node), masks of every kind: all,
    none, one type, a type nobody has."""
    rng = np.random.default_rng(seed)
    query = rng.integers(-2, 3, (Q, H)).astype(np.float32)
    table = rng.integers(-2, 3, (N, H)).astype(np.float32)
    target = rng.integers(0, N, Q)
    ctype = rng.integers(0, T - 1, N)
    allowed = rng.integers(0, 1 << T, Q)
    allowed[0], allowed[1], allowed[2], allowed[3] = (1 << T) - 1, 0, 1 << int(ctype[target[2]]), 1 << (T - 1)
    lists = [sorted(set(rng.integers(0, N, int(rng.integers(0, 7))).tolist()) | ({int(target[i])} if i % 3 == 0 else set()))
             for i in range(Q)]
    return query, table, target, ctype, allowed, lists


def _loops(query, table, target, ctype, allowed, lists):
    """The definition: int64 scores, membership by index."""
    s = query.astype(np.int64) @ table.astype(np.int64).T
    g, e, c = [], [], []
    for i in range(len(target)):
        cand = [j for j in range(table.shape[0])
                if j != target[i] and j not in lists[i] and 0 <= ctype[j] <= 62 and (int(allowed[i]) >> int(ctype[j])) & 1]
        t = s[i, target[i]]
        g.append(sum(1 for j in cand if s[i, j] > t))
        e.append(sum(1 for j in cand if s[i, j] == t))
        c.append(len(cand))
    return g, e, c


def _csr(lists):
    ptr = th.tensor(np.cumsum([0] + [len(l) for l in lists]), dtype=th.int64)
    idx = th.tensor([c for l in lists for c in l], dtype=th.int64)
    return ptr, idx


@pytest.mark.parametrize("filtered", [False, True])
def test_typed_tensor_form_equals_the_definition(filtered):
    from dualmessagepassing_amd.unc_eval import rank_counts_typed, rank_counts_typed_tensor
    query, table, target, ctype, allowed, lists = _typed_case(3)
    if not filtered:
        lists = [[] for _ in lists]
    want = _loops(query, table, target, ctype, allowed, lists)
    args = [th.from_numpy(a) for a in (query, table, target, ctype, allowed)]
    f = _csr(lists) if filtered else ()
    for fn in (rank_counts_typed_tensor, rank_counts_typed):          # on the CPU the second is the first
        got = fn(*args, *f)
        assert [x.dtype for x in got] == [th.int32] * 3
        assert [x.tolist() for x in got] == [list(w) for w in want]
    # chunked by a budget of two rows: the same vectors
    got = rank_counts_typed_tensor(*args, *f, budget_bytes=2 * table.shape[0] * 4)
    assert [x.tolist() for x in got] == [list(w) for w in want]
    assert want[2][1] == 0 and want[2][3] == 0 and want[0][1] == 0          # rows that admit nothing rank against nobody


def test_a_type_code_above_62_is_admitted_by_nobody_in_the_tensor_form():
    from dualmessagepassing_amd.unc_eval import rank_counts_typed_tensor
    query, table, target, ctype, allowed, lists = _typed_case(4)
    ctype = ctype.copy()
    ctype[[5, 17]] = [63, 200]
    allowed[:] = -1                  # every bit, 63 included
    want = _loops(query, table, target, ctype, allowed & ((1 << 63) - 1), lists)
    got = rank_counts_typed_tensor(*[th.from_numpy(a) for a in (query, table, target, ctype, allowed)], *_csr(lists))
    assert [x.tolist() for x in got] == [list(w) for w in want]


def test_relation_type_masks_equal_a_dict_of_sets():
    from dualmessagepassing_amd.unc_eval import relation_type_masks
    rng = np.random.default_rng(5)
    N, R, M = 40, 5, 120
    ntype = rng.integers(0, 4, N)
    ntype[ntype == 2] = 62                          # type 2 on no node, the largest code on some
    known = np.stack([rng.integers(0, N, M), rng.integers(0, R - 1, M), rng.integers(0, N, M)], 1)      # relation R - 1: no triplet
    want = {(r, side): set() for r in range(R) for side in (0, 1)}
    for s, r, o in known:
        want[(r, 0)].add(int(ntype[s]))
        want[(r, 1)].add(int(ntype[o]))
    got = relation_type_masks(th.from_numpy(known), th.from_numpy(ntype), R)
    assert got.dtype == th.int64 and got.shape == (R, 2)
    for (r, side), types in want.items():
        assert int(got[r, side]) == sum(1 << t for t in types), (r, side)
    assert got[R - 1].tolist() == [0, 0] and bool((got >= 0).all())
    assert all((int(got[r, side]) >> 2) & 1 == 0 for r in range(R) for side in (0, 1))
    with pytest.raises(ValueError, match="0 .. 62"):
        relation_type_masks(th.from_numpy(known), th.from_numpy(np.where(ntype == 62, 63, ntype)), R)


def _hetero(rng, N=36, H=6):
    """Nodes of three types, relations 0: type 0 -> type 1, 1: type 1 -> type 2, 2: type 0 -> type 2, integer embeddings."""
    ntype = np.arange(N) % 3
    pair = {0: (0, 1), 1: (1, 2), 2: (0, 2)}
    trip = []
    for _ in range(60):
        r = int(rng.integers(0, 3))
        s = int(rng.choice(np.flatnonzero(ntype == pair[r][0])))
        o = int(rng.choice(np.flatnonzero(ntype == pair[r][1])))
        trip.append((s, r, o))
    trip = np.unique(np.asarray(trip, dtype=np.int64), axis=0)
    emb = th.from_numpy(rng.integers(-2, 3, (N, H)).astype(np.float32))
    w_rel = th.from_numpy(rng.integers(-1, 2, (3, H)).astype(np.float32))
    return th.from_numpy(ntype), th.from_numpy(trip), emb, w_rel


def test_link_ranks_with_types_on_a_hand_checked_graph():
    from dualmessagepassing_amd.unc_eval import link_ranks, relation_type_masks
    rng = np.random.default_rng(6)
    ntype, trip, emb, w_rel = _hetero(rng)
    N = emb.size(0)
    test, known = trip[::4], trip
    raw, raw_c = link_ranks(w_rel, emb, test, known=known, return_considered=True)
    typed, typed_c = link_ranks(w_rel, emb, test, known=known, node_type=ntype, return_considered=True)
    assert typed.dtype == th.float64 and typed.shape == raw.shape == (test.size(0), 2) and typed_c.dtype == th.int64
    # the definition, per query: candidates of the admitted type, the target and the other known entities left out
    known_set = {tuple(t) for t in known.tolist()}
    for n, (s, r, o) in enumerate(test.tolist()):
        for col, (fixed, tgt, side_type) in enumerate(((s, o, int(ntype[o])), (o, s, int(ntype[s])))):
            q = emb[fixed] * w_rel[r]
            score = (emb * q).sum(1)
            listed = {c for c in range(N) if ((s, r, c) if col == 0 else (c, r, o)) in known_set}
            cand = [c for c in range(N) if c != tgt and c not in listed and int(ntype[c]) == side_type]
            g = sum(1 for c in cand if score[c] > score[tgt])
            e = sum(1 for c in cand if score[c] == score[tgt])
            assert typed[n, col].item() == 1 + g + 0.5 * e and typed_c[n, col].item() == len(cand), (n, col)
            assert raw_c[n, col].item() == N - 1 - len(listed - {tgt})
    # set inclusion, elementwise and without a tolerance
    assert bool((typed <= raw).all()) and bool((typed_c <= raw_c).all()) and bool((typed_c < raw_c).any())
    for ties in ("optimistic", "pessimistic"):
        assert bool((link_ranks(w_rel, emb, test, known=known, node_type=ntype, ties=ties) <= link_ranks(w_rel, emb, test, known=known, ties=ties)).all())
    # every type admitted: the untyped ranks, bit for bit
    every = th.full((3, 2), (1 << 3) - 1, dtype=th.int64)
    same, same_c = link_ranks(w_rel, emb, test, known=known, node_type=ntype, type_masks=every, return_considered=True)
    assert th.equal(same, raw) and th.equal(same_c, raw_c)
    # the default masks are those of `known`
    assert th.equal(link_ranks(w_rel, emb, test, known=known, node_type=ntype, type_masks=relation_type_masks(known, ntype, 3)), typed)


def test_typed_counts_are_bounded_by_the_untyped_ones_and_the_target_type_is_admitted():
    """greater_typed <= greater and equal_typed <= equal per query (C_typed is a subset of C); a relation mask that leaves
    the target's own type out still ranks against that type; a filter entry of a non-admitted type is subtracted once."""
    from dualmessagepassing_amd.unc_eval import known_filter, link_ranks, rank_counts_tensor, rank_counts_typed_tensor
    rng = np.random.default_rng(7)
    ntype, trip, emb, w_rel = _hetero(rng)
    N = emb.size(0)
    test = trip[::3]
    fixed, tgt = test[:, 0], test[:, 2]
    query = emb[fixed] * w_rel[test[:, 1]]
    # filters that hold nodes of EVERY type: most entries are of a type the row does not admit
    lists = [sorted(set(rng.integers(0, N, 9).tolist())) for _ in range(test.size(0))]
    ptr, idx = _csr(lists)
    allowed = th.ones_like(tgt) << ntype[tgt]
    g, e = rank_counts_tensor(query, emb, tgt, ptr, idx)
    gt, et, ct = rank_counts_typed_tensor(query, emb, tgt, ntype, allowed, ptr, idx)
    assert bool((gt <= g).all()) and bool((et <= e).all())
    for i in range(test.size(0)):
        same = [c for c in range(N) if int(ntype[c]) == int(ntype[tgt[i]]) and c != int(tgt[i])]
        assert ct[i].item() == len([c for c in same if c not in lists[i]])          # not len(same) - len(lists[i])
    # masks of zero: only the target's own type is left, through link_ranks
    zero = th.zeros(3, 2, dtype=th.int64)
    ranks, cons = link_ranks(w_rel, emb, test, node_type=ntype, type_masks=zero, return_considered=True)
    for i in range(test.size(0)):
        for col, t in enumerate((int(test[i, 2]), int(test[i, 0]))):
            assert cons[i, col].item() == int((ntype == ntype[t]).sum()) - 1
    with pytest.raises(ValueError, match="0 .. 62"):
        link_ranks(w_rel, emb, test, node_type=ntype + 61)
    with pytest.raises(ValueError, match="node_type"):
        link_ranks(w_rel, emb, test, node_type=ntype[:-1])


def test_amri_by_hand_and_at_its_two_ends():
    from dualmessagepassing_amd.unc_eval import link_metrics
    ranks = th.tensor([[1.0, 3.0], [2.0, 1.0], [4.5, 2.0]], dtype=th.float64)
    cons = th.tensor([[4, 10], [6, 3], [8, 2]])
    m = link_metrics(ranks, considered=cons)
    #   sum(rank - 1) = 0 + 2 + 1 + 0 + 3.5 + 1 = 7.5, sum(considered) / 2 = 33 / 2
    assert m["AMRI"] == pytest.approx(1 - 7.5 / 16.5, abs=1e-15) and m["candidates"] == pytest.approx(33 / 6, abs=1e-15)
    assert m["object/AMRI"] == pytest.approx(1 - 4.5 / 9.0, abs=1e-15) and m["subject/AMRI"] == pytest.approx(1 - 3.0 / 7.5, abs=1e-15)
    assert m["object/candidates"] == 6.0 and m["subject/candidates"] == 5.0
    plain = link_metrics(ranks)
    assert "AMRI" not in plain and all(m[k] == v for k, v in plain.items())          # the other entries do not move
    assert link_metrics(th.ones(5, 2, dtype=th.float64), considered=cons.repeat(2, 1)[:5])["AMRI"] == 1.0
    middle = link_metrics(1.0 + cons.to(th.float64) / 2, considered=cons)
    assert middle["AMRI"] == 0.0 and middle["object/AMRI"] == 0.0 and middle["subject/AMRI"] == 0.0
    with pytest.raises(ValueError):
        link_metrics(ranks, considered=cons[:2])


def test_metrics_by_relation_by_hand():
    from dualmessagepassing_amd.unc_eval import link_metrics_by_relation
    ranks = th.tensor([[1.0, 2.0], [4.0, 1.0], [10.0, 20.0]], dtype=th.float64)
    rel = th.tensor([0, 2, 0])
    m = link_metrics_by_relation(ranks, rel, 4, ks=(1, 3))
    assert [m["relation/%d/count" % r] for r in range(4)] == [4, 0, 2, 0]
    assert m["relation/0/MRR"] == pytest.approx((1 + 0.5 + 0.1 + 0.05) / 4, abs=1e-15) and m["relation/0/MR"] == 33.0 / 4
    assert m["relation/0/Hits@1"] == 0.25 and m["relation/0/Hits@3"] == 0.5
    assert m["relation/2/MRR"] == pytest.approx(1.25 / 2, abs=1e-15) and m["relation/2/MR"] == 2.5 and m["relation/2/Hits@3"] == 0.5
    assert all(not math.isnan(v) for v in m.values())
    assert [m["relation/1/" + k] for k in ("MRR", "MR", "Hits@1", "Hits@3")] == [0.0] * 4
    assert link_metrics_by_relation(ranks[:, 0], rel, 4)["relation/0/count"] == 2          # one column


def test_load_nodes_reads_types_and_attributes(tmp_path):
    from dualmessagepassing_amd.unc_harness import load_nodes
    three = tmp_path / "node3.dat"
    three.write_text("2\tgene c\t1\n0\tgene a\t0\n1\tdisease b\t3\n")          # ids out of order, names with blanks
    ntype, attr = load_nodes(str(three))
    assert ntype.dtype == th.int64 and ntype.tolist() == [0, 3, 1] and attr is None
    four = tmp_path / "node4.dat"
    four.write_text("1\tb\t2\t0.5,-1,2\n0\ta\t0\t1,2,3\n\n2\tc\t2\t0,0,0.25\n")
    ntype, attr = load_nodes(str(four))
    assert ntype.tolist() == [0, 2, 2] and attr.dtype == th.float32
    assert attr.tolist() == [[1.0, 2.0, 3.0], [0.5, -1.0, 2.0], [0.0, 0.0, 0.25]]
    two = tmp_path / "node2.dat"
    two.write_text("0\t1,2,3\n1\t4,5,6\n")
    with pytest.raises(ValueError, match="type column"):
        load_nodes(str(two))
    gap = tmp_path / "gap.dat"
    gap.write_text("0\ta\t0\n2\tc\t1\n")
    with pytest.raises(ValueError, match="each once"):
        load_nodes(str(gap))


def test_evaluate_links_takes_the_new_arguments():
    import inspect
    from dualmessagepassing_amd.unc_harness import evaluate_links
    p = inspect.signature(evaluate_links).parameters
    assert p["node_type"].default is None and p["by_relation"].default is False


def test_library_exports_the_typed_entry_at_abi_97():
    import ctypes
    from dualmessagepassing_amd import _abi, _build
    lib = ctypes.CDLL(_build.build_lib())
    assert lib.dmp_abi_version() == 97 == _abi.ABI_VERSION
    assert hasattr(lib, "dmp_rank_counts_typed") and "dmp_rank_counts_typed" in _abi.SIGNATURES
    words = lib.dmp_rank_typed_workspace_words
    words.restype, words.argtypes = _abi.SIGNATURES["dmp_rank_typed_workspace_words"]
    assert [words(n) for n in (0, 1, 128, 129, 63109)] == [0, 1, 1, 2, 494]          # one word per tile of 128 candidates
    fn = lib.dmp_rank_counts_typed
    fn.restype, fn.argtypes = _abi.SIGNATURES["dmp_rank_counts_typed"]
    # refused on the host before anything is launched: no type array, no masks, no workspace, a width beyond 256
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    base = [p, p, p, None, None, 0, p, p, 2, 4, 8, p, p, p, p, None, None]
    for hole in (6, 7, 14):
        args = list(base)
        args[hole] = None
        assert fn(*args) == -1, hole
    args = list(base)
    args[10] = 257
    assert fn(*args) == -2
    assert _abi.DMP_RANK_BAD_TYPE == 1
