"""The type-constrained score-and-rank kernel (csrc/dmp_rank_typed.hip + dmp_rank_kernel.h through
unc_eval.rank_counts_typed) against its definition in int64 on exact inputs, in fp64 with a rounding bracket on random ones,
against the untyped kernel with every type admitted, through ``link_ranks`` against the tensor route, and end to end on a
graph of three node types."""
import functools

import numpy as np
import pytest
import torch as th

pytestmark = pytest.mark.gpu

# (Q, N, H): the shapes of test_gpu_unc_rank.py -- a workgroup owns 128 queries and candidate tiles of 128; from five tiles on
# (N > 512) grid.y splits the candidates, 5000 takes ten splits
SHAPES = [(1, 1, 1), (70, 333, 50), (70, 513, 50), (130, 600, 33), (33, 5000, 64), (64, 256, 256), (70, 333, 130)]
RANDOM_WIDTHS = [50, 64, 256]
# how the candidates' types lie and what the rows admit (see _layout)
LAYOUTS = ["sorted", "interleaved", "gap", "types63", "own", "not_own", "one_type"]


def _layout(name, rng, Q, N, target):
    """-> (types [N], allowed [Q]).
    sorted       four types in contiguous ranges whose boundaries fall inside a tile, a random mask per row (the rows of a
                 workgroup differ; rows 0 / 1 admit nothing / everything)
    interleaved  type = c % 3: every tile is mixed, nothing can be skipped
    gap          types 0, 2, 5 in ranges: type 1 has no candidate, and rows admit it
    types63      all 63 codes (ranges when N allows), masks over 63 bits
    own          a row admits the type of its own target and nothing else
    not_own      a row admits everything except the type of its target
    one_type     sorted, and every row of a workgroup admits the same single type (another per workgroup): whole ranges of
                 tiles are stepped over, with them the filter entries that lie there, and some splits have nothing to do"""
    c = np.arange(N)
    if name == "interleaved":
        types, bits = c % 3, 3
    elif name == "gap":
        types, bits = np.asarray([0, 2, 5])[c * 3 // N], 6
    elif name == "types63":
        types, bits = (c * 63 // N if N >= 63 else c % 63), 63
    else:
        types, bits = c * 4 // N, 4
    allowed = rng.integers(0, 1 << bits, Q, dtype=np.int64)
    allowed[0] = 0
    if Q > 1:
        allowed[1] = (1 << bits) - 1
    if name == "own":
        allowed = np.int64(1) << types[target]
    elif name == "not_own":
        allowed = ((1 << bits) - 1) & ~(np.int64(1) << types[target])
    elif name == "one_type":
        allowed = np.int64(1) << ((np.arange(Q) // 128 * 3 + 2) % 4)
    return types.astype(np.int64), allowed.astype(np.int64)


def _filters(rng, Q, N, target):
    """Sorted lists over candidates of every type: one holding the target, an empty one, one covering a whole candidate tile
    (and the whole of the last partial tile), random ones elsewhere."""
    lists = []
    for i in range(Q):
        kind = i % 5
        if kind == 0:
            l = set(rng.integers(0, N, 3).tolist()) | {int(target[i])}
        elif kind == 1:
            l = set()
        elif kind == 2:
            lo = 128 if N >= 256 else 0
            l = set(range(lo, min(N, lo + 128))) | set(range(N - N % 128, N))
        else:
            l = set(rng.integers(0, N, int(rng.integers(1, 12))).tolist())
        lists.append(sorted(l))
    ptr = np.cumsum([0] + [len(l) for l in lists]).astype(np.int64)
    idx = np.asarray([c for l in lists for c in l], dtype=np.int64)
    return ptr, idx


def _keep(Q, N, target, ptr=None, idx=None):
    keep = np.ones((Q, N), dtype=bool)
    keep[np.arange(Q), target] = False
    if ptr is not None:
        rows = np.repeat(np.arange(Q), np.diff(ptr))
        keep[rows, idx] = False
    return keep


def _admitted(types, allowed):
    ok = (types >= 0) & (types <= 62)
    return (((allowed[:, None] >> np.clip(types, 0, 62)[None, :]) & 1) != 0) & ok[None, :]


@functools.lru_cache(maxsize=None)
def _exact_inputs(shape):
    """Integers in [-3, 3] stored as fp32: every product and partial sum is an integer below 2^24, exact in fp32 in any
    order.  -> inputs, filter, the int64 scores and target scores."""
    Q, N, H = shape
    rng = np.random.default_rng(1000 + Q + N + H)
    query = rng.integers(-3, 4, (Q, H))
    table = rng.integers(-3, 4, (N, H))
    target = rng.integers(0, N, Q)
    target[-1] = N - 1                            # targets in the last (partial) tile
    target[Q // 2] = max(0, N - 2)
    ptr, idx = _filters(rng, Q, N, target)
    s = query.astype(np.int64) @ table.astype(np.int64).T
    t = s[np.arange(Q), target][:, None]
    return query.astype(np.float32), table.astype(np.float32), target, ptr, idx, s, t


def _dev(gpu, *arrays):
    return [th.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays]


def _assert_counts(got, want, what):
    for name, g, w in zip(("greater", "equal", "considered"), got, want):
        assert g.dtype == th.int32 and g.shape == (len(w),)
        assert th.equal(g.cpu().to(th.int64), th.from_numpy(np.asarray(w, dtype=np.int64))), (what, name, g.cpu().tolist(), list(w))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "Q%d-N%d-H%d" % s)
def test_exact_inputs_give_the_int64_counts(shape, layout, gpu):
    from dualmessagepassing_amd.unc_eval import rank_counts_typed
    Q, N, H = shape
    query, table, target, ptr, idx, s, t = _exact_inputs(shape)
    types, allowed = _layout(layout, np.random.default_rng(7 + Q + N), Q, N, target)
    adm = _admitted(types, allowed)
    q, x, tg, p, ix, ty, al = _dev(gpu, query, table, target, ptr, idx, types, allowed)
    for f, fd in (((), ()), ((ptr, idx), (p, ix))):
        keep = _keep(Q, N, target, *f) & adm
        want = (((s > t) & keep).sum(1), ((s == t) & keep).sum(1), keep.sum(1))
        _assert_counts(rank_counts_typed(q, x, tg, ty, al, *fd), want, (layout, bool(f)))
    if layout == "own" and N > 1:
        assert (adm.sum(1) < N).any()                                        # the layout does restrict
    if layout == "not_own":
        assert not adm[np.arange(Q), target].any()                          # a target of a non-admitted type, scored all the same
    if N >= 256:
        rows = np.repeat(np.arange(Q), np.diff(ptr))
        assert (~adm[rows, idx]).any() and adm[rows, idx].any()             # filter entries of both kinds


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "Q%d-N%d-H%d" % s)
def test_every_type_admitted_equals_the_untyped_kernel(shape, gpu):
    from dualmessagepassing_amd.unc_eval import rank_counts, rank_counts_typed
    Q, N, H = shape
    query, table, target, ptr, idx, _, _ = _exact_inputs(shape)
    types, _ = _layout("sorted", np.random.default_rng(1), Q, N, target)
    q, x, tg, p, ix, ty = _dev(gpu, query, table, target, ptr, idx, types)
    every = th.full((Q,), -1, dtype=th.int64, device=gpu)              # all 64 bits: bit 63 is ignored
    listed = np.asarray([len(set(idx[ptr[i]:ptr[i + 1]].tolist()) - {int(target[i])}) for i in range(Q)])
    for fd, gone in (((), np.zeros(Q, dtype=np.int64)), ((p, ix), listed)):
        g, e = rank_counts(q, x, tg, *fd)
        gt, et, ct = rank_counts_typed(q, x, tg, ty, every, *fd)
        assert th.equal(g, gt) and th.equal(e, et)
        assert ct.cpu().tolist() == (N - 1 - gone).tolist()


@functools.lru_cache(maxsize=None)
def _random_case(H):
    """Standard normal Q = 96, N = 1000, four types in ranges, a random mask per row; table rows 7 and 200 copy row 3 (one
    type), the first four targets are 3, 7, 200, 3 and their rows admit that type.  -> inputs and the fp64 bracket [lo, hi]
    of greater / greater + equal."""
    Q, N = 96, 1000
    rng = np.random.default_rng(2024 + H)
    query = rng.standard_normal((Q, H)).astype(np.float32)
    table = rng.standard_normal((N, H)).astype(np.float32)
    table[7] = table[3]
    table[200] = table[3]
    target = rng.integers(0, N, Q)
    target[:4] = [3, 7, 200, 3]
    types, allowed = _layout("sorted", rng, Q, N, target)
    allowed[:4] |= 1
    q64, x64 = query.astype(np.float64), table.astype(np.float64)
    s = q64 @ x64.T
    t = s[np.arange(Q), target][:, None]
    # every score is one fp32 fmaf chain of H terms: |fl(s) - s| <= gamma_H sum |q x|, gamma_H = H u / (1 - H u), u = 2^-24, so
    # the computed s - t is off by at most gamma_H sum_h |q_ih| (|x_ch| + |x_th|).  The kernel uses the exact f32-input MFMA
    # (no dropped bf16 cross terms), so the margin's factor is 2: the bound itself and as much again in slack.
    u = 2.0 ** -24
    gamma = H * u / (1 - H * u)
    aq, ax = np.abs(q64), np.abs(x64)
    d = 2 * gamma * (aq @ ax.T + (aq * ax[target]).sum(1)[:, None])
    keep = _keep(Q, N, target) & _admitted(types, allowed)
    lo = ((s - t > d) & keep).sum(1)
    hi = ((s - t >= -d) & keep).sum(1)
    return query, table, target, types, allowed, lo, hi, keep.sum(1)


@pytest.mark.parametrize("H", RANDOM_WIDTHS)
def test_random_inputs_stay_inside_the_fp64_bracket_and_repeat_bitwise(H, gpu):
    from dualmessagepassing_amd.unc_eval import rank_counts_typed
    query, table, target, types, allowed, lo, hi, cons = _random_case(H)
    Q, N = query.shape[0], table.shape[0]
    undecided = float((hi - lo).sum()) / (Q * N)
    print("H=%d undecided share %.3g" % (H, undecided))
    assert undecided <= 2e-3, undecided           # else the bracket decides nothing
    q, x, tg, ty, al = _dev(gpu, query, table, target, types, allowed)
    g, e, c = rank_counts_typed(q, x, tg, ty, al)
    gc, ec = g.cpu().numpy().astype(np.int64), e.cpu().numpy().astype(np.int64)
    assert (lo <= gc).all() and (gc + ec <= hi).all(), (np.flatnonzero(lo > gc).tolist(), np.flatnonzero(gc + ec > hi).tolist())
    assert c.cpu().tolist() == cons.tolist()
    # a candidate whose table row equals the target's row bit for bit ties with it: rows 3, 7, 200 are one row of one type
    assert (ec[:4] >= 2).all(), ec[:4].tolist()
    # integer partial counts: a second call gives the same vectors
    g2, e2, c2 = rank_counts_typed(q, x, tg, ty, al)
    assert th.equal(g, g2) and th.equal(e, e2) and th.equal(c, c2)


def _hetero(rng, n, m):
    """Nodes of three types (ids interleaved: type = id % 3), relations 0: type 0 -> 1, 1: type 1 -> 2, 2: type 0 -> 2."""
    ntype = np.arange(n) % 3
    pair = np.asarray([(0, 1), (1, 2), (0, 2)])
    r = rng.integers(0, 3, m)
    s = rng.integers(0, n // 3, m) * 3 + pair[r, 0]
    o = rng.integers(0, n // 3, m) * 3 + pair[r, 1]
    return ntype, np.unique(np.stack([s, r, o], 1), axis=0)


def test_link_ranks_kernel_route_equals_the_tensor_route(gpu):
    """Integer embeddings: both routes are exact.  The kernel route ranks against the type-sorted table with the queries
    sorted by mask, the tensor route (fp64 embeddings are not the kernel's) in the caller's order."""
    from dualmessagepassing_amd import unc_eval
    rng = np.random.default_rng(11)
    n = 300
    ntype, trip = _hetero(rng, n, 900)
    emb = th.from_numpy(rng.integers(-3, 4, (n, 40)).astype(np.float32)).to(gpu)
    w_rel = th.from_numpy(rng.integers(-2, 3, (3, 40)).astype(np.float32)).to(gpu)
    known = th.from_numpy(trip).to(gpu)
    test = known[::3]
    nt = th.from_numpy(ntype).to(gpu)
    calls = []
    orig = unc_eval.rank_counts_typed
    unc_eval.rank_counts_typed = lambda q, x, *a, **k: (calls.append(unc_eval._on_kernel(q, x)), orig(q, x, *a, **k))[1]
    try:
        for kn in (None, known):
            rk, ck = unc_eval.link_ranks(w_rel, emb, test, known=kn, node_type=nt, return_considered=True)
            rt, ct = unc_eval.link_ranks(w_rel.double(), emb.double(), test, known=kn, node_type=nt, return_considered=True)
            assert th.equal(rk, rt) and th.equal(ck, ct)
            assert int(ck.max()) <= n // 3
    finally:
        unc_eval.rank_counts_typed = orig
    assert calls == [True, True, False, False] * 2          # the first of every pair did take the kernel
    untyped = unc_eval.link_ranks(w_rel, emb, test, known=known)
    assert bool((rk <= untyped).all()) and bool((rk < untyped).any())


def test_bad_type_codes_and_null_arrays_are_refused_without_a_fault(gpu):
    """A NULL type array, mask array or workspace is DMP_ERR_BAD_ARG from the host, before any launch.  A type code of 63 or
    above lies in device memory: the entry does not wait for the device, so it cannot return it; the status word on the
    device says DMP_RANK_BAD_TYPE, and such a candidate is admitted by no row, whatever its mask.  (``link_ranks`` refuses
    such a ``node_type`` on the host: tests/test_unc_eval_typed_cpu.py.)  Every pointer handed over is valid."""
    from dualmessagepassing_amd import _abi, _lib
    from dualmessagepassing_amd.unc_eval import rank_counts_typed
    shape = (70, 333, 50)
    Q, N, H = shape
    query, table, target, ptr, idx, s, t = _exact_inputs(shape)
    types, _ = _layout("sorted", np.random.default_rng(1), Q, N, target)
    types = types.copy()
    bad = [c for c in (5, 130, 332) if c not in set(target.tolist())]
    types[bad] = [63, 64, 255][:len(bad)]
    allowed = np.full(Q, -1, dtype=np.int64)
    q, x, tg, ty, al = _dev(gpu, query, table, target, types, allowed)
    status = th.full((1,), 7, dtype=th.int64, device=gpu)
    keep = _keep(Q, N, target)
    keep[:, bad] = False
    got = rank_counts_typed(q, x, tg, ty, al, status=status)
    _assert_counts(got, (((s > t) & keep).sum(1), ((s == t) & keep).sum(1), keep.sum(1)), "bad codes")
    assert status.item() == _abi.DMP_RANK_BAD_TYPE
    types[bad] = 0
    rank_counts_typed(q, x, tg, th.from_numpy(types).to(gpu), al, status=status)
    assert status.item() == 0                                            # zeroed by every call
    # NULL arrays, straight at the C entry
    lib = _lib.load()
    ty8 = ty.to(th.uint8)
    g, e, c = (th.zeros(Q, dtype=th.int32, device=gpu) for _ in range(3))
    ws = th.zeros(lib.dmp_rank_typed_workspace_words(N), dtype=th.int64, device=gpu)
    args = [q, x, tg, None, None, 0, ty8, al, Q, N, H, g, e, c, ws, None]
    for hole in (6, 7, 14):
        a = [v.data_ptr() if isinstance(v, th.Tensor) else v for v in args]
        a[hole] = None
        assert lib.dmp_rank_counts_typed(*a, _lib.stream_ptr()) == -1
    th.cuda.synchronize()
    assert int(g.sum()) == 0 and int(c.sum()) == 0                       # nothing was launched
    with pytest.raises(_lib.DmpError):
        rank_counts_typed(th.zeros(4, 257, device=gpu), th.zeros(9, 257, device=gpu), th.zeros(4, dtype=th.int64, device=gpu),
                          th.zeros(9, dtype=th.uint8, device=gpu), th.ones(4, dtype=th.int64, device=gpu))


def test_typed_evaluation_end_to_end_on_three_node_types(gpu):
    """240 nodes of three types, three relations each between a fixed pair of types, 10 % of the links held out, a few
    epochs of the training of test_gpu_unc_harness.py: ``evaluate_links(node_type=..., by_relation=True)`` ranks every query
    against fewer than N - 1 candidates, no typed rank is worse than the untyped rank of the same query on the same
    embeddings, and the per-relation query counts add up to the test links times the two sides."""
    from dualmessagepassing_amd import unc_eval
    from dualmessagepassing_amd.unc import TrainModel
    from dualmessagepassing_amd.unc_harness import (collect_node_embeddings, evaluate_links, graph_of, split_links,
                                                    train_unsupervised)
    rng = np.random.default_rng(7)
    n = 240
    ntype, trip = _hetero(rng, n, 1500)
    train, test = split_links(th.from_numpy(trip), 0.1, seed=5)
    graph, train = graph_of(train.numpy(), n, 3, gpu)
    test = test.to(gpu)
    nt = th.from_numpy(ntype).to(gpu)
    th.manual_seed(0)
    model = TrainModel(None, n, 64, 3, 0, num_hidden_layers=2, dropout=0.0, reg_param=0.01).to(gpu)
    sampling = dict(graph_batch_size=300, sampler="neighbor", sample_depth=2, sample_width=8, negative_sample=3, seed=2)
    train_unsupervised(model, graph, train, n_epochs=3, graph_batch_size=300, lr=5e-3, sampler="neighbor", sample_depth=2,
                       sample_width=8, negative_sample=3, rescale_epochs=False, seed=1)
    plain = evaluate_links(model, graph, train, test, **sampling)
    typed = evaluate_links(model, graph, train, test, node_type=nt, by_relation=True, **sampling)
    print("typed MRR %.4f MR %.2f AMRI %.4f candidates %.1f; untyped MRR %.4f MR %.2f" %
          (typed["MRR"], typed["MR"], typed["AMRI"], typed["candidates"], plain["MRR"], plain["MR"]))
    assert "AMRI" not in plain and "relation/0/MRR" not in plain
    assert 0 < typed["candidates"] < n - 1 and typed["candidates"] <= n // 3
    assert typed["object/candidates"] < n - 1 and typed["subject/candidates"] < n - 1
    assert -1.0 <= typed["AMRI"] <= 1.0
    counts = [typed["relation/%d/count" % r] for r in range(3)]
    assert sum(counts) == 2 * test.size(0) and all(k > 0 for k in counts)
    assert counts == [2 * int((test[:, 1] == r).sum()) for r in range(3)]
    for key in ("MRR", "MR", "Hits@10"):          # the block is a partition of the queries
        assert sum(typed["relation/%d/%s" % (r, key)] * counts[r] for r in range(3)) / sum(counts) == pytest.approx(typed[key], rel=1e-12)
    # per query, on one set of embeddings
    emb, _ = collect_node_embeddings(model, graph, train, **sampling)
    known = th.cat([train, test])
    raw = unc_eval.link_ranks(model.w_relation, emb, test, known=known)
    ranks, cons = unc_eval.link_ranks(model.w_relation, emb, test, known=known, node_type=nt, return_considered=True)
    assert bool((ranks <= raw).all())
    assert bool((cons < n // 3).all())
