"""The fused score-and-rank kernel (csrc/dmp_rank.hip through unc_eval.rank_counts) against its definition restated on the
CPU -- in int64 where the inputs make every score exact, in fp64 with a rounding bracket where they do not -- and the
ranking evaluation end to end on the two-community graph of the UNC harness test."""
import functools

import numpy as np
import pytest
import torch as th

pytestmark = pytest.mark.gpu

# (Q, N, H); a workgroup owns 128 queries and candidate tiles of 128, and one query tile's candidates are split over
# workgroups from five tiles on (N > 512): 513 and 600 lie just past that, 5000 takes ten splits
EXACT_SHAPES = [(70, 333, 50), (1, 1, 1), (33, 5000, 64), (70, 333, 130), (64, 256, 256), (70, 513, 50), (130, 600, 33)]
RANDOM_WIDTHS = [50, 64, 256]


def _filters(rng, Q, N, target):
    """Sorted lists per query: one holding the target, an empty one, one covering a whole candidate tile (and the whole of
    the last partial tile), random ones elsewhere."""
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


@functools.lru_cache(maxsize=None)
def _exact_case(shape):
    """Integers in [-3, 3] stored as fp32: every product and partial sum is an integer below 2^24, exact in fp32 in any
    order.  -> inputs, filter and the int64 counts without / with the filter."""
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
    want = []
    for f in ((), (ptr, idx)):
        keep = _keep(Q, N, target, *f)
        want.append((((s > t) & keep).sum(1), ((s == t) & keep).sum(1)))
    ties = ((s == t).sum() - Q) / max(1, Q * (N - 1))
    return query.astype(np.float32), table.astype(np.float32), target, ptr, idx, want, ties


def _dev(gpu, *arrays):
    return [th.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays]


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=lambda s: "Q%d-N%d-H%d" % s)
def test_exact_inputs_give_the_int64_counts(shape, gpu):
    from dualmessagepassing_amd.unc_eval import rank_counts
    query, table, target, ptr, idx, want, ties = _exact_case(shape)
    q, x, tg, p, ix = _dev(gpu, query, table, target, ptr, idx)
    if shape[1] >= 256 and shape[2] >= 33:
        assert 0.002 < ties < 0.2, ties           # the inputs do tie (about 1 % at the wide shapes)
    for f, (wg, we) in zip(((), (p, ix)), want):
        g, e = rank_counts(q, x, tg, *f)
        assert g.dtype == th.int32 and e.dtype == th.int32 and g.shape == (shape[0],)
        assert th.equal(g.cpu().to(th.int64), th.from_numpy(wg)), (g.cpu().tolist(), wg.tolist())
        assert th.equal(e.cpu().to(th.int64), th.from_numpy(we)), (e.cpu().tolist(), we.tolist())
    assert (want[0][0] != want[1][0]).any() or (want[0][1] != want[1][1]).any() or shape[1] == 1      # the filter matters


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=lambda s: "Q%d-N%d-H%d" % s)
def test_kernel_route_equals_the_tensor_route_on_exact_inputs(shape, gpu):
    """The route, not the definition: the same call through ``rank_counts_tensor`` on the GPU."""
    from dualmessagepassing_amd.unc_eval import rank_counts, rank_counts_tensor
    query, table, target, ptr, idx, _, _ = _exact_case(shape)
    q, x, tg, p, ix = _dev(gpu, query, table, target, ptr, idx)
    for f in ((), (p, ix)):
        g, e = rank_counts(q, x, tg, *f)
        g2, e2 = rank_counts_tensor(q, x, tg, *f)
        assert th.equal(g, g2) and th.equal(e, e2)


@functools.lru_cache(maxsize=None)
def _random_case(H):
    """Standard normal Q = 96, N = 1000; table rows 7 and 500 copy row 3, the first four targets are 3, 7, 500, 3.  -> inputs
    and the fp64 bracket [lo, hi] of greater / greater + equal."""
    Q, N = 96, 1000
    rng = np.random.default_rng(2024 + H)
    query = rng.standard_normal((Q, H)).astype(np.float32)
    table = rng.standard_normal((N, H)).astype(np.float32)
    table[7] = table[3]
    table[500] = table[3]
    target = rng.integers(0, N, Q)
    target[:4] = [3, 7, 500, 3]
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
    keep = _keep(Q, N, target)
    lo = ((s - t > d) & keep).sum(1)
    hi = ((s - t >= -d) & keep).sum(1)
    return query, table, target, lo, hi


@pytest.mark.parametrize("H", RANDOM_WIDTHS)
def test_random_inputs_stay_inside_the_fp64_bracket_and_repeat_bitwise(H, gpu):
    from dualmessagepassing_amd.unc_eval import rank_counts
    query, table, target, lo, hi = _random_case(H)
    Q, N = query.shape[0], table.shape[0]
    undecided = float((hi - lo).sum()) / (Q * N)
    print("H=%d undecided share %.3g" % (H, undecided))
    assert undecided <= 2e-3, undecided           # else the bracket decides nothing
    q, x, tg = _dev(gpu, query, table, target)
    g, e = rank_counts(q, x, tg)
    gc, ec = g.cpu().numpy().astype(np.int64), e.cpu().numpy().astype(np.int64)
    assert (lo <= gc).all() and (gc + ec <= hi).all(), (np.flatnonzero(lo > gc).tolist(), np.flatnonzero(gc + ec > hi).tolist())
    # a candidate whose table row equals the target's row bit for bit ties with it: rows 3, 7, 500 are one row
    assert (ec[:4] >= 2).all(), ec[:4].tolist()
    # integer partial counts: a second call gives the same vectors
    g2, e2 = rank_counts(q, x, tg)
    assert th.equal(g, g2) and th.equal(e, e2)


def test_nan_scores_count_nowhere_and_bad_widths_are_refused(gpu):
    from dualmessagepassing_amd import _lib
    from dualmessagepassing_amd.unc_eval import rank_counts
    query, table, target, _, _, want, _ = _exact_case((70, 333, 50))
    table = table.copy()
    bad = [5, 200, 332]
    bad = [c for c in bad if c not in set(target.tolist())]
    table[bad, 0] = np.nan
    q, x, tg = _dev(gpu, query, table, target)
    g, e = rank_counts(q, x, tg)
    s = query.astype(np.float64) @ np.nan_to_num(table, nan=0.0).astype(np.float64).T
    t = s[np.arange(70), target][:, None]
    keep = _keep(70, 333, target)
    keep[:, bad] = False
    assert g.cpu().tolist() == ((s > t) & keep).sum(1).tolist() and e.cpu().tolist() == ((s == t) & keep).sum(1).tolist()
    with pytest.raises(_lib.DmpError):
        rank_counts(th.zeros(4, 257, device=gpu), th.zeros(9, 257, device=gpu), th.zeros(4, dtype=th.int64, device=gpu))


def _two_communities(rng, n=240, m=1500):
    half = n // 2
    u = rng.integers(0, n, 4 * m)
    v = rng.integers(0, n, 4 * m)
    same = (u < half) == (v < half)
    keep = (u != v) & (same | (rng.random(4 * m) < 0.03))          # mostly intra-community edges
    pairs = np.unique(np.stack([u[keep], v[keep]], 1), axis=0)[:m]
    return np.stack([pairs[:, 0], np.zeros(len(pairs), np.int64), pairs[:, 1]], 1)


@pytest.mark.parametrize("replay", [False, True], ids=["eager", "replay"])
def test_training_raises_the_filtered_mrr_of_held_out_links(replay, gpu):
    """Two communities of 120 nodes, 10 % of the links held out, the training of test_gpu_unc_harness.py on the rest: the
    filtered MRR of the held-out links is above the untrained model's (same seed), above a random ranking's expectation
    (1/N) sum_{k <= N} 1/k = 0.0252 and not below the raw MRR; no query's filtered rank is worse than its raw rank.
    Measured on an MI355X (profiles/unc_rank_e2e.json): filtered MRR 0.0324 before the training, 0.0569 after it (0.0590 with
    ``replay=True``), raw MRR after it 0.0518 (0.0536)."""
    from dualmessagepassing_amd import unc_eval
    from dualmessagepassing_amd.unc import TrainModel
    from dualmessagepassing_amd.unc_harness import (collect_node_embeddings, evaluate_links, graph_of, split_links,
                                                    train_unsupervised)
    rng = np.random.default_rng(7)
    n = 240
    trip_all = th.from_numpy(_two_communities(rng, n))
    train, test = split_links(trip_all, 0.1, seed=5)
    assert test.size(0) == round(0.1 * trip_all.size(0))
    graph, train = graph_of(train.numpy(), n, 1, gpu)
    test = test.to(gpu)
    th.manual_seed(0)
    model = TrainModel(None, n, 64, 1, 0, num_hidden_layers=2, dropout=0.0, reg_param=0.01).to(gpu)
    sampling = dict(graph_batch_size=300, sampler="neighbor", sample_depth=2, sample_width=8, negative_sample=3, seed=2)
    before = evaluate_links(model, graph, train, test, **sampling)
    train_unsupervised(model, graph, train, n_epochs=6, graph_batch_size=300, lr=5e-3, sampler="neighbor", sample_depth=2,
                       sample_width=8, negative_sample=3, rescale_epochs=False, seed=1, replay=replay)
    after = evaluate_links(model, graph, train, test, **sampling)
    emb, _ = collect_node_embeddings(model, graph, train, **sampling)
    known = th.cat([train, test])
    raw = unc_eval.link_ranks(model.w_relation, emb, test)
    filt = unc_eval.link_ranks(model.w_relation, emb, test, known=known)
    raw_mrr, filt_mrr = unc_eval.link_metrics(raw)["MRR"], unc_eval.link_metrics(filt)["MRR"]
    random_mrr = sum(1.0 / k for k in range(1, n + 1)) / n
    print("replay=%s filtered MRR before %.4f after %.4f raw MRR after %.4f (filtered on the same embeddings %.4f) random %.4f" %
          (replay, before["MRR"], after["MRR"], raw_mrr, filt_mrr, random_mrr))
    assert set(after) >= {"MRR", "MR", "Hits@1", "Hits@3", "Hits@10", "object/MRR", "subject/MRR"}
    assert after["MRR"] > before["MRR"]
    assert after["MRR"] > random_mrr
    assert bool((filt <= raw).all()) and filt_mrr >= raw_mrr
