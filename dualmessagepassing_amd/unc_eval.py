"""Ranking evaluation of the UNC link predictor (``unc.TrainModel``'s DistMult head: ``w_relation`` / ``calc_score``):
filtered MRR, mean rank and Hits@k of held-out links.  The reference's UNC drivers stop at writing the embeddings
(main.py:185-211) and score them with sklearn's LinearSVC, which stays out of scope; this is the decoder's own
measure.

* ``rank_counts``: per query, how many candidates score above / exactly at the target -- on the GPU one launch of
  ``dmp_rank_counts`` (csrc/dmp_rank.hip), which never stores the ``[Q, N]`` scores; ``rank_counts_tensor`` is the same
  function in tensor ops (the CPU path and the timing yardstick);
* ``known_filter``: the CSR of known true candidates per query (the "filtered" setting);
* ``link_ranks`` / ``link_metrics``: DistMult queries for both sides, tie policy, MRR / MR / Hits@k.
"""
import torch

from . import _lib

TENSOR_SCORE_BYTES = 1 << 28         # live score block of ``rank_counts_tensor`` unless the caller says otherwise
TIE_POLICIES = ("mean", "optimistic", "pessimistic")


def rows_per_chunk(num_candidates, itemsize, budget_bytes):
    """Query rows of one chunk of ``rank_counts_tensor``: the most whose ``[rows, N]`` score block stays within the budget."""
    return max(1, int(budget_bytes) // max(1, int(num_candidates) * int(itemsize)))


def _check(query, table, target, filt_ptr, filt_idx):
    if query.dim() != 2 or table.dim() != 2 or query.size(1) != table.size(1):
        raise ValueError("query [Q, H] and table [N, H] expected, got %s and %s" % (tuple(query.shape), tuple(table.shape)))
    if table.size(0) < 1 or query.size(1) < 1:
        raise ValueError("the table needs at least one row and one column")
    if target.dim() != 1 or target.size(0) != query.size(0):
        raise ValueError("target [Q] expected, got %s" % (tuple(target.shape),))
    if (filt_ptr is None) != (filt_idx is None):
        raise ValueError("filt_ptr and filt_idx come together")
    if filt_ptr is not None and (filt_ptr.dim() != 1 or filt_ptr.size(0) != query.size(0) + 1):
        raise ValueError("filt_ptr [Q + 1] expected, got %s" % (tuple(filt_ptr.shape),))


@torch.no_grad()
def rank_counts_tensor(query, table, target, filt_ptr=None, filt_idx=None, budget_bytes=TENSOR_SCORE_BYTES):
    """``rank_counts`` in tensor ops, chunked over the queries so that the live ``[rows, N]`` score block stays within
    ``budget_bytes``.  The target's score is read out of the same product as every candidate's."""
    _check(query, table, target, filt_ptr, filt_idx)
    Q, N = query.size(0), table.size(0)
    dev = query.device
    target = target.to(torch.int64)
    greater = torch.zeros(Q, dtype=torch.int32, device=dev)
    equal = torch.zeros(Q, dtype=torch.int32, device=dev)
    step = rows_per_chunk(N, query.element_size(), budget_bytes)
    starts = list(range(0, Q, step))
    bounds = None
    if filt_ptr is not None:
        filt_ptr = filt_ptr.to(torch.int64)
        bounds = filt_ptr[torch.tensor(starts + [Q], dtype=torch.int64, device=filt_ptr.device)].tolist()
    table_t = table.t()
    for n, q0 in enumerate(starts):
        q1 = min(Q, q0 + step)
        s = query[q0:q1] @ table_t
        tgt = target[q0:q1].view(-1, 1)
        t = s.gather(1, tgt)
        keep = torch.ones(q1 - q0, N, dtype=torch.bool, device=dev)
        keep.scatter_(1, tgt, False)
        if bounds is not None and bounds[n + 1] > bounds[n]:
            counts = filt_ptr[q0 + 1:q1 + 1] - filt_ptr[q0:q1]
            rows = torch.repeat_interleave(torch.arange(q1 - q0, device=dev), counts, output_size=bounds[n + 1] - bounds[n])
            keep[rows, filt_idx[bounds[n]:bounds[n + 1]].to(torch.int64)] = False
        greater[q0:q1] = ((s > t) & keep).sum(1).to(torch.int32)
        equal[q0:q1] = ((s == t) & keep).sum(1).to(torch.int32)
    return greater, equal


def _on_kernel(query, table):
    return (query.is_cuda and table.is_cuda and query.dtype == torch.float32 and table.dtype == torch.float32
            and query.is_contiguous() and table.is_contiguous())


@torch.no_grad()
def rank_counts(query, table, target, filt_ptr=None, filt_idx=None):
    """For every query row ``i`` with ``score(i, c) = query[i] . table[c]`` and ``t_i = score(i, target[i])``:
    ``greater[i]`` / ``equal[i]`` = the number of candidates ``c != target[i]``, ``c`` not in the row's filter list
    (``filt_idx[filt_ptr[i]:filt_ptr[i + 1]]``, ascending), that score above / exactly at ``t_i``.  Two int32 ``[Q]``.

    fp32 contiguous tensors on the GPU: one launch of ``dmp_rank_counts`` on the current stream, no host sync, nothing
    allocated beyond the two outputs (a width the kernel does not take is an error, not a detour).  Anything else (CPU,
    other dtypes, strided views): ``rank_counts_tensor``."""
    if not _on_kernel(query, table):
        return rank_counts_tensor(query, table, target, filt_ptr, filt_idx)
    _check(query, table, target, filt_ptr, filt_idx)
    Q, H, N = query.size(0), query.size(1), table.size(0)
    lib = _lib.load()
    if not lib.dmp_rank_supported(H):
        raise _lib.DmpError("dmp_rank_counts takes 1 <= H <= 256, got H = %d" % H)
    target = target.to(device=query.device, dtype=torch.int64).contiguous()
    nnz = 0
    if filt_ptr is not None:
        filt_ptr = filt_ptr.to(device=query.device, dtype=torch.int64).contiguous()
        filt_idx = filt_idx.to(device=query.device, dtype=torch.int64).contiguous()
        nnz = filt_idx.numel()
    _lib.require_gpu(query, table, target, filt_ptr, filt_idx)
    greater = torch.empty(Q, dtype=torch.int32, device=query.device)
    equal = torch.empty(Q, dtype=torch.int32, device=query.device)
    _lib.pin_for_capture(target, filt_ptr, filt_idx)
    with _lib.timed("rank_counts_h%d", (H,), 4 * (Q + N) * H):
        code = lib.dmp_rank_counts(_lib.ptr(query), _lib.ptr(table), _lib.ptr(target), _lib.ptr(filt_ptr),
                                   _lib.ptr(filt_idx) if nnz else None, nnz, Q, N, H, _lib.ptr(greater), _lib.ptr(equal),
                                   _lib.stream_ptr())
    _lib.check(code, "dmp_rank_counts")
    return greater, equal


@torch.no_grad()
def known_filter(triplets_known, queries_sr, num_rels, side):
    """The CSR of known true candidates per query.  ``triplets_known`` [M, 3] (s, r, o); ``queries_sr`` [Q, 2]: the fixed
    entity and the relation of every query.  ``side="object"``: the fixed entity is the subject, the list every ``o'`` with
    ``(s, r, o')`` known; ``side="subject"``: the fixed entity is the object, the list every ``s'`` with ``(s', r, o)`` known.
    -> ``(filt_ptr int64 [Q + 1], filt_idx int64)``, ascending and without repeats inside a row.  Index building on the
    device (sort / searchsorted; two host reads of a size)."""
    if side not in ("object", "subject"):
        raise ValueError("side is 'object' or 'subject', got %r" % (side,))
    known = triplets_known[:, :3].to(torch.int64)
    queries = queries_sr.to(device=known.device, dtype=torch.int64)
    fixed, cand = (known[:, 0], known[:, 2]) if side == "object" else (known[:, 2], known[:, 0])
    pairs = torch.unique(torch.stack([fixed * num_rels + known[:, 1], cand], 1), dim=0)       # sorted by (key, candidate)
    keys = pairs[:, 0].contiguous()
    qkey = queries[:, 0] * num_rels + queries[:, 1]
    lo = torch.searchsorted(keys, qkey, right=False)
    hi = torch.searchsorted(keys, qkey, right=True)
    counts = hi - lo
    ptr = torch.zeros(queries.size(0) + 1, dtype=torch.int64, device=known.device)
    torch.cumsum(counts, 0, out=ptr[1:])
    total = int(ptr[-1])
    first = torch.repeat_interleave(lo - ptr[:-1], counts, output_size=total)
    idx = pairs[:, 1][first + torch.arange(total, device=known.device)]
    return ptr, idx


def ranks_of(greater, equal, ties="mean"):
    """Float ranks from the two counts: ``mean`` 1 + greater + equal / 2 (a collapsed embedding, every score equal, ranks
    in the middle instead of first), ``optimistic`` 1 + greater, ``pessimistic`` 1 + greater + equal."""
    if ties not in TIE_POLICIES:
        raise ValueError("ties is one of %s, got %r" % (TIE_POLICIES, ties))
    g, e = greater.to(torch.float64), equal.to(torch.float64)
    return 1.0 + g + {"mean": 0.5, "optimistic": 0.0, "pessimistic": 1.0}[ties] * e


@torch.no_grad()
def link_ranks(w_relation, node_emb, triplets, known=None, sides=("object", "subject"), ties="mean"):
    """Ranks of the true entity of every triplet under DistMult, ``score(s, r, o) = sum(emb[s] * w_relation[r] * emb[o])``.
    Object side: the query ``emb[s] * w_relation[r]`` against every node, target ``o``; subject side: ``emb[o] *
    w_relation[r]``, target ``s``.  ``known`` [M, 3]: the triplets whose entities are filtered out of a query's candidates
    (usually training + test links; the target itself always stays).  -> float64 ranks ``[T, len(sides)]``."""
    triplets = triplets[:, :3].to(torch.int64)
    w_relation, node_emb = w_relation.detach(), node_emb.detach()
    table = node_emb.contiguous()
    out = []
    for side in sides:
        if side not in ("object", "subject"):
            raise ValueError("sides holds 'object' / 'subject', got %r" % (side,))
        fixed, tgt = (triplets[:, 0], triplets[:, 2]) if side == "object" else (triplets[:, 2], triplets[:, 0])
        query = (node_emb[fixed] * w_relation[triplets[:, 1]]).contiguous()
        ptr = idx = None
        if known is not None:
            ptr, idx = known_filter(known, torch.stack([fixed, triplets[:, 1]], 1), w_relation.size(0), side)
        g, e = rank_counts(query, table, tgt, ptr, idx)
        out.append(ranks_of(g, e, ties))
    return torch.stack(out, 1)


@torch.no_grad()
def link_metrics(ranks, ks=(1, 3, 10), sides=("object", "subject")):
    """``{"MRR", "MR", "Hits@k" ...}`` over every rank, and the same under ``"<side>/"`` per column.  One host sync."""
    ranks = ranks.view(ranks.size(0), -1).to(torch.float64)
    names = ["%s/" % s for s in sides[:ranks.size(1)]] if ranks.size(1) == len(sides) else ["side%d/" % i for i in range(ranks.size(1))]
    cols = [ranks.reshape(-1)] + [ranks[:, i] for i in range(ranks.size(1))]
    rows = torch.stack([torch.stack([(1.0 / c).mean(), c.mean()] + [(c <= k).to(torch.float64).mean() for k in ks]) for c in cols])
    rows = rows.tolist()
    out = {}
    for prefix, row in zip([""] + names, rows):
        out[prefix + "MRR"], out[prefix + "MR"] = row[0], row[1]
        for k, v in zip(ks, row[2:]):
            out[prefix + "Hits@%d" % k] = v
    return out
