"""Ranking evaluation of the UNC link predictor (``unc.TrainModel``'s DistMult head: ``w_relation`` / ``calc_score``):
filtered MRR, mean rank and Hits@k of held-out links.  The reference's UNC drivers stop at writing the embeddings
(main.py:185-211) and score them with sklearn's LinearSVC, which stays out of scope; this is the decoder's own
measure.

* ``rank_counts``: per query, how many candidates score above / exactly at the target -- on the GPU one launch of
  ``dmp_rank_counts`` (csrc/dmp_rank.hip), which never stores the ``[Q, N]`` scores; ``rank_counts_tensor`` is the same
  function in tensor ops (the CPU path and the timing yardstick);
* ``known_filter``: the CSR of known true candidates per query (the "filtered" setting);
* ``link_ranks`` / ``link_metrics``: DistMult queries for both sides, tie policy, MRR / MR / Hits@k;
* ``rank_counts_typed`` / ``relation_type_masks`` / ``link_ranks(node_type=...)``: the type-constrained protocol of
  heterogeneous graphs -- a query is ranked against the nodes of the types its relation joins on that side, on the GPU by
  ``dmp_rank_counts_typed`` (csrc/dmp_rank_typed.hip), which steps over the candidate tiles of other types; ``link_metrics``
  then adds the candidate count and the adjusted mean rank index, ``link_metrics_by_relation`` the per-relation block.
"""
import torch

from . import _lib

TENSOR_SCORE_BYTES = 1 << 28         # live score block of ``rank_counts_tensor`` unless the caller says otherwise
TIE_POLICIES = ("mean", "optimistic", "pessimistic")
MAX_NODE_TYPES = 63                  # type codes 0 .. 62: an admitted-type mask is a non-negative int64


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


def _check_typed(query, table, cand_type, allowed):
    if cand_type.dim() != 1 or cand_type.size(0) != table.size(0):
        raise ValueError("cand_type [N] expected, got %s" % (tuple(cand_type.shape),))
    if allowed.dim() != 1 or allowed.size(0) != query.size(0):
        raise ValueError("allowed [Q] expected, got %s" % (tuple(allowed.shape),))
    if cand_type.dtype.is_floating_point or allowed.dtype.is_floating_point:
        raise ValueError("cand_type and allowed are integer tensors")


@torch.no_grad()
def rank_counts_tensor(query, table, target, filt_ptr=None, filt_idx=None, budget_bytes=TENSOR_SCORE_BYTES):
    """``rank_counts`` in tensor ops, chunked over the queries so that the live ``[rows, N]`` score block stays within
    ``budget_bytes``.  The target's score is read out of the same product as every candidate's."""
    return _counts_tensor(query, table, target, None, None, filt_ptr, filt_idx, budget_bytes)[:2]


@torch.no_grad()
def rank_counts_typed_tensor(query, table, target, cand_type, allowed, filt_ptr=None, filt_idx=None,
                             budget_bytes=TENSOR_SCORE_BYTES):
    """``rank_counts_typed`` in tensor ops, chunked by the budget rule of ``rank_counts_tensor``."""
    _check_typed(query, table, cand_type, allowed)
    return _counts_tensor(query, table, target, cand_type, allowed, filt_ptr, filt_idx, budget_bytes)


def _counts_tensor(query, table, target, cand_type, allowed, filt_ptr, filt_idx, budget_bytes):
    """(greater, equal, considered); ``cand_type`` None: every candidate is admitted."""
    _check(query, table, target, filt_ptr, filt_idx)
    Q, N = query.size(0), table.size(0)
    dev = query.device
    target = target.to(torch.int64)
    greater = torch.zeros(Q, dtype=torch.int32, device=dev)
    equal = torch.zeros(Q, dtype=torch.int32, device=dev)
    considered = torch.zeros(Q, dtype=torch.int32, device=dev)
    if cand_type is not None:
        cand_type = cand_type.to(device=dev, dtype=torch.int64)
        typed_ok = ((cand_type >= 0) & (cand_type < MAX_NODE_TYPES)).view(1, -1)       # any other code: admitted by nobody
        shift = cand_type.clamp(0, MAX_NODE_TYPES - 1).view(1, -1)
        allowed = allowed.to(device=dev, dtype=torch.int64)
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
        if cand_type is not None:
            keep &= (((allowed[q0:q1].view(-1, 1) >> shift) & 1) != 0) & typed_ok
        greater[q0:q1] = ((s > t) & keep).sum(1).to(torch.int32)
        equal[q0:q1] = ((s == t) & keep).sum(1).to(torch.int32)
        considered[q0:q1] = keep.sum(1).to(torch.int32)
    return greater, equal, considered


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
def rank_counts_typed(query, table, target, cand_type, allowed, filt_ptr=None, filt_idx=None, status=None):
    """``rank_counts`` against the candidates of the admitted node types: candidate ``c`` counts for row ``i`` when bit
    ``cand_type[c]`` of ``allowed[i]`` is set (``cand_type`` [N]: codes 0 .. 62, ``allowed`` [Q]: non-negative int64 masks),
    besides ``c != target[i]`` and ``c`` not in the row's filter list; ``t_i`` is the target's score whatever its type.
    -> ``(greater, equal, considered)`` int32 ``[Q]``, ``considered[i]`` the number of candidates row ``i`` was ranked against.

    fp32 contiguous tensors on the GPU: ``dmp_rank_counts_typed`` on the current stream (a pre-pass over the types and the
    ranking launch), no host sync; allocated beyond the outputs: the type bytes, if ``cand_type`` is not uint8 yet, and one
    word per 128 candidates.  The kernel steps over candidate tiles that hold no type a workgroup's 128 rows admit, so it pays
    to order the candidates by type and the queries by mask, as ``link_ranks`` does; any order gives the same counts.  A
    code outside 0 .. 62 is admitted by nobody, and ``status`` (an int64 ``[1]`` tensor on the device, if given) is set to
    ``DMP_RANK_BAD_TYPE`` -- the host cannot see it without a sync, ``link_ranks`` checks its ``node_type`` once instead.
    Anything else (CPU, other dtypes, strided views): ``rank_counts_typed_tensor``."""
    if not _on_kernel(query, table):
        return rank_counts_typed_tensor(query, table, target, cand_type, allowed, filt_ptr, filt_idx)
    _check(query, table, target, filt_ptr, filt_idx)
    _check_typed(query, table, cand_type, allowed)
    Q, H, N = query.size(0), query.size(1), table.size(0)
    lib = _lib.load()
    if not lib.dmp_rank_supported(H):
        raise _lib.DmpError("dmp_rank_counts_typed takes 1 <= H <= 256, got H = %d" % H)
    dev = query.device
    target = target.to(device=dev, dtype=torch.int64).contiguous()
    if cand_type.dtype != torch.uint8:          # (a negative code becomes 255: refused like every code above 62)
        cand_type = cand_type.to(device=dev, dtype=torch.int64).clamp(-1, 255).to(torch.uint8)
    cand_type = cand_type.to(dev).contiguous()
    allowed = allowed.to(device=dev, dtype=torch.int64).contiguous()
    nnz = 0
    if filt_ptr is not None:
        filt_ptr = filt_ptr.to(device=dev, dtype=torch.int64).contiguous()
        filt_idx = filt_idx.to(device=dev, dtype=torch.int64).contiguous()
        nnz = filt_idx.numel()
    _lib.require_gpu(query, table, target, filt_ptr, filt_idx, cand_type, allowed, status)
    if status is not None and (status.dtype != torch.int64 or status.numel() != 1):
        raise ValueError("status is an int64 tensor of one element")
    greater = torch.empty(Q, dtype=torch.int32, device=dev)
    equal = torch.empty(Q, dtype=torch.int32, device=dev)
    considered = torch.empty(Q, dtype=torch.int32, device=dev)
    tile_types = torch.empty(lib.dmp_rank_typed_workspace_words(N), dtype=torch.int64, device=dev)
    _lib.pin_for_capture(target, filt_ptr, filt_idx, cand_type, allowed, tile_types)
    with _lib.timed("rank_counts_typed_h%d", (H,), 4 * (Q + N) * H):
        code = lib.dmp_rank_counts_typed(_lib.ptr(query), _lib.ptr(table), _lib.ptr(target), _lib.ptr(filt_ptr),
                                         _lib.ptr(filt_idx) if nnz else None, nnz, _lib.ptr(cand_type), _lib.ptr(allowed), Q, N, H,
                                         _lib.ptr(greater), _lib.ptr(equal), _lib.ptr(considered), _lib.ptr(tile_types),
                                         _lib.ptr(status), _lib.stream_ptr())
    _lib.check(code, "dmp_rank_counts_typed")
    return greater, equal, considered


def _checked_types(node_type, num_nodes, device):
    """``node_type`` as int64 ``[N]`` on the device (``num_nodes`` None: any length), its codes inside 0 .. 62 (one host read)."""
    if node_type.dtype.is_floating_point or node_type.dim() != 1 or (num_nodes is not None and node_type.size(0) != num_nodes):
        raise ValueError("node_type: integer codes [%s] expected, got %s %s" % ("N" if num_nodes is None else num_nodes, node_type.dtype,
                                                                              tuple(node_type.shape)))
    node_type = node_type.to(device=device, dtype=torch.int64)
    lo, hi = torch.stack(torch.aminmax(node_type)).tolist() if node_type.numel() else (0, 0)
    if lo < 0 or hi >= MAX_NODE_TYPES:
        raise ValueError("node types are codes 0 .. %d (one bit of an int64 mask each), got %d .. %d" % (MAX_NODE_TYPES - 1, lo, hi))
    return node_type


@torch.no_grad()
def relation_type_masks(known, node_type, num_rels):
    """The node types every relation joins, read off the known triplets: int64 ``[num_rels, 2]``, column 0 the OR of
    ``1 << node_type[s]`` over the relation's known ``(s, r, o)``, column 1 the same over ``o``; a relation without a known
    triplet gets 0.  Tensor ops on the device of ``known``; the codes are checked to lie in 0 .. 62 (one host read)."""
    known = known[:, :3].to(torch.int64)
    dev = known.device
    node_type = _checked_types(node_type, None, dev)
    bit = torch.ones((), dtype=torch.int64, device=dev) << torch.arange(MAX_NODE_TYPES, dtype=torch.int64, device=dev)
    out = []
    for col in (0, 2):
        present = torch.zeros(num_rels, MAX_NODE_TYPES, dtype=torch.bool, device=dev)
        present[known[:, 1], node_type[known[:, col]]] = True
        out.append((present.to(torch.int64) * bit).sum(1))
    return torch.stack(out, 1)


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


def _typed_order(query, tgt, allowed, ptr, idx, inv, num_nodes):
    """The typed kernel's order: the queries sorted by mask (a workgroup's 128 rows then share one), targets and filter
    entries mapped into the type-sorted table through ``inv``, the filter rows re-sorted ascending.  -> the reordered
    ``(query, target, allowed, filt_ptr, filt_idx)`` and ``qorder`` (row ``j`` of them is row ``qorder[j]`` of the caller)."""
    Q = query.size(0)
    qorder = torch.argsort(allowed, stable=True)
    if ptr is not None:
        counts = ptr[1:] - ptr[:-1]
        total = idx.numel()
        qpos = torch.empty_like(qorder)
        qpos[qorder] = torch.arange(Q, device=qorder.device)
        rows = torch.repeat_interleave(qpos, counts, output_size=total)
        key = torch.sort(rows * num_nodes + inv[idx]).values          # by (new row, new candidate): one sort for both
        idx = key % num_nodes
        ptr = torch.zeros_like(ptr)
        torch.cumsum(counts[qorder], 0, out=ptr[1:])
    return query[qorder].contiguous(), inv[tgt[qorder]], allowed[qorder], ptr, idx, qorder


@torch.no_grad()
def link_ranks(w_relation, node_emb, triplets, known=None, sides=("object", "subject"), ties="mean", node_type=None,
               type_masks=None, return_considered=False):
    """Ranks of the true entity of every triplet under DistMult, ``score(s, r, o) = sum(emb[s] * w_relation[r] * emb[o])``.
    Object side: the query ``emb[s] * w_relation[r]`` against every node, target ``o``; subject side: ``emb[o] *
    w_relation[r]``, target ``s``.  ``known`` [M, 3]: the triplets whose entities are filtered out of a query's candidates
    (usually training + test links; the target itself always stays).  -> float64 ranks ``[T, len(sides)]``.

    ``node_type`` [N] (codes 0 .. 62): the type-constrained protocol -- a query is ranked against the nodes whose type its
    relation admits on that side, ``type_masks[r, 0]`` for subjects and ``type_masks[r, 1]`` for objects (by default
    ``relation_type_masks`` of ``known``, of ``triplets`` themselves without it), and against the type of its own target in
    any case.  On the kernel route the table is permuted once so that every type is one contiguous range and the queries are
    sorted by mask, which is what lets ``dmp_rank_counts_typed`` step over the tiles of other types; the ranks come back in
    the caller's order.  ``return_considered``: ``(ranks, considered int64 [T, len(sides)])``, the candidates every query was
    ranked against (all but the target and the filtered ones without ``node_type``)."""
    triplets = triplets[:, :3].to(torch.int64)
    w_relation, node_emb = w_relation.detach(), node_emb.detach()
    table = node_emb.contiguous()
    out, cons = [], []
    N = table.size(0)
    if node_type is not None:
        node_type = _checked_types(node_type, N, table.device)
        if type_masks is None:
            type_masks = relation_type_masks(triplets if known is None else known, node_type, w_relation.size(0))
        type_masks = type_masks.to(device=table.device, dtype=torch.int64)
        on_kernel = _on_kernel(table, table) and w_relation.dtype == torch.float32
        if on_kernel:
            order = torch.argsort(node_type, stable=True)
            inv = torch.empty_like(order)
            inv[order] = torch.arange(N, device=order.device)
            table_t, type_t = table[order].contiguous(), node_type[order].to(torch.uint8)
    for side in sides:
        if side not in ("object", "subject"):
            raise ValueError("sides holds 'object' / 'subject', got %r" % (side,))
        fixed, tgt = (triplets[:, 0], triplets[:, 2]) if side == "object" else (triplets[:, 2], triplets[:, 0])
        query = (node_emb[fixed] * w_relation[triplets[:, 1]]).contiguous()
        ptr = idx = None
        if known is not None:
            ptr, idx = known_filter(known, torch.stack([fixed, triplets[:, 1]], 1), w_relation.size(0), side)
        if node_type is None:
            g, e = rank_counts(query, table, tgt, ptr, idx)
            if return_considered:
                listed = 0 if ptr is None else (ptr[1:] - ptr[:-1]) - _rows_holding(ptr, idx, tgt)
                cons.append(N - 1 - listed + torch.zeros_like(tgt))
        else:
            allowed = type_masks[triplets[:, 1], 0 if side == "subject" else 1] | (torch.ones_like(tgt) << node_type[tgt])
            if on_kernel:
                q_s, tgt_s, allowed_s, ptr_s, idx_s, qorder = _typed_order(query, tgt, allowed, ptr, idx, inv, N)
                g_s, e_s, c_s = rank_counts_typed(q_s, table_t, tgt_s, type_t, allowed_s, ptr_s, idx_s)
                g, e, c = torch.empty_like(g_s), torch.empty_like(e_s), torch.empty_like(c_s)
                g[qorder], e[qorder], c[qorder] = g_s, e_s, c_s
            else:
                g, e, c = rank_counts_typed(query, table, tgt, node_type, allowed, ptr, idx)
            cons.append(c.to(torch.int64))
        out.append(ranks_of(g, e, ties))
    return (torch.stack(out, 1), torch.stack(cons, 1)) if return_considered else torch.stack(out, 1)


def _rows_holding(ptr, idx, value):
    """1 where row ``i`` of the CSR holds ``value[i]``, else 0 (int64 ``[Q]``)."""
    counts = ptr[1:] - ptr[:-1]
    rows = torch.repeat_interleave(torch.arange(value.size(0), device=idx.device), counts, output_size=idx.numel())
    hit = torch.zeros(value.size(0), dtype=torch.int64, device=idx.device)
    hit.index_add_(0, rows, (idx == value[rows]).to(torch.int64))
    return hit.clamp_(max=1)


@torch.no_grad()
def link_metrics(ranks, ks=(1, 3, 10), sides=("object", "subject"), considered=None):
    """``{"MRR", "MR", "Hits@k" ...}`` over every rank, and the same under ``"<side>/"`` per column.  One host sync.
    ``considered`` (the shape of ``ranks``: ``link_ranks(return_considered=True)``) adds ``"candidates"``, the mean number
    of candidates a query was ranked against, and ``"AMRI" = 1 - sum(rank - 1) / sum(considered / 2)``, the adjusted mean
    rank index: 0 is what a random order gives, 1 a perfect one, whatever the number of candidates -- the figure to compare
    across relations and type mixes (NaN when nothing was considered at all)."""
    ranks = ranks.view(ranks.size(0), -1).to(torch.float64)
    names = ["%s/" % s for s in sides[:ranks.size(1)]] if ranks.size(1) == len(sides) else ["side%d/" % i for i in range(ranks.size(1))]
    cols = [ranks.reshape(-1)] + [ranks[:, i] for i in range(ranks.size(1))]
    rows = torch.stack([torch.stack([(1.0 / c).mean(), c.mean()] + [(c <= k).to(torch.float64).mean() for k in ks]) for c in cols])
    if considered is not None:
        considered = considered.view(considered.size(0), -1).to(device=ranks.device, dtype=torch.float64)
        if considered.shape != ranks.shape:
            raise ValueError("considered has the shape of ranks, got %s and %s" % (tuple(considered.shape), tuple(ranks.shape)))
        ccols = [considered.reshape(-1)] + [considered[:, i] for i in range(considered.size(1))]
        extra = torch.stack([torch.stack([n.mean(), 1.0 - (c - 1.0).sum() / (0.5 * n.sum())]) for c, n in zip(cols, ccols)])
        rows = torch.cat([rows, extra], 1)
    rows = rows.tolist()
    out = {}
    for prefix, row in zip([""] + names, rows):
        out[prefix + "MRR"], out[prefix + "MR"] = row[0], row[1]
        for k, v in zip(ks, row[2:]):
            out[prefix + "Hits@%d" % k] = v
        if considered is not None:
            out[prefix + "candidates"], out[prefix + "AMRI"] = row[-2], row[-1]
    return out


@torch.no_grad()
def link_metrics_by_relation(ranks, relations, num_rels, ks=(1, 3, 10)):
    """MRR, MR, Hits@k and the number of queries of every relation: ``{"relation/<r>/MRR", ".../MR", ".../Hits@k",
    ".../count"}``.  ``ranks`` [T] or [T, S] (every column counts as a query of the row's relation), ``relations`` [T].
    Segment sums on the device, one host sync; a relation without a query reports count 0 and zeros."""
    ranks = ranks.view(ranks.size(0), -1).to(torch.float64)
    rel = relations.to(device=ranks.device, dtype=torch.int64).view(-1, 1).expand_as(ranks).reshape(-1)
    flat = ranks.reshape(-1)
    feats = torch.stack([torch.ones_like(flat), 1.0 / flat, flat] + [(flat <= k).to(torch.float64) for k in ks], 1)
    sums = torch.zeros(num_rels, feats.size(1), dtype=torch.float64, device=ranks.device).index_add_(0, rel, feats)
    sums[:, 1:] /= sums[:, :1].clamp(min=1.0)
    out = {}
    for r, row in enumerate(sums.tolist()):
        prefix = "relation/%d/" % r
        out[prefix + "count"], out[prefix + "MRR"], out[prefix + "MR"] = int(row[0]), row[1], row[2]
        for k, v in zip(ks, row[3:]):
            out[prefix + "Hits@%d" % k] = v
    return out
