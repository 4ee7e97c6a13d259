"""Local relational pooling on the gather / segment-sum kernels: ``LRPLayer`` / ``LRP`` and ``DMPLRPPoolLayer`` / ``DMPLRP``
(SubgraphCountingMatching/models/lrp.py:18-390, models/dmplrp.py:20-470).

What the reference does per layer with three ``torch.sparse.mm`` calls (lrp.py:66-73, dmplrp.py:188-194):

    rows = node_to_perm @ node_feat + edge_to_perm @ edge_feat      [P * L*L, in]   P permutations, L = lrp_seq_len
    out  = einsum('dab,bca->dc', rows.view(P, L*L, in), weight)     [P, hid]
    node = pooling @ out                                            [N, hid]

The two selection matrices have unit entries and at most one entry per row between them (slot (i, i) of a permutation
holds its i-th node, slot (i, j) the edge from its i-th to its j-th node if there is one, dataset.py:1759-1776), and
the pooling matrix averages a CONTIGUOUS range of permutations per node (dataset.py:1795-1811).  Here therefore:

    rows = take_rows([node_feat ; edge_feat ; 0], slot)            one row gather (backward: fixed-order segment sum)
    out  = rows.view(P, L*L*in) @ weight.permute(2, 0, 1).reshape(L*L*in, hid)     one dense product, K = 16 in
    node = scale[:, None] * seg_pool(out, ranges)                  the segment-sum kernel over contiguous ranges

At widths 64 / 128 the first two lines are one launch sequence of csrc/dmp_lrppool.hip (``perm_product``, ``USE_POOL_KERNEL``):
the rows are gathered inside the kernels, forward and backward, and no [P * L*L, in] matrix exists.

``PermIndex`` holds the slot vector / ranges / scales of a batch; it is built from the reference's three sparse
tensors (``from_sparse``: what ``LRPDataset.batchify`` hands over), from the ego-net permutations enumerated on the host
(``from_graphs``) or from the batched graph itself on the device (``from_batched``: csrc/dmp_lrp.hip, count -> scan -> fill).
``model(pattern, graph)`` builds both sides' indexes with ``from_batched``: the call form of the training loop.
"""
from itertools import permutations

import numpy as np
import torch as th
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _abi, _lib, ops
from .act import init_module, init_weight, map_activation_str_to_layer
from .basemodel import GraphAdjModelV2
from .constants import INDEGREE, REVFLAG
from .dmpnn import DMPLayer
from .graph import as_batched


class PermIndex:
    """Slots, pooling ranges and scales of the permutations of one batched graph (device tensors).

    slot  int64 [P * L*L]  row of ``[node rows ; edge rows ; one zero row]`` that fills the slot
    sizes int64 [N]        permutations of node v: the next ``sizes[v]`` of them
    scale float [N]        factor on node v's sum (1 / sizes[v] for the reference's mean pooling)"""

    def __init__(self, slot, sizes, scale, num_nodes, num_edges, seq_len):
        self.slot, self.sizes, self.scale = slot, sizes, scale
        self.num_nodes, self.num_edges, self.seq_len = int(num_nodes), int(num_edges), int(seq_len)
        self.num_perms = int(slot.numel()) // (seq_len * seq_len)
        self._pool = None
        self._csr = None
        self._key_csr = None
        self.status = None      # from_batched: int64 [1] on the device, the OR of the DMP_LRP_* bits
        self.live = None        # an index padded to a capacity: float [num_perms], 1 for the real permutations, 0 for the tail

    @classmethod
    def from_sparse(cls, pooling_matrix, node_to_perm, edge_to_perm, seq_len=4):
        """From the reference's ``(p_perm_pool, (p_n_perm_matrix, p_e_perm_matrix))`` sparse COO tensors."""
        n2p, e2p, pool = node_to_perm.coalesce(), edge_to_perm.coalesce(), pooling_matrix.coalesce()
        _lib.require_gpu(n2p.values(), e2p.values(), pool.values())
        rows, N, E = n2p.shape[0], n2p.shape[1], e2p.shape[1]
        dev = n2p.values().device
        slot = th.full((rows,), N + E, dtype=th.int64, device=dev)            # empty slots read the zero row
        slot[n2p.indices()[0]] = n2p.indices()[1]
        slot[e2p.indices()[0]] = N + e2p.indices()[1]
        prow = pool.indices()[0]
        marks = th.searchsorted(prow, th.arange(pool.shape[0] + 1, device=dev))   # rows are sorted after coalesce()
        sizes = marks[1:] - marks[:-1]
        first = marks[:-1].clamp(max=max(int(prow.numel()) - 1, 0))
        scale = th.where(sizes > 0, pool.values()[first] if prow.numel() else th.zeros_like(sizes, dtype=th.float32),
                         th.zeros((), dtype=th.float32, device=dev))
        return cls(slot, sizes, scale.float(), N, E, seq_len)

    @classmethod
    def from_graphs(cls, graphs, device, seq_len=4, pooling="mean"):
        """From single graphs given as ``(src, dst, num_nodes[, is_reversed])`` host arrays: the ego-net permutations of
        ``LRPDataset.graph_to_egonet_seq`` (dataset.py:1751-1793: for every node, the permutations of up to
        ``seq_len - 1`` of its out-neighbours over the non-reversed edges, in ``itertools.permutations`` order) laid out
        like ``build_batch_graph_to_perm_matrices`` / ``build_perm_pooling_matrix`` do for a batch."""
        L, slots, sizes = seq_len, [], []
        n_off = e_off = 0
        total_n = sum(int(g[2]) for g in graphs)
        total_e = sum(len(g[0]) for g in graphs)
        zero = total_n + total_e
        for g in graphs:
            src, dst, n = np.asarray(g[0]), np.asarray(g[1]), int(g[2])
            keep = np.ones(len(src), bool) if len(g) < 4 or g[3] is None else ~np.asarray(g[3], bool)
            eid = {}
            adj = [[] for _ in range(n)]
            for e in np.nonzero(keep)[0]:
                u, v = int(src[e]), int(dst[e])
                if (u, v) not in eid:          # scipy's csr_matrix merges duplicate (u, v) entries into one neighbour
                    adj[u].append(v)
                eid[(u, v)] = int(e)           # the dict keeps the LAST edge of a pair
            for v in range(n):
                nbrs = sorted(adj[v])          # csr indices come out sorted by column
                perms = [(v,) + p for p in permutations(nbrs, min(L - 1, len(nbrs)))]
                sizes.append(len(perms))
                for perm in perms:
                    block = np.full(L * L, zero, np.int64)
                    for i, a in enumerate(perm):
                        block[i * (L + 1)] = n_off + a
                        for j, b in enumerate(perm):
                            if (a, b) in eid:
                                block[i * L + j] = total_n + e_off + eid[(a, b)]
                    slots.append(block)
            n_off += n
            e_off += len(src)
        slot = th.from_numpy(np.concatenate(slots) if slots else np.zeros(0, np.int64)).to(device)
        sizes = th.tensor(sizes, dtype=th.int64, device=device)
        scale = th.where(sizes > 0, 1.0 / sizes.clamp(min=1).float(), th.zeros((), device=device)) if pooling == "mean" \
            else th.ones(sizes.numel(), device=device)
        return cls(slot, sizes, scale, total_n, total_e, seq_len)

    @staticmethod
    def counts_host(src, dst, num_nodes, is_reversed=None, seq_len=4):
        """``(permutations, largest number of distinct neighbours, has a non-reversed self-loop)`` of ONE graph from its degree
        sequence alone: a node with n distinct non-reversed out-neighbours has n! / (n - k)! permutations, k = min(L - 1, n)
        (host arrays; no enumeration)."""
        src, dst, n = np.asarray(src, np.int64), np.asarray(dst, np.int64), int(num_nodes)
        if is_reversed is not None:
            keep = ~np.asarray(is_reversed, bool)
            src, dst = src[keep], dst[keep]
        deg = np.bincount(np.unique(src * max(n, 1) + dst) // max(n, 1), minlength=n) if len(src) else np.zeros(n, np.int64)
        total = 0
        for d, many in zip(*np.unique(deg, return_counts=True)):
            f = 1
            for i in range(min(seq_len - 1, int(d))):
                f *= int(d) - i
            total += f * int(many)
        return total, int(deg.max(initial=0)), bool((src == dst).any())

    @classmethod
    def from_batched(cls, graph, seq_len=4, pooling="mean", total=None, capacity=None):
        """From the batched graph itself, on the device (``dmp_lrp_count`` -> ``dmp_exclusive_scan_i64`` -> ``dmp_lrp_fill``):
        the index ``from_graphs`` builds for the batch's single graphs, memoised on the graph object per ``seq_len``.
        ``total``: the number of permutations where the caller knows it (a dataset does: ``counts_host``), else ONE read from
        the device sizes the output.  ``capacity`` (in permutations): the index then holds exactly ``capacity`` permutations
        -- the tail reads the zero row, is pooled by no node and is masked out of ``perm_pool`` (``live``) -- the total is
        never read back, and surplus permutations are dropped with ``DMP_LRP_DROPPED`` in ``status``: the form a recorded
        step needs.  A graph object that carries ``lrp_max_degree`` (the dataset's validation: largest number of distinct
        neighbours, no self-loop) is not asked for its status word; any other costs one read of it.  A non-reversed
        self-loop is a ``ValueError``; a node above ``DMP_LRP_MAX_NEIGHBOURS``, a ``seq_len`` outside the kernels' range or
        a graph that is not on the GPU goes through ``from_graphs`` on the batch split into its graphs: the same result."""
        g = as_batched(graph)
        L = int(seq_len)
        if L < 1:
            raise ValueError("lrp_seq_len must be positive")
        ix = g.index() if g._src.is_cuda else None
        memo = g.__dict__.setdefault("_lrp_index", {})
        key = (L, pooling, None if capacity is None else int(capacity))
        hit = memo.get(key)
        if hit is not None and hit[0] is ix:
            _lib.pin_for_capture(hit[1].slot, hit[1].sizes, hit[1].scale, hit[1].live)
            return hit[1]
        N, E = g.number_of_nodes(), g.number_of_edges()
        known = getattr(g, "lrp_max_degree", None)
        admitted = (ix is not None and 1 <= L <= _abi.DMP_LRP_MAX_SEQ_LEN and N + E + 1 < (1 << 31)
                    and (known is None or known <= _abi.DMP_LRP_MAX_NEIGHBOURS))
        perm = cls._build_device(g, ix, L, pooling, total, capacity, known is None) if admitted else None
        if perm is None:
            perm = cls._build_host(g, L, pooling, capacity)
        if not (g._src.is_cuda and th.cuda.is_current_stream_capturing()):     # arrays made inside a recording live in its pool
            memo[key] = (ix, perm)
        return perm

    @classmethod
    def _build_device(cls, g, ix, L, pooling, total, capacity, read_status):
        """The kernels' index, or None when the status word names a node above the neighbour cap."""
        lib = _lib.load()
        N, E, dev = g.number_of_nodes(), g.number_of_edges(), g.device
        i64 = dict(dtype=th.int64, device=dev)
        sizes, scale = th.empty(N, **i64), th.empty(N, dtype=th.float32, device=dev)
        off = th.empty(N + 2, **i64)                       # [N + 1] offsets (off[N]: the total), then the status word
        status = off[N + 1:]
        ws = th.empty(int(lib.dmp_lrp_workspace_words(N, E)), dtype=th.int32, device=dev)
        scan_ws = th.empty(int(lib.dmp_scan_workspace_words(N)), **i64)
        st = _lib.stream_ptr()
        _lib.check(lib.dmp_lrp_count(_lib.ptr(ix.out_ptr), _lib.ptr(ix.out_ent), _lib.ptr(ix.dst32), N, E, L, int(pooling == "mean"),
                                     _lib.ptr(ws), _lib.ptr(sizes), _lib.ptr(scale), _lib.ptr(status), st), "dmp_lrp_count")
        _lib.check(lib.dmp_exclusive_scan_i64(_lib.ptr(sizes), N, _lib.ptr(off), _lib.ptr(scan_ws), st), "dmp_exclusive_scan_i64")
        if read_status or (total is None and capacity is None):
            real, bits = (int(x) for x in off[N:].tolist())             # the one read: total and status side by side
            if bits & _abi.DMP_LRP_SELF_LOOP:
                raise ValueError("PermIndex.from_batched: a non-reversed self-loop (slot (i, i) cannot hold a node and an edge)")
            if bits & _abi.DMP_LRP_OVER_CAP:
                return None
            if total is not None and int(total) != real:
                raise ValueError("PermIndex.from_batched: total=%d but the graph has %d permutations" % (int(total), real))
            total = real
        P = int(total) if capacity is None else int(capacity)
        slot = th.empty(P * L * L, **i64)
        _lib.check(lib.dmp_lrp_fill(_lib.ptr(ix.out_ptr), _lib.ptr(ws), _lib.ptr(off), N, E, L, P, _lib.ptr(slot), _lib.ptr(status), st),
                   "dmp_lrp_fill")
        perm = cls(slot, sizes, scale, N, E, L)
        perm.status = status
        if capacity is not None:
            perm.live = (th.arange(P, device=dev) < off[N:N + 1]).float()
        return perm

    @classmethod
    def _build_host(cls, g, L, pooling, capacity):
        """``from_graphs`` on the batch split back into its graphs (host speed), padded or cut to ``capacity``."""
        src, dst = g._src.cpu().numpy(), g._dst.cpu().numpy()
        rev = g.edata[REVFLAG].cpu().numpy().astype(bool) if REVFLAG in g.edata else None
        bnn, bne = g.batch_num_nodes().cpu().tolist(), g.batch_num_edges().cpu().tolist()
        graphs, n0, e0 = [], 0, 0
        for n, e in zip(bnn, bne):
            s, d = src[e0:e0 + e] - n0, dst[e0:e0 + e] - n0
            r = None if rev is None else rev[e0:e0 + e]
            if bool(((s == d) & (True if r is None else ~r)).any()):
                raise ValueError("PermIndex.from_batched: a non-reversed self-loop (slot (i, i) cannot hold a node and an edge)")
            graphs.append((s, d, n, r))
            n0, e0 = n0 + n, e0 + e
        perm = cls.from_graphs(graphs, g.device, L, pooling)
        perm.status = th.zeros(1, dtype=th.int64, device=g.device)
        if capacity is not None:
            P, real, L2 = int(capacity), perm.num_perms, L * L
            slot = th.full((P * L2,), perm.num_nodes + perm.num_edges, dtype=th.int64, device=g.device)
            slot[:min(P, real) * L2] = perm.slot[:min(P, real) * L2]
            if real > P:
                perm.status += _abi.DMP_LRP_DROPPED
            perm.slot, perm.num_perms = slot, P
            perm.live = (th.arange(P, device=g.device) < real).float()
        return perm

    def slot_csr(self):
        """``(slot32, rowptr, ent)``: the slots as int32 (the gather's index) and the CSR of the slots by table row over the
        node and edge rows only -- the zero row fills most slots of a batch and its gradient is nobody's: a slot that reads
        it is outside ``[0, N + E)`` for ``dmp_csr_build``, which leaves such entries out (one row of several 10^5 entries
        would otherwise be sorted and summed by a single thread)."""
        if self._csr is None:
            lib = _lib.load()
            M, R, dev = int(self.slot.numel()), self.num_nodes + self.num_edges, self.slot.device
            i32 = dict(dtype=th.int32, device=dev)
            rowptr, ent, status = th.empty(R + 1, **i32), th.empty(M, **i32), th.empty(1, **i32)
            ws = th.empty(int(lib.dmp_csr_workspace_words(R, M)), **i32)
            _lib.check(lib.dmp_csr_build(_lib.ptr(self.slot), None, M, R, _lib.ptr(rowptr), _lib.ptr(ent), None, None, _lib.ptr(status),
                                         _lib.ptr(ws), _lib.stream_ptr()), "dmp_csr_build(slots)")
            self._csr = (self.slot.to(th.int32), rowptr, ent)
        return self._csr

    def key_csr(self):
        """``(rowptr, entp)`` of the pool kernels' table gradient: the CSR of the slots by the key ``slot * L*L + s`` over
        ``(N + E) * L*L`` rows -- one row per (table row, slot position) -- with the permutation of every entry, ascending
        inside a row.  A slot that reads the zero row has a key past the last row and stays behind ``rowptr[-1]``.
        ``(None, None)`` for an index without permutations.  One stable sort of the keys: ``dmp_csr_build`` sorts every row
        with one thread, and a hub's slot 0 -- every permutation of the node, 1,716 entries at 13 neighbours -- made that
        2.1 ms per index at 9 x 10^5 slots."""
        if self._key_csr is None:
            L2 = self.seq_len * self.seq_len
            M, rows, dev = int(self.slot.numel()), (self.num_nodes + self.num_edges) * L2, self.slot.device
            if M == 0:
                self._key_csr = (None, None)
                return self._key_csr
            key = self.slot * L2
            key.view(self.num_perms, L2).add_(th.arange(L2, device=dev))
            key, order = th.sort(key, stable=True)                                     # equal keys: ascending entry = ascending p
            rowptr = th.searchsorted(key, th.arange(rows + 1, device=dev)).to(th.int32)
            self._key_csr = (rowptr, th.div(order, L2, rounding_mode="floor").to(th.int32))   # entry p * L*L + s -> p
        _lib.pin_for_capture(*self._key_csr)
        return self._key_csr

    def pool_index(self):
        if self._pool is None:
            self._pool = ops.PoolIndex(self.sizes, num_rows=self.num_perms)
        return self._pool


def as_perm_index(graph, pooling_matrix, node_to_perm, edge_to_perm, seq_len):
    """The layer's three matrix arguments -> a ``PermIndex`` (a PermIndex passed in their first position is taken as is;
    the conversion of sparse tensors is cached on the pooling matrix object: every layer of a rep-net gets the same three)."""
    if isinstance(pooling_matrix, PermIndex):
        return pooling_matrix
    cached = getattr(pooling_matrix, "_dmp_perm_index", None)
    if cached is None or cached[0] is not node_to_perm or cached[1] is not edge_to_perm:
        cached = (node_to_perm, edge_to_perm, PermIndex.from_sparse(pooling_matrix, node_to_perm, edge_to_perm, seq_len))
        try:
            pooling_matrix._dmp_perm_index = cached
        except Exception:
            pass
    return cached[2]


class _SlotRows(th.autograd.Function):
    """Rows of ``[node_feat ; edge_feat ; 0]`` at the slots of a ``PermIndex``: forward one row gather, backward the
    fixed-order segment sum over ``PermIndex.slot_csr`` straight into the two gradients."""

    @staticmethod
    def forward(ctx, node_feat, edge_feat, perm):
        _lib.require_gpu(node_feat, edge_feat, perm.slot)
        slot32, ctx.rowptr, ctx.ent = perm.slot_csr()
        ctx.N, ctx.E = perm.num_nodes, perm.num_edges
        table = th.cat([node_feat, edge_feat, node_feat.new_zeros((1, node_feat.size(1)))], dim=0)
        return ops.gather_rows_raw(table, slot32)

    @staticmethod
    @once_differentiable
    def backward(ctx, d):
        g = ops.seg_sum_raw(d.contiguous(), ctx.rowptr, ctx.ent, ctx.N + ctx.E, rows_shared=False)
        return g[:ctx.N], g[ctx.N:], None


# True: ``perm_pool`` takes the product before bias and activation on the pool kernels (csrc/dmp_lrppool.hip: no
# [P * L*L, in] matrix in either pass) wherever they admit the shape; False: gather, dense product, segment sum.
USE_POOL_KERNEL = True


class _PermProduct(th.autograd.Function):
    """``einsum(slots(node_feat, edge_feat), weight)`` [P, hid] on the pool kernels: the rows are gathered inside them,
    forward and backward; the backward's table gradient runs over ``PermIndex.key_csr``.  ``calls``: forward launches so
    far (what a test reads to see which route ran)."""

    calls = 0

    @staticmethod
    def forward(ctx, node_feat, edge_feat, weight, perm):
        lib = _lib.load()
        _lib.require_gpu(node_feat, edge_feat, weight, perm.slot)
        x, z, w = node_feat.contiguous(), edge_feat.contiguous(), weight.contiguous()
        P, L, fin, hid = perm.num_perms, perm.seq_len, w.size(0), w.size(1)
        out = th.empty((P, hid), dtype=th.float32, device=x.device)
        ws = th.empty(int(lib.dmp_lrp_pool_workspace_words(P, fin, hid, L)), dtype=th.int32, device=x.device)
        with _lib.timed("lrp_pool_fwd[in=%d,hid=%d,L=%d,P=%d]", (fin, hid, L, P),
                        4 * (P * hid + (x.size(0) + z.size(0)) * fin + w.numel()) + 8 * P * L * L):
            _lib.check(lib.dmp_lrp_pool_fwd(_lib.ptr(x), _lib.ptr(z), _lib.ptr(w), _lib.ptr(perm.slot), P, perm.num_nodes, perm.num_edges,
                                            fin, hid, L, _lib.ptr(out), _lib.ptr(ws), _lib.stream_ptr()), "dmp_lrp_pool_fwd")
        ctx.save_for_backward(x, z, w)
        ctx.perm = perm
        _PermProduct.calls += 1
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, d):
        lib = _lib.load()
        x, z, w = ctx.saved_tensors
        perm = ctx.perm
        P, L, fin, hid = perm.num_perms, perm.seq_len, w.size(0), w.size(1)
        d = d.contiguous()
        rowptr, entp = perm.key_csr()
        dx, dz, dw = th.empty_like(x), th.empty_like(z), th.empty_like(w)
        ws = th.empty(int(lib.dmp_lrp_pool_workspace_words(P, fin, hid, L)), dtype=th.int32, device=x.device)
        with _lib.timed("lrp_pool_bwd[in=%d,hid=%d,L=%d,P=%d]", (fin, hid, L, P),
                        4 * (2 * P * hid + 2 * (x.size(0) + z.size(0)) * fin + 2 * w.numel()) + 12 * P * L * L):
            _lib.check(lib.dmp_lrp_pool_bwd(_lib.ptr(x), _lib.ptr(z), _lib.ptr(w), _lib.ptr(perm.slot), _lib.ptr(rowptr), _lib.ptr(entp),
                                            _lib.ptr(d), P, perm.num_nodes, perm.num_edges, fin, hid, L, _lib.ptr(dx), _lib.ptr(dz),
                                            _lib.ptr(dw), _lib.ptr(ws), _lib.stream_ptr()), "dmp_lrp_pool_bwd")
        return dx, dz, dw, None


def _pool_kernel_ok(perm, node_feat, edge_feat, weight):
    """The shapes ``dmp_lrp_pool_fwd`` / ``_bwd`` admit: fp32 on the GPU, widths 64 / 128, index sizes inside int32."""
    L2 = perm.seq_len * perm.seq_len
    return (weight.dim() == 3 and weight.size(2) == L2 and node_feat.size(1) == edge_feat.size(1) == weight.size(0)
            and all(t.is_cuda and t.dtype == th.float32 for t in (node_feat, edge_feat, weight)) and perm.slot.is_cuda
            and (perm.num_perms + 64) * L2 < (1 << 31) and (perm.num_nodes + perm.num_edges + 32) * L2 + 1 < (1 << 31)
            and bool(_lib.load().dmp_lrp_pool_supported(weight.size(0), weight.size(1), perm.seq_len)))


def perm_product(perm, node_feat, edge_feat, weight):
    """``einsum(slots(node_feat, edge_feat), weight)`` [P, hid], the product over the L*L slots before bias and activation: on
    the pool kernels where they admit the shape (``USE_POOL_KERNEL``), else one row gather and one dense product."""
    L2 = perm.seq_len * perm.seq_len
    if USE_POOL_KERNEL and _pool_kernel_ok(perm, node_feat, edge_feat, weight):
        return _PermProduct.apply(node_feat, edge_feat, weight, perm)
    rows = _SlotRows.apply(node_feat, edge_feat, perm)                            # [P * L*L, in]
    w = weight.permute(2, 0, 1).reshape(L2 * weight.size(0), weight.size(1))      # [(slot, in), hid]
    return ops.matmul_xw(rows.view(perm.num_perms, L2 * weight.size(0)), w)


def perm_pool(perm, node_feat, edge_feat, weight, bias=None, act=None):
    """``pooling @ act(einsum(slots(node_feat, edge_feat), weight) + bias)`` (lrp.py:66-73 / dmplrp.py:188-194 with
    ``act`` None): the product over the L*L slots (``perm_product``), per-node segment sum, scale."""
    if node_feat.size(0) != perm.num_nodes or edge_feat.size(0) != perm.num_edges:
        raise ValueError("perm_pool: the permutation index was built for %d nodes / %d edges" % (perm.num_nodes, perm.num_edges))
    out = perm_product(perm, node_feat, edge_feat, weight)
    if bias is not None:
        out = out + bias
    if act is not None:
        out = act(out)
    if perm.live is not None:          # the tail of an index at a capacity: exact zeros forward and backward
        out = out * perm.live.view(-1, 1)
    return ops.seg_pool(out, perm.pool_index()) * perm.scale.view(-1, 1)


class LRPLayer(nn.Module):
    """models/lrp.py:18-104."""

    def __init__(self, input_dim=2, hidden_dim=128, lrp_seq_len=4, bias=True, act_func="relu", batch_norm=False, mlp=False,
                 dropout=0.0):
        super(LRPLayer, self).__init__()
        self.lrp_seq_len, self.input_dim, self.hidden_dim = lrp_seq_len, input_dim, hidden_dim
        self.weight = nn.Parameter(th.empty(input_dim, hidden_dim, lrp_seq_len * lrp_seq_len))
        self.degnet_0 = nn.Linear(1, 2 * hidden_dim)
        self.degnet_1 = nn.Linear(2 * hidden_dim, hidden_dim)
        if bias:
            self.bias = nn.Parameter(th.empty(hidden_dim))
        else:
            self.register_parameter("bias", None)
        self.act = map_activation_str_to_layer(act_func)
        self.bn = nn.BatchNorm1d(hidden_dim) if batch_norm else None
        self.mlp = nn.Linear(hidden_dim, hidden_dim) if mlp else None
        self.drop = nn.Dropout(dropout)
        init_weight(self.weight, activation=act_func, init="uniform")
        init_module(self.degnet_0, activation=act_func, init="uniform")
        init_module(self.degnet_1, activation=act_func, init="uniform")
        if bias:
            nn.init.zeros_(self.bias)
        if mlp:
            init_module(self.mlp, activation=act_func, init="uniform")

    @_lib.on_input_device
    def forward(self, graph, node_feat, edge_feat, pooling_matrix, node_to_perm_matrix=None, edge_to_perm_matrix=None):
        g = as_batched(graph)
        perm = as_perm_index(g, pooling_matrix, node_to_perm_matrix, edge_to_perm_matrix, self.lrp_seq_len)
        node_out = perm_pool(perm, node_feat, edge_feat, self.weight, self.bias, self.act)
        deg = g.ndata[INDEGREE] if INDEGREE in g.ndata else g.in_degrees()
        factor = self.degnet_1(self.act(self.degnet_0(deg.float().unsqueeze(1))))
        node_out = self.act(node_out * factor)
        if self.bn is not None:
            node_out = self.bn(node_out)
        if self.mlp is not None:
            node_out = self.act(self.mlp(node_out))
        return self.drop(node_out), edge_feat

    def get_output_dim(self):
        return self.hidden_dim


class DMPLRPPoolLayer(DMPLayer):
    """models/dmplrp.py:20-213: a DMPLayer whose node and edge outputs go through the permutation pooling."""

    def __init__(self, input_dim, hidden_dim, init_neigenv=4.0, init_eeigenv=4.0, lrp_seq_len=4, bias=True, num_mlp_layers=2,
                 batch_norm=True, act_func="relu", dropout=0.0):
        nn.Module.__init__(self)
        self.input_dim, self.hidden_dim, self.lrp_seq_len = input_dim, hidden_dim, lrp_seq_len
        names = ("in_weight", "out_weight", "src_weight", "dst_weight", "nloop_weight", "eloop_weight")
        for name in names:                                     # registration order of dmplrp.py:39-45
            setattr(self, name, nn.Parameter(th.empty(input_dim, hidden_dim)))
        self.lrp_weight = nn.Parameter(th.empty(input_dim, hidden_dim, lrp_seq_len * lrp_seq_len))
        for name in ("nbias", "ebias", "lrp_bias"):
            if bias:
                setattr(self, name, nn.Parameter(th.empty(hidden_dim)))
            else:
                self.register_parameter(name, None)
        self.nmlp = self._make_mlp(hidden_dim, num_mlp_layers, batch_norm, act_func)
        self.emlp = self._make_mlp(hidden_dim, num_mlp_layers, batch_norm, act_func)
        self.act = map_activation_str_to_layer(act_func)
        self.drop = nn.Dropout(dropout)
        self.write_edge_agg = False
        for name in names:                                     # initialisation order of dmplrp.py:73-90
            init_weight(getattr(self, name), activation=act_func, init="uniform")
        init_weight(self.lrp_weight, init="uniform")
        for module in list(self.nmlp.modules()) + list(self.emlp.modules()):
            init_module(module, activation=act_func, init="uniform")
        if bias:
            for name in ("nbias", "ebias", "lrp_bias"):
                nn.init.zeros_(getattr(self, name))
        with th.no_grad():
            for name in ("in_weight", "out_weight", "nloop_weight"):
                getattr(self, name).div_(init_neigenv)
            for name in ("src_weight", "dst_weight", "eloop_weight"):
                getattr(self, name).div_(init_eeigenv)

    def fused_ok(self, *a, **k):                               # the pooled node output replaces the layer's: modular path
        return False

    @_lib.on_input_device
    def forward(self, graph, node_feat, edge_feat, pooling_matrix, node_to_perm_matrix=None, edge_to_perm_matrix=None):
        g = as_batched(graph)
        perm = as_perm_index(g, pooling_matrix, node_to_perm_matrix, edge_to_perm_matrix, self.lrp_seq_len)
        node_out, edge_out = DMPLayer.forward.__wrapped__(self, g, node_feat, edge_feat)
        node_out = perm_pool(perm, node_out, edge_out, self.lrp_weight, self.lrp_bias, None)
        return node_out, edge_out, pooling_matrix, node_to_perm_matrix, edge_to_perm_matrix


class _PermRepMixin:
    """``create_rep_net`` / ``get_pattern_rep`` / ``get_graph_rep`` of LRP / DMPLRP (lrp.py:108-220, dmplrp.py:216-330):
    the layer loop with the three permutation inputs handed through; the residual sum is taken by DMPLRP only (the LRP
    loop appends ``v`` on both branches, lrp.py:162-167)."""

    rep_key, residual_sum = None, False

    def _make_layer(self, **kw):
        raise NotImplementedError

    def create_rep_net(self, type, **kw):
        if type == "pattern" and self.share_rep_net:
            return self.g_rep_net
        num_layers = kw.get("rep_num_graph_layers" if type == "graph" else "rep_num_pattern_layers", 1)
        layers = nn.ModuleList()
        for i in range(num_layers):
            layers.add_module("%s_%s_(%d)" % (type, self.rep_key, i), self._make_layer(**kw))
        return nn.ModuleDict({self.rep_key: layers})

    def _run(self, net, graph, v, e, perm, v_gate=None, e_gate=None, v_zero=None, e_zero=None):
        for layer in net[self.rep_key]:
            nv, ne = layer(graph, v, e, *perm)[:2]
            if v_zero is not None:
                nv = nv.masked_fill(v_zero, 0.0)
            if e_zero is not None:
                ne = ne.masked_fill(e_zero, 0.0)
            if v_gate is not None:
                nv = nv * v_gate
            if e_gate is not None:
                ne = ne * e_gate
            if self.residual_sum and self.rep_residual and nv.size() == v.size() and ne.size() == e.size():
                v, e = v + nv, e + ne
            else:
                v, e = nv, ne
        return v, e

    def get_pattern_rep(self, pattern, p_v_emb, p_e_emb, p_perm_pool, p_n_perm_matrix=None, p_e_perm_matrix=None, v_mask=None,
                        e_mask=None):
        v_zero = None if v_mask is None else ~v_mask
        e_zero = None if e_mask is None else ~e_mask
        v = p_v_emb if v_zero is None else p_v_emb.masked_fill(v_zero, 0.0)
        e = p_e_emb if e_zero is None else p_e_emb.masked_fill(e_zero, 0.0)
        return self._run(self.p_rep_net, pattern, v, e, (p_perm_pool, p_n_perm_matrix, p_e_perm_matrix), v_zero=v_zero, e_zero=e_zero)

    def get_graph_rep(self, graph, g_v_emb, g_e_emb, g_perm_pool, g_n_perm_matrix=None, g_e_perm_matrix=None, v_mask=None,
                      e_mask=None, v_gate=None, e_gate=None):
        if v_mask is not None:
            v_gate = v_mask.float() if v_gate is None else v_mask.float() * v_gate
        if e_mask is not None:
            e_gate = e_mask.float() if e_gate is None else e_mask.float() * e_gate
        v = g_v_emb if v_gate is None else g_v_emb * v_gate
        e = g_e_emb if e_gate is None else g_e_emb * e_gate
        return self._run(self.g_rep_net, graph, v, e, (g_perm_pool, g_n_perm_matrix, g_e_perm_matrix), v_gate=v_gate, e_gate=e_gate)


def _is_graph(obj):
    return hasattr(obj, "all_edges") and hasattr(obj, "number_of_nodes")


class _PermModel(_PermRepMixin, GraphAdjModelV2):
    """The 8-argument forward of lrp.py:222-390 / dmplrp.py:332-470 on the common skeleton: the permutation inputs ride
    along on the graph objects while ``GraphAdjModelV2.forward`` runs.  ``model(pattern, graph)`` -- the call form of the
    training loop -- builds (or reuses) both sides' indexes on the device (``PermIndex.from_batched``), with the host hints
    a dataset leaves on the graphs (``lrp_total`` / ``lrp_capacity``, valid for ``lrp_seq_len``)."""

    edge_head_skips_reversed = False      # lrp.py:240-243 / dmplrp.py:350-353: plain length masks

    def _seq_len(self):
        return next(iter(self.g_rep_net[self.rep_key])).lrp_seq_len

    def _own_index(self, graph):
        L = self._seq_len()
        hinted = getattr(graph, "lrp_seq_len", None) == L
        return PermIndex.from_batched(graph, L, total=getattr(graph, "lrp_total", None) if hinted else None,
                                      capacity=getattr(graph, "lrp_capacity", None) if hinted else None)

    def forward(self, pattern, p_perm_pool, p_n_perm_matrix=None, p_e_perm_matrix=None, graph=None, g_perm_pool=None,
                g_n_perm_matrix=None, g_e_perm_matrix=None):
        if graph is None and p_n_perm_matrix is None and _is_graph(p_perm_pool):      # model(pattern, graph)
            pattern, graph = as_batched(pattern), as_batched(p_perm_pool)
            p_perm_pool, g_perm_pool = self._own_index(pattern), self._own_index(graph)
        pattern, graph = as_batched(pattern), as_batched(graph)
        self._perm = {id(pattern): (p_perm_pool, p_n_perm_matrix, p_e_perm_matrix), id(graph): (g_perm_pool, g_n_perm_matrix, g_e_perm_matrix)}
        try:
            return GraphAdjModelV2.forward(self, pattern, graph)
        finally:
            self._perm = None

    def get_pattern_rep(self, pattern, p_v_emb, p_e_emb, *perm, **kw):
        perm = perm or self._perm[id(pattern)]
        return _PermRepMixin.get_pattern_rep(self, pattern, p_v_emb, p_e_emb, *perm, **kw)

    def get_graph_rep(self, graph, g_v_emb, g_e_emb, *perm, **kw):
        perm = perm or self._perm[id(graph)]
        return _PermRepMixin.get_graph_rep(self, graph, g_v_emb, g_e_emb, *perm, **kw)


class LRP(_PermModel):
    rep_key, residual_sum = "lrp", False

    def _make_layer(self, **kw):
        return LRPLayer(self.hid_dim, self.hid_dim, lrp_seq_len=kw.get("lrp_seq_len", 4), batch_norm=kw.get("rep_lrp_batch_norm", False),
                        act_func=kw.get("rep_act_func", "relu"), dropout=kw.get("rep_dropout", 0.0))


class DMPLRP(_PermModel):
    rep_key, residual_sum = "DMPLRP", True

    def _make_layer(self, **kw):
        return DMPLRPPoolLayer(self.hid_dim, self.hid_dim, init_neigenv=kw.get("init_neigenv", 4.0), init_eeigenv=kw.get("init_eeigenv", 4.0),
                               lrp_seq_len=kw.get("lrp_seq_len", 4), num_mlp_layers=kw.get("rep_dmpnn_num_mlp_layers", 2),
                               batch_norm=kw.get("rep_dmpnn_batch_norm", False), act_func=kw.get("rep_act_func", "relu"),
                               dropout=kw.get("rep_dropout", 0.0))
