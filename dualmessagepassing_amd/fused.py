"""One DMPLayer (+ the rep-net's gate and residual) as a single autograd node.

Same math as ``dmpnn.dual_message_passing`` + the two 2-layer ReLU MLPs + ``v*gate`` +
residual add (SubgraphCountingMatching/models/dmpnn.py:111-166,245-277), but forward and
backward are orchestrated by hand so that every elementwise step between the GEMMs is one
HIP streaming pass (``csrc/dmp_fused.hip``) and gradient accumulation happens inside the
kernels / GEMM epilogues instead of as separate ``add`` launches:

The first Linear of each MLP follows the message sum with no non-linearity in between
(dmpnn.py:131-136,147-152), so its weight is folded into the projections:
``(Z Wel + c Z Wsd + P_d[v] - P_s[u] + be) W0^T + b0 = Z (Wel W0^T) + c Z (Wsd W0^T) + P'_d[v] - P'_s[u] + b'``
-- one [E,H]x[H,H] product less per layer in forward, input-gradient and weight-gradient
(9 instead of 12 E-row GEMM units), and the pre-activation tensor never exists.

  forward   S=seg_sum2(Z) | XP=X[Wnl W0n^T | Wdst W0e^T | Wsrc W0e^T] | H1n=relu(XP0+S Bn+b'n) | On | Xn=X+gv*On
            G=Z[Wel W0e^T | (Wsrc-Wdst) W0e^T] | H1e=edge_combine_relu(G,XP12,b'e) | Oe | Zn=Z+ge*Oe
  backward  gate*dOut (+colsum) -> GEMMs -> relu_bwd fused with edge_combine's backward (+colsum),
            seg_sum2 over the incidence CSR, dZ = dZn + gather_select(dS), dZ += dG W'^T,
            then the small [H,H] chain back to the individual parameters
  saved     X, Z, S, H1n, H1e  (ONE new [E,H] tensor per layer)

Eligibility (``DMPLayer.fused_ok``): 2-layer MLPs, ReLU, no BatchNorm, bias, no active dropout,
square weights, H % 4 == 0, ``is_reversed`` present, gates without gradient.  Anything else
takes the modular path (same kernels, torch autograd in between).
"""
import ctypes as _ctypes
import os as _os
import threading

import torch
from torch.autograd.function import once_differentiable

from . import _abi, _lib, gatememo, ops, side
from ._lib import check, ptr, stream_ptr


def _partials(rows, H, dev):
    lib = _lib.load()
    return torch.empty((int(lib.dmp_colsum_partial_rows(rows, H)), H), dtype=torch.float32, device=dev)


MAX_REDUCE_SEGMENTS = _abi.DMP_REDUCE_MAX_SEGMENTS


class _Deferred(threading.local):
    """Per-thread stack of active ``deferred_reductions`` collectors (autograd runs backward on one worker thread
    per device: a job must never land in another thread's collector, whose flush is on another stream)."""

    def __init__(self):
        self.stack = []


_deferred = _Deferred()


class deferred_reductions:
    """Inside the block ``reduce_partials`` only records its job and returns the (not yet written) result
    tensor; the jobs run as ONE launch (``dmp_reduce_partials_multi``) when the block is left.  For results
    that are consumed later anyway -- a layer backward's parameter gradients: 9 reductions -> 1."""

    def __enter__(self):
        self.jobs = []
        _deferred.stack.append(self)
        return self

    def flush(self):
        import ctypes
        lib = _lib.load()
        jobs, self.jobs = self.jobs, []
        for i in range(0, len(jobs), MAX_REDUCE_SEGMENTS):
            chunk = jobs[i:i + MAX_REDUCE_SEGMENTS]
            n = len(chunk)
            P = (ctypes.c_void_p * n)(*[ptr(j[0]) for j in chunk])
            S = (ctypes.c_int64 * n)(*[j[1] for j in chunk])
            L = (ctypes.c_int64 * n)(*[j[2] for j in chunk])
            O = (ctypes.c_void_p * n)(*[ptr(j[3]) for j in chunk])
            check(lib.dmp_reduce_partials_multi(P, S, L, O, n, stream_ptr()), "dmp_reduce_partials_multi")

    def __exit__(self, exc_type, exc, tb):
        _deferred.stack.remove(self)
        if exc_type is None:
            self.flush()
        return False


def reduce_partials(partial, out=None, accumulate=False):
    """``out[l] (+)= sum_s partial[s, l]`` in a fixed order (HIP)."""
    lib = _lib.load()
    S = partial.size(0)
    L = partial.numel() // max(S, 1)
    if out is None:
        out = torch.empty(L, dtype=torch.float32, device=partial.device)
    if _deferred.stack and not accumulate and partial.is_contiguous():
        _deferred.stack[-1].jobs.append((partial, S, L, out))      # keeps ``partial`` alive until the launch
        return out
    check(lib.dmp_reduce_partials(ptr(partial), S, L, ptr(out), int(accumulate), stream_ptr()), "dmp_reduce_partials")
    return out


def gate_residual(prev, upd, gate):
    lib = _lib.load()
    R, H = upd.shape
    out = torch.empty_like(upd)
    with _lib.timed("gate_residual[H=%d,R=%d]", (H, R), 4 * H * R * (3 if prev is not None else 2) + (4 * R if gate is not None else 0)):
        check(lib.dmp_gate_residual(ptr(prev), H, ptr(upd), H, ptr(gate), R, H, ptr(out), H, stream_ptr()),
              "dmp_gate_residual")
    return out


def add_bias_relu_(a, b, bias, slope=0.0):
    """a <- act(a + b + bias) in one pass (``b`` may be a column slice of a wider matrix); act = ReLU, or LeakyReLU
    with negative slope ``slope``."""
    lib = _lib.load()
    R, H = a.shape
    with _lib.timed("add_bias_relu[H=%d,R=%d]", (H, R), 12 * H * R):
        check(lib.dmp_add_bias_relu(ptr(a), a.stride(0), ptr(b), b.stride(0), ptr(bias), R, H, slope, ptr(a), a.stride(0),
                                    stream_ptr()), "dmp_add_bias_relu")
    return a


def scale_rows_colsum(d_out, gate):
    """-> (gate (.) d_out  [aliases d_out when gate is None], column sums [H])."""
    lib = _lib.load()
    R, H = d_out.shape
    part = _partials(R, H, d_out.device)
    d_upd = torch.empty_like(d_out) if gate is not None else None
    with _lib.timed("scale_rows_colsum[H=%d,R=%d]", (H, R), 4 * H * R * (2 if gate is not None else 1)):
        check(lib.dmp_scale_rows_colsum(ptr(d_out), H, ptr(gate), R, H, ptr(d_upd), H, ptr(part), stream_ptr()),
              "dmp_scale_rows_colsum")
    return (d_upd if gate is not None else d_out), reduce_partials(part)


def relu_bwd_colsum_(d_h, act, out=None, slope=0.0):
    """d_h <- act > 0 ? d_h : slope * d_h (in place, or into ``out``: e.g. a column slice of a wider matrix);
    returns (result, column sums [H])."""
    lib = _lib.load()
    R, H = d_h.shape
    part = _partials(R, H, d_h.device)
    dst = d_h if out is None else out
    ldo = dst.stride(0) if R > 1 else H
    with _lib.timed("relu_bwd_colsum[H=%d,R=%d]", (H, R), 12 * H * R):
        check(lib.dmp_relu_bwd_colsum(ptr(d_h), H, ptr(act), H, R, H, slope, ptr(dst), ldo, ptr(part), stream_ptr()),
              "dmp_relu_bwd_colsum")
    return dst, reduce_partials(part)


def relu_bwd_gathered_colsum(table, rowmap, gate, act, slope=0.0):
    """``dPre[r] = act[r] > 0 ? u : slope * u`` with ``u = gate[r] * table[rowmap[r]]`` (a zero row where ``rowmap[r] < 0``), and
    the column sums of dPre: the activation backward of a layer whose upstream gradient is one [H] vector per graph."""
    lib = _lib.load()
    R, H = act.shape
    part = _partials(R, H, act.device)
    out = torch.empty((R, H), dtype=torch.float32, device=act.device)
    with _lib.timed("relu_bwd_gathered[H=%d,R=%d]", (H, R), 8 * H * R + 8 * R + 4 * H * table.size(0)):
        check(lib.dmp_relu_bwd_gathered_colsum(ptr(table), table.stride(0), ptr(rowmap), ptr(gate), ptr(act), act.stride(0), R, H,
                                               slope, ptr(out), H, ptr(part), stream_ptr()), "dmp_relu_bwd_gathered_colsum")
    return out, reduce_partials(part)


def pool_relu_bwd(table, rowmap, gate, act, pool, slope=0.0, skip_dead=False, chunk_sums=False):
    """``relu_bwd_gathered_colsum`` and ``pool_rows(act, pool, gate)`` in ONE pass over ``act`` (``dmp_pool_relu_bwd``):
    -> (dPre [R, H], column sums of dPre [H], Q [graphs, 2H] = gated per-graph sums of ``act`` by flag).
    ``skip_dead`` (every consumer of dPre leaves out the rows under a zero of the 0 / 1 ``gate``): the pass walks the kept
    rows' chunk table (``keep_pool_csr``) -- dPre's rows under a zero gate are not stored, nor are their entries walked.
    ``chunk_sums``: the third result is the pass's own [chunks, 2H] table instead of Q (``pool_wgrad`` sums it per graph itself)."""
    lib = _lib.load()
    R, H = act.shape
    V = pool.num_chunks
    nb = int(lib.dmp_pool_relu_bwd_blocks(V, H))
    part = torch.empty((nb, H), dtype=torch.float32, device=act.device)
    kc = keep_pool_csr(pool, gate) if skip_dead else None
    vptr, vent = (pool.vptr, pool.vent) if kc is None else kc
    out = dead_rows_buffer((R, H), act.device) if kc is not None else torch.empty((R, H), dtype=torch.float32, device=act.device)
    qc = torch.empty((V, 2 * H), dtype=torch.float32, device=act.device)
    with _lib.timed("pool_relu_bwd[H=%d,R=%d]", (H, R), 8 * H * R + 12 * R + 8 * H * V):
        check(lib.dmp_pool_relu_bwd(ptr(act), act.stride(0), ptr(table), table.stride(0), ptr(rowmap), ptr(gate), ptr(vptr),
                                    ptr(vent), V, R, H, slope, ptr(out), H, ptr(qc), ptr(part), stream_ptr()), "dmp_pool_relu_bwd")
    if chunk_sums:
        return out, reduce_partials(part), qc
    Q = ops.seg_sum_raw(qc, pool.gptr, pool.gent, pool.num_graphs, None, False, rows_shared=False)
    return out, reduce_partials(part), Q


def keep_pool_csr(pool, gate):
    """``(ptr, ent)``: the chunk table of ``pool`` over the rows a 0 / 1 ``gate`` keeps (``dmp_csr_keep`` on the pooling index's
    chunk CSR), memoised on the gate per index, or None.  A pooled pass with a 0 / 1 row weight is then the PLAIN segment sum
    over 42 % of the entries (full load slots) instead of the weighted one that walks every entry: 46 -> 28 us at bench.py's
    shape; same sums, same order (the skipped rows added zeros)."""
    own = None if gate is None else gatememo.owner(gate)
    if not has_row_mask(own, True, True) or pool.num_chunks == 0 or gate.numel() == 0:
        return None
    return gatememo.memo(own, ("keep_pool", id(pool)), (pool,), lambda: _csr_keep(pool.vptr, pool.vent, gate, pool.num_chunks), True)


def _csr_keep_buffers(rows, entries, device):
    """``(row counts (scratch), ptr [rows + 1], ent [entries])`` of ``dmp_csr_keep`` / ``dmp_incidence_keep``: one allocation."""
    nscr = int(_lib.load().dmp_csr_keep_scratch_words(rows))
    ws = torch.empty(nscr + rows + 1 + entries, dtype=torch.int32, device=device)
    return ws[:nscr], ws[nscr:nscr + rows + 1], ws[nscr + rows + 1:]


def _csr_keep(csr_ptr, csr_ent, gate, rows):
    """``(ptr, ent)``: the CSR ``(csr_ptr, csr_ent)`` of ``rows`` rows over the entries whose ``gate`` is not zero (``dmp_csr_keep``)."""
    row_cnt, kptr, kent = _csr_keep_buffers(rows, csr_ent.numel(), csr_ptr.device)
    check(_lib.load().dmp_csr_keep(ptr(csr_ptr), ptr(csr_ent), ptr(gate.reshape(-1)), rows, csr_ent.numel(), ptr(row_cnt), ptr(kptr),
                                   ptr(kent), stream_ptr()), "dmp_csr_keep")
    return kptr, kent


def pool_rows(x, pool, weight=None):
    """Per-graph sums of the rows of ``x`` over ``pool`` (``ops.PoolIndex``): [G, H], or [G, 2H] = [non-flagged | flagged] when
    the index carries a flag; ``weight`` [rows]: a row scale (a 0 / 1 gate: the pass runs over the kept rows' chunk table,
    ``keep_pool_csr``).  Raw (no autograd): two launches of the segment-sum kernel."""
    return ops.seg_sum_raw(pool_chunk_sums(x, pool, weight), pool.gptr, pool.gent, pool.num_graphs, None, False, rows_shared=False)


def pool_chunk_sums(x, pool, weight=None):
    """The first level of ``pool_rows``: the sums of the rows of ``x`` per chunk of ``pool`` -> [chunks, H] (with a flag [chunks, 2H])."""
    split = pool.flag8 is not None
    kc = keep_pool_csr(pool, weight) if (weight is not None and x.size(1) % 4 == 0 and x.is_contiguous()) else None
    if kc is not None:
        return ops.seg_sum_raw(x, kc[0], kc[1], pool.num_chunks, None, split, 1.0, 1.0, rows_shared=False)
    return ops.seg_sum_raw(x, pool.vptr, pool.vent, pool.num_chunks, weight, split, 1.0, 1.0, rows_shared=False)


USE_POOL_ALGEBRA = True     # the pooled last layer's per-graph algebra as three launches (``pool_out``, ``rows_gemm``, ``pool_wgrad``)
POOL_ALGEBRA_WIDTHS = (64, 128)


def _aligned(*tensors):
    """Contiguous fp32 tensors at 16-byte aligned addresses (None passes)."""
    return all(t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0) for t in tensors)


def pool_algebra_ok(index, H, epool, eW2, eb2):
    """The ONE host condition of the three-launch route, for both passes of a call of the layer's row-less form (kept on its
    ``_LayerCall``): the kernels' widths, fp32 parameters they can read as float4, an index over rows in their own order (the
    gated counts, ``pool_weight_sums``), and the conditions of the backward's lazy form (``_grad_seeds``), whose algebra this is."""
    return bool(USE_POOL_ALGEBRA and H in POOL_ALGEBRA_WIDTHS and getattr(epool, "rows_in_order", False) and epool.num_graphs > 0
                and index.num_edges > 0 and typed_ok(index, H) and eb2 is not None and _aligned(eW2, eb2))


def pool_out(partH, partZ, pool, gcnt, W2, b2, partX=None, vpool=None, want_q=False):
    """The second level of the pooled sums and the second Linear on them in ONE launch (``dmp_pool_out``):
    ``es [G, H] = sum_chunks partZ[:, :H] + (sum_chunks partH[:, :H]) W2^T + gcnt[:, 0] b2`` over the chunk sums of ``pool``
    (``pool_chunk_sums``: the non-flagged half only), ``vs [Gn, H] = sum_chunks partX`` over ``vpool``'s; chunks in ascending
    order: ``vs`` and the inner ``Q`` have ``pool_rows``' bits -> ``(es, vs or None[, Q])``."""
    lib = _lib.load()
    H, G, V = W2.size(0), pool.num_graphs, pool.num_chunks
    halves = partH.size(1) // H
    dev = partH.device
    es = torch.empty((G, H), dtype=torch.float32, device=dev)
    Q = torch.empty((G, H), dtype=torch.float32, device=dev) if want_q else None
    Gn, Vn = (vpool.num_graphs, vpool.num_chunks) if partX is not None else (0, 0)
    vs = torch.empty((Gn, H), dtype=torch.float32, device=dev) if partX is not None else None
    nbytes = 4 * H * (V * (2 if partZ is not None else 1) + H + G + Vn + Gn) + 4 * (V + Vn + 2 * G + Gn)
    with _lib.timed("pool_out[H=%d,G=%d]", (H, G), nbytes):
        check(lib.dmp_pool_out(ptr(partH), ptr(partZ), V, halves, ptr(pool.gptr), ptr(pool.gent), G, ptr(gcnt), ptr(W2), ptr(b2),
                               ptr(partX), Vn, ptr(vpool.gptr) if partX is not None else None,
                               ptr(vpool.gent) if partX is not None else None, Gn, H, ptr(es), ptr(vs), ptr(Q), stream_ptr()),
              "dmp_pool_out")
    return (es, vs, Q) if want_q else (es, vs)


def rows_gemm(a, W, w_out_in):
    """``a W^T`` (``w_out_in``: ``W`` in nn.Linear layout) or ``a W`` for [rows, H] x [H, H] on the heads' tiles (``dmp_rows_gemm``)."""
    lib = _lib.load()
    R, H = a.shape
    out = torch.empty((R, H), dtype=torch.float32, device=a.device)
    with _lib.timed("rows_gemm[H=%d,R=%d]", (H, R), 4 * H * (2 * R + H)):
        check(lib.dmp_rows_gemm(ptr(a), a.stride(0) if R > 1 else H, R, H, ptr(W), int(bool(w_out_in)), ptr(out), H, stream_ptr()),
              "dmp_rows_gemm")
    return out


def pool_wgrad(qc, pool, T, gcnt, want_q=False):
    """The second Linear's parameter gradients from the per-graph table ``T`` alone (``dmp_pool_wgrad``): with ``Q`` = the per-graph
    sums of the non-flagged half of the chunk sums ``qc`` (formed in LDS, chunks ascending), ``dW2 = T^T Q`` and ``db2 = gcnt[:, 0] T``
    as per-workgroup partials, finished by ``reduce_partials`` (deferred inside ``deferred_reductions``) -> ``(dW2, db2[, Q])``."""
    lib = _lib.load()
    G, H = T.shape
    V = pool.num_chunks
    nb = int(lib.dmp_pool_wgrad_blocks(G))
    if nb == 0:
        z = torch.zeros(H * H + H, dtype=torch.float32, device=T.device)
        return (z[:H * H].view(H, H), z[H * H:]) + ((torch.empty((0, H), dtype=torch.float32, device=T.device),) if want_q else ())
    part = torch.empty((nb, H * H + H), dtype=torch.float32, device=T.device)
    Q = torch.empty((G, H), dtype=torch.float32, device=T.device) if want_q else None
    with _lib.timed("pool_wgrad[H=%d,G=%d]", (H, G), 4 * H * (V + G) + 4 * (V + 2 * G) + 4 * nb * (H * H + H)):
        check(lib.dmp_pool_wgrad(ptr(qc), qc.size(1), V, gcnt.size(1), ptr(pool.gptr), ptr(pool.gent), G, ptr(T), T.stride(0) if G > 1 else H, ptr(gcnt),
                                 H, ptr(part), ptr(Q), stream_ptr()), "dmp_pool_wgrad")
    out = reduce_partials(part)
    return (out[:H * H].view(H, H), out[H * H:]) + ((Q,) if want_q else ())


def pool_weight_sums(pool, weight=None):
    """[G, 1] per-graph sums of a row weight over ``pool`` (``ops.PoolIndex``), [G, 2] = [non-flagged | flagged] when the
    index carries a flag; ``weight`` None: row counts (``dmp_pool_weight_sums``)."""
    lib = _lib.load()
    if not getattr(pool, "rows_in_order", False):
        raise _lib.DmpError("pool_weight_sums: an index over rows in their own order")

    def build():
        halves = 2 if pool.flag8 is not None else 1
        out = torch.empty((pool.num_graphs, halves), dtype=torch.float32, device=pool.offsets.device)
        w = None if weight is None else weight.reshape(-1).contiguous()
        check(lib.dmp_pool_weight_sums(ptr(w), ptr(pool.flag8), ptr(pool.offsets), pool.num_graphs, ptr(out), stream_ptr()),
              "dmp_pool_weight_sums")
        return out

    # (a gate's sums are memoised on the gate per index: dmpnn.prefetch_joint_indexes makes them ahead, on the side stream)
    if weight is None or weight.requires_grad:
        return build()
    return gatememo.memo(weight, "pool_weight_sums", (pool,), build)


def pool_rowmap(pool):
    """int32 [rows]: the graph of every row, -1 for flagged rows (they are masked out of the pooled sum)."""
    m = getattr(pool, "_rowmap", None)                  # written by the index build itself (dmp_pool_index_jobs) where it ran
    if m is None:
        m = pool.seg32 if pool.flag8 is None else torch.where(pool.flag8 != 0, torch.full_like(pool.seg32, -1), pool.seg32)
        pool._rowmap = m
    return m


def bwd_g_colsum(d_y, coef, dst32):
    lib = _lib.load()
    E, H = d_y.shape
    part = _partials(E, H, d_y.device)
    d_g = torch.empty((E, 2 * H), dtype=torch.float32, device=d_y.device)
    with _lib.timed("edge_combine_bwd_g[H=%d,E=%d]", (H, E), 12 * H * E + 4 * E + 4 * coef.numel()):
        check(lib.dmp_edge_combine_bwd_g_colsum(ptr(d_y), H, ptr(coef), ptr(dst32), E, H, ptr(d_g), 2 * H, ptr(part),
                                                stream_ptr()), "dmp_edge_combine_bwd_g_colsum")
    return d_g, reduce_partials(part)


def colsum(a):
    lib = _lib.load()
    R, H = a.shape
    part = _partials(R, H, a.device)
    check(lib.dmp_colsum_partials(ptr(a), H, R, H, ptr(part), stream_ptr()), "dmp_colsum_partials")
    return reduce_partials(part)


def atb(a, b):
    """``a.T @ b`` for tall-skinny operands: batched GEMM over 4096-row slices (MFMA through
    hipBLASLt) + the fixed-order HIP reduction of the slice products."""
    R = a.size(0)
    rows = ops._SPLITK_ROWS
    if R < 4 * rows:
        return a.t() @ b
    S = R // rows
    main = S * rows
    tail = 1 if main < R else 0
    part = torch.empty((S + tail, a.size(1), b.size(1)), dtype=a.dtype, device=a.device)
    torch.bmm(a[:main].view(S, rows, a.size(1)).transpose(1, 2), b[:main].view(S, rows, b.size(1)), out=part[:S])
    if tail:
        torch.mm(a[main:].t(), b[main:], out=part[S])        # the ragged last slice: one more partial
    return reduce_partials(part.view(S + tail, -1)).view(a.size(1), b.size(1))


def edge_combine_raw(G, ldg, P, ldp, bias, coef, index, H, relu=False, slope=0.0):
    lib = _lib.load()
    E = index.num_edges
    Y = torch.empty((E, H), dtype=torch.float32, device=G.device)
    with _lib.timed("edge_combine[H=%d,E=%d]", (H, E), 4 * H * (3 * E + 2 * index.num_nodes) + 9 * E + 4 * index.num_nodes):
        check(lib.dmp_edge_combine(ptr(G), ldg, ptr(P), ldp, ptr(coef), ptr(bias), ptr(index.src32), ptr(index.dst32),
                                   ptr(index.rev8), E, H, int(relu), slope, ptr(Y), H, stream_ptr()), "dmp_edge_combine")
    return Y


def relu_bwd_g_colsum(d_h, act, coef, dst32, slope=0.0):
    """-> (dG = [dPre | coef[dst] dPre] with dPre = act>0 ? d_h : slope d_h,  column sums of dPre)."""
    lib = _lib.load()
    E, H = d_h.shape
    part = _partials(E, H, d_h.device)
    d_g = torch.empty((E, 2 * H), dtype=torch.float32, device=d_h.device)
    with _lib.timed("relu_bwd_g_colsum[H=%d,E=%d]", (H, E), 16 * H * E + 4 * E + 4 * coef.numel()):
        check(lib.dmp_relu_bwd_g_colsum(ptr(d_h), H, ptr(act), H, ptr(coef), ptr(dst32), E, H, slope, ptr(d_g), 2 * H,
                                        ptr(part), stream_ptr()), "dmp_relu_bwd_g_colsum")
    return d_g, reduce_partials(part)


MFMA_WIDTHS = (128, 64)  # one-panel kernels (out_fwd, bwd_h1), class-typed kernels and the weight-gradient kernels


def mfma_ok(index, H):
    """The fused MFMA kernels take H = 128 and address the gathered tables / per-edge arrays with
    32-bit byte offsets: [N, 3H] fp32 projections and E-float arrays must stay below 4 GiB."""
    return H == 128 and index.num_nodes * 3 * H * 4 < 2 ** 32 and index.num_edges * 4 < 2 ** 32


def onepanel_ok(H):
    """out_fwd_mfma / bwd_h1_mfma (dPre alone) take this width (128, or the reference's shipped 64)."""
    return H in MFMA_WIDTHS


def edge_fwd_mfma(z, Wes, P, ldp, bias, coef, index, slope=0.0):
    """act(z Wes[:, :H] + coef[dst] z Wes[:, H:] + gathers(P) + bias): one fused MFMA kernel (H=128; the class-typed variant also H=64)."""
    lib = _lib.load()
    E, H = z.shape
    out = torch.empty((E, H), dtype=torch.float32, device=z.device)
    Wes = Wes.contiguous()
    sel_a, sel_b, coef_e = index.edge_select(coef)
    with _lib.timed("edge_fwd_mfma[H=%d,E=%d]", (H, E), 4 * H * (2 * E + 2 * index.num_nodes) + 12 * E):
        check(lib.dmp_edge_fwd_fused(ptr(z), H, ptr(Wes), Wes.size(1), ptr(P), ldp, index.num_nodes, ptr(bias),
                                     ptr(sel_a), ptr(sel_b), ptr(coef_e), E, H, slope, ptr(out), H, stream_ptr()),
              "dmp_edge_fwd_fused")
    return out


def typed_ok(index, H):
    """Class-typed kernels: rows are addressed by index (structured buffer descriptors), so the [E, H] arrays may be of
    any size (BASELINE config 4's 1024-pair shard: 8.4 M edge rows, 4.3 GB per array, one pass); what is 32-bit are the
    packed (row << 1 | flag) index entries and the per-edge int32 arrays."""
    return onepanel_ok(H) and index.num_nodes < 2 ** 31 and index.num_edges < 2 ** 30


def edge_fwd_typed(z, Wes, P, ldp, bias, coef, index, slope=0.0, dead_gate=None, sel=None):
    """edge_fwd_mfma with W_g = Wes[:, :H] + c_g Wes[:, H:] per degree class: one product instead of two.
    ``dead_gate``: an edge gate all of whose zeros mark DEAD output rows (every consumer multiplies them by that zero and
    skips them): those edges are padding slots of the tile list -- nothing is read, computed or stored for them.
    ``sel`` = ``NodeRows.sel``: the selectors with the nodes whose rows of ``P`` were never written replaced by -1 (read as zeros)."""
    lib = _lib.load()
    E, H = z.shape
    out = dead_rows_buffer((E, H), z.device)
    Wes = Wes.contiguous()
    sel_a, sel_b = (sel[0], sel[1]) if sel is not None else index.edge_select(coef)[:2]
    lt = live_tiles(index, coef, dead_gate) if dead_gate is not None else None
    if lt is not None:
        slot_edge, tile_scale, num_tiles, bound = lt
    else:
        slot_edge, tile_scale, num_tiles, bound = index.class_tiles(coef)
        ms = masked_slots(index, coef, dead_gate) if dead_gate is not None else None
        if ms is not None:
            slot_edge = ms
    with _lib.timed("edge_fwd_typed[H=%d,E=%d]", (H, E), 4 * H * (2 * E + 2 * index.num_nodes) + 12 * E):
        check(lib.dmp_edge_fwd_typed(ptr(z), H, ptr(Wes), Wes.size(1), ptr(P), ldp, index.num_nodes, ptr(bias),
                                     ptr(sel_a), ptr(sel_b), ptr(slot_edge), ptr(tile_scale), ptr(num_tiles), bound,
                                     E, H, slope, ptr(out), H, stream_ptr()), "dmp_edge_fwd_typed")
    return out


def masked_slots(index, coef, gate):
    """The class-tile slot list of ``index`` with the edges under a zero ``gate`` turned into padding (``dmp_mask_slots``), or
    None (no gate, masks off, a gate known to be dense).  For kernels whose streamed rows are ZERO for such edges -- ``dPre``
    of a gated layer: ``atb_typed`` skips the edge, ``bwd_z_typed`` skips the fetch of its ``dPre`` row.  Memoised on the gate
    (shared by the layers of a rep-net) per slot list."""
    own = None if gate is None else gatememo.owner(gate)
    if not has_row_mask(own, resolved=True):
        return None
    slot_edge = index.class_tiles(coef)[0]

    def build():
        out = torch.empty_like(slot_edge)
        check(_lib.load().dmp_mask_slots(ptr(slot_edge), slot_edge.numel(), ptr(gate), gate.numel(), ptr(out), stream_ptr()), "dmp_mask_slots")
        return out

    return gatememo.memo(own, "masked_slots", (slot_edge,), build, True)


USE_LIVE_TILES = True      # (module attributes, not environment switches: tests flip them; the documented DMP_* switches are listed in DESIGN.md 2)


def live_tiles(index, coef, gate):
    """The class-tile list of ``index`` over the edges a 0 / 1 ``gate`` keeps (``GraphIndex.class_tiles_gated``: an edge under
    a zero gate has no slot at all, so the kernels walk 46 % of the tiles of a ScalarFilter batch instead of all of them with
    padding slots inside), or None -- a gate not flagged 0 / 1, masks off, a coefficient of unknown origin.  For the launches
    that LEAVE OUT such edges (``masked_slots`` turns them into padding where every edge needs its slot).  Memoised on the gate."""
    own = None if gate is None else gatememo.owner(gate)
    if not live_tiles_ok(index, coef, own):
        return None
    return gatememo.memo(own, "live_tiles", (index, coef), lambda: index.class_tiles_gated(coef, gate.reshape(-1)), True)


def keep_in_csr(index, gate):
    """``(keep_ptr, keep_ent)``: ``index``'s CSR by destination over the edges a 0 / 1 ``gate`` keeps (``dmp_csr_keep``), memoised
    on the gate (the layers of a rep-net share it), or None."""
    own = None if gate is None else gatememo.owner(gate)
    if index.num_edges == 0 or not has_row_mask(own, True, True):
        return None
    return gatememo.memo(own, "keep_in_csr", (index,), lambda: _csr_keep(index.in_ptr, index.in_ent, gate, index.num_nodes), True)


_ZEROS = {}


def const_zeros(n, device):
    """A read-only float32 zero vector of ``n`` entries (a view of one cached buffer per device): the ``tile_scale`` of tile lists
    whose kernels use a plain panel -- nobody writes it, so no launch fills it step after step.  Inside a stream capture a
    buffer made NOW would belong to the recording's pool: a fresh tensor there, as before."""
    key = (device.type, device.index)
    buf = _ZEROS.get(key)
    if buf is None or buf.numel() < n:
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            return torch.zeros(n, dtype=torch.float32, device=device)
        buf = _ZEROS[key] = torch.zeros(max(n, 1 << 16), dtype=torch.float32, device=device)
    return buf[:n]


_IDENTITY_TILES = {}


def identity_tiles(R, device):
    """The tile slot list of ALL rows 0 .. R-1 in order (padding -1 up to a whole tile), for the tile kernels on launches without
    a gate: ``(slot, tile_scale (zeros), num_tiles, bound)``.  A constant of (R, device): built once outside any recording."""
    key = (int(R), device.type, device.index)
    hit = _IDENTITY_TILES.get(key)
    if hit is not None:
        return hit
    if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
        return None                      # (never made inside a recording: the first, eager step of a shape makes it)
    bound = (R + 31) // 32
    slot = torch.arange(bound * 32, dtype=torch.int32, device=device)
    slot[R:] = -1
    res = (slot, const_zeros(bound, device), torch.tensor([bound], dtype=torch.int32, device=device), bound)
    if len(_IDENTITY_TILES) < 64:
        _IDENTITY_TILES[key] = res
    return res


def ascending_tiles(gate):
    """The rows a 0 / 1 ``gate`` keeps as a tile slot list in ASCENDING row order (``dmp_kept_rows(tiles = 1)``; the class tiles list
    them class by class): for the launches over the kept edges' tiles whose panel does not depend on the degree class (the second
    Linear forward / backward, its weight gradient ``dO^T H1``) the 512-byte row gathers then walk memory front to back (measured
    on one box: atb_typed plain 81 -> 71 us, bwd_h1_typed 77 -> 72 us; -0.03 ms per step).  ``(slot, tile_scale (zeros), num_tiles,
    bound)`` or None; memoised on the gate."""
    mask = binary_gate_mask(gate)
    if mask is None:
        return None

    def build():
        R = gate.numel()
        lst, cnt = kept_rows(mask, 0, R, tiles=True)
        bound = (R + 31) // 32
        return lst, const_zeros(bound, mask.device), cnt[1:2], bound

    return gatememo.memo(gate, "ascending_tiles", (), build)


def bwd_z_typed(d_pre, ld_pre, Wes, d_s, base, coef, index, WesT=None, base_map=None, gate=None, dead_rows=None, dst=None):
    """bwd_z_mfma with the per-class matrix: base + gather_select(d_s) + dPre W_g^T  (dPre [E, H], leading dim ld_pre).
    ``WesT``: ``[A'^T | B'^T]`` if the caller has it already (``fold_layers`` makes it in its launch).
    ``base_map`` (int32 [E]): ``base`` is a small table and edge e adds its row ``base_map[e]`` (< 0: nothing).
    ``gate``: the layer's edge gate when ``d_pre`` is the gated layer's (its rows under a zero gate ARE zero): those rows are
    not fetched (``masked_slots``).  ``dead_rows`` (with ``gate``; ``zero_rows_gate`` holds): the input gradient of an edge
    under a zero gate is never used as a number (whoever made the rows multiplied them by the gate) -- ``"leave"``: those edges
    are padding slots, nothing is fetched, computed or stored for them (every reader of the result leaves them out);
    ``"zero"``: likewise, their output rows are zeros.
    ``dst`` (``NodeRows.sel[2]``): the destinations with the nodes whose rows of ``d_s`` were never written replaced by -1."""
    lib = _lib.load()
    E, H = d_pre.size(0), Wes.size(0)
    lt = live_tiles(index, coef, gate) if dead_rows is not None else None
    ms = lt[0] if lt is not None else masked_slots(index, coef, gate)
    if ms is None:
        dead_rows = None
    out = (torch.zeros((E, H), dtype=torch.float32, device=d_pre.device) if dead_rows == "zero" else
           dead_rows_buffer((E, H), d_pre.device) if dead_rows == "leave" else torch.empty((E, H), dtype=torch.float32, device=d_pre.device))
    # [A'^T | B'^T]: the kernel's per-class panel reads become coalesced (instead of a strided 128-instruction
    # panel read per class segment in each of its 768 workgroups)
    if WesT is None:
        WesT = torch.cat([Wes[:, :H].t(), Wes[:, H:].t()], dim=1)
    d_s = d_s.contiguous()
    if lt is not None:
        slot_edge, tile_scale, num_tiles, bound = lt
    else:
        slot_edge, tile_scale, num_tiles, bound = index.class_tiles(coef)
        if dead_rows is not None:
            slot_edge = ms
    with _lib.timed("bwd_z_typed[H=%d,E=%d]", (H, E), 4 * H * E * (3 if base is not None else 2) + 5 * E):
        check(lib.dmp_bwd_z_typed_arow(ptr(d_pre), ld_pre, ptr(WesT), WesT.size(1), ptr(d_s), d_s.size(1), index.num_nodes,
                                       ptr(base), base.stride(0) if base is not None else H, ptr(index.dst32 if dst is None else dst), ptr(index.rev8), -1.0, 1.0,
                                       ptr(slot_edge), ptr(ms), ptr(tile_scale), ptr(num_tiles), bound, E, H, 1,
                                       ptr(base_map), base.size(0) if base_map is not None else 0, ptr(out), H, stream_ptr()),
              "dmp_bwd_z_typed")
    return out


def bwd_z_w(d_pre, z, Wes, d_s, base, coef, index, WesT=None, base_map=None, gate=None, dead_rows=None, dst=None):
    """``(dz, dWes)`` = ``(bwd_z_typed(...), atb_typed(z, d_pre, ...))`` from one pass over ``d_pre`` (``dmp_bwd_z_w``: the two-role kernel
    of csrc/dmp_h1w.hip with the class-typed panel and the class emission), or None where it does not apply: it needs the kept edges'
    class tiles of a 0 / 1 gate with ``dead_rows`` set (both launches then walk the SAME list), H = 128, bf16x6, arrays below 4 GiB."""
    lib = _lib.load()
    E, H = d_pre.size(0), Wes.size(0)
    lim = (1 << 32) - 65536
    if ((dead_rows is None) != (gate is None) or H != 128 or lib.dmp_dev_get_exact_fp32() or z is None or z.size(0) != E or E * H * 4 >= lim
            or E * d_pre.stride(0) * 4 >= lim or E * z.stride(0) * 4 >= lim or d_pre.data_ptr() % 16 or z.data_ptr() % 16
            or d_pre.stride(0) % 4 or z.stride(0) % 4 or index.num_nodes * d_s.size(1) * 4 >= lim):
        return None
    if gate is None:          # no gate at all (the all-rows step): the class tiles over every edge, every output row written
        if getattr(index, "_coef_deg", None) is None or index._coef_deg[0] is not coef or index.num_edges == 0:
            return None
        lt = index.class_tiles(coef)
    else:
        lt = live_tiles(index, coef, gate)
    if lt is None:
        return None
    if base is not None and (base.stride(0) % 4 or base.data_ptr() % 16 or base.size(0) * base.stride(0) * 4 >= lim):
        return None
    slot_edge, tile_scale, num_tiles, bound = lt
    out = (torch.zeros((E, H), dtype=torch.float32, device=d_pre.device) if dead_rows == "zero" else
           dead_rows_buffer((E, H), d_pre.device) if dead_rows == "leave" else torch.empty((E, H), dtype=torch.float32, device=d_pre.device))
    if WesT is None:
        WesT = torch.cat([Wes[:, :H].t(), Wes[:, H:].t()], dim=1)
    d_s = d_s.contiguous()
    G = int(lib.dmp_bwd_h1_w_blocks(bound))
    part = torch.empty((G, H * 2 * H), dtype=torch.float32, device=d_pre.device)
    with _lib.timed("bwd_z_w[H=%d,E=%d]", (H, E), 4 * H * E * (4 if base is not None else 3) + 5 * E):
        check(lib.dmp_bwd_z_w(ptr(d_pre), d_pre.stride(0), ptr(z), z.stride(0), ptr(WesT), WesT.size(1), ptr(d_s), d_s.size(1), index.num_nodes,
                              ptr(base), base.stride(0) if base is not None else H, ptr(index.dst32 if dst is None else dst), ptr(index.rev8), -1.0, 1.0,
                              ptr(slot_edge), ptr(tile_scale), ptr(num_tiles), bound, E, H, ptr(base_map),
                              base.size(0) if base_map is not None else 0, ptr(out), H, ptr(part), stream_ptr()), "dmp_bwd_z_w")
    return out, reduce_partials(part).view(H, 2 * H)


USE_ATB2 = True     # the tile-list weight gradients on the bf16-piece LDS image (``dmp_atb2_jobs``)


def atb2_ok(a, b, H):
    lib = _lib.load()
    lim = (1 << 32) - 65536
    return bool(USE_ATB2 and H == 128 and not lib.dmp_dev_get_exact_fp32() and a.size(0) == b.size(0) and a.size(0) * a.stride(0) * 4 < lim
                and b.size(0) * b.stride(0) * 4 < lim and a.stride(0) % 4 == 0 and b.stride(0) % 4 == 0
                and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0)


def atb2(pairs, tiles, wide=False):
    """``[a^T b for (a, b) in pairs]`` over the rows of ``tiles`` (a, b: [R, 128] operands, column slices allowed): the products of
    ONE launch (``dmp_atb2_jobs``: at most 6).  ``wide``: each result is ``[a^T b | a^T (c (.) b)]`` ([128, 256]; c = the class
    coefficient of a row's tile: ``atb_typed``'s layout of dWes)."""
    lib = _lib.load()
    slot, tile_scale, num_tiles, bound = tiles
    n, H = len(pairs), 128
    R = pairs[0][0].size(0)
    G = int(lib.dmp_atb2_blocks(bound, n))
    W = 2 * H if wide else H
    jobs = (_abi.dmp_atb2_job * n)()
    parts = []
    for j, (a, b) in enumerate(pairs):
        part = torch.empty((G, H * W), dtype=torch.float32, device=a.device)
        parts.append(part)
        jobs[j].Z, jobs[j].ldz, jobs[j].D, jobs[j].ldd = a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0)
        jobs[j].partial_T, jobs[j].partial_B = part.data_ptr(), (part.data_ptr() + 4 * H if wide else None)
        jobs[j].partial_stride, jobs[j].ldp = H * W, W
    with _lib.timed("atb2[jobs=%d,R=%d]", (n, R), 8 * H * R * n):
        check(lib.dmp_atb2_jobs(jobs, n, ptr(slot), ptr(tile_scale), ptr(num_tiles), bound, R, H, stream_ptr()), "dmp_atb2_jobs")
    return [reduce_partials(part).view(H, W) for part in parts]


def atb_typed(z, d_pre, coef, index, gate=None, plain=False):
    """``[z^T d_pre | z^T (coef[dst] (.) d_pre)]``  ([H, 2H]: the gradient of ``Wes`` in its layout) over the
    class-sorted tiles: one product's worth of MFMAs for both halves (csrc/dmp_atb.hip), one fixed-order
    reduction of the workgroup partials.  ``gate``: the layer's edge gate when ``d_pre`` is the gated layer's (zero rows under
    a zero gate): those edges are skipped, neither of their rows is fetched (``masked_slots``)."""
    lib = _lib.load()
    E, H = z.shape
    lt = live_tiles(index, coef, gate)
    if plain and lt is not None:
        at = ascending_tiles(gate)
        if at is not None:
            lt = at
    if lt is not None:
        slot_edge, tile_scale, num_tiles, bound = lt
    else:
        slot_edge, tile_scale, num_tiles, bound = index.class_tiles(coef)
        ms = masked_slots(index, coef, gate)
        if ms is not None:
            slot_edge = ms
    if atb2_ok(z, d_pre, H):
        # every fetched element split into bf16 pieces once, fragments through transposed LDS reads (csrc/dmp_h1w.hip::atb2_k)
        return atb2([(z, d_pre)], (slot_edge, tile_scale, num_tiles, bound), wide=not plain)[0]
    G = int(lib.dmp_atb_typed_blocks_h(bound, H))
    if plain:       # ``z^T d_pre`` alone ([H, H]): half the partials
        part = torch.empty((G, H, H), dtype=torch.float32, device=z.device)
        with _lib.timed("atb_typed[H=%d,E=%d]", (H, E), 8 * H * E):
            check(lib.dmp_atb_typed(ptr(z), z.stride(0), ptr(d_pre), d_pre.stride(0), ptr(slot_edge), ptr(tile_scale),
                                    ptr(num_tiles), bound, E, H, ptr(part), None, stream_ptr()), "dmp_atb_typed")
        return reduce_partials(part.view(G, -1)).view(H, H)
    part = torch.empty((G, H, 2 * H), dtype=torch.float32, device=z.device)
    with _lib.timed("atb_typed[H=%d,E=%d]", (H, E), 8 * H * E):
        check(lib.dmp_atb_typed(ptr(z), z.stride(0), ptr(d_pre), d_pre.stride(0), ptr(slot_edge), ptr(tile_scale),
                                ptr(num_tiles), bound, E, H, ptr(part), ptr(part[0, 0, H:]), stream_ptr()), "dmp_atb_typed")
    return reduce_partials(part.view(G, -1)).view(H, 2 * H)


USE_ROW_MASKS = _os.environ.get("DMP_ROW_MASKS", "1") == "1"   # gated E-row kernels do not fetch the rows a zero gate annihilates
# ... and the two kernels that PRODUCE the first MLP's activation H1 leave out the rows all of whose consumers skip them
# (dead values: out_fwd, bwd_h1, atb_rows, the pooled passes multiply them by the zero gate).  Only with USE_ROW_MASKS.
SKIP_DEAD_ROWS = True
POISON_DEAD_ROWS = _os.environ.get("DMP_POISON_DEAD_ROWS", "0") == "1"   # testing aid: buffers with dead rows start as NaN


def dead_rows_buffer(shape, device):
    """An [E, H] buffer whose dead rows nobody writes: uninitialised -- or NaN throughout under ``POISON_DEAD_ROWS``, so that a
    consumer that does fetch a dead row shows up as NaN in its results."""
    if POISON_DEAD_ROWS:
        return torch.full(shape, float("nan"), dtype=torch.float32, device=device)
    return torch.empty(shape, dtype=torch.float32, device=device)


def gate_row_mask(gate):
    """uint32 [(R + 31) // 32]: bit r of word t = (gate[32 t + r] != 0) (``dmp_row_mask_bits``), for the ``_masked`` kernels;
    memoised on the gate tensor (a layer's forward and backward, and every layer of a rep-net, share the gate)."""
    own = None if gate is None else gatememo.owner(gate)
    if not has_row_mask(own, resolved=True):
        return None

    def build():
        # (a miss on the caller's stream while index builds are in flight on the side stream: the gate itself may have been
        # written THERE (dmpnn.prefetch_joint_indexes makes the union's gates inside its fork) -- order this stream behind that
        # stage before reading it.  The prefetch normally builds this mask too and the memo returns it: no wait.)
        from . import side
        side.wait("erows")
        R = gate.numel()
        mask = torch.empty(((R + 31) // 32,), dtype=torch.int32, device=gate.device)
        check(_lib.load().dmp_row_mask_bits(ptr(gate), R, ptr(mask), stream_ptr()), "dmp_row_mask_bits")
        return mask

    return gatememo.memo(own, "row_mask", (), build, True)


def code_row_mask(enc, K):
    """uint32 [(R + 31) // 32]: bit r of word t = (row 32 t + r of ``enc`` has a non-zero among its first K entries)
    (``dmp_row_mask_rows``): the packed label codes' live rows -- a gated-out row is all zeros, and so is every product with it."""
    if not USE_ROW_MASKS or enc is None:
        return None
    lib = _lib.load()
    R = enc.size(0)
    mask = torch.empty(((R + 31) // 32,), dtype=torch.int32, device=enc.device)
    check(lib.dmp_row_mask_rows(ptr(enc), enc.stride(0), int(K), R, ptr(mask), stream_ptr()), "dmp_row_mask_rows")
    return mask


def out_fwd_mfma(h1, W2, b2, gate, prev, W2t=None, dead_rows=0):
    """prev + gate * (h1 W2^T + b2): Linear + gate + residual in one fused MFMA kernel (H = 128 or 64).
    ``W2t``: ``W2.t()`` contiguous if the caller has it already (``fold_layers`` makes it in its launch).
    With a gate the rows of ``h1`` under a zero gate are not fetched (``gate_row_mask``): their term is multiplied by 0.
    ``dead_rows`` (``zero_rows_gate`` holds for the gate): 1 = the rows of ``prev`` under a zero gate are zeros and not fetched;
    3 = the output rows under a zero gate (zeros) are not stored either -- every reader leaves them out."""
    lib = _lib.load()
    R, H = h1.shape
    mask = gate_row_mask(gate)
    if mask is None:
        dead_rows = 0
    out = dead_rows_buffer((R, H), h1.device) if dead_rows & 2 else torch.empty((R, H), dtype=torch.float32, device=h1.device)
    if W2t is None:
        W2t = W2.t().contiguous() # [in, out]: coalesced weight-panel reads in each of the kernel's workgroups
    with _lib.timed("out_fwd_mfma[H=%d,R=%d]", (H, R), 4 * H * R * (3 if prev is not None else 2)):
        check(lib.dmp_out_fwd_fused_rows(ptr(h1), H, ptr(W2t), W2t.size(1), ptr(b2), ptr(gate), ptr(mask), int(dead_rows), ptr(prev), H,
                                         R, H, 1, ptr(out), H, stream_ptr()), "dmp_out_fwd_fused")
    return out


def typed_jobs(jobs, tiles):
    """Up to six products ``out = prev + prev2 + (a W + bias)`` (optionally through LeakyReLU) for the rows of ONE tile list in
    ONE launch (``dmp_out_fwd_typed``: grid.y = the job).  ``jobs``: dicts with ``a`` [R, H] (any row stride), ``W`` (``[in, out]``,
    or with ``w_in_out=False`` a Linear's ``[out, in]``; any row stride: a block of a wider matrix), ``out`` [R, H] view, and
    optionally ``bias``, ``prev``, ``prev2``, ``slope``.  Rows outside the tiles are not written."""
    lib = _lib.load()
    slot_edge, tile_scale, num_tiles, bound = tiles
    R, H = jobs[0]["a"].shape
    J = (_abi.dmp_typed_job * len(jobs))()
    for j, q in zip(J, jobs):
        a, W, out = q["a"], q["W"], q["out"]
        prev, prev2, slope = q.get("prev"), q.get("prev2"), q.get("slope")
        _lib.require_gpu(a, W, out, prev, prev2, q.get("bias"))
        j.Hin, j.ldh, j.W2, j.ldw, j.w_in_out = a.data_ptr(), a.stride(0), W.data_ptr(), W.stride(0), int(bool(q.get("w_in_out", True)))
        j.bias = ptr(q.get("bias"))
        j.R, j.ldr = ptr(prev), (prev.stride(0) if prev is not None else H)
        j.R2, j.ldr2 = ptr(prev2), (prev2.stride(0) if prev2 is not None else H)
        j.act, j.slope = int(slope is not None), float(slope or 0.0)
        j.out, j.ldo = out.data_ptr(), out.stride(0)
    with _lib.timed("out_fwd_typed[H=%d,R=%d,jobs=%d]", (H, R, len(jobs)), 4 * H * R * 3 * len(jobs)):
        check(lib.dmp_out_fwd_typed(J, len(jobs), ptr(slot_edge), ptr(tile_scale), ptr(num_tiles), bound, R, H, stream_ptr()),
              "dmp_out_fwd_typed")


def l0_rows(l0, W0, z):
    """The first layer's edge rows ``z``: as given, or -- when ``dmpnn.joint_rep`` left them out (``l0.z_from_codes``) and the layer
    did not take the launch that forms them in registers -- made here: the pattern's embedded rows (``l0.z_head``) over the target's
    from their label codes."""
    if l0 is None or not l0.z_from_codes:
        return z
    n, K, H = l0.z_head.size(0), l0.K, W0.size(1)
    out = torch.empty((l0.enc.size(0), H), dtype=torch.float32, device=l0.enc.device)
    out[:n].copy_(l0.z_head)
    if out.size(0) > n:
        smallk_embed(l0.enc[n:, :K], W0.detach()[-K:], None, out[n:], H)
    return out


USE_OUT_CODES = True   # the first layer's residual rows z0 = codes W_e as a K-extension of its second Linear


def out_codes_ok(h1, enc, K, Wc):
    """``out_fwd_typed_codes`` applies: H = 128, bf16x6, at most 16 code columns in rows of whole 16-byte pieces, arrays below 4 GiB."""
    lib = _lib.load()
    lim = (1 << 32) - 65536
    return bool(USE_OUT_CODES and h1.size(1) == 128 and not lib.dmp_dev_get_exact_fp32() and 1 <= K <= 16 and Wc.size(0) == K and Wc.size(1) == 128
                and enc.dtype == torch.float32 and enc.stride(1) == 1 and enc.stride(0) % 4 == 0 and enc.data_ptr() % 16 == 0
                and enc.size(0) == h1.size(0) and h1.size(0) * 128 * 4 < lim and Wc.stride(1) == 1)


def out_fwd_typed_codes(h1, W2t, b2, enc, K, Wc, tiles, prev=None, out=None, w_in_out=True, row0=0, first=None):
    """``prev + (h1 W2^T + enc[:, :K] Wc + b2)`` for the rows of ``tiles`` (``dmp_out_fwd_typed_codes``): the second Linear of a FIRST
    layer whose residual rows are the label embedding ``enc Wc`` -- added as one more 16-deep k-group of the product, so the [E, H] rows
    ``z0`` are neither written (``dmp_smallk_embed_live``) nor read.  ``row0``: the rows below it take no codes term (the pattern's
    edges, embedded by another table); ``prev`` may then hold just those rows ([row0 or more, H]: missing rows count as zeros).
    ``first``: ``h1`` does not exist yet -- the keyword arguments of the layer's first Linear on the same codes (``M, tables, split, P,
    ldp, bias, coef, index, slope`` of ``l0_edge_fwd``, ``M`` holding every table's rows, the rows below ``split`` being the first
    table's) whose output it is: both Linears then run as ONE launch over ``tiles`` (``dmp_l0_edge_mlp_fwd``, through ``l0_edge_fwd``),
    which fills ``h1`` on the way."""
    lib = _lib.load()
    slot_edge, tile_scale, num_tiles, bound = tiles
    R, H = h1.shape
    if out is None:
        out = dead_rows_buffer((R, H), h1.device)
    Wc = Wc.detach()
    if first is not None:
        l0_edge_fwd(enc, K, first["M"], first["P"], first["ldp"], first["bias"], first["coef"], first["index"], first["slope"], out=h1,
                    mlp=dict(tables=first["tables"], split=first["split"], W2t=W2t, b2=b2, Wc=Wc, row0=row0, prev=prev, tiles=tiles,
                             w_in_out=w_in_out, out=out))
        return out
    _lib.require_gpu(h1, W2t, out, prev, b2, enc, Wc)
    j = _abi.dmp_typed_job()
    j.Hin, j.ldh, j.W2, j.ldw, j.w_in_out = h1.data_ptr(), h1.stride(0), W2t.data_ptr(), W2t.stride(0), int(bool(w_in_out))
    j.bias = ptr(b2)
    j.R, j.ldr = ptr(prev), (prev.stride(0) if prev is not None else H)
    j.R2, j.ldr2 = None, H
    j.act, j.slope = 0, 0.0
    j.out, j.ldo = out.data_ptr(), out.stride(0)
    with _lib.timed("out_fwd_typed_codes[H=%d,R=%d]", (H, R), 4 * H * R * 2 + 4 * enc.size(1) * R):
        check(lib.dmp_out_fwd_typed_codes(_ctypes.byref(j), ptr(enc), enc.stride(0), int(K), ptr(Wc), Wc.stride(0), int(row0),
                                          0 if prev is None else min(R, prev.size(0)), ptr(slot_edge), ptr(tile_scale),
                                          ptr(num_tiles), bound, R, H, stream_ptr()), "dmp_out_fwd_typed_codes")
    return out


def out_fwd_typed(h1, W2t, b2, prev, tiles, out=None, w_in_out=True, slope=None, prev2=None, first=None):
    """``prev + (h1 W2^T + b2)`` for the rows of ``tiles`` (``live_tiles``: the edges a 0 / 1 gate keeps, gate 1 there; or
    ``NodeRows.tiles``: the kept nodes); the other rows of the result are not written (``dead_rows_buffer``).  ``W2t`` [in, out]
    (any row stride: a column block of a wider matrix), or with ``w_in_out=False`` the Linear's own [out, in].  ``out``: the
    destination (may be ``prev``: a product accumulates onto its own output); ``prev2``: a second addend; ``slope``:
    LeakyReLU(slope) on the result.
    ``first``: ``h1`` does not exist yet -- the keyword arguments of the edge MLP's first Linear (``z, Wes, P, ldp, bias, coef, index,
    slope, sel`` of ``edge_fwd_typed``) whose output it is: both Linears then run as ONE launch over the class tiles ``tiles``
    (``edge_mlp_fwd``), which fills ``h1`` on the way (no ``prev2``, no activation on the result)."""
    R, H = h1.shape
    if out is None:
        out = dead_rows_buffer((R, H), h1.device)
    if first is not None:
        if prev2 is not None or slope is not None:
            raise _lib.DmpError("out_fwd_typed(first=...): neither a second addend nor an activation on the result")
        edge_mlp_fwd(first["z"], first["Wes"], first["P"], first["ldp"], first["bias"], first["coef"], first["index"], first["slope"],
                     W2t, b2, prev, tiles, sel=first.get("sel"), w_in_out=w_in_out, h1=h1, out=out)
        return out
    typed_jobs([dict(a=h1, W=W2t, bias=b2, prev=prev, prev2=prev2, out=out, w_in_out=w_in_out, slope=slope)], tiles)
    return out


USE_EDGE_MLP_FWD = True   # a gated inner layer's edge MLP forward over the kept edges' tiles as one launch (csrc/dmp_edgemlp.hip) instead of two


def edge_mlp_fwd_ok(H, *tensors):
    """``edge_mlp_fwd`` applies: H = 128, the bf16x6 arithmetic, fp32 operands with unit column stride in rows of whole 16-byte pieces,
    arrays below 4 GiB.  Otherwise the two launches (``edge_fwd_typed`` / ``out_fwd_typed``) run."""
    return bool(USE_EDGE_MLP_FWD and _one_launch_mlp_operands_ok(H, tensors))


def _one_launch_mlp_operands_ok(H, tensors):
    if H != 128 or _lib.load().dmp_dev_get_exact_fp32():
        return False
    lim = (1 << 32) - 65536
    for a in tensors:
        if a is None:
            continue
        if (a.dtype != torch.float32 or a.dim() != 2 or a.stride(1) != 1 or a.stride(0) % 4 or a.stride(0) * 4 > 16383
                or a.data_ptr() % 16 or a.size(0) * a.stride(0) * 4 >= lim):
            return False
    return True


USE_L0_EDGE_MLP = True    # the first layer's edge MLP forward from the label codes as one launch (csrc/dmp_l0mlp.hip) instead of one per table + one


def l0_edge_mlp_ok(H, K, tables, *tensors):
    """The one-launch form of ``l0_edge_fwd`` + ``out_fwd_typed_codes`` applies: H = 128, the bf16x6 arithmetic, at most two embedding
    tables of at most ``dmp_l0_edge_mlp_max_codes()`` code columns, fp32 operands with unit column stride in rows of whole 16-byte
    pieces, arrays below 4 GiB.  Otherwise the launches of their own run."""
    return bool(USE_L0_EDGE_MLP and 1 <= tables <= 2 and 1 <= K <= _lib.load().dmp_l0_edge_mlp_max_codes()
                and _one_launch_mlp_operands_ok(H, tensors))


def edge_mlp_fwd(z, Wes, P, ldp, bias, coef, index, slope, W2t, b2, prev, tiles, sel=None, w_in_out=True, h1=None, out=None):
    """``(H1e, zn)`` of a layer's edge MLP for the edges of ``tiles`` (``live_tiles``: the class tiles of the edges a 0 / 1 gate keeps)
    in ONE launch (``dmp_edge_mlp_fwd``): ``H1e = act(z W_g + P[a] - P[b] + bias)`` as ``edge_fwd_typed`` makes it and
    ``zn = prev + (H1e W2t + b2)`` as ``out_fwd_typed`` does, bit for bit -- H1e is stored once and not read back.  Rows outside the
    tiles are neither read nor written (``dead_rows_buffer``).  ``P``: the gathered projections with leading dimension ``ldp``;
    ``sel`` as in ``edge_fwd_typed``; ``prev`` None: no residual."""
    lib = _lib.load()
    E, H = z.shape
    slot_edge, tile_scale, num_tiles, bound = tiles
    if h1 is None:
        h1 = dead_rows_buffer((E, H), z.device)
    if out is None:
        out = dead_rows_buffer((E, H), z.device)
    Wes = Wes.contiguous()
    sel_a, sel_b = (sel[0], sel[1]) if sel is not None else index.edge_select(coef)[:2]
    _lib.require_gpu(z, Wes, P, bias, W2t, b2, prev, h1, out)
    # (the record form of the first of the two launches this one replaces: bench.py prices the names it knows at the kept rows)
    with _lib.timed("edge_fwd_typed[H=%d,E=%d]", (H, E), 4 * H * (2 * E + 2 * index.num_nodes) + 12 * E):
        check(lib.dmp_edge_mlp_fwd(ptr(z), z.stride(0), ptr(Wes), Wes.size(1), ptr(P), ldp, index.num_nodes, ptr(bias), ptr(sel_a), ptr(sel_b),
                                   ptr(W2t), W2t.stride(0), int(bool(w_in_out)), ptr(b2), ptr(prev), prev.stride(0) if prev is not None else H,
                                   ptr(slot_edge), ptr(tile_scale), ptr(num_tiles), bound, E, H, float(slope), ptr(h1), h1.stride(0),
                                   ptr(out), out.stride(0), stream_ptr()), "dmp_edge_mlp_fwd")
    return h1, out


def bwd_h1_typed(d_o, W2, h1, tiles, slope=0.0, out=None):
    """``(dPre, column sums of dPre, column sums of the kept rows of d_o)`` with ``dPre[e] = act'(h1[e]) (.) (d_o[e] W2)`` for the
    rows of ``tiles`` (``live_tiles`` / ``NodeRows.tiles``); the other rows of ``dPre`` are not written (``dead_rows_buffer``, or
    ``out``: e.g. a column block of a wider matrix)."""
    lib = _lib.load()
    E, H = d_o.shape
    slot_edge, tile_scale, num_tiles, bound = tiles
    d_g = out if out is not None else dead_rows_buffer((E, H), d_o.device)
    G = int(lib.dmp_typed_partial_rows(bound, H))
    part = torch.empty((G, H), dtype=torch.float32, device=d_o.device)
    part_rows = torch.empty_like(part)
    W2 = W2.contiguous()
    with _lib.timed("bwd_h1_typed[H=%d,E=%d]", (H, E), 12 * H * E + 4 * E):
        check(lib.dmp_bwd_h1_typed(ptr(d_o), d_o.stride(0), ptr(W2), W2.size(1), ptr(h1), h1.stride(0), ptr(slot_edge), ptr(tile_scale),
                                   ptr(num_tiles), bound, E, H, slope, ptr(d_g), d_g.stride(0), ptr(part), ptr(part_rows), stream_ptr()),
              "dmp_bwd_h1_typed")
    return d_g, reduce_partials(part), reduce_partials(part_rows)


USE_NODE_CHAIN = True   # a layer's node side over the kept nodes' tiles as one launch per pass (csrc/dmp_nodechain.hip) instead of three


def node_chain_ok(H, *tensors):
    """``node_chain_fwd`` / ``node_chain_bwd`` apply: H = 128, the bf16x6 arithmetic, fp32 operands with unit column stride in rows of
    whole 16-byte pieces, arrays below 4 GiB.  Otherwise the three-launch chain (``typed_jobs`` / ``out_fwd_typed`` / ``bwd_h1_typed``) runs."""
    if not USE_NODE_CHAIN or H != 128 or _lib.load().dmp_dev_get_exact_fp32():
        return False
    lim = (1 << 32) - 65536
    for a in tensors:
        if a is None:
            continue
        if (a.dtype != torch.float32 or a.dim() != 2 or a.stride(1) != 1 or a.stride(0) % 4 or a.stride(0) * 4 > 16383
                or a.data_ptr() % 16 or a.size(0) * a.stride(0) * 4 >= lim):
            return False
    return True


def node_chain_panels(Bn, Wx, nW2):
    """``(forward panels, backward panels)``: the six weight panels of each pass of a layer's node side as bf16 pieces in the kernel's
    fragment order (``dmp_node_chain_pack``: one launch for both; made once per layer and step, beside the parameter fold, not per
    workgroup).  Forward: Wx1, Wx2, Wx0, Bn_in, Bn_out, W2^T; backward: W2, Bn_in^T, Bn_out^T, Wx0^T, Wx1^T, Wx2^T."""
    lib = _lib.load()
    H = Bn.size(1)
    Bn, Wx, nW2 = Bn.detach(), Wx.detach(), nW2.detach()
    _lib.require_gpu(Bn, Wx, nW2)
    if not (Bn.is_contiguous() and Wx.is_contiguous() and nW2.is_contiguous()):
        raise _lib.DmpError("node_chain_panels: contiguous weights expected")
    words = int(lib.dmp_node_chain_panel_words())
    out = torch.empty(12 * words, dtype=torch.int32, device=Bn.device)
    e = Bn.element_size()
    spec = [(Wx.data_ptr() + H * e, 3 * H, 0), (Wx.data_ptr() + 2 * H * e, 3 * H, 0), (Wx.data_ptr(), 3 * H, 0),
            (Bn.data_ptr(), H, 0), (Bn.data_ptr() + H * H * e, H, 0), (nW2.data_ptr(), H, 1),
            (nW2.data_ptr(), H, 0), (Bn.data_ptr(), H, 1), (Bn.data_ptr() + H * H * e, H, 1),
            (Wx.data_ptr(), 3 * H, 1), (Wx.data_ptr() + H * e, 3 * H, 1), (Wx.data_ptr() + 2 * H * e, 3 * H, 1)]
    J = (_abi.dmp_chain_panel * len(spec))()
    for j, (w, ld, tr) in zip(J, spec):
        j.W, j.ld, j.transposed = w, ld, tr
    check(lib.dmp_node_chain_pack(J, len(spec), ptr(out), stream_ptr()), "dmp_node_chain_pack")
    return out[:6 * words], out[6 * words:]


def node_chain_fwd(x, S, panels, bn, b2, residual, slope, tiles, H1n, P, xn):
    """The forward node side of a layer for the rows of ``tiles`` in ONE launch (``dmp_node_chain_fwd``): ``H1n = act(x Wx0 + S_in Bn_in
    + S_out Bn_out + bn)``, ``P = [x Wx1 | x Wx2]``, ``xn = x + H1n W2^T + b2`` (``residual`` false: without x).  ``S`` [R, >= 2H] =
    [S_in | S_out], ``P`` [R, >= 2H]; any row strides (column blocks of wider buffers).  ``panels``: ``node_chain_panels(...)[0]``.
    Rows outside the tiles are neither read nor written."""
    lib = _lib.load()
    slot, _, num_tiles, bound = tiles
    R, H = x.shape
    _lib.require_gpu(x, S, panels, bn, b2, H1n, P, xn)
    # (the record form of the launches this one replaces: bench.py prices the names it knows at the kept rows -- 6 arrays here, 7 moved)
    with _lib.timed("out_fwd_typed[H=%d,R=%d,jobs=2]", (H, R), 4 * H * R * 6):
        check(lib.dmp_node_chain_fwd(ptr(x), x.stride(0), ptr(S), S.stride(0), ptr(panels), ptr(bn), ptr(b2), int(bool(residual)), float(slope),
                                     ptr(slot), ptr(num_tiles), bound, R, H, ptr(H1n), H1n.stride(0), ptr(P), P.stride(0), ptr(xn), xn.stride(0),
                                     stream_ptr()), "dmp_node_chain_fwd")
    return H1n, P, xn


def node_chain_bwd(dxn, H1n, dP, panels, residual, slope, tiles, dPn, dS, dx=None):
    """The backward node side of a layer for the rows of ``tiles`` in ONE launch (``dmp_node_chain_bwd``): ``dPn = act'(H1n) (.) (dxn W2)``,
    ``dS = [dPn Bn_in^T | dPn Bn_out^T]``, ``dx = dxn + dPn Wx0^T + dP[:, :H] Wx1^T + dP[:, H:] Wx2^T`` (``residual`` false: without dxn;
    ``dx`` None: not formed, ``dP`` not read).  Returns ``(column sums of dPn, column sums of the kept rows of dxn)`` as
    ``bwd_h1_typed`` does (``reduce_partials``: deferred inside ``deferred_reductions``).  ``panels``: ``node_chain_panels(...)[1]``."""
    lib = _lib.load()
    slot, _, num_tiles, bound = tiles
    R, H = dxn.shape
    _lib.require_gpu(dxn, H1n, dP, panels, dPn, dS, dx)
    G = int(lib.dmp_node_chain_blocks(bound))
    part = torch.empty((G, H), dtype=torch.float32, device=dxn.device)
    part_rows = torch.empty_like(part)
    with _lib.timed("out_fwd_typed[H=%d,R=%d,jobs=2]", (H, R), 4 * H * R * 6):
        check(lib.dmp_node_chain_bwd(ptr(dxn), dxn.stride(0), ptr(H1n), H1n.stride(0), ptr(dP), dP.stride(0) if dP is not None else 2 * H,
                                     ptr(panels), int(bool(residual)), float(slope), ptr(slot), ptr(num_tiles), bound, R, H,
                                     ptr(dPn), dPn.stride(0), ptr(dS), dS.stride(0), ptr(dx), dx.stride(0) if dx is not None else H,
                                     ptr(part), ptr(part_rows), stream_ptr()), "dmp_node_chain_bwd")
    return reduce_partials(part), reduce_partials(part_rows)


def h1w_ok(d_o, h1, H):
    """The one-launch form of ``bwd_h1_typed`` + ``atb_typed(plain=True)`` applies: H = 128, the bf16x6 arithmetic, arrays below 4 GiB."""
    lib = _lib.load()
    return (H == 128 and not lib.dmp_dev_get_exact_fp32() and d_o.size(0) * d_o.stride(0) * 4 < (1 << 32) - 65536
            and h1.size(0) * h1.stride(0) * 4 < (1 << 32) - 65536 and d_o.size(0) * H * 4 < (1 << 32) - 65536)


USE_H1W_CODES = True      # the first layer's code weight gradient of the target table from ``bwd_h1_w``'s launch (csrc/dmp_h1w.hip) instead of ``l0_bwd_w``'s
H1W_MAX_CODES = 16        # ``dmp_bwd_h1_w_max_codes()``: one 16-row half of the 32-row code operand


def h1w_codes_ok(l0, tables, walked, h1w=True):
    """``bwd_h1_w(codes=...)`` takes over the LAST embedding table's ``l0_bwd_w`` launch: the layer is the first one (``l0``: its
    ``Layer0Codes``), the one-launch kernel runs (``h1w``: ``h1w_ok`` -- H = 128, bf16x6, arrays below 4 GiB), at most
    ``H1W_MAX_CODES`` fp32 code columns with unit stride, two tables or more (the pattern's rows keep their ``l0_bwd_w`` launch) of
    which the last has edge rows, and ``l0_bwd_w`` would have walked the rows of the tile list that lie in the table's range --
    ``walked``: "kept" (the list holds the rows a 0 / 1 gate keeps, and ``l0_bwd_w`` walks the gate's mask over the range) or "all"
    (the identity list of a step without a gate: ``l0_bwd_w`` leaves out at most rows whose codes are zeros, which add zeros)."""
    if not (USE_H1W_CODES and l0 is not None and h1w and walked in ("kept", "all")):
        return False
    enc = l0.enc
    return bool(1 <= l0.K <= H1W_MAX_CODES and len(tables) >= 2 and tables[-1][1][1] > tables[-1][1][0]
                and enc.dtype == torch.float32 and enc.dim() == 2 and enc.stride(1) == 1 and enc.size(1) >= l0.K
                and enc.size(0) * enc.stride(0) * 4 < (1 << 32) - 65536)


def bwd_h1_w(d_o, W2, h1, tiles, slope=0.0, out=None, codes=None):
    """``(dPre, column sums of dPre, column sums of the kept rows of d_o, d_o^T h1)`` over the rows of ``tiles``: what
    ``bwd_h1_typed`` and ``atb_typed(d_o, h1, plain=True)`` return, from one pass over the two operands (``dmp_bwd_h1_w``).
    ``codes = dict(enc, K, coef_e, rows=(r0, r1), residual[, out])``: the first layer's launch (``dmp_bwd_h1_w_codes``) -- a fifth
    value ``[enc^T dPre | (coef_e enc)^T dPre (| enc^T d_o)]``, [K, 2H or 3H], over the rows of ``tiles`` inside ``rows``: what
    ``l0_bwd_w`` makes from a second read of ``dPre`` and ``d_o`` (``out``: where the reduced block goes)."""
    lib = _lib.load()
    E, H = d_o.shape
    slot_edge, _, num_tiles, bound = tiles
    d_g = out if out is not None else dead_rows_buffer((E, H), d_o.device)
    G = int(lib.dmp_bwd_h1_w_blocks(bound))
    part = torch.empty((G, H), dtype=torch.float32, device=d_o.device)
    part_rows = torch.empty_like(part)
    part_w = torch.empty((G, H * H), dtype=torch.float32, device=d_o.device)
    W2 = W2.contiguous()
    if codes is not None:
        enc, K, coef_e, (r0, r1), residual = codes["enc"], int(codes["K"]), codes["coef_e"], codes["rows"], bool(codes["residual"])
        _lib.require_gpu(enc, coef_e)
        if enc.dtype != torch.float32 or enc.stride(1) != 1 or coef_e.dtype != torch.float32 or not coef_e.is_contiguous() or coef_e.numel() < E:
            raise _lib.DmpError("bwd_h1_w: codes need fp32 code rows of unit column stride and one fp32 coefficient per edge row")
        nb = 3 if residual else 2
        part_x = torch.empty((G, K * nb * H), dtype=torch.float32, device=d_o.device)
        with _lib.timed("bwd_h1_w[H=%d,E=%d]", (H, E), 12 * H * E + 4 * E):
            check(lib.dmp_bwd_h1_w_codes(ptr(d_o), d_o.stride(0), ptr(W2), W2.size(1), ptr(h1), h1.stride(0), ptr(slot_edge), ptr(num_tiles),
                                         bound, E, H, slope, ptr(d_g), d_g.stride(0), ptr(part), ptr(part_rows), ptr(part_w),
                                         ptr(enc), enc.stride(0), K, ptr(coef_e), int(r0), int(r1), int(residual), ptr(part_x), stream_ptr()),
                  "dmp_bwd_h1_w_codes")
        xo = codes.get("out")
        xx = reduce_partials(part_x, None if xo is None else xo.view(-1)).view(K, nb * H)
        return d_g, reduce_partials(part), reduce_partials(part_rows), reduce_partials(part_w).view(H, H), xx
    with _lib.timed("bwd_h1_w[H=%d,E=%d]", (H, E), 12 * H * E + 4 * E):
        check(lib.dmp_bwd_h1_w(ptr(d_o), d_o.stride(0), ptr(W2), W2.size(1), ptr(h1), h1.stride(0), ptr(slot_edge), ptr(num_tiles), bound,
                               E, H, slope, ptr(d_g), d_g.stride(0), ptr(part), ptr(part_rows), ptr(part_w), stream_ptr()), "dmp_bwd_h1_w")
    return d_g, reduce_partials(part), reduce_partials(part_rows), reduce_partials(part_w).view(H, H)


USE_MASKED_SUMS = True   # the scatter-adds skip the rows a 0 / 1 edge gate wiped


def zero_rows_gate(gate):
    """``gate`` is 0 / 1 (``gatememo.mark(binary=)``) AND its maker multiplied the rep-net's input rows by it (``zero_rows=``, set by
    ``dmpnn.joint_rep``: the union's edge rows are ``[pattern rows | gate * target rows]``): every layer's input rows under a
    zero of the gate are zeros -- ``zn = z + gate (...)`` (dmpnn.py:215-277) keeps them so -- and sums over rows may leave
    them out."""
    own = None if gate is None else gatememo.owner(gate)
    return bool(USE_MASKED_SUMS and has_row_mask(own, True, True) and gatememo.flag(own, "zero_rows", True))


def binary_gate_mask(gate):
    """The row mask of a gate flagged 0 / 1 (e.g. a ScalarFilter gate), else None: for such a gate the mask says everything the
    gate says."""
    if gate is None or not USE_PLAIN_ATB or not gatememo.flag(gate, "binary"):
        return None
    return gate_row_mask(gate)


# ---- the dead-row conditions of a joint pass.  A row that one launch leaves unwritten must be left out by every reader, so each
# verdict is stated ONCE, here: host tests of the index's sizes, H, the gates' marks and the switches as they stand at the call (no
# launch, no memo build), asked by the layer's forward and backward, ``l0_dead_inputs`` and ``dmpnn.prefetch_joint_indexes``.
def has_row_mask(gate, binary=False, resolved=False):
    """``gate_row_mask(gate) is not None``, without building it; ``binary``: ... and flagged 0 / 1 (the kept-row lists, tiles, CSRs)."""
    own = gate if resolved or gate is None else gatememo.owner(gate)
    return bool(own is not None and USE_ROW_MASKS and (gatememo.skips_rows(own, True) if binary else not gatememo.flag(own, "dense", True)))


def dead_h1_rows(index, H, e_gate):
    """The rows of the edge MLP's activation H1e under a zero of ``e_gate`` are DEAD: their producers leave them out, every
    consumer (out_fwd / the pooled passes; bwd_h1, atb_rows, pool_relu_bwd) multiplies them by that zero without fetching."""
    return bool(SKIP_DEAD_ROWS and has_row_mask(e_gate) and typed_ok(index, H))


def live_tiles_ok(index, coef, gate):
    """``live_tiles(index, coef, gate) is not None``, without building them (``coef``: ``index``'s own, built from its integer degrees)."""
    src = getattr(index, "_coef_deg", None)
    return bool(USE_LIVE_TILES and has_row_mask(gate, binary=True) and src is not None and src[0] is coef and index.num_edges > 0)


def dead_edge_rows(index, H, e_gate, coef=None):
    """... and so are the layer's INPUT edge rows and their gradient rows (``zero_rows_gate``): not fetched, not computed.  With
    ``coef``: nor, in an inner layer, written -- the class-tile launches walk ``live_tiles``, which can be built."""
    own = None if e_gate is None else gatememo.owner(e_gate)      # (resolved once: the layers ask this several times per pass)
    return dead_h1_rows(index, H, own) and zero_rows_gate(own) and (coef is None or live_tiles_ok(index, coef, own))


def kept_node_path(index, H, v_gate, l0=None, min_nodes=4096):
    """A layer's node side runs on the nodes the 0 / 1 ``v_gate`` keeps (``node_rows``; from ``min_nodes`` nodes on: below, the
    dense launches are as fast).  ``l0``: the first layer on the label codes -- its backward's row masks start at a table's first node."""
    N = index.num_nodes
    return bool(USE_NODE_ROWS and USE_PLAIN_ATB and N >= min_nodes and index.num_edges > 0 and typed_ok(index, H) and zero_rows_gate(v_gate)
                and not (l0 is not None and any(n0 % 32 for _, _, (n0, _) in l0.tables(index.num_edges, N))))


def l0_row_list(r0, rows):
    """The first layer's launches over the ``rows`` edge rows from ``r0`` on walk a kept-row list (``kept_rows``) of their mask."""
    return bool(USE_L0_ROW_LISTS and r0 % 32 == 0 and rows >= L0_LIST_MIN_ROWS)


def kept_incidence_sums(index, H, e_gate, kept_nodes):
    """The backward's endpoint sums run over ``NodeRows.kept_incidence`` (``kept_nodes``: ``kept_node_path`` held)."""
    return bool(kept_nodes and dead_edge_rows(index, H, e_gate))


def bwd_h1_mfma(d_o, W2, h1, coef=None, index=None, both_halves=True, gate=None, out=None, slope=0.0, rows_colsum=False,
                skip_dead_stores=False):
    """-> (dG = [dPre | coef[dst] dPre] (or dPre alone) with dPre = h1>0 ? d_o W2 : slope (d_o W2), column sums of dPre); H=128.
    ``gate`` (dPre alone only): ``d_o`` is the ungated output gradient, its rows are scaled by the gate here.
    ``out`` (dPre alone only): destination [R, H], e.g. a column slice of a wider matrix.
    ``rows_colsum``: a third result, the column sums of the rows of ``d_o`` the kernel fetched -- with the row mask of a 0 / 1
    gate (``binary_gate_mask``) that is ``sum_e gate_e d_o[e]``, the bias gradient of the Linear behind the gate.
    ``skip_dead_stores`` (dPre alone, gated): dPre's rows under a zero gate (zeros) are not stored: every reader leaves them out."""
    lib = _lib.load()
    E, H = d_o.shape
    mask = gate_row_mask(gate)
    skip_dead_stores = bool(skip_dead_stores and mask is not None and not both_halves and out is None)
    if both_halves:
        d_g = torch.empty((E, 2 * H), dtype=torch.float32, device=d_o.device)
        coef_e = index.edge_select(coef)[2]
    else:
        d_g = out if out is not None else (dead_rows_buffer((E, H), d_o.device) if skip_dead_stores
                                           else torch.empty((E, H), dtype=torch.float32, device=d_o.device))
        coef_e = None
    part = torch.empty((int(lib.dmp_mfma_partial_rows_h(E, H)), H), dtype=torch.float32, device=d_o.device)
    W2 = W2.contiguous()
    with _lib.timed("bwd_h1_mfma[H=%d,E=%d]", (H, E), (16 if both_halves else 12) * H * E + 4 * E):
        part_rows = torch.empty_like(part) if rows_colsum else None
        check(lib.dmp_bwd_h1_fused_rows(ptr(d_o), d_o.stride(0), ptr(W2), W2.size(1), ptr(h1), h1.stride(0), ptr(coef_e),
                                        ptr(gate), ptr(mask), int(skip_dead_stores), E, H, slope, ptr(d_g),
                                        d_g.stride(0) if E > 1 else d_g.size(1), ptr(part), ptr(part_rows), stream_ptr()),
              "dmp_bwd_h1_fused")
    if rows_colsum:
        return d_g, reduce_partials(part), reduce_partials(part_rows)
    return d_g, reduce_partials(part)


USE_PLAIN_ATB = True


def atb_rows(a, b, gate=None, colsum=True):
    """``((gate (.) a)^T b  [M,N],  column sums of gate (.) a  [M] (or None))`` in one MFMA pass over the rows
    (csrc/dmp_atb.hip); M, N multiples of 128 (or of 64).  A Linear's weight and bias gradient with a row gate fused in.
    A gate flagged as 0 / 1 (``gatememo.mark(binary=)``: a ScalarFilter gate) is fully expressed by its row mask: the product then runs
    ungated over the masked-in rows on the bf16 pipe (``dmp_atb_rows_plain``), the column sums as a one-column ``smallk_atb``."""
    lib = _lib.load()
    R, M = a.shape
    N = b.size(1)
    blk = atb_block(M, N)
    G = int(lib.dmp_atb_rows_blocks_h(R, M, N, blk))
    part = torch.empty((G, M * N), dtype=torch.float32, device=a.device)
    mask = binary_gate_mask(gate)
    if mask is not None and M % blk == 0 and blk in (64, 128):
        with _lib.timed("atb_rows_plain[M=%d,N=%d,R=%d]", (M, N, R), 4 * (M + N) * R):
            check(lib.dmp_atb_rows_plain(ptr(a), a.stride(0), ptr(b), b.stride(0), ptr(mask), R, M, N, blk, ptr(part), stream_ptr()),
                  "dmp_atb_rows_plain")
        cs = None
        if colsum:   # sum over the kept rows of a = gate^T a: the K = 1 case of the narrow weight-gradient kernel, same mask
            cs = smallk_atb_cols(gate.reshape(-1, 1), a, H=blk, mask=mask).reshape(M)
        return reduce_partials(part).view(M, N), cs
    part_cs = torch.empty((G, M), dtype=torch.float32, device=a.device) if colsum else None
    with _lib.timed("atb_rows[M=%d,N=%d,R=%d]", (M, N, R), 4 * (M + N) * R + (4 * R if gate is not None else 0)):
        check(lib.dmp_atb_rows_masked(ptr(a), a.stride(0), ptr(b), b.stride(0), ptr(gate), ptr(gate_row_mask(gate)),
                                      R, M, N, blk, ptr(part), ptr(part_cs), stream_ptr()), "dmp_atb_rows_masked")
    return reduce_partials(part).view(M, N), (reduce_partials(part_cs) if colsum else None)


SMALLK_MAX = 16


def smallk_atb(x, d, gate=None, out=None):
    """``x^T (gate (.) d)``  ([K, H], K <= 16, H = 128 or 64) in one pass over ``d``: the weight gradient of a narrow
    input layer (label encodings @ W) whose output was gated row-wise (csrc/dmp_fused.hip::smallk_atb_k)."""
    lib = _lib.load()
    R, K = x.shape
    H = d.size(1)
    G = int(lib.dmp_smallk_atb_blocks(R))
    part = torch.empty((G, K * H), dtype=torch.float32, device=d.device)
    with _lib.timed("smallk_atb[K=%d,R=%d]", (K, R), 4 * (H + K + 1) * R):
        check(lib.dmp_smallk_atb(ptr(x), x.stride(0), K, ptr(d), d.stride(0), ptr(gate), R, H, ptr(part), stream_ptr()),
              "dmp_smallk_atb")
    return reduce_partials(part, None if out is None else out.view(-1)).view(K, H)


def smallk_embed(x, W, gate=None, out=None, H=None):
    """``gate (.) (x @ W)``  for a narrow ``x`` ([R, K <= 16]: label encodings) and ``W`` [K, C]: one pass, the K rows of W
    in registers (csrc/dmp_fused.hip::smallk_embed_k).  C = 128 or 64, or a multiple of 128 (one launch, a grid row per
    block of 128 columns); ``W`` / ``out`` may be column blocks of wider matrices (unit inner stride)."""
    lib = _lib.load()
    R, K = x.shape
    C = W.size(1)
    H = H if H is not None else (C if C in (64, 128) else 128)
    ncols = C // H
    if out is None:
        out = torch.empty((R, C), dtype=torch.float32, device=x.device)
    with _lib.timed("smallk_embed[K=%d,R=%d]", (K, R), 4 * (C + K + 1) * R):
        check(lib.dmp_smallk_embed_cols(ptr(x), x.stride(0), K, ptr(W), W.stride(0), ptr(gate), R, H, ncols, ptr(out), out.stride(0),
                                        stream_ptr()), "dmp_smallk_embed_cols")
    return out


def smallk_atb_cols(x, d, d2=None, out=None, H=None, mask=None, rows=None):
    """``x^T [d | d2]`` per block of 128 (or 64: one block) columns -> [blocks, K, H]: ``smallk_atb`` over the column blocks
    of ``d`` [R, ncols H] and one more matrix ``d2`` [R, H] in ONE launch.  ``mask`` (uint32 words, ``gate_row_mask``, aligned
    to x's first row): the rows of ``d`` / ``d2`` whose row of ``x`` is known to be all zeros are not fetched.  ``rows`` =
    ``(list, count)`` (``kept_rows`` relative to x's first row) instead of ``mask``: the launch walks the list -- every batch of
    rows is live rows; a row outside the list must be a zero row of ``x``."""
    lib = _lib.load()
    R, K = x.shape
    C = d.size(1)
    H = H if H is not None else (C if C in (64, 128) else 128)
    ncols = C // H
    nblk = ncols + (1 if d2 is not None else 0)
    G = int(lib.dmp_smallk_atb_blocks(R))
    part = torch.empty((nblk, G, K * H), dtype=torch.float32, device=d.device)
    if out is None:
        out = torch.empty((nblk, K, H), dtype=torch.float32, device=d.device)
    with _lib.timed("smallk_atb[K=%d,R=%d]", (K, R), 4 * (nblk * H + K + 1) * R):
        if rows is not None:
            check(lib.dmp_smallk_atb_cols_rows(ptr(x), x.stride(0), K, ptr(d), d.stride(0), ncols, ptr(d2),
                                               d2.stride(0) if d2 is not None else 0, ptr(rows[0]), ptr(rows[1]), R, H, ptr(part), stream_ptr()),
                  "dmp_smallk_atb_cols_rows")
        else:
            check(lib.dmp_smallk_atb_cols_masked(ptr(x), x.stride(0), K, ptr(d), d.stride(0), ncols, ptr(d2),
                                                 d2.stride(0) if d2 is not None else 0, None, ptr(mask), R, H, ptr(part), stream_ptr()),
                  "dmp_smallk_atb_cols")
    for j in range(nblk):
        reduce_partials(part[j], out[j].view(-1))
    return out


def smallk_atb_jobs(jobs, H):
    """Several ``smallk_atb`` products of the same K and H in ONE launch (``dmp_smallk_atb_jobs``): ``jobs`` = up to four
    ``(x [R, K], d [R, H], out [K, H], mask or None)`` (``mask``: ``gate_row_mask`` words aligned to the job's first row).  The
    sums land in each job's ``out``."""
    lib = _lib.load()
    K = jobs[0][0].size(1)
    J = (_abi.dmp_smallk_job * len(jobs))()
    parts = []
    for n, (x, d, out, mask) in enumerate(jobs):
        R = x.size(0)
        _lib.require_gpu(x, d, out, mask)
        if x.size(1) != K or d.size(0) != R or d.size(1) != H or tuple(out.shape) != (K, H) or not out.is_contiguous():
            raise _lib.DmpError("smallk_atb_jobs: shapes of job %d" % n)
        part = torch.empty((int(lib.dmp_smallk_atb_blocks(R)), K * H), dtype=torch.float32, device=d.device)
        J[n].X, J[n].ldx, J[n].D, J[n].ldd = (x.data_ptr() if R else None), x.stride(0) if R > 1 else max(K, x.stride(0)), (d.data_ptr() if R else None), d.stride(0) if R > 1 else max(H, d.stride(0))
        J[n].gate, J[n].rowmask, J[n].R, J[n].partial = None, ptr(mask), R, part.data_ptr()
        parts.append(part)
    with _lib.timed("smallk_atb_jobs[K=%d,R=%d]", (K, sum(j[0].size(0) for j in jobs)), sum(4 * (H + K + 1) * j[0].size(0) for j in jobs)):
        check(lib.dmp_smallk_atb_jobs(J, len(jobs), K, H, stream_ptr()), "dmp_smallk_atb_jobs")
    for part, (_, _, out, _) in zip(parts, jobs):
        reduce_partials(part, out.view(-1))


# ---- the first layer of a rep-net straight from the label codes (csrc/dmp_layer0.hip)
L0_KMAX = 16
# the joint rep-net pass hands the first layer the packed label codes instead of differentiable [E, H] rows
# (dmpnn.joint_rep); DMP_LAYER0=0 keeps the general path
USE_LAYER0 = _os.environ.get("DMP_LAYER0", "1") == "1"


def l0_pack(enc_p, enc_g, gate=None, stacked=False):
    """``[enc_p ; gate * enc_g]`` zero-padded to a multiple of 4 columns: the gated label codes of the union's rows.
    ``stacked``: the second kind of rows keep their codes in columns K..2K-1, so that two embedding tables stacked to
    [2K, H] act as ONE table on the packed codes (the node rows: 2K <= 16)."""
    lib = _lib.load()
    _lib.require_gpu(enc_p, enc_g)
    K = enc_g.size(1)
    goff = K if stacked else 0
    Kpad = (goff + K + 3) // 4 * 4
    n, rows_g = enc_p.size(0), enc_g.size(0)
    out = torch.empty((n + rows_g, Kpad), dtype=torch.float32, device=enc_g.device)
    gt = None if gate is None else gate.reshape(-1).contiguous()
    check(lib.dmp_l0_pack(ptr(enc_p), enc_p.stride(0) if n else K, n, ptr(enc_g), enc_g.stride(0) if rows_g else K, ptr(gt), rows_g,
                          K, Kpad, goff, ptr(out), stream_ptr()), "dmp_l0_pack")
    return out


def l0_pack_many(specs):
    """``[l0_pack(*spec) for spec in specs]`` (``spec`` = ``(enc_p, enc_g, gate, stacked)``; at most two) in ONE launch
    (``dmp_l0_pack_jobs``): a step's edge codes and node codes."""
    lib = _lib.load()
    J = (_abi.dmp_l0_pack_job * len(specs))()
    outs, keep = [], []
    for i, (enc_p, enc_g, gate, stacked) in enumerate(specs):
        _lib.require_gpu(enc_p, enc_g)
        K = enc_g.size(1)
        goff = K if stacked else 0
        Kpad = (goff + K + 3) // 4 * 4
        n, rows_g = enc_p.size(0), enc_g.size(0)
        out = torch.empty((n + rows_g, Kpad), dtype=torch.float32, device=enc_g.device)
        gt = None if gate is None else gate.reshape(-1).contiguous()
        J[i].enc_p, J[i].ldp, J[i].rows_p = ptr(enc_p), (enc_p.stride(0) if n else K), n
        J[i].enc_g, J[i].ldg, J[i].gate, J[i].rows_g = ptr(enc_g), (enc_g.stride(0) if rows_g else K), ptr(gt), rows_g
        J[i].K, J[i].Kpad, J[i].goff, J[i].out = K, Kpad, goff, out.data_ptr()
        outs.append(out)
        keep.append(gt)
    check(lib.dmp_l0_pack_jobs(J, len(specs), stream_ptr()), "dmp_l0_pack_jobs")
    return outs


USE_L0_ROW_LISTS = True
L0_LIST_MIN_ROWS = 32768       # shorter row ranges (the pattern side) keep the masked form: the list costs two launches


def _kept_rows_buffers(R, tiles, device):
    """``(list, count, scratch)`` of ``dmp_kept_rows`` over ``R`` rows, one allocation: the list (``tiles``: padded to whole 32-row
    tiles), its count words (rows; ``tiles``: rows, tiles), the kernel's scratch."""
    cap, ncnt = ((R + 31) // 32 * 32, 2) if tiles else (R, 1)
    out = torch.empty(cap + ncnt + int(_lib.load().dmp_kept_rows_scratch_words(R)), dtype=torch.int32, device=device)
    return out[:cap], out[cap:cap + ncnt], out[cap + ncnt:]


def kept_rows_name(r0, r1, tiles=False):
    """The name under which ``kept_rows(mask, r0, r1, tiles)`` hangs on ``mask`` (``gatememo``)."""
    return ("kept_rows", tiles, r0, r1)           # (False == 0 and True == 1, also as parts of a dict key)


def kept_rows(mask, r0, r1, tiles=False):
    """``(list int32 [r1 - r0], count int32 [1])``: the rows of ``[r0, r1)`` (r0 a multiple of 32) whose bit of ``mask`` is set, as
    ids relative to r0, ascending (``dmp_kept_rows``); memoised on the mask tensor (the forward and the backward of a layer
    share it).  ``tiles``: the list padded with -1 to whole 32-row tiles and ``count`` int32 [2] = (rows, tiles): a slot list
    for the tile kernels (``node_tiles``)."""
    def build():
        R = r1 - r0
        lst, cnt, scratch = _kept_rows_buffers(R, tiles, mask.device)
        check(_lib.load().dmp_kept_rows(ptr(mask[r0 // 32:]), R, int(bool(tiles)), ptr(scratch), ptr(lst), ptr(cnt), stream_ptr()), "dmp_kept_rows")
        return lst, cnt

    return gatememo.memo(mask, kept_rows_name(r0, r1, tiles), (), build)


USE_GATE_BUNDLE = True      # the index arrays a step derives from its two 0 / 1 gates in three launches instead of ten (``gate_bundle``)


def gate_bundle(index, v_gate, e_gate, want_nodes=False, l0_range=None, want_ascending=False):
    """What ``gate_row_mask`` (both gates), ``kept_rows`` (the kept nodes' tiles, the first layer's kept target rows, the kept
    edges' ascending tiles) and ``GraphIndex.edge_select_nodes`` build in ten launches of ~5 us -- links of the step's index
    chain, which the first layer waits for -- in THREE: both masks (``dmp_row_mask_bits_jobs``), then every list's block counts
    and the selectors, then every list's fill (``dmp_kept_rows_jobs``).  Each product is planted in the memo its own function
    looks it up in (same bits: the multi-job kernels are the single ones over ``blockIdx.y``); anything not asked for, or
    already there, is left to those functions."""
    if not USE_GATE_BUNDLE or not USE_ROW_MASKS:
        return
    lib = _lib.load()
    todo = []
    for g in (v_gate, e_gate):
        if g is None or not g.is_cuda or g.dtype != torch.float32 or gatememo.flag(g, "dense"):
            return
        if gatememo.peek(g, "row_mask") is None:
            todo.append(g)
    if todo:
        jobs = (_abi.dmp_rowmask_job * len(todo))()
        masks = [torch.empty(((g.numel() + 31) // 32,), dtype=torch.int32, device=g.device) for g in todo]
        for j, (g, m) in enumerate(zip(todo, masks)):
            jobs[j].gate, jobs[j].R, jobs[j].mask = ptr(g), g.numel(), ptr(m)
        check(lib.dmp_row_mask_bits_jobs(jobs, len(todo), stream_ptr()), "dmp_row_mask_bits_jobs")
        for g, m in zip(todo, masks):
            gatememo.plant(g, "row_mask", (), m)
    vmask, emask = gate_row_mask(v_gate), gate_row_mask(e_gate)
    if vmask is None or emask is None:
        return
    N, E = index.num_nodes, index.num_edges
    lists = [(vmask, 0, N, 1)] if want_nodes and N > 0 else []                 # (mask, r0, r1, tiles)
    if l0_range is not None and l0_range[1] > l0_range[0] and l0_range[0] % 32 == 0:
        lists.append((emask, l0_range[0], l0_range[1], 0))
    if want_ascending and E > 0:
        lists.append((emask, 0, E, 1))
    lists = [l for l in lists if gatememo.peek(l[0], kept_rows_name(*l[1:])) is None]
    sel = want_nodes and E > 0 and gatememo.peek(index, "edge_select_nodes", (vmask,)) is None
    if not lists and not sel:
        return
    jobs = (_abi.dmp_kept_job * max(len(lists), 1))()
    made = []
    for j, (m, r0, r1, tiles) in enumerate(lists):
        lst, cnt, scratch = _kept_rows_buffers(r1 - r0, tiles, m.device)
        jobs[j].mask, jobs[j].R, jobs[j].tiles, jobs[j].scratch, jobs[j].list, jobs[j].count = ptr(m[r0 // 32:]), r1 - r0, tiles, ptr(scratch), ptr(lst), ptr(cnt)
        made.append((lst, cnt))
    so = torch.empty((3, E), dtype=torch.int32, device=index.device) if sel else None
    check(lib.dmp_kept_rows_jobs(jobs, len(lists), ptr(index.src32) if sel else None, ptr(index.dst32) if sel else None,
                                 ptr(index.rev8) if sel else None, ptr(vmask) if sel else None, E if sel else 0,
                                 ptr(so[0]) if sel else None, ptr(so[1]) if sel else None, ptr(so[2]) if sel else None, stream_ptr()),
          "dmp_kept_rows_jobs")
    for (m, r0, r1, tiles), val in zip(lists, made):
        gatememo.plant(m, kept_rows_name(r0, r1, tiles), (), val)
    if sel:
        gatememo.plant(index, "edge_select_nodes", (vmask,), (so[0], so[1], so[2]))


USE_NODE_ROWS = _os.environ.get("DMP_NODE_ROWS", "1") == "1"   # the node side of a layer over the nodes a 0 / 1 node gate keeps


class NodeRows:
    """The nodes a 0 / 1 node gate keeps, as the kernels of a layer's node side want them (``node_rows``): ``mask`` (uint32
    words, bit = kept), ``rows`` = ``(list, count)`` ascending ids (``dmp_kept_rows``), ``tiles`` = the same list as a tile slot
    list ``(slot, tile_scale, num_tiles, bound)`` for ``dmp_out_fwd_typed`` / ``dmp_bwd_h1_typed``, ``sel`` = the per-edge
    selectors / destinations with the other nodes replaced by -1 (``GraphIndex.edge_select_nodes``)."""

    def __init__(self, mask, rows, tiles, sel, prefix=0):
        self.mask, self.rows, self.tiles, self.sel = mask, rows, tiles, sel
        self.prefix = int(prefix)     # the first ``prefix`` nodes are all kept (the pattern's nodes of a joint pass): list[q] == q there

    def kept_incidence(self, index, e_gate, in_only=False):
        """``(ptr, ent)``: the incidence CSR over the edges the 0 / 1 ``e_gate`` keeps, one row per POSITION of ``rows``
        (``dmp_incidence_keep``): what the backward's endpoint sums walk -- an edge row without a kept endpoint is never
        fetched.  ``in_only``: the in-entries alone = the kept edges' CSR by destination, a row per position (the forward
        aggregation).  Memoised on the gate per ``NodeRows`` (the layers of a rep-net share it)."""
        def build():
            N = index.num_nodes
            row_cnt, kptr, kent = _csr_keep_buffers(N, (1 if in_only else 2) * index.num_edges, index.in_ptr.device)
            check(_lib.load().dmp_incidence_keep(ptr(index.in_ptr), ptr(index.in_ent), None if in_only else ptr(index.out_ptr),
                                                 None if in_only else ptr(index.out_ent), ptr(e_gate.reshape(-1)),
                                                 ptr(self.rows[0]), ptr(self.rows[1]), N, ptr(row_cnt), ptr(kptr), ptr(kent), stream_ptr()),
                  "dmp_incidence_keep")
            return kptr, kent

        return gatememo.memo(e_gate, ("kept_incidence", bool(in_only)), (self,), build)


def node_rows(index, v_gate, H):
    """``NodeRows`` when a layer's node side can run on the kept nodes only: ``v_gate`` is 0 / 1 and its maker multiplied the
    rep-net's input node rows by it (``zero_rows_gate``: the rows under its zeros are zeros in EVERY layer, dmpnn.py:245-277,
    so for such a node v the aggregate A[v], the projections P[v], node_out[v] and every gradient row of v are dead), the
    tile kernels take the shape.  Memoised on the gate (the layers of a rep-net share it).  Else None."""
    if not kept_node_path(index, H, v_gate, min_nodes=0):      # (the list itself can be built for any number of nodes)
        return None
    mask = gate_row_mask(v_gate)

    def build():
        N = index.num_nodes
        lst, cnt = kept_rows(mask, 0, N, tiles=True)
        bound = (N + 31) // 32
        scale = const_zeros(bound, mask.device)
        return NodeRows(mask, (lst, cnt[0:1]), (lst, scale, cnt[1:2], bound), index.edge_select_nodes(mask),
                        prefix=min(int(gatememo.flag(v_gate, "ones_prefix")), N))

    return gatememo.memo(v_gate, "node_rows", (index,), build)


# (measured, round 5: LARGE kernels do not gain from the side stream -- the weight-gradient launches of a layer's backward beside its
# data-gradient chain +2.6 %, the second half of a layer's node side beside its edge side +1.8 % per step: two bandwidth-bound
# launches in flight slow each other down by more than the tails they fill; the partial reductions of a layer's weight gradients
# beside the rest of its backward +1 %, the first layer's pass over dPre / dZn beside the node side's short launches +0.7 %, the first
# layer's input rows (a 119 MB store) on a second side lane beside the layer's first launches +0.6 %.  The side stream carries the small
# index builds only.)
L0_NODE_MAX_COLS = 40      # code columns per node row that kernel holds in registers: VK + 2 K0


def l0_node_pack(VK, K0, H, Mv, Ma, Mb):
    """The packed matrix ``dmp_l0_node_fwd`` reads, [L0_NODE_MAX_COLS, 3H], from its three parts (``Mv`` [VK, 3H] = WV0 Wx, ``Ma`` /
    ``Mb`` [K0, H] = W0 Bn_in / W0 Bn_out); the layer writes the parts in place instead (one small-product launch)."""
    W = torch.zeros((L0_NODE_MAX_COLS, 3 * H), dtype=torch.float32, device=Mv.device)
    W[:VK] = Mv
    W[VK:VK + K0, :H] = Ma
    W[VK + K0:VK + 2 * K0, :H] = Mb
    return W


def l0_node_fwd(venc, VK, S0, K0, Kp, W, bias, slope, mask, n0, n1, H, h1, P, rows=None, q_begin=0):
    """``h1[n0:n1] = act([venc | S0_in | S0_out] W[:, :H] + bias)`` and ``P[n0:n1] = [venc | ..] W[:, H:3H]`` from the node rows'
    label codes and their edges' code sums (``dmp_l0_node_fwd``; ``W``: the packed matrix, ``l0_node_pack``); ``mask``: the
    kept nodes (``NodeRows.mask``) -- a dead node's ``h1`` row is left unwritten, its ``P`` row is zeros; ``rows`` =
    ``NodeRows.rows`` (the kept nodes' list over ALL nodes, with ``mask``): the launch walks the list instead of the masked rows,
    from position ``q_begin`` on (<= n0: e.g. ``NodeRows.prefix``, the leading nodes known to be all kept)."""
    lib = _lib.load()
    lst, cnt = rows if (rows is not None and mask is not None) else (None, None)
    with _lib.timed("l0_node_fwd[K=%d,R=%d]", (VK + 2 * K0, n1 - n0), 4 * (3 * H + VK + 2 * K0) * (n1 - n0)):
        check(lib.dmp_l0_node_fwd(ptr(venc), venc.stride(0), VK, ptr(S0), S0.stride(0), K0, Kp, ptr(W), W.stride(0), ptr(bias), float(slope),
                                  ptr(mask), ptr(lst), ptr(cnt), 0 if lst is None else lst.numel(), min(int(q_begin), n0), n0, n1, H,
                                  ptr(h1), h1.stride(0), ptr(P), P.stride(0), stream_ptr()), "dmp_l0_node_fwd")


USE_L0_NODE_MFMA = True        # the first layer's node side from the label codes as ONE launch on the matrix pipe (csrc/dmp_l0node.hip)
L0_NODE_MFMA_MAX_CODES = 16    # ... whose k-groups hold that many columns of venc / S0_in / S0_out each (dmp_l0_node_fwd_mfma_max_codes)


def l0_node_mfma_ok(H, VK, K0, Kp, tables, N, venc, S0, exact_fp32=None):
    """Whether ``l0_node_fwd_mfma`` takes the node side of a first layer (else ``l0_node_fwd`` per table): H = 128 on the bf16x6
    products, node codes, at most ``L0_NODE_MFMA_MAX_CODES`` columns per block and ``L0_NODE_MAX_COLS`` together, at most two
    tables, code rows of whole 16 bytes that the kernel's descriptors address (strides below 16 KiB, arrays below 4 GiB).
    ``exact_fp32``: the development switch's state (None: asked of the library)."""
    if not USE_L0_NODE_MFMA or H != 128 or venc is None or S0 is None or tables < 1 or tables > 2:
        return False
    if VK < 1 or K0 < 1 or VK > L0_NODE_MFMA_MAX_CODES or K0 > L0_NODE_MFMA_MAX_CODES or VK + 2 * K0 > L0_NODE_MAX_COLS:
        return False
    if exact_fp32 is None:
        exact_fp32 = _lib.load().dmp_dev_get_exact_fp32()
    if exact_fp32:
        return False
    lim = (1 << 32) - 65536
    ldv, lds = venc.stride(0), S0.stride(0)
    if Kp % 4 or Kp < K0 or lds < 2 * Kp or ldv < VK or ldv % 4 or lds % 4 or venc.data_ptr() % 16 or S0.data_ptr() % 16:
        return False
    return bool(ldv * 4 <= 16383 and lds * 4 <= 16383 and N * ldv * 4 < lim and N * lds * 4 < lim and N * 2 * H * 4 < lim)


def l0_node_fwd_mfma(venc, VK, S0, K0, Kp, WP, row_split, bias, slope, N, H, h1, P, mask=None, rows=None, prefix=0):
    """``l0_node_fwd`` for every embedding table in ONE launch on the matrix pipe (``dmp_l0_node_fwd_mfma``): ``WP`` [tables, ..,
    3H] the packed matrices (``l0_node_pack``), a row below ``row_split`` taking the first; ``rows`` = ``NodeRows.rows`` (the kept
    nodes over all N, whose first ``prefix`` entries are 0 .. prefix-1; None: every row), ``mask``: the nodes whose ``P`` rows are
    written as zeros where their bit is 0.  A node outside ``rows`` is not read and its ``h1`` row stays unwritten."""
    lib = _lib.load()
    WP = WP if WP.dim() == 3 else WP.unsqueeze(0)
    lst, cnt = rows if rows is not None else (None, None)
    K = VK + 2 * K0
    # (the host knows the kept rows only as far as the prefix: under a mask the count is what the launch moves at least -- every
    # node's P row, zeros or not, and the prefix's code and H1n rows)
    known = N if lst is None else min(int(prefix), N)
    nbytes = 4 * (H + K) * known + (8 * H * N if (mask is not None or lst is None) else 8 * H * known) + (N // 8 if mask is not None else 0)
    with _lib.timed("l0_node_mfma[K=%d,N=%d,kept>=%d]", (K, N, known), nbytes):
        check(lib.dmp_l0_node_fwd_mfma(ptr(venc), venc.stride(0), VK, ptr(S0), S0.stride(0), K0, Kp, ptr(WP), WP.stride(1), WP.stride(0),
                                       WP.size(0), int(row_split), ptr(bias), float(slope), ptr(mask), ptr(lst), ptr(cnt),
                                       0 if lst is None else lst.numel(), 0 if lst is None else min(int(prefix), N, lst.numel()), N, H,
                                       ptr(h1), h1.stride(0), ptr(P), P.stride(0), stream_ptr()), "dmp_l0_node_fwd_mfma")


def l0_node_bwd_ok(H, VK, K0, Kp, tables, vtables, N, venc, S0, dXP, dxn=None, exact_fp32=None):
    """Whether ``l0_node_codes_bwd`` takes the K-column products of a first layer's node side backward (else ``smallk_atb_jobs`` and
    ``smallk_atb_cols``): the forward's condition, one venc table or one per table of S0, and gradient rows of whole 8 bytes
    that the descriptors address."""
    if not l0_node_mfma_ok(H, VK, K0, Kp, tables, N, venc, S0, exact_fp32) or vtables < 1 or vtables > tables or dXP is None:
        return False
    lim = (1 << 32) - 65536
    for d, cols in ((dXP, 3 * H), (dxn, H)):
        if d is None:
            continue
        ld = d.stride(0)
        if d.stride(1) != 1 or d.size(1) < cols or ld % 2 or d.data_ptr() % 8 or ld * 4 > 16383 or N * ld * 4 >= lim:
            return False
    return True


def l0_node_codes_bwd(venc, VK, vtables, S0, K0, Kp, tables, row_split, dXP, dxn, N, H, Xn, Yn, rows=None, prefix=0):
    """``Xn[h, t K0 : (t+1) K0] = S0_h^T dXP[:, :H]`` per table and ``Yn[b, tv VK : (tv+1) VK] = venc^T (block b of [dXP | dxn])``
    over the kept rows in ONE launch on the matrix pipe (``dmp_l0_node_codes_bwd``); the workgroups' partials join the deferred
    reduction (``reduce_partials``): a fixed order, no atomics.  ``rows`` / ``prefix`` as for ``l0_node_fwd_mfma``."""
    lib = _lib.load()
    lst, cnt = rows if rows is not None else (None, None)
    bound = N if lst is None else min(lst.numel(), N)
    G = int(lib.dmp_l0_node_codes_bwd_blocks(bound))
    nblk = 3 if dxn is None else 4
    partX = torch.empty((G, 2 * tables * K0 * H), dtype=torch.float32, device=dXP.device)
    partY = torch.empty((G, nblk * vtables * VK * H), dtype=torch.float32, device=dXP.device)
    known = N if lst is None else min(int(prefix), N)
    with _lib.timed("l0_node_bwd[K=%d,N=%d,kept>=%d]", (VK + 2 * K0, N, known),
                    4 * (nblk * H + VK + 2 * K0) * known + 4 * (partX.numel() + partY.numel())):
        check(lib.dmp_l0_node_codes_bwd(ptr(venc), venc.stride(0), VK, vtables, ptr(S0), S0.stride(0), K0, Kp, tables, int(row_split),
                                        ptr(dXP), dXP.stride(0), ptr(dxn), 0 if dxn is None else dxn.stride(0), ptr(lst), ptr(cnt),
                                        0 if lst is None else lst.numel(), 0 if lst is None else min(int(prefix), N, lst.numel()), N, H,
                                        ptr(partX), ptr(partY), stream_ptr()), "dmp_l0_node_codes_bwd")
    reduce_partials(partX, Xn.view(-1))
    reduce_partials(partY, Yn.view(-1))
    return Xn, Yn


def l0_edge_fwd(enc, K, M, P, ldp, bias, coef, index, slope=0.0, rows=None, out=None, mask=None, mlp=None):
    """``act(enc M[:, :H] + coef[dst] enc M[:, H:] + P[a, 0:H] - P[b, H:2H] + bias)`` -- ``edge_fwd_typed`` for input rows
    ``enc W`` of rank K with ``M = W Wes``: no class tiles, rows in their own order.  ``rows = (r0, r1)``: only that range
    of the edge rows (written into ``out[r0:r1]``): rows of another embedding table take another ``M``.  ``mask`` (a
    ``gate_row_mask`` over all E rows): its zero bits mark DEAD output rows, left out entirely.
    ``mlp``: the layer's second Linear rides in the same launch (``dmp_l0_edge_mlp_fwd``, see ``out_fwd_typed_codes(first=...)``):
    ``M`` then holds the ``mlp["tables"]`` tables' rows (rows below ``mlp["split"]``: the first table's), the launch walks
    ``mlp["tiles"]`` -- rows outside them are neither read nor written -- and also fills ``mlp["out"]`` (a selector of -1 reads zeros there)."""
    lib = _lib.load()
    E, H = enc.size(0), M.size(1) // 2
    if out is None:
        out = torch.empty((E, H), dtype=torch.float32, device=enc.device)
    r0, r1 = (0, E) if rows is None else rows
    sel_a, sel_b, coef_e = index.edge_select(coef)
    if mlp is not None:
        slot_edge, _, num_tiles, bound = mlp["tiles"]
        W2t, b2, Wc, prev, zn = mlp["W2t"], mlp["b2"], mlp["Wc"], mlp["prev"], mlp["out"]
        tables = int(mlp["tables"])
        split = int(mlp["split"]) if tables == 2 else 0
        _lib.require_gpu(enc, M, P, bias, W2t, b2, Wc, prev, out, zn)
        # (the record form of the first of the launches this one replaces, at the second table's row count: bench.py prices the
        # names it knows at the kept rows)
        with _lib.timed("l0_edge_fwd[K=%d,E=%d]", (K, E - split), 4 * H * (E + min(2 * index.num_nodes, 2 * E)) + (4 * enc.size(1) + 12) * E):
            check(lib.dmp_l0_edge_mlp_fwd(ptr(enc), enc.stride(0), int(K), ptr(M), M.stride(0), tables, split, ptr(P), ldp, index.num_nodes,
                                          ptr(bias), ptr(coef_e), ptr(sel_a), ptr(sel_b), float(slope), ptr(W2t), W2t.stride(0),
                                          int(bool(mlp.get("w_in_out", True))), ptr(b2), ptr(Wc), Wc.stride(0), int(mlp["row0"]), ptr(prev),
                                          prev.stride(0) if prev is not None else H, 0 if prev is None else min(E, prev.size(0)),
                                          ptr(slot_edge), ptr(num_tiles), bound, E, H, ptr(out), out.stride(0), ptr(zn), zn.stride(0),
                                          stream_ptr()), "dmp_l0_edge_mlp_fwd")
        return out
    if mask is not None and r0 % 32 != 0:
        mask = None
    if mask is not None and l0_row_list(r0, r1 - r0):
        lst, cnt = kept_rows(mask, r0, r1)
        with _lib.timed("l0_edge_fwd[K=%d,E=%d]", (K, r1 - r0), 4 * H * (r1 - r0 + min(2 * index.num_nodes, 2 * (r1 - r0))) + (4 * enc.size(1) + 12) * (r1 - r0)):
            check(lib.dmp_l0_edge_fwd_rows(ptr(enc[r0:]), enc.stride(0), K, ptr(M), M.stride(0), ptr(P), ldp, ptr(bias), ptr(coef_e[r0:]),
                                           ptr(sel_a[r0:]), ptr(sel_b[r0:]), ptr(lst), ptr(cnt), r1 - r0, H, slope, ptr(out[r0:]),
                                           out.stride(0), stream_ptr()), "dmp_l0_edge_fwd_rows")
        return out
    with _lib.timed("l0_edge_fwd[K=%d,E=%d]", (K, r1 - r0), 4 * H * (r1 - r0 + min(2 * index.num_nodes, 2 * (r1 - r0))) + (4 * enc.size(1) + 12) * (r1 - r0)):
        check(lib.dmp_l0_edge_fwd_masked(ptr(enc[r0:]), enc.stride(0), K, ptr(M), M.stride(0), ptr(P), ldp, ptr(bias), ptr(coef_e[r0:]),
                                         ptr(sel_a[r0:]), ptr(sel_b[r0:]), None if mask is None else ptr(mask[r0 // 32:]), r1 - r0, H,
                                         slope, ptr(out[r0:]), out.stride(0), stream_ptr()),
              "dmp_l0_edge_fwd")
    return out


def l0_bwd_w(enc, K, coef_e, d_pre, d_zn=None, rows=None, out=None, mask=None):
    """-> ``[enc^T dPre | (coef_e enc)^T dPre (| enc^T dZn)]`` as one [K, 2H or 3H] matrix: one pass over the gradients
    (over the rows ``rows = (r0, r1)`` only; ``out``: where the reduced sums go).  ``mask`` (``code_row_mask(enc, K)``): the
    gradient rows of all-zero code rows are not fetched."""
    lib = _lib.load()
    E, H = d_pre.shape
    r0, r1 = (0, E) if rows is None else rows
    own = False                          # ``mask`` covers the range alone (bit 0 = row r0), not all E rows
    if mask is not None and r0 % 32 != 0:
        # a row range that starts inside a mask word (a ragged pattern batch: the target's rows begin anywhere): the range's own
        # mask from its code rows.  NOT optional: where the layers leave dead rows unwritten (``dead_rows_buffer``) the rows
        # of ``d_pre`` / ``d_zn`` under a zero gate hold garbage -- their code rows are zeros, so this mask leaves them out
        mask, own = code_row_mask(enc[r0:r1], K), True
    nacc = (3 if d_zn is not None else 2) * K
    G = int(lib.dmp_l0_bwd_w_blocks(r1 - r0))
    part = torch.empty((G, nacc * H), dtype=torch.float32, device=d_pre.device)
    if mask is not None and l0_row_list(0 if own else r0, r1 - r0):
        lst, cnt = kept_rows(mask, 0, r1 - r0) if own else kept_rows(mask, r0, r1)
        with _lib.timed("l0_bwd_w[K=%d,E=%d]", (K, r1 - r0), 4 * (H * (2 if d_zn is not None else 1) + enc.size(1) + 1) * (r1 - r0)):
            check(lib.dmp_l0_bwd_w_rows(ptr(enc[r0:]), enc.stride(0), K, ptr(coef_e[r0:]), ptr(d_pre[r0:]), d_pre.stride(0),
                                        ptr(d_zn[r0:]) if d_zn is not None else None, d_zn.stride(0) if d_zn is not None else 0,
                                        ptr(lst), ptr(cnt), r1 - r0, H, ptr(part), stream_ptr()), "dmp_l0_bwd_w_rows")
        return reduce_partials(part, None if out is None else out.view(-1)).view(K, (nacc // K) * H)
    words = None if mask is None else (mask if own else mask[r0 // 32:])
    with _lib.timed("l0_bwd_w[K=%d,E=%d]", (K, r1 - r0), 4 * (H * (2 if d_zn is not None else 1) + enc.size(1) + 1) * (r1 - r0)):
        check(lib.dmp_l0_bwd_w_masked(ptr(enc[r0:]), enc.stride(0), K, ptr(coef_e[r0:]), ptr(d_pre[r0:]), d_pre.stride(0),
                                      ptr(d_zn[r0:]) if d_zn is not None else None, d_zn.stride(0) if d_zn is not None else 0,
                                      ptr(words), r1 - r0, H, ptr(part), stream_ptr()),
              "dmp_l0_bwd_w")
    return reduce_partials(part, None if out is None else out.view(-1)).view(K, (nacc // K) * H)


class Layer0Codes:
    """What the first layer of a rep-net needs INSTEAD of differentiable input rows, when those rows are label embeddings.
    ``enc`` [E, Kpad]: the packed gated label codes of the union's edge rows (``l0_pack``), ``K`` of them per row;
    ``W`` [K, H]: the embedding table (edge rows = ``enc W``), or [2K, H] = the pattern's table over the target's, the
    pattern's rows being the first ``esplit`` edges / ``nsplit`` nodes.  Optionally the same for the node rows:
    ``venc`` [N, Kvpad], ``VK``, ``WV`` [VK or 2 VK, H].
    What ``dmpnn.joint_rep`` may add: ``z_from_codes`` (the target's edge rows are not in memory: ``l0_z_from_codes``) with
    ``z_head`` (the pattern's embedded edge rows), ``enc_mask`` / ``venc_mask`` (``code_row_mask`` of ``enc`` / ``venc``)."""

    def __init__(self, enc, K, W, esplit=0, nsplit=0, venc=None, VK=0, WV=None, z_from_codes=False, z_head=None, enc_mask=None,
                 venc_mask=None):
        self.enc, self.K, self.W, self.esplit, self.nsplit = enc, K, W, esplit, nsplit
        self.venc, self.VK, self.WV = venc, VK, WV
        self.z_from_codes, self.z_head, self.enc_mask, self.venc_mask = z_from_codes, z_head, enc_mask, venc_mask

    def vtables(self, N):
        """-> one ``(table, node rows)`` per table of the node rows' embedding."""
        if self.WV.size(0) == self.VK:
            return [(0, (0, N))]
        return [t for t in ((0, (0, self.nsplit)), (1, (self.nsplit, N))) if t[1][1] > t[1][0]]

    def tables(self, E, N):
        """-> one ``(table, edge rows, node rows)`` per embedding table."""
        if self.W.size(0) == self.K:
            return [(0, (0, E), (0, N))]
        # a table stays in the list while it has edge rows OR node rows (a pattern batch without edges still has nodes, whose
        # aggregates are zero rows): the loops over the list skip the empty range themselves
        return [t for t in ((0, (0, self.esplit), (0, self.nsplit)), (1, (self.esplit, E), (self.nsplit, N)))
                if t[1][1] > t[1][0] or t[2][1] > t[2][0]]


def atb_rows_multi(products, tiles=None):
    """Several ``atb_rows`` products over the SAME rows in ONE launch: ``products`` = list of ``(a, b, gate, colsum[, mask])``
    (a [R, 128 ma], b [R, 128 nb]; ``mask``: a ``gate_row_mask`` whose zero bits mark rows where ``gate (.) a`` or ``b`` is
    known to be all zeros: not fetched); returns a list of ``(a^T b  [128 ma, 128 nb], column sums or None)``.  The launch's
    workgroups are shared by all 128 x 128 output blocks, so short inputs (the node side: R = nodes) get long
    tile ranges per workgroup instead of paying every workgroup's fixed costs once per product.
    ``tiles`` (``NodeRows.tiles``): the products run over that tile list (rows gathered by slot: the kept nodes of a 0 / 1 node
    gate) instead of all rows -- jobs then carry neither gates, column sums nor masks: the list says which rows take part."""
    lib = _lib.load()
    R = products[0][0].size(0)
    products = [tuple(pr) + (None,) * (5 - len(pr)) for pr in products]
    if (tiles is not None and all(gate is None and not colsum and mask is None for _, _, gate, colsum, mask in products)
            and all(a.size(1) % 128 == 0 and b.size(1) % 128 == 0 and atb2_ok(a, b, 128) for a, b, _, _, _ in products)):
        # over a tile list: 128 x 128 output blocks as jobs of ``dmp_atb2_jobs`` (at most 6 per launch), every product's blocks
        # written into ONE partial of its own shape, so that one fixed-order reduction per product gives the [M, N] result
        blocks = [(pi, ia, ib) for pi, (a, b, _, _, _) in enumerate(products) for ia in range(a.size(1) // 128) for ib in range(b.size(1) // 128)]
        slot, tile_scale, num_tiles, bound = tiles
        res = []
        for i0 in range(0, len(blocks), 6):
            chunk = blocks[i0:i0 + 6]
            G = int(lib.dmp_atb2_blocks(bound, len(chunk)))
            jobs2 = (_abi.dmp_atb2_job * len(chunk))()
            parts2 = {}
            for j, (pi, ia, ib) in enumerate(chunk):
                a, b = products[pi][0], products[pi][1]
                M, N = a.size(1), b.size(1)
                if pi not in parts2:
                    parts2[pi] = torch.empty((G, M * N), dtype=torch.float32, device=a.device)
                jobs2[j].Z, jobs2[j].ldz = a.data_ptr() + 4 * 128 * ia, a.stride(0)
                jobs2[j].D, jobs2[j].ldd = b.data_ptr() + 4 * 128 * ib, b.stride(0)
                jobs2[j].partial_T, jobs2[j].partial_B = parts2[pi].data_ptr() + 4 * (ia * 128 * N + ib * 128), None
                jobs2[j].partial_stride, jobs2[j].ldp = M * N, N
            with _lib.timed("atb2[jobs=%d,R=%d]", (len(chunk), R), 8 * 128 * R * len(chunk)):
                check(lib.dmp_atb2_jobs(jobs2, len(chunk), ptr(slot), ptr(tile_scale), ptr(num_tiles), bound, R, 128, stream_ptr()), "dmp_atb2_jobs")
            res.append(parts2)
        out = []
        for pi, (a, b, _, _, _) in enumerate(products):
            hold = [r_[pi] for r_ in res if pi in r_]
            if len(hold) != 1:      # (a product whose blocks fell into two launches: not with <= 6 blocks; kept simple)
                raise _lib.DmpError("atb_rows_multi(tiles=...): a product's blocks must share one launch")
            out.append((reduce_partials(hold[0]).view(a.size(1), b.size(1)), None))
        return out
    blk = min(atb_block(a.size(1), b.size(1)) for a, b, _, _, _ in products)     # one block size per launch
    nblk = sum((a.size(1) // blk) * (b.size(1) // blk) for a, b, _, _, _ in products)
    if nblk > _abi.DMP_ATB_MAX_JOBS:
        raise ValueError("atb_rows_multi: more than %d output blocks" % _abi.DMP_ATB_MAX_JOBS)
    if tiles is not None and any(gate is not None or colsum or mask is not None for _, _, gate, colsum, mask in products):
        raise _lib.DmpError("atb_rows_multi(tiles=...): jobs without gate, column sums or mask")
    G = int(lib.dmp_atb_tile_jobs_blocks(tiles[3], nblk, blk)) if tiles is not None else int(lib.dmp_atb_jobs_blocks_h(R, nblk, blk))
    jobs = (_abi.dmp_atb_job * nblk)()
    parts, k = [], 0
    for a, b, gate, colsum, mask in products:
        M, N = a.size(1), b.size(1)
        part = torch.empty((G, M * N), dtype=torch.float32, device=a.device)
        part_cs = torch.empty((G, M), dtype=torch.float32, device=a.device) if colsum else None
        parts.append((part, part_cs, M, N))
        for ia in range(M // blk):
            for ib in range(N // blk):
                j = jobs[k]
                j.A, j.lda, j.B, j.ldb = a.data_ptr() + 4 * blk * ia, a.stride(0), b.data_ptr() + 4 * blk * ib, b.stride(0)
                j.gate = ptr(gate)
                j.rowmask = ptr(mask)
                j.partial, j.partial_stride, j.ldp = part.data_ptr() + 4 * (ia * blk * N + ib * blk), M * N, N
                j.partial_colsum = (part_cs.data_ptr() + 4 * blk * ia) if (colsum and ib == 0) else None
                j.cs_ld = M
                k += 1
    with _lib.timed("atb_rows_multi[blocks=%d,R=%d]", (nblk, R), 0):
        if tiles is not None:
            check(lib.dmp_atb_rows_jobs_h(jobs, nblk, R, blk, ptr(tiles[0]), ptr(tiles[1]), ptr(tiles[2]), tiles[3], stream_ptr()),
                  "dmp_atb_rows_jobs_h")
        else:
            check(lib.dmp_atb_rows_jobs_h(jobs, nblk, R, blk, None, None, None, 0, stream_ptr()), "dmp_atb_rows_jobs_h")
    return [(reduce_partials(part).view(M, N), (reduce_partials(part_cs) if part_cs is not None else None))
            for part, part_cs, M, N in parts]


def atb_block(M, N):
    """Output block size of the MFMA weight-gradient kernel for an [M, N] product: 128, 64 or 0 (not taken)."""
    if M % 128 == 0 and N % 128 == 0:
        return 128
    return 64 if (M % 64 == 0 and N % 64 == 0 and 64 in MFMA_WIDTHS) else 0


def atb_ok(a, b):
    """The MFMA weight-gradient kernel takes this product (else: ``atb``, batched library GEMMs)."""
    return (a.is_cuda and a.dtype == torch.float32 and atb_block(a.size(1), b.size(1)) > 0 and a.size(0) >= 4096
            and a.stride(1) == 1 and b.stride(1) == 1 and a.stride(0) % 4 == 0 and b.stride(0) % 4 == 0
            and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
            and a.size(0) < 2 ** 31 - 64 and max(a.stride(0), b.stride(0)) * 4 <= 16383)   # rows by index: any array size


def bwd_z_mfma(d_g, Wes, d_s, base, coef, index):
    """base + gather_select(d_s) + dPre Wes[:, :H]^T + coef[dst] dPre Wes[:, H:]^T  (dPre = d_g[:, :H]); H=128."""
    lib = _lib.load()
    E, H = d_g.size(0), d_g.size(1) // 2
    out = torch.empty((E, H), dtype=torch.float32, device=d_g.device)
    Wes = Wes.contiguous()
    d_s = d_s.contiguous()
    with _lib.timed("bwd_z_mfma[H=%d,E=%d]", (H, E), 4 * H * E * (3 if base is not None else 2) + 5 * E):
        check(lib.dmp_bwd_z_fused(ptr(d_g), 2 * H, ptr(Wes), Wes.size(1), ptr(d_s), d_s.size(1), index.num_nodes,
                                  ptr(base), H, ptr(index.edge_select(coef)[2]), ptr(index.dst32), ptr(index.rev8),
                                  -1.0, 1.0, E, H, ptr(out), H, stream_ptr()), "dmp_bwd_z_fused")
    return out


# ----------------------------------------------------------------------------- parameter algebra (fold / unfold)
_FOLD_IN = ("nloop_w", "in_w", "out_w", "nbias", "eloop_w", "src_w", "dst_w", "ebias", "nW0", "nb0", "eW0", "eb0")
_FOLD_AUX_IN = ("nW2", "eW2", "eye")          # forward only: no gradient flows through the transposed copies
_FOLD_OUT = ("Bn", "bn", "Wx", "Wes", "be")
_FOLD_AUX_OUT = ("WesT", "nW2t", "eW2t")
_FOLD_GRAD = ("nloop_w", "in_w", "out_w", "nbias", "eloop_w", "src_w", "dst_w", "ebias", "nW0", "eW0")


def _carve(buf, shapes):
    out, off = [], 0
    for shp in shapes:
        n = 1
        for d in shp:
            n *= d
        out.append(buf[off:off + n].view(shp))
        off += n
    return out


_EYE = {}


class _FoldLayers(torch.autograd.Function):
    """The first MLP Linear of every layer folded into its projections (see include/dmp_hip.h,
    ``dmp_fold_layers``): one launch forward, two backward, for all layers -- instead of a dozen small
    library products, concatenations and additions per layer and direction."""

    @staticmethod
    def forward(ctx, L, *params):
        # per layer: the 12 folded inputs + the two second Linears (nW2, eW2: only their transposes are made here)
        lib = _lib.load()
        params = [p.detach().contiguous() for p in params]
        _lib.require_gpu(*params)
        H = params[0].size(1)
        dev = params[0].device
        eye = _EYE.get((dev.index, H))
        if eye is None:
            eye = _EYE[(dev.index, H)] = torch.eye(H, dtype=torch.float32, device=dev)
        shapes = [(2 * H, H), (H,), (H, 3 * H), (H, 2 * H), (H,), (H, 2 * H), (H, H), (H, H)]
        per = sum(a[0] * (a[1] if len(a) > 1 else 1) for a in shapes)
        buf = torch.empty(L * per, dtype=torch.float32, device=dev)
        W, F, outs, aux = (_abi.dmp_layer_weights * L)(), (_abi.dmp_layer_folded * L)(), [], []
        for l in range(L):
            pl = params[14 * l:14 * l + 14]
            for name, t in zip(_FOLD_IN + _FOLD_AUX_IN, pl + [eye]):
                setattr(W[l], name, ptr(t))
            views = _carve(buf[l * per:(l + 1) * per], shapes)
            for name, t in zip(_FOLD_OUT + _FOLD_AUX_OUT, views):
                setattr(F[l], name, ptr(t))
            outs += views
            aux += views[5:]
        check(lib.dmp_fold_layers(W, F, L, H, stream_ptr()), "dmp_fold_layers")
        ctx.save_for_backward(*params)
        ctx.L, ctx.H, ctx.weights = L, H, W
        ctx.mark_non_differentiable(*aux)
        ctx.set_materialize_grads(False)   # no zero tensors for the (non-differentiable) transposed copies
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        lib = _lib.load()
        params = ctx.saved_tensors
        L, H = ctx.L, ctx.H
        shapes = [(H, H), (H, H), (H, H), (H,), (H, H), (H, H), (H, H), (H,), (H, H), (H, H)]
        per = 8 * H * H + 2 * H
        buf = torch.empty(L * per, dtype=torch.float32, device=params[0].device)
        G, D, out, keep = (_abi.dmp_layer_folded_grads * L)(), (_abi.dmp_layer_weight_grads * L)(), [None], []
        fshapes = [(2 * H, H), (H,), (H, 3 * H), (H, 2 * H), (H,)]
        for l in range(L):
            gl = []
            for g, shp, name in zip(grads[8 * l:8 * l + 5], fshapes, _FOLD_OUT):
                g = torch.zeros(shp, dtype=torch.float32, device=buf.device) if g is None else g.contiguous()
                setattr(G[l], "d" + name, ptr(g))
                gl.append(g)
            keep.append(gl)
            d = _carve(buf[l * per:(l + 1) * per], shapes)
            for name, t in zip(_FOLD_GRAD, d):
                setattr(D[l], name, ptr(t))
            # order of the inputs: nloop, in, out, nbias, eloop, src, dst, ebias, nW0, nb0 (= dbn), eW0, eb0 (= dbe)
            out += d[:9] + [gl[1], d[9], gl[4], None, None]          # + nW2, eW2: nothing flows back through the transposes
        check(lib.dmp_unfold_layers(ctx.weights, G, D, L, H, stream_ptr()), "dmp_unfold_layers")
        return tuple(out)


def _layer_params(layer):
    n0, e0 = layer.nmlp[0], layer.emlp[0]
    return (layer.nloop_weight, layer.in_weight, layer.out_weight, layer.nbias, layer.eloop_weight, layer.src_weight,
            layer.dst_weight, layer.ebias, n0.weight, n0.bias, e0.weight, e0.bias)


def _layer_aux_params(layer):
    return (layer.nmlp[2].weight, layer.emlp[2].weight)


def fold_layers(layers):
    """-> one ``(Bn, bn, Wx, Wes, be, WesT, nW2t, eW2t)`` per layer (the last three: transposed copies without
    gradient, the layouts the kernels read coalesced).  H = 128 / 64 on the GPU: one HIP launch for all layers (and two for
    their backward); otherwise the same algebra in differentiable torch ops."""
    layers = list(layers)
    H = layers[0].nloop_weight.size(1)
    if H in MFMA_WIDTHS and layers[0].nloop_weight.is_cuda and all(l.nloop_weight.size(1) == H for l in layers):
        flat = _FoldLayers.apply(len(layers), *[p for l in layers for p in _layer_params(l) + _layer_aux_params(l)])
        return [tuple(flat[8 * i:8 * i + 8]) for i in range(len(layers))]
    out = []
    for l in layers:
        nloop, in_w, out_w, nbias, eloop, src_w, dst_w, ebias, nW0, nb0, eW0, eb0 = _layer_params(l)
        Cn = torch.cat([nloop, in_w, out_w, nbias.unsqueeze(0)], dim=0) @ nW0.t()               # [3H+1, H]
        Ce = torch.cat([eloop, src_w - dst_w, dst_w, src_w, ebias.unsqueeze(0)], dim=0) @ eW0.t()  # [4H+1, H]
        Wes = torch.cat([Ce[:H], Ce[H:2 * H]], dim=1)
        nW2, eW2 = _layer_aux_params(l)
        with torch.no_grad():
            aux = (torch.cat([Wes[:, :H].t(), Wes[:, H:].t()], dim=1), nW2.t().contiguous(), eW2.t().contiguous())
        out.append((Cn[H:3 * H], Cn[3 * H] + nb0, torch.cat([Cn[:H], Ce[2 * H:3 * H], Ce[3 * H:4 * H]], dim=1),
                    Wes, Ce[4 * H] + eb0) + aux)
    return out


SMALL_GEMM_MAX_ROWS = 1024     # output rows up to which a product goes into the small-product launch (latency-oriented: a column per thread)


def small_gemm_jobs(jobs):
    """Several small fp32 products in ONE launch (``dmp_small_gemm_jobs``, csrc/dmp_fold.hip).  ``jobs``: list of
    ``(out, terms, addend)`` with ``terms`` a list of ``(A, transA, B, transB)`` -- ``out = sum_t op(A_t) op(B_t) (+ addend)``,
    ``op(X) = X^T`` when the flag is set; operands are 2-D fp32 tensors with unit inner stride (any row stride: column slices
    and ``out`` views of wider tensors are fine), ``out`` must not alias an operand.  At most ``DMP_GEMM_MAX_JOBS`` jobs of at most ``DMP_GEMM_MAX_TERMS`` terms."""
    lib = _lib.load()
    if not 0 < len(jobs) <= _abi.DMP_GEMM_MAX_JOBS:
        raise _lib.DmpError("small_gemm_jobs: 1..%d jobs" % _abi.DMP_GEMM_MAX_JOBS)
    J = (_abi.dmp_gemm_job * len(jobs))()

    def ld(t):
        if t.dim() != 2 or t.dtype != torch.float32 or (t.size(1) > 1 and t.stride(1) != 1):
            raise _lib.DmpError("small_gemm_jobs: 2-D fp32 operands with unit inner stride")
        return t.stride(0) if t.size(0) > 1 else max(t.size(1), 1)

    keep = []
    for n, (out, terms, addend) in enumerate(jobs):
        M, N = out.shape
        if not 0 < len(terms) <= _abi.DMP_GEMM_MAX_TERMS:
            raise _lib.DmpError("small_gemm_jobs: 1..%d terms per job" % _abi.DMP_GEMM_MAX_TERMS)
        _lib.require_gpu(out, addend, *[x for tm in terms for x in (tm[0], tm[2])])
        for q, (A, ta, B, tb) in enumerate(terms):
            K = A.size(0) if ta else A.size(1)
            if (A.size(1) if ta else A.size(0)) != M or (B.size(1) if tb else B.size(0)) != K or (B.size(0) if tb else B.size(1)) != N:
                raise _lib.DmpError("small_gemm_jobs: shapes of job %d, term %d" % (n, q))
            T = J[n].term[q]
            T.A, T.lda, T.B, T.ldb, T.transA, T.transB, T.K = A.data_ptr(), ld(A), B.data_ptr(), ld(B), int(bool(ta)), int(bool(tb)), K
            keep.append((A, B))
        J[n].num_terms, J[n].M, J[n].N, J[n].C, J[n].ldc = len(terms), M, N, out.data_ptr(), ld(out)
        if addend is not None:
            if addend.shape != out.shape:
                raise _lib.DmpError("small_gemm_jobs: addend shape")
            J[n].C0, J[n].ldc0 = addend.data_ptr(), ld(addend)
    check(lib.dmp_small_gemm_jobs(J, len(jobs), stream_ptr()), "dmp_small_gemm_jobs")


# ----------------------------------------------------------------------------- the fused layer: one call's facts, then its stages
class _LayerCall:
    """The immutable facts of one call of the fused layer, built once in ``_FusedDMPLayer.forward`` and kept on ``ctx``: what the
    stages of both passes read and none of them writes.  What a stage MAKES travels through its arguments and its return value."""
    __slots__ = ("index", "coef", "residual", "H", "N", "slope", "inner", "v_gate", "e_gate", "Bn", "bn", "Wx", "Wes", "be",
                 "nW2", "nb2", "eW2", "eb2", "WesT", "nW2t", "eW2t", "l0", "W0", "WV0", "nd", "vpool", "epool", "poolalg")

    def __init__(self, **facts):
        for name in self.__slots__:
            setattr(self, name, facts[name])


# ---- forward stages, in the order ``_FusedDMPLayer.forward`` runs them
def _kept_nodes(index, H, v_gate, l0):
    """Stage: the nodes a 0 / 1 node gate keeps (``node_rows``), or None.  A node under a zero of a gate whose maker wiped the input
    rows is a zero row in every layer, so its aggregate, its projections, its update and all of its gradient rows are dead -- the
    node side runs on the kept nodes' tiles, the edge kernels read a dead node's (unwritten) rows as zeros."""
    side.wait("nodes")      # (index builds issued ahead on the side stream, dmpnn.prefetch_joint_indexes: wait for a stage at its first use)
    return node_rows(index, v_gate, H) if kept_node_path(index, H, v_gate, l0) else None


def _xn_buffer(c, device):
    """The node rows a layer hands out under ``c.nd``.  An INNER layer's xn is read by the next layer of this rep-net only, under the
    same gate: the dead rows stay unwritten; the last layer's rows go to the caller: zeros there."""
    return dead_rows_buffer((c.N, c.H), device) if (c.inner & 1) else torch.zeros((c.N, c.H), dtype=torch.float32, device=device)


def _l0_param_products(c, node_pass, device):
    """The parameter-only products of a first layer on the label codes in ONE launch: W0 Bn_in, W0 Bn_out, W0 [A | B], WV0 Wx
    -> ``(M0, WP, WB, MV)``: ``WP`` with the node pass, ``WB`` (and, with node codes, ``MV``) without."""
    l0, W0, WV0, H, Bn, Wx = c.l0, c.W0, c.WV0, c.H, c.Bn, c.Wx
    K0, TK = l0.K, W0.size(0)
    M0 = torch.empty((TK, 2 * H), dtype=torch.float32, device=device)
    jobs = [(M0, [(W0, False, c.Wes, False)], None)]
    WP = WB = MV = None
    if node_pass:
        # ... written straight into the node pass's packed matrix, one per embedding table: rows 0 .. VK-1 = WV0 Wx (three
        # column blocks), then K0 rows W0 Bn_in and K0 rows W0 Bn_out in the first block; zeros elsewhere
        VK = l0.VK
        WP = torch.zeros((TK // K0, L0_NODE_MAX_COLS, 3 * H), dtype=torch.float32, device=device)
        for t in range(TK // K0):
            WVt = WV0 if WV0.size(0) == VK else WV0[t * VK:(t + 1) * VK]
            jobs += [(WP[t, :VK], [(WVt, False, Wx, False)], None),
                     (WP[t, VK:VK + K0, :H], [(W0[t * K0:(t + 1) * K0], False, Bn[:H], False)], None),
                     (WP[t, VK + K0:VK + 2 * K0, :H], [(W0[t * K0:(t + 1) * K0], False, Bn[H:], False)], None)]
    else:
        WB = torch.empty((2, TK, H), dtype=torch.float32, device=device)
        jobs += [(WB[0], [(W0, False, Bn[:H], False)], None), (WB[1], [(W0, False, Bn[H:], False)], None)]
        if l0.venc is not None:
            MV = torch.empty((WV0.size(0), 3 * H), dtype=torch.float32, device=device)
            jobs.append((MV, [(WV0, False, Wx, False)], None))
    small_gemm_jobs(jobs)
    return M0, WP, WB, MV


def _node_first_codes(c, x, z):
    """Stage, codes variant (dmpnn.py:113,121,125 + fn.sum + 129-136): the node side of a first layer on the label codes up to
    ``H1n`` and the gathered projections -> ``(S0, M0, tables, H1n, P, ldp)``.  Sum of z over a node's edges = (sum of the label
    codes) W0:  S = [S0_in W0 | S0_out W0] is never built,  S Bn = S0_in (W0 Bn_in) + S0_out (W0 Bn_out), two K-column products."""
    l0, nd, H, N, W0 = c.l0, c.nd, c.H, c.N, c.W0
    enc0, K0 = l0.enc, l0.K
    tables = l0.tables(z.size(0), N)
    if nd is not None and enc0.size(1) % 4 == 0:
        # (the code sums of the kept nodes only: every reader -- the node pass over the kept list, the backward's masked
        # K-column products -- leaves the dead nodes' rows out)
        S0 = ops.seg_sum_raw(enc0, c.index.in_ptr, c.index.in_ent, N, None, True, -1.0, 1.0,
                             out=dead_rows_buffer((N, 2 * enc0.size(1)), z.device), rows=nd.rows, tag="seg_sum2_codes")
    else:
        S0 = ops.seg_sum_raw(enc0, c.index.in_ptr, c.index.in_ent, N, None, True, -1.0, 1.0)    # [N, 2 Kpad] = [in | out]
    Kp = enc0.size(1)
    node_pass = (l0.venc is not None and H in MFMA_WIDTHS and l0.VK + 2 * K0 <= L0_NODE_MAX_COLS and W0.size(0) // K0 <= 2)
    M0, WP, WB, MV = _l0_param_products(c, node_pass, z.device)
    if node_pass:
        # the whole node side before the second Linear in ONE pass over the codes: H1n and the two projection blocks
        # (the kept nodes' H1n rows only; a dead node's projection rows are zeros)
        H1n = dead_rows_buffer((N, H), z.device) if nd is not None else torch.empty((N, H), dtype=torch.float32, device=z.device)
        PX = torch.empty((N, 2 * H), dtype=torch.float32, device=z.device)      # the gathered projections [P_dst | P_src]
        # (a node gate WITHOUT the kept-node path -- DMP_ROW_MASKS=0, fewer than 4,096 nodes -- keeps the launch per table: there the
        # step's gradients moved by 1e-4 of their largest entry under a last-bit change of P's kept rows, docs/HISTORY.md (ss))
        if (nd is not None or c.v_gate is None) and l0_node_mfma_ok(H, l0.VK, K0, Kp, WP.size(0), N, l0.venc, S0):
            # ... every table's rows in one launch on the matrix pipe (the kept nodes' tiles; a row below the split: the first table)
            l0_node_fwd_mfma(l0.venc, l0.VK, S0, K0, Kp, WP, l0.nsplit if WP.size(0) == 2 else N, c.bn, c.slope, N, H, H1n, PX,
                             mask=None if nd is None else nd.mask, rows=None if nd is None else nd.rows,
                             prefix=0 if nd is None else nd.prefix)
            return S0, M0, tables, H1n, PX, 2 * H
        for t, _, (n0, n1) in tables:
            if n1 > n0 and (nd is None or n1 <= nd.prefix):      # (no gate, or the pattern's nodes -- all kept: every row)
                l0_node_fwd(l0.venc, l0.VK, S0, K0, Kp, WP[t], c.bn, c.slope, None, n0, n1, H, H1n, PX)
            elif n1 > n0:
                l0_node_fwd(l0.venc, l0.VK, S0, K0, Kp, WP[t], c.bn, c.slope, nd.mask, n0, n1, H, H1n, PX, rows=nd.rows,
                            q_begin=min(nd.prefix, n0))
        return S0, M0, tables, H1n, PX, 2 * H
    SB = torch.empty((N, H), dtype=torch.float32, device=z.device)
    for t, _, (n0, n1) in tables:      # (N-row products: the small-product kernel is built for a few hundred rows)
        if n1 > n0:
            torch.mm(S0[n0:n1, :K0], WB[0, t * K0:(t + 1) * K0], out=SB[n0:n1])
            SB[n0:n1].addmm_(S0[n0:n1, Kp:Kp + K0], WB[1, t * K0:(t + 1) * K0])
    if l0.venc is not None:     # x Wx = venc (WV0 Wx): three column blocks of K-column products
        VK = l0.VK
        XP = torch.empty((N, 3 * H), dtype=torch.float32, device=z.device)
        for t, (n0, n1) in l0.vtables(N):
            smallk_embed(l0.venc[n0:n1, :VK], MV[t * VK:(t + 1) * VK], None, XP[n0:n1], H)
    else:
        XP = x @ c.Wx
    return S0, M0, tables, add_bias_relu_(SB, XP[:, :H], c.bn, c.slope), XP[:, H:], 3 * H


def _node_first_rows(c, x, z):
    """Stage, rows variant (dmpnn.py:113,121,125 + fn.sum + 129-136): ``S`` over the (kept) CSR, then the node side up to ``H1n`` and
    the gathered projections -> ``(S, H1n, P, ldp, xn, chain_panels)``; the last two only where the kept-node chain ran, which
    makes ``xn`` in the same launch."""
    nd, H, N, Bn, Wx, e_gate = c.nd, c.H, c.N, c.Bn, c.Wx, c.e_gate
    # (input rows under a zero of a gate whose maker wiped them -- ``zero_rows_gate`` -- are zeros: not fetched)
    side.wait("keepcsr")
    kc = keep_in_csr(c.index, e_gate) if zero_rows_gate(e_gate) else None
    if kc is not None and nd is not None:   # ... and over the kept NODES' rows only: the others' aggregates are dead
        # (measured twice -- before and after the remap fix of finding (u): row pointers by list position,
        # ``NodeRows.kept_incidence(in_only=True)``, one dependent load less per row group, leave the launch where it is)
        S = ops.seg_sum_raw(z, kc[0], kc[1], N, None, True, -1.0, 1.0, out=dead_rows_buffer((N, 2 * H), z.device), rows=nd.rows)
    elif kc is not None:      # the CSR over the kept edges: the plain kernel, no entries of skipped rows in its stream
        S = ops.seg_sum_raw(z, kc[0], kc[1], N, None, True, -1.0, 1.0)
    else:
        S = ops.seg_sum_raw(z, c.index.in_ptr, c.index.in_ent, N, e_gate.reshape(-1) if zero_rows_gate(e_gate) else None, True, -1.0, 1.0)
    if nd is None:
        SB = S @ Bn
        XP = x @ Wx
        return S, add_bias_relu_(SB, XP[:, :H], c.bn, c.slope), XP[:, H:], 3 * H, None, None
    # the node side on the kept nodes' tiles (the tile kernel with a plain panel, 128-wide block products; independent
    # products share a launch): H1n = act(x Wx0 + S_in Bn_in + S_out Bn_out + bn) as two partial products + a third
    # that adds them up, the two gathered projection blocks, xn = x + (H1n W2^T + b2) -- nothing is read or written
    # for the other nodes
    T = nd.tiles
    H1n = dead_rows_buffer((N, H), z.device)
    if node_chain_ok(H, x, S, Bn, Wx, c.nW2):
        # ... as ONE launch: the rows stay in the workgroup, the six panels stream through LDS (csrc/dmp_nodechain.hip) --
        # the partial products x Wx0 + bn and S_in Bn_in never go through memory
        PX = dead_rows_buffer((N, 2 * H), z.device)      # [P_dst | P_src]
        xn = _xn_buffer(c, z.device)
        chain_panels = node_chain_panels(Bn, Wx, c.nW2)    # (both passes' panels: one launch per layer and step)
        node_chain_fwd(x, S, chain_panels[0], c.bn, c.nb2, c.residual, c.slope, T, H1n, PX, xn)
        return S, H1n, PX, 2 * H, xn, chain_panels
    XP = dead_rows_buffer((N, 3 * H), z.device)          # [x Wx0 + bn (a partial) | P_dst | P_src]
    T1 = dead_rows_buffer((N, H), z.device)
    typed_jobs([dict(a=x, W=Wx[:, :H], bias=c.bn, out=XP[:, :H]), dict(a=S[:, :H], W=Bn[:H], out=T1),
                dict(a=x, W=Wx[:, H:2 * H], out=XP[:, H:2 * H]), dict(a=x, W=Wx[:, 2 * H:], out=XP[:, 2 * H:])], T)
    out_fwd_typed(S[:, H:], Bn[H:], None, XP[:, :H], T, out=H1n, slope=c.slope, prev2=T1)
    return S, H1n, XP[:, H:], 3 * H, None, None


def _node_out(c, x, H1n):
    """Stage (dmpnn.py:137-140): the node side's second Linear + gate + residual -> ``xn`` (where the chain did not make it)."""
    prev = x if c.residual else None
    if c.nd is not None:
        xn = _xn_buffer(c, x.device)
        if c.nW2t is not None:
            return out_fwd_typed(H1n, c.nW2t, c.nb2, prev, c.nd.tiles, out=xn)
        return out_fwd_typed(H1n, c.nW2, c.nb2, prev, c.nd.tiles, out=xn, w_in_out=False)
    if onepanel_ok(c.H):   # Linear + gate + residual in one fused MFMA kernel, as on the edge side
        return out_fwd_mfma(H1n, c.nW2, c.nb2, c.v_gate, prev, c.nW2t)
    return gate_residual(prev, torch.addmm(c.nb2, H1n, c.nW2.t()), c.v_gate)


def _dead_edge_rows_of(c):
    """``(dead_gate, dead)`` of the edge side's forward: the gate whose zeros mark dead rows of H1e (the two producers of H1e leave
    them out), or None; and what is dead beside them -- 0: nothing, 1: z's rows under the gate's zeros (a gate whose maker wiped the
    rep-net's input rows, ``zero_rows_gate``: zeros, not fetched), 3: as an INNER layer of a rep-net (the next layer of the same
    rep-net, under the same gate, is the only reader of zn) the output's zero rows as well: not stored either."""
    dead_gate = c.e_gate if dead_h1_rows(c.index, c.H, c.e_gate) else None
    dead_in = dead_gate is not None and dead_edge_rows(c.index, c.H, c.e_gate)
    return dead_gate, (3 if (c.inner & 1) else 1) if dead_in else 0


def _residual_from_codes(c, H1e):
    """The target's residual rows z = enc W0 are not in memory at all (``dmpnn.joint_rep`` did not make them): the second Linear adds
    them as one more k-group over their codes (``out_fwd_typed_codes``); the pattern's few rows (their own table) come in as the
    residual operand."""
    l0 = c.l0
    return bool(l0 is not None and c.residual and l0.z_from_codes and out_codes_ok(H1e, l0.enc, l0.K, c.W0[-l0.K:]))


def _edge_out_tiles(c, like, dead, codes):
    """The launch of the edge side's second Linear, decided ONCE (by whichever stage issues it): the tile list it walks, or None --
    ``out_fwd_mfma`` over all rows.  With ``dead == 3`` nothing is written for the rows under a zero gate: the kept edges' class
    tiles (``live_tiles``: the first Linear, where it rides in the launch, needs the class scale per tile; a launch with a plain
    panel needs no class and walks ``ascending_tiles(c.e_gate) or`` these).  Without any gate (the all-rows step) a first layer whose
    residual comes from the ``codes``: the same launch over the identity tile list.  ``like``: any tensor of the edge rows."""
    if dead == 3 and c.eW2t is not None:
        lt = live_tiles(c.index, c.coef, c.e_gate)
        if lt is not None:
            return lt
    if codes and c.e_gate is None and c.eW2t is not None:
        return identity_tiles(like.size(0), like.device)
    return None


def _edge_first_codes(c, z, M0, tables, P, ldp, sums_only):
    """Stage, codes variant (dmpnn.py:112,120,124 + 142-152): the edge side's first Linear from the label codes -> ``(H1e, zn)``;
    ``zn`` is None unless the second Linear's launch took the first along."""
    l0, H, W0 = c.l0, c.H, c.W0
    enc0, K0 = l0.enc, l0.K
    side.wait("erows")      # (a layer on the label codes needs the tiles only for its second Linear)
    dead_gate, dead = _dead_edge_rows_of(c)
    H1e = dead_rows_buffer((z.size(0), H), z.device) if dead_gate is not None else torch.empty((z.size(0), H), dtype=torch.float32, device=z.device)
    # the one-launch edge MLP stands exactly where the route is l0_edge_fwd per table + out_fwd_typed_codes (``_edge_out``): over the
    # kept edges' tiles under the gates (whose zero rows are dead rows of H1e: the per-table launches leave them out as well,
    # where their mask starts at a whole word), over the identity tiles without a gate
    # (212 against 275 us for the launches of their own; the first build was time-neutral here: docs/HISTORY.md (oo))
    codes = _residual_from_codes(c, H1e)
    if (codes and not sums_only and c.eW2t is not None
            and l0_edge_mlp_ok(H, K0, W0.size(0) // K0, enc0, P, c.eW2t, l0.z_head)):
        if dead == 3:
            side.wait("tiles")
        tiles = _edge_out_tiles(c, H1e, dead, codes)
        if tiles is not None:
            # both Linears as ONE launch: H1e goes from the first to the second on the chip, the code rows are fetched once
            # (through the second Linear's wrapper, as every E-row Linear + residual launch goes: it fills H1e on the way)
            zn = out_fwd_typed_codes(H1e, c.eW2t, c.eb2, enc0, K0, W0[-K0:], ascending_tiles(c.e_gate) or tiles, prev=l0.z_head,
                                     row0=l0.z_head.size(0),
                                     first=dict(M=M0, tables=W0.size(0) // K0, split=l0.esplit, P=P, ldp=ldp, bias=c.be, coef=c.coef,
                                                index=c.index, slope=c.slope))
            return H1e, zn
    for t, rows, _ in tables:
        if rows[1] > rows[0]:
            l0_edge_fwd(enc0, K0, M0[t * K0:(t + 1) * K0], P, ldp, c.be, c.coef, c.index, c.slope, rows, H1e,
                        mask=gate_row_mask(dead_gate) if dead_gate is not None else None)
    return H1e, None


def _edge_first_rows(c, z, P, ldp, sums_only):
    """Stage, rows variant (dmpnn.py:112,120,124 + 142-152): the edge side's first Linear on the edge rows -> ``(H1e, zn)``; ``zn``
    is None unless the second Linear's launch took the first along -- or the un-typed route made it with the library."""
    H, nd = c.H, c.nd
    side.wait("tiles")
    dead_gate, dead = _dead_edge_rows_of(c)
    sel = None if nd is None else nd.sel
    # the one-launch edge MLP stands exactly where the route is edge_fwd_typed + out_fwd_typed over the kept edges' tiles
    # (``_edge_out`` with dead == 3, live_tiles and the folded W2^T): a gated INNER layer whose edge rows are wanted, with its residual
    if not sums_only and c.residual and edge_mlp_fwd_ok(H, z, P, c.eW2t):
        tiles = _edge_out_tiles(c, z, dead, False)
        if tiles is not None:
            # both Linears over the kept edges' class tiles as ONE launch: H1e goes from the first to the second on the chip
            # (through the second Linear's wrapper, as every E-row Linear + residual launch goes: it fills H1e on the way)
            H1e = dead_rows_buffer((z.size(0), H), z.device)
            zn = out_fwd_typed(H1e, c.eW2t, c.eb2, z, tiles,
                               first=dict(z=z, Wes=c.Wes, P=P, ldp=ldp, bias=c.be, coef=c.coef, index=c.index, slope=c.slope, sel=sel))
            return H1e, zn
    if typed_ok(c.index, H):
        # (under ``nd`` the projection rows of the dead nodes were never written: their selectors read as zeros)
        return edge_fwd_typed(z, c.Wes, P, ldp, c.be, c.coef, c.index, c.slope, dead_gate=dead_gate, sel=sel), None
    G = z @ c.Wes
    H1e = edge_combine_raw(G, 2 * H, P, ldp, c.be, c.coef, c.index, H, relu=True, slope=c.slope)
    del G
    if sums_only:
        return H1e, None
    Oe = torch.addmm(c.eb2, H1e, c.eW2.t())
    return H1e, gate_residual(z if c.residual else None, Oe, c.e_gate)


def _edge_out(c, z, H1e):
    """Stage (dmpnn.py:153-156): the edge side's second Linear + gate + residual -> ``zn``, where no launch has made it yet."""
    l0 = c.l0
    _, dead = _dead_edge_rows_of(c)
    side.wait("tiles")
    codes = _residual_from_codes(c, H1e)
    tiles = _edge_out_tiles(c, H1e, dead, codes)
    if tiles is None:
        return out_fwd_mfma(H1e, c.eW2, c.eb2, c.e_gate, l0_rows(l0, c.W0, z) if c.residual else None, c.eW2t, dead_rows=dead)
    # (a plain panel needs no class: the kept edges' tiles in ascending row order -- ``ascending_tiles``)
    walk = ascending_tiles(c.e_gate) or tiles
    if codes:
        return out_fwd_typed_codes(H1e, c.eW2t, c.eb2, l0.enc, l0.K, c.W0[-l0.K:], walk, prev=l0.z_head, row0=l0.z_head.size(0))
    return out_fwd_typed(H1e, c.eW2t, c.eb2, l0_rows(l0, c.W0, z) if c.residual else None, walk)


def _pooled_outputs(c, z, xn, zn, H1e, sums_only):
    """Stage (the LAST layer under pooling heads): the per-graph sums of both outputs -> ``(vs, es, gcnt)``; ``gcnt``: the gated
    row counts per graph of the row-less form (``sums_only``: no ``zn``), which the backward's db2 needs again."""
    H, epool, e_gate, eW2, eb2 = c.H, c.epool, c.e_gate, c.eW2, c.eb2
    if c.poolalg:       # (``pool_algebra_ok``: the row-less form; the chunk tables the launch reads are this stage's own)
        # the three first-level passes, then ONE launch: their second level, the product with W2 on the non-flagged half
        # (the only one handed out), the bias and the residual term (csrc/dmp_heads.hip)
        vp = c.vpool if (c.vpool is not None and c.vpool.flag8 is None) else None
        partX = pool_chunk_sums(xn, vp) if vp is not None else None
        partH = pool_chunk_sums(H1e, epool, e_gate)
        gcnt = pool_weight_sums(epool, e_gate)
        partZ = pool_chunk_sums(z, epool, e_gate if zero_rows_gate(e_gate) else None) if c.residual else None
        es, vs = pool_out(partH, partZ, epool, gcnt, eW2, eb2, partX, vp)
        if vp is None and c.vpool is not None:
            vs = pool_rows(xn, c.vpool)
        return vs, es, gcnt
    vs = pool_rows(xn, c.vpool) if c.vpool is not None else None
    if not sums_only:
        return vs, (pool_rows(zn, epool) if epool is not None else None), None
    halves = 2 if epool.flag8 is not None else 1
    G_ = epool.num_graphs
    Q = pool_rows(H1e, epool, e_gate).view(G_ * halves, H)                      # sum of g H1 per graph (and flag)
    gcnt = pool_weight_sums(epool, e_gate)                                       # sum of g per graph (and flag)
    cnt = gcnt.view(G_ * halves, 1)
    # (z's rows under a zero of a gate whose maker wiped the input are zeros, and as an inner layer's output not even
    # written: weight 0, not fetched)
    zs = pool_rows(z, epool, e_gate if zero_rows_gate(e_gate) else None).view(G_ * halves, H) if c.residual else None
    if Q.is_contiguous() and eW2.is_contiguous() and Q.size(0) <= SMALL_GEMM_MAX_ROWS:
        es = torch.empty((G_ * halves, H), dtype=torch.float32, device=Q.device)  # Q W2^T + cnt b2 (+ sum of z): one launch
        small_gemm_jobs([(es, [(Q, False, eW2, True), (cnt, False, eb2.view(1, H), False)], zs)])
    else:
        # (thousands of graphs: the small-product kernel is built for a few hundred rows -- 43 us at 4096 rows against
        # 13 for a library product + one row pass)
        es = torch.addmm(zs, Q, eW2.t()) if c.residual else Q @ eW2.t()
        es.addcmul_(cnt, eb2.view(1, H))
    # ... of which only the NON-FLAGGED half is returned ([G, H]): without the rows the backward propagates a gradient
    # through that half only (the row map is -1 for flagged rows), so the flagged sums are not handed out as if they
    # were differentiable (the heads mask reversed edges out and read [:, :H] anyway, basemodel.py:1545-1631)
    return vs, es.view(G_, halves * H)[:, :H], gcnt


# ---- backward stages, in the order ``_FusedDMPLayer.backward`` runs them
def _grad_seeds(c, x, z, H1e, dxn, dzn, dvs, des, typed):
    """Stage: the gradients through the pooled sums (last layer) -> ``(dxn, dzn, lazy)``.  Node side: expanded (N rows are cheap).
    Edge side: if the sums are the ONLY consumer of zn, dzn[e] = T[graph of e] (zero for reversed edges) with T = des[:, :H] and
      dH1 = (g (.) dzn) W2 = g[e] (T W2)[graph of e]             -> no E-row product, no [E, H] gradient tensor
      dW2 = (g (.) dzn)^T H1 = T^T Q,  Q[b] = sum_{e in b} g[e] H1[e]   -> one pooled pass over H1
      db2 = T^T (sum_{e in b} g[e])
    and the residual term of dz reads T through the row map: ``lazy = (T, row map, pool index)``, ``dzn`` stays None."""
    H = c.H
    lazy = None
    if dvs is not None:
        exp = ops.gather_rows_raw(dvs.contiguous(), c.vpool.seg32)
        dxn = exp if dxn is None else dxn + exp
    if des is not None:
        ep = c.epool
        if dzn is None and typed and H1e.size(0) > 0 and des.size(1) == H:
            # des is [G, H]: the row-less forward hands out the non-flagged sums only, or no flag splits the sums.  A
            # [G, 2H] gradient (forward with rows, flag-split sums) may carry a flagged half: the expanded path below
            lazy = (des.contiguous(), pool_rowmap(ep), ep)
        else:
            if ep.flag8 is not None and des.size(1) == H:     # the row-less forward's [G, H]: nothing flows to the flagged rows
                des = torch.cat([des, torch.zeros_like(des)], dim=1)
            exp = (ops.gather_select_raw(des.contiguous(), ep.seg32, ep.flag8, H, None, 1.0, 1.0) if ep.flag8 is not None
                   else ops.gather_rows_raw(des.contiguous(), ep.seg32))
            dzn = exp if dzn is None else dzn + exp
    if dxn is None:
        dxn = torch.zeros_like(x)
    if dzn is None and lazy is None:
        dzn = torch.zeros_like(z)
    return dxn.contiguous(), (dzn.contiguous() if dzn is not None else None), lazy


def l0_tables_full(l0, tables, W0):
    """Every table has edge rows and node rows: every block of the first layer's code products is written."""
    return all(r[1] > r[0] and n[1] > n[0] for _, r, n in tables) and len(tables) * l0.K == W0.size(0)


def l0_codes_buffer(l0, tables, W0, residual, H, device):
    """[TK, 2H or 3H] for ``enc^T [dPre | c dPre (| dzn)]``: a table without edge rows leaves its block to the zeros."""
    return (torch.empty if l0_tables_full(l0, tables, W0) else torch.zeros)((W0.size(0), (3 if residual else 2) * H),
                                                                           dtype=torch.float32, device=device)


def l0_codes_block(c, tables, device, walked):
    """``(XX, codes)`` where ``bwd_h1_w`` takes the last table's code weight gradient along (``h1w_codes_ok``), else None: the
    buffer of ``l0_codes_buffer`` and the ``codes=`` argument that writes the table's block of it."""
    if not h1w_codes_ok(c.l0, tables or (), walked):
        return None
    t, rows, _ = tables[-1]
    XX, K0 = l0_codes_buffer(c.l0, tables, c.W0, c.residual, c.H, device), c.l0.K
    return XX, dict(enc=c.l0.enc, K=K0, coef_e=c.index.edge_select(c.coef)[2], rows=rows, residual=c.residual, out=XX[t * K0:(t + 1) * K0])


def _edge_out_bwd_lazy(c, H1e, lazy, gcnt):
    """The edge side's second Linear backward from the per-graph table alone (``_grad_seeds``) -> ``(dG, dbe, dW2e, db2e)``."""
    H, e_gate = c.H, c.e_gate
    T, emap, ep = lazy
    if c.poolalg:
        # three launches on the per-graph tiles (csrc/dmp_heads.hip): T W2, the one pass over H1e, then both parameter
        # gradients from the pass's chunk sums -- their second level is formed inside, their partials join the layer's reduction
        T = T if _aligned(T) else T.clone(memory_format=torch.contiguous_format)
        skip = c.l0 is None and c.nd is not None and USE_PLAIN_ATB and dead_edge_rows(c.index, H, e_gate, c.coef)
        dG, dbe, qc = pool_relu_bwd(rows_gemm(T, c.eW2, False), emap, e_gate, H1e, ep, c.slope, skip_dead=skip, chunk_sums=True)
        if gcnt is None:
            gcnt = pool_weight_sums(ep, e_gate)
        dW2e, db2e = pool_wgrad(qc, ep, T, gcnt)
        return dG, dbe, dW2e, db2e
    if H % 4 == 0 and H <= 256:
        # (dPre's rows under a zero of a 0 / 1 gate: every reader below leaves them out -- the kept incidence sums,
        # the class-tile kernels over the kept edges' tiles)
        skip = c.l0 is None and c.nd is not None and USE_PLAIN_ATB and dead_edge_rows(c.index, H, e_gate, c.coef)
        dG, dbe, Q = pool_relu_bwd(T @ c.eW2, emap, e_gate, H1e, ep, c.slope, skip_dead=skip)       # dG is dPre; one pass over H1e
        Q = Q[:, :H]
    else:
        dG, dbe = relu_bwd_gathered_colsum(T @ c.eW2, emap, e_gate, H1e, c.slope)
        Q = pool_rows(H1e, ep, e_gate)[:, :H]
    dW2e = T.t() @ Q
    if gcnt is None:        # gated row counts per graph
        gcnt = pool_weight_sums(ep, e_gate)
    return dG, dbe, dW2e, gcnt[:, 0] @ T


def _edge_out_bwd_typed(c, tables, H1e, dzn):
    """The edge side's second Linear backward on the tile / one-panel kernels -> ``(dG, dbe, dW2e, db2e, l0_XX)``.  The gate is
    applied inside the two consumers of dO = gate * dzn (no [E,H] pass of its own).  ``l0_XX``: ``l0_codes_block`` once
    ``bwd_h1_w`` took the last table's code weight gradient along, else None."""
    ix, coef, H, slope, e_gate, eW2 = c.index, c.coef, c.H, c.slope, c.e_gate, c.eW2
    l0_XX = None
    if binary_gate_mask(e_gate) is not None:
        # a 0 / 1 gate: bwd_h1 hands out sum_e g_e dzn[e] (db2) from the rows it fetches anyway, and the weight
        # gradient runs ungated over the masked-in rows on the bf16 pipe
        # (dPre's zero rows are not stored: the class-tile kernels, the scatter-add and the layer-0 products below
        # leave them out)
        skip = USE_MASKED_SUMS and dead_h1_rows(ix, H, e_gate) and (c.l0 is None or c.l0.enc_mask is not None)
        lt = live_tiles(ix, coef, e_gate) if skip else None
        if lt is not None and h1w_ok(dzn, H1e, H):
            # both products of the second Linear's backward from ONE pass over dO and H1 (csrc/dmp_h1w.hip) -- and, in
            # the first layer, the target table's code weight gradient over the same kept rows (``l0_bwd_w``'s launch)
            l0_XX = l0_codes_block(c, tables, dzn.device, "kept")
            dG, dbe, db2e, dW2e = bwd_h1_w(dzn, eW2, H1e, ascending_tiles(e_gate) or lt, slope, codes=l0_XX and l0_XX[1])[:4]
        elif lt is not None:      # over the kept edges' tiles only
            dG, dbe, db2e = bwd_h1_typed(dzn, eW2, H1e, ascending_tiles(e_gate) or lt, slope)
            # dO^T H1 over the kept edges' tiles: the class-tile weight-gradient kernel's first half (its class-scaled
            # second half costs no further products) -- no tiles' worth of zero rows in between
            dW2e = atb_typed(dzn, H1e, coef, ix, gate=e_gate, plain=True)
        else:
            dG, dbe, db2e = bwd_h1_mfma(dzn, eW2, H1e, coef, ix, both_halves=False, gate=e_gate, slope=slope, rows_colsum=True,
                                        skip_dead_stores=skip)
            dW2e = atb_rows(dzn, H1e, e_gate, colsum=False)[0]
        return dG, dbe, dW2e, db2e, l0_XX
    it = identity_tiles(dzn.size(0), dzn.device) if (e_gate is None and h1w_ok(dzn, H1e, H)) else None
    if it is not None:
        # no gate at all (a model without a filter net: the reference's one-label datasets): every row is live --
        # both products of the second Linear's backward in one launch over the identity tile list
        l0_XX = l0_codes_block(c, tables, dzn.device, "all")
        dG, dbe, db2e, dW2e = bwd_h1_w(dzn, eW2, H1e, it, slope, codes=l0_XX and l0_XX[1])[:4]
    else:
        dW2e, db2e = atb_rows(dzn, H1e, e_gate)
        dG, dbe = bwd_h1_mfma(dzn, eW2, H1e, coef, ix, both_halves=False, gate=e_gate, slope=slope)  # dG is dPre
    return dG, dbe, dW2e, db2e, l0_XX


def _edge_out_bwd(c, tables, H1e, dzn, lazy, gcnt, typed):
    """Stage: the edge side, down to the gathered node projections -- the second Linear's backward and the activation's
    -> ``(dG, dbe, dW2e, db2e, l0_XX)``; ``dG[:, :H]`` is dPre."""
    if lazy is not None:
        return _edge_out_bwd_lazy(c, H1e, lazy, gcnt) + (None,)
    if typed:
        return _edge_out_bwd_typed(c, tables, H1e, dzn)
    dOe, db2e = scale_rows_colsum(dzn, c.e_gate)
    dW2e = atb(dOe, H1e)
    dH1e = dOe @ c.eW2
    dG, dbe = relu_bwd_g_colsum(dH1e, H1e, c.coef, c.index.dst32, c.slope)
    return dG, dbe, dW2e, db2e, None


def _endpoint_sums(c, dG, typed, device):
    """Stage: dPre into both endpoints' rows, the backward scatter-add (dPre's rows under a zero edge gate are zeros: not fetched)
    -> ``dXP`` = [dPn | dP] with its last two column blocks written: the node side writes dPn in place, no concatenation (under
    ``c.nd``: the kept nodes' rows only)."""
    ix, H, N, nd, e_gate = c.index, c.H, c.N, c.nd, c.e_gate
    dXP = dead_rows_buffer((N, 3 * H), device) if nd is not None else torch.empty((N, 3 * H), dtype=torch.float32, device=device)
    sums_masked = typed and USE_MASKED_SUMS and has_row_mask(e_gate)
    # (... and the rows of the dead nodes are neither summed nor stored)
    if kept_incidence_sums(ix, H, e_gate, nd is not None):
        # every kept node's two sums over its KEPT edges (the incidence CSR over the kept edges, a row per kept node):
        # the plain segment-sum kernel, ascending edge id -- an edge row without a kept endpoint is never fetched
        kp, ke = nd.kept_incidence(ix, e_gate)
        ops.seg_sum_raw(dG[:, :H], kp, ke, N, None, True, 1.0, -1.0, out=dXP[:, H:], rows=nd.rows, ptr_by_pos=True, tag="seg_sum2_kept_inc",
                        incidence=True)
    else:
        nodes = (nd.mask, nd.sel[:2]) if (nd is not None and sums_masked and ops.graph_seg_ok(ix, dG[:, :H], H, dXP[:, H:])) else None
        ops.endpoint_sums(dG[:, :H], ix, out=dXP[:, H:], mask=gate_row_mask(e_gate) if sums_masked else None,
                          gate=e_gate if sums_masked else None, nodes=nodes)
    return dXP


def _l0_edge_code_products(c, tables, dG, dzn, l0_XX):
    """Stage, codes variant: z = enc W0 -- one pass over dPre (and the residual gradient) on the K-column factor -> ``XX`` =
    enc^T [dPre | c dPre (| dzn)] per table.  (The last table's block may be there already: ``bwd_h1_w(codes=...)`` made it in its
    launch, ``l0_XX``.)"""
    l0, e_gate, K0 = c.l0, c.e_gate, c.l0.K
    XX = l0_XX[0] if l0_XX is not None else l0_codes_buffer(l0, tables, c.W0, c.residual, c.H, dG.device)
    for t, rows, _ in (tables[:-1] if l0_XX is not None else tables):
        if rows[1] > rows[0]:
            # (the rows to add: those with a non-zero code row -- or, where dPre's rows under a zero gate were not
            # stored, the rows the gate keeps: the same list the forward walked; a kept row with a zero code adds zeros)
            l0_bwd_w(l0.enc, K0, c.index.edge_select(c.coef)[2], dG, dzn if c.residual else None, rows, XX[t * K0:(t + 1) * K0],
                     mask=(gate_row_mask(e_gate) if (l0.enc_mask is not None and binary_gate_mask(e_gate) is not None)
                           else l0.enc_mask))
    return XX


def _edge_first_wgrad(c, z, dG, typed, want_dz):
    """Stage, rows variant: the first Linear's weight gradient [H,2H] = [dA_e | dB_e] -- or None: with the input gradient still to
    come (``_edge_input_grad``, over the same tile list) both products of dPre run in ONE launch there, ``bwd_z_w``: decided here,
    made there.  (dG = dPre has zero rows under a zero edge gate, whichever kernel made it: the typed kernels skip those edges.)"""
    ix, H, e_gate = c.index, c.H, c.e_gate
    if typed and want_dz and H == 128 and (e_gate is None or dead_edge_rows(ix, H, e_gate, c.coef)):
        return None
    return atb_typed(z, dG, c.coef, ix, gate=e_gate) if typed else atb(z, dG)


def _wgrad(a, b, kernel):
    """A node-side weight gradient a^T b of its own: the MFMA kernel (``kernel``: ``atb_ok`` of the widest product) or library GEMMs."""
    return atb_rows(a, b, colsum=False)[0] if kernel else atb(a, b)


def _node_one_launch(c, x, S, H1n, dxn, dXP):
    """The node side's weight gradients share one launch (``_node_wgrads``); the kept-node path has no other form."""
    one_launch = onepanel_ok(c.H) and atb_ok(dxn, H1n) and atb_ok(x, dXP) and (S is None or atb_ok(S, dXP))
    if c.nd is not None and not (one_launch and binary_gate_mask(c.v_gate) is not None):
        raise _lib.DmpError("fused layer backward: the kept-node path needs the masked weight-gradient launch")
    return one_launch


def _node_out_bwd(c, dxn, H1n, dXP, own_dW2n, kernel):
    """The node side's second Linear backward and the activation's -> ``(dPn, dbn, db2n, dW2n)``: ``dPn`` is written into
    ``dXP[:, :H]``; ``dW2n`` only with ``own_dW2n`` (else it comes out of ``_node_wgrads``, with ``db2n`` where that is None here)."""
    nd, H, slope, v_gate, nW2 = c.nd, c.H, c.slope, c.v_gate, c.nW2
    dW2n = db2n = None
    if nd is not None:
        # dPn = act'(H1n) (.) (dxn W2) on the kept nodes' tiles; db2n = the column sums of the dxn rows it fetches
        dPn, dbn, db2n = bwd_h1_typed(dxn, nW2, H1n, nd.tiles, slope, out=dXP[:, :H])
        if own_dW2n:
            dW2n = atb_rows(dxn, H1n, v_gate, colsum=False)[0]
    elif onepanel_ok(H) and atb_ok(dxn, H1n):
        # as on the edge side: the node gate lives inside the two consumers of dO = v_gate * dxn
        if binary_gate_mask(v_gate) is not None:
            # a 0 / 1 node gate: db2n from the rows bwd_h1 fetches, the weight gradient(s) ungated over the masked-in rows
            dPn, dbn, db2n = bwd_h1_mfma(dxn, nW2, H1n, both_halves=False, gate=v_gate, out=dXP[:, :H], slope=slope,
                                         rows_colsum=True)
            if own_dW2n:
                dW2n = atb_rows(dxn, H1n, v_gate, colsum=False)[0]
        else:
            if own_dW2n:
                dW2n, db2n = atb_rows(dxn, H1n, v_gate)
            dPn, dbn = bwd_h1_mfma(dxn, nW2, H1n, both_halves=False, gate=v_gate, out=dXP[:, :H], slope=slope)
    else:
        dOn, db2n = scale_rows_colsum(dxn, v_gate)
        dW2n = _wgrad(dOn, H1n, kernel)
        dH1n = dOn @ nW2
        dPn, dbn = relu_bwd_colsum_(dH1n, H1n, out=dXP[:, :H], slope=slope)
    return dPn, dbn, db2n, dW2n


def _node_wgrads(c, products):
    """The node side's weight gradients ``a^T b`` of ``products`` = [(dxn, H1n), (S, dPn) unless on the codes, (x, dXP)] (1 + 2 + 3
    output blocks) in ONE launch -> ``(the gradients, db2n or None)``.  (dPn = act'(H1n) ((v_gate dxn) W2): zero rows under a zero
    node gate -- all products but the last skip them.)"""
    nd, v_gate = c.nd, c.v_gate
    last = products[-1] + (None, False)
    if nd is not None:
        # the products over the kept nodes' tiles (rows gathered by slot): 41 % of the row tiles at bench.py's labels, and
        # nothing of a dead node's (unwritten) rows is touched
        res = atb_rows_multi([(a, b, None, False) for a, b in products], tiles=nd.tiles)
        return [r[0] for r in res], None
    vm = binary_gate_mask(v_gate)
    if vm is not None:    # (db2n came from bwd_h1; no job carries a gate: the launch runs on the bf16 pipe)
        res = atb_rows_multi([(a, b, None, False, vm) for a, b in products[:-1]] + [last])
        return [r[0] for r in res], None
    vm = gate_row_mask(v_gate)
    res = atb_rows_multi([products[0] + (v_gate, True, vm)] + [(a, b, None, False, vm) for a, b in products[1:-1]] + [last])
    return [r[0] for r in res], res[0][1]


def _dx_buffer(c, device):
    """The node input gradient under ``c.nd``.  A dead node's row is multiplied by the gate's zero further down: left unwritten where
    the layer before is the only reader (``inner`` bit 1), zeros for whoever made the first layer's rows."""
    return dead_rows_buffer((c.N, c.H), device) if (c.inner & 2) else torch.zeros((c.N, c.H), dtype=torch.float32, device=device)


def _node_dS(c, dPn, dXP, dxn, want_dx):
    """Rows variant: dS = dPn Bn^T -> ``(dS, dxU)``; ``dxU``: under ``c.nd`` with ``want_dx``, two of the three partial products of
    dx = dxn + dXP Wx^T, made in the same launch (``_node_dx`` adds the third), else None."""
    nd, H, N, Bn, Wx = c.nd, c.H, c.N, c.Bn, c.Wx
    if nd is None:
        return dPn @ Bn.t(), None
    # dS = dPn Bn^T on the kept nodes' tiles; the edge kernel reads a dead node's rows as zeros
    dS, dxU = dead_rows_buffer((N, 2 * H), dXP.device), None
    jobs = [dict(a=dPn, W=Bn[:H], w_in_out=False, out=dS[:, :H]), dict(a=dPn, W=Bn[H:], w_in_out=False, out=dS[:, H:])]
    if want_dx:    # ... and in the same launch two of the three partial products of dx = dxn + dXP Wx^T
        dxU = dead_rows_buffer((N, 2 * H), dXP.device)
        jobs += [dict(a=dXP[:, :H], W=Wx[:, :H], w_in_out=False, prev=dxn if c.residual else None, out=dxU[:, :H]),
                 dict(a=dXP[:, H:2 * H], W=Wx[:, H:2 * H], w_in_out=False, out=dxU[:, H:])]
    typed_jobs(jobs, nd.tiles)
    return dS, dxU


def _node_dx(c, dxn, dXP, dxU):
    """dx = dxn + dXP Wx^T.  Under ``c.nd`` on the kept nodes' tiles: the third 128-deep block of the contraction + the two partial
    products made beside dS (``dxU``) -- or, for a first layer on the label codes of its edge rows only (no dS launch to share:
    ``dxU`` None), block after block."""
    nd, H, Wx = c.nd, c.H, c.Wx
    if nd is None:
        return torch.addmm(dxn, dXP, Wx.t()) if c.residual else dXP @ Wx.t()
    dx = _dx_buffer(c, dXP.device)
    if dxU is not None:
        return out_fwd_typed(dXP[:, 2 * H:], Wx[:, 2 * H:], None, dxU[:, :H], nd.tiles, out=dx, w_in_out=False, prev2=dxU[:, H:])
    for b3 in range(3):
        out_fwd_typed(dXP[:, b3 * H:(b3 + 1) * H], Wx[:, b3 * H:(b3 + 1) * H], None,
                      (dxn if c.residual else None) if b3 == 0 else dx, nd.tiles, out=dx, w_in_out=False)
    return dx


def _node_bwd_rows(c, chain_panels, x, S, H1n, dxn, dXP, want_dx):
    """Stage, rows variant: the node side backward -> ``(dBn, dbn, dWx, dW2n, db2n, dS, dx)``: dPn with the bias gradients, dS,
    the weight gradients, dx -- the kept-node chain makes all but the weight gradients in its one launch."""
    nd, H = c.nd, c.H
    one_launch, kernel = _node_one_launch(c, x, S, H1n, dxn, dXP), atb_ok(x, dXP)
    chained = nd is not None and chain_panels is not None and node_chain_ok(H, dxn, H1n, dXP)
    dx = None
    if chained:
        # the kept-node chain as ONE launch (csrc/dmp_nodechain.hip): dPn with its two column sums, dS = dPn Bn^T and
        # dx = dxn + dXP Wx^T -- the partial products of dx never go through memory
        dPn, dW2n = dXP[:, :H], None
        dS = dead_rows_buffer((c.N, 2 * H), x.device)
        if want_dx:
            dx = _dx_buffer(c, x.device)
        dbn, db2n = node_chain_bwd(dxn, H1n, dXP[:, H:], chain_panels[1], c.residual, c.slope, nd.tiles, dPn, dS, dx)
    else:
        dPn, dbn, db2n, dW2n = _node_out_bwd(c, dxn, H1n, dXP, not one_launch, kernel)
        dS, dxU = _node_dS(c, dPn, dXP, dxn, want_dx)
    if one_launch:   # the three node-side weight gradients share one launch
        (dW2n, dBn, dWx), db2 = _node_wgrads(c, [(dxn, H1n), (S, dPn), (x, dXP)])
        db2n = db2n if db2 is None else db2
    else:
        dBn = _wgrad(S, dPn, kernel)                                         # [2H,H]
        dWx = _wgrad(x, dXP, kernel)                                         # [H,3H] = [dA_n | dPd | dPs]
    if want_dx and not chained:
        dx = _node_dx(c, dxn, dXP, dxU)
    return dBn, dbn, dWx, dW2n, db2n, dS, dx


def _l0_node_sum_products(c, tables, S0, dPn):
    """Codes variant: S = [S0_in W0 | S0_out W0] was never built: X[h] = S0_h^T dPn per table (N rows, K columns) carries both
    dBn_h = W0^T X[h] and the segment sums' part of the embedding gradient, sum_h X[h] Bn_h^T (no dS either) -> ``Xn`` [2, TK, H]."""
    l0, nd, H = c.l0, c.nd, c.H
    K0, Kp = l0.K, l0.enc.size(1)
    Xn = (torch.empty if l0_tables_full(l0, tables, c.W0) else torch.zeros)((2, c.W0.size(0), H), dtype=torch.float32, device=dPn.device)
    xjobs = [(S0[n0:n1, h * Kp:h * Kp + K0], dPn[n0:n1], Xn[h, t * K0:(t + 1) * K0],
              nd.mask[n0 // 32:] if nd is not None else None) for t, _, (n0, n1) in tables if n1 > n0 for h in (0, 1)]
    if 0 < len(xjobs) <= 4 and dPn.stride(1) == 1 and dPn.stride(0) % 2 == 0 and dPn.data_ptr() % 8 == 0:
        smallk_atb_jobs(xjobs, H)          # both tables x both halves: one launch
        return Xn
    for t, _, (n0, n1) in (tables if xjobs else []):
        if n1 > n0:
            for h in (0, 1):
                if nd is not None:     # (dPn's rows of the dead nodes were not written: masked out)
                    smallk_atb_cols(S0[n0:n1, h * Kp:h * Kp + K0], dPn[n0:n1], None, Xn[h, t * K0:(t + 1) * K0].unsqueeze(0), H,
                                    mask=nd.mask[n0 // 32:])
                else:
                    smallk_atb(S0[n0:n1, h * Kp:h * Kp + K0], dPn[n0:n1], out=Xn[h, t * K0:(t + 1) * K0])
    return Xn


def _l0_node_code_products(c, dXP, dxn):
    """Codes variant with node codes: x = venc WV0:  x^T dXP = WV0^T (venc^T dXP)  and  venc^T dx = venc^T dxn + (venc^T dXP) Wx^T
    -- N-row passes on K columns instead of two [N,H] x [H,3H] products and the three-block weight gradient -> ``Yn``
    [3 (or 4: with the residual's venc^T dxn), TVK, H]."""
    l0, nd, H, N = c.l0, c.nd, c.H, c.N
    VK, TVK = l0.VK, c.WV0.size(0)
    vfull = all(n1 > n0 for _, (n0, n1) in l0.vtables(N)) and len(l0.vtables(N)) * VK == TVK
    Yn = (torch.empty if vfull else torch.zeros)((4 if c.residual else 3, TVK, H), dtype=torch.float32, device=dXP.device)
    vmask = l0.venc_mask
    for t, (n0, n1) in l0.vtables(N):
        # (the packed node codes carry the node gate: a gated-out node's code row is all zeros)
        # (one table over all nodes under the node gate: the kept nodes' list -- a node outside it has a zero code row)
        klist = nd.rows if (nd is not None and n0 == 0 and n1 == N) else None
        smallk_atb_cols(l0.venc[n0:n1, :VK], dXP[n0:n1], dxn[n0:n1] if c.residual else None,
                        Yn[:, t * VK:(t + 1) * VK], H,
                        mask=vmask[n0 // 32:] if (klist is None and vmask is not None and n0 % 32 == 0) else None, rows=klist)
    return Yn


def _node_bwd_codes(c, tables, S0, x, H1n, dxn, dXP, want_dx):
    """Stage, codes variant: the node side backward of a first layer on the label codes -> ``(dbn, dWx, dW2n, db2n, Xn, Yn, dx)``:
    dPn with the bias gradients, the K-column products in place of dS / dBn (``Xn``) and, with node codes, of dWx (``Yn``: then
    ``dWx`` is None here), the remaining weight gradients, dx."""
    vcodes = c.l0.venc is not None
    one_launch, kernel = _node_one_launch(c, x, None, H1n, dxn, dXP), atb_ok(x, dXP)
    dPn, dbn, db2n, dW2n = _node_out_bwd(c, dxn, H1n, dXP, not one_launch or vcodes, kernel)
    Yn = dWx = None
    l0, N, H = c.l0, c.N, c.H
    stables, vtables = c.W0.size(0) // l0.K, (c.WV0.size(0) // l0.VK if vcodes else 0)
    dres = dxn if c.residual else None
    if vcodes and (c.nd is not None or c.v_gate is None) and l0_node_bwd_ok(H, l0.VK, l0.K, l0.enc.size(1), stables, vtables, N, l0.venc, S0,
                                                                             dXP, dres):
        # both families of K-column products from ONE pass over the kept nodes' gradient rows on the matrix pipe
        Xn = torch.empty((2, c.W0.size(0), H), dtype=torch.float32, device=dXP.device)
        Yn = torch.empty((4 if c.residual else 3, c.WV0.size(0), H), dtype=torch.float32, device=dXP.device)
        nd = c.nd
        l0_node_codes_bwd(l0.venc, l0.VK, vtables, S0, l0.K, l0.enc.size(1), stables, l0.nsplit if stables == 2 else N, dXP, dres, N, H,
                          Xn, Yn, rows=None if nd is None else nd.rows, prefix=0 if nd is None else nd.prefix)
        return dbn, dWx, dW2n, db2n, Xn, Yn, (_node_dx(c, dxn, dXP, None) if want_dx else None)
    Xn = _l0_node_sum_products(c, tables, S0, dPn)
    if vcodes:
        Yn = _l0_node_code_products(c, dXP, dxn)
    elif one_launch:
        (dW2n, dWx), db2 = _node_wgrads(c, [(dxn, H1n), (x, dXP)])
        db2n = db2n if db2 is None else db2
    else:
        dWx = _wgrad(x, dXP, kernel)
    return dbn, dWx, dW2n, db2n, Xn, Yn, (_node_dx(c, dxn, dXP, None) if want_dx else None)


def _edge_input_grad(c, z, dG, dS, dzn, lazy, dWes, typed):
    """Stage, rows variant: the edge input gradient -- residual + seg_sum2 backward + GEMM, accumulated in place -> ``(dz, dWes)``
    (``dWes`` None on entry: ``_edge_first_wgrad`` left it to ``bwd_z_w``'s launch here).
    The input gradient of an edge under a zero of a gate that wiped the rep-net's input rows is multiplied by that zero further
    down: not computed.  After the first layer (``inner`` bit 1) its reader is the layer before, which leaves those rows out; the
    first layer hands zeros to whoever made the rows."""
    ix, coef, H, e_gate, Wes, nd = c.index, c.coef, c.H, c.e_gate, c.Wes, c.nd
    if not typed:
        dz = ops.gather_select_raw(dS, ix.dst32, ix.rev8, H, None, -1.0, 1.0, base=dzn if c.residual else None)
        dz.addmm_(dG, Wes.t())
        return dz, dWes
    dead_dz = (("leave" if (c.inner & 2) else "zero") if dead_edge_rows(ix, H, e_gate) else None)
    dst_m = None if nd is None else nd.sel[2]      # (dS's rows of the dead nodes were not written: read as zeros)
    base = None if not c.residual else (lazy[0] if lazy is not None else dzn)
    base_map = lazy[1] if (lazy is not None and c.residual) else None
    if dWes is None:
        both = bwd_z_w(dG, z, Wes, dS, base, coef, ix, c.WesT, base_map=base_map, gate=e_gate, dead_rows=dead_dz, dst=dst_m)
        if both is not None:
            return both
        dWes = atb_typed(z, dG, coef, ix, gate=e_gate)
    return bwd_z_typed(dG, dG.stride(0), Wes, dS, base, coef, ix, c.WesT, base_map=base_map, gate=e_gate, dead_rows=dead_dz,
                       dst=dst_m), dWes


def _l0_final_products(c, XX, Xn, Yn, dWx):
    """Stage, codes variant, after the reductions of the stages before have run: ONE launch -> ``(dBn, dWx, dWes, dW0, dWV0)``.
    dWes = W0^T (enc^T [dPre | c dPre]);  dBn_h = W0^T X_h;  enc^T dz = (enc^T [dPre | c dPre]) [A | B]^T + sum_h X_h Bn_h^T
    (+ enc^T dzn);  with node codes dWx = WV0^T (venc^T dXP) block by block and venc^T dx = sum_b Y_b Wx_b^T (+ venc^T dxn)."""
    H, W0, WV0, Bn, Wx, dev = c.H, c.W0, c.WV0, c.Bn, c.Wx, XX.device
    dWes = torch.empty((H, 2 * H), dtype=torch.float32, device=dev)
    dBn = torch.empty((2 * H, H), dtype=torch.float32, device=dev)
    dW0 = torch.empty((W0.size(0), H), dtype=torch.float32, device=dev)
    dWV0 = None
    jobs = [(dWes, [(W0, True, XX[:, :2 * H], False)], None),
            (dBn[:H], [(W0, True, Xn[0], False)], None), (dBn[H:], [(W0, True, Xn[1], False)], None),
            (dW0, [(XX[:, :2 * H], False, c.Wes, True), (Xn[0], False, Bn[:H], True), (Xn[1], False, Bn[H:], True)],
             XX[:, 2 * H:] if c.residual else None)]
    if Yn is not None:
        dWx = torch.empty((H, 3 * H), dtype=torch.float32, device=dev)
        dWV0 = torch.empty((WV0.size(0), H), dtype=torch.float32, device=dev)
        for b3 in range(3):
            jobs.append((dWx[:, b3 * H:(b3 + 1) * H], [(WV0, True, Yn[b3], False)], None))
        jobs.append((dWV0, [(Yn[b3], False, Wx[:, b3 * H:(b3 + 1) * H], True) for b3 in range(3)], Yn[3] if c.residual else None))
    small_gemm_jobs(jobs)
    return dBn, dWx, dWes, dW0, dWV0


class _FusedDMPLayer(torch.autograd.Function):
    """One DMPNN layer + gate + residual over the folded weights of ``fold_layers``: each pass a short list of the stages above."""

    @staticmethod
    def forward(ctx, index, coef, residual, x, z, v_gate, e_gate, Bn, bn, Wx, Wes, be, nW2, nb2, eW2, eb2,
                WesT=None, nW2t=None, eW2t=None, slope=0.0, vpool=None, epool=None, l0=None, W0=None, WV0=None, edge_rows=True,
                inner=0):
        """``inner``: this layer's place among the layers of a rep-net that share its gates -- bit 0: another layer follows (the
        only reader of the edge rows returned here), bit 1: another layer precedes (the only reader of the edge rows' gradient).
        ``l0`` (``Layer0Codes``) with ``W0 = l0.W`` / ``WV0 = l0.WV`` as differentiable inputs: the FIRST layer of a rep-net
        whose edge rows are a label embedding, ``z = enc W0``.  Every product with ``z`` runs on its K-column factor
        (csrc/dmp_layer0.hip); ``z`` itself is only read as the residual and takes no gradient: the embedding's gradient comes
        back as ``dW0``.  With ``l0.venc`` the same for the node rows ``x = venc WV0`` (products with ``x`` -> ``dWV0``).
        ``edge_rows=False`` (with ``epool``): ``zn`` is not formed (None is returned in its place); its per-graph sums are
        ``pool(zn) = pool(z) + pool(g (.) H1) W2^T + (sum g) b2`` -- two pooled passes over E rows instead of the Linear +
        gate + residual kernel (two reads, one write) and a pooled pass over its output.
        ``vpool`` / ``epool`` (``ops.PoolIndex`` over the node / edge rows; the LAST layer of a rep-net whose outputs
        feed sum / mean pooling heads): two more outputs, the per-graph sums of ``xn`` / ``zn`` ([G, H]; edges with a flag
        [G, 2H] = [non-reversed | reversed]).  A gradient that arrives ONLY through the edge sums is never expanded to
        [E, H]: every row of a graph has the same gradient vector, see ``_grad_seeds``."""
        _lib.require_gpu(x, z)
        H = Bn.size(1)
        x, z = x.contiguous(), z.contiguous()
        sums_only = epool is not None and not edge_rows
        c = _LayerCall(index=index, coef=coef, residual=residual, H=H, N=index.num_nodes, slope=slope, inner=int(inner),
                       v_gate=v_gate, e_gate=e_gate, Bn=Bn.contiguous(), bn=bn, Wx=Wx.contiguous(), Wes=Wes.contiguous(), be=be,
                       nW2=nW2, nb2=nb2, eW2=eW2, eb2=eb2, WesT=WesT, nW2t=nW2t, eW2t=eW2t, l0=l0,
                       W0=None if l0 is None else W0.detach(), WV0=None if (l0 is None or WV0 is None) else WV0.detach(),
                       nd=_kept_nodes(index, H, v_gate, l0), vpool=vpool, epool=epool,
                       poolalg=sums_only and pool_algebra_ok(index, H, epool, eW2, eb2))
        # ---- node side (dmpnn.py:113,121,125 + fn.sum + 129-140)
        S = S0 = M0 = tables = xn = chain_panels = None
        if l0 is not None:
            S0, M0, tables, H1n, P, ldp = _node_first_codes(c, x, z)
        else:
            S, H1n, P, ldp, xn, chain_panels = _node_first_rows(c, x, z)
        if xn is None:
            xn = _node_out(c, x, H1n)
        # ---- edge side (dmpnn.py:112,120,124 + 142-156)
        if l0 is not None:
            H1e, zn = _edge_first_codes(c, z, M0, tables, P, ldp, sums_only)
        else:
            H1e, zn = _edge_first_rows(c, z, P, ldp, sums_only)
        if zn is None and not sums_only:
            zn = _edge_out(c, z, H1e)
        ctx.call, ctx.chain_panels, ctx.l0_S0, ctx.l0_tables, ctx.gcnt = c, chain_panels, S0, tables, None
        ctx.save_for_backward(x, z if l0 is None else None, S, H1n, H1e)
        if vpool is None and epool is None:
            return xn, zn
        ctx.set_materialize_grads(False)    # a missing gradient stays None (the common case: only the sums are used)
        vs, es, ctx.gcnt = _pooled_outputs(c, z, xn, zn, H1e, sums_only)
        return xn, zn, vs, es

    @staticmethod
    @once_differentiable
    def backward(ctx, dxn, dzn, dvs=None, des=None):
        x, z, S, H1n, H1e = ctx.saved_tensors
        c, tables = ctx.call, ctx.l0_tables
        typed = typed_ok(c.index, c.H)
        want_dx, want_dz = ctx.needs_input_grad[3], ctx.needs_input_grad[4]
        dxn, dzn, lazy = _grad_seeds(c, x, z, H1e, dxn, dzn, dvs, des, typed)
        dz = dW0 = dWV0 = None
        # the parameter-gradient partials (biases, split-K weight gradients) are consumed after the layer (by the
        # unfold of fold_layers / the optimizer): their reductions run as one launch when this block is left
        with deferred_reductions():
            dG, dbe, dW2e, db2e, l0_XX = _edge_out_bwd(c, tables, H1e, dzn, lazy, ctx.gcnt, typed)
            dXP = _endpoint_sums(c, dG, typed, x.device)
            if c.l0 is not None:
                XX = _l0_edge_code_products(c, tables, dG, dzn, l0_XX)
                dbn, dWx, dW2n, db2n, Xn, Yn, dx = _node_bwd_codes(c, tables, ctx.l0_S0, x, H1n, dxn, dXP, want_dx)
            else:
                dWes = _edge_first_wgrad(c, z, dG, typed, want_dz)
                dBn, dbn, dWx, dW2n, db2n, dS, dx = _node_bwd_rows(c, ctx.chain_panels, x, S, H1n, dxn, dXP, want_dx)
                if want_dz:
                    dz, dWes = _edge_input_grad(c, z, dG, dS, dzn, lazy, dWes, typed)
        if c.l0 is not None:
            dBn, dWx, dWes, dW0, dWV0 = _l0_final_products(c, XX, Xn, Yn, dWx)
        return (None, None, None, dx, dz, None, None, dBn, dbn, dWx, dWes, dbe, dW2n, db2n, dW2e, db2e, None, None, None, None,
                None, None, None, dW0, dWV0, None, None)


def l0_z_from_codes(index, H, eg, l0, live_edges, residual):
    """May ``dmpnn.joint_rep`` leave the target's part of the first layer's edge rows ``z = enc W`` out of memory altogether?  With
    a residual layer and the conditions under which its second Linear runs over the kept edges' tiles (``l0_dead_inputs``' edge
    half) -- or without any edge gate, over all rows -- that launch adds ``enc W`` as one more k-group (``out_fwd_typed_codes``).
    (A layer that ends up elsewhere makes the rows itself: ``l0_rows``.)"""
    return bool(USE_OUT_CODES and (live_edges or eg is None) and residual and l0 is not None and H == 128
                and not _lib.load().dmp_dev_get_exact_fp32() and l0.enc.stride(0) % 4 == 0 and l0.enc.data_ptr() % 16 == 0
                and index.num_edges * 128 * 4 < (1 << 32) - 65536)


def l0_dead_inputs(index, H, vg, eg, l0, coef):
    """``(edges, nodes)``: may the input rows of a first layer on the label codes (``l0``) stay UNWRITTEN under the zeros of the
    union's 0 / 1 gates?  The layer reads its edge rows ``z`` only as the residual term of its second Linear -- over the kept
    edges' tiles under ``dead_edge_rows`` -- and its node rows ``x`` (with node codes) only as the residual term over the kept
    nodes' tiles (``kept_node_path``)."""
    return (l0 is not None and dead_edge_rows(index, H, eg, coef),
            bool(l0 is not None and l0.venc is not None and kept_node_path(index, H, vg, l0)))


def activation_slope(act):
    """Negative slope of an MLP activation module the fused path can run: 0.0 for ``nn.ReLU``, ``negative_slope``
    for ``nn.LeakyReLU`` (the reference's default ``leaky_relu``: 1/5.5, utils/act.py:27,466); None otherwise."""
    if type(act) is torch.nn.ReLU:
        return 0.0
    if type(act) is torch.nn.LeakyReLU and 0.0 <= float(act.negative_slope) <= 1.0:
        return float(act.negative_slope)
    return None


def l0_ok(index, H, enc_p, enc_g, W_p, W_g):
    """The first layer can run on the label codes: embedding tables of the same (at most L0_KMAX) number of rows on both
    sides, the class-typed kernels' shape limits (the backward's dPre comes from them)."""
    return (USE_LAYER0 and H in MFMA_WIDTHS and enc_p.size(1) == enc_g.size(1) == W_g.size(0) == W_p.size(0) <= L0_KMAX
            and W_g.size(1) == W_p.size(1) == H and W_g.dtype == W_p.dtype == enc_p.dtype == enc_g.dtype == torch.float32
            and enc_p.stride(1) == 1 and enc_g.stride(1) == 1 and enc_g.is_cuda and index.num_edges > 0 and typed_ok(index, H)
            and onepanel_ok(H))


def l0_nodes_ok(H, enc_p, enc_g, W_p, W_g):
    """The node rows of the first layer can run on their label codes as well (same conditions as the edge rows)."""
    return (enc_p.size(1) == enc_g.size(1) == W_g.size(0) == W_p.size(0) <= SMALLK_MAX and W_g.size(1) == W_p.size(1) == H
            and W_g.dtype == W_p.dtype == enc_p.dtype == enc_g.dtype == torch.float32 and enc_p.stride(1) == 1
            and enc_g.stride(1) == 1 and enc_g.is_cuda and H in MFMA_WIDTHS)


def fused_dmp_layer(index, coef, residual, x, z, v_gate, e_gate, layer, folded=None, pools=None, l0=None, inner=0):
    """``folded``: this layer's entry of ``fold_layers`` (rep-nets fold all their layers in one launch).
    ``pools`` = ``(node PoolIndex or None, edge PoolIndex or None[, edge rows wanted])``: also returns the per-graph sums of
    both outputs; with the third entry False the edge rows themselves are not formed (None in their place).
    ``l0`` (``Layer0Codes``): ``z`` is ``l0.enc @ l0.W`` (and ``x`` is ``l0.venc @ l0.WV``), see ``_FusedDMPLayer.forward``."""
    n2, e2 = layer.nmlp[2], layer.emlp[2]
    Bn, bn, Wx, Wes, be, WesT, nW2t, eW2t = folded if folded is not None else fold_layers([layer])[0]
    vpool, epool = pools[:2] if pools is not None else (None, None)
    edge_rows = pools[2] if pools is not None and len(pools) > 2 else True
    return _FusedDMPLayer.apply(index, coef, bool(residual), x, z, v_gate, e_gate, Bn, bn, Wx, Wes, be,
                                n2.weight, n2.bias, e2.weight, e2.bias, WesT, nW2t, eW2t, activation_slope(layer.nmlp[1]),
                                vpool, epool, l0, None if l0 is None else l0.W, None if l0 is None else l0.WV, edge_rows, int(inner))
