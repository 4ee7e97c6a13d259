"""Memory initialisation of the memory-attention heads and DIAMNet (``SubgraphCountingMatching/models/pred.py:648-1328``):
every pair's padded rows pooled into ``M`` memory slots.

Two implementations of one function:

* ``MemInit`` -- fp32 on the GPU, ``D % 4 == 0``: the kernels of ``csrc/dmp_mem.hip`` (one launch pools the key and the
  value memory of an attention; the windows are found on the device, so nothing is read back to the host).
* ``memory_tensor`` -- the same function in tensor ops (gather of every window's rows): the CPU path, and the GPU path for
  non-fp32 inputs or ``D % 4 != 0``.

Semantics (the reference's ``init_mem`` applied per pair, which ``MemDotAttention.init_memory`` and ``DIAMNet.init_memory``
do in Python loops): s / e = first / last live position of the pair's mask (both 0 when none is live); the segment is the
``n`` rows from s as they are (masked interior rows included, each with its own mask bit), n = e - s for the
memory-attention heads (the reference's slice ends at e) and e - s + 1 for DIAMNet.  ``circular_*`` extends the segment
to n' = n + ceil((n + 1) / 2) - 1 rows (row p = segment row p mod n).  n' <= M: the rows fill the last n' slots, the others
are zero with mask 0.  n' > M: stride = n' // M, k = n' - (M - 1) stride, slot i pools rows i stride .. i stride + k - 1
(mean, sum or max; the mask is the OR of the window's bits; the gradient of max goes to the window's first maximum).
"""
import torch as th

from . import _abi

MODES = {"mean": _abi.DMP_MEM_MEAN, "sum": _abi.DMP_MEM_SUM, "max": _abi.DMP_MEM_MAX}
UNBUILT = ("attn", "lstm", "circular_attn", "circular_lstm")


def parse_mem_init(mem_init):
    """``mem_init`` -> (pooling mode, circular).  attn / lstm memory initialisation is not built: the reference's attn path
    fails whenever a segment fits in the memory (``mk`` is used before it is assigned, pred.py:680) and its lstm path runs a
    sequential LSTM per window."""
    if mem_init in UNBUILT:
        raise NotImplementedError("mem_init=%s is not built: only mean / sum / max pooling (optionally circular_) initialise "
                                  "the memory on the MI355X path" % mem_init)
    circular = mem_init.startswith("circular_")
    mode = mem_init[len("circular_"):] if circular else mem_init
    if mode not in MODES:
        raise ValueError("mem_init=%s is not one of the reference's choices" % mem_init)
    return mode, circular


def start_end(mask):
    """utils/dl.py:130-135: (first live position, last live position) per row of ``mask`` [B, L]; (0, 0) for a row with
    no live position."""
    live = mask != 0
    idx = th.arange(mask.size(1), device=mask.device)
    first = idx.masked_fill(~live, mask.size(1)).amin(dim=1)
    last = idx.masked_fill(~live, -1).amax(dim=1)
    none = last < 0
    return first.masked_fill(none, 0), last.masked_fill(none, 0)


def windows(mask, M, circular, inclusive_end):
    """Per slot the rows it pools: (row [B, M, K] int64, valid [B, M, K] bool, count [B, M] int64).  K is a bound from the
    shapes alone (no host read): k = n' // M + n' % M <= L' // M + M - 1 for the longest extended segment L'."""
    B, L = mask.shape
    dev = mask.device
    s, e = start_end(mask)
    n = e - s + 1 if inclusive_end else e - s
    Lx = L + (L + 2) // 2 - 1 if circular else L
    K = max(1, min(Lx, Lx // M + M - 1))
    np_ = n + (n + 2) // 2 - 1 if circular else n
    big = np_ > M
    stride = th.where(big, np_ // M, th.ones_like(np_))
    k = th.where(big, np_ - (M - 1) * stride, th.ones_like(np_))
    i = th.arange(M, device=dev).view(1, M)
    q0 = th.where(big.view(B, 1), i * stride.view(B, 1), i - (M - np_).view(B, 1))
    cnt = th.where(big.view(B, 1), k.view(B, 1).expand(B, M), (q0 >= 0).long())
    j = th.arange(K, device=dev).view(1, 1, K)
    valid = j < cnt.unsqueeze(-1)
    q = th.where(valid, q0.unsqueeze(-1) + j, th.zeros_like(j))
    row = s.view(B, 1, 1) + q % n.clamp_min(1).view(B, 1, 1)
    return row.clamp(0, L - 1), valid, cnt


def memory_tensor(xs, mask, M, mode, circular, inclusive_end):
    """The memory of every tensor of ``xs`` ([B, L, D] each) and the memory mask [B, M] (bool), in tensor ops."""
    B, L = mask.shape
    row, valid, cnt = windows(mask, M, circular, inclusive_end)
    bidx = th.arange(B, device=mask.device).view(B, 1, 1)
    mmask = ((mask[bidx, row] != 0) & valid).any(dim=2)
    out = []
    for x in xs:
        g = x[bidx, row]                                         # [B, M, K, D]
        v = valid.unsqueeze(-1)
        if mode == "max":
            m = g.masked_fill(~v, float("-inf")).max(dim=2)[0]
            m = m.masked_fill((cnt == 0).unsqueeze(-1), 0.0)
        else:
            m = g.masked_fill(~v, 0.0).sum(dim=2)
            if mode == "mean":
                m = m / cnt.clamp_min(1).unsqueeze(-1).to(m.dtype)
        out.append(m)
    return out, mmask


def _rows_view(x):
    """x [B, L, D] as the kernels take it: unit column stride, a 16-byte row stride and L rows per pair."""
    B, L, D = x.shape
    if not (x.stride(2) == 1 and x.stride(1) % 4 == 0 and x.stride(1) >= D and x.stride(0) == L * x.stride(1)
            and x.data_ptr() % 16 == 0):
        x = x.contiguous()
    return x


def _out(shape, dtype, dev):
    from .attn import _out as out
    return out(shape, dtype, dev)


class MemInit(th.autograd.Function):
    """The HIP kernels (csrc/dmp_mem.hip) as one autograd node over one or two tensors that share the mask: forward
    ``dmp_mem_init_fwd``, backward ``dmp_mem_init_bwd``.  Outputs: the memories, then the memory mask (uint8)."""

    @staticmethod
    def forward(ctx, mask, M, mode, circular, inclusive_end, *xs):
        from . import _lib
        lib = _lib.load()
        xs = [_rows_view(x) for x in xs]
        _lib.require_gpu(*xs)
        B, L, D = xs[0].shape
        dev = xs[0].device
        m8 = (mask.reshape(B, L) != 0).contiguous().view(th.uint8)
        ys = [_out((B, M, D), th.float32, dev) for _ in xs]
        ymask = _out((B, M), th.uint8, dev)
        seg = _out((B, 2), th.int32, dev)
        args = [_out((B, M, D), th.int32, dev) for _ in xs] if mode == "max" else []
        x1 = xs[1] if len(xs) > 1 else None
        _lib.check(lib.dmp_mem_init_fwd(xs[0].data_ptr(), xs[0].stride(1), _lib.ptr(x1), x1.stride(1) if x1 is not None else 0,
                                        m8.data_ptr(), B, L, D, M, MODES[mode], int(circular), int(inclusive_end),
                                        ys[0].data_ptr(), _lib.ptr(ys[1] if x1 is not None else None), ymask.data_ptr(),
                                        _lib.ptr(args[0] if args else None), _lib.ptr(args[1] if len(args) > 1 else None),
                                        seg.data_ptr(), _lib.stream_ptr()), "dmp_mem_init_fwd")
        ctx.save_for_backward(seg, *args)
        ctx.shape, ctx.M, ctx.mode, ctx.circular, ctx.n = (B, L, D), M, mode, circular, len(xs)
        ctx.mark_non_differentiable(ymask)
        return tuple(ys) + (ymask,)

    @staticmethod
    def backward(ctx, *grads):
        from . import _lib
        lib = _lib.load()
        seg, *args = ctx.saved_tensors
        B, L, D = ctx.shape
        dys = [(g if g is not None else th.zeros((B, ctx.M, D), dtype=th.float32, device=seg.device)).contiguous()
               for g in grads[:ctx.n]]
        dxs = [_out((B, L, D), th.float32, seg.device) for _ in dys]
        two = ctx.n > 1
        _lib.check(lib.dmp_mem_init_bwd(dys[0].data_ptr(), _lib.ptr(dys[1] if two else None), _lib.ptr(args[0] if args else None),
                                        _lib.ptr(args[1] if two and args else None), seg.data_ptr(), B, L, D, ctx.M,
                                        MODES[ctx.mode], int(ctx.circular), dxs[0].data_ptr(), _lib.ptr(dxs[1] if two else None),
                                        _lib.stream_ptr()), "dmp_mem_init_bwd")
        return (None, None, None, None, None) + tuple(dxs)


def kernel_ok(xs):
    """The HIP kernels take these inputs: fp32 on the GPU, equal shapes, width a multiple of 4."""
    x = xs[0]
    return (x.is_cuda and x.dim() == 3 and x.size(2) % 4 == 0 and x.size(1) >= 1 and x.size(0) < 65536
            and all(t.dtype == th.float32 and t.shape == x.shape for t in xs))


def memory_init(xs, mask, mem_len, mem_init, inclusive_end=False):
    """Pool every tensor of ``xs`` ([B, L, D] each, one or two) over the windows of ``mask`` [B, L] (nonzero = live):
    (list of memories [B, mem_len, D], memory mask [B, mem_len] bool).  The kernels where ``kernel_ok``, else
    ``memory_tensor``."""
    mode, circular = parse_mem_init(mem_init)
    if mask is None:
        raise ValueError("the memory is initialised from the live positions of a mask: mask must be given")
    B, L = xs[0].shape[:2]
    mask = mask.reshape(B, L)
    if kernel_ok(xs):
        outs = MemInit.apply(mask, mem_len, mode, circular, bool(inclusive_end), *xs)
        return list(outs[:-1]), outs[-1].view(th.bool)
    return memory_tensor(xs, mask, mem_len, mode, circular, inclusive_end)
