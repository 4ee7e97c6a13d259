"""Masked multi-head attention with sparsemax weights (the core of the attention prediction heads' ``DotAttention``,
``SubgraphCountingMatching/models/pred.py:240-487``; sparsemax ``utils/act.py:255-316``).

Two implementations of one function:

* ``SparsemaxAttention`` -- fp32 on the GPU, head widths ``KERNEL_DH``: the fused kernels of ``csrc/dmp_attn.hip``
  (no ``[B, Lq, Lk, heads]`` tensor; forward keeps one threshold and one support size per row and head).
* ``attention_tensor`` -- the same function in tensor ops (padded score tensor, sort-based sparsemax): the CPU path,
  and the GPU path for head widths outside ``KERNEL_DH`` or for non-fp32 inputs.

Semantics (the reference's): masked keys are filled with -1e30 before the sparsemax over the key axis, which blocks
their gradient; a row whose keys are all masked therefore weighs every padded position by 1 / Lk and passes no
gradient to its scores; rows with a masked query are zeroed after the weights are applied to V.
"""
import torch as th

from .constants import _INF

KERNEL_DH = (4, 8, 16, 32, 64)


def sparsemax(x, dim=-1):
    """Euclidean projection of ``x`` onto the probability simplex along ``dim``: ``max(0, x - tau)`` with the
    threshold tau = (sum of the k largest - 1) / k for the largest k with 1 + k z_(k) > sum_{i <= k} z_(i)
    (z sorted descending).  Autograd through these ops gives the sparsemax Jacobian."""
    x = x.transpose(dim, -1)
    z = x - x.max(dim=-1, keepdim=True)[0]
    zs = th.sort(z, dim=-1, descending=True)[0]
    k = th.arange(1, z.size(-1) + 1, dtype=z.dtype, device=z.device)
    cs = zs.cumsum(dim=-1)
    size = (1.0 + k * zs > cs).sum(dim=-1, keepdim=True)          # the support is a prefix of the sorted row
    tau = (cs.gather(-1, size - 1) - 1.0) / size.to(z.dtype)
    return th.clamp_min(z - tau, 0.0).transpose(dim, -1)


def _as_mask(m, B, L):
    return None if m is None else m.reshape(B, L)


def attention_tensor(q, k, v, qmask, kmask, num_heads, scale):
    """q [B, Lq, nh * dh], k / v [B, Lk, nh * dh], masks [B, L] (nonzero = live) or None -> [B, Lq, nh * dh]."""
    B, Lq, D = q.shape
    Lk = k.size(1)
    dh = D // num_heads                          # (spelled out: -1 cannot be inferred for an empty batch or query set)
    qh, kh, vh = q.view(B, Lq, num_heads, dh), k.view(B, Lk, num_heads, dh), v.view(B, Lk, num_heads, dh)
    s = th.einsum("bind,bjnd->bijn", qh, kh) * scale
    if kmask is not None:
        s = s.masked_fill(_as_mask(kmask, B, Lk).view(B, 1, Lk, 1) == 0, _INF)
    p = sparsemax(s, dim=2)
    o = th.einsum("bijn,bjnd->bind", p, vh).reshape(B, Lq, D)
    if qmask is not None:
        o = o.masked_fill(_as_mask(qmask, B, Lq).view(B, Lq, 1) == 0, 0.0)
    return o


def _out(shape, dtype, dev):
    """Output buffers of the kernels: NaN-filled under DMP_POISON_DEAD_ROWS=1 (every element must be written)."""
    from .fused import POISON_DEAD_ROWS
    if POISON_DEAD_ROWS:
        return th.full(shape, float("nan"), dtype=dtype, device=dev) if dtype.is_floating_point else th.full(shape, -1, dtype=dtype, device=dev)
    return th.empty(shape, dtype=dtype, device=dev)


def _u8(m, B, L):
    if m is None:
        return None
    m = m.reshape(B, L)
    if m.dtype == th.bool:
        return m.contiguous().view(th.uint8)
    return (m != 0).contiguous().view(th.uint8)


def _aligned(t):
    """``t`` as the kernels read it (row-major, float4 loads): itself where it is contiguous and 16-byte aligned, else a
    copy (a contiguous view at an odd offset into a larger buffer is contiguous and not aligned)."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class SparsemaxAttention(th.autograd.Function):
    """The HIP kernels (csrc/dmp_attn.hip) as one autograd node: forward ``dmp_attn_fwd``, backward ``dmp_attn_bwd``
    (scores recomputed from Q and K).  No host round trip: workspaces follow from the shapes alone."""

    @staticmethod
    def forward(ctx, q, k, v, qmask, kmask, num_heads, scale):
        from . import _lib
        lib = _lib.load()
        B, Lq, D = q.shape
        Lk = k.size(1)
        dh = D // num_heads
        q, k, v = _aligned(q), _aligned(k), _aligned(v)
        _lib.require_gpu(q, k, v)
        qm, km = _u8(qmask, B, Lq), _u8(kmask, B, Lk)
        o = _out(q.shape, th.float32, q.device)
        tau = _out((B, Lq, num_heads), th.float32, q.device)
        supp = _out((B, Lq, num_heads), th.int32, q.device)
        _lib.check(lib.dmp_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), _lib.ptr(qm), _lib.ptr(km), B, Lq, Lk, num_heads, dh,
                                    float(scale), o.data_ptr(), tau.data_ptr(), supp.data_ptr(), _lib.stream_ptr()), "dmp_attn_fwd")
        ctx.save_for_backward(q, k, v, tau, supp)
        ctx.masks, ctx.num_heads, ctx.scale = (qm, km), num_heads, float(scale)
        ctx.mark_non_differentiable(tau, supp)
        return o, tau, supp

    @staticmethod
    def backward(ctx, do, _dtau=None, _dsupp=None):
        from . import _lib
        lib = _lib.load()
        q, k, v, tau, supp = ctx.saved_tensors
        qm, km = ctx.masks
        B, Lq, D = q.shape
        Lk = k.size(1)
        do = _aligned(do)
        delta = _out((B, Lq, ctx.num_heads), th.float32, q.device)
        dq, dk, dv = _out(q.shape, th.float32, q.device), _out(k.shape, th.float32, q.device), _out(v.shape, th.float32, q.device)
        _lib.check(lib.dmp_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), _lib.ptr(qm), _lib.ptr(km), do.data_ptr(), tau.data_ptr(),
                                    supp.data_ptr(), B, Lq, Lk, ctx.num_heads, D // ctx.num_heads, ctx.scale, delta.data_ptr(),
                                    dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), _lib.stream_ptr()), "dmp_attn_bwd")
        return dq, dk, dv, None, None, None, None


def kernel_ok(q, k, v, num_heads):
    """The HIP kernels take these inputs: fp32 on the GPU, head width in ``KERNEL_DH``, at least one key."""
    D = q.size(-1)
    return (q.is_cuda and all(t.dtype == th.float32 for t in (q, k, v)) and D % num_heads == 0
            and D // num_heads in KERNEL_DH and v.size(-1) == D and k.size(-1) == D and k.size(1) >= 1)


def sparsemax_attention(q, k, v, qmask, kmask, num_heads, scale):
    """``sparsemax(scale q k^T, keys masked) v`` per head, query-masked rows zeroed; the kernels where ``kernel_ok``,
    else ``attention_tensor``."""
    if kernel_ok(q, k, v, num_heads):
        return SparsemaxAttention.apply(q, k, v, qmask, kmask, num_heads, scale)[0]
    return attention_tensor(q, k, v, qmask, kmask, num_heads, scale)
