"""The CNN rep-net layer (``SubgraphCountingMatching/models/cnn.py:13-172``) on the HIP kernels of ``csrc/dmp_cnn.hip``.

``CNNLayerHIP`` is one autograd node per layer on channels-last rows ``[B, L, H]``:

* forward  -- ``dmp_cnn_fwd``: conv + bias + activation + max-pool (+ gate and residual without BatchNorm) in one launch;
  it also writes the gate after the layer and one byte per output (the pool window's arg-max and the activation's sign);
* backward -- ``dmp_cnn_route_bwd`` (pool and activation), ``dmp_cnn_fwd`` on the flipped weight (dX as the transposed
  conv), ``dmp_cnn_wgrad`` + ``dmp_reduce_partials`` (dW, db as split-K partials summed in a fixed order).  No float
  atomics: two runs are bitwise equal.

With ``rep_cnn_batch_norm`` the kernel stops after the pool; ``nn.BatchNorm1d``'s function then runs over all ``B L'``
positions (``F.batch_norm`` on the ``[B L', H]`` rows), and the gate and the residual follow in tensor ops.

``hip_layer_ok`` decides: stride 1, dilation 1, kernel sizes 1-8 (pool padding at most half the pool kernel), H 64 or
128, fp32 on the GPU, relu / leaky_relu, dropout 0 or eval mode.  Anything else runs the reference's tensor ops
(``CNNLayer.forward`` on a transposed view) -- also the CPU implementation -- which raise the reference's own errors for
the geometries the reference cannot run."""
import torch as th
import torch.nn as nn
import torch.nn.functional as F


def _act_slope(layer):
    from .fused import activation_slope
    return activation_slope(layer.act)


def hip_layer_ok(layer, x, gate):
    c, p = layer.conv, layer.pool
    k = c.kernel_size[0]
    pk = p.kernel_size if isinstance(p.kernel_size, int) else p.kernel_size[0]
    pp = p.padding if isinstance(p.padding, int) else p.padding[0]
    pad = c.padding[0] if isinstance(c.padding, tuple) else c.padding
    if not (x.is_cuda and x.dtype == th.float32 and x.dim() == 3 and x.size(2) in (64, 128) and x.size(1) >= 1):
        return False
    if not (c.stride == (1,) and c.dilation == (1,) and c.groups == 1 and isinstance(pad, int) and 1 <= k <= 8 and 0 <= pad < k):
        return False
    if not (c.in_channels == c.out_channels == x.size(2) and c.bias is not None and c.weight.dtype == th.float32):
        return False
    if not (p.stride in (1, (1,)) and p.dilation in (1, (1,)) and not p.ceil_mode and 1 <= pk <= k and 0 <= 2 * pp <= pk):
        return False
    if layer.drop.p > 0 and layer.training:
        return False
    if layer.bn is not None and not isinstance(layer.bn, nn.BatchNorm1d):
        return False
    slope = _act_slope(layer)
    if slope is None:
        return False
    L = x.size(1)
    Lc = L + 2 * pad - k + 1
    if Lc < 1 or Lc + 2 * pp - pk + 1 < 1 or x.size(0) >= 65536:
        return False
    return gate is None or (gate.is_cuda and gate.shape == x.shape[:2])


def _geometry(layer):
    c, p = layer.conv, layer.pool
    k = c.kernel_size[0]
    pad = c.padding[0]
    pk = p.kernel_size if isinstance(p.kernel_size, int) else p.kernel_size[0]
    pp = p.padding if isinstance(p.padding, int) else p.padding[0]
    return k, pad, pk, pp


class CNNLayerHIP(th.autograd.Function):
    """Y = pool(act(conv(x) + b)) [* gate' + x]: the kernels of csrc/dmp_cnn.hip.  Outputs (Y, gate' or None)."""

    @staticmethod
    def forward(ctx, x, weight, bias, gate, geo, slope, fuse, residual):
        from . import _lib
        lib = _lib.load()
        k, pad, pk, pp = geo
        x = x.contiguous()
        _lib.require_gpu(x, weight, bias, gate)
        B, L, H = x.shape
        Lc = L + 2 * pad - k + 1
        Lout = Lc + 2 * pp - pk + 1
        dev = x.device
        wt = weight.detach().permute(2, 1, 0).contiguous()              # Wt[j][i][o] = W[o, i, j]
        g_in = gate.contiguous().float() if gate is not None else None
        g_out = th.empty((B, Lout), dtype=th.float32, device=dev) if gate is not None else None
        res = fuse and residual and Lout == L
        y = th.empty((B, Lout, H), dtype=th.float32, device=dev)
        arg = th.empty((B, Lout, H), dtype=th.uint8, device=dev)
        _lib.check(lib.dmp_cnn_fwd(x.data_ptr(), B, L, H, wt.data_ptr(), bias.detach().contiguous().data_ptr(), k, pad, pk, pp, 1,
                                   float(slope), _lib.ptr(g_in), int(fuse), _lib.ptr(x if res else None), y.data_ptr(),
                                   arg.data_ptr(), _lib.ptr(g_out), _lib.stream_ptr()), "dmp_cnn_fwd")
        ctx.save_for_backward(x, weight, arg, g_out if fuse else None)
        ctx.geo, ctx.slope, ctx.res, ctx.dims = geo, float(slope), res, (B, L, H, Lc, Lout)
        if g_out is not None:
            ctx.mark_non_differentiable(g_out)
        return y, g_out

    @staticmethod
    def backward(ctx, dy, _dg):
        from . import _lib
        lib = _lib.load()
        x, weight, arg, g = ctx.saved_tensors
        k, pad, pk, pp = ctx.geo
        B, L, H, Lc, Lout = ctx.dims
        dev = x.device
        dy = dy.contiguous()
        stream = _lib.stream_ptr()
        dC = th.empty((B, Lc, H), dtype=th.float32, device=dev)
        _lib.check(lib.dmp_cnn_route_bwd(dy.data_ptr(), _lib.ptr(g), arg.data_ptr(), B, Lc, Lout, H, pk, pp, ctx.slope,
                                         dC.data_ptr(), stream), "dmp_cnn_route_bwd")
        dx = None
        if ctx.needs_input_grad[0]:
            w2t = weight.detach().flip(2).permute(2, 0, 1).contiguous()   # W2t[j][o][i] = W[o, i, k - 1 - j]
            dx = th.empty((B, L, H), dtype=th.float32, device=dev)
            _lib.check(lib.dmp_cnn_fwd(dC.data_ptr(), B, Lc, H, w2t.data_ptr(), None, k, k - 1 - pad, 1, 0, 0, 0.0, None, 0,
                                       _lib.ptr(dy if ctx.res else None), dx.data_ptr(), None, None, stream), "dmp_cnn_fwd (dX)")
        dw = db = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            chunks = int(lib.dmp_cnn_wgrad_chunks(B * Lc))
            width = k * H * H + H
            part = th.empty((chunks, width), dtype=th.float32, device=dev)
            _lib.check(lib.dmp_cnn_wgrad(dC.data_ptr(), x.data_ptr(), B, L, Lc, H, k, pad, part.data_ptr(), stream), "dmp_cnn_wgrad")
            red = th.empty(width, dtype=th.float32, device=dev)
            _lib.check(lib.dmp_reduce_partials(part.data_ptr(), chunks, width, red.data_ptr(), 0, stream), "dmp_reduce_partials")
            dw = red[:k * H * H].view(k, H, H).permute(1, 2, 0).contiguous()    # [k][o][i] -> [o, i, k]
            db = red[k * H * H:].clone()
        return dx, dw, db, None, None, None, None, None


def cnn_layer_hip(layer, x, gate, residual):
    """``CNNLayer.forward_rows`` on the kernels: (out [B, L', H], gate after the layer or None)."""
    geo = _geometry(layer)
    slope = _act_slope(layer)
    if layer.bn is None:
        return CNNLayerHIP.apply(x, layer.conv.weight, layer.conv.bias, gate, geo, slope, True, residual)
    p, g = CNNLayerHIP.apply(x, layer.conv.weight, layer.conv.bias, gate, geo, slope, False, residual)
    B, Lout, H = p.shape
    bn = layer.bn
    track = bn.training and bn.track_running_stats
    if track and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    momentum = 0.0 if bn.momentum is None else bn.momentum
    if track and bn.momentum is None:
        momentum = 1.0 / float(bn.num_batches_tracked)
    o = F.batch_norm(p.reshape(B * Lout, H), bn.running_mean if (not bn.training or bn.track_running_stats) else None,
                     bn.running_var if (not bn.training or bn.track_running_stats) else None, bn.weight, bn.bias,
                     bn.training or not bn.track_running_stats, momentum, bn.eps).view(B, Lout, H)
    o = layer.drop(o)
    if g is not None:
        o = o * g.unsqueeze(-1)
    if residual and o.size() == x.size():
        o = x + o
    return o, g

