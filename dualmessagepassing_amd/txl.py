"""The Transformer-XL rep-net layer (``SubgraphCountingMatching/models/txl.py:18-209``) and its relative-position
attention on the HIP kernels of ``csrc/dmp_txl.hip``.

``rel_attention`` is the core of ``TXLAttn.forward`` as the model runs it (``encoder_forward``: the attention mask is all
ones, so nothing is masked).  Per sequence and head, with ``m = klen - qlen``::

    BD[i, p] = (Q_i + r_r_bias) . R_p          S[i, j] = scale * ((Q_i + r_w_bias) . K_j + shift(BD)[i, j])
    P = softmax_j S                            O = P V

``shift`` is the reference's ``rel_shift``, the pad-and-reshape trick WITHOUT the causal mask that normally hides its
wrap-around, so the wrapped entries take part (``rel_shift`` below is its closed form, ``rel_shift_pad`` the trick)::

    j - i <  m + 1:  BD[i, qlen - 1 - i + j]       j - i == m + 1:  0       j - i > m + 1:  BD[i + 1, j - i - m - 2]

Two implementations of one function:

* ``RelAttention`` -- fp32 on the GPU, shapes ``dmp_txl_supported`` admits (qlen <= 64, qlen <= klen <= 128, head width
  16, 32, 64 or 128): one autograd node, one launch forward (no ``[N, q, k, heads]`` tensor; it keeps each row's maximum
  and sum) and one launch plus a fixed-order reduction backward (dQ, dK, dV, dR and the two bias gradients; no float
  atomics, two runs are bitwise equal).
* ``rel_attention_tensor`` -- the same function in tensor ops: the CPU path, other shapes, and dropout on the attention
  weights in training, which the kernels do not do.
"""
import torch as th
import torch.nn as nn
import torch.nn.functional as F

from .act import init_module, map_activation_str_to_layer

_SHIFT_INDEX = {}


def shift_index(qlen, klen, device):
    """(src [qlen * klen] int64, zero [qlen * klen] bool): shift(BD).flatten()[e] = BD.flatten()[src[e]], 0 where zero."""
    key = (qlen, klen, str(device))
    if key not in _SHIFT_INDEX:
        i = th.arange(qlen).view(-1, 1)
        j = th.arange(klen).view(1, -1)
        m = klen - qlen
        d = j - i
        same = i * klen + (qlen - 1 - i + j)
        wrap = (i + 1) * klen + (d - m - 2)
        src = th.where(d < m + 1, same, th.where(d > m + 1, wrap, th.zeros_like(same)))
        _SHIFT_INDEX[key] = (src.reshape(-1).to(device), (d == m + 1).reshape(-1).to(device))
    return _SHIFT_INDEX[key]


def rel_shift(bd):
    """bd [N, qlen, klen, heads] -> shift(bd), by the closed form above."""
    N, qlen, klen, nh = bd.shape
    src, zero = shift_index(qlen, klen, bd.device)
    out = bd.reshape(N, qlen * klen, nh).index_select(1, src).masked_fill(zero.view(1, -1, 1), 0.0)
    return out.view(N, qlen, klen, nh)


def rel_shift_pad(bd):
    """The same by the pad-and-reshape trick (txl.py:95-108): a zero column in front of the key axis, the [qlen, klen + 1]
    block read as [klen + 1, qlen], its first row dropped, the rest read as [qlen, klen]."""
    N, qlen, klen, nh = bd.shape
    padded = F.pad(bd, (0, 0, 1, 0))
    return padded.view(N, klen + 1, qlen, nh)[:, 1:].reshape(N, qlen, klen, nh)


def rel_attention_tensor(q, k, v, r, r_w_bias, r_r_bias, scale, drop=None, shift=rel_shift):
    """q [N, qlen, heads, dh], k / v [N, klen, heads, dh], r [klen, heads, dh], biases [heads, dh] -> [N, qlen, heads * dh]."""
    ac = th.einsum("bind,bjnd->bijn", q + r_w_bias, k)
    bd = shift(th.einsum("bind,jnd->bijn", q + r_r_bias, r))
    p = F.softmax((ac + bd) * scale, dim=2)
    if drop is not None:
        p = drop(p)
    return th.einsum("bijn,bjnd->bind", p, v).reshape(q.size(0), q.size(1), -1)


def fwd_bytes(N, ql, kl, nh, dh):
    """Bytes the forward must move: Q, K, V in, O and the two row statistics out, R and the biases once."""
    return 4 * (N * (2 * ql + 2 * kl) * nh * dh + 2 * N * nh * ql + (kl + 2) * nh * dh)


def bwd_bytes(N, ql, kl, nh, dh, groups):
    """Q, K, V, dO and the row statistics in, dQ, dK, dV out, and the partials of dR and the bias gradients written once by
    their workgroup and read once by the reduction."""
    return 4 * (N * (4 * ql + 4 * kl) * nh * dh + 2 * N * nh * ql + (2 * groups + 2) * (kl + 2) * nh * dh)


class RelAttention(th.autograd.Function):
    """The kernels of csrc/dmp_txl.hip as one autograd node; S is recomputed in the backward."""

    @staticmethod
    def forward(ctx, q, k, v, r, r_w_bias, r_r_bias, scale):
        from . import _lib
        from .attn import _out
        lib = _lib.load()
        q, k, v, r = q.contiguous(), k.contiguous(), v.contiguous(), r.contiguous()
        bw, br = r_w_bias.contiguous(), r_r_bias.contiguous()
        _lib.require_gpu(q, k, v, r, bw, br)
        N, ql, nh, dh = q.shape
        kl = k.size(1)
        o = _out((N, ql, nh * dh), th.float32, q.device)
        mx, sm = _out((N, nh, ql), th.float32, q.device), _out((N, nh, ql), th.float32, q.device)
        with _lib.timed("txl_attn_fwd q%d k%d nh%d dh%d", (ql, kl, nh, dh), fwd_bytes(N, ql, kl, nh, dh)):
            _lib.check(lib.dmp_txl_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), r.data_ptr(), bw.data_ptr(), br.data_ptr(), N, ql,
                                            kl, nh, dh, float(scale), o.data_ptr(), mx.data_ptr(), sm.data_ptr(), _lib.stream_ptr()),
                       "dmp_txl_attn_fwd")
        ctx.save_for_backward(q, k, v, r, bw, br, mx, sm)
        ctx.scale = float(scale)
        return o

    @staticmethod
    def backward(ctx, do):
        from . import _lib
        from .attn import _out
        lib = _lib.load()
        q, k, v, r, bw, br, mx, sm = ctx.saved_tensors
        N, ql, nh, dh = q.shape
        kl = k.size(1)
        do = do.contiguous()
        dev = q.device
        groups = lib.dmp_txl_bwd_groups(N, nh)
        partial = _out((groups, kl + 2, nh, dh), th.float32, dev)
        red = _out((kl + 2, nh, dh), th.float32, dev)            # rows: dR [klen], d r_w_bias, d r_r_bias
        dq, dk, dv = _out(q.shape, th.float32, dev), _out(k.shape, th.float32, dev), _out(v.shape, th.float32, dev)
        with _lib.timed("txl_attn_bwd q%d k%d nh%d dh%d", (ql, kl, nh, dh), bwd_bytes(N, ql, kl, nh, dh, groups)):
            _lib.check(lib.dmp_txl_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), r.data_ptr(), bw.data_ptr(), br.data_ptr(),
                                            do.data_ptr(), mx.data_ptr(), sm.data_ptr(), N, ql, kl, nh, dh, ctx.scale, dq.data_ptr(),
                                            dk.data_ptr(), dv.data_ptr(), partial.data_ptr(), _lib.stream_ptr()), "dmp_txl_attn_bwd")
            _lib.check(lib.dmp_reduce_partials(partial.data_ptr(), groups, (kl + 2) * nh * dh, red.data_ptr(), 0, _lib.stream_ptr()),
                       "dmp_reduce_partials")
        return dq, dk, dv, red[:kl], red[kl], red[kl + 1], None


def kernel_ok(q, k, v, r, r_w_bias, r_r_bias):
    """The HIP kernels take these inputs: fp32 on one GPU, a shape ``dmp_txl_supported`` admits, at least one sequence."""
    ts = (q, k, v, r, r_w_bias, r_r_bias)
    if not all(t.is_cuda and t.dtype == th.float32 and t.device == q.device for t in ts):
        return False
    if q.dim() != 4 or q.size(0) < 1 or q.size(0) * q.size(2) >= (1 << 31):
        return False
    from . import _lib
    return bool(_lib.load().dmp_txl_supported(q.size(1), k.size(1), q.size(3)))


def rel_attention(q, k, v, r, r_w_bias, r_r_bias, scale, drop=None):
    """``softmax(scale ((q + r_w_bias) k^T + shift((q + r_r_bias) r^T))) v`` per sequence and head.  ``drop``: the module applied
    to the attention weights; while it is active the tensor ops run (the kernels have no dropout)."""
    if drop is not None and not (drop.training and drop.p > 0):
        drop = None
    if drop is None and kernel_ok(q, k, v, r, r_w_bias, r_r_bias):
        return RelAttention.apply(q, k, v, r, r_w_bias, r_r_bias, scale)
    return rel_attention_tensor(q, k, v, r, r_w_bias, r_r_bias, scale, drop)


class TXLFF(nn.Module):
    """txl.py:18-58: Linear, activation, Linear around a residual and a LayerNorm (before or after).  With ``pre_lnorm`` the
    residual adds the NORMALISED input, as the reference does."""

    def __init__(self, input_dim, hid_dim, act_func="relu", dropout=0.0, pre_lnorm=False):
        super(TXLFF, self).__init__()
        self.input_dim = input_dim
        self.hid_dim = hid_dim
        self.pre_lnorm = pre_lnorm
        self.layer1 = nn.Linear(input_dim, hid_dim)
        self.layer2 = nn.Linear(hid_dim, input_dim)
        self.act = map_activation_str_to_layer(act_func)
        self.drop = nn.Dropout(dropout)
        self.layer_norm = nn.LayerNorm(input_dim)
        init_module(self.layer1, activation=act_func, init="normal")
        init_module(self.layer2, init="normal")

    def forward(self, x):
        if self.pre_lnorm:
            x = self.layer_norm(x)
        o = self.drop(self.layer2(self.drop(self.act(self.layer1(x))))) + x
        return o if self.pre_lnorm else self.layer_norm(o)

    def get_output_dim(self):
        return self.input_dim


class TXLAttn(nn.Module):
    """txl.py:61-183.  ``seg_len`` / ``ext_len`` / ``mem_len`` are accepted and unused, as in the reference."""

    def __init__(self, input_dim, hid_dim, num_heads=1, dropout=0.0, seg_len=None, ext_len=None, mem_len=None, pre_lnorm=False):
        super(TXLAttn, self).__init__()
        self.input_dim = input_dim
        self.hid_dim = hid_dim
        self.num_heads = num_heads
        self.scale = 1 / ((hid_dim / num_heads) ** 0.5)
        self.pre_lnorm = pre_lnorm
        self.drop = nn.Dropout(dropout)
        self.q_net = nn.Linear(input_dim, hid_dim, bias=False)
        self.k_net = nn.Linear(input_dim, hid_dim, bias=False)
        self.v_net = nn.Linear(input_dim, hid_dim, bias=False)
        self.r_net = nn.Linear(input_dim, hid_dim, bias=False)
        self.o_net = nn.Linear(input_dim, hid_dim)
        self.layer_norm = nn.LayerNorm(input_dim)
        for net in (self.q_net, self.k_net, self.v_net, self.r_net, self.o_net):
            init_module(net, init="normal")

    def forward(self, w, r, r_w_bias, r_r_bias, mems=None):
        """w [B, qlen, H]; r [1, klen, H] position rows (klen - 1 down to 0); mems [B, mlen, H] or None: klen = mlen + qlen."""
        bsz, qlen = w.size(0), w.size(1)
        residual = w
        c = th.cat([mems, w], dim=1) if mems is not None and mems.size(1) > 0 else w
        klen = c.size(1)
        if self.pre_lnorm:
            w = self.layer_norm(w)
            c = w if c is residual else self.layer_norm(c)
        nh = self.num_heads
        r_k = self.r_net(r).view(klen, nh, -1)
        q = self.q_net(w).view(bsz, qlen, nh, -1)
        k = self.k_net(c).view(bsz, klen, nh, -1)
        v = self.v_net(c).view(bsz, klen, nh, -1)
        vec = rel_attention(q, k, v, r_k, r_w_bias, r_r_bias, self.scale, self.drop)
        out = self.drop(self.o_net(vec)) + residual
        return out if self.pre_lnorm else self.layer_norm(out)

    def get_output_dim(self):
        return self.input_dim


class TXLLayer(nn.Module):
    """txl.py:186-209."""

    def __init__(self, input_dim, hid_dim, num_heads, dropout=0.0, act_func="relu", pre_lnorm=False):
        super(TXLLayer, self).__init__()
        self.attn = TXLAttn(input_dim, hid_dim, num_heads=num_heads, dropout=dropout, pre_lnorm=pre_lnorm)
        self.ff = TXLFF(input_dim, hid_dim, act_func=act_func, dropout=dropout, pre_lnorm=pre_lnorm)

    def forward(self, x, r, r_w_bias, r_r_bias, mems=None):
        return self.ff(self.attn(x, r, r_w_bias, r_r_bias, mems=mems))

    def get_output_dim(self):
        return self.ff.get_output_dim()


class RepNetDict(nn.Module):
    """The reference's ``MixtureDict`` (models/container.py) as far as the TXL rep-net uses it: modules under ``_module_dict``,
    parameters under ``_param_dict`` (hence the ``state_dict`` keys), both reached by ``net[key]``; ``len`` counts every entry."""

    def __init__(self, entries):
        super(RepNetDict, self).__init__()
        self._module_dict = nn.ModuleDict()
        self._param_dict = nn.ParameterDict()
        for key, value in entries.items():
            if isinstance(value, nn.Parameter):
                self._param_dict[key] = value
            else:
                self._module_dict[key] = value

    def __getitem__(self, key):
        if key in self._param_dict:
            return self._param_dict[key]
        return self._module_dict[key]

    def __len__(self):
        return len(self._param_dict) + len(self._module_dict)

    def __contains__(self, key):
        return key in self._param_dict or key in self._module_dict
