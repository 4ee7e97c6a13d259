"""Fixed encodings and learned embeddings of the model skeleton -- same classes, shapes and
initialisers as ``SubgraphCountingMatching/models/embed.py`` (the numba helpers restated in
numpy; they only run at construction time)."""
import numpy as np
import torch as th
import torch.nn as nn

from . import ops


def get_enc_len(x, base=10):
    """embed.py:8-35: number of base-``base`` digits of x (at least 1)."""
    def one(n):
        n, cnt = int(n), 0
        while n > 0:
            n //= base
            cnt += 1
        return max(cnt, 1)
    if isinstance(x, (int, float, np.integer)):
        return one(x)
    arr = np.asarray(x).astype(np.int64)
    return np.array([one(v) for v in arr.reshape(-1)], dtype=np.int64).reshape(arr.shape)


def int2multihot(x, len_x, base=10):
    """embed.py:70-100: per digit position a one-hot of size ``base`` (most significant first;
    leading positions encode digit 0)."""
    arr = np.atleast_1d(np.asarray(x)).astype(np.int64)
    rep = np.zeros((len(arr), len_x * base), dtype=np.int64)
    for i, n in enumerate(arr):
        n = int(n) % base ** len_x
        idx = (len_x - 1) * base
        while n:
            rep[i, idx + n % base] = 1
            n //= base
            idx -= base
        while idx >= 0:
            rep[i, idx] = 1
            idx -= base
    return rep


def lookup_rows(nets, ids):
    """``[net(i) for net, i in zip(nets, ids)]`` for index inputs.  Frozen fp32 tables on the device (the multi-hot /
    position encodings, embed.py:199-224): ONE launch for all of them (csrc/dmp_graph.hip::table_rows_k) instead
    of one gather each; anything else goes through the modules."""
    from . import _abi, _lib
    ok = len(nets) <= _abi.DMP_LOOKUP_MAX_JOBS and all(
        isinstance(n, nn.Embedding) and n.padding_idx is None and n.max_norm is None and not n.weight.requires_grad
        and n.weight.is_cuda and n.weight.dtype == th.float32 and n.weight.stride(1) == 1
        and i.dtype == th.long and i.is_cuda and i.dim() == 1 for n, i in zip(nets, ids))
    if not ok:
        return [n(i) for n, i in zip(nets, ids)]
    lib = _lib.load()
    J, keep, outs = (_abi.dmp_lookup_job * len(nets))(), [], []
    for k, (n, i) in enumerate(zip(nets, ids)):
        w, i = n.weight.detach(), i.contiguous()
        out = th.empty((i.numel(), w.size(1)), dtype=th.float32, device=w.device)
        J[k].table, J[k].ld, J[k].table_rows, J[k].width = w.data_ptr(), w.stride(0), w.size(0), w.size(1)
        J[k].idx, J[k].rows, J[k].out = i.data_ptr(), i.numel(), out.data_ptr()
        keep.append((w, i))
        outs.append(out)
    _lib.check(lib.dmp_table_rows(J, len(nets), _lib.stream_ptr()), "dmp_table_rows")
    return outs


class Embedding(nn.Embedding):
    """embed.py:103-120: index lookup for long inputs, ``x @ weight`` for float encodings."""

    def forward(self, x):
        if x.dtype == th.long:
            return super(Embedding, self).forward(x)
        if x.dtype == th.float and x.size(-1) == self.num_embeddings:
            x_size = x.size()
            # x @ weight; the weight gradient x^T dOut has K = #rows (5e5 edges): split-K product
            x2d = x.view(-1, x_size[-1])
            emb = ops.matmul_xw(x2d, self.weight).view(x_size[:-1] + (self.embedding_dim,))
            # where the embedding came from: a consumer that gates the rows (the joint rep-net pass) can then
            # produce the weight gradient in one pass over its own upstream gradient (fused.smallk_atb)
            emb._dmp_src = (x2d, self.weight)
            return emb
        raise NotImplementedError

    def get_output_dim(self):
        return self.embedding_dim


class DeferredEmbedding:
    """``net(enc)`` (a label embedding ``enc @ weight``) that has not been computed.  The joint rep-net pass builds its
    gated input rows straight from the encodings (``dmpnn._GateConcat``), so the [rows, hid] embedding tensor is only needed
    if somebody reads it (``OutputDict["g_e_emb"]``, a fallback path): ``materialize()`` runs the module then -- same
    values, same autograd history.  At BASELINE config 2 the target edge embedding is a 268 MB write per step."""

    def __init__(self, net, enc):
        self.net, self.enc, self._value = net, enc, None
        x2d = enc.view(-1, enc.size(-1))
        self._dmp_src = (x2d, net.weight)
        self.shape = th.Size((x2d.size(0), net.embedding_dim))
        self.dtype, self.device, self.is_cuda = net.weight.dtype, net.weight.device, net.weight.is_cuda

    def size(self, i=None):
        return self.shape if i is None else self.shape[i]

    def dim(self):
        return 2

    def materialize(self):
        if self._value is None:
            self._value = self.net(self.enc)
        return self._value


class DeferredRows:
    """A [rows, width] tensor that is computed (by ``fn``, once) only if somebody reads it -- the edge representation of the
    LAST rep-net layer under sum / mean pooling heads: the heads read per-graph sums, which the layer produces without ever
    forming the rows (``fused._FusedDMPLayer``, ``edge_rows=False``); ``OutputDict["g_e_rep"]`` and friends still deliver the
    rows, differentiable, by running the layer's ordinary form on first access."""

    def __init__(self, fn, shape, dtype, device):
        self._fn, self._value = fn, None
        self.shape, self.dtype, self.device, self.is_cuda = th.Size(shape), dtype, device, device.type == "cuda"

    def size(self, i=None):
        return self.shape if i is None else self.shape[i]

    def dim(self):
        return len(self.shape)

    def materialize(self):
        if self._value is None:
            self._value = self._fn()
            self._fn = None
        return self._value


def materialize(t):
    """The tensor behind ``t`` (a tensor, None, a ``DeferredEmbedding`` or ``DeferredRows``)."""
    return t.materialize() if isinstance(t, (DeferredEmbedding, DeferredRows)) else t


def _zero_pad(emb):
    if emb.padding_idx is not None:
        with th.no_grad():
            emb.weight[emb.padding_idx].fill_(0)


class NormalEmbedding(Embedding):
    def __init__(self, num_embeddings, embedding_dim, **kw):
        super(NormalEmbedding, self).__init__(num_embeddings, embedding_dim, **kw)
        nn.init.normal_(self.weight, 0.0, 1.0)
        _zero_pad(self)


class UniformEmbedding(Embedding):
    def __init__(self, num_embeddings, embedding_dim, **kw):
        super(UniformEmbedding, self).__init__(num_embeddings, embedding_dim, **kw)
        nn.init.uniform_(self.weight, -1.0, 1.0)
        _zero_pad(self)


class OrthogonalEmbedding(Embedding):
    def __init__(self, num_embeddings, embedding_dim, **kw):
        super(OrthogonalEmbedding, self).__init__(num_embeddings, embedding_dim, **kw)
        nn.init.orthogonal_(self.weight)
        _zero_pad(self)


class EquivariantEmbedding(Embedding):
    """embed.py:162-196: rows are rolls of one learned vector; ``weight`` and ``row_vec`` are both
    Parameters, as in the reference."""

    def __init__(self, num_embeddings, embedding_dim, **kw):
        super(EquivariantEmbedding, self).__init__(num_embeddings, embedding_dim, **kw)
        self.row_vec = nn.Parameter(th.empty(self.embedding_dim))
        nn.init.normal_(self.row_vec, 0.0, 1.0)
        with th.no_grad():
            for i in range(num_embeddings):
                self.weight[i].copy_(th.roll(self.row_vec, i, 0))


class MultihotEmbedding(Embedding):
    """embed.py:199-210: frozen multi-hot code table ``[max_n, 2 * enc_len]``."""

    def __init__(self, max_n=1024, base=2):
        self.max_n, self.base = max_n, base
        enc_len = int(get_enc_len(max_n - 1, base))
        super(MultihotEmbedding, self).__init__(max_n, 2 * enc_len)
        with th.no_grad():
            self.weight.copy_(th.from_numpy(int2multihot(np.arange(0, max_n), enc_len, base)).float())

    def extra_repr(self):
        return "base=%d, max_n=%d, enc_dim=%d" % (self.base, self.max_n, self.weight.shape[1])


class PositionEmbedding(Embedding):
    """embed.py:213-224: frozen sinusoid table."""

    def __init__(self, embedding_dim, max_len=512, scale=1):
        freq_seq = th.arange(0, embedding_dim, 2.0, dtype=th.float)
        inv_freq = th.pow(10000, (freq_seq / embedding_dim)).reciprocal()
        sinusoid_inp = th.outer(th.arange(0, max_len, 1.0), inv_freq)
        super(PositionEmbedding, self).__init__(max_len, embedding_dim)
        with th.no_grad():
            self.weight.copy_(th.cat([th.sin(sinusoid_inp), th.cos(sinusoid_inp)], dim=-1) * scale)
