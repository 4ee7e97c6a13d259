"""The UNC baseline encoders R-GCN and R-GIN (UnsupervisedNodeClassification/Model/{R-GCN,R-GIN}/src/model.py) on the
MI355X kernels, with their operator, DGL 0.6's ``RelGraphConv`` (regularizer "basis").

    W_r   = weight[r]                                  (num_bases == R)
          = (w_comp @ weight.view(B, in * out))[r]      (num_bases  < R)
    agg_v = sum_{e: dst e = v} norm_e x[src e] W_{t_e}  (norm_e = 1 without a norm)
    out   = dropout(act(agg + h_bias + x loop_weight))

Transform, then aggregate: ``Y = x @ W_cat`` with ``W_cat = [W_0 | ... | W_{R-1} | loop_weight]`` (every block padded to a
multiple of 4 columns) is one GEMM, and ``dmp_relconv_fwd`` sums the typed source rows of ``Y`` over the in-CSR and adds the
bias, the self-loop block and tanh in the same launch.  Its backward ``dmp_relconv_bwd`` runs over the out-CSR and returns
``dY``; the two GEMMs of ``Y = x @ W_cat`` and the small tensor ops that form ``W_cat`` carry the gradient on to ``x``,
``weight``, ``w_comp`` and ``loop_weight``.  No host sync anywhere, so a sampled step records (``unc_harness.SampledStep``).
Shapes the kernels refuse (``dmp_relconv_supported``), and CPU tensors, take the same arithmetic as tensor ops.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib, ops
from ._lib import check, on_input_device, ptr, stream_ptr
from .graph import as_batched
from .unc import EmbeddingLayer, EmbeddingLayerAttri

ACT_NONE, ACT_TANH = 0, 1


def padded_width(out_feat):
    """Columns of one block of ``W_cat``: ``out_feat`` rounded up to 4 floats, so every gathered row segment is 16-byte aligned."""
    return (int(out_feat) + 3) // 4 * 4


class _RelAgg(torch.autograd.Function):
    """``out = act(sum_e norm_e Y[src e, t_e] + bias + Y[v, R])`` on ``dmp_relconv_fwd`` / ``dmp_relconv_bwd``."""

    @staticmethod
    def forward(ctx, Y, bias, ix, etype, norm, R, loop, H, P, act):
        lib = _lib.load()
        _lib.require_gpu(Y, bias, etype, norm)
        N = ix.num_nodes
        out = torch.empty(N, H, dtype=torch.float32, device=Y.device)
        check(lib.dmp_relconv_fwd(ptr(Y), ptr(ix.in_ptr), ptr(ix.in_ent), ptr(ix.src32), ptr(etype), ptr(norm), ptr(bias), N, R,
                                  loop, H, P, act, ptr(out), stream_ptr()), "dmp_relconv_fwd")
        ctx.ix, ctx.etype, ctx.norm = ix, etype, norm
        ctx.shape = (R, loop, H, P, act)
        ctx.has_bias = bias is not None
        ctx.save_for_backward(out if act == ACT_TANH else None)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        lib = _lib.load()
        (out,) = ctx.saved_tensors
        R, loop, H, P, act = ctx.shape
        ix = ctx.ix
        N = ix.num_nodes
        dout = dout.contiguous()
        dY = torch.empty(N, (R + loop) * P, dtype=torch.float32, device=dout.device)
        check(lib.dmp_relconv_bwd(ptr(dout), ptr(out), ptr(ix.out_ptr), ptr(ix.out_ent), ptr(ix.dst32), ptr(ctx.etype), ptr(ctx.norm),
                                  N, R, loop, H, P, act, ptr(dY), stream_ptr()), "dmp_relconv_bwd")
        dbias = None
        if ctx.has_bias and ctx.needs_input_grad[1]:
            # g = dOut act'(out) is the self-loop block of dY when there is one; a fixed-order column sum either way
            g = dY.view(N, R + loop, P)[:, R, :H] if loop else (dout * (1 - out * out) if act == ACT_TANH else dout)
            dbias = g.sum(0)
        return dY, dbias, None, None, None, None, None, None, None, None


def rel_conv_tensor_ops(Y, bias, src, dst, etype, norm, N, R, loop, H, P):
    """The same arithmetic as tensor ops (CPU, and the shapes the kernels refuse): pre-activation [N, H]."""
    Yv = Y.view(N, R + loop, P)
    msg = Yv[src, etype.view(-1)][:, :H]
    if norm is not None:
        msg = msg * norm.view(-1, 1)
    out = torch.zeros(N, H, dtype=Y.dtype, device=Y.device).index_add_(0, dst, msg)
    if bias is not None:
        out = out + bias
    if loop:
        out = out + Yv[:, R, :H]
    return out


class RelGraphConv(nn.Module):
    """DGL 0.6 ``dgl.nn.pytorch.RelGraphConv`` with ``regularizer="basis"``: constructor arguments, parameter names, shapes and
    initialisation as there; ``forward(g, feat, etypes, norm=None)``.  ``norm`` (or ``g.edata["norm"]``, as DGL's message
    function reads it) scales the messages.  ``regularizer="bdd"``, ``layer_norm=True`` and integer node-id input raise."""

    def __init__(self, in_feat, out_feat, num_rels, regularizer="basis", num_bases=None, bias=True, activation=None, self_loop=True,
                 low_mem=False, dropout=0.0, layer_norm=False):
        super(RelGraphConv, self).__init__()
        if regularizer != "basis":
            raise NotImplementedError("RelGraphConv: only regularizer='basis' is built (the reference uses no other)")
        if layer_norm:
            raise NotImplementedError("RelGraphConv: layer_norm=True is not built (the reference does not use it)")
        self.in_feat, self.out_feat, self.num_rels = int(in_feat), int(out_feat), int(num_rels)
        self.regularizer = regularizer
        self.num_bases = num_bases
        if self.num_bases is None or self.num_bases > self.num_rels or self.num_bases <= 0:
            self.num_bases = self.num_rels
        self.bias, self.activation, self.self_loop = bias, activation, self_loop
        self.low_mem, self.layer_norm = low_mem, layer_norm
        # DGL 0.6 relgraphconv.py: the basis weights (and their coefficients), then the bias, then the self-loop weight
        self.weight = nn.Parameter(torch.Tensor(self.num_bases, self.in_feat, self.out_feat))
        if self.num_bases < self.num_rels:
            self.w_comp = nn.Parameter(torch.Tensor(self.num_rels, self.num_bases))
        nn.init.xavier_uniform_(self.weight, gain=nn.init.calculate_gain("relu"))
        if self.num_bases < self.num_rels:
            nn.init.xavier_uniform_(self.w_comp, gain=nn.init.calculate_gain("relu"))
        if self.bias:
            self.h_bias = nn.Parameter(torch.Tensor(self.out_feat))
            nn.init.zeros_(self.h_bias)
        if self.self_loop:
            self.loop_weight = nn.Parameter(torch.Tensor(self.in_feat, self.out_feat))
            nn.init.xavier_uniform_(self.loop_weight, gain=nn.init.calculate_gain("relu"))
        self.dropout = nn.Dropout(dropout)

    def relation_weights(self):
        """``[R, in, out]``: the basis weights, or their combination by ``w_comp``."""
        if self.num_bases < self.num_rels:
            w = self.weight.view(self.num_bases, self.in_feat * self.out_feat)
            return torch.matmul(self.w_comp, w).view(self.num_rels, self.in_feat, self.out_feat)
        return self.weight

    def stacked_weight(self, P):
        """``W_cat [in, (R + loop) P]``: the relation blocks then the self-loop block, each padded with zero columns to P."""
        blocks = self.relation_weights()
        if self.self_loop:
            blocks = torch.cat([blocks, self.loop_weight.unsqueeze(0)], 0)
        if P != self.out_feat:
            blocks = nn.functional.pad(blocks, (0, P - self.out_feat))
        return blocks.permute(1, 0, 2).reshape(self.in_feat, -1)

    def conv(self, g, feat, etypes, norm=None):
        """act(agg + h_bias + loop message), before the dropout."""
        if feat.dtype == torch.int64 and feat.dim() == 1:
            raise NotImplementedError("RelGraphConv: integer node-id input is not built (the reference does not use it)")
        g = as_batched(g)
        if norm is None:
            norm = g.edata.get("norm")
        if isinstance(etypes, (list, tuple)) or etypes.numel() != g.number_of_edges():
            raise ValueError("RelGraphConv: etypes must be a tensor with one entry per edge")
        if norm is not None and norm.numel() != g.number_of_edges():
            raise ValueError("RelGraphConv: norm must have one entry per edge")
        if feat.dim() != 2 or feat.size(0) != g.number_of_nodes() or feat.size(1) != self.in_feat:
            raise ValueError("RelGraphConv: feat must be [num_nodes, in_feat]")
        R, loop, H = self.num_rels, int(bool(self.self_loop)), self.out_feat
        P = padded_width(H)
        bias = self.h_bias if self.bias else None
        act = ACT_TANH if isinstance(self.activation, nn.Tanh) else ACT_NONE
        Y = ops.matmul_xw(feat, self.stacked_weight(P))
        N = g.number_of_nodes()
        if (feat.is_cuda and feat.dtype == torch.float32 and (norm is None or not norm.requires_grad)
                and _lib.load().dmp_relconv_supported(R, P)):
            nrm = None if norm is None else norm.reshape(-1).to(torch.float32).contiguous()
            out = _RelAgg.apply(Y.contiguous(), bias, g.index(), etypes.reshape(-1).to(torch.int64).contiguous(), nrm, R, loop, H, P, act)
        else:
            src, dst = g.all_edges(form="uv", order="eid")
            out = rel_conv_tensor_ops(Y, bias, src, dst, etypes, norm, N, R, loop, H, P)
            if act == ACT_TANH:
                out = torch.tanh(out)
        if self.activation is not None and act == ACT_NONE:
            out = self.activation(out)
        return out

    @on_input_device
    def forward(self, g, feat, etypes, norm=None):
        return self.dropout(self.conv(g, feat, etypes, norm))

    def extra_repr(self):
        return "in=%d, out=%d, num_rels=%d, num_bases=%d, self_loop=%s" % (self.in_feat, self.out_feat, self.num_rels,
                                                                           self.num_bases, self.self_loop)


class RelGraphIso(RelGraphConv):
    """R-GIN's layer (R-GIN/src/model.py:117-157): RelGraphConv without a norm, then ``out_layer`` (Linear out -> out), the
    activation again and the dropout again."""

    def __init__(self, in_feat, out_feat, num_rels, regularizer="basis", num_bases=None, bias=True, activation=None, self_loop=True,
                 low_mem=False, dropout=0.0, layer_norm=False):
        super().__init__(in_feat, out_feat, num_rels, regularizer=regularizer, num_bases=num_bases, bias=bias, activation=activation,
                         self_loop=self_loop, low_mem=low_mem, dropout=dropout, layer_norm=layer_norm)
        self.out_layer = nn.Linear(out_feat, out_feat)
        nn.init.xavier_uniform_(self.out_layer.weight, gain=nn.init.calculate_gain("relu"))
        nn.init.zeros_(self.out_layer.bias)

    @on_input_device
    def forward(self, g, feat, etypes, norm=None):
        # super().forward(g, feat, etypes, norm=None): DGL still reads a norm left on the graph -- the model pops it first
        o = self.dropout(self.conv(g, feat, etypes, None))
        o = self.out_layer(o)
        if self.activation:
            o = self.activation(o)
        return self.dropout(o)


class _RelEncoder(nn.Module):
    """``BaseModel`` of the reference with ``build_input_layer`` = the node table only (``rel_emb`` None) and
    ``num_hidden_layers`` relational layers, Tanh between them and none after the last.  ``forward(g, h, r, norm)`` returns the
    node tensor itself (not a tuple)."""

    layer_cls = None

    def __init__(self, node_attri, rel_attri, num_nodes, h_dim, out_dim, num_rels, num_hidden_layers=1, dropout=0, use_cuda=False):
        super(_RelEncoder, self).__init__()
        self.num_nodes, self.h_dim, self.out_dim = num_nodes, h_dim, out_dim
        self.num_rels, self.num_hidden_layers, self.dropout, self.use_cuda = num_rels, num_hidden_layers, dropout, use_cuda
        self.node_emb = EmbeddingLayerAttri(node_attri) if node_attri is not None else EmbeddingLayer(num_nodes, h_dim)
        self.rel_emb = None
        self.layers = nn.ModuleList()
        for idx in range(num_hidden_layers):
            in_dim = h_dim if idx == 0 else out_dim
            act = nn.Tanh() if idx < num_hidden_layers - 1 else None
            self.layers.append(self._layer(in_dim, act))


class RGCN(_RelEncoder):
    """R-GCN/src/model.py:117-147: RelGraphConv(basis, num_bases -1 = R, bias, self-loop); the sub-graph's edge norm."""

    def _layer(self, in_dim, act):
        return RelGraphConv(in_dim, self.out_dim, self.num_rels, regularizer="basis", num_bases=-1, bias=True, activation=act,
                            self_loop=True, dropout=self.dropout)

    @on_input_device
    def forward(self, g, h, r, norm):
        h = self.node_emb(g, h)
        for layer in self.layers:
            h = layer(g, h, r, norm)
        return h


class RGIN(_RelEncoder):
    """R-GIN/src/model.py:160-196: RelGraphIso(basis, num_bases R); ``edata["norm"]`` is taken off the graph for the pass."""

    def _layer(self, in_dim, act):
        return RelGraphIso(in_dim, self.out_dim, self.num_rels, "basis", self.num_rels, activation=act, self_loop=True,
                           dropout=self.dropout)

    @on_input_device
    def forward(self, g, h, r, norm):
        h = self.node_emb(g, h)
        has_norm = "norm" in g.edata
        if has_norm:
            norm = g.edata.pop("norm")
        try:
            for layer in self.layers:
                h = layer(g, h, r, None)
        finally:
            if has_norm:
                g.edata["norm"] = norm
        return h
