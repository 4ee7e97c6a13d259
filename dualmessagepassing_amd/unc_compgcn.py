"""The UNC baseline encoder CompGCN (UnsupervisedNodeClassification/Model/CompGCN/src/model.py) on the MI355X kernels.

Its layer, ``CompGraphConv`` as ``CompGCN`` builds it (``comp_opt="corr"``, self loop, bias, no batch norm):

    corr(a, b)[k] = sum_i a[i] b[(i + k) mod I]                      (= irfft(conj(rfft a) rfft b))
    msg_e = norm_e corr(h[src e], r_e) @ in_weight
    out_v = act(((sum_{e -> v} msg_e) + corr(h_v, loop_rel) @ loop_weight) * 0.3333333 + bias)
    r'_e  = r_e @ rel_weight

The edge rows start as ``rel_emb[type_e]`` and every layer maps them linearly, so they only ever take ``R = 2 num_rels``
distinct values: a table ``T [R, I]`` with ``T' = T @ rel_weight``.  And the correlation is linear in its first argument,
``corr(h, t) = h @ C(t)`` with ``C(t)[i, k] = t[(i + k) mod I]``, so an edge of type b sends ``h[src] @ W_b`` with
``W_b = C(T[b]) @ in_weight`` and the self loop is one more block, ``C(loop_rel) @ loop_weight``.  That is the
transform-then-aggregate form of ``unc_rel``: ``dmp_relcorr_weights_fwd`` forms ``W_cat = 0.3333333 [W_0 | ... | W_{R-1} |
W_loop]`` in one launch, ``Y = h @ W_cat`` is one GEMM, and ``dmp_relconv_fwd`` does the typed sum, the bias, the loop
block and tanh.  The backward is ``dmp_relconv_bwd``, the GEMM's two products and ``dmp_relcorr_weights_bwd``.  No per-edge
FFT, no ``[E, I]`` composed rows, no host sync: a sampled step records (``unc_harness.SampledStep``).

An edge whose type is outside ``[0, R)`` sends no message and its row of the returned ``r`` is zero, on every path (the
kernels skip such an edge; the tensor-op path masks it).  The reference raises an IndexError in its embedding lookup
there; checking on the GPU would cost a host sync per step.

``TrainModel`` here is the reference's ``TrainModel`` of Model/CompGCN (one per model directory there too); it is not an
``encoder=`` of ``unc.TrainModel``.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib, ops, unc
from ._lib import check, on_input_device, ptr, stream_ptr
from .graph import as_batched
from .unc import EmbeddingLayer, EmbeddingLayerAttri
from .unc_rel import ACT_NONE, ACT_TANH, _RelAgg, padded_width

LOOP_SCALE = 0.3333333     # model.py:223 (not 1 / 3)


def corr(a, b):
    """model.py:192-198: ``corr(a, b)[..., k] = sum_i a[..., i] b[..., (i + k) mod I]``."""
    n = a.size(-1)
    return torch.fft.irfft(torch.conj(torch.fft.rfft(a, dim=-1)) * torch.fft.rfft(b, dim=-1), n=n, dim=-1)


def compose(a, b, comp_opt):
    if comp_opt == "sub":
        return a - b
    if comp_opt == "mult":
        return a * b
    if comp_opt == "corr":
        return corr(a, b)
    raise NotImplementedError(comp_opt)


def circulant(t):
    """``C(t)[..., i, k] = t[..., (i + k) mod I]``: ``corr(h, t) == h @ C(t)``."""
    n = t.size(-1)
    i = torch.arange(n, device=t.device)
    return t[..., (i.view(-1, 1) + i.view(1, -1)) % n]


def corr_weights_tensor_ops(T, loop_rel, Win, Wloop, P, scale):
    """``W_cat [I, (R + 1) P]`` as tensor ops: block b is ``scale C(T[b]) @ Win``, block R ``scale C(loop_rel) @ Wloop``,
    each padded with zero columns to P."""
    R, H = T.size(0), Win.size(1)
    C = circulant(torch.cat([T, loop_rel.view(1, -1)], 0))                       # [R + 1, I, I]
    blocks = torch.cat([torch.matmul(C[:R], Win), torch.matmul(C[R:], Wloop)], 0) * scale
    if P != H:
        blocks = nn.functional.pad(blocks, (0, P - H))
    return blocks.permute(1, 0, 2).reshape(T.size(1), -1)


class _RelCorrWeights(torch.autograd.Function):
    """``corr_weights_tensor_ops`` on ``dmp_relcorr_weights_fwd`` / ``dmp_relcorr_weights_bwd``: one launch each way."""

    @staticmethod
    def forward(ctx, T, loop_rel, Win, Wloop, P, scale):
        lib = _lib.load()
        _lib.require_gpu(T, loop_rel, Win, Wloop)
        T, loop_rel, Win, Wloop = T.contiguous(), loop_rel.contiguous(), Win.contiguous(), Wloop.contiguous()
        R, I, H = T.size(0), T.size(1), Win.size(1)
        Wcat = torch.empty(I, (R + 1) * P, dtype=torch.float32, device=T.device)
        check(lib.dmp_relcorr_weights_fwd(ptr(T), ptr(loop_rel), ptr(Win), ptr(Wloop), R, I, H, P, scale, ptr(Wcat), stream_ptr()),
              "dmp_relcorr_weights_fwd")
        ctx.shape = (R, I, H, P, scale)
        ctx.save_for_backward(T, loop_rel, Win, Wloop)
        return Wcat

    @staticmethod
    @once_differentiable
    def backward(ctx, dWcat):
        lib = _lib.load()
        T, loop_rel, Win, Wloop = ctx.saved_tensors
        R, I, H, P, scale = ctx.shape
        dWcat = dWcat.contiguous()
        dT, dloop, dWin, dWloop = torch.empty_like(T), torch.empty_like(loop_rel), torch.empty_like(Win), torch.empty_like(Wloop)
        check(lib.dmp_relcorr_weights_bwd(ptr(dWcat), ptr(T), ptr(loop_rel), ptr(Win), ptr(Wloop), R, I, H, P, scale, ptr(dT), ptr(dloop),
                                          ptr(dWin), ptr(dWloop), stream_ptr()), "dmp_relcorr_weights_bwd")
        return dT, dloop, dWin, dWloop, None, None


def kernels_admit(I, H, R, P):
    """The shapes both kernel families take: ``dmp_relcorr_supported`` (4 <= I, H <= 256, R + 1 <= 17) and ``dmp_relconv_supported``."""
    lib = _lib.load()
    return bool(lib.dmp_relcorr_supported(I, H, R + 1)) and bool(lib.dmp_relconv_supported(R, P))


def corr_weights(T, loop_rel, Win, Wloop, P, scale=LOOP_SCALE):
    """``W_cat``: on the kernels for fp32 GPU tensors of a shape ``kernels_admit`` takes, as tensor ops otherwise."""
    if T.is_cuda and T.dtype == torch.float32 and Win.dtype == torch.float32 and kernels_admit(T.size(1), Win.size(1), T.size(0), P):
        return _RelCorrWeights.apply(T, loop_rel, Win, Wloop, P, scale)
    return corr_weights_tensor_ops(T, loop_rel, Win, Wloop, P, scale)


class CompGraphConv(nn.Module):
    """model.py:117-264: constructor arguments, parameter names, registration order and initialisers as there.

    ``forward(graph, node_feat, edge_feat, edge_norm=None)`` with one row of ``edge_feat`` per edge is the reference's call,
    run as tensor ops for every option.  ``forward_table(graph, node_feat, rel_table, etypes, edge_norm=None)`` takes the
    ``[R, I]`` table the edge rows are drawn from instead and returns ``(node_out, rel_table @ rel_weight)``: the fast path
    of the module docstring when the layer is the one ``CompGCN`` builds, the same table algebra as tensor ops otherwise."""

    def __init__(self, input_dim, hidden_dim, self_loop=True, comp_opt="mult", bias=True, batch_norm=False, activation=None,
                 dropout=0.0):
        super(CompGraphConv, self).__init__()
        assert comp_opt in ["sub", "mult", "corr"]
        self.input_dim, self.hidden_dim, self.self_loop, self.comp_opt = input_dim, hidden_dim, self_loop, comp_opt
        self.in_weight = nn.Parameter(torch.Tensor(input_dim, hidden_dim))
        self.out_weight = nn.Parameter(torch.Tensor(input_dim, hidden_dim))
        self.rel_weight = nn.Parameter(torch.Tensor(input_dim, hidden_dim))
        if self_loop:
            self.num_rels = 3
            self.loop_weight = nn.Parameter(torch.Tensor(input_dim, hidden_dim))
            self.loop_rel = nn.Parameter(torch.Tensor(1, input_dim))
        else:
            self.num_rels = 2
            self.register_parameter("loop_weight", None)
            self.register_parameter("loop_rel", None)
        if bias:
            self.bias = nn.Parameter(torch.Tensor(hidden_dim))
        else:
            self.register_parameter("bias", None)
        self.bn = nn.BatchNorm1d(hidden_dim) if batch_norm else None
        self.act = activation
        self.drop = nn.Dropout(dropout)
        nn.init.xavier_uniform_(self.in_weight)
        nn.init.xavier_uniform_(self.out_weight)
        nn.init.xavier_uniform_(self.rel_weight)
        if self_loop:
            nn.init.xavier_uniform_(self.loop_weight)
            nn.init.xavier_uniform_(self.loop_rel)
        if bias:
            nn.init.zeros_(self.bias)

    # ---- the reference's arithmetic, edge by edge (model.py:202-240)
    def _finish(self, out):
        """model.py:229-233 after the bias: batch norm, activation, dropout."""
        if self.bn is not None:
            out = self.bn(out)
        if self.act is not None:
            out = self.act(out)
        return self.drop(out)

    def _edge_pass(self, g, node_feat, edge_rows, norm, keep=None):
        """``edge_rows`` [E, I]: one relation row per edge.  ``keep`` (0 / 1 per edge, or None): edges that send nothing."""
        src, dst = g.all_edges(form="uv", order="eid")
        comp = compose(node_feat[src], edge_rows, self.comp_opt)
        msg = torch.matmul(comp, self.in_weight)
        if "is_rev" in g.edata:
            msg = torch.where(g.edata["is_rev"].view(-1, 1).bool(), torch.matmul(comp, self.out_weight), msg)
        if norm is not None:
            msg = msg * norm.view(-1, 1)
        if keep is not None:
            msg = msg * keep.view(-1, 1)
        agg = torch.zeros(g.number_of_nodes(), self.hidden_dim, dtype=msg.dtype, device=msg.device).index_add_(0, dst, msg)
        if self.loop_weight is not None:
            out = (agg + torch.matmul(compose(node_feat, self.loop_rel, self.comp_opt), self.loop_weight)) * LOOP_SCALE
        else:
            out = agg * 0.5
        if self.bias is not None:
            out = out + self.bias
        return self._finish(out)

    @staticmethod
    def _norm_of(g, edge_norm):
        norm = edge_norm if edge_norm is not None else g.edata.get("norm")      # (the message function reads the graph's)
        if norm is not None and norm.numel() != g.number_of_edges():
            raise ValueError("CompGraphConv: edge_norm must have one entry per edge")
        return norm

    # ---- the table form
    def _table_pass(self, g, node_feat, T, etypes, norm):
        N, R, H = g.number_of_nodes(), T.size(0), self.hidden_dim
        P = padded_width(H)
        etypes = etypes.reshape(-1)
        if etypes.numel() != g.number_of_edges():
            raise ValueError("CompGraphConv: etypes must have one entry per edge")
        if self.comp_opt != "corr" or self.loop_weight is None or "is_rev" in g.edata:
            keep = ((etypes >= 0) & (etypes < R)).to(node_feat.dtype)
            return self._edge_pass(g, node_feat, T[etypes.clamp(0, R - 1)], norm, keep)
        Y = ops.matmul_xw(node_feat, corr_weights(T, self.loop_rel, self.in_weight, self.loop_weight, P))
        act = ACT_TANH if isinstance(self.act, nn.Tanh) else ACT_NONE
        if (node_feat.is_cuda and node_feat.dtype == torch.float32 and Y.dtype == torch.float32 and self.bn is None
                and (self.act is None or act == ACT_TANH) and (self.drop.p == 0 or not self.training)
                and (norm is None or not norm.requires_grad) and kernels_admit(T.size(1), H, R, P)):
            nrm = None if norm is None else norm.reshape(-1).to(torch.float32).contiguous()
            return _RelAgg.apply(Y.contiguous(), self.bias, g.index(), etypes.to(torch.int64).contiguous(), nrm, R, 1, H, P, act)
        src, dst = g.all_edges(form="uv", order="eid")
        keep = ((etypes >= 0) & (etypes < R)).to(Y.dtype)
        w = keep if norm is None else keep * norm.view(-1).to(Y.dtype)
        Yv = Y.view(N, R + 1, P)
        msg = Yv[src, etypes.clamp(0, R - 1)][:, :H] * w.view(-1, 1)
        out = torch.zeros(N, H, dtype=Y.dtype, device=Y.device).index_add_(0, dst, msg) + Yv[:, R, :H]
        if self.bias is not None:
            out = out + self.bias
        return self._finish(out)

    @on_input_device
    def forward(self, graph, node_feat, edge_feat, edge_norm=None, etypes=None):
        """``etypes`` None: the reference's call, ``edge_feat`` [E, I] -> ``(node_out, edge_feat @ rel_weight)``.
        ``etypes`` [E]: ``edge_feat`` is the relation table [R, I] (``forward_table``)."""
        g = as_batched(graph)
        if node_feat.dim() != 2 or node_feat.size(0) != g.number_of_nodes() or node_feat.size(1) != self.input_dim:
            raise ValueError("CompGraphConv: node_feat must be [num_nodes, input_dim]")
        norm = self._norm_of(g, edge_norm)
        if etypes is None:
            if edge_feat.size(0) != g.number_of_edges():
                raise ValueError("CompGraphConv: edge_feat must have one row per edge")
            node_out = self._edge_pass(g, node_feat, edge_feat, norm)
        else:
            node_out = self._table_pass(g, node_feat, edge_feat, etypes, norm)
        return node_out, torch.matmul(edge_feat, self.rel_weight)

    def forward_table(self, graph, node_feat, rel_table, etypes, edge_norm=None):
        return self(graph, node_feat, rel_table, edge_norm, etypes=etypes)

    def extra_repr(self):
        return "in=%s, out=%s, comp_opt=%s, self_loop=%s, bias=%s" % (self.input_dim, self.hidden_dim, self.comp_opt, self.self_loop,
                                                                     self.bias is not None)


class BaseModel(nn.Module):
    """model.py:67-114."""

    def __init__(self, node_attri, rel_attri, num_nodes, h_dim, out_dim, num_rels, num_hidden_layers=1, dropout=0, use_cuda=False):
        super(BaseModel, self).__init__()
        self.num_nodes, self.h_dim, self.out_dim = num_nodes, h_dim, out_dim
        self.num_rels, self.num_hidden_layers, self.dropout, self.use_cuda = num_rels, num_hidden_layers, dropout, use_cuda
        self.build_model(node_attri, rel_attri)

    def build_model(self, node_attri, rel_attri):
        self.node_emb, self.rel_emb = self.build_input_layer(node_attri, rel_attri)
        self.layers = nn.ModuleList()
        for idx in range(self.num_hidden_layers):
            self.layers.append(self.build_hidden_layer(idx))
        h2o = self.build_output_layer()
        if h2o is not None:
            self.layers.append(h2o)

    def build_input_layer(self, node_attri, rel_attri):
        return None, None

    def build_hidden_layer(self, idx):
        raise NotImplementedError

    def build_output_layer(self):
        return None

    def forward(self, g, h, r, norm):
        raise NotImplementedError


class CompGCN(BaseModel):
    """model.py:267-305.  ``forward(g, h, r, norm) -> (h [N, out], r [E, out])`` with ``r`` the last layer's relation table
    gathered by the edge types."""

    def build_input_layer(self, node_attri, rel_attri):
        node_emb = EmbeddingLayerAttri(node_attri) if node_attri is not None else EmbeddingLayer(self.num_nodes, self.h_dim)
        rel_emb = EmbeddingLayerAttri(rel_attri) if rel_attri is not None else EmbeddingLayer(self.num_rels, self.h_dim)
        return node_emb, rel_emb

    def build_hidden_layer(self, idx):
        in_dim = self.h_dim if idx == 0 else self.out_dim
        act = nn.Tanh() if idx < self.num_hidden_layers - 1 else None
        return CompGraphConv(in_dim, self.out_dim, comp_opt="corr", self_loop=True, activation=act, dropout=self.dropout)

    def _rows_of(self, r, R):
        """The edge types as row numbers of the table extended by a zero row R (types outside [0, R) read that row); kept
        per edge-type tensor, so that the keyed index of the gather's backward is memoised with it.  The same identity-and-
        version memo as ``unc.TrainModel``'s ``_etype_cache`` and ``unc.DMPNN._rel_pool`` (the rules are ``ops.mark_immutable``'s)."""
        key = (r.data_ptr(), r._version, int(r.numel()), r.device, R)
        usable = ops._memo_usable(r)                           # being recorded and not marked immutable: rebuilt in the recording
        cached = getattr(self, "_rows_cache", None) if usable else None
        if cached is not None and cached[0] == key:
            return cached[1]
        rows = torch.where((r >= 0) & (r < R), r, torch.full_like(r, R))
        if usable and not (r.is_cuda and torch.cuda.is_current_stream_capturing()):   # (made in a recording: its pool's, unfilled)
            self._rows_cache = (key, rows, r)                  # r kept alive: its address stays unique
            if ops.is_immutable(r):
                ops.mark_immutable(rows)
        return rows

    @on_input_device
    def forward(self, g, h, r, norm):
        h = self.node_emb(g, h)
        T = self.rel_emb.weight
        r = r.reshape(-1)
        for layer in self.layers:
            h, T = layer.forward_table(g, h, T, r, norm)
        table = torch.cat([T, T.new_zeros(1, T.size(1))], 0)
        rows = self._rows_of(r, T.size(0))
        if table.is_cuda and table.dtype == torch.float32:
            return h, ops.take_rows_small_table(table, rows)   # (backward: a fixed-order keyed segment sum)
        return h, table[rows]


class TrainModel(unc.TrainModel):
    """model.py:308-412: the CompGCN encoder over ``2 num_rels`` edge types with the link-prediction (DistMult) or
    node-classification head; ``forward(g, h, edge_type, edge_norm) -> ((h, r), pred)``.  The heads, the score, the
    regulariser (its means over the E gathered rows of ``r``; with N == E the node rows take the edge term too) and the two
    losses are the ones of ``unc.TrainModel`` -- the reference repeats them verbatim in every model directory -- so only the
    constructor is stated here, in the reference's order of registration and initialisation."""

    def __init__(self, node_attri, num_nodes, o_dim, num_rels, nlabel, num_hidden_layers=1, dropout=0, use_cuda=False, reg_param=0):
        nn.Module.__init__(self)
        i_dim = o_dim if node_attri is None else node_attri.shape[1]
        self.model = CompGCN(node_attri, None, num_nodes, i_dim, o_dim, num_rels * 2, num_hidden_layers, dropout, use_cuda)
        self.encoder = "CompGCN"
        self.reg_param = reg_param
        if nlabel == 0:
            self.supervised = False
            self.w_relation = nn.Parameter(torch.Tensor(num_rels, o_dim))
            nn.init.xavier_uniform_(self.w_relation, gain=nn.init.calculate_gain("relu"))
        else:
            self.supervised = True
            self.node_fc = nn.Linear(o_dim, nlabel)
            nn.init.xavier_uniform_(self.node_fc.weight, gain=nn.init.calculate_gain("sigmoid"))
            nn.init.zeros_(self.node_fc.bias)
        self.edge_fc = nn.Linear(o_dim, o_dim)
        nn.init.xavier_uniform_(self.edge_fc.weight, gain=nn.init.calculate_gain("sigmoid"))
        nn.init.zeros_(self.edge_fc.bias)
