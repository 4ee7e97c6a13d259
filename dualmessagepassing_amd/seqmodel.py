"""The edge-sequence models: ``EdgeSeqModel`` (``SubgraphCountingMatching/models/basemodel.py:222-617``) and its
rep-nets ``CNN`` (``models/cnn.py``) and ``RNN`` (``models/rnn.py``).

Same constructor keywords, sub-module names (hence ``state_dict`` keys), initialisers and seeded RNG order as the
reference, and ``forward(pattern, graph) -> OutputDict`` with its 15 keys (the ``*_v_*`` entries None).  The inputs are
``edgeseq.EdgeSeq`` batches.  Activations stay channels-last ``[B, L, H]``: a CNN layer runs either the fused HIP kernels
of ``cnn.py`` (``cnn.hip_layer_ok``) or the reference's tensor ops on a transposed view, an RNN layer either the recurrence
kernels of ``rnn.py`` (``rnn.hip_layer_ok``) or its own ``nn.LSTM`` / ``nn.GRU`` / ``nn.RNN``; both compute the same
function."""
from collections import OrderedDict

import torch as th
import torch.nn as nn
import torch.nn.functional as F

from . import cnn as _cnn
from . import rnn as _rnn
from ._lib import on_input_device
from .act import init_module, map_activation_str_to_layer
from .basemodel import BaseModel, OutputDict, ScalarFilter
from .constants import REVFLAG
from .embed import (EquivariantEmbedding, MultihotEmbedding, NormalEmbedding, OrthogonalEmbedding, PositionEmbedding,
                    UniformEmbedding, get_enc_len)
from .pred import PRED_NETS, pred_net_kwargs

SEQ_KEYS = ("u", "v", "ul", "el", "vl")


def len_to_mask_pre_pad(lens, L):
    """utils/dl.py:113-127 with ``pre_pad``: the last ``len`` positions of each row; a row of length 0 is all ones
    (the reference's ``mask[i, :-0]`` selects nothing to clear)."""
    col = th.arange(L, device=lens.device).view(1, L)
    return (col >= (L - lens).view(-1, 1)) | (lens == 0).view(-1, 1)


class EdgeSeqModel(BaseModel):
    """basemodel.py:222-617."""

    def _enc_set(self, enc_net, nv, nvl, nel):
        def enc(n):
            if enc_net == "Multihot":
                return MultihotEmbedding(n, self.base)
            if enc_net == "Position":
                return PositionEmbedding(int(get_enc_len(n - 1, self.base)) * self.base, n)
            raise NotImplementedError(enc_net)
        return OrderedDict([("u", enc(nv)), ("v", enc(nv)), ("ul", enc(nvl)), ("el", enc(nel)), ("vl", enc(nvl))])

    def create_enc_net(self, type, **kw):
        enc_net = kw.get("enc_net", "Multihot")
        if type == "graph":
            nets = self._enc_set(enc_net, self.max_ngv, self.max_ngvl, self.max_ngel)
        elif type == "pattern":
            if self.share_enc_net:
                return self.g_enc_net
            nets = self._enc_set(enc_net, self.max_npv, self.max_npvl, self.max_npel)
        else:
            raise ValueError(type)
        for net in nets.values():
            net.weight.requires_grad = False
        return nn.ModuleDict(nets)

    def create_filter_net(self, **kw):
        filter_net = kw.get("filter_net", "None")
        if filter_net == "None":
            return None
        if filter_net == "ScalarFilter":
            return nn.ModuleDict({k: ScalarFilter() for k in ("ul", "el", "vl")})
        raise ValueError(filter_net)

    def create_emb_net(self, type, **kw):
        emb_net = kw.get("emb_net", "Orthogonal")
        dims = self.get_graph_enc_dims() if type == "graph" else self.get_pattern_enc_dims()
        cls = {"Orthogonal": OrthogonalEmbedding, "Normal": NormalEmbedding, "Uniform": UniformEmbedding,
               "Equivariant": EquivariantEmbedding}.get(emb_net)
        if cls is None:
            raise ValueError(emb_net)
        return nn.ModuleDict(OrderedDict((k, cls(v, self.hid_dim)) for k, v in dims.items()))

    def create_pred_net(self, **kw):
        name = kw.get("pred_net", "SumPredictNet")
        if name not in PRED_NETS:
            raise ValueError(name)
        return PRED_NETS[name](self.get_rep_dim(), hidden_dim=kw.get("pred_hid_dim", 64),
                               act_func=kw.get("pred_act_func", "relu"), dropout=kw.get("pred_dropout", 0.0),
                               return_weights="edge" in kw.get("pred_return_weights", "none"), **pred_net_kwargs(name, kw))

    def _enc_dims(self, nv, nvl, nel):
        d = lambda n: int(get_enc_len(n - 1, self.base)) * self.base
        return OrderedDict([("u", d(nv)), ("v", d(nv)), ("ul", d(nvl)), ("el", d(nel)), ("vl", d(nvl))])

    def get_graph_enc_dims(self):
        return self._enc_dims(self.max_ngv, self.max_ngvl, self.max_ngel)

    def get_pattern_enc_dims(self):
        return self.get_graph_enc_dims() if self.share_enc_net else self._enc_dims(self.max_npv, self.max_npvl, self.max_npel)

    def get_rep_dim(self):  # basemodel.py:117-123
        rep_dim = self.hid_dim
        if self.pred_with_enc:
            rep_dim += sum(self.get_graph_enc_dims().values())
        if self.pred_with_deg:
            rep_dim += 2
        return rep_dim

    def get_filter_gate(self, pattern, graph):
        if self.filter_net is None or len(self.filter_net) == 0:
            return None
        ul = self.filter_net["ul"](pattern.ul, graph.ul)
        el = self.filter_net["el"](pattern.el, graph.el)
        vl = self.filter_net["vl"](pattern.vl, graph.vl)
        return (ul & vl) & el

    @staticmethod
    def _enc(net, seq):
        return OrderedDict((k, net[k](seq.tdata[k])) for k in SEQ_KEYS)

    def get_pattern_enc(self, pattern):
        return self._enc(self.p_enc_net, pattern)

    def get_graph_enc(self, graph):
        return self._enc(self.g_enc_net, graph)

    @staticmethod
    def _emb(net, enc):
        emb = None
        for k in SEQ_KEYS:
            x = net[k](enc[k])
            emb = x if emb is None else emb + x
        return emb

    def get_pattern_emb(self, p_enc):
        return self._emb(self.p_emb_net, p_enc)

    def get_graph_emb(self, g_enc):
        return self._emb(self.g_emb_net, g_enc)

    def get_pattern_rep(self, p_emb, mask=None):
        raise NotImplementedError

    def get_graph_rep(self, g_emb, mask=None, gate=None):
        raise NotImplementedError

    def get_subiso_pred(self, p_e_rep, p_e_mask, g_e_rep, g_e_mask):
        pred_c, pred_w = self.pred_net(p_e_rep, p_e_mask, g_e_rep, g_e_mask)
        return pred_c, (None, pred_w)

    @staticmethod
    def _deg_feats(seq):
        num_v = seq.batch_num_nodes().view(-1, 1)
        shift = num_v.max() - num_v                                  # pre-padding
        out_deg, in_deg = seq.out_degrees().float(), seq.in_degrees().float()
        return [th.gather(out_deg, 1, seq.u + shift).unsqueeze(-1), th.gather(in_deg, 1, seq.v + shift).unsqueeze(-1)]

    @on_input_device
    def forward(self, pattern, graph):  # basemodel.py:533-617
        bsz = pattern.batch_size
        p_e_mask = len_to_mask_pre_pad(pattern.batch_num_tuples(), pattern.u.size(1)).view(bsz, -1, 1)
        g_e_mask = len_to_mask_pre_pad(graph.batch_num_tuples(), graph.u.size(1)).view(bsz, -1, 1)
        el_gate = self.get_filter_gate(pattern, graph).view(bsz, -1, 1).float()

        p_enc = self.get_pattern_enc(pattern)
        p_e_emb = self.get_pattern_emb(p_enc)
        p_e_rep = self.get_pattern_rep(p_e_emb, mask=p_e_mask)

        g_enc = self.get_graph_enc(graph)
        g_e_emb = self.get_graph_emb(g_enc)
        g_e_rep = self.get_graph_rep(g_e_emb, mask=g_e_mask, gate=el_gate)

        if REVFLAG in pattern.tdata:
            p_e_mask = p_e_mask.masked_fill(pattern.tdata[REVFLAG].view(bsz, -1, 1), 0)
        if REVFLAG in graph.tdata:
            g_e_mask = g_e_mask.masked_fill(graph.tdata[REVFLAG].view(bsz, -1, 1), 0)

        p_add, g_add = [], []
        if self.pred_with_enc:
            p_add += [p_enc[k] for k in SEQ_KEYS]
            g_add += [g_enc[k] for k in SEQ_KEYS]
        if self.pred_with_deg:
            p_add += self._deg_feats(pattern)
            g_add += self._deg_feats(graph)
        if p_add:
            p_add = self.refine_edge_weights(th.cat(p_add, dim=-1).masked_fill(~p_e_mask, 0))
            g_add = self.refine_edge_weights(th.cat(g_add, dim=-1).masked_fill(~g_e_mask, 0))
            p_e_output = th.cat([p_add, p_e_rep], dim=-1)
            g_e_output = th.cat([g_add, g_e_rep], dim=-1)
        else:
            p_e_output, g_e_output = p_e_rep, g_e_rep
        del p_add, g_add

        p_e_mask = self.refine_edge_weights(p_e_mask.float(), use_max=True).bool().view(bsz, -1)
        g_e_mask = self.refine_edge_weights(g_e_mask.float(), use_max=True).bool().view(bsz, -1)

        pred_c, (pred_v, pred_e) = self.get_subiso_pred(p_e_output, p_e_mask, g_e_output, g_e_mask)
        return OutputDict(p_v_emb=None, p_e_emb=p_e_emb, g_v_emb=None, g_e_emb=g_e_emb, p_v_rep=None, p_e_rep=p_e_rep,
                          g_v_rep=None, g_e_rep=g_e_rep, p_v_mask=None, p_e_mask=p_e_mask, g_v_mask=None, g_e_mask=g_e_mask,
                          pred_c=pred_c, pred_v=pred_v, pred_e=pred_e)


class CNNLayer(nn.Module):
    """cnn.py:13-64: conv -> act -> max-pool -> (BatchNorm) -> dropout on ``[B, H, L]``.  ``forward`` keeps that
    interface; the model calls ``forward_rows`` on channels-last rows with the gate and the residual."""

    def __init__(self, in_channels, out_channels, kernel_size, padding=-1, stride=1, groups=1, dilation=1, batch_norm=True,
                 act_func="relu", dropout=0.0):
        super(CNNLayer, self).__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        if padding == -1:
            padding = kernel_size // 2
        self.act_func = act_func
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size=kernel_size, padding=padding, stride=stride, groups=groups,
                              dilation=dilation)
        self.act = map_activation_str_to_layer(act_func)     # the shared module is not switched to in-place here
        self.pool = nn.MaxPool1d(kernel_size=kernel_size // stride, stride=1, padding=padding)
        self.bn = nn.BatchNorm1d(out_channels) if batch_norm else None
        self.drop = nn.Dropout(dropout)
        init_module(self.conv, init="normal", activation=act_func)

    def forward(self, x):
        o = self.pool(self.act(self.conv(x)))
        if self.bn is not None:
            o = self.bn(o)
        return self.drop(o)

    def get_output_dim(self):
        return self.out_channels

    def gate_next(self, gate):
        """The gate after this layer (cnn.py:122-135): max-pooled with the conv geometry, then with the pool geometry.
        gate [B, 1, L]."""
        c, p = self.conv, self.pool
        gate = F.max_pool1d(gate, kernel_size=c.kernel_size, stride=c.stride, padding=c.padding, dilation=c.dilation)
        return F.max_pool1d(gate, kernel_size=p.kernel_size, stride=p.stride, padding=p.padding, dilation=p.dilation)

    def forward_rows(self, x, gate, residual):
        """x [B, L, H] channels-last, gate [B, L] float or None -> (out [B, L', H], gate after the layer [B, L'] or None):
        ``layer(x) * gate' (+ x when residual and the sizes match)``."""
        if _cnn.hip_layer_ok(self, x, gate):
            return _cnn.cnn_layer_hip(self, x, gate, residual)
        o = self(x.transpose(1, 2))
        if gate is not None:
            gate = self.gate_next(gate.unsqueeze(1)).squeeze(1)
            o = o * gate.unsqueeze(1)
        o = o.transpose(1, 2)
        if residual and o.size() == x.size():
            o = x + o
        return o, gate


class CNN(EdgeSeqModel):
    """cnn.py:67-237."""

    def create_rep_net(self, type, **kw):
        if type == "graph":
            num_layers = kw.get("rep_num_graph_layers", 1)
        elif type == "pattern":
            if self.share_rep_net:
                return self.g_rep_net
            num_layers = kw.get("rep_num_pattern_layers", 1)
        else:
            raise ValueError(type)
        act_func = kw.get("rep_act_func", "relu")
        dropout = kw.get("rep_dropout", 0.0)
        batch_norm = kw.get("rep_cnn_batch_norm", True)
        sizes = kw.get("rep_cnn_kernel_sizes", 2)
        paddings = kw.get("rep_cnn_paddings", -1)
        strides = kw.get("rep_cnn_strides", 1)
        sizes = [sizes] * num_layers if isinstance(sizes, int) else sizes
        paddings = [paddings] * num_layers if isinstance(paddings, int) else paddings
        strides = [strides] * num_layers if isinstance(strides, int) else strides
        cnn = nn.ModuleList()
        for i in range(num_layers):
            cnn.add_module("%s_cnn_(%d)" % (type, i),
                           CNNLayer(self.hid_dim, self.hid_dim, kernel_size=sizes[i], padding=paddings[i], stride=strides[i],
                                    batch_norm=batch_norm, act_func=act_func, dropout=dropout))
        return nn.ModuleDict({"cnn": cnn})

    def _rep(self, net, emb, gate):
        if gate is None:
            x = emb
        else:
            x = emb * gate.unsqueeze(-1)
        for layer in net["cnn"]:
            x, gate = layer.forward_rows(x, gate, self.rep_residual)
        return x

    def get_pattern_rep(self, p_emb, mask=None):
        return self._rep(self.p_rep_net, p_emb, None if mask is None else mask.float().view(mask.size(0), -1))

    def get_graph_rep(self, g_emb, mask=None, gate=None):
        if mask is None and gate is None:
            return self._rep(self.g_rep_net, g_emb, None)
        g = (mask.float() if mask is not None else 1) * (gate if gate is not None else 1)
        return self._rep(self.g_rep_net, g_emb, g.view(g_emb.size(0), -1))

    def refine_edge_weights(self, weights, use_max=False):  # cnn.py:175-237
        if weights is None:
            return None
        dim, dtype = weights.dim(), weights.dtype
        if dim == 2:
            weights = weights.unsqueeze(-1)
        weights = weights.transpose(1, 2).float()
        for layer in self.g_rep_net["cnn"]:
            if not isinstance(layer, CNNLayer):
                continue
            c, p = layer.conv, layer.pool
            if use_max:
                weights = F.max_pool1d(weights, kernel_size=c.kernel_size, stride=c.stride, padding=c.padding, dilation=c.dilation)
            else:
                weights = sum(c.kernel_size) * F.avg_pool1d(weights, kernel_size=c.kernel_size, stride=c.stride, padding=c.padding)
            weights = F.max_pool1d(weights, kernel_size=p.kernel_size, stride=p.stride, padding=p.padding, dilation=p.dilation)
        weights = weights.transpose(1, 2)
        if dim == 2:
            weights = weights.squeeze(-1)
        return weights.to(dtype)


class RNNLayer(nn.Module):
    """rnn.py:13-52: a one-layer ``nn.LSTM`` / ``nn.GRU`` / ``nn.RNN`` (tanh), batch first, hidden ``hid_dim // 2`` per
    direction when bidirectional, then dropout.  The reference's ``layer_norm`` argument is kept, but its ``RNN`` never
    passes it.  The model calls ``forward_rows`` with the gate and the residual."""

    def __init__(self, rep_rnn_type, input_dim, hid_dim, layer_norm=False, bidirectional=False, dropout=0.0):
        super(RNNLayer, self).__init__()
        self.input_dim = input_dim
        self.hid_dim = hid_dim
        cls = {"LSTM": nn.LSTM, "GRU": nn.GRU, "RNN": nn.RNN}.get(rep_rnn_type)
        if cls is None:
            raise ValueError("rep_rnn_type=%s is not supported (LSTM, GRU or RNN)" % (rep_rnn_type,))
        self.rnn_type = rep_rnn_type
        self.layer = cls(input_dim, hid_dim // 2 if bidirectional else hid_dim, bidirectional=bidirectional, batch_first=True)
        self.ln = nn.LayerNorm(hid_dim) if layer_norm else None
        self.drop = nn.Dropout(dropout)
        init_module(self.layer)

    def forward(self, x):
        o = self.layer(x)[0]
        if self.ln is not None:
            o = self.ln(o)
        return self.drop(o)

    def get_output_dim(self):
        return self.hid_dim - self.hid_dim % 2

    def forward_rows(self, x, gate, residual):
        """x [B, L, H], gate [B, L] float or None -> ``layer(x) * gate (+ x when residual and the sizes match)``.  The
        recurrence runs over all L positions, the padding included, as the reference's does."""
        if _rnn.hip_layer_ok(self, x, gate):
            return _rnn.rnn_layer_hip(self, x, gate, residual)
        o = self(x)
        if gate is not None:
            o = o * gate.unsqueeze(-1)
        if residual and o.size() == x.size():
            o = x + o
        return o


class RNN(EdgeSeqModel):
    """rnn.py:55-124."""

    def create_rep_net(self, type, **kw):
        if type == "graph":
            num_layers = kw.get("rep_num_graph_layers", 1)
        elif type == "pattern":
            if self.share_rep_net:
                return self.g_rep_net
            num_layers = kw.get("rep_num_pattern_layers", 1)
        else:
            raise ValueError(type)
        rep_rnn_type = kw.get("rep_rnn_type", "LSTM")
        bidirectional = kw.get("rep_rnn_bidirectional", False)
        dropout = kw.get("rep_dropout", 0.0)
        rnn = nn.ModuleList()
        for i in range(num_layers):
            rnn.add_module("%s_rnn_(%d)" % (type, i),
                           RNNLayer(rep_rnn_type, self.hid_dim, self.hid_dim, bidirectional=bidirectional, dropout=dropout))
        return nn.ModuleDict({"rnn": rnn})

    def _rep(self, net, x, gate, residual):
        for layer in net["rnn"]:
            x = layer.forward_rows(x, gate, residual)
        return x

    def get_pattern_rep(self, p_emb, mask=None):
        # with a mask (forward always passes one): masked input, every layer's output masked, no residual
        if mask is None:
            return self._rep(self.p_rep_net, p_emb, None, self.rep_residual)
        m = mask.float().view(mask.size(0), -1)
        return self._rep(self.p_rep_net, p_emb.masked_fill(~mask, 0.0), m, False)

    def get_graph_rep(self, g_emb, mask=None, gate=None):
        if mask is None and gate is None:
            return self._rep(self.g_rep_net, g_emb, None, self.rep_residual)
        g = (mask.float() if mask is not None else 1) * (gate if gate is not None else 1)
        return self._rep(self.g_rep_net, g_emb * g, g.view(g_emb.size(0), -1), self.rep_residual)


SEQ_MODELS = {"CNN": CNN, "RNN": RNN}
