"""The edge-sequence models: ``EdgeSeqModel`` (``SubgraphCountingMatching/models/basemodel.py:222-617``) and its
rep-nets ``CNN`` (``models/cnn.py``), ``RNN`` (``models/rnn.py``) and ``TXL`` (``models/txl.py``).

Same constructor keywords, sub-module names (hence ``state_dict`` keys), initialisers and seeded RNG order as the
reference, and ``forward(pattern, graph) -> OutputDict`` with its 15 keys (the ``*_v_*`` entries None).  The inputs are
``edgeseq.EdgeSeq`` batches.  Activations stay channels-last ``[B, L, H]``: a CNN layer runs either the fused HIP kernels
of ``cnn.py`` (``cnn.hip_layer_ok``) or the reference's tensor ops on a transposed view, an RNN layer either the recurrence
kernels of ``rnn.py`` (``rnn.hip_layer_ok``) or its own ``nn.LSTM`` / ``nn.GRU`` / ``nn.RNN``; both compute the same
function.  A TXL layer's attention is ``txl.rel_attention``: the kernels of ``csrc/dmp_txl.hip`` or the same in tensor ops."""
from collections import OrderedDict

import torch as th
import torch.nn as nn
import torch.nn.functional as F

from . import cnn as _cnn
from . import rnn as _rnn
from . import txl as _txl
from ._lib import on_input_device
from .act import init_module, init_weight, map_activation_str_to_layer
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


class TXL(EdgeSeqModel):
    """txl.py:212-383 (``TransformerXL``), as the reference computes it:

    * keywords ``seg_len`` (64), ``mem_len`` (64), ``clamp_len`` (-1), ``num_heads`` (1), ``pre_lnorm`` (False) are read bare;
      ``ext_len`` is read from ``seg_len`` too (default 0).  Hence two memory regimes.  ``seg_len`` not passed: ``ext_len = 0`` and
      layer i of a segment also attends the previous segment's input to layer i (detached; ``klen = mem_len + seg_len`` from
      the second segment on).  ``seg_len`` passed: ``ext_len = seg_len``, the memory stays empty and every segment is attended
      on its own; the segments are then independent and ``fold_segments`` runs them as one batch ``[B S, seg_len, H]``;
    * the sequence is padded to a multiple of ``seg_len`` AFTER its rows, the mask BEFORE them, and the result is the last L
      rows: with padding, data, mask and output are offset by the pad;
    * nothing is masked inside the attention (padding rows and zeroed memory rows are attended); the mask zeroes every
      layer's output rows;
    * ``init_mems`` makes ``len(rep_net) + 1 = 4`` memories, so more than 4 layers fail; they are refused at construction."""

    MAX_LAYERS = 4          # len(RepNetDict) + 1 memories, layer i reads memory i

    def __init__(self, **kw):
        self.seg_len = kw.get("seg_len", 64)
        self.ext_len = kw.get("seg_len", 0)
        self.mem_len = kw.get("mem_len", 64)
        self.clamp_len = kw.get("clamp_len", -1)
        self.max_len = self.seg_len + self.ext_len + self.mem_len
        self.num_heads = kw.get("num_heads", 1)
        self.fold_segments = True
        super(TXL, self).__init__(**kw)
        self.pos_emb = PositionEmbedding(self.hid_dim, max_len=max(self.clamp_len, self.max_len))
        self.pos_emb.weight.requires_grad = False
        self.drop = nn.Dropout(kw.get("rep_dropout", 0.0))

    def create_rep_net(self, type, **kw):
        if type == "graph":
            num_layers = kw.get("rep_num_graph_layers", 1)
        elif type == "pattern":
            if self.share_rep_net:
                return self.g_rep_net
            num_layers = kw.get("rep_num_pattern_layers", 1)
        else:
            raise ValueError(type)
        if self.mem_len > 0 and num_layers > self.MAX_LAYERS:
            raise ValueError("rep_net=TXL with %d %s layers: the reference keeps %d memories (one per entry of its rep-net "
                             "container plus one) and layer i reads memory i, so more than %d layers fail"
                             % (num_layers, type, self.MAX_LAYERS, self.MAX_LAYERS))
        num_heads = self.num_heads
        dropout = kw.get("rep_dropout", 0.0)
        act_func = kw.get("rep_act_func", "relu")
        pre_lnorm = kw.get("pre_lnorm", False)
        txl = nn.ModuleList()
        for i in range(num_layers):
            txl.add_module("%s_txl_(%d)" % (type, i),
                           _txl.TXLLayer(self.hid_dim, self.hid_dim, num_heads=num_heads, dropout=dropout, act_func=act_func,
                                         pre_lnorm=pre_lnorm))
        r_w_bias = nn.Parameter(th.Tensor(num_heads, self.hid_dim // num_heads))
        r_r_bias = nn.Parameter(th.Tensor(num_heads, self.hid_dim // num_heads))
        init_weight(r_w_bias, init="normal")
        init_weight(r_r_bias, init="normal")
        return _txl.RepNetDict({"txl": txl, "r_w_bias": r_w_bias, "r_r_bias": r_r_bias})

    def memory_stays_empty(self):
        """update_mems keeps ``cat(mem, hid)[:, beg:end]`` with ``end = mlen + max(0, qlen - ext_len)`` and qlen = seg_len."""
        return self.mem_len <= 0 or self.ext_len >= self.seg_len

    def _update_mems(self, hids, mems, mlen, qlen):
        end = mlen + max(0, qlen - self.ext_len)
        beg = max(0, end - self.mem_len)
        new = []
        for i, hid in enumerate(hids):
            rows = hid if mlen == 0 else th.cat([mems[i], hid], dim=1)
            new.append(rows[:, beg:end].detach())
        return new

    def _segment(self, x, x_mask, net, mems):
        """One segment through every layer (txl.py:290-317): x [B, qlen, H], x_mask [B, qlen, 1] bool, mems a list of
        [B, mlen, H] or None -> (output, the next segment's memories)."""
        qlen = x.size(1)
        mlen = mems[0].size(1) if mems is not None else 0
        pos_seq = th.arange(mlen + qlen - 1, -1, -1, dtype=th.long, device=x.device)
        if self.clamp_len > 0:
            pos_seq = pos_seq.clamp(max=self.clamp_len)
        outputs = [self.drop(x)]
        r = self.drop(self.pos_emb(pos_seq).unsqueeze(0))
        dead = ~x_mask
        for i, layer in enumerate(net["txl"]):
            m = None if mems is None else mems[i]
            outputs.append(layer(outputs[-1], r, net["r_w_bias"], net["r_r_bias"], mems=m).masked_fill(dead, 0.0))
        return outputs[-1], (None if mems is None else self._update_mems(outputs, mems, mlen, qlen))

    def _rep(self, net, x, mask):
        """x [B, L, H] (masked rows already zero), mask [B, L, 1] bool -> [B, L, H] (txl.py:350-358 with utils/dl.py:17-27)."""
        B, L, H = x.shape
        seg = self.seg_len
        pad = (-L) % seg
        if pad:                                  # the data is padded after its rows, the mask before them
            x = th.cat([x, x.new_zeros((B, pad, H))], dim=1)
            mask = th.cat([mask.new_zeros((B, pad, 1)), mask], dim=1)
        S = (L + pad) // seg
        if S > 1 and self.fold_segments and self.memory_stays_empty():
            out, _ = self._segment(x.reshape(B * S, seg, H), mask.reshape(B * S, seg, 1), net, None)
            return out.view(B, S * seg, H)[:, S * seg - L:]
        mems = [x.new_empty((B, 0, H)) for _ in range(len(net) + 1)] if self.mem_len > 0 else None
        outs = []
        for s in range(S):
            o, mems = self._segment(x[:, s * seg:(s + 1) * seg], mask[:, s * seg:(s + 1) * seg], net, mems)
            outs.append(o)
        return th.cat(outs, dim=1)[:, S * seg - L:]

    def get_pattern_rep(self, p_emb, mask=None):
        if mask is None:
            mask = th.ones(p_emb.size()[:2] + (1,), dtype=th.bool, device=p_emb.device)
        else:
            p_emb = p_emb.masked_fill(~mask, 0.0)
        return self._rep(self.p_rep_net, p_emb, mask)

    def get_graph_rep(self, g_emb, mask=None, gate=None):
        if mask is None:
            mask = th.ones(g_emb.size()[:2] + (1,), dtype=th.bool, device=g_emb.device)
        else:
            g_emb = g_emb.masked_fill(~mask, 0.0)
        if gate is not None:
            g_emb = g_emb * gate
        out = self._rep(self.g_rep_net, g_emb, mask)
        return out if gate is None else out * gate


SEQ_MODELS = {"CNN": CNN, "RNN": RNN, "TXL": TXL}
