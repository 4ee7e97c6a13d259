"""The RNN rep-net layer (``SubgraphCountingMatching/models/rnn.py:13-52``) on the HIP kernels of ``csrc/dmp_rnn.hip``.

``RNNLayerHIP`` is one autograd node per layer on rows ``[B, L, H]``, for ``nn.LSTM``, ``nn.GRU`` and ``nn.RNN`` (tanh),
uni- or bidirectional.  It reads the parameters of the layer's own torch module, so nothing is copied that could go stale:

* forward  -- ``P = X W_ihᵀ + b`` for every position and both directions as one GEMM (``b = b_ih + b_hh``; GRU keeps
  ``b_hn`` out of ``P``: it sits inside ``r * (W_hn h + b_hn)``), then ``dmp_rnn_fwd``: one launch runs all L steps of
  every direction and writes ``Y = h * gate (+ X)`` into its half of ``[B, L, D Hd]``.  It saves h and what the backward
  needs of the cell (LSTM i, f, g, o, c; GRU r, z, n, ``W_hn h + b_hn``);
* backward -- ``dmp_rnn_bwd``: the reverse-time recurrence in one launch, writing the pre-activation gate gradients
  ``dG``; then ``dX = dG W_ih``, ``dW_ih = dGᵀ X``, ``dW_hh = Σ_t dG_tᵀ h_{t-1}`` as GEMMs and ``db`` as column sums.
  No float atomics: two runs are bitwise equal.

The recurrence runs over all L positions, the pre-padding included, as the reference's module does.

``hip_layer_ok`` decides: Hd (hidden size per direction) 32, 64 or 128, any input width (it only shapes ``W_ih`` and the
GEMMs around the recurrence; the residual is added when it equals the output width ``D Hd``, as ``forward_rows`` does),
fp32 on the GPU, dropout 0 or eval mode.  Anything else runs the layer's torch module (also the CPU path)."""
import torch as th

CELLS = {"LSTM": (0, 4), "GRU": (1, 3), "RNN": (2, 1)}     # name -> (kernel code, gates per direction)
SAVED = {"LSTM": 5, "GRU": 4, "RNN": 0}                     # cell values saved per hidden unit (i f g o c / r z n hn)
GRADS = {"LSTM": 4, "GRU": 4, "RNN": 1}                     # dG values per hidden unit (GRU: dr dz dn and d(W_hn h + b_hn))


def _params(layer):
    m = layer.layer
    sfx = [""] + (["_reverse"] if m.bidirectional else [])
    out = []
    for s in sfx:
        out += [getattr(m, "weight_ih_l0" + s), getattr(m, "weight_hh_l0" + s), getattr(m, "bias_ih_l0" + s),
                getattr(m, "bias_hh_l0" + s)]
    return out


def hip_layer_ok(layer, x, gate):
    m = layer.layer
    if layer.rnn_type not in CELLS or layer.ln is not None:
        return False
    if getattr(m, "nonlinearity", "tanh") != "tanh" or m.num_layers != 1 or not m.bias or getattr(m, "proj_size", 0):
        return False
    Hd = m.hidden_size
    if not (x.is_cuda and x.dtype == th.float32 and x.dim() == 3 and Hd in (32, 64, 128) and x.size(2) == m.input_size):
        return False
    if x.size(0) < 1 or x.size(1) < 1 or x.size(0) >= (1 << 30):
        return False
    if layer.drop.p > 0 and layer.training:
        return False
    if any(not (p.is_cuda and p.dtype == th.float32 and p.device == x.device) for p in _params(layer)):
        return False
    return gate is None or (gate.is_cuda and gate.shape == x.shape[:2])


class RNNLayerHIP(th.autograd.Function):
    """Y = rnn(x) * gate (+ x): the kernels of csrc/dmp_rnn.hip.  ``params``: (W_ih, W_hh, b_ih, b_hh) per direction."""

    @staticmethod
    def forward(ctx, x, gate, cell, residual, *params):
        from . import _lib
        lib = _lib.load()
        x = x.contiguous()
        _lib.require_gpu(x, gate, *params)
        code, G = CELLS[cell]
        D = len(params) // 4
        B, L, Hin = x.shape
        Hd = params[1].size(1)
        dev = x.device
        w_ih = th.cat([params[4 * d].detach() for d in range(D)], 0)                 # [D G Hd, Hin]
        w_hh = th.stack([params[4 * d + 1].detach() for d in range(D)], 0).contiguous()   # [D, G Hd, Hd]
        b_ih = [params[4 * d + 2].detach() for d in range(D)]
        b_hh = [params[4 * d + 3].detach() for d in range(D)]
        if cell == "GRU":
            bias = th.cat([th.cat([bi[:2 * Hd] + bh[:2 * Hd], bi[2 * Hd:]]) for bi, bh in zip(b_ih, b_hh)])
            b_hn = th.stack([bh[2 * Hd:] for bh in b_hh], 0).contiguous()
        else:
            bias = th.cat([bi + bh for bi, bh in zip(b_ih, b_hh)])
            b_hn = None
        P = th.addmm(bias, x.view(B * L, Hin), w_ih.t())                              # [B L, D G Hd]
        g_in = gate.contiguous().float() if gate is not None else None
        res = residual and Hin == D * Hd
        y = th.empty((B, L, D * Hd), dtype=th.float32, device=dev)
        h = th.empty((B, L, D * Hd), dtype=th.float32, device=dev)
        ns = SAVED[cell]
        sv = th.empty((B, L, D, ns * Hd), dtype=th.float32, device=dev) if ns else None
        _lib.check(lib.dmp_rnn_fwd(P.data_ptr(), w_hh.data_ptr(), _lib.ptr(b_hn), _lib.ptr(g_in), _lib.ptr(x if res else None),
                                   B, L, D, Hd, code, y.data_ptr(), h.data_ptr(), _lib.ptr(sv), _lib.stream_ptr()), "dmp_rnn_fwd")
        ctx.save_for_backward(x, g_in, h, sv, *params)
        ctx.cell, ctx.res, ctx.dims = cell, res, (B, L, Hin, D, Hd)
        return y

    @staticmethod
    def backward(ctx, dy):
        from . import _lib
        lib = _lib.load()
        x, g, h, sv, *params = ctx.saved_tensors
        cell = ctx.cell
        code, G = CELLS[cell]
        B, L, Hin, D, Hd = ctx.dims
        dev = x.device
        dy = dy.contiguous()
        w_hh = th.stack([params[4 * d + 1].detach() for d in range(D)], 0).contiguous()
        ng = GRADS[cell]
        dG = th.empty((B, L, D, ng * Hd), dtype=th.float32, device=dev)
        _lib.check(lib.dmp_rnn_bwd(dy.data_ptr(), _lib.ptr(g), w_hh.data_ptr(), h.data_ptr(), _lib.ptr(sv), B, L, D, Hd, code,
                                   dG.data_ptr(), _lib.stream_ptr()), "dmp_rnn_bwd")
        N = B * L
        X = x.view(N, Hin)
        H = h.view(B, L, D, Hd)
        # the input-side gradient per direction: GRU's n block is d(pre-activation of n); the recurrent side takes
        # d(W_hn h + b_hn) in its place
        dgx = dG[..., :G * Hd] if cell != "GRU" else dG[..., :3 * Hd]
        dgh = dgx if cell != "GRU" else th.cat([dG[..., :2 * Hd], dG[..., 3 * Hd:]], -1)
        dgx = dgx.reshape(N, D * G * Hd)
        dx = None
        if ctx.needs_input_grad[0]:
            w_ih = th.cat([params[4 * d].detach() for d in range(D)], 0)
            dx = th.mm(dgx, w_ih).view(B, L, Hin)
            if ctx.res:
                dx = dx + dy
        grads = []
        for d in range(D):
            gx = dgx[:, d * G * Hd:(d + 1) * G * Hd]
            gh = dgh[:, :, d].reshape(N, G * Hd)
            hp = th.zeros_like(H[:, :, d])                               # h_{t-1} of direction d (zero at its start)
            if d == 0:
                hp[:, 1:] = H[:, :-1, 0]
            else:
                hp[:, :-1] = H[:, 1:, 1]
            grads += [th.mm(gx.t(), X), th.mm(gh.t(), hp.reshape(N, Hd)), gx.sum(0), gh.sum(0)]
        return (dx, None, None, None) + tuple(grads)


def rnn_layer_hip(layer, x, gate, residual):
    """``RNNLayer.forward_rows`` on the kernels: out [B, L, D Hd]."""
    return RNNLayerHIP.apply(x, gate, layer.rnn_type, bool(residual), *_params(layer))
