"""Float64 CPU restatements of the CNN layer, the RNN layer and the relational conv, written from the operators' public
definitions (not by running the code under test in double), and the case lists that ``test_fp64_refs_cpu.py`` and the three
``test_gpu_*_fp64.py`` modules share, so the CPU check of the yardsticks covers exactly what the GPU modules run.

Distances are measured as everywhere in the suite: ``max |a - ref| <= tol * max(1, max |ref|)``."""
import torch as th
import torch.nn.functional as F

NEG_INF = float("-inf")
TAU = 1e-4                  # perturbation of the pre-activations under which a safe output keeps its winner and its sign
UNSAFE_CAP = 1e-3           # at most this share of a case's outputs may be unsafe (a condition on the inputs, asserted)


def dist(a, ref):
    """(max |a - ref|, max(1, max |ref|)) in double on the CPU."""
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    if ref.numel() == 0:
        return 0.0, 1.0
    return float((a - ref).abs().max()), max(1.0, float(ref.abs().max()))


def close(a, ref, tol, what):
    assert tuple(a.shape) == tuple(ref.shape), (what, tuple(a.shape), tuple(ref.shape))
    assert bool(th.isfinite(a).all()), what + ": not finite"
    err, scale = dist(a, ref)
    assert err <= tol * scale, "%s: %g (scale %g, tol %g)" % (what, err, scale, tol)


def within_band(a, ref, yard, tol, what, table=None):
    """``a`` passes if it is within the project's figure ``tol``, or within four times the distance of ``yard`` (the fp32
    tensor-op result of the same operation) from the fp64 ``ref``.  Prints both distances, relative to the scale."""
    assert bool(th.isfinite(a).all()), what + ": not finite"
    err, scale = dist(a, ref)
    yerr, _ = dist(yard, ref)
    print("FP64BAND %s kernel %.3g yardstick %.3g (x scale %.3g)" % (what, err / scale, yerr / scale, scale))
    if table is not None:
        table.append((what, err / scale, yerr / scale))
    assert err <= max(tol * scale, 4.0 * yerr), "%s: %g against fp64, the fp32 tensor ops %g (scale %g, tol %g)" % (
        what, err, yerr, scale, tol)


# ------------------------------------------------------------------------------------------------------------------ CNN

def max_pool_rows(v, kernel, pad):
    """Max-pool along the last axis, stride 1, ``pad`` positions of -inf on both sides: (max, offset of the FIRST maximum in
    the window, counted from the window's start in the padded row), both [..., L + 2 pad - kernel + 1]."""
    win = F.pad(v, (pad, pad), value=NEG_INF).unfold(-1, kernel, 1)
    best = win.max(-1).values
    first = (win == best.unsqueeze(-1)).to(th.int64).argmax(-1)
    return best, first, win


def cnn_gate_fp64(gate, k, pad, pk, pp):
    """The gate after the layer: max-pool of the gate [B, L] with the conv geometry, then with the pool geometry."""
    g = max_pool_rows(gate.double(), k, pad)[0]
    return max_pool_rows(g, pk, pp)[0]


def cnn_layer_fp64(weight, bias, x, gate, k, pad, pk, pp, slope, residual, act=True, apply_gate=True, post=None, tau=TAU):
    """``pool(act(conv(x) + b)) * gate' (+ x when the sizes match)`` on channels-last rows in double.

    weight [H, H, k] (out, in, tap), bias [H] or None, x [B, L, H], gate [B, L] or None; ``slope`` is the activation's
    negative slope (0 for relu), ``act=False`` leaves the conv linear; ``post`` maps the pooled rows [B, L', H] before the
    gate (BatchNorm).  Returns (y [B, L', H], gate' [B, L'] or None, safe [B, L', H] bool, arg [B, L', H] int64: the window
    offset of the first maximum, plus 128 where the maximum is positive).

    An output is safe when neither its winner nor the winner's sign can change if every pre-activation of its window moves
    by up to ``tau``: the winner leads the runner-up by more than 2 tau and is further than tau from zero.  With relu a
    window whose pre-activations are all below -tau is safe as well: whoever wins, the output and its gradient are zero."""
    B, L, H = x.shape
    conv = F.conv1d(x.transpose(1, 2), weight, bias, padding=pad)                     # [B, H, Lc]
    a = th.where(conv > 0, conv, conv * slope) if act else conv
    best, first, win = max_pool_rows(a, pk, pp)
    idx = first.unsqueeze(-1)
    pool = win.gather(-1, idx).squeeze(-1)                                             # the gradient goes to the first maximum
    with th.no_grad():
        cwin = F.pad(conv, (pp, pp), value=NEG_INF).unfold(-1, pk, 1)
        top = cwin.topk(min(2, pk), dim=-1).values
        lead = top[..., 0] - top[..., 1] if pk > 1 else th.full_like(top[..., 0], float("inf"))
        safe = (lead > 2 * tau) & (top[..., 0].abs() > tau) if act else th.ones_like(lead, dtype=th.bool)
        if act and slope == 0:
            safe = safe | (top[..., 0] < -tau)
        arg = first + 128 * (best > 0).to(th.int64)
    y = pool.transpose(1, 2)                                                           # [B, L', H]
    if post is not None:
        y = post(y)
    g = None
    if gate is not None:
        g = cnn_gate_fp64(gate, k, pad, pk, pp)
        if apply_gate:
            y = y * g.unsqueeze(-1)
    if residual and y.size() == x.size():
        y = x + y
    return y, g, safe.transpose(1, 2), arg.transpose(1, 2)


def batch_norm_fp64(p, weight, bias, mean, var, training, momentum, eps, tracked):
    """nn.BatchNorm1d over all rows of p [B, L', H]: (out, running mean, running var after the call).  ``momentum`` None is
    the cumulative average 1 / (batches tracked, this one included)."""
    rows = p.reshape(-1, p.size(-1))
    if not training:
        return (p - mean) / th.sqrt(var + eps) * weight + bias, mean, var
    n = rows.size(0)
    m = rows.mean(0)
    v = ((rows - m) ** 2).mean(0)
    f = 1.0 / (tracked + 1) if momentum is None else momentum
    with th.no_grad():
        new_mean = (1 - f) * mean + f * m
        new_var = (1 - f) * var + f * v * n / max(n - 1, 1)
    return (p - m) / th.sqrt(v + eps) * weight + bias, new_mean, new_var


def cnn_geometries():
    """Every (k, pad) that ``cnn.hip_layer_ok`` admits for a ``CNNLayer`` (pool kernel k, pool padding pad): 24."""
    return [(k, pad) for k in range(1, 9) for pad in range(0, k // 2 + 1)]


def cnn_lengths(k, pad):
    """Input lengths that put L' at TP - 1, TP, TP + 1, 2 TP, 2 TP + 1 (TP = 65 - k pool rows per workgroup), the smallest
    admitted length (one conv row where the pool admits it) and k - 1 where that is admitted."""
    tp = 65 - k
    shift = 4 * pad - 2 * k + 2                                    # L' = L + shift
    lmin = max(1, k - 2 * pad, 1 - shift)
    out = [n - shift for n in (tp - 1, tp, tp + 1, 2 * tp, 2 * tp + 1)] + [lmin]
    if k - 1 >= lmin:
        out.append(k - 1)
    return sorted(set(out))


def cnn_layer_cases():
    """ids -> (H, k, pad, act): all 24 geometries at both widths with both activations."""
    return {"H%d-k%d-p%d-%s" % (H, k, pad, act): (H, k, pad, act)
            for H in (64, 128) for (k, pad) in cnn_geometries() for act in ("relu", "leaky_relu")}


def cnn_layer_runs(k, pad):
    """The runs of one layer case: (B, L, gated, residual).  Every length runs with the gate and without it, the residual
    alternating; where L' = L (the only sizes at which the residual is added) all four combinations run; B = 1 at one
    length."""
    runs = []
    same = 4 * pad - 2 * k + 2 == 0
    for i, L in enumerate(cnn_lengths(k, pad)):
        B = 1 if i == 2 else 3
        for gated in (True, False):
            for residual in ((True, False) if same else ((i + gated) % 2 == 0,)):
                runs.append((B, L, gated, residual))
    return runs


def cnn_make_layer(H, k, pad, act, bn=False, seed=0, momentum=0.1):
    from dualmessagepassing_amd.seqmodel import CNNLayer
    th.manual_seed(seed)
    layer = CNNLayer(H, H, kernel_size=k, padding=pad, batch_norm=bn, act_func=act)
    with th.no_grad():
        layer.conv.bias.uniform_(-0.2, 0.2)
        if bn:
            layer.bn.weight.uniform_(0.5, 1.5)
            layer.bn.bias.uniform_(-0.3, 0.3)
            layer.bn.running_mean.uniform_(-0.2, 0.2)
            layer.bn.running_var.uniform_(0.5, 1.5)
            layer.bn.momentum = momentum
    return layer


def cnn_inputs(B, L, H, gated, seed):
    """N(0, 1) rows (not masked: exact zeros would tie every pool window) and a gate with pre-padding, holes and, from
    B = 3 on, an empty row; the upstream weight is drawn by the caller."""
    g = th.Generator().manual_seed(seed)
    x = th.randn(B, L, H, generator=g)
    if not gated:
        return x, None
    gate = th.ones(B, L)
    if B > 1:
        gate[1, :L - L // 2] = 0.0
    if B > 2:
        gate[2] = 0.0
    for t in (L // 3, L // 3 + 1, L - 1 - L // 5):
        if L > 4:
            gate[0, t] = 0.0
    return x, gate


def cnn_slope(act):
    return {"relu": 0.0, "leaky_relu": 1.0 / 5.5}[act]


def cnn_bn_cases():
    """ids -> (H, k, pad, act, training, momentum, B, L).  The training cases are small enough to have no unsafe output at
    all (asserted): BatchNorm's backward spreads every upstream entry over all pooled rows, so masking cannot isolate one."""
    return {"train-m0.1": (64, 3, 1, "relu", True, 0.1, 3, 19), "train-mNone": (128, 2, 1, "leaky_relu", True, None, 2, 12),
            "train-k5": (64, 5, 1, "leaky_relu", True, 0.3, 2, 23), "eval": (128, 4, 2, "relu", False, 0.1, 3, 70),
            "eval-mNone": (64, 6, 3, "leaky_relu", False, None, 3, 64)}


def cnn_bn_inputs(case, layer):
    """(x, gate) of a BatchNorm case.  A training case takes the first seed at which the reference (alone) finds no unsafe
    output."""
    H, k, pad, act, training, momentum, B, L = cnn_bn_cases()[case]
    W, b = layer.conv.weight.detach().cpu().double(), layer.conv.bias.detach().cpu().double()
    for seed in range(stable_seed(case), stable_seed(case) + 64):
        x, gate = cnn_inputs(B, L, H, True, seed)
        safe = cnn_layer_fp64(W, b, x.double(), gate, k, pad, k, pad, cnn_slope(act), True)[2]
        if not training or bool(safe.all()):
            return x, gate
    raise AssertionError("no seed without an unsafe output for " + case)


# ------------------------------------------------------------------------------------------------------------------ RNN

def rnn_layer_fp64(cell, params, x, gate, residual):
    """One-layer LSTM / GRU / RNN (tanh), batch first, as an explicit time loop over the gate equations (PyTorch's gate
    order i f g o / r z n; GRU's ``b_hn`` inside ``r * (W_hn h + b_hn)``), one or two directions, over all L positions.
    ``params``: [W_ih, W_hh, b_ih, b_hh] per direction, flat; x [B, L, Hin]; gate [B, L] or None.
    Returns ``rnn(x) * gate (+ x when the widths match)`` [B, L, D Hd]."""
    B, L, _ = x.shape
    outs = []
    for d in range(len(params) // 4):
        wi, wh, bi, bh = params[4 * d:4 * d + 4]
        hd = wh.size(1)
        h = x.new_zeros(B, hd)
        c = x.new_zeros(B, hd)
        ys = [None] * L
        for t in (range(L) if d == 0 else range(L - 1, -1, -1)):
            gi = x[:, t] @ wi.t() + bi
            gh = h @ wh.t() + bh
            if cell == "LSTM":
                i, f, g, o = (gi + gh).split(hd, 1)
                c = th.sigmoid(f) * c + th.sigmoid(i) * th.tanh(g)
                h = th.sigmoid(o) * th.tanh(c)
            elif cell == "GRU":
                r = th.sigmoid(gi[:, :hd] + gh[:, :hd])
                z = th.sigmoid(gi[:, hd:2 * hd] + gh[:, hd:2 * hd])
                n = th.tanh(gi[:, 2 * hd:] + r * gh[:, 2 * hd:])
                h = (1 - z) * n + z * h
            else:
                h = th.tanh(gi + gh)
            ys[t] = h
        outs.append(th.stack(ys, 1))
    y = th.cat(outs, -1)
    if gate is not None:
        y = y * gate.unsqueeze(-1)
    if residual and y.size() == x.size():
        y = x + y
    return y


RNN_FP32_SHARE = 0.25       # the reference loop run in float32 stays within this share of a short case's tolerance (asserted)


def rnn_cases():
    """ids -> dict(cell, bi, hd, din (None: the output width), B, L, gate, residual, scale, band).

    gate: "mixed" (pre-padding, holes, an empty row), None, "zero-row", "ends" (holes at the first and the last position).
    ``band`` marks the cases whose error grows with a size nobody measured against fp64 (L 700, saturated gates)."""
    cases = {}

    def add(name, cell, bi, hd, din=None, B=5, L=33, gate="mixed", residual=True, scale=1.0, band=False):
        cases[name] = dict(cell=cell, bi=bi, hd=hd, din=din, B=B, L=L, gate=gate, residual=residual, scale=scale, band=band)

    for cell in ("LSTM", "GRU", "RNN"):
        for bi in (False, True):
            tag = "%s-%s" % (cell, "bi" if bi else "uni")
            for hd in (32, 64, 128):
                add("%s-hd%d" % (tag, hd), cell, bi, hd, B=7, L=61, residual=hd != 64)
            # unequal widths: hid_dim fixed at 64 (Hd 64 or 32 per direction), the input narrower, wider, and odd
            hd = 32 if bi else 64
            for din in (50, 4 * hd, hd // 2):
                add("%s-in%d" % (tag, din), cell, bi, hd, din=din, B=5, L=21)
            add(tag + "-nogate", cell, bi, 64, B=3, L=17, gate=None)
            add(tag + "-ends", cell, bi, 32, B=2, L=9, gate="ends")
            add(tag + "-saturated", cell, bi, 64, B=3, L=40, scale=15.0, band=True)
        for B in (1, 4, 8):
            add("%s-B%d" % (cell, B), cell, False, 32, B=B, L=11)
        add("%s-bi-B9" % cell, cell, True, 32, B=9, L=11)
        add("%s-bi-L1" % cell, cell, True, 64, B=3, L=1)
        add("%s-uni-L2" % cell, cell, False, 128, B=5, L=2, residual=False)
        add("%s-bi-zero-row" % cell, cell, True, 32, B=4, L=13, gate="zero-row")
        add("%s-uni-L700" % cell, cell, False, 128, B=5, L=700, band=True)
        add("%s-bi-L700" % cell, cell, True, 64, B=2, L=700, band=True)
    return cases


def rnn_make_layer(c, seed=0):
    from dualmessagepassing_amd.seqmodel import RNNLayer
    th.manual_seed(seed)
    hid = c["hd"] * (2 if c["bi"] else 1)
    layer = RNNLayer(c["cell"], c["din"] or hid, hid, bidirectional=c["bi"])
    with th.no_grad():
        for k, p in layer.named_parameters():
            if "bias" in k:
                p.uniform_(-0.3, 0.3)
            elif c["cell"] != "RNN":
                p.mul_(1.5)         # not the plain tanh cell: at that gain it amplifies fp32 rounding itself (RNN_FP32_SHARE)
    return layer


def rnn_inputs(c, seed=1):
    """Rows N(0, 1) times ``scale`` (15: sigmoids at 0 / 1, tanh at +-1), zero where the gate is zero as the model feeds them."""
    B, L = c["B"], c["L"]
    hid = c["hd"] * (2 if c["bi"] else 1)
    g = th.Generator().manual_seed(seed)
    x = th.randn(B, L, c["din"] or hid, generator=g) * c["scale"]
    kind = c["gate"]
    if kind is None:
        return x, None
    gate = th.ones(B, L)
    if kind == "mixed":
        for b in range(1, B):
            n = (0, 1, L // 2, L - 1)[b % 4]
            gate[b, :L - n] = 0.0
        for t in (L // 3, L // 3 + 1, L - 2):
            if 0 <= t < L and L > 3:
                gate[0, t] = 0.0
    elif kind == "zero-row":
        gate[1] = 0.0
    elif kind == "ends":
        gate[0, 0] = 0.0
        gate[0, L - 1] = 0.0
        gate[1, 0] = 0.0
    return x * gate.unsqueeze(-1), gate


def rnn_param_names(bi):
    return [n + s for s in ([""] + (["_reverse"] if bi else [])) for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]


# -------------------------------------------------------------------------------------------------------- relational conv

def relagg_fp64(Y, bias, src, dst, et, norm, N, R, loop, H, P, act):
    """``act(sum_{e: dst e = v, 0 <= t_e < R} norm_e Y[src e, t_e] + bias + Y[v, R])`` per edge in double: Y [N, (R + loop) P]
    as blocks of P columns of which the first H count.  Edges whose type is outside [0, R) are dropped."""
    Yv = Y.view(N, R + loop, P)
    keep = (et >= 0) & (et < R)
    s, d, t = src[keep], dst[keep], et[keep]
    msg = Yv[s, t][:, :H]
    if norm is not None:
        msg = msg * norm.reshape(-1, 1)[keep]
    out = th.zeros(N, H, dtype=Y.dtype).index_add(0, d, msg)
    if bias is not None:
        out = out + bias
    if loop:
        out = out + Yv[:, R, :H]
    return th.tanh(out) if act else out


def relconv_fp64(m, x, src, dst, et, norm, act):
    """DGL 0.6's RelGraphConv (basis regulariser) in float64 on the CPU: per-edge x[src] @ W[type], times norm, summed by
    destination, plus the bias and the self-loop message where the module has them, then tanh.  Edges whose type is outside
    [0, R) are dropped.  Returns (out, x as a double leaf, the parameters as double leaves by name)."""
    p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.named_parameters()}
    xd = x.detach().cpu().double().requires_grad_(True)
    s, d, t = src.cpu(), dst.cpu(), et.cpu().reshape(-1)
    keep = (t >= 0) & (t < m.num_rels)
    s, d, t = s[keep], d[keep], t[keep]
    if "w_comp" in p:
        W = (p["w_comp"] @ p["weight"].view(m.num_bases, -1)).view(m.num_rels, m.in_feat, m.out_feat)
    else:
        W = p["weight"]
    msg = th.bmm(xd[s].unsqueeze(1), W[t]).squeeze(1)
    if norm is not None:
        msg = msg * norm.detach().cpu().double().reshape(-1, 1)[keep]
    out = th.zeros(x.size(0), m.out_feat, dtype=th.float64).index_add(0, d, msg)
    if "h_bias" in p:
        out = out + p["h_bias"]
    if "loop_weight" in p:
        out = out + xd @ p["loop_weight"]
    if act:
        out = th.tanh(out)
    return out, xd, p


def relconv_cases():
    """ids -> dict(N, E, din, width, R, bases, bias, loop, act, norm, graph, hip, band).

    graph: "random", "multi" (every (u, v, t) four times), "one-type", "self" (self-loop edges only).  ``hip`` is the path
    the case must take.  ``band``: width 516, where a row's sums run over three column passes."""
    cases = {}

    def add(name, width, R, N=131, E=700, din=24, bases=None, bias=True, loop=True, act=True, norm=True, graph="random",
            hip=True, band=False):
        cases[name] = dict(N=N, E=E, din=din, width=width, R=R, bases=bases, bias=bias, loop=loop, act=act, norm=norm,
                           graph=graph, hip=hip, band=band)

    for bias in (True, False):
        for loop in (True, False):
            for act in (True, False):
                for bases in (None, 2):
                    add("b%d-l%d-a%d-%s" % (bias, loop, act, "bases" if bases else "full"), 50, 5, bases=bases, bias=bias,
                        loop=loop, act=act, norm=act != loop)
    add("w300", 300, 3, N=90, E=500)
    add("w300-nobias-noloop", 300, 3, N=90, E=500, bias=False, loop=False)
    add("w516", 516, 2, N=70, E=400, band=True)
    add("w513", 513, 2, N=70, E=400, loop=False, band=True)
    add("w1", 1, 4)
    add("w3", 3, 4, bias=False)
    add("lds-edge", 256, 64, N=40, E=600, din=8)                        # R P 4 = 65536: one row per backward workgroup
    add("lds-over", 256, 65, N=40, E=600, din=8, hip=False)
    add("lds-edge-p4", 2, 4096, N=30, E=300, din=4, act=False)          # P = 4: a workgroup of one 4-lane group
    add("n1-self", 50, 3, N=1, E=5, graph="self")
    add("multi", 64, 4, N=40, E=100, graph="multi")
    add("one-type", 64, 6, graph="one-type")
    for width in (13, 32, 61, 128, 256):                                # 4 .. 64 lanes per row; 65 = rows per workgroup + 1
        add("n65-w%d" % width, width, 3, N=65, E=400, act=width % 2 == 0)
    return cases


def relconv_graph(c, seed):
    """(src, dst, etype, norm [E, 1]) of a case, on the CPU."""
    gen = th.Generator().manual_seed(seed)
    N, E, R = c["N"], c["E"], c["R"]
    if c["graph"] == "self":
        src = th.zeros(E, dtype=th.int64)
        dst = src.clone()
    else:
        src = th.randint(0, N, (E,), generator=gen)
        dst = th.randint(0, max(1, N - 3), (E,), generator=gen)         # the last nodes have no in-edge
    et = th.randint(0, R, (E,), generator=gen)
    if c["graph"] == "one-type":
        et = th.full((E,), R - 2, dtype=th.int64)
    if c["graph"] == "multi":
        perm = th.randperm(4 * E, generator=gen)
        src, dst, et = src.repeat(4)[perm], dst.repeat(4)[perm], et.repeat(4)[perm]
    norm = th.rand(src.numel(), 1, generator=gen) + 0.1
    return src, dst, et, norm


def relconv_make(c, seed=0):
    from dualmessagepassing_amd.unc_rel import RelGraphConv
    th.manual_seed(seed)
    m = RelGraphConv(c["din"], c["width"], c["R"], num_bases=c["bases"], bias=c["bias"], self_loop=c["loop"],
                     activation=th.nn.Tanh() if c["act"] else None)
    with th.no_grad():
        if c["bias"]:
            m.h_bias.uniform_(-0.2, 0.2)
    x = th.randn(c["N"], c["din"])
    w_out = th.randn(c["N"], c["width"])
    return m, x, w_out


def stable_seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100003
