"""Float64 CPU restatements of the CNN layer, the RNN layer, the relational conv, the pooled prediction heads and their blend,
the count loss and training-mode BatchNorm (+ activation) over the live rows of a padded batch, written from the operators'
public definitions (not by running the code under test in double), and the case lists that ``test_fp64_refs_cpu.py`` and the
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


def batch_norm_fp64(p, weight, bias, mean, var, training, momentum, eps, tracked, n=None, slope=None):
    """nn.BatchNorm1d over all rows of p [B, L', H]: (out, running mean, running var after the call).  ``momentum`` None is
    the cumulative average 1 / (batches tracked, this one included).  ``weight`` / ``bias`` None: not affine.  Training mode
    only: ``n`` (1 <= n <= rows): only the first n rows exist -- the statistics are theirs, the other rows of the output (and
    so of dx) are zeros; one row has variance 0 and leaves ``running_var`` the biased value.  ``slope``: the negative slope of
    an activation after the normalisation (None: none, 0: relu)."""
    gam = 1.0 if weight is None else weight
    bet = 0.0 if bias is None else bias
    if not training:
        return (p - mean) / th.sqrt(var + eps) * gam + bet, mean, var
    rows = p.reshape(-1, p.size(-1))
    n = rows.size(0) if n is None else n
    live = rows[:n]
    m = live.mean(0)
    v = ((live - m) ** 2).mean(0)
    f = 1.0 / (tracked + 1) if momentum is None else momentum
    with th.no_grad():
        new_mean = (1 - f) * mean + f * m
        new_var = (1 - f) * var + f * v * n / max(n - 1, 1)
    out = (live - m) / th.sqrt(v + eps) * gam + bet
    if slope is not None:
        out = th.where(out > 0, out, out * slope)
    if n < rows.size(0):
        out = th.cat([out, out.new_zeros(rows.size(0) - n, rows.size(1))])
    return out.reshape(p.shape), new_mean, new_var


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


# ---------------------------------------------------------------------------------------------------------- pooled heads

HEADS_TIE = 1e-5            # a row is unsafe when a pre-activation of its hidden layer lies within this share of max |pre| of zero
HEADS_UNSAFE_ROWS = 0.02    # at most this share of the rows of a case with B >= 255 (none at B <= 17: the seed is chosen so)
FP32_SHARE = 0.25           # the fp32 tensor-op restatement stays within this share of a non-band case's tolerance (asserted)
HEAD_PARAMS = ("Wp", "bp", "Wg", "bg", "W1", "b1", "W2", "b2")
HEADS_MAX = 2               # DMP_HEADS_MAX of include/dmp_hip.h (tests/test_lib_abi.py holds the binding to the header)


def leaky(v, slope):
    """torch's leaky_relu: the negative slope at v <= 0 (slope 0: relu)."""
    return th.where(v > 0, v, v * slope)


def heads_fp64(params, ps, gs, pl, gl, scale_p, scale_g, slope):
    """The pooled count head: p = ps Wp^T + scale_p bp, g = gs Wg^T + scale_g bg, s = [pl, gl, 1/pl, 1/gl],
    f = [p | g | g - p | g * p | s], y1 = act(f W1^T + b1), y = [y1 | s] W2^T + b2.  ``params``: Wp, bp, Wg, bg, W1, b1, W2, b2
    in nn.Linear layout; ps, gs [B, H]; pl, gl [B, 1].  Returns (y [B, 1], the pre-activation [B, H], safe [B] bool: no entry of
    the row's pre-activation within HEADS_TIE max |pre| of zero).  Runs in the dtype of its arguments."""
    Wp, bp, Wg, bg, W1, b1, W2, b2 = params
    p = ps @ Wp.t() + scale_p * bp
    g = gs @ Wg.t() + scale_g * bg
    s = th.cat([pl, gl, 1.0 / pl, 1.0 / gl], 1)
    f = th.cat([p, g, g - p, g * p, s], 1)
    pre = f @ W1.t() + b1
    y = th.cat([leaky(pre, slope), s], 1) @ W2.t() + b2
    with th.no_grad():
        safe = (pre.abs() > HEADS_TIE * pre.abs().max()).all(1)
    return y, pre.detach(), safe


def heads_blend_fp64(ys, gls):
    """Blend by the sizes of the target graphs: weights gl_i / sum_j gl_j (list of [B, 1]), the blended count sum_i w_i y_i."""
    total = sum(gls)
    ws = [g / total for g in gls]
    return sum(w * y for w, y in zip(ws, ys)), ws


def heads_cases():
    """ids -> dict(H, slope, B, heads, blend (None, "given", "len"), pool ("sum": bias factors L; "mean": 1), stride (None, "pass":
    a column slice the op passes through, "copy": one it has to copy), lmax (pl, gl in 1..8 / 1..64, or both in 1..lmax), band).

    Every B at both widths with every slope; the head count and the blend, the bias factors and the row stride rotate over the
    six cases of a B, shifted from one B to the next, so each meets every tile edge; ``band``: B >= 1024."""
    cases = {}
    combos = [(1, None), (2, "given"), (2, "len"), (2, None)]
    strides = [None, "pass", "copy"]
    for hi, H in enumerate((64, 128)):
        for bi, B in enumerate((1, 3, 15, 16, 17, 255, 256, 257, 1024, 1025)):
            for si, slope in enumerate((0.0, 1.0 / 5.5, 0.01)):
                k = 3 * hi + si                                   # 0 .. 5 within one B: all four combos, all three strides
                heads, blend = combos[(k + bi) % 4]
                pool, stride = "mean" if (k + bi) % 3 == 0 else "sum", strides[(k + 2 * bi) % 3]
                cases["H%d-B%d-s%.2g-%dh-%s-%s-%s" % (H, B, slope, heads, blend or "sum", pool, stride or "dense")] = dict(
                    H=H, slope=slope, B=B, heads=heads, blend=blend, pool=pool, stride=stride, lmax=None, band=B >= 1024)
    cases["H128-B257-len512"] = dict(H=128, slope=1.0 / 5.5, B=257, heads=2, blend="len", pool="sum", stride=None, lmax=512, band=False)
    cases["H64-B17-len512"] = dict(H=64, slope=0.0, B=17, heads=1, blend=None, pool="sum", stride="pass", lmax=512, band=False)
    return cases


def heads_stride_geometry(H, kind):
    """(width of the matrix the rows are a column slice of, first column).  "pass": stride H + 8 and a start 16 bytes in, which
    the kernels take as they are; "copy": stride H + 6, no multiple of 4."""
    return {None: (H, 0), "pass": (H + 8, 4), "copy": (H + 6, 1)}[kind]


def heads_inputs(name):
    """The CPU inputs of a case: dict(params: per head the eight tensors N(0, 0.2); wide: per head [2B, width] N(0, 1), of which
    columns c0 .. c0 + H are the pattern sums (rows < B) and the target sums; pl, gl: per head [B, 1]; Lp, Lg: the padded
    lengths; scale_p, scale_g; blends: per head [B, 1] or None; cot [B, 1]; c0).  At B <= 17 the first seed at which no row of
    any head is unsafe."""
    c = heads_cases()[name]
    H, B, n = c["H"], c["B"], c["heads"]
    width, c0 = heads_stride_geometry(H, c["stride"])
    Lp, Lg = (8.0, 64.0) if c["lmax"] is None else (float(c["lmax"]),) * 2
    sp, sg = (Lp, Lg) if c["pool"] == "sum" else (1.0, 1.0)
    for seed in range(stable_seed(name), stable_seed(name) + 64):
        g = th.Generator().manual_seed(seed)
        params = [[th.randn(shape, generator=g) * 0.2 for shape in ((H, H), (H,), (H, H), (H,), (H, 4 * H + 4), (H,), (1, H + 4), (1,))]
                  for _ in range(n)]
        wide = [th.randn(2 * B, width, generator=g) for _ in range(n)]
        pls = [th.randint(1, int(Lp) + 1, (B, 1), generator=g).float() for _ in range(n)]
        gls = [th.randint(1, int(Lg) + 1, (B, 1), generator=g).float() for _ in range(n)]
        cot = th.randn(B, 1, generator=g)
        blends = [None] * n
        if c["blend"] == "given":
            blends = [gl / sum(gls) for gl in gls]
        d = dict(params=params, wide=wide, pl=pls, gl=gls, Lp=Lp, Lg=Lg, scale_p=sp, scale_g=sg, blends=blends, cot=cot, c0=c0)
        if B > 17 or bool(heads_reference(c, d)["safe"].all()):
            return d
    raise AssertionError("no seed without an unsafe row for " + name)


def heads_reference(c, d, dtype=th.float64, device="cpu", safe=None):
    """The blended count of a case and, with the cotangent zeroed on the unsafe rows, d wide and the eight parameter gradients
    per head, from ``heads_fp64`` / ``heads_blend_fp64`` in ``dtype`` (float64: the reference; float32: the tensor-op
    yardstick, which takes the reference's ``safe``)."""
    H, B, c0 = c["H"], c["B"], d["c0"]
    cast = lambda t: t.detach().to(device=device, dtype=dtype)
    params = [[cast(t).requires_grad_(True) for t in head] for head in d["params"]]
    wide = [cast(t).requires_grad_(True) for t in d["wide"]]
    ys, ok = [], th.ones(B, dtype=th.bool, device=device)
    for prm, w, pl, gl in zip(params, wide, d["pl"], d["gl"]):
        y, _, s = heads_fp64(prm, w[:B, c0:c0 + H], w[B:, c0:c0 + H], cast(pl), cast(gl), d["scale_p"], d["scale_g"], c["slope"])
        ys.append(y)
        ok &= s
    if c["blend"] == "len":
        y = heads_blend_fp64(ys, [cast(g) for g in d["gl"]])[0]
    else:
        y = sum(yi if b is None else cast(b) * yi for yi, b in zip(ys, d["blends"]))
    safe = ok if safe is None else safe.to(device)
    (y * cast(d["cot"]) * safe.view(-1, 1).to(dtype)).sum().backward()
    return dict(y=y.detach(), safe=safe.cpu(), dwide=[w.grad for w in wide], dparams=[[t.grad for t in head] for head in params])


# ------------------------------------------------------------------------------------------------------------ count loss

LOSS_KINDS = ("MSE", "MAE", "SMSE")          # kind 0, 1, 2 of dmp_count_loss; SMSE: smooth L1 with beta 1


def count_loss_fp64(pred, target, kind, slope):
    """mean_i crit(act(pred_i) - target_i) and its gradient by pred, in double: act = leaky_relu(slope) with the negative slope
    at pred <= 0; MSE d^2; MAE |d| with sign(0) = 0; smooth L1 d^2 / 2 inside |d| < 1 and |d| - 1/2 from |d| = 1 on."""
    p, t = pred.detach().cpu().double().reshape(-1), target.detach().cpu().double().reshape(-1)
    da = th.where(p > 0, th.ones_like(p), th.full_like(p, slope))
    d = p * da - t
    if kind == "MSE":
        v, g = d * d, 2 * d
    elif kind == "MAE":
        v, g = d.abs(), th.sign(d)
    else:
        inside = d.abs() < 1
        v, g = th.where(inside, 0.5 * d * d, d.abs() - 0.5), th.where(inside, d, th.sign(d))
    return v.mean(), (g * da / p.numel()).reshape(pred.shape)


def count_loss_cases():
    """ids -> (n, kind, slope, band): n on both sides of the workgroup's 1024 threads, the three criteria, slopes 1 (no
    activation), 0.01 and 0 (relu); ``band``: n = 65537."""
    return {"n%d-%s-s%g" % (n, kind, slope): (n, kind, slope, n == 65537)
            for n in (1, 2, 1023, 1024, 1025, 4096, 65537) for kind in LOSS_KINDS for slope in (1.0, 0.01, 0.0)}


def count_loss_inputs(name):
    """(pred [n, 1] N(0, 3), target [n, 1] integers 0 .. 5).  The first min(n, 16) entries sit exactly on the kinks, four kinds in
    turn starting at one the case's name picks (so n = 1 and n = 2 meet all of them over the cases): pred = 0;
    act(pred) = target; act(pred) - target = 1; act(pred) - target = -1.  All of these are exact in fp32."""
    n, kind, slope, _ = count_loss_cases()[name]
    g = th.Generator().manual_seed(stable_seed(name))
    pred = th.randn(n, 1, generator=g) * 3
    target = th.randint(0, 6, (n, 1), generator=g).float()
    for i in range(min(n, 16)):
        t = float(target[i])
        k = (i + stable_seed(name)) % 4
        if k == 0:
            pred[i] = 0.0
        elif k == 1:
            pred[i] = t                                   # t = 0: pred = 0 is on two kinks at once
        elif k == 2:
            pred[i] = t + 1.0
        elif t >= 2:
            pred[i] = t - 1.0
        else:
            pred[i], target[i] = 0.0, 1.0                 # act(0) = 0 whatever the slope
    return pred, target


# -------------------------------------------------------------------------------------------------------------- BatchNorm

BN_WIDTHS = (4, 8, 16, 32, 64, 128, 256, 512, 1024)      # every width csrc/dmp_bn.hip admits: C / 4 divides 256, C <= 1024
BN_SLOPES = (None, 0.0, 1.0 / 5.5)
BN_VAR_FLOOR = 1.0          # of a column over two or three live rows (see bn_inputs); the rows are drawn with variance 9


def bn_rows(C):
    """Row counts around the rows a workgroup takes per pass (256 lanes, C / 4 lanes per row)."""
    rpp = 256 // (C // 4)
    return sorted({2, 3, rpp - 1, rpp, rpp + 1, 4 * rpp + 1} - {0, 1})


def bn_cases():
    """ids -> dict(C, affine, runs: [(R, live row count or None, slope)], outlier, band, momentum).

    "C<width>-affine<0/1>": every row count of ``bn_rows`` with every slope.  "long-*": 70001 x 128 (band) and 10858 x 256.
    "pad-C*": a batch padded to cap = 4 rows_per_pass + 3 rows (259 for "pad-C16-plain": not affine, no activation) with live counts 1, 2, cap - 1, cap, and 0 and cap + 7, which the
    kernel clamps to 1 and cap.  "outlier-*" (band): row 0 at 50 standard deviations from the column mean."""
    cases = {}
    for C in BN_WIDTHS:
        for affine in (True, False):
            cases["C%d-affine%d" % (C, affine)] = dict(C=C, affine=affine, runs=[(R, None, s) for R in bn_rows(C) for s in BN_SLOPES],
                                                       outlier=False, band=False, momentum=0.1 if affine else 0.3)
    cases["long-128"] = dict(C=128, affine=True, runs=[(70001, None, 1.0 / 5.5)], outlier=False, band=True, momentum=0.1)
    cases["long-256"] = dict(C=256, affine=True, runs=[(10858, None, 0.0)], outlier=False, band=False, momentum=0.1)
    for i, C in enumerate((8, 64, 256, 1024)):
        cap = 4 * (256 // (C // 4)) + 3
        cases["pad-C%d" % C] = dict(C=C, affine=True, outlier=False, band=False, momentum=0.1,
                                    runs=[(cap, n, BN_SLOPES[(i + j) % 3]) for j, n in enumerate((1, 2, cap - 1, cap, 0, cap + 7))])
    # not affine: one live row comes out as exact zeros, which an activation would have to be masked on entirely
    cases["pad-C16-plain"] = dict(C=16, affine=False, outlier=False, band=False, momentum=0.3,
                                  runs=[(259, n, None) for n in (1, 2, 258, 259, 0, 266)])
    cases["outlier-256"] = dict(C=256, affine=True, runs=[(2708, None, 1.0 / 5.5)], outlier=True, band=True, momentum=0.1)
    cases["outlier-128"] = dict(C=128, affine=True, runs=[(70001, None, None)], outlier=True, band=True, momentum=0.1)
    return cases


def bn_live(R, n):
    """The row count the kernels use for a device-side count n on a batch of capacity R: clamped to [1, R]."""
    return R if n is None else min(max(n, 1), R)


def bn_inputs(name, run, C=None):
    """(x [R, C], dy [R, C], gamma, beta, running mean, running var) of run ``run`` of a case: rows 3 N(0, 1) + 5 N(0, 1) per
    column (means far from 0), as ``test_gpu_batchnorm.py`` draws them; +-1e6 in the padding rows of x and dy; with ``outlier``
    row 0 sits 50 standard deviations of the other rows above their mean; with two or three live rows no column's variance is
    under BN_VAR_FLOOR."""
    c = bn_cases()[name]
    C = C or c["C"]
    R, n, _ = c["runs"][run]
    g = th.Generator().manual_seed(stable_seed(name) + run)
    x = th.randn(R, C, generator=g) * 3.0 + th.randn(C, generator=g) * 5.0
    dy = th.randn(R, C, generator=g)
    gamma, beta = th.rand(C, generator=g) + 0.5, th.randn(C, generator=g)
    mean, var = th.randn(C, generator=g), th.rand(C, generator=g) + 0.5
    if c["outlier"]:
        x[0] = x[1:].mean(0) + 50.0 * x[1:].std(0)
    live = bn_live(R, n)
    bn_floor_rows(x, live)
    if n is not None:
        x[live:] = 1e6
        dy[live:] = -1e6
        x[live::2] = -1e6
    return x, dy, gamma, beta, mean, var


def bn_floor_rows(x, live):
    if 2 <= live <= 3:
        # two or three rows that nearly agree in a column: half an ulp of the column mean (|x| up to 30: 1e-6) moves xhat by
        # 1e-6 / sqrt(var + eps), up to 3e-4, in any fp32 statement, the tensor ops' included, and dx, which all but cancels
        # over two rows, by as much.  A column under the floor gets its second row put four above its first (the rows are
        # drawn with standard deviation 3).
        flat = x[:live].double().var(0, unbiased=False) < BN_VAR_FLOOR
        x[1, flat] = x[0, flat] + 4.0


def bn_reference(x, dy, gamma, beta, mean, var, momentum, eps, live, slope, steps=2, dtype=th.float64, safe=None, tracked=0):
    """``steps`` consecutive training calls of BatchNorm (+ activation) on the same rows through ``batch_norm_fp64`` in
    ``dtype``: dict(y, mean, var (the running statistics after the last call), dx, dgamma, dbeta (of the last call, the
    upstream gradient zeroed where ``safe`` is False), safe: |the value before the activation| > TAU, all True without one)."""
    cast = lambda t: None if t is None else t.detach().cpu().to(dtype)
    xd = cast(x).requires_grad_(True)
    gd, bd = (None, None) if gamma is None else (cast(gamma).requires_grad_(True), cast(beta).requires_grad_(True))
    m, v = cast(mean), cast(var)
    for step in range(steps):
        pre, _, _ = batch_norm_fp64(xd, gd, bd, m, v, True, momentum, eps, tracked + step, n=live)
        y, m, v = batch_norm_fp64(xd, gd, bd, m, v, True, momentum, eps, tracked + step, n=live, slope=slope)
    if safe is None:
        safe = th.ones_like(pre, dtype=th.bool) if slope is None else pre.detach().abs() > TAU
        safe[live:] = True                                # padding rows: the output and dx are zeros whatever arrives
    grads = th.autograd.grad(y, [xd] + ([] if gd is None else [gd, bd]), th.where(safe, cast(dy), th.zeros((), dtype=dtype)))
    return dict(y=y.detach(), mean=m, var=v, dx=grads[0], dgamma=None if gd is None else grads[1],
                dbeta=None if gd is None else grads[2], safe=safe)


MASKED_BN_RUNS = [(1024, n, momentum) for n in (1, 3, 700, 0, 1031) for momentum in (0.1, None)]   # (cap, rows_dev, momentum)


def masked_bn_inputs(cap, n, C=64):
    """(x [cap, C], dy, gamma, beta, running mean, running var) for ``ops.masked_batch_norm``: 64 columns, of which the first 50
    are the reference's shipped UNC width (no multiple of 4: tensor ops) and all 64 the next width the kernels take (52 is
    none: 13 lanes per row do not divide a workgroup's 256); +-1e4 in the padding rows."""
    g = th.Generator().manual_seed(cap + n + C)
    x = th.randn(cap, C, generator=g) * 2.0 + 3.0
    dy = th.randn(cap, C, generator=g)
    live = bn_live(cap, n)
    bn_floor_rows(x, live)
    x[live:], dy[live:] = 1e4, -1e4
    return x, dy, th.rand(C, generator=g) + 0.5, th.randn(C, generator=g), th.randn(C, generator=g), th.rand(C, generator=g) + 0.5
