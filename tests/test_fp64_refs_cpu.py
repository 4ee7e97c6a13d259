"""The float64 references of ``util_fp64.py`` against the project's own CPU path in float64 (``CNNLayer``, ``RNNLayer``,
``RelGraphConv`` after ``.double()``), outputs and every gradient to 1e-10, at every case the GPU modules
``test_gpu_cnn_fp64.py``, ``test_gpu_rnn_fp64.py`` and ``test_gpu_relconv_fp64.py`` parametrize (the case lists are shared):
two independent statements agreeing in double is what makes the yardstick trustworthy before a GPU is involved.  Also the
condition on the conv inputs: at most 0.1 % of a case's outputs are unsafe (near-ties of the pool or of the activation)."""
import pytest
import torch as th

import util_fp64 as U

TOL = 1e-10


def _leaf(t):
    return t.detach().double().clone().requires_grad_(True)


def _cnn_ref(layer, x, gate, residual, w, post=None):
    """Reference run with the upstream weight masked by the safe flag: (y, gate', safe, dx, dW, db)."""
    c, p = layer.conv, layer.pool
    W, b, xd = _leaf(c.weight), _leaf(c.bias), _leaf(x)
    y, g, safe, _ = U.cnn_layer_fp64(W, b, xd, gate, c.kernel_size[0], c.padding[0], p.kernel_size, p.padding,
                                     U.cnn_slope(layer.act_func), residual, post=post)
    (y * w.double() * safe).sum().backward()
    return y.detach(), g, safe, xd.grad, W.grad, b.grad


def _cnn_project(layer, x, gate, residual, w, safe):
    layer.zero_grad(set_to_none=True)
    xd = _leaf(x)
    y, g = layer.forward_rows(xd, None if gate is None else gate.double(), residual)
    (y * w.double() * safe).sum().backward()
    return y.detach(), g, xd.grad, layer.conv.weight.grad, layer.conv.bias.grad


@pytest.mark.parametrize("case", sorted(U.cnn_layer_cases()))
def test_cnn_reference_equals_the_layer_in_double(case):
    H, k, pad, act = U.cnn_layer_cases()[case]
    layer = U.cnn_make_layer(H, k, pad, act).double()
    unsafe = total = 0
    for n, (B, L, gated, residual) in enumerate(U.cnn_layer_runs(k, pad)):
        x, gate = U.cnn_inputs(B, L, H, gated, U.stable_seed(case) + n)
        Lout = L + 4 * pad - 2 * k + 2
        w = th.randn(B, Lout, H, generator=th.Generator().manual_seed(5 + n))
        y0, g0, safe, dx0, dW0, db0 = _cnn_ref(layer, x, gate, residual, w)
        y1, g1, dx1, dW1, db1 = _cnn_project(layer, x, gate, residual, w, safe)
        what = "%s run %d" % (case, n)
        U.close(y1, y0, TOL, what + " y")
        assert (g0 is None) == (g1 is None) and (g0 is None or th.equal(g0, g1)), what
        U.close(dx1, dx0, TOL, what + " dx")
        U.close(dW1, dW0, TOL, what + " dW")
        U.close(db1, db0, TOL, what + " db")
        unsafe += int((~safe).sum())
        total += safe.numel()
    assert unsafe <= U.UNSAFE_CAP * total, (case, unsafe, total)


def test_cnn_lengths_sit_on_the_tile_edges():
    assert len(U.cnn_geometries()) == 24
    for k, pad in U.cnn_geometries():
        tp = 65 - k
        louts = {L + 4 * pad - 2 * k + 2 for L in U.cnn_lengths(k, pad)}
        assert {tp - 1, tp, tp + 1, 2 * tp, 2 * tp + 1} <= louts and min(louts) >= 1
        lmin = min(U.cnn_lengths(k, pad))
        assert lmin >= 1 and lmin + 2 * pad - k + 1 >= 1
        assert lmin == 1 or lmin - 1 + 2 * pad - k + 1 < 1 or lmin - 1 + 4 * pad - 2 * k + 2 < 1
        assert any(B == 1 for B, _, _, _ in U.cnn_layer_runs(k, pad))


@pytest.mark.parametrize("case", sorted(U.cnn_bn_cases()))
def test_cnn_reference_with_batch_norm_equals_the_layer_in_double(case):
    H, k, pad, act, training, momentum, B, L = U.cnn_bn_cases()[case]
    layer = U.cnn_make_layer(H, k, pad, act, bn=True, momentum=momentum).double()
    layer.train(training)
    bn = layer.bn
    x, gate = U.cnn_bn_inputs(case, layer)
    w = th.randn(B, L + 4 * pad - 2 * k + 2, H, generator=th.Generator().manual_seed(5))
    stats = {}
    gamma, beta = _leaf(bn.weight), _leaf(bn.bias)
    mean0, var0 = bn.running_mean.clone(), bn.running_var.clone()

    def post(p):
        o, stats["mean"], stats["var"] = U.batch_norm_fp64(p, gamma, beta, mean0, var0, training, momentum, bn.eps,
                                                           int(bn.num_batches_tracked))
        return o

    y0, g0, safe, dx0, dW0, db0 = _cnn_ref(layer, x, gate, True, w, post=post)
    y1, g1, dx1, dW1, db1 = _cnn_project(layer, x, gate, True, w, safe)
    if training:
        assert bool(safe.all()), (case, int((~safe).sum()))
    else:
        assert int((~safe).sum()) <= U.UNSAFE_CAP * safe.numel()
    U.close(y1, y0, TOL, "y")
    assert th.equal(g0, g1)
    for a, b, n in ((dx1, dx0, "dx"), (dW1, dW0, "dW"), (db1, db0, "db"), (bn.weight.grad, gamma.grad, "dgamma"),
                    (bn.bias.grad, beta.grad, "dbeta"), (bn.running_mean, stats["mean"], "running_mean"),
                    (bn.running_var, stats["var"], "running_var")):
        U.close(a, b, TOL, n)


@pytest.mark.parametrize("case", sorted(U.rnn_cases()))
def test_rnn_reference_equals_the_layer_in_double(case):
    c = U.rnn_cases()[case]
    layer = U.rnn_make_layer(c).double()
    x, gate = U.rnn_inputs(c)
    names = U.rnn_param_names(c["bi"])
    params = [_leaf(getattr(layer.layer, n)) for n in names]
    xd = _leaf(x)
    y0 = U.rnn_layer_fp64(c["cell"], params, xd, None if gate is None else gate.double(), c["residual"])
    w = th.randn(y0.shape, generator=th.Generator().manual_seed(5)).double()
    (y0 * w).sum().backward()
    xp = _leaf(x)
    y1 = layer.forward_rows(xp, None if gate is None else gate.double(), c["residual"])
    (y1 * w).sum().backward()
    assert y0.size(2) == c["hd"] * (2 if c["bi"] else 1)
    U.close(y1, y0, TOL, "y")
    U.close(xp.grad, xd.grad, TOL, "dx")
    for n, p in zip(names, params):
        U.close(getattr(layer.layer, n).grad, p.grad, TOL, n)
    if c["band"]:
        return
    # the condition on a short case's inputs: the same loop in float32 keeps a fourfold distance from the GPU modules' 1e-4 /
    # 2e-4, so what a kernel is held to there is not the rounding of the number format itself
    p32 = [getattr(layer.layer, n).detach().float().requires_grad_(True) for n in names]
    x32 = x.clone().requires_grad_(True)
    y2 = U.rnn_layer_fp64(c["cell"], p32, x32, gate, c["residual"])
    (y2 * w.float()).sum().backward()
    U.close(y2, y0, U.RNN_FP32_SHARE * 1e-4, "fp32 loop y")
    U.close(x32.grad, xd.grad, U.RNN_FP32_SHARE * 2e-4, "fp32 loop dx")
    for q, p, n in zip(p32, params, names):
        U.close(q.grad, p.grad, U.RNN_FP32_SHARE * 2e-4, "fp32 loop " + n)


@pytest.mark.parametrize("case", sorted(U.relconv_cases()))
def test_relconv_reference_equals_the_module_in_double(case):
    from dualmessagepassing_amd.graph import BatchedGraph
    c = U.relconv_cases()[case]
    m, x, w_out = U.relconv_make(c)
    src, dst, et, norm = U.relconv_graph(c, U.stable_seed(case))
    norm = norm if c["norm"] else None
    ref, xd, p = U.relconv_fp64(m, x, src, dst, et, norm, c["act"])
    (ref * w_out.double()).sum().backward()
    m = m.double()
    xp = _leaf(x)
    out = m(BatchedGraph(src, dst, c["N"]), xp, et, None if norm is None else norm.double())
    (out * w_out.double()).sum().backward()
    U.close(out, ref, TOL, "out")
    U.close(xp.grad, xd.grad, TOL, "dx")
    assert sorted(p) == sorted(k for k, _ in m.named_parameters())
    for k, q in m.named_parameters():
        U.close(q.grad, p[k].grad, TOL, "grad " + k)


def test_relagg_reference_drops_edges_of_unknown_type_and_equals_the_layer_reference():
    c = dict(U.relconv_cases()["b1-l1-a1-full"])
    m, x, w_out = U.relconv_make(c)
    src, dst, et, norm = U.relconv_graph(c, 3)
    bad = et.clone()
    bad[::7] = -1
    bad[3::11] = c["R"]
    keep = (bad >= 0) & (bad < c["R"])
    a, _, _ = U.relconv_fp64(m, x, src, dst, bad, norm, True)
    b, _, _ = U.relconv_fp64(m, x, src[keep], dst[keep], bad[keep], norm[keep], True)
    assert th.equal(a, b) and 0 < int(keep.sum()) < keep.numel()
    P = (c["width"] + 3) // 4 * 4
    Y = x.double() @ m.double().stacked_weight(P)
    o = U.relagg_fp64(Y, m.h_bias.double(), src, dst, bad, norm.double(), c["N"], c["R"], 1, c["width"], P, True)
    U.close(o, a, TOL, "relagg")
