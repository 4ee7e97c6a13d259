"""The float64 references of ``util_fp64.py`` against the project's own CPU path in float64 (``CNNLayer``, ``RNNLayer``,
``RelGraphConv`` after ``.double()``), outputs and every gradient to 1e-10, at every case the GPU modules
``test_gpu_cnn_fp64.py``, ``test_gpu_rnn_fp64.py`` and ``test_gpu_relconv_fp64.py`` parametrize (the case lists are shared):
two independent statements agreeing in double is what makes the yardstick trustworthy before a GPU is involved.  Also the
condition on the conv inputs: at most 0.1 % of a case's outputs are unsafe (near-ties of the pool or of the activation).

Likewise for ``test_gpu_heads_fp64.py`` and ``test_gpu_bn_fp64.py``: the pooled heads against the op-by-op ``pred._PooledHead``
in double, the count loss against torch's criteria in double, BatchNorm (+ activation) against ``nn.BatchNorm1d`` in double on
the live rows (one live row, which the module refuses, against the closed form), ``ops.masked_batch_norm`` in double against
the same reference; the shares of unsafe rows / entries; and, for every case that is held to a fixed tolerance, that the
restatement run in float32 stays within a quarter of it."""
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


# ------------------------------------------------------------------------------------- pooled heads, count loss, BatchNorm

@pytest.mark.parametrize("case", sorted(U.heads_cases()))
def test_heads_reference_equals_the_op_by_op_head_in_double(case):
    from dualmessagepassing_amd.pred import _PooledHead
    c = U.heads_cases()[case]
    d = U.heads_inputs(case)
    H, B, c0 = c["H"], c["B"], d["c0"]
    ref = U.heads_reference(c, d)
    unsafe = int((~ref["safe"]).sum())
    assert unsafe == 0 if B <= 17 else unsafe <= U.HEADS_UNSAFE_ROWS * B, (case, unsafe, B)
    assert c["band"] == (B >= 1024) and c["heads"] <= U.HEADS_MAX
    params = [[_leaf(t) for t in head] for head in d["params"]]
    wide = [_leaf(t) for t in d["wide"]]
    ys = [_PooledHead.apply(w[:B, c0:c0 + H], w[B:, c0:c0 + H], pl.double(), gl.double(), d["scale_p"], d["scale_g"], *prm, c["slope"])
          for prm, w, pl, gl in zip(params, wide, d["pl"], d["gl"])]
    total = sum(g.double() for g in d["gl"])
    blends = [g.double() / total for g in d["gl"]] if c["blend"] == "len" else d["blends"]
    y = sum(yi if b is None else b.double() * yi for yi, b in zip(ys, blends))
    (y * d["cot"].double() * ref["safe"].view(-1, 1)).sum().backward()
    U.close(y, ref["y"], TOL, "y")
    for i in range(c["heads"]):
        U.close(wide[i].grad, ref["dwide"][i], TOL, "d sums %d" % i)
        lo, hi = ref["dwide"][i][:, :c0], ref["dwide"][i][:, c0 + H:]
        assert not bool(lo.any()) and not bool(hi.any())
        for n, a, b in zip(U.HEAD_PARAMS, params[i], ref["dparams"][i]):
            U.close(a.grad, b, TOL, "d%s %d" % (n, i))
    if c["band"]:
        return
    y32 = U.heads_reference(c, d, dtype=th.float32, safe=ref["safe"])
    U.close(y32["y"], ref["y"], U.FP32_SHARE * 1e-5, "fp32 y")
    for i in range(c["heads"]):
        U.close(y32["dwide"][i], ref["dwide"][i], U.FP32_SHARE * 1e-4, "fp32 d sums %d" % i)
        for n, a, b in zip(U.HEAD_PARAMS, y32["dparams"][i], ref["dparams"][i]):
            U.close(a, b, U.FP32_SHARE * 1e-4, "fp32 d%s %d" % (n, i))


def test_heads_cases_meet_every_tile_edge_with_every_feature():
    cs = list(U.heads_cases().values())
    for B in (1, 3, 15, 16, 17, 255, 256, 257, 1024, 1025):
        mine = [c for c in cs if c["B"] == B]
        assert {c["H"] for c in mine} == {64, 128} and len({c["slope"] for c in mine}) == 3
        assert {c["stride"] for c in mine} >= {None, "pass", "copy"}
        assert {(c["heads"], c["blend"]) for c in mine} >= {(1, None), (2, "given"), (2, "len")}
        assert {c["pool"] for c in mine} == {"sum", "mean"}
    assert any(c["lmax"] == 512 for c in cs)
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dmp_hip.h")) as f:
        assert int(re.search(r"#define\s+DMP_HEADS_MAX\s+(\d+)", f.read()).group(1)) == U.HEADS_MAX == max(c["heads"] for c in cs)


@pytest.mark.parametrize("case", sorted(U.count_loss_cases()))
def test_count_loss_reference_equals_the_criterion_in_double(case):
    import torch.nn.functional as F
    n, kind, slope, band = U.count_loss_cases()[case]
    pred, target = U.count_loss_inputs(case)
    crit = {"MSE": F.mse_loss, "MAE": F.l1_loss, "SMSE": F.smooth_l1_loss}[kind]
    loss0, dp0 = U.count_loss_fp64(pred, target, kind, slope)
    for dtype, tol in ((th.float64, TOL),) + (() if band else ((th.float32, U.FP32_SHARE * 1e-5),)):
        p = pred.to(dtype).requires_grad_(True)
        loss = crit(F.leaky_relu(p, slope), target.to(dtype))
        loss.backward()
        U.close(loss, loss0, tol, "%s loss" % dtype)
        U.close(p.grad, dp0, tol, "%s dpred" % dtype)
    # the entries on the kinks are there, and exactly there
    m = min(n, 16)
    p, t = pred[:m, 0].double(), target[:m, 0].double()
    dlt = U.leaky(p, slope) - t
    assert bool(((p == 0) | (dlt == 0) | (dlt.abs() == 1)).all())
    if n >= 16:
        assert bool((p == 0).any()) and bool((dlt == 0).any()) and bool((dlt == 1).any()) and bool((dlt == -1).any())


def test_count_loss_reference_follows_the_conventions_at_the_kinks():
    pred, target = th.tensor([0.0, 2.0, 3.0, 1.0, 0.0]), th.tensor([4.0, 2.0, 2.0, 2.0, 0.0])
    for kind, want in (("MAE", [-0.5, 0.0, 1.0, -1.0, 0.0]), ("SMSE", [-0.5, 0.0, 1.0, -1.0, 0.0]), ("MSE", [-4.0, 0.0, 2.0, -2.0, 0.0])):
        loss, dp = U.count_loss_fp64(pred, target, kind, 0.5)
        assert dp.mul(5).tolist() == want, (kind, dp.mul(5).tolist())
    assert float(U.count_loss_fp64(pred, target, "SMSE", 0.5)[0]) == (3.5 + 0 + 0.5 + 0.5 + 0) / 5


def _module_bn(C, affine, momentum, gamma, beta, mean, var):
    bn = th.nn.BatchNorm1d(C, affine=affine, momentum=momentum).double()
    with th.no_grad():
        bn.running_mean.copy_(mean)
        bn.running_var.copy_(var)
        if affine:
            bn.weight.copy_(gamma)
            bn.bias.copy_(beta)
    return bn


@pytest.mark.parametrize("case", sorted(U.bn_cases()))
def test_batch_norm_reference_equals_the_module_in_double_on_the_live_rows(case):
    c = U.bn_cases()[case]
    C, affine = c["C"], c["affine"]
    unsafe = total = 0
    for run, (R, n, slope) in enumerate(c["runs"]):
        x, dy, gamma, beta, mean, var = U.bn_inputs(case, run)
        live = U.bn_live(R, n)
        if not affine:
            gamma = beta = None
        ref = U.bn_reference(x, dy, gamma, beta, mean, var, c["momentum"], 1e-5, live, slope)
        unsafe += int((~ref["safe"]).sum())
        total += live * C
        what = "%s run %d " % (case, run)
        assert not bool(ref["y"][live:].any()) and not bool(ref["dx"][live:].any()), what
        dyl = th.where(ref["safe"], dy.double(), th.zeros((), dtype=th.float64))[:live]
        if live > 1:
            bn = _module_bn(C, affine, c["momentum"], gamma, beta, mean, var)
            xl = _leaf(x[:live])
            for _ in range(2):
                y = bn(xl)
                y = y if slope is None else U.leaky(y, slope)
            got = th.autograd.grad(y, [xl] + list(bn.parameters()), dyl)
            U.close(y, ref["y"][:live], TOL, what + "y")
            U.close(bn.running_mean, ref["mean"], TOL, what + "running_mean")
            U.close(bn.running_var, ref["var"], TOL, what + "running_var")
            U.close(got[0], ref["dx"][:live], TOL, what + "dx")
            if affine:
                U.close(got[1], ref["dgamma"], TOL, what + "dgamma")
                U.close(got[2], ref["dbeta"], TOL, what + "dbeta")
        else:       # the module refuses one row; the closed form: xhat = 0, variance 0 (and unbiased: 0, nothing to divide by)
            b = th.zeros(C, dtype=th.float64) if beta is None else beta.double()
            act = b if slope is None else U.leaky(b, slope)
            dact = th.ones_like(b) if slope is None else th.where(b > 0, th.ones_like(b), th.full_like(b, slope))
            U.close(ref["y"][0], act, TOL, what + "y")
            assert not bool(ref["dx"].any()), what
            m = c["momentum"]
            U.close(ref["mean"], (1 - m) ** 2 * mean.double() + (1 - (1 - m) ** 2) * x[0].double(), TOL, what + "running_mean")
            U.close(ref["var"], (1 - m) ** 2 * var.double(), TOL, what + "running_var")
            if affine:
                assert not bool(ref["dgamma"].any())
                U.close(ref["dbeta"], dact * dyl[0], TOL, what + "dbeta")
        if 2 <= live <= 3:
            assert float(x[:live].double().var(0, unbiased=False).min()) >= U.BN_VAR_FLOOR
        if c["outlier"]:
            xd = x.double()
            z = (xd[0] - xd[1:].mean(0)) / xd[1:].std(0)
            assert 49.9 < float(z.min()) and float(z.max()) < 50.1, (float(z.min()), float(z.max()))
        if c["band"]:
            continue
        y32 = U.bn_reference(x, dy, gamma, beta, mean, var, c["momentum"], 1e-5, live, slope, dtype=th.float32, safe=ref["safe"])
        U.close(y32["y"], ref["y"], U.FP32_SHARE * 1e-5, what + "fp32 y")
        U.close(y32["mean"], ref["mean"], U.FP32_SHARE * 1e-5, what + "fp32 running_mean")
        U.close(y32["var"], ref["var"], U.FP32_SHARE * 1e-5, what + "fp32 running_var")
        for k in ("dx", "dgamma", "dbeta"):
            if ref[k] is not None:
                U.close(y32[k], ref[k], U.FP32_SHARE * 5e-5, what + "fp32 " + k)
    assert unsafe <= U.UNSAFE_CAP * total, (case, unsafe, total)


def test_batch_norm_cases_cover_every_admitted_width_and_the_pass_edges():
    cs = U.bn_cases()
    admitted = [C for C in range(1, 1100) if C % 4 == 0 and C <= 1024 and 256 % (C // 4) == 0]
    assert list(U.BN_WIDTHS) == admitted
    for C in U.BN_WIDTHS:
        rpp = 256 // (C // 4)
        for affine in (True, False):
            c = cs["C%d-affine%d" % (C, affine)]
            assert {r for r, _, _ in c["runs"]} >= {2, 3, rpp + 1, 4 * rpp + 1} | ({rpp} if rpp > 1 else set())
            assert {s for _, _, s in c["runs"]} == set(U.BN_SLOPES)
    for name in ("pad-C8", "pad-C64", "pad-C256", "pad-C1024", "pad-C16-plain"):
        cap = cs[name]["runs"][0][0]
        assert [n for _, n, _ in cs[name]["runs"]] == [1, 2, cap - 1, cap, 0, cap + 7]


@pytest.mark.parametrize("cap,n,momentum", U.MASKED_BN_RUNS)
def test_masked_batch_norm_in_double_equals_the_reference(cap, n, momentum):
    """``ops.masked_batch_norm`` (plain tensor ops): two calls, so that ``momentum=None`` is seen to be the cumulative average
    (factors 1, then 1/2) and not a fixed 0.1; a count of 0 or above the capacity is clamped as the kernels clamp it."""
    from dualmessagepassing_amd import ops
    C = 50
    x, dy, gamma, beta, mean, var = [t[..., :C] for t in U.masked_bn_inputs(cap, n)]
    live = U.bn_live(cap, n)
    ref = U.bn_reference(x, dy, gamma, beta, mean, var, momentum, 1e-5, live, None)
    bn = _module_bn(C, True, momentum, gamma, beta, mean, var)
    xl = _leaf(x)
    rows_dev = th.tensor([n], dtype=th.int64)
    for _ in range(2):
        y = ops.masked_batch_norm(bn, xl, rows_dev)
    got = th.autograd.grad(y, [xl, bn.weight, bn.bias], dy.double())
    U.close(y, ref["y"], TOL, "y")
    assert not bool(y[live:].any()) and not bool(got[0][live:].any())
    U.close(bn.running_mean, ref["mean"], TOL, "running_mean")
    U.close(bn.running_var, ref["var"], TOL, "running_var")
    assert int(bn.num_batches_tracked) == 2
    for a, k in zip(got, ("dx", "dgamma", "dbeta")):
        U.close(a, ref[k], TOL, k)
