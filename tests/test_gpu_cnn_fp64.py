"""The CNN layer's kernels (csrc/dmp_cnn.hip) against the float64 restatement of ``util_fp64.cnn_layer_fp64`` over everything
``cnn.hip_layer_ok`` admits: all 24 (k, pad) geometries at both widths with relu and leaky_relu, the residual on and off, a
gate with pre-padding, holes and an empty row and no gate, lengths that put L' on the edges of the forward's 64-row tiles
(TP - 1, TP, TP + 1, 2 TP, 2 TP + 1 with TP = 65 - k), the smallest admitted length, L < k, B = 1; with BatchNorm in both
modes; and, through the C entry points, the calling modes the layer cannot reach (pool kernels below k, pool padding 0 under a
padded conv, the plain conv of the backward at every padding, no arg, a residual), the routing kernel and the split-K weight
gradient alone, and the host-side refusals.

The forward is compared on all outputs.  Gradients are taken with the upstream weight multiplied by the reference's safe mask
on both sides (outputs whose pool winner or activation sign sits within 1e-4 of a tie feed no gradient anywhere); the CPU
module ``test_fp64_refs_cpu.py`` asserts that at most 0.1 % of a case's outputs are unsafe.  Tolerances are those of
``test_gpu_cnn.py``: y 1e-5, gradients 1e-4; the gate after the layer and the arg byte on safe outputs are exact."""
import pytest
import torch as th

import util_fp64 as U

pytestmark = pytest.mark.gpu
BAD_ARG = -1


def _leaf(t):
    return t.detach().cpu().double().clone().requires_grad_(True)


def _spy(monkeypatch):
    from dualmessagepassing_amd import cnn
    calls = []
    real = cnn.cnn_layer_hip
    monkeypatch.setattr(cnn, "cnn_layer_hip", lambda *a: (calls.append(1), real(*a))[1])
    return calls


def _reference(layer, x, gate, residual, w, post=None):
    c, p = layer.conv, layer.pool
    W, b, xd = _leaf(c.weight), _leaf(c.bias), _leaf(x)
    y, g, safe, _ = U.cnn_layer_fp64(W, b, xd, gate, c.kernel_size[0], c.padding[0], p.kernel_size, p.padding,
                                     U.cnn_slope(layer.act_func), residual, post=post)
    (y * w.double() * safe).sum().backward()
    return y.detach(), g, safe, xd.grad, W.grad, b.grad


def _product(layer, x, gate, residual, w, safe, gpu):
    from dualmessagepassing_amd import cnn
    layer.zero_grad(set_to_none=True)
    xg = x.to(gpu).requires_grad_(True)
    gg = None if gate is None else gate.to(gpu)
    assert cnn.hip_layer_ok(layer, xg, gg)
    y, g = layer.forward_rows(xg, gg, residual)
    (y * (w * safe).to(gpu)).sum().backward()
    return y.detach(), g, xg.grad, layer.conv.weight.grad, layer.conv.bias.grad


@pytest.mark.parametrize("case", sorted(U.cnn_layer_cases()))
def test_layer_matches_fp64_at_every_admitted_geometry(case, gpu, monkeypatch):
    H, k, pad, act = U.cnn_layer_cases()[case]
    calls = _spy(monkeypatch)
    layer = U.cnn_make_layer(H, k, pad, act)
    dev = U.cnn_make_layer(H, k, pad, act).to(gpu)
    runs = U.cnn_layer_runs(k, pad)
    for n, (B, L, gated, residual) in enumerate(runs):
        x, gate = U.cnn_inputs(B, L, H, gated, U.stable_seed(case) + n)
        w = th.randn(B, L + 4 * pad - 2 * k + 2, H, generator=th.Generator().manual_seed(5 + n))
        y0, g0, safe, dx0, dW0, db0 = _reference(layer, x, gate, residual, w)
        y1, g1, dx1, dW1, db1 = _product(dev, x, gate, residual, w, safe, gpu)
        what = "%s B%d L%d gate%d res%d " % (case, B, L, gated, residual)
        U.close(y1, y0, 1e-5, what + "y")
        assert (g0 is None) == (g1 is None) and (g0 is None or th.equal(g1.cpu().double(), g0)), what + "gate"
        U.close(dx1, dx0, 1e-4, what + "dx")
        U.close(dW1, dW0, 1e-4, what + "dW")
        U.close(db1, db0, 1e-4, what + "db")
    assert len(calls) == len(runs), "the HIP path was not taken"


@pytest.mark.parametrize("case", sorted(U.cnn_bn_cases()))
def test_layer_with_batch_norm_matches_fp64(case, gpu, monkeypatch):
    H, k, pad, act, training, momentum, B, L = U.cnn_bn_cases()[case]
    calls = _spy(monkeypatch)
    layer = U.cnn_make_layer(H, k, pad, act, bn=True, momentum=momentum).train(training)
    dev = U.cnn_make_layer(H, k, pad, act, bn=True, momentum=momentum).train(training).to(gpu)
    bn = layer.bn
    x, gate = U.cnn_bn_inputs(case, layer)
    w = th.randn(B, L + 4 * pad - 2 * k + 2, H, generator=th.Generator().manual_seed(5))
    gamma, beta, stats = _leaf(bn.weight), _leaf(bn.bias), {}

    def post(p):
        o, stats["mean"], stats["var"] = U.batch_norm_fp64(p, gamma, beta, bn.running_mean.double(), bn.running_var.double(),
                                                           training, momentum, bn.eps, int(bn.num_batches_tracked))
        return o

    y0, g0, safe, dx0, dW0, db0 = _reference(layer, x, gate, True, w, post=post)
    assert bool(safe.all()) or not training
    y1, g1, dx1, dW1, db1 = _product(dev, x, gate, True, w, safe, gpu)
    assert len(calls) == 1, "the HIP path was not taken"
    U.close(y1, y0, 1e-5, "y")
    assert th.equal(g1.cpu().double(), g0)
    for a, b, n in ((dx1, dx0, "dx"), (dW1, dW0, "dW"), (db1, db0, "db"), (dev.bn.weight.grad, gamma.grad, "dgamma"),
                    (dev.bn.bias.grad, beta.grad, "dbeta")):
        U.close(a, b, 1e-4, n)
    U.close(dev.bn.running_mean, stats["mean"], 1e-5, "running_mean")
    U.close(dev.bn.running_var, stats["var"], 1e-5, "running_var")
    assert int(dev.bn.num_batches_tracked) == int(training)


# ------------------------------------------------------------------------------------------------- through the C entry points

def _lib():
    from dualmessagepassing_amd import _lib as L
    return L, L.load()


def _weights(H, k, seed):
    g = th.Generator().manual_seed(seed)
    W = th.randn(H, H, k, generator=g) / (H * k) ** 0.5
    b = th.rand(H, generator=g) * 0.4 - 0.2
    return W, b


def _fwd(gpu, x, W, bias, k, pad, pk, pp, act, slope, gate, apply_gate, resid, want_arg):
    """dmp_cnn_fwd on the device copies: (code, y, arg or None, gate_out or None)."""
    L, lib = _lib()
    B, Ln, H = x.shape
    Lout = Ln + 2 * pad - k + 1 + 2 * pp - pk + 1
    xg = x.to(gpu).contiguous()
    wt = W.permute(2, 1, 0).contiguous().to(gpu)
    bg = None if bias is None else bias.to(gpu)
    gg = None if gate is None else gate.to(gpu).contiguous()
    rg = None if resid is None else resid.to(gpu).contiguous()
    y = th.full((B, max(Lout, 1), H), float("nan"), device=gpu)
    arg = th.zeros((B, max(Lout, 1), H), dtype=th.uint8, device=gpu) if want_arg else None
    go = th.full((B, max(Lout, 1)), float("nan"), device=gpu) if gate is not None else None
    code = lib.dmp_cnn_fwd(xg.data_ptr(), B, Ln, H, wt.data_ptr(), L.ptr(bg), k, pad, pk, pp, act, float(slope), L.ptr(gg),
                           int(apply_gate), L.ptr(rg), y.data_ptr(), L.ptr(arg), L.ptr(go), L.stream_ptr())
    th.cuda.synchronize()
    return code, y, arg, go


POOL_MODES = [  # (H, k, pad, pk, pp, slope, B, L, apply_gate, resid): pool kernels below k, pool padding 0 under a padded conv
    (64, 5, 2, 2, 0, 0.0, 3, 70, 1, False), (128, 8, 3, 3, 1, 1.0 / 5.5, 2, 131, 1, True), (64, 4, 1, 1, 0, 0.0, 3, 66, 0, True),
    (128, 3, 2, 3, 0, 1.0 / 5.5, 3, 62, 1, False), (64, 8, 7, 4, 2, 0.0, 1, 9, 1, True), (128, 6, 5, 6, 0, 0.0, 3, 59, 0, False),
    (64, 7, 0, 2, 1, 1.0 / 5.5, 3, 71, 1, True), (128, 2, 1, 1, 0, 0.0, 2, 64, 1, False)]


@pytest.mark.parametrize("mode", POOL_MODES, ids=lambda m: "H%d-k%d-p%d-pk%d-pp%d" % m[:5])
def test_entry_point_pool_modes_match_fp64_and_the_arg_byte_is_exact(mode, gpu):
    H, k, pad, pk, pp, slope, B, Ln, apply_gate, with_resid = mode
    W, b = _weights(H, k, 11)
    x, gate = U.cnn_inputs(B, Ln, H, True, 100 + k)
    Lout = Ln + 2 * pad - k + 1 + 2 * pp - pk + 1
    resid = th.randn(B, Lout, H, generator=th.Generator().manual_seed(3)) if with_resid else None
    y0, g0, safe, arg0 = U.cnn_layer_fp64(W.double(), b.double(), x.double(), gate, k, pad, pk, pp, slope, False,
                                          apply_gate=bool(apply_gate))
    if resid is not None:
        y0 = y0 + resid.double()
    code, y, arg, go = _fwd(gpu, x, W, b, k, pad, pk, pp, 1, slope, gate, apply_gate, resid, True)
    assert code == 0
    U.close(y, y0, 1e-5, "y")
    assert th.equal(go.cpu().double(), g0)
    assert int((~safe).sum()) <= U.UNSAFE_CAP * safe.numel()
    assert th.equal(arg.cpu().to(th.int64)[safe], arg0[safe])
    # the same launch without an arg buffer and without a gate
    code, y2, _, _ = _fwd(gpu, x, W, b, k, pad, pk, pp, 1, slope, None, 0, resid, False)
    assert code == 0
    ref2 = U.cnn_layer_fp64(W.double(), b.double(), x.double(), None, k, pad, pk, pp, slope, False)[0]
    U.close(y2, ref2 + (0 if resid is None else resid.double()), 1e-5, "y without arg")


@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("k", range(1, 9))
def test_entry_point_plain_conv_at_every_padding(k, H, gpu):
    """act 0, pk 1: the calling mode of the backward's dX, paddings 0 .. k - 1, with and without bias and residual."""
    W, b = _weights(H, k, 20 + k)
    for pad in range(k):
        B, Ln = (1, 67) if pad % 2 else (3, 64 + k)
        x = th.randn(B, Ln, H, generator=th.Generator().manual_seed(pad))
        Lout = Ln + 2 * pad - k + 1
        bias = b if pad % 3 == 0 else None
        resid = th.randn(B, Lout, H, generator=th.Generator().manual_seed(4)) if pad % 2 == 0 else None
        y0 = U.cnn_layer_fp64(W.double(), None if bias is None else bias.double(), x.double(), None, k, pad, 1, 0, 0.0, False,
                              act=False)[0]
        if resid is not None:
            y0 = y0 + resid.double()
        code, y, _, _ = _fwd(gpu, x, W, bias, k, pad, 1, 0, 0, 0.0, None, 0, resid, False)
        assert code == 0
        U.close(y, y0, 1e-5, "k%d pad%d" % (k, pad))


@pytest.mark.parametrize("geo", [(64, 1, 0, 0.0), (128, 3, 1, 1.0 / 5.5), (64, 5, 2, 0.0), (128, 8, 4, 1.0 / 5.5), (64, 4, 0, 0.5),
                                 (20, 6, 3, 0.0)], ids=lambda g: "H%d-pk%d-pp%d" % g[:3])
def test_route_bwd_alone_against_a_scatter_of_the_arg_bytes(geo, gpu):
    """dC[b, t - pp + q, c] += dY[b, t, c] gate[b, t] (1 if the byte's sign bit is set, else slope), q the byte's offset."""
    H, pk, pp, slope = geo
    L, lib = _lib()
    B, Lc = 3, 77
    Lout = Lc + 2 * pp - pk + 1
    g = th.Generator().manual_seed(pk * 10 + pp)
    t = th.arange(Lout).view(1, Lout, 1)
    lo, hi = (pp - t).clamp(min=0), (Lc - 1 - t + pp).clamp(max=pk - 1)
    q = lo + (th.rand(B, Lout, H, generator=g) * (hi - lo + 1)).floor().to(th.int64).clamp(max=pk - 1)
    q = th.minimum(q, hi.expand_as(q))
    pos = th.rand(B, Lout, H, generator=g) < 0.6
    arg = (q + 128 * pos.to(th.int64)).to(th.uint8)
    dY = th.randn(B, Lout, H, generator=g)
    gate = (th.rand(B, Lout, generator=g) < 0.8).float()
    for use_gate in (True, False):
        v = dY.double() * th.where(pos, 1.0, slope) * (gate.double().unsqueeze(-1) if use_gate else 1.0)
        ref = th.zeros(B, Lc, H, dtype=th.float64).scatter_add(1, t - pp + q, v)
        dYg, argg, gg = dY.to(gpu), arg.to(gpu), gate.to(gpu)
        dC = th.full((B, Lc, H), float("nan"), device=gpu)
        code = lib.dmp_cnn_route_bwd(dYg.data_ptr(), gg.data_ptr() if use_gate else None, argg.data_ptr(), B, Lc, Lout, H, pk, pp,
                                     float(slope), dC.data_ptr(), L.stream_ptr())
        th.cuda.synchronize()
        assert code == 0
        U.close(dC, ref, 1e-4, "dC gate%d" % use_gate)


WGRAD = [  # (H, k, pad, B, Lc, band): B Lc = 1, 1023, 1024, 1025 rows (one chunk is 1024), and several chunks
    (64, 3, 1, 1, 1, False), (128, 2, 1, 1, 1023, False), (64, 8, 3, 2, 512, False), (128, 5, 0, 5, 205, False),
    (64, 1, 0, 1, 1025, False), (128, 8, 7, 3, 1400, True), (64, 4, 2, 7, 600, True)]


@pytest.mark.parametrize("shape", WGRAD, ids=lambda s: "H%d-k%d-p%d-B%d-Lc%d" % s[:5])
def test_wgrad_and_reduce_alone_against_fp64(shape, gpu):
    H, k, pad, B, Lc, band = shape
    L, lib = _lib()
    Ln = Lc - 2 * pad + k - 1
    assert Ln >= 1
    g = th.Generator().manual_seed(H + k + Lc)
    dC, x = th.randn(B, Lc, H, generator=g), th.randn(B, Ln, H, generator=g)

    def grads(dc, xx):                       # dW[j][o][i] = sum_{b, s} dC[b, s, o] x[b, s - pad + j, i], x zero outside [0, L)
        xp = th.nn.functional.pad(xx, (0, 0, pad, pad))
        return th.stack([th.einsum("bso,bsi->oi", dc, xp[:, j:j + Lc]) for j in range(k)]), dc.sum((0, 1))

    dW0, db0 = grads(dC.double(), x.double())
    dCg, xg = dC.to(gpu), x.to(gpu)
    chunks = int(lib.dmp_cnn_wgrad_chunks(B * Lc))
    assert chunks == (B * Lc + 1023) // 1024
    width = k * H * H + H
    part = th.full((chunks, width), float("nan"), device=gpu)
    red = th.full((width,), float("nan"), device=gpu)
    assert lib.dmp_cnn_wgrad(dCg.data_ptr(), xg.data_ptr(), B, Ln, Lc, H, k, pad, part.data_ptr(), L.stream_ptr()) == 0
    assert lib.dmp_reduce_partials(part.data_ptr(), chunks, width, red.data_ptr(), 0, L.stream_ptr()) == 0
    th.cuda.synchronize()
    dW, db = red[:k * H * H].view(k, H, H), red[k * H * H:]
    if band:
        prev = th.backends.cuda.matmul.allow_tf32
        th.backends.cuda.matmul.allow_tf32 = False
        try:
            dWy, dby = grads(dCg, xg)
        finally:
            th.backends.cuda.matmul.allow_tf32 = prev
        U.within_band(dW, dW0, dWy, 1e-4, "cnn-wgrad H%d k%d rows %d dW" % (H, k, B * Lc))
        U.within_band(db, db0, dby, 1e-4, "cnn-wgrad H%d k%d rows %d db" % (H, k, B * Lc))
    else:
        U.close(dW, dW0, 1e-4, "dW")
        U.close(db, db0, 1e-4, "db")


@pytest.mark.parametrize("bad", [dict(pad=3, k=3), dict(pad=5, k=3), dict(pp=2, pk=3), dict(H=96), dict(L=2, k=5, pad=0, pk=1, pp=0),
                                 dict(L=4, k=4, pad=0, pk=4, pp=1), dict(k=9, pad=0), dict(pk=4, k=3, pad=1)],
                         ids=["pad=k", "pad>k", "2pp>pk", "H96", "Lc<1", "Lout<1", "k>8", "pk>k"])
def test_host_side_refusals_return_bad_arg(bad, gpu):
    """Refused on the host before any launch: the output buffer keeps its fill."""
    a = dict(H=64, L=40, k=3, pad=1, pk=3, pp=1)
    a.update(bad)
    L, lib = _lib()
    x = th.zeros(2, a["L"], a["H"], device=gpu)
    wt = th.zeros(9, a["H"], a["H"], device=gpu)
    y = th.full((2, 64, a["H"]), 7.0, device=gpu)
    code = lib.dmp_cnn_fwd(x.data_ptr(), 2, a["L"], a["H"], wt.data_ptr(), None, a["k"], a["pad"], a["pk"], a["pp"], 1, 0.0, None, 0,
                           None, y.data_ptr(), None, None, L.stream_ptr())
    th.cuda.synchronize()
    assert code == BAD_ARG
    assert bool((y == 7.0).all())
