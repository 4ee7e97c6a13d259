"""The RNN layer's kernels (csrc/dmp_rnn.hip) against the explicit float64 time loop of ``util_fp64.rnn_layer_fp64``: LSTM / GRU
/ RNN, one and two directions, Hd 32 / 64 / 128; an input width that differs from the output width (narrower, wider, odd);
no gate; B = 1, a full 4-sequence tile, two tiles, 4n + 1 with both directions; L = 1 and 2; a row whose gate is all zero;
holes at the first and the last position; rows of 700 positions; saturated gates.  Output, dx and every parameter gradient.

Tolerances are those of ``test_gpu_rnn.py`` for short rows: y 1e-4, gradients 2e-4.  For the cases whose error grows with a
size nobody had measured against fp64 (L = 700, pre-activations around 15) the layer's own nn.LSTM / nn.GRU / nn.RNN runs in
fp32 on the GPU beside the kernels, and the kernels pass within those figures or within four times the module's own distance
from fp64; both distances are printed (DESIGN.md section 5 has the table)."""
import pytest
import torch as th

import util_fp64 as U

pytestmark = pytest.mark.gpu


def _leaf(t):
    return t.detach().cpu().double().clone().requires_grad_(True)


def _run(layer, x, gate, residual, w, gpu, hip):
    """(y, dx, parameter gradients by name) of the layer on the GPU: through ``forward_rows`` (the kernels), or the torch
    module in fp32."""
    layer.zero_grad(set_to_none=True)
    xg = x.to(gpu).requires_grad_(True)
    gg = None if gate is None else gate.to(gpu)
    if hip:
        y = layer.forward_rows(xg, gg, residual)
    else:
        y = layer(xg)
        if gg is not None:
            y = y * gg.unsqueeze(-1)
        if residual and y.size() == xg.size():
            y = xg + y
    (y * w.to(gpu)).sum().backward()
    return y.detach(), xg.grad, {n: p.grad.clone() for n, p in layer.layer.named_parameters()}


@pytest.mark.parametrize("case", sorted(U.rnn_cases()))
def test_layer_matches_the_fp64_time_loop(case, gpu, monkeypatch):
    from dualmessagepassing_amd import rnn
    c = U.rnn_cases()[case]
    layer = U.rnn_make_layer(c).to(gpu)
    x, gate = U.rnn_inputs(c)
    names = U.rnn_param_names(c["bi"])
    params = [_leaf(getattr(layer.layer, n)) for n in names]
    xd = _leaf(x)
    y0 = U.rnn_layer_fp64(c["cell"], params, xd, None if gate is None else gate.double(), c["residual"])
    w = th.randn(y0.shape, generator=th.Generator().manual_seed(5))
    (y0 * w.double()).sum().backward()

    calls = []
    real = rnn.rnn_layer_hip
    monkeypatch.setattr(rnn, "rnn_layer_hip", lambda *a: (calls.append(1), real(*a))[1])
    assert rnn.hip_layer_ok(layer, x.to(gpu), None if gate is None else gate.to(gpu))
    y1, dx1, dp1 = _run(layer, x, gate, c["residual"], w, gpu, hip=True)
    assert len(calls) == 1, "the HIP path was not taken"
    assert sorted(dp1) == sorted(names)
    if c["din"] is not None:
        assert x.size(2) != y1.size(2) and dx1.shape == x.shape
    if not c["band"]:
        U.close(y1, y0, 1e-4, "y")
        U.close(dx1, xd.grad, 2e-4, "dx")
        for n, p in zip(names, params):
            U.close(dp1[n], p.grad, 2e-4, n)
        return
    y2, dx2, dp2 = _run(layer, x, gate, c["residual"], w, gpu, hip=False)
    assert len(calls) == 1
    U.within_band(y1, y0, y2, 1e-4, "rnn %s y" % case)
    U.within_band(dx1, xd.grad, dx2, 2e-4, "rnn %s dx" % case)
    rows = []
    for n, p in zip(names, params):
        assert bool(th.isfinite(dp1[n]).all()), n
        err, scale = U.dist(dp1[n], p.grad)
        yerr, _ = U.dist(dp2[n], p.grad)
        rows.append((err / scale, yerr / scale, scale, n))
        assert err <= max(2e-4 * scale, 4.0 * yerr), "%s: %g against fp64, the module %g (scale %g)" % (n, err, yerr, scale)
    print("FP64BAND rnn %s worst-grad(%s) kernel %.3g yardstick %.3g (x scale %.3g)" % ((case, max(rows)[3]) + max(rows)[:3]))


def test_two_runs_at_unequal_widths_are_bitwise_equal(gpu):
    c = U.rnn_cases()["GRU-bi-in50"]
    layer = U.rnn_make_layer(c).to(gpu)
    x, gate = U.rnn_inputs(c)
    w = th.randn(c["B"], c["L"], 64, generator=th.Generator().manual_seed(5))
    a = _run(layer, x, gate, True, w, gpu, hip=True)
    b = _run(layer, x, gate, True, w, gpu, hip=True)
    assert th.equal(a[0], b[0]) and th.equal(a[1], b[1])
    for n in a[2]:
        assert th.equal(a[2][n], b[2][n]), n
