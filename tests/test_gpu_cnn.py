"""The CNN layer on the HIP kernels of csrc/dmp_cnn.hip against the tensor-op path (F.conv1d, max-pool, BatchNorm1d in the
reference's [B, H, L] layout), forward and every gradient; bitwise reproducibility; the full CNN model on the GPU against
the reference's fixtures; the fallback for uncovered shapes; a short training run."""
import os

import numpy as np
import pytest
import torch as th

from test_edgeseq_cnn_cpu import ES, _load, build_seeded, model_inputs, run_and_check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _layer(H, k, act="relu", bn=False, seed=0):
    from dualmessagepassing_amd.seqmodel import CNNLayer
    th.manual_seed(seed)
    layer = CNNLayer(H, H, kernel_size=k, batch_norm=bn, act_func=act)
    with th.no_grad():
        layer.conv.bias.uniform_(-0.2, 0.2)
    return layer.to(DEV)


def _inputs(B, L, H, lens, holes=(), seed=1):
    g = th.Generator().manual_seed(seed)
    x = th.randn(B, L, H, generator=g)
    gate = th.zeros(B, L)
    for b, n in enumerate(lens):
        if n:
            gate[b, L - n:] = 1.0
    for b, t in holes:
        gate[b, t] = 0.0
    return (x * gate.unsqueeze(-1)).to(DEV), gate.to(DEV)


def _run(layer, x, gate, residual, hip):
    from dualmessagepassing_amd import cnn
    x = x.clone().requires_grad_(True)
    for p in layer.parameters():
        p.grad = None
    if hip:
        assert cnn.hip_layer_ok(layer, x, gate)
        y, g = cnn.cnn_layer_hip(layer, x, gate, residual)
    else:
        o = layer(x.transpose(1, 2))
        g = layer.gate_next(gate.unsqueeze(1)).squeeze(1)
        y = (o * g.unsqueeze(1)).transpose(1, 2)
        if residual and y.size() == x.size():
            y = x + y
    w = th.randn(y.shape, generator=th.Generator().manual_seed(5)).to(DEV)
    (y * w).sum().backward()
    return y.detach(), g, x.grad, {k: p.grad.clone() for k, p in layer.named_parameters()}


def _close(a, b, tol, what):
    a, b = a.detach(), b.detach()
    scale = max(1.0, float(b.abs().max()))
    err = float((a.double() - b.double()).abs().max())
    assert err <= tol * scale, (what, err, scale)


@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_hip_layer_matches_tensor_ops(H, k):
    layer = _layer(H, k, act="relu" if k % 2 else "leaky_relu")
    x, gate = _inputs(5, 77, H, [77, 40, 0, 1, 70], holes=[(0, 10), (0, 11), (1, 50), (4, 20)])
    for residual in (True, False):
        y0, g0, dx0, dp0 = _run(layer, x, gate, residual, hip=False)
        y1, g1, dx1, dp1 = _run(layer, x, gate, residual, hip=True)
        assert th.equal(g0, g1)
        _close(y1, y0, 1e-5, "y")
        _close(dx1, dx0, 1e-4, "dx")
        for n in dp0:
            _close(dp1[n], dp0[n], 1e-4, n)


@pytest.mark.parametrize("bn", [False, True])
def test_batch_one_and_long_rows_and_batch_norm(bn):
    for B, L in ((1, 5), (3, 200)):
        layer = _layer(128, 2, bn=bn)
        x, gate = _inputs(B, L, 128, [L] + [L // 2] * (B - 1))
        y0, g0, dx0, dp0 = _run(layer, x, gate, True, hip=False)
        layer2 = _layer(128, 2, bn=bn)
        y1, g1, dx1, dp1 = _run(layer2, x, gate, True, hip=True)
        _close(y1, y0, 1e-4, "y")
        _close(dx1, dx0, 1e-4, "dx")
        for n in dp0:
            _close(dp1[n], dp0[n], 2e-4, n)
        if bn:
            _close(layer2.bn.running_mean, layer.bn.running_mean, 1e-5, "running_mean")
            _close(layer2.bn.running_var, layer.bn.running_var, 1e-5, "running_var")


def test_two_runs_are_bitwise_equal():
    layer = _layer(128, 3)
    x, gate = _inputs(16, 300, 128, [300, 120, 0] + [250] * 13)
    a = _run(layer, x, gate, True, hip=True)
    b = _run(layer, x, gate, True, hip=True)
    assert th.equal(a[0], b[0]) and th.equal(a[2], b[2])
    for n in a[3]:
        assert th.equal(a[3][n], b[3][n]), n


def test_uncovered_shapes_take_the_tensor_ops_and_match():
    from dualmessagepassing_amd import cnn
    for H, act in ((32, "relu"), (128, "tanh")):
        layer = _layer(H, 2, act=act)
        x, gate = _inputs(3, 20, H, [20, 5, 9])
        assert not cnn.hip_layer_ok(layer, x, gate)
        y, g = layer.forward_rows(x, gate, True)
        cpu = layer.to("cpu")
        yc, gc = cpu.forward_rows(x.cpu(), gate.cpu(), True)
        _close(y.cpu(), yc, 1e-5, "y")
        assert th.equal(g.cpu(), gc)


@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "e", "f"])
def test_cnn_model_on_the_gpu_matches_the_fixtures(tag):
    d = _load("model_" + tag)
    config, pattern, graph = model_inputs(d, DEV)
    model = build_seeded(d).to(DEV)
    run_and_check(d, model, pattern, graph, device=DEV, tol=2e-4, gtol=5e-4)


def test_cnn_model_takes_the_hip_path_at_width_128():
    from dualmessagepassing_amd import cnn
    from dualmessagepassing_amd.harness import SyntheticPairs
    ds = SyntheticPairs(8, 4, 5, 16, 40, 3, 2, seed=3)
    es = ds.edge_seq()
    model = __import__("dualmessagepassing_amd.basemodel", fromlist=["build_model"]).build_model(
        ds.model_config(hid_dim=128, rep_net="CNN", rep_cnn_batch_norm=False, pred_return_weights="edge")).to(DEV)
    pattern, graph, counts, (_, w) = es.batchify(np.arange(8), DEV, return_weights="edge")
    seen = []
    orig = cnn.cnn_layer_hip
    try:
        cnn.cnn_layer_hip = lambda *a: seen.append(1) or orig(*a)
        out = model(pattern, graph)
    finally:
        cnn.cnn_layer_hip = orig
    assert len(seen) == 3 * 2                                    # every layer, pattern and graph side
    assert out["pred_e"].shape == out["g_e_mask"].shape and w.shape == graph.u.shape


def test_fit_trains_a_cnn_on_synthetic_pairs():
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.harness import GraphedTrainStep, SmallLikePairs, train_epoch
    th.manual_seed(0)
    ds = SmallLikePairs(48, seed=7)
    es = ds.edge_seq()
    model = build_model(ds.model_config(hid_dim=64, rep_net="CNN", rep_cnn_batch_norm=False, pred_return_weights="edge")).to(DEV)
    opt = th.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for epoch in range(6):
        r = train_epoch(model, opt, es, 16, DEV, neg_slp=0.1, match_loss_w=0.1, match_reg_w=0.01, order=np.arange(len(es)))
        losses.append(r["bp_loss"])
    assert all(np.isfinite(losses)) and losses[0] > 0, losses
    assert losses[-1] < losses[0], losses
    with pytest.raises(ValueError, match="edge-sequence"):
        GraphedTrainStep(model, opt, None)
