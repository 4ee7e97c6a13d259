"""The RNN layer on the HIP kernels of csrc/dmp_rnn.hip against the layer's own nn.LSTM / nn.GRU / nn.RNN module, forward and
every gradient, for each cell, direction count and width of the path; bitwise reproducibility; the fallback for uncovered
shapes; the full RNN model on the GPU against the reference's fixtures; a short training run."""
import glob
import os

import numpy as np
import pytest
import torch as th

from test_edgeseq_cnn_cpu import build_seeded, model_inputs, run_and_check
from test_rnn_cpu import RN, _load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAGS = sorted(os.path.basename(p)[len("model_"):-4] for p in glob.glob(os.path.join(RN, "model_*.npz")))


def _layer(cell, hid, bi, seed=0):
    from dualmessagepassing_amd.seqmodel import RNNLayer
    th.manual_seed(seed)
    layer = RNNLayer(cell, hid, hid, bidirectional=bi)
    with th.no_grad():
        for k, p in layer.named_parameters():
            if "bias" in k:
                p.uniform_(-0.3, 0.3)
            else:
                p.mul_(1.5)
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
    from dualmessagepassing_amd import rnn
    x = x.clone().requires_grad_(True)
    for p in layer.parameters():
        p.grad = None
    if hip:
        assert rnn.hip_layer_ok(layer, x, gate)
        y = rnn.rnn_layer_hip(layer, x, gate, residual)
    else:
        y = layer(x) * gate.unsqueeze(-1)
        if residual and y.size() == x.size():
            y = x + y
    w = th.randn(y.shape, generator=th.Generator().manual_seed(5)).to(DEV)
    (y * w).sum().backward()
    return y.detach(), x.grad, {k: p.grad.clone() for k, p in layer.named_parameters()}


def _close(a, b, tol, what):
    a, b = a.detach(), b.detach()
    scale = max(1.0, float(b.abs().max()))
    err = float((a.double() - b.double()).abs().max())
    assert err <= tol * scale, (what, err, scale)


def _compare(layer, x, gate, residual, tol=1e-4, gtol=2e-4):
    y0, dx0, dp0 = _run(layer, x, gate, residual, hip=False)
    y1, dx1, dp1 = _run(layer, x, gate, residual, hip=True)
    _close(y1, y0, tol, "y")
    _close(dx1, dx0, gtol, "dx")
    assert sorted(dp0) == sorted(dp1)
    for n in dp0:
        _close(dp1[n], dp0[n], gtol, n)


@pytest.mark.parametrize("hd", [32, 64, 128])
@pytest.mark.parametrize("bi", [False, True], ids=["uni", "bi"])
@pytest.mark.parametrize("cell", ["LSTM", "GRU", "RNN"])
def test_hip_layer_matches_the_module(cell, bi, hd):
    hid = 2 * hd if bi else hd
    layer = _layer(cell, hid, bi)
    # B 7: not a multiple of the 4-sequence tile; pre-padding, holes and a row of length 0
    x, gate = _inputs(7, 61, hid, [61, 30, 0, 1, 58, 39, 5], holes=[(0, 10), (0, 11), (1, 50), (4, 20)])
    for residual in (True, False):
        _compare(layer, x, gate, residual)


@pytest.mark.parametrize("cell", ["LSTM", "GRU", "RNN"])
def test_length_one_and_long_rows(cell):
    for B, L, bi in ((3, 1, True), (5, 700, False), (2, 720, True)):
        layer = _layer(cell, 128, bi, seed=2)
        x, gate = _inputs(B, L, 128, [L] + [L // 3] * (B - 1), holes=[(0, 0)])
        _compare(layer, x, gate, True, tol=2e-4, gtol=5e-4)


def test_two_runs_are_bitwise_equal():
    for cell, bi in (("LSTM", True), ("GRU", False), ("RNN", True)):
        layer = _layer(cell, 128, bi)
        x, gate = _inputs(37, 300, 128, [300, 120, 0] + [250] * 34)
        a = _run(layer, x, gate, True, hip=True)
        b = _run(layer, x, gate, True, hip=True)
        assert th.equal(a[0], b[0]) and th.equal(a[1], b[1]), cell
        for n in a[2]:
            assert th.equal(a[2][n], b[2][n]), (cell, n)


def test_uncovered_shapes_take_the_module_path_and_match_the_cpu():
    from dualmessagepassing_amd import rnn
    from dualmessagepassing_amd.seqmodel import RNNLayer
    for cell, hid, bi, dtype in (("LSTM", 16, False, th.float32), ("RNN", 64, True, th.float64), ("GRU", 96, False, th.float32)):
        th.manual_seed(4)
        layer = RNNLayer(cell, hid, hid, bidirectional=bi).to(DEV, dtype)
        x, gate = _inputs(3, 20, hid, [20, 5, 9])
        x, gate = x.to(dtype), gate.to(dtype)
        assert not rnn.hip_layer_ok(layer, x, gate), cell
        y = layer.forward_rows(x, gate, True)
        yc = layer.to("cpu").forward_rows(x.cpu(), gate.cpu(), True)
        _close(y.cpu(), yc, 1e-5, cell)


def test_dropout_in_training_takes_the_module_path():
    from dualmessagepassing_amd import rnn
    from dualmessagepassing_amd.seqmodel import RNNLayer
    layer = RNNLayer("LSTM", 64, 64, dropout=0.5).to(DEV)
    x, gate = _inputs(3, 20, 64, [20, 5, 9])
    layer.train()
    assert not rnn.hip_layer_ok(layer, x, gate)
    layer.eval()
    assert rnn.hip_layer_ok(layer, x, gate)


@pytest.mark.parametrize("tag", TAGS)
def test_rnn_model_on_the_gpu_matches_the_fixtures(tag):
    d = _load("model_" + tag)
    config, pattern, graph = model_inputs(d, DEV)
    model = build_seeded(d).to(DEV)
    run_and_check(d, model, pattern, graph, device=DEV, tol=2e-4, gtol=5e-4)


@pytest.mark.parametrize("tag", ["lstm_bi_h64", "gru_uni_h64"])
def test_fixtures_at_width_64_go_through_the_hip_path(tag):
    from dualmessagepassing_amd import rnn
    d = _load("model_" + tag)
    config, pattern, graph = model_inputs(d, DEV)
    model = build_seeded(d).to(DEV)
    seen = []
    orig = rnn.rnn_layer_hip
    try:
        rnn.rnn_layer_hip = lambda *a: seen.append(1) or orig(*a)
        run_and_check(d, model, pattern, graph, device=DEV, tol=2e-4, gtol=5e-4)
    finally:
        rnn.rnn_layer_hip = orig
    assert len(seen) == 3 * 2


@pytest.mark.parametrize("cell", ["LSTM", "GRU"])
def test_rnn_model_takes_the_hip_path_at_width_128(cell):
    from dualmessagepassing_amd import rnn
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.harness import SyntheticPairs
    ds = SyntheticPairs(8, 4, 5, 16, 40, 3, 2, seed=3)
    es = ds.edge_seq()
    model = build_model(ds.model_config(hid_dim=128, rep_net="RNN", rep_rnn_type=cell, share_rep_net=False,
                                        pred_return_weights="edge")).to(DEV)
    pattern, graph, counts, (_, w) = es.batchify(np.arange(8), DEV, return_weights="edge")
    seen = []
    orig = rnn.rnn_layer_hip
    try:
        rnn.rnn_layer_hip = lambda *a: seen.append(1) or orig(*a)
        out = model(pattern, graph)
    finally:
        rnn.rnn_layer_hip = orig
    assert len(seen) == 3 * 2                                    # every layer, pattern and graph side
    assert out["pred_e"].shape == out["g_e_mask"].shape and w.shape == graph.u.shape


def test_fit_trains_an_lstm_on_small_like_pairs():
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.harness import GraphedTrainStep, SmallLikePairs, train_epoch
    th.manual_seed(0)
    ds = SmallLikePairs(48, seed=7)
    es = ds.edge_seq()
    model = build_model(ds.model_config(hid_dim=64, rep_net="RNN", rep_rnn_type="LSTM", pred_return_weights="edge")).to(DEV)
    opt = th.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for epoch in range(6):
        r = train_epoch(model, opt, es, 16, DEV, neg_slp=0.1, match_loss_w=0.1, match_reg_w=0.01, order=np.arange(len(es)))
        losses.append(r["bp_loss"])
    assert all(np.isfinite(losses)) and losses[0] > 0, losses
    assert losses[-1] < losses[0], losses
    with pytest.raises(ValueError, match="edge-sequence"):
        GraphedTrainStep(model, opt, None)
