"""The TXL rep-net on the GPU: the full model with the kernels of csrc/dmp_txl.hip under its attention against the
reference's fixtures (outputs 1e-4, gradients 2e-4, the figures of the attention and RNN GPU tests), the folded batch of the
empty-memory regime against the segment loop, and bitwise reproducibility of the kernels."""
import glob
import os

import pytest
import torch as th

from test_edgeseq_cnn_cpu import build_seeded, model_inputs, run_and_check
from test_txl_cpu import TX, _load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAGS = sorted(os.path.basename(p)[len("model_"):-4] for p in glob.glob(os.path.join(TX, "model_*.npz")))
# head widths 16 and 64 (hid 16 with one head, hid 64 with one or four heads): the kernels; 4 and 8: the tensor ops
KERNEL_TAGS = {"default", "default_h64", "seg8_h64", "clamp"}


def _count_kernel_calls(monkeypatch):
    from dualmessagepassing_amd import txl
    calls = []
    real = txl.RelAttention.apply

    def spy(*a):
        calls.append(tuple(a[0].shape) + (a[1].size(1),))
        return real(*a)
    monkeypatch.setattr(txl.RelAttention, "apply", spy)
    return calls


@pytest.mark.parametrize("tag", TAGS)
def test_txl_model_on_the_gpu_matches_the_reference(tag, monkeypatch):
    d = _load("model_" + tag)
    calls = _count_kernel_calls(monkeypatch)
    config, pattern, graph = model_inputs(d, DEV)
    model = build_seeded(d)
    run_and_check(d, model, pattern, graph, device=DEV, tol=1e-4, gtol=2e-4)
    assert bool(calls) == (tag in KERNEL_TAGS), (tag, calls)
    if tag == "default_h64":            # the driver's shape with a full memory: q 64, k 128, one head of 64
        assert (4, 64, 1, 64, 128) in calls and (4, 64, 1, 64, 64) in calls
    if tag == "seg8_h64":               # every segment of every sequence in one launch per layer
        S = -(-graph.u.size(1) // 8)
        assert (4 * S, 8, 4, 16, 8) in calls


def test_folded_batch_equals_the_segment_loop_on_the_kernels(monkeypatch):
    """Empty memory: the segments are independent.  The attention kernels treat a sequence the same wherever it sits in the
    batch; the GEMMs around them may block the rows differently, hence 1e-6 of the scale and not bit for bit."""
    d = _load("model_seg8_h64")
    config, pattern, graph = model_inputs(d, DEV)
    res = []
    for fold in (True, False):
        calls = _count_kernel_calls(monkeypatch)
        model = build_seeded(d)
        model.fold_segments = fold
        out = run_and_check(d, model, pattern, graph, device=DEV, tol=1e-4, gtol=2e-4)
        res.append((out["g_e_rep"].detach(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}, len(calls)))
        monkeypatch.undo()
    (a, ga, na), (b, gb, nb) = res
    assert na < nb                       # one launch per layer against one per layer and segment
    assert float((a - b).abs().max()) <= 1e-6 * max(1.0, float(b.abs().max()))
    for k in gb:
        assert float((ga[k] - gb[k]).abs().max()) <= 1e-6 * max(1.0, float(gb[k].abs().max())), k


@pytest.mark.parametrize("N,q,k,nh,dh", [(300, 8, 16, 1, 16), (130, 5, 7, 4, 32), (3, 64, 128, 2, 64), (70, 37, 101, 4, 32)])
def test_two_runs_are_bitwise_equal(N, q, k, nh, dh):
    """More sequences than backward workgroups per head (256 / heads), so a workgroup adds several sequences into its partial;
    the last shape does so at ragged sizes, where a tile's padding still holds the sequence before."""
    from dualmessagepassing_amd import txl
    g = th.Generator().manual_seed(7)
    args = [th.randn(N, q, nh, dh, generator=g), th.randn(N, k, nh, dh, generator=g), th.randn(N, k, nh, dh, generator=g),
            th.randn(k, nh, dh, generator=g), 0.5 * th.randn(nh, dh, generator=g), 0.5 * th.randn(nh, dh, generator=g)]
    w = th.randn(N, q, nh * dh, generator=g).to(DEV)
    runs = []
    for _ in range(2):
        xs = [a.to(DEV).requires_grad_(True) for a in args]
        assert txl.kernel_ok(*xs)
        o = txl.rel_attention(*xs, dh ** -0.5)
        (o * w).sum().backward()
        runs.append([o.detach()] + [x.grad for x in xs])
    for a, b in zip(*runs):
        assert th.equal(a, b)


def test_unsupported_shapes_take_the_tensor_ops():
    from dualmessagepassing_amd import txl
    lib_ok = lambda q, k, dh: txl.kernel_ok(th.zeros(1, q, 1, dh, device=DEV), th.zeros(1, k, 1, dh, device=DEV), th.zeros(1, k, 1, dh, device=DEV),
                                            th.zeros(k, 1, dh, device=DEV), th.zeros(1, dh, device=DEV), th.zeros(1, dh, device=DEV))
    assert lib_ok(64, 128, 128) and lib_ok(1, 1, 16) and lib_ok(5, 7, 64) and lib_ok(64, 64, 32)
    assert not lib_ok(65, 65, 16) and not lib_ok(64, 129, 16) and not lib_ok(8, 8, 8) and not lib_ok(8, 7, 16) and not lib_ok(8, 8, 48)
    drop = th.nn.Dropout(0.5)
    q = th.randn(2, 4, 1, 16, device=DEV)
    r, b = th.randn(4, 1, 16, device=DEV), th.randn(1, 16, device=DEV)
    th.manual_seed(0)
    a = txl.rel_attention(q, q, q, r, b, b, 0.25, drop)          # training-mode dropout: the tensor ops
    th.manual_seed(0)
    assert th.equal(a, txl.rel_attention_tensor(q, q, q, r, b, b, 0.25, drop))
    drop.eval()
    assert th.equal(txl.rel_attention(q, q, q, r, b, b, 0.25, drop), txl.RelAttention.apply(q, q, q, r, b, b, 0.25))
