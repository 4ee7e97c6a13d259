"""CompGCN on the kernels (``unc_compgcn``): ``dmp_relcorr_weights_fwd`` / ``_bwd`` against the fp64 restatement with explicit
circulants (tests/util_fp64_compgcn.py) over ``FORMER_SHAPES`` -- the smallest and the largest admitted size; I != H, I no
power of two with padding columns; each of the three routes of the dT gradient (one, two or four column groups: H <= 64,
H <= 128, above) with full and with partial last groups; one and several column tiles with a partial last one (H 65, 129,
130, 200); I no multiple of 8 at H > 64; I far below and far above H at R = 16 -- bitwise repeatable, and a refused shape that
must fall back; every reference fixture on the kernel path; the kernel
path against the tensor-op path of the same module on a 2,000-node graph with edge types outside the table; replayed
training against the eager loop.

The kernel's bound is not fitted to the kernel: the fp32 tensor-op former's distance from fp64 is measured on the CPU for the
same inputs, and the kernel may be 4 times as far, or SURVEY section 8(c)'s 1e-5 max(1, |ref|max), whichever is larger."""
import copy

import numpy as np
import pytest
import torch as th

pytestmark = pytest.mark.gpu


def _spy(monkeypatch):
    from dualmessagepassing_amd import unc_compgcn
    calls = []
    real = unc_compgcn._RelCorrWeights.apply
    monkeypatch.setattr(unc_compgcn._RelCorrWeights, "apply", lambda *a: (calls.append(1), real(*a))[1])
    return calls


def _spy_agg(monkeypatch):
    """Calls of the typed sum's kernel path, ``unc_rel._RelAgg`` as ``unc_compgcn`` reaches it."""
    from dualmessagepassing_amd import unc_compgcn
    calls = []
    real = unc_compgcn._RelAgg.apply
    monkeypatch.setattr(unc_compgcn._RelAgg, "apply", lambda *a: (calls.append(1), real(*a))[1])
    return calls


def _close(a, b, tol, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = max(1.0, float(b.abs().max())) if b.numel() else 1.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    assert err <= tol * scale, "%s: %g (scale %g)" % (what, err, scale)


def _former_case(I, H, R, gpu, calls, repeatable=True):
    """Kernel (or fallback) and fp32 CPU tensor ops against fp64: prints every distance, then asserts the rule above."""
    from dualmessagepassing_amd.unc_compgcn import LOOP_SCALE, corr_weights, corr_weights_tensor_ops
    from dualmessagepassing_amd.unc_rel import padded_width
    from util_fp64_compgcn import relcorr_weights_bwd_fp64, relcorr_weights_fp64
    gen = th.Generator().manual_seed(1000 * I + 10 * H + R)
    P = padded_width(H)
    shapes = ((R, I), (1, I), (I, H), (I, H))
    host = [th.randn(*s, generator=gen) * (1.0 if k < 2 else I ** -0.5) for k, s in enumerate(shapes)]
    d = th.randn(I, (R + 1) * P, generator=gen)
    np64 = [x.double().numpy() for x in host]
    want = [relcorr_weights_fp64(*np64, P, LOOP_SCALE)] + list(relcorr_weights_bwd_fp64(d.double().numpy(), *np64, P, LOOP_SCALE))

    def run(device, fn):
        leaves = [x.clone().to(device).requires_grad_(True) for x in host]
        out = fn(*leaves, P, LOOP_SCALE)
        out.backward(d.to(device))
        return [out.detach()] + [x.grad for x in leaves]

    cpu = run("cpu", corr_weights_tensor_ops)
    got = run(gpu, corr_weights)
    again = run(gpu, corr_weights)
    names = ("Wcat", "dT", "dloop_rel", "dWin", "dWloop")
    fails = []
    for name, g, c, w, g2 in zip(names, got, cpu, want, again):
        w = th.from_numpy(np.asarray(w)).reshape(g.shape)
        e_cpu = float((c.double() - w).abs().max())
        e_gpu = float((g.cpu().double() - w).abs().max())
        bound = max(4 * e_cpu, 1e-5 * max(1.0, float(w.abs().max())))
        print("relcorr (I %d, H %d, R %d) %-9s |ref|max %.3g  fp32 tensor ops %.3g  gpu %.3g  bound %.3g  kernel calls %d"
              % (I, H, R, name, float(w.abs().max()), e_cpu, e_gpu, bound, len(calls)))
        if not e_gpu <= bound:
            fails.append((name, e_gpu, bound))
        assert not repeatable or th.equal(g, g2), name + " differs between two launches"
    assert not fails, fails
    Wv = got[0].view(I, R + 1, P)
    if P != H:
        assert float(Wv[:, :, H:].abs().max()) == 0.0          # the padding columns: exactly zero
    return got


FORMER_SHAPES = [
    (4, 4, 1), (12, 8, 2), (50, 50, 2), (64, 64, 8), (256, 256, 16),
    # dT over two column groups (64 < H <= 128), each taking half of the rows
    (40, 100, 3), (100, 72, 2), (13, 128, 1),
    (72, 65, 4),             # P = 68: the second column tile has one live column
    (5, 64, 1),              # the widest H on the one-group route, I below a lane's 8 rows
    # dT over four column groups with a partial last one; more than one column tile, the last one partial; I % 8 != 0
    (64, 129, 1), (30, 130, 2), (255, 200, 3),
    (9, 255, 16),            # I << H at the largest R
    (256, 5, 16),            # I >> H: the largest backward LDS at a narrow width
]


@pytest.mark.parametrize("I,H,R", FORMER_SHAPES)
def test_relcorr_weights_match_fp64_and_are_repeatable(I, H, R, gpu, monkeypatch):
    from dualmessagepassing_amd import _lib
    calls = _spy(monkeypatch)
    assert _lib.load().dmp_relcorr_supported(I, H, R + 1) == 1
    _former_case(I, H, R, gpu, calls)
    assert len(calls) == 2, "the HIP path was not taken"


@pytest.mark.parametrize("I,H,R", [(260, 8, 2), (8, 8, 17), (3, 8, 2)])
def test_a_refused_shape_falls_back_and_still_agrees(I, H, R, gpu, monkeypatch):
    from dualmessagepassing_amd import _lib
    calls = _spy(monkeypatch)
    assert _lib.load().dmp_relcorr_supported(I, H, R + 1) == 0
    _former_case(I, H, R, gpu, calls, repeatable=False)      # (torch's indexing backward adds with float atomics)
    assert not calls


def test_supported_is_the_documented_range():
    from dualmessagepassing_amd import _lib
    sup = _lib.load().dmp_relcorr_supported
    assert all(sup(i, h, n) == 1 for i in (4, 50, 256) for h in (4, 50, 256) for n in (2, 17))
    assert not any(sup(*a) for a in ((3, 8, 2), (257, 8, 2), (8, 3, 2), (8, 257, 2), (8, 8, 1), (8, 8, 18), (8, 8, 0), (-4, 8, 2)))


@pytest.mark.parametrize("tag", __import__("test_unc_compgcn_cpu").TAGS)
def test_hip_path_matches_the_reference_fixtures(tag, gpu, monkeypatch):
    from test_unc_compgcn_cpu import check_case, load_case, run_case
    calls, aggs = _spy(monkeypatch), _spy_agg(monkeypatch)
    d = load_case(tag)
    model, outs, embed, loss = run_case(d, gpu)
    assert len(calls) == len(aggs) == int(d["layers"]), "the HIP path was not taken"
    check_case(tag, d, model, outs, embed, loss, out_tol=2e-5, grad_tol=5e-4)


def test_kernel_path_equals_the_tensor_op_path_with_types_outside_the_table(gpu, monkeypatch):
    """N 2,000, E 10,000, R 8, H 64, two layers; one edge in ten carries a type outside [0, R) (negative or too large): it
    sends nothing and its row of ``r`` is zero, on both paths -- what ``dmp_relconv_fwd`` does with such an edge."""
    from dualmessagepassing_amd import unc_compgcn
    from dualmessagepassing_amd.graph import BatchedGraph
    calls, aggs = _spy(monkeypatch), _spy_agg(monkeypatch)
    gen = th.Generator().manual_seed(4)
    N, E, R, H = 2000, 10000, 8, 64
    src, dst = th.randint(0, N, (E,), generator=gen), th.randint(0, N - 8, (E,), generator=gen)
    et = th.randint(0, R, (E,), generator=gen)
    odd = th.rand(E, generator=gen) < 0.1
    et = th.where(odd, th.where(th.rand(E, generator=gen) < 0.5, th.full_like(et, -1), et + R), et)
    norm = th.rand(E, 1, generator=gen) + 0.1
    th.manual_seed(0)
    enc = unc_compgcn.CompGCN(None, None, N, H, H, R, num_hidden_layers=2).to(gpu)
    with th.no_grad():
        for layer in enc.layers:
            layer.bias.uniform_(-0.2, 0.2)
    twin = copy.deepcopy(enc)
    wh, wr = th.randn(N, H, generator=gen).to(gpu), th.randn(E, H, generator=gen).to(gpu)
    src, dst, et, norm = src.to(gpu), dst.to(gpu), et.to(gpu), norm.to(gpu)
    nid = th.arange(N, device=gpu).view(-1, 1)

    def run(m):
        h, r = m(BatchedGraph(src, dst, N), nid, et, norm)
        ((h * wh).sum() + (r * wr).sum()).backward()
        return h, r

    h, r = run(enc)
    assert len(calls) == len(aggs) == 2, "the HIP path was not taken"
    with th.no_grad():   # an outside edge sends nothing: the same graph without those edges gives the same nodes
        keep = (et >= 0) & (et < R)
        h3, _ = enc(BatchedGraph(src[keep], dst[keep], N), nid, et[keep], norm[keep])
    assert len(calls) == 4
    _close(h3, h, 2e-5, "h without the outside edges")
    monkeypatch.setattr(unc_compgcn, "kernels_admit", lambda *a: False)
    h2, r2 = run(twin)
    assert len(calls) == len(aggs) == 4                            # the twin took neither kernel
    outside = (et < 0) | (et >= R)
    assert int(outside.sum()) > 500 and float(r.detach()[outside].abs().max()) == 0.0 and float(r2.detach()[outside].abs().max()) == 0.0
    _close(h, h2, 2e-5, "h")
    _close(r, r2, 2e-5, "r")
    for (k, p), q in zip(enc.named_parameters(), twin.parameters()):
        assert (p.grad is None) == (q.grad is None), k
        if p.grad is not None:
            _close(p.grad, q.grad, 2e-4, "grad " + k)


def _two_communities(rng, n, m=1500):
    half = n // 2
    u = rng.integers(0, n, 4 * m)
    v = rng.integers(0, n, 4 * m)
    same = (u < half) == (v < half)
    keep = (u != v) & (same | (rng.random(4 * m) < 0.03))
    pairs = np.unique(np.stack([u[keep], v[keep]], 1), axis=0)[:m]
    return np.stack([pairs[:, 0], rng.integers(0, 3, len(pairs)), pairs[:, 1]], 1)


def test_replayed_training_follows_the_eager_loss_curve(gpu, monkeypatch):
    """``train_unsupervised(replay=True)`` records and replays this model's sampled step; per-epoch losses as the eager loop's to
    1e-3 (the figure of tests/test_gpu_unc_harness.py), most steps replays; ``collect_node_embeddings`` takes the tuple."""
    from dualmessagepassing_amd import unc_harness
    from dualmessagepassing_amd.unc_compgcn import TrainModel
    calls, aggs = _spy(monkeypatch), _spy_agg(monkeypatch)
    rng = np.random.default_rng(11)
    n = 900
    graph, trip = unc_harness.graph_of(_two_communities(rng, n), n, 3, gpu)
    th.manual_seed(0)
    model = TrainModel(None, n, 50, 3, 0, num_hidden_layers=2, dropout=0.0, reg_param=0.01).to(gpu)
    twin = copy.deepcopy(model)
    kw = dict(n_epochs=2, graph_batch_size=300, lr=5e-3, sampler="neighbor", sample_depth=2, sample_width=8, negative_sample=3,
              rescale_epochs=False, seed=1)
    ref = unc_harness.train_unsupervised(model, graph, trip, **kw)
    assert calls and len(aggs) == len(calls), "the HIP path was not taken"
    made = []
    real = unc_harness.SampledStep
    monkeypatch.setattr(unc_harness, "SampledStep", lambda *a, **k: (made.append(real(*a, **k)), made[-1])[1])
    got = unc_harness.train_unsupervised(twin, graph, trip, replay=True, **kw)
    assert len(got) == len(ref) and np.isfinite(got).all()
    for a, b in zip(got, ref):
        assert abs(a - b) <= 1e-3 * max(1.0, abs(b)), (got, ref)
    sg = made[0].steps
    assert sg.replays >= 0.5 * (sg.replays + sg.eager_calls), (sg.replays, sg.eager_calls)
    emb, covered = unc_harness.collect_node_embeddings(twin, graph, trip, graph_batch_size=300, sampler="neighbor", sample_depth=2,
                                                       sample_width=8, negative_sample=3, seed=2)
    assert emb.shape == (n, 50) and bool(th.isfinite(emb).all()) and bool(covered.any())
