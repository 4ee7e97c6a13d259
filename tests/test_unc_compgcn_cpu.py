"""The UNC CompGCN encoder (``unc_compgcn``) on the CPU path against the reference's own model code
(tests/golden/unc_compgcn/, ``scripts/make_golden_unc_compgcn.py``): the reference's state_dict keys and seeded initial
values, per-layer ``(h, r)``, the loss and every parameter gradient; the per-edge call against the table call for the three
compositions; the tensor-op weight former against explicit circulant matrices in fp64 -- value and gradient, on rows that are
not symmetric, so that a convolution in place of the correlation fails."""
import glob
import os

import numpy as np
import pytest
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "unc_compgcn")
CASES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLD, "*.npz")))
TAGS = ["r2_attri_i12_h8_l2", "r2_h50_l1_norm", "r4_h64_l2_n_eq_e", "r8_h50_l2_nonorm", "r8_h64_l2_norm"]


def load_case(tag):
    with np.load(os.path.join(GOLD, tag + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def fresh_model(d):
    from dualmessagepassing_amd.unc_compgcn import TrainModel
    th.manual_seed(int(d["seed"]))
    return TrainModel(d.get("attri"), int(d["num_nodes_table"]), int(d["width"]), int(d["num_rels"]), 0,
                      num_hidden_layers=int(d["layers"]), dropout=0, reg_param=0.01)


def model_of(d, device="cpu"):
    model = fresh_model(d)
    model.load_state_dict({k[3:]: th.from_numpy(v) for k, v in d.items() if k.startswith("sd.")}, strict=True)
    return model.to(device)


def run_case(d, device="cpu"):
    """-> (model, per-layer (h, next table), (h, r), loss) after the backward of the unsupervised loss."""
    from dualmessagepassing_amd.graph import BatchedGraph
    model = model_of(d, device)
    t = lambda k: th.from_numpy(d[k]).to(device)   # noqa: E731
    g = BatchedGraph(t("src"), t("dst"), int(d["nid"].shape[0]))
    norm = t("norm") if int(d["with_norm"]) else None
    outs = []
    hooks = [layer.register_forward_hook(lambda m, a, o: outs.append(o)) for layer in model.model.layers]
    edge_type = t("etype")
    embed, pred = model(g, t("nid").view(-1, 1), edge_type, norm)
    for h in hooks:
        h.remove()
    assert pred is None
    loss = model.get_unsupervised_loss(g, embed, edge_type, t("triplets"), t("labels"))
    loss.backward()
    return model, outs, embed, loss


def close(got, want, rtol, what):
    got, want = got.detach().cpu().double(), th.from_numpy(np.asarray(want)).double()
    assert got.shape == want.shape, what
    scale = max(1.0, float(want.abs().max())) if want.numel() else 1.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    assert err <= rtol * scale, "%s: %g (scale %g)" % (what, err, scale)


def check_case(tag, d, model, outs, embed, loss, out_tol, grad_tol):
    etype = th.from_numpy(d["etype"])
    assert isinstance(embed, tuple) and len(embed) == 2 and len(outs) == int(d["layers"])
    for i, (h, table) in enumerate(outs):
        assert table.shape == (2 * int(d["num_rels"]), int(d["width"]))
        close(h, d["out.layer%d.h" % i], out_tol, "%s layer %d h" % (tag, i))
        close(table.detach().cpu()[etype], d["out.layer%d.r" % i], out_tol, "%s layer %d r" % (tag, i))
    close(embed[0], d["embed.h"], out_tol, tag + " embed h")
    close(embed[1], d["embed.r"], out_tol, tag + " embed r")
    close(loss.view(()), d["loss"], out_tol, tag + " loss")
    grads = {k[5:]: v for k, v in d.items() if k.startswith("grad.")}
    have = {k for k, p in model.named_parameters() if p.grad is not None}
    assert have == set(grads), sorted(have ^ set(grads))
    for k, p in model.named_parameters():
        if k.endswith("out_weight"):
            assert p.grad is None, k
        elif p.grad is not None:
            close(p.grad, grads[k], grad_tol, "%s grad %s" % (tag, k))


def test_the_fixture_set_is_complete():
    assert CASES == TAGS


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_and_seeded_initial_values_are_the_reference_ones(tag):
    """strict load; the keys in the reference's order; a model built from the fixture's seed holds the fixture's values (the
    generator redraws the layers' biases and ``edge_fc.bias`` before its forward: zero at initialisation)."""
    d = load_case(tag)
    model_of(d)
    model = fresh_model(d)
    sd = model.state_dict()
    assert list(sd.keys()) == [k[3:] for k in d if k.startswith("sd.")]
    assert "model.rel_emb.embedding.weight" in sd and "model.layers.0.loop_rel" in sd and "w_relation" in sd
    for k, v in sd.items():
        if k.endswith(".bias") and (".layers." in k or k == "edge_fc.bias"):
            assert float(v.abs().max()) == 0.0, k
        else:
            assert th.equal(v, th.from_numpy(d["sd." + k])), k


@pytest.mark.parametrize("tag", TAGS)
def test_cpu_path_matches_the_reference(tag):
    d = load_case(tag)
    check_case(tag, d, *run_case(d), out_tol=1e-5, grad_tol=2e-4)


def _layer_inputs(comp_opt, with_rev, seed=0):
    from dualmessagepassing_amd.graph import BatchedGraph
    from dualmessagepassing_amd.unc_compgcn import CompGraphConv
    gen = th.Generator().manual_seed(seed)
    N, E, R, I, H = 9, 40, 4, 7, 5
    g = BatchedGraph(th.randint(0, N, (E,), generator=gen), th.randint(0, N - 2, (E,), generator=gen), N)
    if with_rev:
        g.edata["is_rev"] = th.rand(E, generator=gen) < 0.5
    th.manual_seed(seed)
    layer = CompGraphConv(I, H, comp_opt=comp_opt, activation=th.nn.Tanh()).double()
    with th.no_grad():
        layer.bias.uniform_(-0.2, 0.2)
    x = th.randn(N, I, generator=gen, dtype=th.float64)
    T = th.randn(R, I, generator=gen, dtype=th.float64)
    et = th.randint(0, R, (E,), generator=gen)
    norm = th.rand(E, 1, generator=gen, dtype=th.float64) + 0.1
    return g, layer, x, T, et, norm


@pytest.mark.parametrize("with_rev", [False, True])
@pytest.mark.parametrize("comp_opt", ["corr", "sub", "mult"])
def test_per_edge_call_equals_the_table_call(comp_opt, with_rev):
    g, layer, x, T, et, norm = _layer_inputs(comp_opt, with_rev)
    h0, r0 = layer(g, x, T[et], norm)
    h1, T1 = layer.forward_table(g, x, T, et, norm)
    assert h0.shape == (9, 5) and r0.shape == (40, 5) and T1.shape == (4, 5)
    assert float((h0 - h1).detach().abs().max()) <= 1e-12 and float((r0 - T1[et]).detach().abs().max()) <= 1e-12
    if with_rev:                                           # the reversed edges went through out_weight
        with th.no_grad():
            layer.out_weight.zero_()
        assert float((layer(g, x, T[et], norm)[0] - h0).detach().abs().max()) > 1e-3


def test_corr_is_the_correlation_of_the_reference():
    """``corr(a, b)[k] = sum_i a[i] b[(i + k) mod I]`` on rows without symmetry, odd and even lengths."""
    from dualmessagepassing_amd.unc_compgcn import circulant, corr
    from util_fp64_compgcn import circulant_fp64, corr_fp64
    gen = th.Generator().manual_seed(3)
    for n in (4, 7, 50):
        a, t = th.randn(6, n, generator=gen, dtype=th.float64), th.randn(n, generator=gen, dtype=th.float64)
        want = corr_fp64(a.numpy(), t.numpy())
        assert np.abs(corr(a, t.view(1, -1)).numpy() - want).max() <= 1e-12
        assert np.array_equal(circulant(t).numpy(), circulant_fp64(t.numpy()))
        i = np.arange(n)
        conv = a.numpy() @ t.numpy()[(i[None, :] - i[:, None]) % n]    # the roll in the other direction: a convolution
        assert np.abs(conv - want).max() > 0.1


@pytest.mark.parametrize("I,H,R", [(4, 4, 1), (12, 8, 2), (50, 50, 2), (7, 5, 3)])
def test_tensor_op_weight_former_equals_explicit_circulants(I, H, R):
    from dualmessagepassing_amd.unc_compgcn import LOOP_SCALE, corr_weights_tensor_ops
    from dualmessagepassing_amd.unc_rel import padded_width
    from util_fp64_compgcn import relcorr_weights_bwd_fp64, relcorr_weights_fp64
    gen = th.Generator().manual_seed(I * 100 + H)
    P = padded_width(H)
    T, lr, Win, Wl = (th.randn(*s, generator=gen, dtype=th.float64).requires_grad_(True) for s in ((R, I), (1, I), (I, H), (I, H)))
    Wcat = corr_weights_tensor_ops(T, lr, Win, Wl, P, LOOP_SCALE)
    want = relcorr_weights_fp64(T.detach().numpy(), lr.detach().numpy(), Win.detach().numpy(), Wl.detach().numpy(), P, LOOP_SCALE)
    assert Wcat.shape == (I, (R + 1) * P) and np.abs(Wcat.detach().numpy() - want).max() <= 1e-12
    if P != H:
        assert float(Wcat.detach().view(I, R + 1, P)[:, :, H:].abs().max()) == 0.0
    d = th.randn(I, (R + 1) * P, generator=gen, dtype=th.float64)
    Wcat.backward(d)
    wants = relcorr_weights_bwd_fp64(d.numpy(), T.detach().numpy(), lr.detach().numpy(), Win.detach().numpy(), Wl.detach().numpy(), P,
                                     LOOP_SCALE)
    for got, w, name in zip((T.grad, lr.grad.view(-1), Win.grad, Wl.grad), wants, ("dT", "dloop_rel", "dWin", "dWloop")):
        assert np.abs(got.numpy() - w).max() <= 1e-11, name
    # h @ W_b is the reference's message: corr(h, t_b) @ in_weight
    from dualmessagepassing_amd.unc_compgcn import corr
    h = th.randn(5, I, generator=gen, dtype=th.float64)
    msg = (h @ Wcat.detach()).view(5, R + 1, P)[:, 0, :H]
    assert float((msg - LOOP_SCALE * corr(h, T.detach()[0:1]) @ Win.detach()).abs().max()) <= 1e-12


def test_edge_types_outside_the_table_send_nothing():
    """Documented in ``unc_compgcn``: a type outside [0, R) sends no message and its row of ``r`` is zero."""
    from dualmessagepassing_amd.graph import BatchedGraph
    from dualmessagepassing_amd.unc_compgcn import CompGCN
    th.manual_seed(0)
    enc = CompGCN(None, None, 6, 8, 8, 4, num_hidden_layers=2)
    src, dst = th.tensor([0, 1, 2, 3, 4]), th.tensor([1, 2, 3, 4, 5])
    et = th.tensor([0, 7, 3, -1, 2])
    nid = th.arange(6).view(-1, 1)
    keep = th.tensor([0, 2, 4])
    with th.no_grad():
        h, r = enc(BatchedGraph(src, dst, 6), nid, et, None)
        h2, r2 = enc(BatchedGraph(src[keep], dst[keep], 6), nid, et[keep], None)
    assert float((h - h2).abs().max()) <= 1e-6 and float((r[keep] - r2).abs().max()) <= 1e-6
    assert float(r[[1, 3]].abs().max()) == 0.0


def test_supervised_head_and_the_other_options_run():
    from dualmessagepassing_amd.graph import BatchedGraph
    from dualmessagepassing_amd.unc_compgcn import CompGraphConv, TrainModel
    th.manual_seed(0)
    model = TrainModel(None, 10, 8, 2, 3, num_hidden_layers=1)
    assert "node_fc.weight" in model.state_dict() and "w_relation" not in model.state_dict()
    g = BatchedGraph(th.tensor([0, 1, 2]), th.tensor([1, 2, 0]), 4)
    (h, r), pred = model(g, th.arange(4).view(-1, 1), th.tensor([0, 3, 1]), None)
    assert h.shape == (4, 8) and r.shape == (3, 8) and pred.shape == (4, 3)
    layer = CompGraphConv(8, 8, self_loop=False, comp_opt="corr", batch_norm=True, activation=th.nn.ReLU(), dropout=0.5)
    assert layer.loop_weight is None and layer.loop_rel is None and layer.num_rels == 2
    out, table = layer.forward_table(g, th.randn(4, 8), th.randn(4, 8), th.tensor([0, 3, 1]))
    assert out.shape == (4, 8) and bool((out >= 0).all()) and table.shape == (4, 8)
