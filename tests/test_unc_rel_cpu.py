"""The UNC baseline encoders R-GCN / R-GIN (``unc_rel``, ``unc.TrainModel(encoder=...)``) on the CPU path against the
reference's own model code (tests/golden/unc_rel/, ``scripts/make_golden_unc_rel.py``): per-layer outputs, the loss and
every parameter gradient; the reference's state_dict keys; the options that are refused; the regulariser on a padded
sub-graph whose node and edge capacities collide."""
import glob
import os

import numpy as np
import pytest
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "unc_rel")
CASES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLD, "*.npz")))


def load_case(tag):
    with np.load(os.path.join(GOLD, tag + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def model_of(d, device="cpu"):
    """``TrainModel`` of the fixture's configuration with its parameters; ``num_bases`` < R rebuilds the layers as the
    generator did."""
    from dualmessagepassing_amd import unc_rel
    from dualmessagepassing_amd.unc import TrainModel
    kind = str(d["kind"])
    encoder = {"R-GCN": "RGCN", "R-GIN": "RGIN"}[kind]
    model = TrainModel(None, int(d["num_nodes_table"]), int(d["width"]), int(d["num_rels"]), 0, num_hidden_layers=int(d["layers"]),
                       dropout=0, reg_param=0.01, encoder=encoder)
    bases = int(d["num_bases"])
    if bases > 0:
        cls = unc_rel.RelGraphIso if kind == "R-GIN" else unc_rel.RelGraphConv
        R = 2 * int(d["num_rels"])
        for i, old in enumerate(model.model.layers):
            model.model.layers[i] = cls(old.in_feat, old.out_feat, R, "basis", bases, activation=old.activation)
    sd = {k[3:]: th.from_numpy(v) for k, v in d.items() if k.startswith("sd.")}
    model.load_state_dict(sd, strict=True)
    return model.to(device)


def run_case(d, device="cpu"):
    """-> (model, per-layer outputs, final embedding, loss) after the backward of the unsupervised loss."""
    from dualmessagepassing_amd.graph import BatchedGraph
    model = model_of(d, device)
    t = lambda k: th.from_numpy(d[k]).to(device)   # noqa: E731
    N = int(d["nid"].shape[0])
    g = BatchedGraph(t("src"), t("dst"), N)
    norm = t("norm") if int(d["with_norm"]) else None
    if norm is not None:
        g.edata["norm"] = norm
    outs = []
    hooks = [layer.register_forward_hook(lambda m, a, o: outs.append(o)) for layer in model.model.layers]
    edge_type = t("etype")
    embed, _ = model(g, t("nid").view(-1, 1), edge_type, norm)
    for h in hooks:
        h.remove()
    loss = model.get_unsupervised_loss(g, embed, edge_type, t("triplets"), t("labels"))
    loss.backward()
    return model, outs, embed, loss


def close(got, want, rtol, what):
    got, want = got.detach().cpu().double(), th.from_numpy(np.asarray(want)).double()
    assert got.shape == want.shape, what
    scale = max(1.0, float(want.abs().max())) if want.numel() else 1.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    assert err <= rtol * scale, "%s: %g (scale %g)" % (what, err, scale)


@pytest.mark.parametrize("tag", CASES)
def test_cpu_path_matches_the_reference(tag):
    d = load_case(tag)
    model, outs, embed, loss = run_case(d)
    assert isinstance(embed, th.Tensor)                          # one node tensor, not a tuple
    assert len(outs) == int(d["layers"])
    for i, o in enumerate(outs):
        close(o, d["out.layer%d" % i], 1e-5, "%s layer %d" % (tag, i))
    close(embed, d["embed"], 1e-5, tag + " embed")
    close(loss.view(()), d["loss"], 1e-5, tag + " loss")
    grads = {k[5:]: v for k, v in d.items() if k.startswith("grad.")}
    have = {k for k, p in model.named_parameters() if p.grad is not None}
    assert have == set(grads), sorted(have ^ set(grads))
    for k, p in model.named_parameters():
        if p.grad is not None:
            close(p.grad, grads[k], 2e-4, "%s grad %s" % (tag, k))


@pytest.mark.parametrize("encoder,kind", [("RGCN", "R-GCN"), ("RGIN", "R-GIN")])
def test_state_dict_keys_are_the_reference_keys(encoder, kind):
    from dualmessagepassing_amd.unc import TrainModel
    tags = [t for t in CASES if str(load_case(t)["kind"]) == kind and int(load_case(t)["num_bases"]) < 0
            and int(load_case(t)["layers"]) == 2]
    d = load_case(tags[0])
    model = TrainModel(None, 30, 16, int(d["num_rels"]), 0, num_hidden_layers=2, encoder=encoder)
    assert list(model.state_dict().keys()) == [k[3:] for k in d if k.startswith("sd.")]
    assert model.model.num_nodes == 30 and model.model.node_emb.weight.shape == (30, 16)
    assert model.model.layers[0].weight.shape == (2 * int(d["num_rels"]), 16, 16)


def test_num_bases_and_parameter_shapes():
    from dualmessagepassing_amd.unc_rel import RelGraphConv
    for nb in (None, 0, -1, 9):
        m = RelGraphConv(5, 7, 6, num_bases=nb)
        assert m.num_bases == 6 and not hasattr(m, "w_comp")
    m = RelGraphConv(5, 7, 6, num_bases=2)
    assert m.weight.shape == (2, 5, 7) and m.w_comp.shape == (6, 2)
    assert m.h_bias.shape == (7,) and m.loop_weight.shape == (5, 7)
    assert float(m.h_bias.detach().abs().max()) == 0.0
    assert [k for k, _ in m.named_parameters()] == ["weight", "w_comp", "h_bias", "loop_weight"]


def test_refused_options_raise():
    from dualmessagepassing_amd.graph import BatchedGraph
    from dualmessagepassing_amd.unc import TrainModel
    from dualmessagepassing_amd.unc_rel import RelGraphConv
    with pytest.raises(NotImplementedError):
        RelGraphConv(4, 4, 2, regularizer="bdd", num_bases=2)
    with pytest.raises(NotImplementedError):
        RelGraphConv(4, 4, 2, layer_norm=True)
    m = RelGraphConv(4, 4, 2)
    g = BatchedGraph(th.tensor([0, 1]), th.tensor([1, 2]), 3)
    with pytest.raises(NotImplementedError):
        m(g, th.tensor([0, 1, 2]), th.tensor([0, 1]))
    with pytest.raises(ValueError):
        TrainModel(None, 10, 8, 2, 0, encoder="CompGCN")


def test_dropout_and_other_activations_run_after_the_conv():
    from dualmessagepassing_amd.graph import BatchedGraph
    from dualmessagepassing_amd.unc_rel import RelGraphConv
    th.manual_seed(0)
    g = BatchedGraph(th.tensor([0, 1, 2, 2]), th.tensor([1, 2, 0, 1]), 3)
    et = th.tensor([0, 1, 1, 0])
    x = th.randn(3, 6)
    m = RelGraphConv(6, 5, 2, activation=th.nn.ReLU(), dropout=0.5)
    m.eval()
    ref = m.conv(g, x, et)
    assert bool((ref >= 0).all())
    m.train()
    out = m(g, x, et)
    assert bool(((out == 0) | th.isclose(out, 2 * ref)).all())


def _padded_pair(N, E, num_rels, d, gen):
    """A sub-graph of N nodes and E edges and its ``pad_sampled`` form (CPU)."""
    from dualmessagepassing_amd.graph import BatchedGraph
    from dualmessagepassing_amd.unc import PaddedRows
    from dualmessagepassing_amd.unc_harness import SUBGRAPH_NID, pad_sampled
    src, dst = th.randint(0, N, (E,), generator=gen), th.randint(0, N, (E,), generator=gen)
    sub = BatchedGraph(src, dst, N)
    sub.ndata[SUBGRAPH_NID] = th.arange(N)
    sub.edata["norm"] = th.rand(E, 1, generator=gen)
    edge_type = th.randint(0, 2 * num_rels, (E,), generator=gen)
    (ncap, ecap), (psrc, pdst, ptype, pnorm, pnid, counts) = pad_sampled(sub, edge_type, parent_nodes=N)
    valid = PaddedRows(counts[0:1], counts[1:2], ncap, ecap)
    return sub, edge_type, (ncap, ecap), ptype, valid


@pytest.mark.parametrize("encoder", ["RGCN", "RGIN", "DMPNN"])
def test_regulariser_on_a_padded_graph_whose_capacities_collide(encoder):
    """N 1600, E 2000: both capacities are 2048.  The padded regulariser must equal the regulariser of the sub-graph itself:
    the edge term never takes the node representation because the padded row counts happen to be equal."""
    from dualmessagepassing_amd.unc import TrainModel
    gen = th.Generator().manual_seed(5)
    N, E, num_rels, dim = 1600, 2000, 3, 16
    sub, edge_type, (ncap, ecap), ptype, valid = _padded_pair(N, E, num_rels, dim, gen)
    assert ncap == ecap == 2048 and N != E
    th.manual_seed(1)
    model = TrainModel(None, N, dim, num_rels, 0, reg_param=0.01, encoder=encoder)
    h = th.randn(N, dim, generator=gen)
    hp = th.cat([h, th.randn(ncap - N, dim, generator=gen)])       # inert rows: anything
    if encoder == "DMPNN":
        z = th.randn(E, dim, generator=gen)
        r = th.randn(2 * num_rels, dim, generator=gen)
        real, padded = (h, z, r), (hp, th.cat([z, th.randn(ecap - E, dim, generator=gen)]), r)
    else:
        real, padded = h, hp
    want = model.unsupervised_regularization_loss(real, edge_type=edge_type)
    got = model.unsupervised_regularization_loss(padded, edge_type=ptype, valid=valid)
    assert abs(float(got) - float(want)) <= 1e-5 * max(1.0, abs(float(want))), (float(got), float(want))


def test_single_tensor_encoders_take_the_edge_term_when_nodes_equal_edges():
    """The reference's rule, eager: a node tensor with as many rows as edges goes through ``edge_fc`` (pinned by the
    ``*_n_eq_e`` fixture); with fewer rows it does not."""
    from dualmessagepassing_amd.unc import TrainModel
    th.manual_seed(0)
    model = TrainModel(None, 10, 8, 2, 0, reg_param=0.01, encoder="RGCN")
    et = th.tensor([0, 1, 2, 3, 0, 1])
    emb = th.randn(6, 8)
    with_term = model.unsupervised_regularization_loss(emb, edge_type=et)
    without = model.unsupervised_regularization_loss(emb[:5], edge_type=et)
    plain = th.mean(model.w_relation.pow(2))
    assert float(without) == pytest.approx(float(plain + emb[:5].pow(2).mean()), rel=1e-6)
    mask = et < 2
    diff = model.edge_fc(emb[mask]) - model.w_relation[et[mask]]
    assert float(with_term) == pytest.approx(float(plain + emb.pow(2).mean() + diff.pow(2).mean()), rel=1e-5)
