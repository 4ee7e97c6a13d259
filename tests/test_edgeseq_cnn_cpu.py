"""The edge-sequence input and the CNN rep-net (dataset.py EdgeSeq, models/basemodel.py EdgeSeqModel, models/cnn.py) on
the CPU against the reference's own runs (tests/golden/edgeseq/*.npz, scripts/make_golden_edgeseq.py): codes, reversed
tuples, batches, degrees and weights bit for bit; the model's seeded state_dict bit for bit, outputs 1e-4 and parameter
gradients 2e-4 (relative to max(1, |ref|max)); a reference state_dict loads with strict=True."""
import glob
import os

import numpy as np
import pytest
import torch as th

from conftest import GOLDEN

ES = os.path.join(GOLDEN, "edgeseq")


def _load(name):
    with np.load(os.path.join(ES, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _t(a):
    return th.from_numpy(np.asarray(a))


def _close(got, ref, tol, what):
    got, ref = got.detach().cpu().double(), _t(ref).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.numel():
        scale = max(1.0, float(ref.abs().max()))
        err = float((got - ref).abs().max())
        assert err <= tol * scale, (what, err, scale)


def _graph(d, prefix):
    return {k: d["%s.%s" % (prefix, k)] for k in ("src", "dst", "nid", "nlabel", "elabel")}


def _code(g):
    from dualmessagepassing_amd import edgeseq
    return edgeseq.from_graph(g["src"], g["dst"], g["nid"], g["nlabel"], g["elabel"])


def config_of(d):
    return {k: eval(v) for k, v in zip(d["config_keys"].tolist(), d["config_vals"].tolist())}


def model_inputs(d, device="cpu"):
    """The fixture's ragged batch through this package's own pipeline: from_graph, add_reversed_edges, EdgeSeq.batch."""
    from dualmessagepassing_amd import edgeseq
    config = config_of(d)
    seqs = {}
    for t, nel in (("p", config["max_npel"] // 2), ("g", config["max_ngel"] // 2)):
        codes, flags = [], []
        for i in range(int(d["num"])):
            c = _code(_graph(d, "%s%d" % (t, i)))
            f = None
            if config["add_rev"]:
                c, f, _ = edgeseq.add_reversed_edges(c, nel)
            codes.append(c)
            flags.append(f)
        seqs[t], _ = edgeseq.EdgeSeq.batch(codes, device, flags=flags if config["add_rev"] else None)
    return config, seqs["p"], seqs["g"]


def build_seeded(d):
    from dualmessagepassing_amd.basemodel import build_model
    config = config_of(d)
    th.manual_seed(int(d["seed"]))
    return build_model(config)


def reference_state(d):
    sd = {k[len("sd_init."):]: _t(v) for k, v in d.items() if k.startswith("sd_init.")}
    sd.update({k[len("sd."):]: _t(v) for k, v in d.items() if k.startswith("sd.")})
    return sd


def run_and_check(d, model, pattern, graph, device="cpu", tol=1e-4, gtol=2e-4):
    model.load_state_dict({k: v.to(device) for k, v in reference_state(d).items()}, strict=True)
    model.to(device)
    out = model(pattern, graph)
    total = out["pred_c"].sum()
    if out["pred_e"] is not None:
        total = total + (out["pred_e"] * th.linspace(-1, 1, out["pred_e"].numel(), device=device).view_as(out["pred_e"])).sum()
    total = total + (out["g_e_rep"] ** 2).sum() * 1e-3
    total.backward()
    for k in out.keys():
        ref = d.get("out." + k)
        if ref is None:
            assert out[k] is None, k
        elif ref.dtype == np.bool_:
            assert th.equal(out[k].cpu(), _t(ref)), k
        else:
            _close(out[k], ref, tol, k)
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert sorted(grads) == sorted(k[len("grad."):] for k in d if k.startswith("grad."))
    for k, g in grads.items():
        _close(g, d["grad." + k], gtol, "grad " + k)
    for k, v in model.state_dict().items():
        if "sd_after." + k in d:
            _close(v, d["sd_after." + k], tol, k)
    return out


MODELS = sorted(glob.glob(os.path.join(ES, "model_*.npz")))


def test_build_model_cnn_is_an_edge_sequence_model():
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.seqmodel import CNN
    d = _load("model_a")
    m = build_model(config_of(d))
    assert isinstance(m, CNN)
    assert [n for n, _ in m.g_rep_net["cnn"].named_children()] == ["graph_cnn_(0)", "graph_cnn_(1)", "graph_cnn_(2)"]
    assert m.g_rep_net is m.p_rep_net


def test_from_graph_and_reversed_tuples_match_the_reference():
    from dualmessagepassing_amd import edgeseq
    d = _load("seq_codes")
    for i in range(int(d["num"])):
        c = _code(_graph(d, "g%d" % i))
        assert np.array_equal(c, d["code%d" % i].reshape(-1, 5)), i
        r, f, _ = edgeseq.add_reversed_edges(c, int(d["max_nel"]))
        assert np.array_equal(r, d["rcode%d" % i].reshape(-1, 5)), i
        assert np.array_equal(f, d["rflag%d" % i]), i


@pytest.mark.parametrize("tag", ["fwd", "rev"])
def test_pre_padded_batch_and_degrees_match_the_reference(tag):
    from dualmessagepassing_amd import edgeseq
    d = _load("seq_codes")
    codes, flags = [], []
    for i in range(int(d["num"])):
        c = _code(_graph(d, "g%d" % i))
        if tag == "rev":
            c, f, _ = edgeseq.add_reversed_edges(c, int(d["max_nel"]))
            flags.append(f)
        codes.append(c)
    b, _ = edgeseq.EdgeSeq.batch(codes, "cpu", flags=flags or None)
    for k in ("u", "v", "ul", "el", "vl") + (("is_reversed",) if tag == "rev" else ()):
        assert th.equal(b.tdata[k], _t(d["%s.%s" % (tag, k)])), k
    assert th.equal(b.batch_num_tuples(), _t(d[tag + ".lens"]))
    assert th.equal(b.batch_num_nodes(), _t(d[tag + ".num_nodes"]))
    assert th.equal(b.in_degrees(), _t(d[tag + ".in_deg"]))
    assert th.equal(b.out_degrees(), _t(d[tag + ".out_deg"]))


def test_edge_weights_before_and_after_reversal_match_the_reference():
    from dualmessagepassing_amd import edgeseq
    d = _load("seq_weights")
    for i in range(int(d["num"])):
        p, g = _code(_graph(d, "p%d" % i)), _code(_graph(d, "g%d" % i))
        subs = d["subs%d" % i]
        w = edgeseq.edge_weights(p, g, subs, len(subs))
        assert np.array_equal(w, d["w_fwd%d" % i]), i
        pr, _, _ = edgeseq.add_reversed_edges(p, int(d["max_npel"]))
        gr, gf, _ = edgeseq.add_reversed_edges(g, int(d["max_ngel"]))
        assert np.array_equal(edgeseq.map_reversed_weights(gr, gf, w, int(d["max_ngel"])), d["w_mapped%d" % i]), i
        assert np.array_equal(edgeseq.edge_weights(pr, gr, subs, len(subs)), d["w_rev%d" % i]), i


@pytest.mark.parametrize("path", MODELS, ids=lambda p: os.path.basename(p)[:-4])
def test_seeded_state_dict_matches_the_reference(path):
    d = _load(os.path.basename(path)[:-4])
    model = build_seeded(d)
    sd = model.state_dict()
    ref = {k[len("sd_init."):]: v for k, v in d.items() if k.startswith("sd_init.")}
    assert sorted(sd) == sorted(ref)
    for k, v in sd.items():
        assert th.equal(v, _t(ref[k])), k


@pytest.mark.parametrize("path", MODELS, ids=lambda p: os.path.basename(p)[:-4])
def test_cnn_model_on_the_cpu_matches_the_reference(path):
    d = _load(os.path.basename(path)[:-4])
    config, pattern, graph = model_inputs(d)
    for t, s in (("p", pattern), ("g", graph)):
        for k, v in s.tdata.items():
            if not k.startswith("_"):
                assert th.equal(v, _t(d["%s.%s" % (t, k)])), (t, k)
    model = build_seeded(d)
    run_and_check(d, model, pattern, graph)
    with th.no_grad():
        for kind, use_max in (("sum", False), ("max", True)):
            for n in ("2", "3"):
                _close(model.refine_edge_weights(_t(d["refine.w" + n]), use_max=use_max), d["refine.%s%s" % (kind, n)], 1e-6, kind + n)
        got = model.refine_edge_weights((_t(d["refine.w2"]) * 5).long())
        assert got.dtype == th.long and th.equal(got, _t(d["refine.long"]))


def test_expand_matches_the_reference():
    d = _load("expand_cnn")
    from dualmessagepassing_amd.basemodel import build_model
    config = config_of(d)
    th.manual_seed(int(d["seed"]))
    model = build_model(config)
    for k, v in model.state_dict().items():
        assert th.equal(v, _t(d["sd." + k])), k
    grow = dict(zip(d["grow_keys"].tolist(), [int(x) for x in d["grow_vals"]]))
    th.manual_seed(int(d["seed_grow"]))
    model.expand(**dict(config, **grow))
    sd = model.state_dict()
    assert sorted(sd) == sorted(k[len("sd_after."):] for k in d if k.startswith("sd_after."))
    for k, v in sd.items():
        assert th.equal(v, _t(d["sd_after." + k])), k


def test_unsupported_pool_geometry_raises_like_the_reference():
    """k = 2 with stride 2: the pool kernel is 1 with padding 1 -- torch refuses it, in the reference as here."""
    from dualmessagepassing_amd.seqmodel import CNNLayer
    layer = CNNLayer(8, 8, kernel_size=2, stride=2, batch_norm=False)
    with pytest.raises(RuntimeError):
        layer.forward_rows(th.randn(2, 5, 8), th.ones(2, 5), True)
