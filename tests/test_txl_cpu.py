"""The TXL rep-net (models/txl.py) on the CPU against the reference's own runs (tests/golden/txl/*.npz,
scripts/make_golden_txl.py): the seeded state_dict bit for bit and its key names, outputs 1e-5 and parameter gradients 1e-4
(relative to max(1, |ref|max)) in both memory regimes; the closed form of the unmasked ``rel_shift`` against the
pad-and-reshape form; the folded batch against the segment loop; expand(); the construction error for more than 4 layers."""
import glob
import os

import numpy as np
import pytest
import torch as th

from conftest import GOLDEN
from test_edgeseq_cnn_cpu import _t, build_seeded, config_of, model_inputs, run_and_check

TX = os.path.join(GOLDEN, "txl")
MODELS = sorted(glob.glob(os.path.join(TX, "model_*.npz")))
TAGS = [os.path.basename(p)[len("model_"):-4] for p in MODELS]


def _load(name):
    with np.load(os.path.join(TX, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_every_fixture_case_is_present():
    assert sorted(TAGS) == sorted(["default", "default_h64", "seg8", "seg8_h64", "seg8_pre", "sep", "clamp", "diam"])


def test_build_model_txl_is_an_edge_sequence_model():
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.seqmodel import SEQ_MODELS, TXL, EdgeSeqModel
    d = _load("model_default")
    m = build_model(config_of(d))
    assert isinstance(m, TXL) and isinstance(m, EdgeSeqModel) and SEQ_MODELS["TXL"] is TXL
    assert [n for n, _ in m.g_rep_net["txl"].named_children()] == ["graph_txl_(0)", "graph_txl_(1)", "graph_txl_(2)"]
    assert m.g_rep_net is m.p_rep_net and len(m.g_rep_net) == 3
    # no TXL keyword: seg 64, mem 64, one head, post-norm, and ext_len 0 -- the memory regime
    assert (m.seg_len, m.ext_len, m.mem_len, m.clamp_len, m.num_heads) == (64, 0, 64, -1, 1) and not m.memory_stays_empty()
    assert not m.pos_emb.weight.requires_grad and tuple(m.pos_emb.weight.shape) == (128, 16)
    s = build_model(config_of(_load("model_seg8")))
    assert (s.seg_len, s.ext_len, s.mem_len, s.num_heads) == (8, 8, 8, 4) and s.memory_stays_empty()


def test_state_dict_keys_are_the_reference_names():
    sd = build_seeded(_load("model_sep")).state_dict()
    for k in ("g_rep_net._module_dict.txl.graph_txl_(0).attn.q_net.weight", "g_rep_net._module_dict.txl.graph_txl_(2).attn.r_net.weight",
              "g_rep_net._module_dict.txl.graph_txl_(0).attn.o_net.bias", "g_rep_net._module_dict.txl.graph_txl_(0).attn.layer_norm.weight",
              "g_rep_net._module_dict.txl.graph_txl_(1).ff.layer1.bias", "g_rep_net._module_dict.txl.graph_txl_(1).ff.layer_norm.bias",
              "g_rep_net._param_dict.r_w_bias", "g_rep_net._param_dict.r_r_bias", "p_rep_net._param_dict.r_r_bias",
              "p_rep_net._module_dict.txl.pattern_txl_(1).ff.layer2.weight", "pos_emb.weight"):
        assert k in sd, k
    assert "p_rep_net._module_dict.txl.pattern_txl_(2).ff.layer2.weight" not in sd
    assert tuple(sd["g_rep_net._param_dict.r_w_bias"].shape) == (4, 4)


@pytest.mark.parametrize("tag", TAGS)
def test_seeded_state_dict_matches_the_reference(tag):
    d = _load("model_" + tag)
    sd = build_seeded(d).state_dict()
    ref = {k[len("sd_init."):]: v for k, v in d.items() if k.startswith("sd_init.")}
    assert sorted(sd) == sorted(ref)
    for k, v in sd.items():
        assert th.equal(v, _t(ref[k])), k


@pytest.mark.parametrize("tag", TAGS)
def test_txl_model_on_the_cpu_matches_the_reference(tag):
    d = _load("model_" + tag)
    # nothing is pinned at an identity: LayerNorm affine parameters and o_net.bias are perturbed
    assert any(k.startswith("sd.") and k.endswith(".attn.layer_norm.weight") for k in d)
    assert any(k.startswith("sd.") and k.endswith(".attn.o_net.bias") for k in d)
    config, pattern, graph = model_inputs(d)
    for t, s in (("p", pattern), ("g", graph)):
        for k, v in s.tdata.items():
            if not k.startswith("_"):
                assert th.equal(v, _t(d["%s.%s" % (t, k)])), (t, k)
    if tag.startswith("default"):         # the memory regime with a full memory, and the pad offset of segmenting
        L = graph.u.size(1)
        assert L > 128 and L % 64 != 0 and int(d["g.lens"].min()) == 0
    model = build_seeded(d)
    run_and_check(d, model, pattern, graph, tol=1e-5, gtol=1e-4)
    w = th.rand(graph.u.shape + (3,))
    assert model.refine_edge_weights(w) is w


@pytest.mark.parametrize("tag", ["seg8", "seg8_pre", "sep"])
def test_folded_batch_equals_the_segment_loop_on_the_cpu(tag):
    """With an empty memory the segments are independent: one batch [B S, seg_len, H] computes what the loop computes (the
    same rows through the same row-wise ops; only the GEMMs' blocking may differ, hence 1e-6 and not bit for bit)."""
    d = _load("model_" + tag)
    config, pattern, graph = model_inputs(d)
    outs = []
    for fold in (True, False):
        model = build_seeded(d)
        assert model.memory_stays_empty() and model.fold_segments
        model.fold_segments = fold
        out = run_and_check(d, model, pattern, graph, tol=1e-5, gtol=1e-4)
        outs.append((out["g_e_rep"].detach(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}))
    (a, ga), (b, gb) = outs
    assert float((a - b).abs().max()) <= 1e-6 * max(1.0, float(b.abs().max()))
    for k in gb:
        assert float((ga[k] - gb[k]).abs().max()) <= 1e-6 * max(1.0, float(gb[k].abs().max())), k


@pytest.mark.parametrize("q,k", [(1, 1), (2, 2), (3, 3), (4, 8), (3, 7), (64, 128)])
def test_closed_form_shift_equals_pad_and_reshape(q, k):
    from dualmessagepassing_amd import txl
    bd = th.randn(2, q, k, 3, generator=th.Generator().manual_seed(q * 131 + k))
    assert th.equal(txl.rel_shift(bd), txl.rel_shift_pad(bd))
    # the three branches, spelled out
    m = k - q
    exp = th.zeros_like(bd)
    for i in range(q):
        for j in range(k):
            if j - i < m + 1:
                exp[:, i, j] = bd[:, i, q - 1 - i + j]
            elif j - i > m + 1:
                exp[:, i, j] = bd[:, i + 1, j - i - m - 2]
    assert th.equal(txl.rel_shift(bd), exp)


@pytest.mark.parametrize("q,k", [(1, 1), (2, 2), (3, 3), (4, 8), (3, 7)])
def test_rel_attention_is_the_same_with_either_shift(q, k):
    from dualmessagepassing_amd import txl
    g = th.Generator().manual_seed(q * 17 + k)
    N, nh, dh = 3, 2, 4
    args = [th.randn(N, q, nh, dh, generator=g), th.randn(N, k, nh, dh, generator=g), th.randn(N, k, nh, dh, generator=g),
            th.randn(k, nh, dh, generator=g), th.randn(nh, dh, generator=g), th.randn(nh, dh, generator=g)]
    res = []
    for shift in (txl.rel_shift, txl.rel_shift_pad):
        xs = [a.clone().requires_grad_(True) for a in args]
        o = txl.rel_attention_tensor(*xs, 0.5, shift=shift)
        (o * th.linspace(-1, 1, o.numel()).view_as(o)).sum().backward()
        res.append([o.detach()] + [x.grad for x in xs])
    for a, b in zip(*res):
        assert th.allclose(a, b, rtol=0, atol=1e-6)
    o = txl.rel_attention(*args, 0.5)            # the public entry on the CPU: the tensor ops
    assert th.equal(o, res[0][0])


def test_gradient_reaches_k_net_through_the_memory_but_not_the_memory():
    """The memory rows are detached values, but k_net / v_net are applied to them inside the segment that reads them."""
    from dualmessagepassing_amd import txl
    th.manual_seed(0)
    attn = txl.TXLAttn(16, 16)
    w = th.randn(2, 4, 16)
    mem = th.randn(2, 4, 16, requires_grad=True)
    r = th.randn(1, 8, 16)
    b = th.randn(1, 16)
    out = attn(w * 0.0, r, b, b, mems=mem.detach())
    out.sum().backward()
    assert mem.grad is None and float(attn.v_net.weight.grad.abs().max()) > 0


def test_more_than_four_layers_raise():
    from dualmessagepassing_amd.basemodel import build_model
    config = config_of(_load("model_default"))
    with pytest.raises(ValueError, match="more than 4 layers"):
        build_model(dict(config, rep_num_graph_layers=5))
    with pytest.raises(ValueError, match="more than 4 layers"):
        build_model(dict(config, share_rep_net=False, rep_num_graph_layers=2, rep_num_pattern_layers=5))
    assert len(build_model(dict(config, rep_num_graph_layers=4)).g_rep_net["txl"]) == 4


def test_expand_matches_the_reference():
    d = _load("expand_txl")
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
