"""The RNN rep-net (models/rnn.py: LSTM, GRU, RNN; uni- and bidirectional) on the CPU against the reference's own runs
(tests/golden/rnn/*.npz, scripts/make_golden_rnn.py): the seeded state_dict bit for bit, outputs 1e-4 and parameter
gradients 2e-4 (relative to max(1, |ref|max)) with nonzero RNN biases over pre-padded, ragged, gated batches; a reference
state_dict loads with strict=True; expand(); the construction errors and keys of the reference."""
import glob
import os

import numpy as np
import pytest
import torch as th

from conftest import GOLDEN
from test_edgeseq_cnn_cpu import _t, build_seeded, config_of, model_inputs, run_and_check

RN = os.path.join(GOLDEN, "rnn")
MODELS = sorted(glob.glob(os.path.join(RN, "model_*.npz")))
TAGS = [os.path.basename(p)[len("model_"):-4] for p in MODELS]


def _load(name):
    with np.load(os.path.join(RN, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_every_fixture_case_is_present():
    assert sorted(TAGS) == sorted(["lstm_uni", "lstm_bi", "gru_uni", "gru_bi", "rnn_uni", "lstm_sep", "gru_diam", "lstm_bi_h64",
                                   "gru_uni_h64"])


def test_build_model_rnn_is_an_edge_sequence_model():
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.seqmodel import RNN, SEQ_MODELS, EdgeSeqModel
    d = _load("model_lstm_bi")
    m = build_model(config_of(d))
    assert isinstance(m, RNN) and isinstance(m, EdgeSeqModel) and SEQ_MODELS["RNN"] is RNN
    assert [n for n, _ in m.g_rep_net["rnn"].named_children()] == ["graph_rnn_(0)", "graph_rnn_(1)", "graph_rnn_(2)"]
    assert m.g_rep_net is m.p_rep_net
    layer = list(m.g_rep_net["rnn"])[0]
    assert isinstance(layer.layer, th.nn.LSTM) and layer.layer.bidirectional and layer.layer.hidden_size == 8
    assert layer.layer.batch_first and layer.get_output_dim() == 16


@pytest.mark.parametrize("tag", TAGS)
def test_seeded_state_dict_matches_the_reference(tag):
    d = _load("model_" + tag)
    sd = build_seeded(d).state_dict()
    ref = {k[len("sd_init."):]: v for k, v in d.items() if k.startswith("sd_init.")}
    assert sorted(sd) == sorted(ref)
    for k, v in sd.items():
        assert th.equal(v, _t(ref[k])), k


@pytest.mark.parametrize("tag", TAGS)
def test_rnn_model_on_the_cpu_matches_the_reference(tag):
    d = _load("model_" + tag)
    assert any(k.startswith("sd.") and ".bias_hh_l0" in k for k in d)      # the fixtures run with nonzero RNN biases
    config, pattern, graph = model_inputs(d)
    for t, s in (("p", pattern), ("g", graph)):
        for k, v in s.tdata.items():
            if not k.startswith("_"):
                assert th.equal(v, _t(d["%s.%s" % (t, k)])), (t, k)
    model = build_seeded(d)
    run_and_check(d, model, pattern, graph)
    w = th.rand(graph.u.shape + (3,))
    assert model.refine_edge_weights(w) is w


def test_padding_is_part_of_the_function():
    """With nonzero biases the forward state drifts through the pre-padding: one more row of padding changes the output
    of a sequence at its real positions (the reference runs the recurrence over all L positions)."""
    from dualmessagepassing_amd.seqmodel import RNNLayer
    th.manual_seed(0)
    layer = RNNLayer("LSTM", 8, 8)
    with th.no_grad():
        layer.layer.bias_ih_l0.uniform_(-0.3, 0.3)
    x = th.randn(1, 5, 8)
    a = layer.forward_rows(x, None, False)
    b = layer.forward_rows(th.cat([th.zeros(1, 1, 8), x], 1), None, False)[:, 1:]
    assert not th.allclose(a, b)


def test_expand_matches_the_reference():
    d = _load("expand_rnn")
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


def test_unknown_rnn_type_raises_at_construction():
    from dualmessagepassing_amd.basemodel import build_model
    config = config_of(_load("model_lstm_uni"))
    with pytest.raises(ValueError, match="rep_rnn_type"):
        build_model(dict(config, rep_rnn_type="SRU"))


def test_layer_norm_flag_adds_no_parameters():
    """The reference reads rep_rnn_layer_norm but never passes it to RNNLayer: no ``ln`` keys."""
    from dualmessagepassing_amd.basemodel import build_model
    config = config_of(_load("model_lstm_uni"))
    th.manual_seed(1)
    a = build_model(dict(config, rep_rnn_layer_norm=True)).state_dict()
    th.manual_seed(1)
    b = build_model(config).state_dict()
    assert not any(".ln." in k for k in a)
    assert sorted(a) == sorted(b) and all(th.equal(a[k], b[k]) for k in a)


def test_rnn_init_branch_is_xavier_at_gain_one_and_zero_bias():
    from dualmessagepassing_amd.act import init_module
    m = th.nn.GRU(16, 8, bidirectional=True)
    th.manual_seed(3)
    init_module(m, activation="relu")
    th.manual_seed(3)
    for layer_weights in m._all_weights:
        for w in layer_weights:
            p = getattr(m, w)
            if "weight" in w:
                a = (6.0 / (p.size(0) + p.size(1))) ** 0.5
                ref = th.empty_like(p).uniform_(-a, a)
                assert th.equal(p, ref), w
            else:
                assert th.equal(p, th.zeros_like(p)), w


def test_cpu_tensors_take_the_module_path():
    from dualmessagepassing_amd import rnn
    from dualmessagepassing_amd.seqmodel import RNNLayer
    layer = RNNLayer("GRU", 64, 64)
    x = th.randn(2, 3, 64)
    assert not rnn.hip_layer_ok(layer, x, None)
    assert layer.forward_rows(x, th.ones(2, 3), True).shape == (2, 3, 64)
