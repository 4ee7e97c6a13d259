"""Emit the RNN rep-net fixtures under tests/golden/rnn/ by running the REFERENCE's own ``models/rnn.py``.

Runs only in the development container (needs the reference checkout), over the DGL / numba / igraph stand-ins of
``oracle/ref_standin.py`` (read-only use of ``oracle/``), single threaded with deterministic algorithms, as
``scripts/make_golden_edgeseq.py`` runs (its batch helpers are reused unchanged).  Outputs are data only: inputs,
parameters, expected outputs and gradients.

    python scripts/make_golden_rnn.py      # writes tests/golden/rnn/*.npz  (DMP_GOLDEN_RNN_OUT: elsewhere)

Every batch is ragged and pre-padded (one empty graph; the shortest rows carry 20 or more rows of padding), the filter
gate opens holes, and after ``sd_init`` is recorded every RNN bias of the rep-net is set to a nonzero value, so that the
forward direction's drift through the padding is part of what the fixtures pin.

Fixtures
  model_<tag>.npz   RNN (EdgeSeqModel) on such a batch: the 15 OutputDict entries, parameter gradients, the seeded
                    state_dict and the perturbed parameters.  Tags: lstm_uni, lstm_bi, gru_uni, gru_bi, rnn_uni (hid_dim
                    16, 3 layers, add_rev, edge weights), lstm_sep (share_rep_net=False with 2 pattern layers,
                    pred_with_enc, pred_with_deg), gru_diam (DIAMNet head), lstm_bi_h64 and gru_uni_h64 (hid_dim 64:
                    Hd 32 and 64, the widths of the HIP path)
  expand_rnn.npz    BaseModel.expand() of an RNN with pred_with_enc
"""
import os
import sys

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("DMP_GOLDEN_RNN_OUT") or os.path.join(ROOT, "tests", "golden", "rnn")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import make_golden as MG            # noqa: E402  (its helpers; importing it sets one thread and deterministic algorithms)
import make_golden_edgeseq as ES    # noqa: E402  (model_batch, put_graph)

th.set_num_threads(1)
th.use_deterministic_algorithms(True)


def save(name, d):
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **MG.t2n(d))
    print("wrote", name + ".npz")


def base_config(**kw):
    c = dict(max_ngv=24, max_ngvl=6, max_nge=64, max_ngel=8, max_npv=8, max_npvl=6, max_npe=16, max_npel=8, base=2, hid_dim=16,
             share_emb_net=True, share_enc_net=True, share_rep_net=True, rep_residual=True, enc_net="Multihot",
             emb_net="Orthogonal", filter_net="ScalarFilter", rep_net="RNN", rep_num_graph_layers=3, rep_num_pattern_layers=3,
             rep_dropout=0.0, rep_rnn_type="LSTM", rep_rnn_bidirectional=False, pred_net="SumPredictNet", pred_hid_dim=16,
             pred_act_func="relu", pred_dropout=0.0, pred_return_weights="edge", add_rev=True)
    c.update(kw)
    return c


MODEL_CASES = [
    ("lstm_uni", dict()),
    ("lstm_bi", dict(rep_rnn_bidirectional=True)),
    ("gru_uni", dict(rep_rnn_type="GRU")),
    ("gru_bi", dict(rep_rnn_type="GRU", rep_rnn_bidirectional=True)),
    ("rnn_uni", dict(rep_rnn_type="RNN")),
    ("lstm_sep", dict(share_rep_net=False, rep_num_pattern_layers=2, pred_with_enc=True, pred_with_deg=True)),
    ("gru_diam", dict(rep_rnn_type="GRU", pred_net="DIAMNet", pred_num_heads=4, pred_infer_steps=1, pred_mem_len=4,
                      pred_mem_init="mean")),
    ("lstm_bi_h64", dict(hid_dim=64, rep_rnn_bidirectional=True)),
    ("gru_uni_h64", dict(hid_dim=64, rep_rnn_type="GRU")),
]


def _perturb(model):
    """Nonzero RNN biases (the padding drift) and a livelier head, after sd_init is recorded."""
    with th.no_grad():
        for k, p in model.named_parameters():
            if "_rep_net.rnn." in k and ".bias_" in k:
                p.uniform_(-0.3, 0.3)
        head = model.pred_net
        head.pred_fc2.weight.uniform_(-0.3, 0.3)
        head.pred_fc2.bias.uniform_(-0.1, 0.1)
        if getattr(head, "weight_fc2", None) is not None:
            head.weight_fc2.weight.uniform_(-0.3, 0.3)
            head.weight_fc2.bias.uniform_(-0.1, 0.1)


def gen_models():
    from models.rnn import RNN
    for tag, extra in MODEL_CASES:
        config = base_config(**extra)
        rng = np.random.default_rng(MG.seed_of("rnn-model", tag) % (2 ** 32))
        th.manual_seed(MG.seed_of("rnn-model", tag))
        ps, gs, P, G = ES.model_batch(rng, config, empty_graph=True)
        model = RNN(**config)
        sd_init = {k: v.clone() for k, v in model.state_dict().items()}
        _perturb(model)
        d = {"config_keys": np.array(sorted(config.keys())), "config_vals": np.array([repr(config[k]) for k in sorted(config.keys())]),
             "seed": MG.seed_of("rnn-model", tag)}
        for i, (p, g) in enumerate(zip(ps, gs)):
            ES.put_graph(d, "p%d" % i, p)
            ES.put_graph(d, "g%d" % i, g)
        d["num"] = len(ps)
        for t, s in (("p", P), ("g", G)):
            for k, v in s.tdata.items():
                d["%s.%s" % (t, k)] = v
            d[t + ".lens"] = s.batch_num_tuples()
        for k, v in sd_init.items():
            d["sd_init." + k] = v
        for k, v in model.state_dict().items():
            if not th.equal(v, sd_init[k]):
                d["sd." + k] = v.clone()
        out = model(P, G)
        total = out["pred_c"].sum()
        if out["pred_e"] is not None:
            total = total + (out["pred_e"] * th.linspace(-1, 1, out["pred_e"].numel()).view_as(out["pred_e"])).sum()
        total = total + (out["g_e_rep"] ** 2).sum() * 1e-3
        total.backward()
        for k, prm in model.named_parameters():
            if prm.grad is not None:
                d["grad." + k] = prm.grad
        for k, v in out.items():
            if v is not None:
                d["out." + k] = v
        save("model_" + tag, d)


def gen_expand():
    from models.rnn import RNN
    th.manual_seed(MG.seed_of("rnn-expand"))
    config = base_config(hid_dim=8, pred_hid_dim=8, share_emb_net=False, share_enc_net=False, pred_with_enc=True,
                         rep_num_graph_layers=1, rep_num_pattern_layers=1)
    grow = dict(max_ngv=40, max_ngvl=9, max_nge=80, max_ngel=20, max_npv=8, max_npvl=7, max_npe=20, max_npel=3)
    model = RNN(**config)
    d = {"config_keys": np.array(sorted(config.keys())), "config_vals": np.array([repr(config[k]) for k in sorted(config.keys())]),
         "grow_keys": np.array(sorted(grow.keys())), "grow_vals": np.array([grow[k] for k in sorted(grow.keys())]),
         "seed": MG.seed_of("rnn-expand"), "seed_grow": MG.seed_of("rnn-expand", "grow")}
    for k, v in model.state_dict().items():
        d["sd." + k] = v.clone()
    th.manual_seed(MG.seed_of("rnn-expand", "grow"))
    model.expand(**dict(config, **grow))
    for k, v in model.state_dict().items():
        d["sd_after." + k] = v.clone()
    save("expand_rnn", d)


GENERATORS = ["models", "expand"]


def main():
    os.makedirs(OUT, exist_ok=True)
    import ref_standin
    ref_standin.import_scm()
    for name in sys.argv[1:] or GENERATORS:
        globals()["gen_" + name]()


if __name__ == "__main__":
    main()
