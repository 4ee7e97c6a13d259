"""Emit the TXL rep-net fixtures under tests/golden/txl/ by running the REFERENCE's own ``models/txl.py``.

Runs only in the development container (needs the reference checkout), over the DGL / numba / igraph stand-ins of
``oracle/ref_standin.py`` (read-only use of ``oracle/``), single threaded with deterministic algorithms, as
``scripts/make_golden_rnn.py`` runs (the helpers of ``make_golden`` / ``make_golden_edgeseq`` are reused unchanged).
Outputs are data only: inputs, parameters, expected outputs and gradients.

    python scripts/make_golden_txl.py      # writes tests/golden/txl/*.npz  (DMP_GOLDEN_TXL_OUT: elsewhere)

The reference's TXL does not run under a current torch as it stands: ``MixtureDict.__setitem__`` (models/container.py) hands
``r_w_bias`` / ``r_r_bias`` to ``ParameterDict.register_parameter``, which no longer enters the key into the dictionary, so
``net["r_w_bias"]`` raises ``KeyError`` and ``len(net)`` is 1 instead of 3.  ``_restore_mixture_dict`` below assigns, at run
time, a ``__setitem__`` that stores parameters as ``self._param_dict[key] = value`` (buffers and modules go where they
went): the behaviour of the torch the reference was written for.  Nothing of the reference is changed on disk.

Fixtures (hid_dim 16 unless named; every batch is ragged and pre-padded, with an empty graph and ScalarFilter holes; after
``sd_init`` is recorded the LayerNorm affine parameters, ``o_net.bias`` and the head are perturbed, so nothing sits at an
identity)
  model_default(_h64)   no TXL keyword: seg 64, mem 64, 1 head, post-norm; ext_len 0, so the memory regime.  Target
                        sequences longer than 128 tuples and no multiple of 64: three segments (klen 64, 128, 128), and the
                        data / mask offset of the padding
  model_seg8(_h64)      seg_len=8, mem_len=8, num_heads=4: ext_len = seg_len, the memory stays empty, many segments
  model_seg8_pre        the same with num_heads=2, pre_lnorm=True
  model_sep             share_rep_net=False with 2 pattern layers (``pattern_txl_(i)`` keys)
  model_clamp           clamp_len=5
  model_diam            a DIAMNet head
  expand_txl.npz        BaseModel.expand() of a TXL with pred_with_enc
"""
import os
import sys

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("DMP_GOLDEN_TXL_OUT") or os.path.join(ROOT, "tests", "golden", "txl")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import make_golden as MG            # noqa: E402  (its helpers; importing it sets one thread and deterministic algorithms)
import make_golden_edgeseq as ES    # noqa: E402  (rand_graph, ref_seq, ref_rev, model_batch, put_graph)

th.set_num_threads(1)
th.use_deterministic_algorithms(True)


def _restore_mixture_dict():
    import torch.nn as nn
    import models.container as C

    def setitem(self, key, value):
        if isinstance(value, nn.Parameter):
            self._param_dict[key] = value
        elif isinstance(value, th.Tensor):
            self._buffer_dict.register_buffer(key, value)
        else:
            self._module_dict.add_module(key, value)
    C.MixtureDict.__setitem__ = setitem


def save(name, d):
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **MG.t2n(d))
    print("wrote", name + ".npz")


def base_config(**kw):
    c = dict(max_ngv=24, max_ngvl=6, max_nge=256, max_ngel=8, max_npv=8, max_npvl=6, max_npe=16, max_npel=8, base=2, hid_dim=16,
             share_emb_net=True, share_enc_net=True, share_rep_net=True, rep_residual=True, enc_net="Multihot",
             emb_net="Orthogonal", filter_net="ScalarFilter", rep_net="TXL", rep_num_graph_layers=3, rep_num_pattern_layers=3,
             rep_act_func="relu", rep_dropout=0.0, pred_net="SumPredictNet", pred_hid_dim=16, pred_act_func="relu",
             pred_dropout=0.0, pred_return_weights="edge", add_rev=True)
    c.update(kw)
    return c


SEG8 = dict(seg_len=8, mem_len=8, num_heads=4)
MODEL_CASES = [                         # (tag, long target sequences, configuration)
    ("default", True, dict()),
    ("default_h64", True, dict(hid_dim=64, rep_num_graph_layers=2, rep_num_pattern_layers=2)),
    ("seg8", False, dict(SEG8)),
    ("seg8_h64", False, dict(SEG8, hid_dim=64, rep_num_graph_layers=2, rep_num_pattern_layers=2)),
    ("seg8_pre", False, dict(SEG8, num_heads=2, pre_lnorm=True)),
    ("sep", False, dict(SEG8, share_rep_net=False, rep_num_pattern_layers=2, pred_with_enc=True, pred_with_deg=True)),
    ("clamp", True, dict(clamp_len=5, rep_num_graph_layers=2, rep_num_pattern_layers=2)),
    ("diam", False, dict(SEG8, pred_net="DIAMNet", pred_num_heads=4, pred_infer_steps=1, pred_mem_len=4, pred_mem_init="mean")),
]


def long_batch(rng, config):
    """As ES.model_batch with an empty graph, but the longest target sequence has more than 128 tuples (and no multiple of
    64): the default TXL then runs three segments, the last two with a full memory."""
    import dataset
    p_sizes = [(3, 3), (4, 5), (2, 1), (5, 7)]
    g_sizes = [(12, 75), (10, 40), (6, 6), (0, 0)]
    ps = [ES.rand_graph(rng, n, m, 3, 3) for n, m in p_sizes]
    gs = [ES.rand_graph(rng, n, m, 3, 3) for n, m in g_sizes]
    rps, rgs = [], []
    for i, (p, g) in enumerate(zip(ps, gs)):
        x = {"id": "P%d-G%d" % (i, i), "pattern": ES.ref_seq(p), "graph": ES.ref_seq(g)}
        if config["add_rev"]:
            x = ES.ref_rev(x, config["max_npel"] // 2, config["max_ngel"] // 2)
        rps.append(x["pattern"])
        rgs.append(x["graph"])
    P = dataset.EdgeSeq.batch(rps, pre_pad=True)
    G = dataset.EdgeSeq.batch(rgs, pre_pad=True)
    L = G.u.size(1)
    assert L > 128 and L % 64 != 0, L
    return ps, gs, P, G


def _perturb(model):
    """LayerNorm affine parameters, o_net.bias and the head away from their initial identities / zeros."""
    with th.no_grad():
        for k, p in model.named_parameters():
            if "_rep_net." in k and ".layer_norm.weight" in k:
                p.uniform_(0.7, 1.3)
            elif "_rep_net." in k and (".layer_norm.bias" in k or ".o_net.bias" in k):
                p.uniform_(-0.2, 0.2)
        head = model.pred_net
        head.pred_fc2.weight.uniform_(-0.3, 0.3)
        head.pred_fc2.bias.uniform_(-0.1, 0.1)
        if getattr(head, "weight_fc2", None) is not None:
            head.weight_fc2.weight.uniform_(-0.3, 0.3)
            head.weight_fc2.bias.uniform_(-0.1, 0.1)


def gen_models():
    from models.txl import TransformerXL
    for tag, long_seq, extra in MODEL_CASES:
        config = base_config(**extra)
        rng = np.random.default_rng(MG.seed_of("txl-model", tag) % (2 ** 32))
        th.manual_seed(MG.seed_of("txl-model", tag))
        ps, gs, P, G = long_batch(rng, config) if long_seq else ES.model_batch(rng, config, empty_graph=True)
        model = TransformerXL(**config)
        sd_init = {k: v.clone() for k, v in model.state_dict().items()}
        _perturb(model)
        d = {"config_keys": np.array(sorted(config.keys())), "config_vals": np.array([repr(config[k]) for k in sorted(config.keys())]),
             "seed": MG.seed_of("txl-model", tag)}
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
    from models.txl import TransformerXL
    th.manual_seed(MG.seed_of("txl-expand"))
    config = base_config(hid_dim=8, pred_hid_dim=8, share_emb_net=False, share_enc_net=False, pred_with_enc=True,
                         rep_num_graph_layers=1, rep_num_pattern_layers=1, max_nge=64)
    grow = dict(max_ngv=40, max_ngvl=9, max_nge=80, max_ngel=20, max_npv=8, max_npvl=7, max_npe=20, max_npel=3)
    model = TransformerXL(**config)
    d = {"config_keys": np.array(sorted(config.keys())), "config_vals": np.array([repr(config[k]) for k in sorted(config.keys())]),
         "grow_keys": np.array(sorted(grow.keys())), "grow_vals": np.array([grow[k] for k in sorted(grow.keys())]),
         "seed": MG.seed_of("txl-expand"), "seed_grow": MG.seed_of("txl-expand", "grow")}
    for k, v in model.state_dict().items():
        d["sd." + k] = v.clone()
    th.manual_seed(MG.seed_of("txl-expand", "grow"))
    model.expand(**dict(config, **grow))
    for k, v in model.state_dict().items():
        d["sd_after." + k] = v.clone()
    save("expand_txl", d)


GENERATORS = ["models", "expand"]


def main():
    os.makedirs(OUT, exist_ok=True)
    import ref_standin
    ref_standin.import_scm()
    _restore_mixture_dict()
    for name in sys.argv[1:] or GENERATORS:
        globals()["gen_" + name]()


if __name__ == "__main__":
    main()
