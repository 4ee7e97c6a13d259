"""Emit the attention-head fixtures under tests/golden/attn/ by running the REFERENCE's own code.

Runs only in the development container (needs the reference checkout): the reference's ``models/pred.py`` and models are
imported over the DGL / numba / igraph stand-ins of ``oracle/ref_standin.py`` (read-only use of ``oracle/``), single
threaded with deterministic algorithms, as ``oracle/make_golden.py`` runs.  Outputs are data only: inputs, parameters,
expected outputs and gradients.

    python scripts/make_golden_attn.py          # writes tests/golden/attn/*.npz  (DMP_GOLDEN_ATTN_OUT: elsewhere)

Fixtures
  sparsemax_*.npz   masked fill (-1e30) + Sparsemax(dim=2) over [B, Lq, Lk, nh] scores (utils/act.py:255-316): output and the
                    autograd gradient of a random upstream gradient
  dotattn_*.npz     gated sparsemax DotAttention (pred.py:240-487): output, input and parameter gradients
  head_*.npz        Sum / Mean / Max AttnPredictNet standalone (pred.py:490-643): count, row weights, gradients
  model_*.npz       DMPNN (GraphAdjModelV2, add_rev, node + edge heads) with SumAttnPredictNet, RGIN (GraphAdjModel) with
                    MaxAttnPredictNet: the 15 OutputDict entries, parameter gradients, the seeded state_dict after construction
  expand_*.npz      BaseModel.expand() of the DMPNN model with an attention head (pred_with_enc: the head grows)
"""
import os
import sys

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("DMP_GOLDEN_ATTN_OUT") or os.path.join(ROOT, "tests", "golden", "attn")
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import make_golden as MG   # noqa: E402  (its helpers; importing it sets one thread and deterministic algorithms)

th.set_num_threads(1)
th.use_deterministic_algorithms(True)
NEG = -1e30     # the reference's _INF (constants.py:6)


def save(name, d):
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **MG.t2n(d))
    print("wrote", name + ".npz")


def prefix_mask(lens, L):
    """pre_pad masks (utils/dl.py:113-127): the last len positions of every row are live."""
    return th.arange(L).unsqueeze(0) >= (L - th.as_tensor(lens)).unsqueeze(1)


def gen_sparsemax():
    from utils.act import Sparsemax
    cases = {
        # masked keys (non-prefix), one all-masked row, equal scores inside the support
        "mixed": (3, 5, 7, 2),
        "wide": (2, 3, 33, 4),
        "lk1": (2, 4, 1, 3),
    }
    for tag, (B, Lq, Lk, nh) in cases.items():
        g = th.Generator().manual_seed(MG.seed_of("sparsemax", tag))
        x = (th.randn(B, Lq, Lk, nh, generator=g) * 1.5).double().float()
        kmask = th.rand(B, Lk, generator=g) > 0.3
        kmask[:, 0] = True
        if tag == "mixed":
            kmask[1] = False                                     # every key of pair 1 masked
            x[0, 1, 2, 0] = x[0, 1, 3, 0] = x[0, 1].max() + 0.3  # a tie at the top, inside the support (no key at the threshold)
            kmask[0, 2] = kmask[0, 3] = True
        if tag == "lk1":
            kmask[1, 0] = False
        x.requires_grad_(True)
        sm = Sparsemax(dim=2)
        y = sm(x.masked_fill(kmask.view(B, 1, Lk, 1) == 0, NEG))
        w = th.randn(y.shape, generator=g)
        (y * w).sum().backward()
        save("sparsemax_" + tag, {"x": x, "kmask": kmask, "y": y, "w": w, "dx": x.grad})


def gen_dotattn():
    from models.pred import DotAttention
    cases = [("cross_h1_d16", 1, 16, 6, 4), ("self_h4_d16", 4, 16, 9, 9), ("cross_h4_d32", 4, 32, 5, 11),
             ("self_h1_d64", 1, 64, 7, 7), ("cross_h4_d64", 4, 64, 3, 6)]
    B, D = 3, 24
    for tag, nh, dh, Lq, Lk in cases:
        th.manual_seed(MG.seed_of("dotattn", tag))
        hid = nh * dh
        attn = DotAttention(D, D, D, hid, num_heads=nh, scale=1 / (hid / nh) ** 0.5, score_func="sparsemax", add_gate=True)
        query = th.randn(B, Lq, D, requires_grad=True)
        if tag.startswith("self"):
            key = value = query
        else:
            key = th.randn(B, Lk, D, requires_grad=True)
            value = th.randn(B, Lk, D, requires_grad=True)
        qmask = th.rand(B, Lq) > 0.25
        kmask = th.rand(B, Lk) > 0.3
        kmask[:, -1] = True
        kmask[2] = False                         # pair 2: every key masked (uniform weights over the padding)
        if tag.startswith("self"):
            kmask = qmask.clone()
            kmask[2] = False
            kmask[:2, -1] = True
        qmask[0, 0] = False
        out = attn(query, key, value, query_mask=qmask, key_mask=kmask)
        w = th.randn(out.shape)
        (out * w).sum().backward()
        d = {"query": query, "qmask": qmask, "kmask": kmask, "out": out, "w": w, "dquery": query.grad,
             "nh": nh, "dh": dh, "self": tag.startswith("self")}
        if not tag.startswith("self"):
            d.update({"key": key, "value": value, "dkey": key.grad, "dvalue": value.grad})
        for k, p in attn.named_parameters():
            d["p." + k] = p
            d["g." + k] = p.grad
        save("dotattn_" + tag, d)


def gen_heads():
    from models.pred import MaxAttnPredictNet, MeanAttnPredictNet, SumAttnPredictNet
    B, D, hid, nh, Lp, Lg = 4, 12, 16, 4, 5, 9
    for name, cls in (("sum", SumAttnPredictNet), ("mean", MeanAttnPredictNet), ("max", MaxAttnPredictNet)):
        for rw in (False, True):
            for steps in (1, 3):
                tag = "%s_rw%d_s%d" % (name, int(rw), steps)
                th.manual_seed(MG.seed_of("head", tag))
                head = cls(D, hid, num_heads=nh, infer_steps=steps, act_func="relu", dropout=0.0, return_weights=rw)
                sd_init = {k: v.clone() for k, v in head.state_dict().items()}
                with th.no_grad():   # pred_fc2 / weight_fc2 are zero-initialised: make the outputs depend on their inputs
                    head.pred_fc2.weight.uniform_(-0.3, 0.3)
                    head.pred_fc2.bias.uniform_(-0.1, 0.1)
                    if rw:
                        head.weight_fc2.weight.uniform_(-0.3, 0.3)
                        head.weight_fc2.bias.uniform_(-0.1, 0.1)
                p_mask = prefix_mask([5, 3, 4, 1], Lp)
                g_mask = prefix_mask([9, 6, 2, 7], Lg)
                p_rep = (th.randn(B, Lp, D) * p_mask.unsqueeze(-1)).requires_grad_(True)
                g_rep = (th.randn(B, Lg, D) * g_mask.unsqueeze(-1)).requires_grad_(True)
                y, wts = head(p_rep, p_mask, g_rep, g_mask)
                loss = y.sum()
                ww = None
                if wts is not None:
                    ww = th.randn(wts.shape)
                    loss = loss + (wts * ww).sum()
                loss.backward()
                d = {"p_rep": p_rep, "p_mask": p_mask, "g_rep": g_rep, "g_mask": g_mask, "y": y, "weights": wts, "ww": ww,
                     "dp_rep": p_rep.grad, "dg_rep": g_rep.grad, "nh": nh, "steps": steps, "hid": hid, "rw": rw}
                for k, v in sd_init.items():
                    d["sd_init." + k] = v
                for k, v in head.state_dict().items():
                    d["sd." + k] = v
                for k, p in head.named_parameters():
                    d["g." + k] = p.grad
                save("head_" + tag, d)


def _dmpnn_config():
    return dict(max_ngv=64, max_ngvl=16, max_nge=512, max_ngel=32, max_npv=8, max_npvl=8, max_npe=24, max_npel=16, base=2,
                hid_dim=16, share_emb_net=True, share_enc_net=True, share_rep_net=True, rep_residual=True, enc_net="Multihot",
                emb_net="Orthogonal", filter_net="ScalarFilter", rep_net="DMPNN", rep_num_graph_layers=2,
                rep_num_pattern_layers=2, rep_dmpnn_num_mlp_layers=2, rep_dmpnn_batch_norm=False, rep_act_func="relu",
                rep_dropout=0.0, init_neigenv=6.0, init_eeigenv=5.0, pred_net="SumAttnPredictNet", pred_hid_dim=16,
                pred_act_func="relu", pred_dropout=0.0, pred_num_heads=4, pred_infer_steps=2, node_pred=True, edge_pred=True,
                pred_return_weights="node,edge")


def _record(model, config, pattern, graph, sd_init, fields):
    d = {"config_keys": np.array(sorted(config.keys())), "config_vals": np.array([repr(config[k]) for k in sorted(config.keys())])}
    for k, v in sd_init.items():
        d["sd_init." + k] = v
    for k, v in model.state_dict().items():
        d["sd." + k] = v.clone()
    out = model(pattern, graph)
    total = out["pred_c"].sum()
    for k in ("pred_v", "pred_e"):
        if out[k] is not None:
            total = total + out[k].sum()
    total.backward()
    for t, g in (("p", pattern), ("g", graph)):
        d.update({t + "_src": g._u, t + "_dst": g._v, t + "_num_nodes": g.number_of_nodes(),
                  t + "_bnn": g.batch_num_nodes(), t + "_bne": g.batch_num_edges()})
        for k in fields[0]:
            d["%s_ndata.%s" % (t, k)] = g.ndata[k]
        for k in fields[1]:
            d["%s_edata.%s" % (t, k)] = g.edata[k]
    for k, p in model.named_parameters():
        if p.grad is not None:
            d["grad." + k] = p.grad
    for k, v in out.items():
        if v is not None:
            d["out." + k] = v
    return d


def _perturb_heads(heads):
    with th.no_grad():   # pred_fc2 / weight_fc2 are zero-initialised: make the head's output depend on its input
        for head in heads:
            head.pred_fc2.weight.uniform_(-0.3, 0.3)
            head.pred_fc2.bias.uniform_(-0.1, 0.1)
            if head.weight_fc2 is not None:
                head.weight_fc2.weight.uniform_(-0.3, 0.3)
                head.weight_fc2.bias.uniform_(-0.1, 0.1)


def gen_models():
    import dgl
    from models.dmpnn import DMPNN
    from models.rgin import RGIN
    ragged_p = [(3, 3), (5, 9), (4, 6), (8, 12), (2, 1), (6, 10)]
    ragged_g = [(10, 30), (16, 50), (7, 12), (20, 64), (5, 8), (12, 40)]

    def batch_rev(sizes, n_vl, n_el, rng):
        gs = []
        for n, m in sizes:
            u, v = MG.er_edges(n, m, rng)
            e = len(u)
            uu, vv, rev = MG.with_rev(u, v)
            g = dgl.DGLGraph.from_edges(uu, vv, n)
            el = rng.integers(0, n_el, size=e)
            g.ndata["id"] = th.arange(n)
            g.ndata["label"] = th.from_numpy(rng.integers(0, n_vl, size=n))
            g.edata["id"] = th.cat([th.arange(e), th.arange(e) + max(m for _, m in sizes)])
            g.edata["label"] = th.from_numpy(np.concatenate([el, el + n_el]))
            g.edata["is_reversed"] = th.from_numpy(rev)
            gs.append(g)
        return dgl.batch(gs)

    rng = np.random.default_rng(51)
    th.manual_seed(MG.seed_of("attn-model", "dmpnn"))
    config = _dmpnn_config()
    pattern, graph = batch_rev(ragged_p, 8, 8, rng), batch_rev(ragged_g, 16, 16, rng)
    model = DMPNN(**config)
    sd_init = {k: v.clone() for k, v in model.state_dict().items()}
    _perturb_heads(model.pred_net.values())
    save("model_dmpnn_sumattn", _record(model, config, pattern, graph, sd_init,
                                        (("id", "label"), ("id", "label", "is_reversed"))))

    def batch_plain(sizes, n_vl, n_el, rng):
        gs = []
        for n, m in sizes:
            u, v = MG.er_edges(n, m, rng)
            g = dgl.DGLGraph.from_edges(u, v, n)
            g.ndata["id"] = th.arange(n)
            g.ndata["label"] = th.from_numpy(rng.integers(0, n_vl, size=n))
            g.edata["id"] = th.arange(m)
            g.edata["label"] = th.from_numpy(rng.integers(0, n_el, size=m))
            gs.append(g)
        return dgl.batch(gs)

    rng = np.random.default_rng(52)
    th.manual_seed(MG.seed_of("attn-model", "rgin"))
    pattern, graph = batch_plain(ragged_p, 4, 3, rng), batch_plain(ragged_g, 6, 5, rng)
    config = dict(max_ngv=20, max_ngvl=6, max_nge=64, max_ngel=5, max_npv=8, max_npvl=4, max_npe=12, max_npel=3, base=2, hid_dim=16,
                  share_emb_net=False, share_enc_net=False, share_rep_net=False, rep_residual=True, enc_net="Multihot",
                  emb_net="Orthogonal", filter_net="ScalarFilter", rep_num_graph_layers=2, rep_num_pattern_layers=2,
                  rep_act_func="relu", rep_dropout=0.0, rep_net="RGIN", rep_rgin_num_bases=2, pred_net="MaxAttnPredictNet",
                  pred_hid_dim=16, pred_act_func="relu", pred_dropout=0.0, pred_num_heads=4, pred_infer_steps=3)
    model = RGIN(**config)
    sd_init = {k: v.clone() for k, v in model.state_dict().items()}
    _perturb_heads([model.pred_net])
    save("model_rgin_maxattn", _record(model, config, pattern, graph, sd_init, (("id", "label"), ("id", "label"))))


def gen_expand():
    from models.dmpnn import DMPNN
    th.manual_seed(MG.seed_of("attn-expand"))
    config = dict(max_ngv=16, max_ngvl=4, max_nge=40, max_ngel=6, max_npv=4, max_npvl=4, max_npe=8, max_npel=6, base=2, hid_dim=8,
                  share_emb_net=False, share_enc_net=False, share_rep_net=True, rep_residual=True, enc_net="Multihot",
                  emb_net="Orthogonal", filter_net="ScalarFilter", rep_net="DMPNN", rep_num_graph_layers=1,
                  rep_num_pattern_layers=1, rep_dmpnn_batch_norm=False, pred_net="SumAttnPredictNet", pred_hid_dim=8,
                  pred_num_heads=2, pred_infer_steps=1, pred_with_enc=True, node_pred=True, edge_pred=True)
    grow = dict(max_ngv=40, max_ngvl=9, max_nge=40, max_ngel=20, max_npv=4, max_npvl=5, max_npe=20, max_npel=3)
    model = DMPNN(**config)
    d = {"config_keys": np.array(sorted(config.keys())), "config_vals": np.array([repr(config[k]) for k in sorted(config.keys())]),
         "grow_keys": np.array(sorted(grow.keys())), "grow_vals": np.array([grow[k] for k in sorted(grow.keys())])}
    for k, v in model.state_dict().items():
        d["sd." + k] = v.clone()
    th.manual_seed(MG.seed_of("attn-expand", "grow"))
    model.expand(**dict(config, **grow))
    for k, v in model.state_dict().items():
        d["sd_after." + k] = v.clone()
    save("expand_dmpnn_sumattn", d)


GENERATORS = ["sparsemax", "dotattn", "heads", "models", "expand"]


def main():
    os.makedirs(OUT, exist_ok=True)
    import ref_standin
    ref_standin.import_scm()
    for name in sys.argv[1:] or GENERATORS:
        globals()["gen_" + name]()


if __name__ == "__main__":
    main()
