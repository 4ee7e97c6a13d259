"""Emit the memory-head fixtures under tests/golden/mem/ by running the REFERENCE's own code.

Runs only in the development container (needs the reference checkout): the reference's ``models/pred.py`` and models are
imported over the DGL / numba / igraph stand-ins of ``oracle/ref_standin.py`` (read-only use of ``oracle/``), single
threaded with deterministic algorithms, as ``oracle/make_golden.py`` runs.  Outputs are data only: inputs, parameters,
expected outputs and gradients.

    python scripts/make_golden_mem.py          # writes tests/golden/mem/*.npz  (DMP_GOLDEN_MEM_OUT: elsewhere)

Fixtures
  initmem_*.npz   MemDotAttention.init_memory ("memattn.*") and DIAMNet.init_memory ("diam.*", mem_layer taken out: the
                  pooling alone) on the same rows for every mean / sum / max (and circular_) mem_init at mem_len 1 and 4:
                  memory, memory mask, input gradient of a random upstream gradient.  Masks: front padding, interior
                  holes, a masked last position, an all-masked pair; "mixed" has pairs with different starts and ends (DIAMNet's per-pair branch), "start0" equal starts
                  (its length buckets)
  memattn_*.npz   MemDotAttention forward and backward (pre_lnorm, gate, sparsemax, scale 1)
  head_*.npz      Sum / Mean / Max MemAttnPredictNet and DIAMNet standalone: count, row weights, gradients, seeded init
  model_*.npz     DMPNN (GraphAdjModelV2, add_rev, node + edge heads) with DIAMNet, RGIN (GraphAdjModel) with
                  MaxMemAttnPredictNet: the 15 OutputDict entries, parameter gradients, the seeded state_dict
  expand_*.npz    BaseModel.expand() of the DMPNN model with DIAMNet (pred_with_enc: the head grows)
"""
import os
import sys

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("DMP_GOLDEN_MEM_OUT") or os.path.join(ROOT, "tests", "golden", "mem")
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import make_golden as MG   # noqa: E402  (its helpers; importing it sets one thread and deterministic algorithms)

th.set_num_threads(1)
th.use_deterministic_algorithms(True)
MODES = ["mean", "sum", "max", "circular_mean", "circular_sum", "circular_max"]


def save(name, d):
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **MG.t2n(d))
    print("wrote", name + ".npz")


def seg_mask(L, s, e, holes=()):
    """Live from s to e (inclusive) except the interior holes; nothing live when s > e."""
    m = th.zeros(L, dtype=th.bool)
    if s <= e:
        m[s:e + 1] = True
        for h in holes:
            m[h] = False
    return m


def mem_masks(M, L):
    """[B, L] masks whose segments (e - s for the memory-attention heads, e - s + 1 for DIAMNet) cover the lengths 0, 1,
    M-1, M, M+1, 2M+1 and about 40, with front padding, interior holes and masked last positions."""
    spans = [0, 1, max(M - 1, 0), M, M + 1, 2 * M + 1, 40]
    mixed, start0 = [th.zeros(L, dtype=th.bool)], []
    for i, n in enumerate(spans):
        s = 1 + i % 3                                             # front padding
        e = s + n
        holes = [s + 1 + j for j in range(0, n - 1, 3)][:4]       # interior holes (reversed edges)
        mixed.append(seg_mask(L, s, e, holes))
        start0.append(seg_mask(L, 0, n, holes[1:]))
    mixed.append(seg_mask(L, 2, 2))                                # one live position
    return th.stack(mixed), th.stack(start0)


def gen_initmem():
    from models.pred import DIAMNet, MemDotAttention
    L, D = 48, 4
    for M in (1, 4):
        for kind, mask in zip(("mixed", "start0"), mem_masks(M, L)):
            for mode in MODES:
                tag = "%s_m%d_%s" % (mode, M, kind)
                th.manual_seed(MG.seed_of("initmem", tag))
                x = th.randn(mask.size(0), L, D)
                d = {"x": x, "mask": mask, "M": M, "mode": mode}
                for cls in ("memattn", "diam"):
                    if cls == "memattn":
                        net = MemDotAttention(D, D, D, D, D, num_heads=1, mem_len=M, mem_init=mode, score_func="sparsemax",
                                              add_gate=True, pre_lnorm=True)
                    else:
                        net = DIAMNet(D, D, num_heads=1, mem_len=M, mem_init=mode)
                        net.mem_layer = th.nn.Identity()          # the pooling alone
                    xg = x.clone().requires_grad_(True)
                    mem, mmask = net.init_memory(xg, mask)
                    w = th.randn(mem.shape)
                    (mem * w).sum().backward()
                    d.update({cls + ".mem": mem, cls + ".mem_mask": mmask.bool(), cls + ".w": w, cls + ".dx": xg.grad})
                save("initmem_" + tag, d)


def gen_memattn():
    from models.pred import MemDotAttention
    cases = [("h1_m1_mean", 1, 1, "mean"), ("h4_m4_sum", 4, 4, "sum"), ("h4_m4_max", 4, 4, "max"), ("h1_m4_cmean", 1, 4, "circular_mean")]
    B, Dq, Dk, hid, Lq, Lk = 4, 12, 20, 16, 6, 15
    for tag, nh, M, mode in cases:
        th.manual_seed(MG.seed_of("memattn", tag))
        attn = MemDotAttention(Dq, Dk, Dk, hid, hid, num_heads=nh, scale=1, mem_len=M, mem_init=mode, score_func="sparsemax",
                               add_gate=True, pre_lnorm=True)
        query = th.randn(B, Lq, Dq, requires_grad=True)
        key = th.randn(B, Lk, Dk, requires_grad=True)
        value = th.randn(B, Lk, Dk, requires_grad=True)
        qmask = th.rand(B, Lq) > 0.2
        kmask = th.stack([seg_mask(Lk, 2, 13, (5, 6)), seg_mask(Lk, 0, 14), seg_mask(Lk, 4, 7), seg_mask(Lk, 1, 10, (3,))])
        out = attn(query, key, value, query_mask=qmask, key_mask=kmask)
        w = th.randn(out.shape)
        (out * w).sum().backward()
        d = {"query": query, "key": key, "value": value, "qmask": qmask, "kmask": kmask, "out": out, "w": w, "dquery": query.grad,
             "dkey": key.grad, "dvalue": value.grad, "nh": nh, "M": M, "mode": mode, "dq": Dq, "dk": Dk, "hid": hid}
        for k, p in attn.named_parameters():
            d["p." + k] = p
            d["g." + k] = p.grad
        save("memattn_" + tag, d)


def head_cases():
    """(tag, class name, num_heads, infer_steps, return_weights, mem_len, mem_init or None)."""
    out = []
    for name in ("sum", "mean", "max", "diam"):
        for rw in (False, True):
            for steps in (1, 3):
                out.append(("%s_h4_rw%d_s%d" % (name, int(rw), steps), name, 4, steps, rw, 4, None))
        if name in ("sum", "diam"):
            out.append(("%s_h1_rw1_s1" % name, name, 1, 1, True, 4, None))
    out.append(("diam_h4_rw0_s1_m2_cmax", "diam", 4, 1, False, 2, "circular_max"))
    out.append(("diam_h1_rw0_s3_m3_sum", "diam", 1, 3, False, 3, "sum"))
    return out


def gen_heads():
    from models import pred
    classes = {"sum": pred.SumMemAttnPredictNet, "mean": pred.MeanMemAttnPredictNet, "max": pred.MaxMemAttnPredictNet,
               "diam": pred.DIAMNet}
    B, D, hid, Lp, Lg = 4, 12, 16, 6, 13
    for tag, name, nh, steps, rw, M, mem_init in head_cases():
        th.manual_seed(MG.seed_of("memhead", tag))
        kw = dict(num_heads=nh, infer_steps=steps, mem_len=M, act_func="relu", dropout=0.0, return_weights=rw)
        if mem_init is not None:
            kw["mem_init"] = mem_init
        head = classes[name](D, hid, **kw)
        sd_init = {k: v.clone() for k, v in head.state_dict().items()}
        with th.no_grad():   # pred_fc2 / weight_fc2 are zero-initialised: make the outputs depend on their inputs
            head.pred_fc2.weight.uniform_(-0.3, 0.3)
            head.pred_fc2.bias.uniform_(-0.1, 0.1)
            if rw:
                head.weight_fc2.weight.uniform_(-0.3, 0.3)
                head.weight_fc2.bias.uniform_(-0.1, 0.1)
        p_mask = th.stack([seg_mask(Lp, 0, 5), seg_mask(Lp, 2, 5), seg_mask(Lp, 1, 4, (2,)), seg_mask(Lp, 3, 5)])
        g_mask = th.stack([seg_mask(Lg, 0, 12, (3, 7)), seg_mask(Lg, 4, 12), seg_mask(Lg, 2, 9, (5,)), seg_mask(Lg, 10, 12)])
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
             "dp_rep": p_rep.grad, "dg_rep": g_rep.grad, "cls": type(head).__name__, "nh": nh, "steps": steps, "hid": hid,
             "rw": rw, "M": M, "mem_init": mem_init or ""}
        for k, v in sd_init.items():
            d["sd_init." + k] = v
        for k in ("pred_fc2.weight", "pred_fc2.bias", "weight_fc2.weight", "weight_fc2.bias"):
            if k in sd_init:
                d["sd." + k] = head.state_dict()[k]
        for k, p in head.named_parameters():
            d["g." + k] = p.grad
        save("head_" + tag, d)


def _record(model, config, pattern, graph, sd_init, fields):
    d = {"config_keys": np.array(sorted(config.keys())), "config_vals": np.array([repr(config[k]) for k in sorted(config.keys())])}
    for k, v in sd_init.items():
        d["sd_init." + k] = v
    for k, v in model.state_dict().items():
        if not th.equal(v, sd_init[k]):
            d["sd." + k] = v.clone()                               # the perturbed entries (the rest is sd_init)
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


def _dmpnn_config():
    return dict(max_ngv=64, max_ngvl=16, max_nge=512, max_ngel=32, max_npv=8, max_npvl=8, max_npe=24, max_npel=16, base=2,
                hid_dim=16, share_emb_net=True, share_enc_net=True, share_rep_net=True, rep_residual=True, enc_net="Multihot",
                emb_net="Orthogonal", filter_net="ScalarFilter", rep_net="DMPNN", rep_num_graph_layers=2,
                rep_num_pattern_layers=2, rep_dmpnn_num_mlp_layers=2, rep_dmpnn_batch_norm=False, rep_act_func="relu",
                rep_dropout=0.0, init_neigenv=6.0, init_eeigenv=5.0, pred_net="DIAMNet", pred_hid_dim=16,
                pred_act_func="relu", pred_dropout=0.0, pred_num_heads=4, pred_infer_steps=2, pred_mem_len=4,
                pred_mem_init="mean", node_pred=True, edge_pred=True, pred_return_weights="node,edge")


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

    rng = np.random.default_rng(61)
    th.manual_seed(MG.seed_of("mem-model", "dmpnn"))
    config = _dmpnn_config()
    pattern, graph = batch_rev(ragged_p, 8, 8, rng), batch_rev(ragged_g, 16, 16, rng)
    model = DMPNN(**config)
    sd_init = {k: v.clone() for k, v in model.state_dict().items()}
    _perturb_heads(model.pred_net.values())
    save("model_dmpnn_diamnet", _record(model, config, pattern, graph, sd_init,
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

    rng = np.random.default_rng(62)
    th.manual_seed(MG.seed_of("mem-model", "rgin"))
    pattern, graph = batch_plain(ragged_p, 4, 3, rng), batch_plain(ragged_g, 6, 5, rng)
    config = dict(max_ngv=20, max_ngvl=6, max_nge=64, max_ngel=5, max_npv=8, max_npvl=4, max_npe=12, max_npel=3, base=2, hid_dim=16,
                  share_emb_net=False, share_enc_net=False, share_rep_net=False, rep_residual=True, enc_net="Multihot",
                  emb_net="Orthogonal", filter_net="ScalarFilter", rep_num_graph_layers=2, rep_num_pattern_layers=2,
                  rep_act_func="relu", rep_dropout=0.0, rep_net="RGIN", rep_rgin_num_bases=2, pred_net="MaxMemAttnPredictNet",
                  pred_hid_dim=16, pred_act_func="relu", pred_dropout=0.0, pred_num_heads=4, pred_infer_steps=3, pred_mem_len=4)
    model = RGIN(**config)
    sd_init = {k: v.clone() for k, v in model.state_dict().items()}
    _perturb_heads([model.pred_net])
    save("model_rgin_maxmemattn", _record(model, config, pattern, graph, sd_init, (("id", "label"), ("id", "label"))))


def gen_expand():
    from models.dmpnn import DMPNN
    th.manual_seed(MG.seed_of("mem-expand"))
    config = dict(max_ngv=16, max_ngvl=4, max_nge=40, max_ngel=6, max_npv=4, max_npvl=4, max_npe=8, max_npel=6, base=2, hid_dim=8,
                  share_emb_net=False, share_enc_net=False, share_rep_net=True, rep_residual=True, enc_net="Multihot",
                  emb_net="Orthogonal", filter_net="ScalarFilter", rep_net="DMPNN", rep_num_graph_layers=1,
                  rep_num_pattern_layers=1, rep_dmpnn_batch_norm=False, pred_net="DIAMNet", pred_hid_dim=8,
                  pred_num_heads=2, pred_infer_steps=1, pred_mem_len=4, pred_with_enc=True, node_pred=True, edge_pred=True)
    grow = dict(max_ngv=40, max_ngvl=9, max_nge=40, max_ngel=20, max_npv=4, max_npvl=5, max_npe=20, max_npel=3)
    model = DMPNN(**config)
    d = {"config_keys": np.array(sorted(config.keys())), "config_vals": np.array([repr(config[k]) for k in sorted(config.keys())]),
         "grow_keys": np.array(sorted(grow.keys())), "grow_vals": np.array([grow[k] for k in sorted(grow.keys())])}
    for k, v in model.state_dict().items():
        d["sd." + k] = v.clone()
    th.manual_seed(MG.seed_of("mem-expand", "grow"))
    model.expand(**dict(config, **grow))
    for k, v in model.state_dict().items():
        d["sd_after." + k] = v.clone()
    save("expand_dmpnn_diamnet", d)


GENERATORS = ["initmem", "memattn", "heads", "models", "expand"]


def main():
    os.makedirs(OUT, exist_ok=True)
    import ref_standin
    ref_standin.import_scm()
    for name in sys.argv[1:] or GENERATORS:
        globals()["gen_" + name]()


if __name__ == "__main__":
    main()
