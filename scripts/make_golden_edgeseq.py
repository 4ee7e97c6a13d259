"""Emit the edge-sequence / CNN fixtures under tests/golden/edgeseq/ by running the REFERENCE's own code.

Runs only in the development container (needs the reference checkout): the reference's ``dataset.EdgeSeq`` /
``EdgeSeqDataset`` and ``models/cnn.py`` are imported over the DGL / numba / igraph stand-ins of ``oracle/ref_standin.py``
(read-only use of ``oracle/``), single threaded with deterministic algorithms, as ``oracle/make_golden.py`` runs.  Outputs
are data only: inputs, parameters, expected outputs and gradients.

    python scripts/make_golden_edgeseq.py      # writes tests/golden/edgeseq/*.npz  (DMP_GOLDEN_EDGESEQ_OUT: elsewhere)

Fixtures
  seq_codes.npz     EdgeSeq.from_graph of graphs with multi-edges and of an empty graph; add_reversed_edges (codes and
                    is_reversed in the merged order); the pre-padded batch of them (tuples, lengths, batch_num_nodes,
                    in / out degrees)
  seq_weights.npz   calculate_edge_weights on the forward sequences, mapped through add_reversed_edges, and
                    calculate_edge_weights on the sequences with reversed tuples
  model_<tag>.npz   CNN (EdgeSeqModel) on a ragged batch: the 15 OutputDict entries, parameter gradients, the seeded
                    state_dict; refine_edge_weights of random weights with use_max both ways.  Tags: a (default k = 2,
                    3 layers, add_rev, edge weights), b (k = 3: the residual applies), c (rep_cnn_batch_norm), d (kernel
                    sizes [2, 3, 4], pred_with_enc + pred_with_deg, leaky_relu), e (DIAMNet), f (share_rep_net=False)
  expand_cnn.npz    BaseModel.expand() of a CNN with pred_with_enc
"""
import os
import sys

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("DMP_GOLDEN_EDGESEQ_OUT") or os.path.join(ROOT, "tests", "golden", "edgeseq")
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import make_golden as MG   # noqa: E402  (its helpers; importing it sets one thread and deterministic algorithms)

th.set_num_threads(1)
th.use_deterministic_algorithms(True)


def save(name, d):
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **MG.t2n(d))
    print("wrote", name + ".npz")


def rand_graph(rng, n, m, n_vl, n_el):
    """n nodes, m edges drawn with repetition (multi-edges, self-loops), random node ids (a permutation) and labels."""
    u = rng.integers(0, n, size=m) if n else np.zeros(0, np.int64)
    v = rng.integers(0, n, size=m) if n else np.zeros(0, np.int64)
    return {"src": u.astype(np.int64), "dst": v.astype(np.int64), "nid": rng.permutation(n).astype(np.int64),
            "nlabel": rng.integers(0, n_vl, size=n).astype(np.int64), "elabel": rng.integers(0, n_el, size=m).astype(np.int64),
            "n": n}


def ref_graph(g):
    import ref_standin

    class DGLGraph(ref_standin.DGLGraph):
        pass
    DGLGraph.__module__, DGLGraph.__qualname__ = "dgl.graph", "DGLGraph"   # the class name EdgeSeq.from_graph dispatches on
    x = DGLGraph.from_edges(th.from_numpy(g["src"]), th.from_numpy(g["dst"]), g["n"])
    x.ndata["id"], x.ndata["label"] = th.from_numpy(g["nid"]), th.from_numpy(g["nlabel"])
    x.edata["label"] = th.from_numpy(g["elabel"])
    return x


def put_graph(d, prefix, g):
    for k in ("src", "dst", "nid", "nlabel", "elabel"):
        d["%s.%s" % (prefix, k)] = g[k]
    d[prefix + ".n"] = g["n"]


def subisos(p, g):
    """Every injective, label-preserving map of p's nodes into g's under which each pattern edge (u, v, el) has a target
    edge (f(u), f(v), el): brute force over small graphs (input data of the weight fixtures)."""
    import itertools
    pe = set(zip(p["src"].tolist(), p["dst"].tolist(), p["elabel"].tolist()))
    ge = set(zip(g["src"].tolist(), g["dst"].tolist(), g["elabel"].tolist()))
    out = []
    for f in itertools.permutations(range(g["n"]), p["n"]):
        if all(p["nlabel"][i] == g["nlabel"][f[i]] for i in range(p["n"])) and all((f[a], f[b], e) in ge for a, b, e in pe):
            out.append(f)
    return np.array(out, np.int64).reshape(-1, p["n"])


def ref_seq(g):
    import dataset
    return dataset.EdgeSeq.from_graph(ref_graph(g))


def ref_rev(x, max_npel, max_ngel):
    import dataset
    return dataset.EdgeSeqDataset.add_reversed_edges(x, 0, max_npel, 0, max_ngel)


def gen_codes():
    import dataset
    rng = np.random.default_rng(71)
    graphs = [rand_graph(rng, 5, 12, 3, 2), rand_graph(rng, 0, 0, 3, 2), rand_graph(rng, 3, 9, 2, 2), rand_graph(rng, 7, 10, 3, 3),
              rand_graph(rng, 1, 2, 2, 2)]
    max_nel = 3
    d = {"num": len(graphs), "max_nel": max_nel}
    seqs, revs = [], []
    for i, g in enumerate(graphs):
        put_graph(d, "g%d" % i, g)
        s = ref_seq(g)
        d["code%d" % i] = th.stack([s.tdata[k] for k in ("u", "v", "ul", "el", "vl")], dim=-1).view(-1, 5)
        x = ref_rev({"id": "P-G%d" % i, "pattern": ref_seq(g), "graph": s}, max_nel, max_nel)
        r = x["graph"]
        d["rcode%d" % i] = th.stack([r.tdata[k] for k in ("u", "v", "ul", "el", "vl")], dim=-1).view(-1, 5)
        d["rflag%d" % i] = r.tdata["is_reversed"]
        seqs.append(ref_seq(g))
        revs.append(r)
    for tag, group in (("fwd", seqs), ("rev", revs)):
        b = dataset.EdgeSeq.batch([dataset.EdgeSeq(x) for x in group], pre_pad=True)
        for k, v in b.tdata.items():
            d["%s.%s" % (tag, k)] = v
        d[tag + ".lens"] = b.batch_num_tuples()
        d[tag + ".num_nodes"] = b.batch_num_nodes()
        d[tag + ".in_deg"] = b.in_degrees()
        d[tag + ".out_deg"] = b.out_degrees()
    save("seq_codes", d)


def gen_weights():
    import dataset
    rng = np.random.default_rng(72)
    d = {}
    pairs = []
    for i in range(4):
        while True:
            g = rand_graph(rng, 6, 14, 2, 2)
            p = {"src": np.array([0, 1, 1], np.int64), "dst": np.array([1, 2, 2], np.int64), "nid": np.arange(3),
                 "nlabel": rng.integers(0, 2, size=3), "elabel": rng.integers(0, 2, size=3), "n": 3}
            if i == 3:
                p["elabel"][2] = p["elabel"][1]                     # a repeated pattern tuple
            subs = subisos(p, g)
            if len(subs) or i == 2:
                break
        pairs.append((p, g, subs))
    max_npel = max_ngel = 2
    d["num"], d["max_npel"], d["max_ngel"] = len(pairs), max_npel, max_ngel
    for i, (p, g, subs) in enumerate(pairs):
        put_graph(d, "p%d" % i, p)
        put_graph(d, "g%d" % i, g)
        d["subs%d" % i] = subs
        x = {"id": "P%d-G%d" % (i, i), "pattern": ref_seq(p), "graph": ref_seq(g), "counts": len(subs),
             "subisomorphisms": th.from_numpy(subs)}
        d["w_fwd%d" % i] = dataset.EdgeSeqDataset.calculate_edge_weights(x)
        x["_edge_weights"] = d["w_fwd%d" % i]
        x = ref_rev(x, max_npel, max_ngel)
        d["w_mapped%d" % i] = x["_edge_weights"]
        del x["_edge_weights"]
        d["w_rev%d" % i] = dataset.EdgeSeqDataset.calculate_edge_weights(x)
    save("seq_weights", d)


def base_config(**kw):
    c = dict(max_ngv=24, max_ngvl=6, max_nge=64, max_ngel=8, max_npv=8, max_npvl=6, max_npe=16, max_npel=8, base=2, hid_dim=16,
             share_emb_net=True, share_enc_net=True, share_rep_net=True, rep_residual=True, enc_net="Multihot",
             emb_net="Orthogonal", filter_net="ScalarFilter", rep_net="CNN", rep_num_graph_layers=3, rep_num_pattern_layers=3,
             rep_act_func="relu", rep_dropout=0.0, rep_cnn_batch_norm=False, rep_cnn_kernel_sizes=2, rep_cnn_paddings=-1,
             rep_cnn_strides=1, pred_net="SumPredictNet", pred_hid_dim=16, pred_act_func="relu", pred_dropout=0.0,
             pred_return_weights="edge", add_rev=True)
    c.update(kw)
    return c


MODEL_CASES = [
    ("a", dict()),
    ("b", dict(rep_cnn_kernel_sizes=3)),
    ("c", dict(rep_cnn_batch_norm=True)),
    ("d", dict(rep_cnn_kernel_sizes=[2, 3, 4], pred_with_enc=True, pred_with_deg=True, rep_act_func="leaky_relu")),
    ("e", dict(pred_net="DIAMNet", pred_num_heads=4, pred_infer_steps=1, pred_mem_len=4, pred_mem_init="mean")),
    ("f", dict(share_rep_net=False, share_emb_net=False, share_enc_net=False, rep_num_pattern_layers=2)),
]


def model_batch(rng, config, empty_graph):
    import dataset
    p_sizes = [(3, 3), (4, 5), (2, 1), (5, 7)]
    g_sizes = [(8, 14), (12, 20), (6, 6), (0, 0) if empty_graph else (9, 11)]
    ps = [rand_graph(rng, n, m, 3, 3) for n, m in p_sizes]
    gs = [rand_graph(rng, n, m, 3, 3) for n, m in g_sizes]
    rps, rgs = [], []
    for i, (p, g) in enumerate(zip(ps, gs)):
        x = {"id": "P%d-G%d" % (i, i), "pattern": ref_seq(p), "graph": ref_seq(g)}
        if config["add_rev"]:
            x = ref_rev(x, config["max_npel"] // 2, config["max_ngel"] // 2)
        rps.append(x["pattern"])
        rgs.append(x["graph"])
    P = dataset.EdgeSeq.batch(rps, pre_pad=True)
    G = dataset.EdgeSeq.batch(rgs, pre_pad=True)
    return ps, gs, P, G


def _perturb(model):
    heads = [model.pred_net]
    with th.no_grad():
        for head in heads:
            head.pred_fc2.weight.uniform_(-0.3, 0.3)
            head.pred_fc2.bias.uniform_(-0.1, 0.1)
            if getattr(head, "weight_fc2", None) is not None:
                head.weight_fc2.weight.uniform_(-0.3, 0.3)
                head.weight_fc2.bias.uniform_(-0.1, 0.1)


def gen_models():
    from models.cnn import CNN
    for tag, extra in MODEL_CASES:
        config = base_config(**extra)
        rng = np.random.default_rng(MG.seed_of("edgeseq-model", tag) % (2 ** 32))
        th.manual_seed(MG.seed_of("edgeseq-model", tag))
        ps, gs, P, G = model_batch(rng, config, empty_graph=(tag == "a"))
        model = CNN(**config)
        sd_init = {k: v.clone() for k, v in model.state_dict().items()}
        _perturb(model)
        d = {"config_keys": np.array(sorted(config.keys())), "config_vals": np.array([repr(config[k]) for k in sorted(config.keys())]),
             "seed": MG.seed_of("edgeseq-model", tag)}
        for i, (p, g) in enumerate(zip(ps, gs)):
            put_graph(d, "p%d" % i, p)
            put_graph(d, "g%d" % i, g)
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
        for k, v in model.state_dict().items():
            if "running" in k:
                d["sd_after." + k] = v.clone()
        w2 = th.rand(G.u.shape)
        w3 = th.rand(G.u.shape + (3,))
        with th.no_grad():
            d["refine.w2"], d["refine.w3"] = w2, w3
            d["refine.sum2"] = model.refine_edge_weights(w2)
            d["refine.max2"] = model.refine_edge_weights(w2, use_max=True)
            d["refine.sum3"] = model.refine_edge_weights(w3)
            d["refine.max3"] = model.refine_edge_weights(w3, use_max=True)
            d["refine.long"] = model.refine_edge_weights((w2 * 5).long())
        save("model_" + tag, d)


def gen_expand():
    from models.cnn import CNN
    th.manual_seed(MG.seed_of("edgeseq-expand"))
    config = base_config(hid_dim=8, pred_hid_dim=8, share_emb_net=False, share_enc_net=False, pred_with_enc=True,
                         rep_num_graph_layers=1, rep_num_pattern_layers=1)
    grow = dict(max_ngv=40, max_ngvl=9, max_nge=80, max_ngel=20, max_npv=8, max_npvl=7, max_npe=20, max_npel=3)
    model = CNN(**config)
    d = {"config_keys": np.array(sorted(config.keys())), "config_vals": np.array([repr(config[k]) for k in sorted(config.keys())]),
         "grow_keys": np.array(sorted(grow.keys())), "grow_vals": np.array([grow[k] for k in sorted(grow.keys())]),
         "seed": MG.seed_of("edgeseq-expand"), "seed_grow": MG.seed_of("edgeseq-expand", "grow")}
    for k, v in model.state_dict().items():
        d["sd." + k] = v.clone()
    th.manual_seed(MG.seed_of("edgeseq-expand", "grow"))
    model.expand(**dict(config, **grow))
    for k, v in model.state_dict().items():
        d["sd_after." + k] = v.clone()
    save("expand_cnn", d)


GENERATORS = ["codes", "weights", "models", "expand"]


def main():
    os.makedirs(OUT, exist_ok=True)
    import ref_standin
    ref_standin.import_scm()
    for name in sys.argv[1:] or GENERATORS:
        globals()["gen_" + name]()


if __name__ == "__main__":
    main()
