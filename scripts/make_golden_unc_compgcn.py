"""Emit the UNC CompGCN fixtures under tests/golden/unc_compgcn/ by running the REFERENCE's own
``UnsupervisedNodeClassification/Model/CompGCN/src/model.py``: ``TrainModel`` forward, the unsupervised loss
(``get_unsupervised_loss``) and its backward.

Runs only in the development container (needs the reference checkout), over the DGL / numba stand-ins of
``oracle/ref_standin.py`` (read-only use of ``oracle/``), single threaded with deterministic algorithms; the import of the
reference's module is ``make_golden_unc_rel.import_reference``.  Outputs are data only: inputs, parameters, the per-layer
``(h, r)`` pairs, the final embedding pair, the loss and the parameter gradients.  The recorded ``state_dict`` is the seeded
initial one except for the biases named below (zero at initialisation).

    python scripts/make_golden_unc_compgcn.py      # writes tests/golden/unc_compgcn/*.npz  (DMP_GOLDEN_UNC_COMPGCN_OUT: elsewhere)

Cases (R = 2 num_rels edge types): R 2, 4 and 8, widths 50 and 64, 1 and 2 layers, with and without the edge norm, one with
as many nodes as edges (the regulariser's edge term then takes the node representation too, model.py:376-383), one with
node attributes of width 12 in front of width 8 (input and output widths differ).  The graph has a hub (node 0) and four
nodes without an in-edge; the biases are set nonzero before the forward.
"""
import os
import sys

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("DMP_GOLDEN_UNC_COMPGCN_OUT") or os.path.join(ROOT, "tests", "golden", "unc_compgcn")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import make_golden as MG                                   # noqa: E402  (its helpers; one thread, deterministic algorithms)
from make_golden_unc_rel import import_reference           # noqa: E402

th.set_num_threads(1)
th.use_deterministic_algorithms(True)

# (tag, num_rels, width, layers, norm, node attribute width (0: a learned table), nodes, edges)
CASES = [
    ("r2_h50_l1_norm", 1, 50, 1, True, 0, 40, 120),
    ("r8_h64_l2_norm", 4, 64, 2, True, 0, 32, 96),
    ("r8_h50_l2_nonorm", 4, 50, 2, False, 0, 40, 140),
    ("r4_h64_l2_n_eq_e", 2, 64, 2, True, 0, 32, 32),
    ("r2_attri_i12_h8_l2", 1, 8, 2, True, 12, 40, 120),
]


def make_case(tag, num_rels, width, layers, with_norm, attri_width, N, E):
    mod = import_reference("CompGCN")
    import dgl
    seed = MG.seed_of("unc-compgcn", tag)
    rng = np.random.default_rng(seed % (2 ** 32))
    th.manual_seed(seed)
    R = 2 * num_rels
    table = N + 7
    # nodes N - 4 .. N - 1 receive no edge (zero in-degree); node 0 is a hub
    src = rng.integers(0, N, E)
    dst = rng.integers(0, N - 4, E)
    dst[: E // 8] = 0
    etype = rng.integers(0, R, E)
    nid = rng.permutation(table)[:N]
    g = dgl.DGLGraph.from_edges(th.from_numpy(src), th.from_numpy(dst), N)
    in_deg = np.bincount(dst, minlength=N).astype(np.float32)
    norm = th.from_numpy((1.0 / in_deg[dst]).reshape(-1, 1).astype(np.float32))
    S = 3 * E // 4
    triplets = np.stack([rng.integers(0, N, S), rng.integers(0, num_rels, S), rng.integers(0, N, S)], 1)
    labels = (rng.random(S) < 0.4).astype(np.float32)
    attri = rng.standard_normal((table, attri_width)).astype(np.float32) * 0.3 if attri_width else None

    model = mod.TrainModel(attri, table, width, num_rels, 0, num_hidden_layers=layers, dropout=0, reg_param=0.01)
    with th.no_grad():
        for k, p in model.named_parameters():
            if k.endswith(".bias") and (".layers." in k or k == "edge_fc.bias"):
                p.uniform_(-0.2, 0.2)
    outs = []
    hooks = [layer.register_forward_hook(lambda m, a, o: outs.append((o[0].detach().clone(), o[1].detach().clone())))
             for layer in model.model.layers]
    edge_type = th.from_numpy(etype)
    embed, _ = model(g, th.from_numpy(nid).view(-1, 1), edge_type, norm if with_norm else None)
    for h in hooks:
        h.remove()
    loss = model.get_unsupervised_loss(g, embed, edge_type, th.from_numpy(triplets), th.from_numpy(labels))
    loss.backward()
    d = {"num_rels": num_rels, "width": width, "layers": layers, "with_norm": int(with_norm), "attri_width": attri_width,
         "num_nodes_table": table, "seed": seed,
         "src": src, "dst": dst, "etype": etype, "nid": nid, "norm": norm, "triplets": triplets, "labels": labels,
         "embed.h": embed[0].detach(), "embed.r": embed[1].detach(), "loss": loss.detach()}
    if attri is not None:
        d["attri"] = attri
    for i, (h, r) in enumerate(outs):
        d["out.layer%d.h" % i] = h
        d["out.layer%d.r" % i] = r
    for k, v in model.state_dict().items():
        d["sd." + k] = v.clone()
    for k, p in model.named_parameters():
        if p.grad is not None:
            d["grad." + k] = p.grad
    np.savez_compressed(os.path.join(OUT, tag + ".npz"), **MG.t2n(d))
    print("wrote", tag + ".npz")


def main():
    os.makedirs(OUT, exist_ok=True)
    want = set(sys.argv[1:])
    for case in CASES:
        if not want or case[0] in want:
            make_case(*case)


if __name__ == "__main__":
    main()
