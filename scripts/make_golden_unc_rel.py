"""Emit the UNC R-GCN / R-GIN fixtures under tests/golden/unc_rel/ by running the REFERENCE's own
``UnsupervisedNodeClassification/Model/R-GCN/src/model.py`` and ``.../R-GIN/src/model.py``: ``TrainModel`` forward, the
unsupervised loss (``get_unsupervised_loss``) and its backward.

Runs only in the development container (needs the reference checkout), over the DGL / numba stand-ins of
``oracle/ref_standin.py`` (read-only use of ``oracle/``), single threaded with deterministic algorithms.  DGL itself is not
installed and the stand-in's ``dgl.nn.pytorch.RelGraphConv`` is an empty module, so after ``ref_standin.install()`` this
script puts ``RelGraphConv06`` below in its place: DGL 0.6's ``RelGraphConv`` (regularizer "basis", the non-low-mem path)
restated from its documented behaviour -- per-edge ``x[src] @ W[type]`` by ``bmm``, scaled by ``edata["norm"]`` when the
graph carries one, summed by destination, then ``+ h_bias``, ``+ x @ loop_weight``, activation, dropout.  Outputs are data
only: inputs, parameters, per-layer outputs, the loss and the parameter gradients.

    python scripts/make_golden_unc_rel.py      # writes tests/golden/unc_rel/*.npz  (DMP_GOLDEN_UNC_REL_OUT: elsewhere)

Cases (R = 2 num_rels edge types): R 2 and 8, widths 50 and 64, 1 and 2 layers, with and without the edge norm, one case
with num_bases < R (the reference's layers rebuilt with ``w_comp``), one with as many nodes as edges (the regulariser's edge
term then takes the node representation, model.py:713-718).  The biases are set nonzero before the forward.
"""
import functools
import os
import sys

import numpy as np
import torch as th
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("DMP_GOLDEN_UNC_REL_OUT") or os.path.join(ROOT, "tests", "golden", "unc_rel")
REF_MODEL = "/root/reference/UnsupervisedNodeClassification/Model"
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import make_golden as MG            # noqa: E402  (its helpers; importing it sets one thread and deterministic algorithms)

th.set_num_threads(1)
th.use_deterministic_algorithms(True)


class RelGraphConv06(nn.Module):
    """DGL 0.6 ``dgl.nn.pytorch.RelGraphConv``, regularizer "basis" only (what the reference uses)."""

    def __init__(self, in_feat, out_feat, num_rels, regularizer="basis", num_bases=None, bias=True, activation=None,
                 self_loop=True, low_mem=False, dropout=0.0, layer_norm=False):
        super().__init__()
        assert regularizer == "basis" and not layer_norm
        self.in_feat, self.out_feat, self.num_rels = in_feat, out_feat, num_rels
        self.regularizer = regularizer
        self.num_bases = num_bases
        if self.num_bases is None or self.num_bases > self.num_rels or self.num_bases <= 0:
            self.num_bases = self.num_rels
        self.bias, self.activation, self.self_loop, self.low_mem, self.layer_norm = bias, activation, self_loop, low_mem, layer_norm
        self.weight = nn.Parameter(th.Tensor(self.num_bases, self.in_feat, self.out_feat))
        if self.num_bases < self.num_rels:
            self.w_comp = nn.Parameter(th.Tensor(self.num_rels, self.num_bases))
        nn.init.xavier_uniform_(self.weight, gain=nn.init.calculate_gain("relu"))
        if self.num_bases < self.num_rels:
            nn.init.xavier_uniform_(self.w_comp, gain=nn.init.calculate_gain("relu"))
        if self.bias:
            self.h_bias = nn.Parameter(th.Tensor(out_feat))
            nn.init.zeros_(self.h_bias)
        if self.self_loop:
            self.loop_weight = nn.Parameter(th.Tensor(in_feat, out_feat))
            nn.init.xavier_uniform_(self.loop_weight, gain=nn.init.calculate_gain("relu"))
        self.dropout = nn.Dropout(dropout)

    def basis_message_func(self, edges, etypes):
        if self.num_bases < self.num_rels:
            weight = self.weight.view(self.num_bases, self.in_feat * self.out_feat)
            weight = th.matmul(self.w_comp, weight).view(self.num_rels, self.in_feat, self.out_feat)
        else:
            weight = self.weight
        h = edges.src["h"]
        msg = th.bmm(h.unsqueeze(1), weight.index_select(0, etypes)).squeeze(1)   # utils.bmm_maybe_select
        if "norm" in edges.data:
            msg = msg * edges.data["norm"]
        return {"msg": msg}

    def forward(self, g, feat, etypes, norm=None):
        import dgl.function as fn
        nd, ed = dict(g.ndata), dict(g.edata)                   # g.local_scope()
        try:
            g.ndata["h"] = feat
            if norm is not None:
                g.edata["norm"] = norm
            if self.self_loop:
                loop_message = th.matmul(feat, self.loop_weight)
            g.update_all(functools.partial(self.basis_message_func, etypes=etypes), fn.sum(msg="msg", out="h"))
            node_repr = g.ndata["h"]
            if self.bias:
                node_repr = node_repr + self.h_bias
            if self.self_loop:
                node_repr = node_repr + loop_message
            if self.activation:
                node_repr = self.activation(node_repr)
            return self.dropout(node_repr)
        finally:
            g.ndata.clear()
            g.ndata.update(nd)
            g.edata.clear()
            g.edata.update(ed)


def import_reference(kind):
    """The reference's ``model`` module of Model/<kind>/src (its own ``utils`` beside it), over the stand-ins."""
    import ref_standin
    ref_standin.install()
    sys.modules["dgl.nn.pytorch"].RelGraphConv = RelGraphConv06
    for name in ("model", "utils"):
        sys.modules.pop(name, None)
    path = os.path.join(REF_MODEL, kind, "src")
    sys.path.insert(0, path)
    try:
        import model
    finally:
        sys.path.remove(path)
    return model


# (tag, reference model dir, num_rels, width, layers, norm, num_bases (None: the reference's own), nodes, edges)
CASES = [
    ("rgcn_r2_h50_l1_norm", "R-GCN", 1, 50, 1, True, None, 40, 120),
    ("rgcn_r8_h64_l2_norm", "R-GCN", 4, 64, 2, True, None, 48, 160),
    ("rgcn_r8_h50_l2_nonorm", "R-GCN", 4, 50, 2, False, None, 40, 140),
    ("rgcn_r8_h50_l2_bases3", "R-GCN", 4, 50, 2, True, 3, 40, 140),
    ("rgcn_r2_h64_l1_n_eq_e", "R-GCN", 1, 64, 1, True, None, 60, 60),
    ("rgin_r2_h64_l1", "R-GIN", 1, 64, 1, True, None, 40, 120),
    ("rgin_r8_h50_l2", "R-GIN", 4, 50, 2, True, None, 48, 160),
    ("rgin_r8_h64_l2_bases2", "R-GIN", 4, 64, 2, False, 2, 40, 140),
]


def make_case(tag, kind, num_rels, width, layers, with_norm, bases, N, E):
    mod = import_reference(kind)
    import dgl
    seed = MG.seed_of("unc-rel", tag)
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
    if with_norm:
        g.edata["norm"] = norm
    S = 3 * E // 4
    triplets = np.stack([rng.integers(0, N, S), rng.integers(0, num_rels, S), rng.integers(0, N, S)], 1)
    labels = (rng.random(S) < 0.4).astype(np.float32)

    model = mod.TrainModel(None, table, width, num_rels, 0, num_hidden_layers=layers, dropout=0, reg_param=0.01)
    if bases is not None:
        cls = mod.RelGraphIso if kind == "R-GIN" else RelGraphConv06
        for i, old in enumerate(model.model.layers):
            model.model.layers[i] = cls(old.in_feat, old.out_feat, R, "basis", bases, activation=old.activation)
    with th.no_grad():
        for k, p in model.named_parameters():
            if k.endswith("h_bias") or k.endswith("out_layer.bias") or k == "edge_fc.bias":
                p.uniform_(-0.2, 0.2)
    outs = []
    hooks = [layer.register_forward_hook(lambda m, a, o: outs.append(o.detach().clone())) for layer in model.model.layers]
    edge_type = th.from_numpy(etype)
    embed, _ = model(g, th.from_numpy(nid).view(-1, 1), edge_type, norm if with_norm else None)
    for h in hooks:
        h.remove()
    loss = model.get_unsupervised_loss(g, embed, edge_type, th.from_numpy(triplets), th.from_numpy(labels))
    loss.backward()
    d = {"kind": kind, "num_rels": num_rels, "width": width, "layers": layers, "with_norm": int(with_norm),
         "num_bases": -1 if bases is None else bases, "num_nodes_table": table, "seed": seed,
         "src": src, "dst": dst, "etype": etype, "nid": nid, "norm": norm, "triplets": triplets, "labels": labels,
         "embed": embed.detach(), "loss": loss.detach()}
    for i, o in enumerate(outs):
        d["out.layer%d" % i] = o
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
