"""GPU parity: the HIP DMPLayer / rep-net against (a) the golden vectors emitted by the
reference's own code and (b) the CPU oracle on seeded random inputs.

Tolerances (fp32): outputs and input grads rtol=atol=1e-5 (x max(1,|ref|max)), parameter grads
2e-4, 3-layer reps 1e-4."""
import numpy as np
import pytest
import torch as th

import dmp_oracle as O
from conftest import golden_files, load_golden
from util_graphs import er_batch

pytestmark = pytest.mark.gpu


def _t(a):
    return th.from_numpy(np.asarray(a))


def _close(got, ref, rtol=1e-5, atol=1e-5, what=""):
    got = got.detach().double().cpu()
    ref = (ref if isinstance(ref, th.Tensor) else _t(ref)).detach().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.numel() == 0:
        return
    scale = max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max())
    # SURVEY 8(c) / BASELINE.md 3: |delta| <= 1e-5 * max(1, |ref|_max) -- rtol = atol = 1e-5 against the array's scale
    assert err <= max(atol, rtol * scale), "%s: max err %g (scale %g)" % (what, err, scale)


def _rep_case(batch, n, m, h, gates, residual, act):
    """Seeded 2-layer rep-net case on the CPU (fp32): graph, parameters, inputs, cotangents, 0 / 1 gates."""
    rng = np.random.default_rng(n * h + batch)
    src, dst, rev, N, bnn, bne = er_batch(batch, n, m, rng)
    E = len(src)
    gen = th.Generator().manual_seed(h + n)
    layers = [O.random_dmp_params(h, h, gen, act) for _ in range(2)]
    v0, e0 = th.randn(N, h, generator=gen), th.randn(E, h, generator=gen)
    wv, we = th.randn(N, h, generator=gen), th.randn(E, h, generator=gen)
    vg = (th.rand(N, 1, generator=gen) < 0.7).float() if gates else None
    eg = (th.rand(E, 1, generator=gen) < 0.7).float() if gates else None
    live = [None if vg is None else vg.view(-1) != 0, None if eg is None else eg.view(-1) != 0] * 2
    return dict(src=_t(src), dst=_t(dst), rev=_t(rev), N=N, E=E, h=h, bnn=_t(bnn), bne=_t(bne), layers=layers, v0=v0, e0=e0, wv=wv,
                we=we, vg=vg, eg=eg, residual=residual, act=act, live=live)


def _oracle_rep(c, dtype, masks=None, probe=False, grads=True):
    """The oracle on a ``_rep_case`` in ``dtype``, its activation derivatives pinned to ``masks`` (None: its own branches) ->
    ({"v_rep", "e_rep", "dv", "de", "<layer>.<parameter>"}, kinked probes or None)."""
    from util_branches import kinked_probes
    cast = lambda t: None if t is None else t.to(dtype)
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(grads)      # (a copy: ``to`` of the same type is the case's own tensor)
    layers = [{k: leaf(v) for k, v in p.items()} for p in c["layers"]]
    v, e = leaf(c["v0"]), leaf(c["e0"])
    fwd = lambda: O.dmpnn_graph_rep(layers, c["src"], c["dst"], c["rev"], O.out_degrees(c["src"], c["N"]), v, e, cast(c["vg"]),
                                    cast(c["eg"]), c["residual"], c["act"])
    O.PROBE = [] if probe else None
    try:
        if masks is None:
            a, b = fwd()
        else:
            with O.pinned(masks):
                a, b = fwd()
        probes = None if O.PROBE is None else kinked_probes(O.PROBE)
    finally:
        O.PROBE = None
    out = {"v_rep": a.detach(), "e_rep": b.detach()}
    if grads:
        leaves = [("dv", v), ("de", e)] + [("%d.%s" % (i, k), p) for i, l in enumerate(layers) for k, p in l.items()]
        got = th.autograd.grad((a * cast(c["wv"])).sum() + (b * cast(c["we"])).sum(), [t for _, t in leaves])
        out.update({k: g for (k, _), g in zip(leaves, got)})
    return out, probes


def _product_rep(c, fused, gpu, dst=None):
    """The product's forward on a ``_rep_case`` (``dst``: other destinations than the case's) -> (``backward`` returning what
    ``_oracle_rep`` returns, hidden rows per site as tests/util_branches.py reads them)."""
    from dualmessagepassing_amd.dmpnn import DMPNNRep
    from dualmessagepassing_amd.graph import BatchedGraph
    from util_branches import fused_hidden, modular_hidden
    L = len(c["layers"])
    net = DMPNNRep(hid_dim=c["h"], rep_num_graph_layers=L, rep_num_pattern_layers=L, share_rep_net=True,
                   rep_residual=c["residual"], rep_dmpnn_batch_norm=False, rep_act_func=c["act"])
    sd = {}
    for i, p in enumerate(c["layers"]):
        for k, v in p.items():
            sd["g_rep_net.dmpnn.graph_dmpnn_(%d).%s" % (i, k)] = v
            sd["p_rep_net.dmpnn.graph_dmpnn_(%d).%s" % (i, k)] = v
    net.load_state_dict(sd, strict=True)
    net.to(gpu)
    net.use_fused = fused
    g = BatchedGraph(c["src"].to(gpu), (c["dst"] if dst is None else dst).to(gpu), c["N"], c["bnn"].to(gpu), c["bne"].to(gpu))
    g.edata["is_reversed"] = c["rev"].to(gpu)
    vgp, egp = c["v0"].to(gpu).requires_grad_(True), c["e0"].to(gpu).requires_grad_(True)
    layers = list(net.g_rep_net["dmpnn"])
    if fused:   # the fast path must be the one that runs for this activation
        assert all(l.fused_ok(g, vgp, egp) for l in layers)
    gates = dict(v_gate=None if c["vg"] is None else c["vg"].to(gpu), e_gate=None if c["eg"] is None else c["eg"].to(gpu))
    if fused:
        a, b = net.get_graph_rep(g, vgp, egp, **gates)
        hidden = fused_hidden((a, b))
    else:
        with modular_hidden(layers) as rec:
            a, b = net.get_graph_rep(g, vgp, egp, **gates)
        hidden = rec.rows((a, b))
    assert len(hidden) == 2 * L, [s for s, _ in hidden]

    def backward():
        ((a * c["wv"].to(gpu)).sum() + (b * c["we"].to(gpu)).sum()).backward()
        out = {"v_rep": a.detach(), "e_rep": b.detach(), "dv": vgp.grad, "de": egp.grad}
        for k, p in net.g_rep_net.named_parameters():       # dmpnn.graph_dmpnn_(<i>).<parameter>
            out["%s.%s" % (k.split("(", 1)[1].split(")", 1)[0], k.split(").", 1)[1])] = p.grad
        return out
    return backward, hidden


def _same_live_branches(ma, mb, live):
    return all(th.equal(x if lv is None else x[lv], y if lv is None else y[lv]) for x, y, lv in zip(ma, mb, live))


def _rep_gradients_close(got, ref, what):
    """The strict rule, everywhere: dv and de at 1e-4, every parameter gradient at 2e-4.  Returns the worst
    error relative to max(1, |ref|max)."""
    worst = 0.0
    for k, r in ref.items():
        if k in ("v_rep", "e_rep"):
            continue
        tol = 1e-4 if k in ("dv", "de") else 2e-4
        _close(got[k], r, tol, tol, "%s %s" % (what, "grad " + k if "." in k else k))
        worst = max(worst, float((got[k].detach().double().cpu() - r.double()).abs().max()) / max(1.0, float(r.abs().max())))
    return worst


def _graph(d, dev, prefix=""):
    from dualmessagepassing_amd.graph import BatchedGraph
    g = BatchedGraph(_t(d[prefix + "src"]).to(dev), _t(d[prefix + "dst"]).to(dev), int(d[prefix + "num_nodes"]))
    if prefix + "rev" in d:
        g.edata["is_reversed"] = _t(d[prefix + "rev"]).to(dev)
    g.ndata["out_deg"] = _t(d[prefix + "out_deg"]).to(dev)
    return g


@pytest.mark.parametrize("path", golden_files("dmplayer_"))
def test_dmplayer_matches_reference_golden(path, gpu):
    from dualmessagepassing_amd.dmpnn import DMPLayer
    d = load_golden(path)
    h = d["x"].shape[1]
    layer = DMPLayer(h, h, num_mlp_layers=int(d["num_mlp_layers"]), batch_norm=False,
                     act_func=str(d["act_func"]), dropout=0.0)
    sd = {k[2:]: _t(v) for k, v in d.items() if k.startswith("p.")}
    layer.load_state_dict(sd, strict=True)  # same parameter names/shapes as the reference
    layer.to(gpu)
    g = _graph(d, gpu)
    g.index(validate=True)
    x = _t(d["x"]).to(gpu).requires_grad_(True)
    z = _t(d["z"]).to(gpu).requires_grad_(True)
    layer.write_edge_agg = True      # the reference's UDF side effect (dmpnn.py:126), opt-in here
    node_out, edge_out = layer(g, x, z)
    _close(node_out, d["node_out"], what="node_out")
    _close(edge_out, d["edge_out"], what="edge_out")
    _close(g.ndata["node_agg"], d["node_agg"], what="node_agg")
    _close(g.edata["edge_agg"], d["edge_agg"], what="edge_agg")
    ((node_out * _t(d["wn"]).to(gpu)).sum() + (edge_out * _t(d["we"]).to(gpu)).sum()).backward()
    _close(x.grad, d["dx"], what="dx")
    _close(z.grad, d["dz"], what="dz")
    for k, p in layer.named_parameters():
        if "g." + k in d:
            _close(p.grad, d["g." + k], 2e-4, 2e-4, what="grad " + k)


def test_dmpnn_rep_matches_reference_golden(gpu):
    from dualmessagepassing_amd.dmpnn import DMPNNRep
    d = load_golden(golden_files("dmpnn_rep")[0])
    h, L = int(d["hid"]), int(d["layers"])
    net = DMPNNRep(hid_dim=h, rep_num_graph_layers=L, rep_num_pattern_layers=L, share_rep_net=True,
                   rep_residual=True, rep_dmpnn_batch_norm=False, rep_act_func="relu")
    sd = {"g_rep_net." + k[2:]: _t(v) for k, v in d.items() if k.startswith("p.")}
    sd.update({"p_rep_net." + k[2:]: _t(v) for k, v in d.items() if k.startswith("p.")})
    net.load_state_dict(sd, strict=True)  # reference key names incl. the shared p_rep_net aliases
    net.to(gpu)
    for tag in ("p", "g"):
        g = _graph(d, gpu, tag + "_")
        v = _t(d[tag + "_v_emb"]).to(gpu).requires_grad_(True)
        e = _t(d[tag + "_e_emb"]).to(gpu).requires_grad_(True)
        net.zero_grad()
        if tag == "p":
            v_rep, e_rep = net.get_pattern_rep(g, v, e)
        else:
            v_rep, e_rep = net.get_graph_rep(g, v, e, v_gate=_t(d["g_v_gate"]).to(gpu),
                                             e_gate=_t(d["g_e_gate"]).to(gpu))
        _close(v_rep, d[tag + "_v_rep"], 1e-4, 1e-4, tag + " v_rep")
        _close(e_rep, d[tag + "_e_rep"], 1e-4, 1e-4, tag + " e_rep")
        ((v_rep * _t(d[tag + "_wv"]).to(gpu)).sum() + (e_rep * _t(d[tag + "_we"]).to(gpu)).sum()).backward()
        _close(v.grad, d[tag + "_dv_emb"], 1e-4, 1e-4, tag + " dv")
        _close(e.grad, d[tag + "_de_emb"], 1e-4, 1e-4, tag + " de")
        for k, p in net.g_rep_net.named_parameters():
            _close(p.grad, d["%s_grad.%s" % (tag, k)], 2e-4, 2e-4, tag + " grad " + k)


@pytest.mark.parametrize("batch,n,m,h,act,rev", [
    (32, 64, 256, 64, "relu", True),       # BASELINE config 1 target shape
    (32, 8, 12, 64, "relu", True),         # config 1 pattern shape
    (8, 64, 256, 128, "leaky_relu", True),  # config 2 width
    (4, 16, 40, 256, "relu", False),       # config 5 width, no REVFLAG
    (3, 7, 9, 20, "relu", True),           # H not a power of two
    (3, 7, 9, 7, "leaky_relu", True),      # H % 4 != 0 -> scalar kernels
])
def test_dmplayer_matches_oracle_random(batch, n, m, h, act, rev, gpu):
    from dualmessagepassing_amd.dmpnn import DMPLayer
    from dualmessagepassing_amd.graph import BatchedGraph
    rng = np.random.default_rng(batch * 1000 + n + h)
    src, dst, r, N, bnn, bne = er_batch(batch, n, m, rng, add_rev=rev)
    gen = th.Generator().manual_seed(h * 7 + n)
    p = O.random_dmp_params(h, h, gen, act)
    x = th.randn(N, h, generator=gen)
    z = th.randn(len(src), h, generator=gen)
    wn, we = th.randn(N, h, generator=gen), th.randn(len(src), h, generator=gen)
    tsrc, tdst = _t(src), _t(dst)
    trev = _t(r) if rev else None
    out_deg = O.out_degrees(tsrc, N)
    # oracle (fp32, reference op order) and its autograd
    po = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    xo, zo = x.clone().requires_grad_(True), z.clone().requires_grad_(True)
    no, eo, _, _ = O.dmp_layer(po, tsrc, tdst, trev, out_deg, xo, zo, act)
    ((no * wn).sum() + (eo * we).sum()).backward()
    # product
    layer = DMPLayer(h, h, batch_norm=False, act_func=act)
    layer.load_state_dict(p, strict=True)
    layer.to(gpu)
    g = BatchedGraph(tsrc.to(gpu), tdst.to(gpu), N, _t(bnn).to(gpu), _t(bne).to(gpu))
    if rev:
        g.edata["is_reversed"] = trev.to(gpu)
    xg, zg = x.to(gpu).requires_grad_(True), z.to(gpu).requires_grad_(True)
    ng, eg = layer(g, xg, zg)
    assert th.equal(g.ndata["out_deg"].cpu(), out_deg)  # integer, exact
    _close(ng, no, what="node_out")
    _close(eg, eo, what="edge_out")
    ((ng * wn.to(gpu)).sum() + (eg * we.to(gpu)).sum()).backward()
    _close(xg.grad, xo.grad, what="dx")
    _close(zg.grad, zo.grad, what="dz")
    for k, q in layer.named_parameters():
        if po[k].grad is not None:
            _close(q.grad, po[k].grad, 2e-4, 2e-4, what="grad " + k)


def test_generic_update_all_path_matches_oracle(gpu):
    """The DGL-style UDF path (update_all / apply_edges with fn.sum) on the HIP seg-sum and
    gather kernels, driven by a reference-shaped message function."""
    from dualmessagepassing_amd.graph import BatchedGraph, function as fn
    rng = np.random.default_rng(3)
    src, dst, r, N, bnn, bne = er_batch(5, 9, 14, rng)
    h = 12
    gen = th.Generator().manual_seed(1)
    x, z = th.randn(N, h, generator=gen), th.randn(len(src), h, generator=gen)
    w = th.randn(h, h, generator=gen)
    g = BatchedGraph(_t(src).to(gpu), _t(dst).to(gpu), N)
    xg, zg, wg = x.to(gpu).requires_grad_(True), z.to(gpu).requires_grad_(True), w.to(gpu)
    g.ndata["h"], g.edata["h"] = xg, zg

    def msg(edges):
        edges.data["side"] = edges.dst["h"] - edges.src["h"]
        return {"m": (edges.src["h"] * edges.data["h"]) @ wg}

    g.update_all(msg, fn.sum(msg="m", out="agg"), lambda nodes: {"out": nodes.data["agg"] + nodes.data["h"]})
    g.apply_edges(lambda edges: {"eout": edges.data["side"] * 2})
    xo, zo = x.clone().requires_grad_(True), z.clone().requires_grad_(True)
    ts, td = _t(src), _t(dst)
    out_o = O.seg_sum((xo[ts] * zo) @ w, td, N) + xo
    eout_o = (xo[td] - xo[ts]) * 2
    _close(g.ndata["out"], out_o, what="out")
    _close(g.edata["eout"], eout_o, what="eout")
    (g.ndata["out"].sum() + (g.edata["eout"] ** 2).sum()).backward()
    (out_o.sum() + (eout_o ** 2).sum()).backward()
    _close(xg.grad, xo.grad, what="dx")
    _close(zg.grad, zo.grad, what="dz")


def test_cpu_tensors_are_rejected():
    """No CPU fallback in the product path."""
    from dualmessagepassing_amd import _lib
    from dualmessagepassing_amd.dmpnn import DMPLayer
    from dualmessagepassing_amd.graph import BatchedGraph
    layer = DMPLayer(8, 8, batch_norm=False)
    g = BatchedGraph(th.tensor([0, 1]), th.tensor([1, 0]), 2)
    with pytest.raises(_lib.DmpError):
        layer(g, th.randn(2, 8), th.randn(2, 8))


@pytest.mark.parametrize("act", ["relu", "leaky_relu"])   # leaky_relu (slope 1/5.5): the reference's default rep_act_func
@pytest.mark.parametrize("batch,n,m,h,gates,residual", [
    (8, 16, 40, 32, True, True), (8, 16, 40, 32, False, True), (8, 16, 40, 32, True, False),
    (64, 64, 256, 128, True, True),      # enough rows for the split-K weight-gradient path
    (32, 64, 256, 64, True, True),       # the reference's hid_dim (README.md:21-119)
    (3, 5, 7, 20, True, True),
])
def test_fused_rep_path_equals_modular_path_and_oracle(batch, n, m, h, gates, residual, act, gpu):
    """The single-node fused layer (fused.py) == the modular layer + gate + residual == oracle.

    Gradients on ONE rule: each path's hidden rows name the derivative branch it took at every ReLU / LeakyReLU unit
    (tests/util_branches.py: checked against the fp64 pre-activations on the live rows), the fp64 oracle is pinned to
    them, and dv / de are held to 1e-4 and every parameter gradient to 2e-4 against it, with no exception for units
    near the kink.  Measured on an MI355X: up to 179 of 2.9 M live units of a site inside the window, at most one branch
    per case on the other side than fp64's, the worst pinned gradient error 2.7e-6 of the reference's largest entry."""
    from util_branches import branch_masks
    c = _rep_case(batch, n, m, h, gates, residual, act)
    free64, probes = _oracle_rep(c, th.float64, probe=True, grads=False)
    free32, _ = _oracle_rep(c, th.float32, grads=False)
    results, masks, ref64, ref32 = {}, {}, {}, {}
    for fused in (True, False):
        what = "fused=%s" % fused
        backward, hidden = _product_rep(c, fused, gpu)
        masks[fused], differing = branch_masks(hidden, probes, c["live"], O.activation(act), 1e-4, what)
        if not fused and _same_live_branches(masks[True], masks[False], c["live"]):
            ref64[fused], ref32[fused] = ref64[True], ref32[True]     # same pieces, same references
        else:
            ref64[fused], _ = _oracle_rep(c, th.float64, masks[fused])
            ref32[fused], _ = _oracle_rep(c, th.float32, masks[fused])
        results[fused] = backward()
        _close(results[fused]["v_rep"], free32["v_rep"], 1e-4, 1e-4, "v_rep " + what)
        _close(results[fused]["e_rep"], free32["e_rep"], 1e-4, 1e-4, "e_rep " + what)
        worst = _rep_gradients_close(results[fused], ref64[fused], what)
        print("%s: %d branches differ from fp64, worst pinned gradient error %.3g" % (what, sum(differing), worst))
    # Against an fp64 run of the same math the product must be no worse than a few times the
    # fp32 restatement of the reference, pinned to the same branches; fused and modular paths differ
    # from each other only by fp32 re-association (the fused path also folds W0 into the projections).
    same = _same_live_branches(masks[True], masks[False], c["live"])
    for name in ("v_rep", "e_rep", "dv", "de"):
        for fused in (True, False):
            r64 = ref64[fused][name]
            scale = max(1.0, float(r64.abs().max()))
            e32 = float((ref32[fused][name].double() - r64).abs().max())
            err = float((results[fused][name].detach().cpu().double() - r64).abs().max())
            assert err <= max(6.0 * e32, 2e-6 * scale), \
                "%s fused=%s: err %g vs fp32-oracle err %g" % (name, fused, err, e32)
        if same or name in ("v_rep", "e_rep"):      # (other branches: each path was held to its own pinned fp64 run above)
            _close(results[True][name], results[False][name].detach().cpu(), 1e-4, 1e-4, "fused vs modular " + name)


@pytest.mark.parametrize("fused", [True, False])
def test_one_flipped_branch_fails_the_pinned_comparison(fused, gpu):
    """(8, 16, 40, 32), gates, residual, leaky_relu: with the product's own masks the strict comparison passes; with ONE
    live unit of them flipped it must fail -- the pin is what makes the strict rule hold, not slack in the rule."""
    from util_branches import branch_masks
    c = _rep_case(8, 16, 40, 32, True, True, "leaky_relu")
    _, probes = _oracle_rep(c, th.float64, probe=True, grads=False)
    backward, hidden = _product_rep(c, fused, gpu)
    masks, _ = branch_masks(hidden, probes, c["live"], O.activation("leaky_relu"), 1e-4, "fused=%s" % fused)
    ref, _ = _oracle_rep(c, th.float64, masks)
    site = 2                                             # the last layer's node MLP: the first live unit far from the kink
    pre = probes[site][1].abs()
    far = (pre > pre[c["live"][site]].median()) & c["live"][site].view(-1, 1)
    r, col = (int(i) for i in far.nonzero()[0])
    flipped = [m.clone() for m in masks]
    flipped[site][r, col] = not bool(flipped[site][r, col])
    wrong, _ = _oracle_rep(c, th.float64, flipped)
    got = backward()
    _rep_gradients_close(got, ref, "own branches")
    with pytest.raises(AssertionError, match="one unit flipped"):
        _rep_gradients_close(got, wrong, "one unit flipped")


def test_pinned_comparison_under_poisoned_dead_rows(gpu, monkeypatch):
    """The same case with every dead-row buffer starting as NaN (``fused.POISON_DEAD_ROWS``): the hidden rows under a zero
    gate are NaN then; none may reach a mask (NaN > 0 is False), a check or a gradient."""
    from dualmessagepassing_amd import fused as F_
    from util_branches import branch_masks
    monkeypatch.setattr(F_, "POISON_DEAD_ROWS", True)
    c = _rep_case(8, 16, 40, 32, True, True, "leaky_relu")
    _, probes = _oracle_rep(c, th.float64, probe=True, grads=False)
    backward, hidden = _product_rep(c, True, gpu)
    masks, _ = branch_masks(hidden, probes, c["live"], O.activation("leaky_relu"), 1e-4, "poisoned")
    for (site, rows), m, lv in zip(hidden, masks, c["live"]):
        assert m.dtype == th.bool and not bool(m[th.isnan(rows).any(1).cpu()].any()), site
        assert bool(th.isfinite(rows[lv.to(rows.device)]).all()), site
    ref, _ = _oracle_rep(c, th.float64, masks)
    got = backward()
    assert all(bool(th.isfinite(t).all()) for t in got.values())
    _rep_gradients_close(got, ref, "poisoned")


def test_joint_pattern_graph_pass_matches_reference_golden(gpu):
    """DMPNNRep.forward runs the SHARED rep-net once over the union of the pattern and target
    batches; results must equal the reference's two separate loops (golden dmpnn_rep.npz), and
    the parameter gradients the sum of both losses' gradients."""
    from dualmessagepassing_amd.dmpnn import DMPNNRep
    d = load_golden(golden_files("dmpnn_rep")[0])
    h, L = int(d["hid"]), int(d["layers"])
    net = DMPNNRep(hid_dim=h, rep_num_graph_layers=L, rep_num_pattern_layers=L, share_rep_net=True,
                   rep_residual=True, rep_dmpnn_batch_norm=False, rep_act_func="relu")
    sd = {"g_rep_net." + k[2:]: _t(v) for k, v in d.items() if k.startswith("p.")}
    sd.update({"p_rep_net." + k[2:]: _t(v) for k, v in d.items() if k.startswith("p.")})
    net.load_state_dict(sd, strict=True)
    net.to(gpu)
    pg, gg = _graph(d, gpu, "p_"), _graph(d, gpu, "g_")
    pv = _t(d["p_v_emb"]).to(gpu).requires_grad_(True)
    pe = _t(d["p_e_emb"]).to(gpu).requires_grad_(True)
    gv = _t(d["g_v_emb"]).to(gpu).requires_grad_(True)
    ge = _t(d["g_e_emb"]).to(gpu).requires_grad_(True)
    assert net.get_joint_rep(pg, gg, pv, pe, gv, ge, _t(d["g_v_gate"]).to(gpu), _t(d["g_e_gate"]).to(gpu)) is not None
    p_v, p_e, g_v, g_e = net(pg, gg, pv, pe, gv, ge, v_gate=_t(d["g_v_gate"]).to(gpu), e_gate=_t(d["g_e_gate"]).to(gpu))
    _close(p_v, d["p_v_rep"], 1e-4, 1e-4, "p_v_rep")
    _close(p_e, d["p_e_rep"], 1e-4, 1e-4, "p_e_rep")
    _close(g_v, d["g_v_rep"], 1e-4, 1e-4, "g_v_rep")
    _close(g_e, d["g_e_rep"], 1e-4, 1e-4, "g_e_rep")
    loss = (p_v * _t(d["p_wv"]).to(gpu)).sum() + (p_e * _t(d["p_we"]).to(gpu)).sum() \
        + (g_v * _t(d["g_wv"]).to(gpu)).sum() + (g_e * _t(d["g_we"]).to(gpu)).sum()
    loss.backward()
    _close(pv.grad, d["p_dv_emb"], 1e-4, 1e-4, "p dv")
    _close(pe.grad, d["p_de_emb"], 1e-4, 1e-4, "p de")
    _close(gv.grad, d["g_dv_emb"], 1e-4, 1e-4, "g dv")
    _close(ge.grad, d["g_de_emb"], 1e-4, 1e-4, "g de")
    for k, p in net.g_rep_net.named_parameters():
        _close(p.grad, _t(d["p_grad." + k]) + _t(d["g_grad." + k]), 2e-4, 2e-4, "grad " + k)


def test_flip_comparator_rejects_an_indexing_error(gpu):
    """Negative test of the pinned comparison: the product is run on a batch of 64 graphs in
    which ONE graph's destinations are rotated -- exactly the kind of error a loose "2 % of the elements may be off"
    comparison lets through.  Against the oracle on the CORRECT batch, pinned to the branches that product took, the
    strict comparison must fail; on the correct batch it must pass."""
    from util_branches import branch_masks
    batch, n, m, h, act = 64, 16, 40, 64, "leaky_relu"
    c = _rep_case(batch, n, m, h, False, True, act)
    _, probes = _oracle_rep(c, th.float64, probe=True, grads=False)
    backward, hidden = _product_rep(c, True, gpu)
    masks, _ = branch_masks(hidden, probes, c["live"], O.activation(act), 1e-4, "correct batch")
    ref, _ = _oracle_rep(c, th.float64, masks)
    _rep_gradients_close(backward(), ref, "correct batch")
    # graph 37: every edge's destination moved to the next node of the same graph
    bad = c["dst"].clone()
    e_lo, n_lo = int(c["bne"][:37].sum()), int(c["bnn"][:37].sum())
    sl = slice(e_lo, e_lo + int(c["bne"][37]))
    bad[sl] = n_lo + (c["dst"][sl] - n_lo + 1) % int(c["bnn"][37])
    backward, hidden = _product_rep(c, True, gpu, dst=bad)
    # the branches that run took are ITS branches: in graph 37 they are those of another function, so the window check is
    # not asked of them -- the oracle of the correct batch is pinned to them as they are
    ref, _ = _oracle_rep(c, th.float64, [rows.detach().cpu() > 0 for _, rows in hidden])
    got = backward()
    for k in ("dv", "de"):
        with pytest.raises(AssertionError, match="rotated " + k):
            _close(got[k], ref[k], 1e-4, 1e-4, "rotated " + k)
    # the comparison this replaces (<= 2 % of the elements off, all within 5e-2) would have passed one of them
    err = (got["dv"].cpu().double() - ref["dv"]).abs()
    assert float((err > 2e-4 * max(1.0, float(ref["dv"].abs().max()))).double().mean()) <= 0.02      # why the old rule was too loose
