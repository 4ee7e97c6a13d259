"""The CompGCN aggregation kernels (csrc/dmp_agg.hip: ``compgcn_agg_vec`` / ``_scalar`` and their backwards) against the
float64 restatement of ``util_fp64_compagg`` at what the layer fixtures do not reach: the 32- and 64-lane groups (widths 68 to
516, the padded widths of ``corr`` at h = 64 .. 512), a second and a third column pass, rows of up to 2 G + 1 in-edges (three
entry chunks, even and odd tails), grids of more than eight workgroups with a one-row tail, the scalar kernels (H % 4 != 0, a
misaligned base, a leading dimension that is no multiple of 4) and the refusal of conj-multiply there, no flag and no norm,
column slices of wider matrices, one node with self loops only and a graph without edges; then ``CompGCNLayer`` with
``comp_opt="corr"`` on the same graphs against the oracle in double.

Figures: 1e-5 of max(1, |ref|max) for outputs and input gradients and 2e-4 for parameter gradients (as
``test_gpu_layers_other.py``); every element is compared and no case has a wider allowance: the hub rows at width 516 and
the layer at h = 256 measured 4.5e-7 and 1.2e-6 at the most.  The same sum done with fp32 tensor ops (gather, compose,
``index_add``; for the layer the oracle in fp32) runs beside every case and both distances from fp64 are printed as FP64BAND
lines (DESIGN.md section 5 has the table)."""
import functools

import pytest
import torch as th

import dmp_oracle as O
import util_fp64_compagg as C

pytestmark = pytest.mark.gpu

CASES = C.compagg_cases()
NAN_BITS = 0x7FC00000


def _code(comp):
    from dualmessagepassing_amd import ops
    return {"sub": ops.COMP_SUB, "mult": ops.COMP_MULT, "cmul": ops.COMP_CMUL}[comp]


def _index(gr, gpu):
    from dualmessagepassing_amd.graph import GraphIndex
    return GraphIndex(gr["src"].to(gpu), gr["dst"].to(gpu), gr["N"], None if gr["rev"] is None else gr["rev"].to(gpu), validate=True)


@functools.lru_cache(maxsize=None)
def _ref(name):
    return C.reference(name)


def _leaf(t, view, gpu, gen):
    """(the leaf, the [rows, H] tensor the op gets: the leaf or a column slice of it)."""
    wide = C.widen(t, view, gen).to(gpu).requires_grad_(True)
    return wide, (wide if view is None else wide[:, view[0]:view[0] + t.size(1)])


def _grad(wide, view, H):
    if view is None:
        return wide.grad
    inside = th.zeros(wide.size(1), dtype=th.bool, device=wide.device)
    inside[view[0]:view[0] + H] = True
    assert float(wide.grad[:, ~inside].abs().sum()) == 0.0, "a gradient outside the slice"
    return wide.grad[:, inside]


def _run(name, gpu, views=True):
    """dict(out, dX, dZ, index) of a case through ``ops.compgcn_agg`` and autograd."""
    from dualmessagepassing_amd import ops
    c = CASES[name]
    gr, X, Z, norm, w = C.case_inputs(name)
    H = c["H"]
    gen = th.Generator().manual_seed(11)
    xview, zview = (c["xview"], c["zview"]) if views else (None, None)
    Xl, xv = _leaf(X, xview, gpu, gen)
    Zl, zv = _leaf(Z, zview, gpu, gen)
    for v, sl in ((xview, xv), (zview, zv)):
        if v is not None:
            assert ops._mat(sl)[0].data_ptr() == sl.data_ptr() and ops._mat(sl)[1] == v[1], "the slice must pass through"
    ix = _index(gr, gpu)
    out = ops.compgcn_agg(xv, zv, None if norm is None else norm.to(gpu), ix, _code(c["comp"]))
    (out * w.to(gpu)).sum().backward()
    return dict(out=out.detach(), dX=_grad(Xl, xview, H), dZ=_grad(Zl, zview, H), index=ix)


def _check(a, ref, yard, tol, what):
    """The figure ``tol`` for every element.  Prints the kernels' and the tensor ops' distance from fp64."""
    err, scale = C.dist(a, ref)
    yerr, _ = C.dist(yard, ref)
    print("FP64BAND %s kernel %.3g yardstick %.3g (x scale %.3g)" % (what, err / scale, yerr / scale, scale))
    C.close(a, ref, tol, what)


@pytest.mark.parametrize("case", sorted(CASES))
def test_compagg_matches_fp64(case, gpu):
    from dualmessagepassing_amd import _lib
    c = CASES[case]
    H = c["H"]
    gr = C.case_graph(c)
    if c["path"] == "unsupported":
        th.cuda.synchronize()
        with pytest.raises(_lib.DmpError, match="DMP_ERR_UNSUPPORTED"):
            _run(case, gpu)
        return
    got = _run(case, gpu)
    ref = _ref(case)
    assert tuple(got["out"].shape) == (gr["N"], 2 * H) and tuple(got["dZ"].shape) == (gr["E"], H)
    if c["graph"] == "n5-e0":
        assert float(got["out"].abs().max()) == 0.0 and float(got["dX"].abs().max()) == 0.0
        assert tuple(got["dX"].shape) == (5, H) and got["dZ"].numel() == 0
        assert float(ref["out"].abs().max()) == 0.0
        return
    yard = C.reference(case, th.float32, gpu)
    for k in ("out", "dX", "dZ"):
        _check(got[k], ref[k], yard[k], C.TOL, "compagg %s %s" % (case, k))
    if gr["rev"] is None:
        assert got["index"].rev8 is None, "the backward must have run without a flag"
        assert int(th.count_nonzero(got["out"][:, H:])) == 0
    if c["graph"] == "ladder":
        assert int(th.count_nonzero(got["out"][gr["ladder"][0]])) == 0            # the node without in-edges: written, zeros


def test_unsupported_launches_nothing(gpu):
    """conj-multiply on rows the float4 kernels cannot take: both entry points return DMP_ERR_UNSUPPORTED and write nothing."""
    from dualmessagepassing_amd import _lib
    from dualmessagepassing_amd._lib import ptr, stream_ptr
    lib = _lib.load()
    gr = C.ladder_graph(64, 0, "mixed")
    ix = _index(gr, gpu)
    N, E, H = gr["N"], gr["E"], 64
    wide = th.randn(N, H + 4, device=gpu)
    X = wide[:, 1:1 + H]
    Z = th.randn(E, H, device=gpu)
    out = th.full((N, 2 * H), float("nan"), device=gpu)
    code = lib.dmp_compgcn_agg(ptr(X), H + 4, ptr(Z), H, ptr(ix.in_ptr), ptr(ix.in_ent), ptr(ix.src32), None, N, H, 2,
                               ptr(out), 2 * H, stream_ptr())
    assert _lib.ERRORS[code] == "DMP_ERR_UNSUPPORTED"
    D = th.randn(N, 2 * H, device=gpu)
    dZ = th.full((E, H), float("nan"), device=gpu)
    dXe = th.full((E, H), float("nan"), device=gpu)
    code = lib.dmp_compgcn_agg_bwd(ptr(D), 2 * H, ptr(X), H + 4, ptr(Z), H, ptr(ix.src32), ptr(ix.dst32), ptr(ix.rev8), None,
                                   E, H, 2, ptr(dZ), H, ptr(dXe), H, stream_ptr())
    assert _lib.ERRORS[code] == "DMP_ERR_UNSUPPORTED"
    th.cuda.synchronize()
    for t in (out, dZ, dXe):
        assert bool((t.view(th.int32) == NAN_BITS).all())


@pytest.mark.parametrize("H,comp", [(64, "cmul"), (3, "sub")])
def test_graph_without_edges_zero_fills_the_rows_and_leaves_the_padding(H, comp, gpu):
    """N = 5, E = 0 through the C ABI (Z, ent and src NULL) into a NaN-filled matrix with ldo = 2H + 4."""
    from dualmessagepassing_amd import _lib
    from dualmessagepassing_amd._lib import ptr, stream_ptr
    lib = _lib.load()
    ix = _index(C.small_graph("n5-e0"), gpu)
    assert ix.in_ptr.tolist() == [0] * 6
    X = th.randn(5, H, device=gpu)
    out = th.full((5, 2 * H + 4), float("nan"), device=gpu)
    _lib.check(lib.dmp_compgcn_agg(ptr(X), H, None, H, ptr(ix.in_ptr), None, None, None, 5, H, _code(comp), ptr(out),
                                   2 * H + 4, stream_ptr()), "dmp_compgcn_agg")
    th.cuda.synchronize()
    assert int(th.count_nonzero(out[:, :2 * H])) == 0 and not bool(th.isnan(out[:, :2 * H]).any())
    assert bool((out[:, 2 * H:].contiguous().view(th.int32) == NAN_BITS).all())


@pytest.mark.parametrize("H,G,comp", [(20, 16, "cmul"), (68, 32, "cmul"), (260, 64, "cmul"), (6, 64, "mult")])
def test_every_output_written_and_padding_untouched(H, G, comp, gpu):
    """Through the C ABI into NaN-filled matrices with four padding columns: every column of the result is written (a node
    without in-edges too) and no padding column is."""
    from dualmessagepassing_amd import _lib
    from dualmessagepassing_amd._lib import ptr, stream_ptr
    lib = _lib.load()
    gr = C.ladder_graph(G, 0, "mixed")
    ix = _index(gr, gpu)
    N, E = gr["N"], gr["E"]
    gen = th.Generator().manual_seed(H)
    X, Z, D = th.randn(N, H, generator=gen), th.randn(E, H, generator=gen), th.randn(N, 2 * H, generator=gen)
    norm = th.rand(E, generator=gen) + 0.1
    Xg, Zg, Dg, ng = X.to(gpu), Z.to(gpu), D.to(gpu), norm.to(gpu)
    nan = float("nan")
    out = th.full((N, 2 * H + 4), nan, device=gpu)
    dZ = th.full((E, H + 4), nan, device=gpu)
    dXe = th.full((E, H + 4), nan, device=gpu)
    _lib.check(lib.dmp_compgcn_agg(ptr(Xg), H, ptr(Zg), H, ptr(ix.in_ptr), ptr(ix.in_ent), ptr(ix.src32), ptr(ng), N, H,
                                   _code(comp), ptr(out), 2 * H + 4, stream_ptr()), "dmp_compgcn_agg")
    _lib.check(lib.dmp_compgcn_agg_bwd(ptr(Dg), 2 * H, ptr(Xg), H, ptr(Zg), H, ptr(ix.src32), ptr(ix.dst32), ptr(ix.rev8),
                                       ptr(ng), E, H, _code(comp), ptr(dZ), H + 4, ptr(dXe), H + 4, stream_ptr()),
               "dmp_compgcn_agg_bwd")
    th.cuda.synchronize()
    for t, width in ((out, 2 * H), (dZ, H), (dXe, H)):
        assert not bool(th.isnan(t[:, :width]).any()), "a column of the result was left unwritten"
        assert bool((t[:, width:].contiguous().view(th.int32) == NAN_BITS).all()), "a padding column was written"
    Xd, Zd = X.double().requires_grad_(True), Z.double().requires_grad_(True)
    ref = C.compagg_fp64(Xd, Zd, gr["src"], gr["dst"], gr["rev"], norm.double(), N, comp)
    (ref * D.double()).sum().backward()
    C.close(out[:, :2 * H], ref.detach(), C.TOL, "out")
    C.close(dZ[:, :H], Zd.grad, C.TOL, "dZ")
    dX = th.zeros(N, H, dtype=th.float64).index_add(0, gr["src"], dXe[:, :H].double().cpu())
    C.close(dX, Xd.grad, C.TOL, "dX")


@pytest.mark.parametrize("case", sorted(n for n in CASES if n.startswith("strided-")))
def test_strided_and_contiguous_inputs_give_the_same_bits(case, gpu):
    a, b = _run(case, gpu, views=True), _run(case, gpu, views=False)
    for k in ("out", "dX", "dZ"):
        assert th.equal(a[k], b[k]), k


@pytest.mark.parametrize("case", ["G16-H64-cmul", "G32-H128-mult", "G64-H516-cmul", "scalar-H130-sub"])
def test_two_runs_are_bitwise_equal(case, gpu):
    a, b = _run(case, gpu), _run(case, gpu)
    for k in ("out", "dX", "dZ"):
        assert th.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------------------ the layer

LAYER_COMBOS = [(sl, rev, en) for sl in (True, False) for rev in ("mixed", "none") for en in ("both", "none")]


def _layer_reference(layer, gr, x, z, wn, we, edge_norm, dtype):
    """(node_out, edge_out, dx, dz, parameter gradients by name) of the oracle's layer on ``dtype`` copies, on the CPU."""
    p = {k: v.detach().cpu().clone().to(dtype).requires_grad_(True) for k, v in layer.named_parameters()}
    xd, zd = x.clone().to(dtype).requires_grad_(True), z.clone().to(dtype).requires_grad_(True)       # copies: x, z stay plain
    no, eo = O.compgcn_layer(p, gr["src"], gr["dst"], gr["rev"], xd, zd, "corr", edge_norm, "none")
    ((no * wn.to(dtype)).sum() + (eo * we.to(dtype)).sum()).backward()
    return no.detach(), eo.detach(), xd.grad, zd.grad, {k: v.grad for k, v in p.items()}


@pytest.mark.parametrize("self_loop,rev,edge_norm", LAYER_COMBOS)
@pytest.mark.parametrize("h", [7, 64, 127, 128, 254, 256])
def test_corr_layer_matches_fp64(h, self_loop, rev, edge_norm, gpu, monkeypatch):
    from dualmessagepassing_amd import compgcn, ops
    from dualmessagepassing_amd.graph import BatchedGraph
    what = "corr layer h%d-loop%d-rev_%s-norm_%s" % (h, self_loop, rev, edge_norm)
    width = compgcn.dft_matrices(h, gpu)[0].size(1)
    G = C.group_lanes(width)
    assert (width, G) == {7: (8, 16), 64: (68, 32), 127: (128, 32), 128: (132, 64), 254: (256, 64), 256: (260, 64)}[h]
    gr = C.ladder_graph(G, 0, rev)
    N, E = gr["N"], gr["E"]
    th.manual_seed(C.stable_seed(what))
    layer = compgcn.CompGCNLayer(h, h, self_loop=self_loop, comp_opt="corr", edge_norm=edge_norm, bias=True, batch_norm=False,
                                 act_func="none")
    with th.no_grad():
        layer.bias.uniform_(-0.2, 0.2)
    gen = th.Generator().manual_seed(C.stable_seed(what) + 1)
    x, z = th.randn(N, h, generator=gen), th.randn(E, h, generator=gen)
    wn, we = th.randn(N, h, generator=gen), th.randn(E, h, generator=gen)
    ref = _layer_reference(layer, gr, x, z, wn, we, edge_norm, th.float64)
    yard = _layer_reference(layer, gr, x, z, wn, we, edge_norm, th.float32)

    def no_gather(*a, **k):
        raise AssertionError("the correlation left the frequency domain: ops.gather_src was called")

    calls = []
    real = ops.compgcn_agg
    monkeypatch.setattr(ops, "gather_src", no_gather)
    monkeypatch.setattr(ops, "compgcn_agg", lambda X, Z, norm, ix, comp: (calls.append((X.size(1), comp)), real(X, Z, norm, ix, comp))[1])
    layer = layer.to(gpu)
    g = BatchedGraph(gr["src"].to(gpu), gr["dst"].to(gpu), N)
    if gr["rev"] is not None:
        g.edata["is_reversed"] = gr["rev"].to(gpu)
    xg, zg = x.to(gpu).requires_grad_(True), z.to(gpu).requires_grad_(True)
    node_out, edge_out = layer(g, xg, zg)
    ((node_out * wn.to(gpu)).sum() + (edge_out * we.to(gpu)).sum()).backward()
    assert calls == [(width, ops.COMP_CMUL)]
    assert (g.index().rev8 is None) == (rev == "none")
    got = (node_out, edge_out, xg.grad, zg.grad)
    for i, k in enumerate(("node_out", "edge_out", "dx", "dz")):
        _check(got[i], ref[i], yard[i], C.TOL, "%s %s" % (what, k))
    grads = {k: v.grad for k, v in layer.named_parameters()}
    assert sorted(grads) == sorted(ref[4])
    for k, gk in grads.items():
        if ref[4][k] is None:                   # out_weight without a flag: unused, as in the reference
            assert gk is None and k == "out_weight" and rev == "none"
            continue
        _check(gk, ref[4][k], yard[4][k], 2e-4, "%s grad %s" % (what, k))
