"""A gated inner layer's edge MLP forward over the kept edges' class tiles as ONE launch (csrc/dmp_edgemlp.hip:
``fused.edge_mlp_fwd``) against the two launches it replaces (``dmp_edge_fwd_typed`` then ``dmp_out_fwd_typed``) and against fp64,
on hand-made tile lists.

The arithmetic contract: the same bf16 piece products in the same order and the same epilogue order, so ``H1e`` and ``zn`` are
``torch.equal`` to the two launches' on every kept row -- although the second of them walks the kept rows in ascending order here and
the fused launch walks the class tiles.  Against torch fp64 on the CPU both stay within ``1e-5 * max(1, |ref|max)``;
the two launches' error is printed beside the fused launch's.  No bit difference is documented, so the bound is that figure alone.
Dead input rows hold NaN; dead output rows must keep their sentinel bit for bit."""
import os
import sys

import pytest
import torch as th

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 128
SLOPE = 1.0 / 5.5
SENT = 7.5


class _Index:
    """What ``fused.edge_mlp_fwd`` / ``fused.edge_fwd_typed`` read of a graph index when the selectors come in through ``sel``."""

    def __init__(self, num_nodes, num_edges):
        self.num_nodes, self.num_edges = num_nodes, num_edges


def _class_tiles(kept, cls, coefs, E):
    """``(slot, tile_scale, num_tiles, bound)`` as ``GraphIndex.class_tiles_gated``: the kept edges class by class, every class padded
    with -1 to whole 32-slot tiles; ``tile_scale`` = the class coefficient of each tile."""
    slots, scale = [], []
    for c in range(len(coefs)):
        ids = kept[cls[kept] == c]
        if ids.numel() == 0:
            continue
        nt = (ids.numel() + 31) // 32
        s = th.full((nt * 32,), -1, dtype=th.int32)
        s[:ids.numel()] = ids.to(th.int32)
        slots.append(s)
        scale += [coefs[c]] * nt
    nt = len(scale)
    bound = (E + 31) // 32 + len(coefs)
    slot = th.full((bound * 32,), -1, dtype=th.int32)
    if slots:
        slot[:nt * 32] = th.cat(slots)
    ts = th.zeros(bound)
    ts[:nt] = th.tensor(scale)
    return slot, ts, th.tensor([nt], dtype=th.int32), bound


def _ascending_tiles(kept, E):
    """The kept rows in ascending order, 32 per tile (``fused.ascending_tiles``): what today's second launch walks."""
    bound = (E + 31) // 32
    slot = th.full((bound * 32,), -1, dtype=th.int32)
    slot[:kept.numel()] = kept.to(th.int32)
    return slot, th.zeros(bound), th.tensor([(kept.numel() + 31) // 32], dtype=th.int32), bound


def _pick(E, n):
    return lambda g: th.randperm(E, generator=g)[:n].sort().values


# name: (E, N, class coefficients, kept edges, class of an edge)
SHAPES = {
    # 77 kept edges in three degree classes (about 26 each): three padded tiles, one per workgroup ...
    "kept77_three_classes": (200, 40, (0.5, 1.0 / 3.0, 0.25), _pick(200, 77), lambda e, g: (th.arange(e) * 3) // e),
    # ... and the same list with a tile bound of ONE, which sizes the grid at one workgroup (the kernels size nothing else by it: the
    # slot list is read through a descriptor of ``num_tiles`` tiles): all three tiles in one range, the panel rebuilt at each boundary
    "kept77_one_workgroup": (200, 40, (0.5, 1.0 / 3.0, 0.25), _pick(200, 77), lambda e, g: (th.arange(e) * 3) // e),
    # exactly 32 kept edges of one class: one full tile, no padding
    "one_full_tile": (64, 16, (0.5,), _pick(64, 32), lambda e, g: th.zeros(e, dtype=th.long)),
    "no_tiles": (200, 40, (0.5, 0.25), lambda g: th.zeros(0, dtype=th.long), lambda e, g: th.zeros(e, dtype=th.long)),
    # ~800 tiles over 256 workgroups (4 per workgroup, the last range short), 25 k kept of 55 k edge rows (the headline's kept share)
    "tiles800": (55000, 9000, (1.0, 0.5, 1.0 / 3.0, 0.25, 0.2, 1.0 / 6.0, 1.0 / 7.0), _pick(55000, 25490),
                 lambda e, g: th.randint(0, 7, (e,), generator=g)),
}
_CASES = {}


def _case(name):
    """Inputs (column blocks of wider buffers, NaN in every dead row), weights, tile lists and the fp64 results of one shape: made once."""
    if name in _CASES:
        return _CASES[name]
    E, N, coefs, pick, classes = SHAPES[name]
    g = th.Generator().manual_seed(len(name) + E)
    kept = pick(g)
    cls = classes(E, g)
    keep = th.zeros(E, dtype=th.bool)
    keep[kept] = True
    r = lambda *s: th.randn(*s, generator=g)
    c = dict(E=E, N=N, kept=kept, keep=keep)
    c["Wes"], c["W2t"], c["be"], c["b2"] = r(H, 2 * H) / (2 * H) ** 0.5, r(H, H) / H ** 0.5, r(H), r(H)
    c["zw"], c["XP"] = r(E, H + 8), r(N, 3 * H)                  # z = zw[:, 4:4 + H]; P = XP[:, H:] (ldp = 3H, as in the layer)
    c["zw"][~keep] = float("nan")
    # the nodes no kept edge selects are dead rows of P: NaN there too
    c["selA"] = th.randint(0, N, (E,), generator=g).to(th.int32)
    c["selB"] = th.randint(0, N, (E,), generator=g).to(th.int32)
    c["selA"][kept[::7]] = -1                                    # (a selector of a node whose row was never written reads as zeros)
    live = th.zeros(N, dtype=th.bool)
    for sel in (c["selA"], c["selB"]):
        ids = sel[kept].long()
        live[ids[ids >= 0]] = True
    c["XP"][~live] = float("nan")
    c["class_tiles"] = _class_tiles(kept, cls, coefs, E)
    c["asc_tiles"] = _ascending_tiles(kept, E)
    d = lambda t: t.double()
    z, P = d(c["zw"][keep][:, 4:4 + H]), d(c["XP"][:, H:])
    ce = th.tensor(coefs, dtype=th.float64)[cls[keep]].view(-1, 1)
    Wes = d(c["Wes"])
    a, b = c["selA"][keep].long(), c["selB"][keep].long()
    pa = th.where((a >= 0).view(-1, 1), P[a.clamp(min=0), :H], th.zeros(1, dtype=th.float64))
    pb = th.where((b >= 0).view(-1, 1), P[b.clamp(min=0), H:], th.zeros(1, dtype=th.float64))
    # (the kernel's panel is the fp32 sum A' + c B': the fp64 reference takes the exact one -- the difference is within the bound)
    h1 = th.nn.functional.leaky_relu(z @ Wes[:, :H] + ce * (z @ Wes[:, H:]) + pa - pb + d(c["be"]), SLOPE)
    c["ref"] = dict(H1e=h1, zn=z + h1 @ d(c["W2t"]) + d(c["b2"]))
    _CASES[name] = c
    return c


def _dev(c, gpu):
    g = lambda t: t.to(gpu)
    zw, XP = g(c["zw"]), g(c["XP"])
    return dict(z=zw[:, 4:4 + H], P=XP[:, H:], Wes=g(c["Wes"]), W2t=g(c["W2t"]), be=g(c["be"]), b2=g(c["b2"]),
                sel=(g(c["selA"]), g(c["selB"])), ct=tuple(g(t) if th.is_tensor(t) else t for t in c["class_tiles"]),
                at=tuple(g(t) if th.is_tensor(t) else t for t in c["asc_tiles"]))


class _LiveTiles:
    """``fused.live_tiles`` answering with the hand-made class tiles while the two launches run (``edge_fwd_typed`` asks for them)."""

    def __init__(self, fused, tiles):
        self.fused, self.tiles = fused, tiles

    def __enter__(self):
        self.real = self.fused.live_tiles
        self.fused.live_tiles = lambda index, coef, gate: self.tiles

    def __exit__(self, *exc):
        self.fused.live_tiles = self.real


def _check(name, what, got, old, ref, keep):
    """Kept rows: bit for bit the two launches', and against fp64; dead rows: bit for bit the sentinel."""
    got_c, old_c = got.cpu(), old.cpu()
    bound = 1e-5 * max(1.0, float(ref.abs().max())) if ref.numel() else 0.0
    e_new = float((got_c[keep].double() - ref).abs().max()) if ref.numel() else 0.0
    e_old = float((old_c[keep].double() - ref).abs().max()) if ref.numel() else 0.0
    print("%s %s: one launch %.3e  two launches %.3e  bound %.3e" % (name, what, e_new, e_old, bound))
    assert bool(th.isfinite(got_c[keep]).all()), what
    assert th.equal(got_c[keep], old_c[keep]), what + ": differs from the two launches"
    assert e_new <= bound, (what, e_new, e_old, bound)
    assert bool((got_c[~keep] == SENT).all()), what + ": a dead row was written"


@pytest.mark.parametrize("name", list(SHAPES))
def test_one_launch_against_the_two_launches_and_fp64(name, gpu):
    from dualmessagepassing_amd import fused
    c = _case(name)
    d = _dev(c, gpu)
    E, N, keep = c["E"], c["N"], c["keep"]
    ix = _Index(N, E)
    assert fused.edge_mlp_fwd_ok(H, d["z"], d["P"], d["W2t"])
    ldp = d["P"].stride(0)
    assert ldp == 3 * H

    def run():
        h1 = th.full((E, H + 4), SENT, device=gpu)               # (outputs: column blocks of wider buffers as well)
        zn = th.full((E, H + 4), SENT, device=gpu)
        fused.edge_mlp_fwd(d["z"], d["Wes"], d["P"], ldp, d["be"], None, ix, SLOPE, d["W2t"], d["b2"], d["z"], d["ct"], sel=d["sel"],
                           h1=h1[:, :H], out=zn[:, 4:])
        return h1, zn

    if name == "kept77_one_workgroup":
        d["ct"] = d["ct"][:3] + (1,)
    h1w, znw = run()
    # the two launches of the present route: the class tiles, then the kept rows in ascending order
    gate = th.ones(E, device=gpu)
    with _LiveTiles(fused, tuple(g_ for g_ in d["ct"][:3]) + (c["class_tiles"][3],)):
        real = fused.dead_rows_buffer
        fused.dead_rows_buffer = lambda shape, dev: th.full(shape, SENT, dtype=th.float32, device=dev)
        try:
            oh1 = fused.edge_fwd_typed(d["z"].contiguous(), d["Wes"], d["P"], ldp, d["be"], None, ix, SLOPE, dead_gate=gate, sel=d["sel"])
        finally:
            fused.dead_rows_buffer = real
    ozn = th.full((E, H), SENT, device=gpu)
    fused.out_fwd_typed(oh1, d["W2t"], d["b2"], d["z"], d["at"], out=ozn)
    _check(name, "H1e", h1w[:, :H], oh1, c["ref"]["H1e"], keep)
    _check(name, "zn", znw[:, 4:], ozn, c["ref"]["zn"], keep)
    assert bool((h1w[:, H:] == SENT).all()) and bool((znw[:, :4] == SENT).all()), "the columns beside an output were written"
    # repeatability: the same bits on a second launch
    h1b, znb = run()
    assert th.equal(h1b, h1w) and th.equal(znb, znw)


def test_fallback_conditions(gpu):
    """The switch, another width, a row stride the descriptors cannot take, another dtype: the two launches stand."""
    from dualmessagepassing_amd import fused
    a = th.zeros(64, H, device=gpu)
    assert fused.edge_mlp_fwd_ok(H, a, None)
    assert not fused.edge_mlp_fwd_ok(64, th.zeros(64, 64, device=gpu))
    assert not fused.edge_mlp_fwd_ok(H, a.double())
    assert not fused.edge_mlp_fwd_ok(H, th.zeros(64, H + 2, device=gpu)[:, :H])
    fused.USE_EDGE_MLP_FWD = False
    try:
        assert not fused.edge_mlp_fwd_ok(H, a)
    finally:
        fused.USE_EDGE_MLP_FWD = True


def _forward_loss_backward(shard, step, model):
    """One step of bench.py's front half on the shard: forward, ``count_loss``, backward, gradient pack -> (pred_c, flat gradients)."""
    from dualmessagepassing_amd.collate import collate_device
    from dualmessagepassing_amd.harness import count_loss
    p, g = shard["p"], shard["g"]
    pattern = collate_device(p["local_src"], p["local_dst"], p["num_nodes"].clone(), p["num_edges"].clone(), p["N"], p["E"],
                             ndata=p["ndata"], edata=dict(p["edata"]), max_nodes=p["max_n"], max_edges=p["max_e"])
    graph = collate_device(g["local_src"], g["local_dst"], g["num_nodes"].clone(), g["num_edges"].clone(), g["N"], g["E"],
                           ndata=g["ndata"], edata=dict(g["edata"]), max_nodes=g["max_n"], max_edges=g["max_e"])
    step.sync.detach_grads()
    out = model(pattern, graph)
    pred = out["pred_c"].detach().clone()
    count_loss(out["pred_c"].view(-1), shard["counts"]).backward()
    step.sync.pack()
    return pred.cpu(), step.sync.flat.detach().cpu().clone()


def test_model_with_the_one_launch_equals_the_model_without_it(gpu):
    """bench.py's model (hid 128, ScalarFilter, 3 layers) on 8 pairs, forward + ``count_loss`` + backward, with ``USE_EDGE_MLP_FWD`` on
    against off: ``pred_c`` and every parameter gradient bit for bit.  On, the one-launch wrapper is reached; off, it is not."""
    from dualmessagepassing_amd import fused
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_compact import _model_and_batch
    sys.path.insert(0, ROOT)
    import bench
    cfg = dict(bench.CFG, batch=8)
    mc = bench.model_config(cfg)
    assert (mc["hid_dim"], mc["filter_net"], mc["rep_num_graph_layers"]) == (128, "ScalarFilter", 3)
    _, shard, step, model = _model_and_batch(cfg, gpu)
    ran = []
    real = fused.edge_mlp_fwd
    fused.edge_mlp_fwd = lambda *a, **k: (ran.append(1), real(*a, **k))[1]
    try:
        fused.USE_EDGE_MLP_FWD = False
        try:
            ref_pred, ref_flat = _forward_loss_backward(shard, step, model)
        finally:
            fused.USE_EDGE_MLP_FWD = True
        assert not ran, "the one-launch edge MLP ran although it was switched off"
        pred, flat = _forward_loss_backward(shard, step, model)
        assert ran, "the one-launch edge MLP did not run"
        assert bool(th.isfinite(pred).all()) and bool(th.isfinite(flat).all())
        assert th.equal(pred, ref_pred)
        for prm, off in zip(step.sync.params, step.sync.offsets):
            assert th.equal(flat[off:off + prm.numel()], ref_flat[off:off + prm.numel()]), off
    finally:
        fused.edge_mlp_fwd = real
