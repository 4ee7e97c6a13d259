"""A layer's node side over the kept nodes' tiles as ONE launch per pass (csrc/dmp_nodechain.hip: ``fused.node_chain_fwd`` /
``fused.node_chain_bwd``) against fp64 and against the three-launch chain it replaces, on hand-made tile lists.

Bounds.  Every output: ``1e-5 * max(1, |ref|max)`` against torch fp64 on the CPU; the three-launch chain's error is
measured in the same test and the new launch is allowed twice that where it is the larger figure.  Column sums: ``2e-6`` of the
column's sum of magnitudes (|dxn| |W2| for the sums of dPn), the figure the tile kernels' own tests use.  Both launches' errors
are printed before they are asserted."""
import os
import sys

import pytest
import torch as th

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 128
SLOPE = 1.0 / 5.5
SENT = 7.5


def _tiles(kept, N, gpu):
    """``(slot, tile_scale, num_tiles, bound)`` as ``NodeRows.tiles``: 32 slots per tile, -1 = padding, the tile count on the device."""
    bound = (N + 31) // 32
    slot = th.full((bound * 32,), -1, dtype=th.int32)
    slot[:kept.numel()] = kept.to(th.int32)
    nt = (kept.numel() + 31) // 32
    return slot.to(gpu), th.zeros(bound, device=gpu), th.tensor([nt], dtype=th.int32, device=gpu), bound


SHAPES = {
    "scattered77": (200, lambda g: th.randperm(200, generator=g)[:77].sort().values),       # 3 tiles, the last one padded
    "one_full_tile": (64, lambda g: th.randperm(64, generator=g)[:32].sort().values),       # exactly 32 kept rows
    "no_tiles": (200, lambda g: th.zeros(0, dtype=th.long)),
    "tiles1300": (45000, lambda g: th.randperm(45000, generator=g)[:1300 * 32 - 5].sort().values),   # 6 tiles per workgroup: 4 + 2, the last range short
}
_CASES = {}


def _case(name, gpu):
    """Inputs (column blocks of wider buffers, NaN in every dead row), weights and the fp64 results of one shape: made once."""
    if name in _CASES:
        return _CASES[name]
    N, pick = SHAPES[name]
    g = th.Generator().manual_seed(len(name) + N)
    kept = pick(g)
    keep = th.zeros(N, dtype=th.bool)
    keep[kept] = True
    r = lambda *s: th.randn(*s, generator=g)
    c = dict(N=N, kept=kept, keep=keep)
    c["Wx"], c["Bn"], c["W2"] = r(H, 3 * H) / (3 * H) ** 0.5, r(2 * H, H) / (3 * H) ** 0.5, r(H, H) / H ** 0.5
    c["bn"], c["b2"] = r(H), r(H)
    wide = dict(x=r(N, H + 8), S=r(N, 3 * H), dxn=r(N, H + 4), dP=r(N, 3 * H), H1=r(N, H))
    for v in wide.values():
        v[~keep] = float("nan")
    c["wide"] = wide
    x, S, dxn, dP, H1 = wide["x"][:, 4:4 + H], wide["S"][:, H:], wide["dxn"][:, :H], wide["dP"][:, H:], wide["H1"]
    k = keep
    d = lambda t: t.double()
    Wx, Bn, W2 = d(c["Wx"]), d(c["Bn"]), d(c["W2"])
    h1 = th.nn.functional.leaky_relu(d(x[k]) @ Wx[:, :H] + d(S[k]) @ Bn + d(c["bn"]), SLOPE)
    c["ref_f"] = dict(H1n=h1, P=d(x[k]) @ Wx[:, H:], xn=d(x[k]) + h1 @ W2.t() + d(c["b2"]))
    dh = d(dxn[k]) @ W2
    dpn = th.where(d(H1[k]) > 0, dh, SLOPE * dh)
    c["ref_b"] = dict(dPn=dpn, dS=th.cat([dpn @ Bn[:H].t(), dpn @ Bn[H:].t()], 1),
                      dx=d(dxn[k]) + dpn @ Wx[:, :H].t() + d(dP[k]) @ Wx[:, H:].t(),
                      dbn=dpn.sum(0), db2n=d(dxn[k]).sum(0),
                      dbn_scale=(d(dxn[k]).abs() @ W2.abs()).sum(0), db2n_scale=d(dxn[k]).abs().sum(0))
    _CASES[name] = c
    return c


def _dev(c, gpu):
    w = {n: v.to(gpu) for n, v in c["wide"].items()}
    return (w["x"][:, 4:4 + H], w["S"][:, H:], w["dxn"][:, :H], w["dP"][:, H:], w["H1"],
            c["Wx"].to(gpu), c["Bn"].to(gpu), c["W2"].to(gpu), c["bn"].to(gpu), c["b2"].to(gpu))


def _check(name, what, got, old, ref, keep):
    """Kept rows against fp64 (the new launch and the three-launch chain), dead rows bit for bit the sentinel."""
    bound = 1e-5 * max(1.0, float(ref.abs().max())) if ref.numel() else 0.0
    e_new = float((got.cpu()[keep].double() - ref).abs().max()) if ref.numel() else 0.0
    e_old = float((old.cpu()[keep].double() - ref).abs().max()) if ref.numel() else 0.0
    print("%s %s: chain %.3e  three launches %.3e  bound %.3e" % (name, what, e_new, e_old, bound))
    assert bool(th.isfinite(got.cpu()[keep]).all()), what
    assert e_new <= max(bound, 2.0 * e_old), (what, e_new, e_old, bound)
    assert bool((got.cpu()[~keep] == SENT).all()), what + ": a dead row was written"


def _buffers(N, gpu):
    XP = th.full((N, 3 * H), SENT, device=gpu)
    return th.full((N, H), SENT, device=gpu), XP, th.full((N, H), SENT, device=gpu)


@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_chain_against_fp64_and_the_three_launches(name, gpu):
    from dualmessagepassing_amd import fused
    c = _case(name, gpu)
    x, S, _, _, _, Wx, Bn, W2, bn, b2 = _dev(c, gpu)
    N, keep = c["N"], c["keep"]
    T = _tiles(c["kept"], N, gpu)
    assert fused.node_chain_ok(H, x, S, Bn, Wx, W2)
    pf, _ = fused.node_chain_panels(Bn, Wx, W2)
    H1n, XP, xn = _buffers(N, gpu)
    fused.node_chain_fwd(x, S, pf, bn, b2, True, SLOPE, T, H1n, XP[:, H:], xn)            # (P: a column block, ld = 3H)
    # the three launches of the present chain
    oH1, oXP, oxn = _buffers(N, gpu)
    T1 = th.full((N, H), SENT, device=gpu)
    fused.typed_jobs([dict(a=x, W=Wx[:, :H], bias=bn, out=oXP[:, :H]), dict(a=S[:, :H], W=Bn[:H], out=T1),
                      dict(a=x, W=Wx[:, H:2 * H], out=oXP[:, H:2 * H]), dict(a=x, W=Wx[:, 2 * H:], out=oXP[:, 2 * H:])], T)
    fused.out_fwd_typed(S[:, H:], Bn[H:], None, oXP[:, :H], T, out=oH1, slope=SLOPE, prev2=T1)
    fused.out_fwd_typed(oH1, W2, b2, x, T, out=oxn, w_in_out=False)
    ref = c["ref_f"]
    _check(name, "H1n", H1n, oH1, ref["H1n"], keep)
    _check(name, "P", XP[:, H:], oXP[:, H:], ref["P"], keep)
    _check(name, "xn", xn, oxn, ref["xn"], keep)
    assert bool((XP[:, :H] == SENT).all()), "the block beside P was written"
    # repeatability: the same bits on a second launch
    H1b, XPb, xnb = _buffers(N, gpu)
    fused.node_chain_fwd(x, S, pf, bn, b2, True, SLOPE, T, H1b, XPb[:, H:], xnb)
    assert th.equal(H1b, H1n) and th.equal(XPb, XP) and th.equal(xnb, xn)
    # without the residual
    H1c, XPc, xnc = _buffers(N, gpu)
    fused.node_chain_fwd(x, S, pf, bn, b2, False, SLOPE, T, H1c, XPc[:, H:], xnc)
    want = ref["xn"] - x.cpu()[keep].double()
    assert th.equal(H1c, H1n)
    if want.numel():
        assert float((xnc.cpu()[keep].double() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("name", list(SHAPES))
def test_backward_chain_against_fp64_and_the_three_launches(name, gpu):
    from dualmessagepassing_amd import fused
    c = _case(name, gpu)
    x, _, dxn, dP, H1, Wx, Bn, W2, _, _ = _dev(c, gpu)
    N, keep = c["N"], c["keep"]
    T = _tiles(c["kept"], N, gpu)
    assert fused.node_chain_ok(H, dxn, H1, dP)
    _, pb = fused.node_chain_panels(Bn, Wx, W2)

    def run(with_dx=True):
        dXP = th.full((N, 3 * H), SENT, device=gpu)
        dXP[:, H:] = dP                                                                   # (the kept-incidence sums wrote it)
        dSw = th.full((N, 2 * H + 4), SENT, device=gpu)
        dx = th.full((N, H), SENT, device=gpu)
        with fused.deferred_reductions():
            dbn, db2n = fused.node_chain_bwd(dxn, H1, dXP[:, H:], pb, True, SLOPE, T, dXP[:, :H], dSw[:, :2 * H], dx if with_dx else None)
        return dXP, dSw, dx, dbn, db2n

    dXP, dSw, dx, dbn, db2n = run()
    # the launches of the present chain
    oXP = th.full((N, 3 * H), SENT, device=gpu)
    oXP[:, H:] = dP
    oS, oU, odx = th.full((N, 2 * H), SENT, device=gpu), th.full((N, 2 * H), SENT, device=gpu), th.full((N, H), SENT, device=gpu)
    _, obn, ob2 = fused.bwd_h1_typed(dxn, W2, H1, T, SLOPE, out=oXP[:, :H])
    fused.typed_jobs([dict(a=oXP[:, :H], W=Bn[:H], w_in_out=False, out=oS[:, :H]), dict(a=oXP[:, :H], W=Bn[H:], w_in_out=False, out=oS[:, H:]),
                      dict(a=oXP[:, :H], W=Wx[:, :H], w_in_out=False, prev=dxn, out=oU[:, :H]),
                      dict(a=oXP[:, H:2 * H], W=Wx[:, H:2 * H], w_in_out=False, out=oU[:, H:])], T)
    fused.out_fwd_typed(oXP[:, 2 * H:], Wx[:, 2 * H:], None, oU[:, :H], T, out=odx, w_in_out=False, prev2=oU[:, H:])
    ref = c["ref_b"]
    _check(name, "dPn", dXP[:, :H], oXP[:, :H], ref["dPn"], keep)
    _check(name, "dS", dSw[:, :2 * H], oS, ref["dS"], keep)
    _check(name, "dx", dx, odx, ref["dx"], keep)
    assert bool((dSw[:, 2 * H:] == SENT).all()), "the columns beside dS were written"
    same = lambda a, b: th.equal(a.view(th.int32), b.view(th.int32))                       # bit for bit (the dead rows of dP hold NaN)
    assert same(dXP[:, H:].contiguous(), dP.contiguous()), "dP was written"
    # the bias partials, reduced: fp64 column sums over the kept rows
    for what, got, old, want, scale in (("dbn", dbn, obn, ref["dbn"], ref["dbn_scale"]), ("db2n", db2n, ob2, ref["db2n"], ref["db2n_scale"])):
        e_new, e_old = float((got.cpu().double() - want).abs().max()), float((old.cpu().double() - want).abs().max())
        tol = 2e-6 * max(1.0, float(scale.max())) if scale.numel() else 0.0
        print("%s %s: chain %.3e  three launches %.3e  bound %.3e" % (name, what, e_new, e_old, tol))
        assert e_new <= tol, (what, e_new, tol)
    # repeatability
    dXP2, dSw2, dx2, dbn2, db2n2 = run()
    assert same(dXP2, dXP) and th.equal(dSw2, dSw) and th.equal(dx2, dx) and th.equal(dbn2, dbn) and th.equal(db2n2, db2n)
    # without dx: dx untouched, the other outputs equal
    dXP3, dSw3, dx3, dbn3, db2n3 = run(with_dx=False)
    assert bool((dx3 == SENT).all())
    assert same(dXP3, dXP) and th.equal(dSw3, dSw) and th.equal(dbn3, dbn) and th.equal(db2n3, db2n)


def test_fallback_conditions(gpu):
    """The switch, another width, a row stride the descriptors cannot take, another dtype: the three-launch chain stands."""
    from dualmessagepassing_amd import fused
    a = th.zeros(64, H, device=gpu)
    assert fused.node_chain_ok(H, a, None)
    assert not fused.node_chain_ok(64, th.zeros(64, 64, device=gpu))
    assert not fused.node_chain_ok(H, a.double())
    assert not fused.node_chain_ok(H, th.zeros(64, H + 2, device=gpu)[:, :H])
    fused.USE_NODE_CHAIN = False
    try:
        assert not fused.node_chain_ok(H, a)
    finally:
        fused.USE_NODE_CHAIN = True


def test_model_with_the_chain_equals_the_model_without_it(gpu):
    """bench.py's model on 80 pairs (5,760 union node rows: the kept-node path runs) with ``USE_NODE_CHAIN`` on against off -- the
    bounds of tests/test_gpu_node_rows.py: all 15 outputs within 2e-5, every parameter gradient within 5e-5 of its largest entry --
    and once more with the dead rows poisoned.  Off, the new launches do not run and the old chain gives the reference."""
    from dualmessagepassing_amd import fused
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_compact import _model_and_batch, _outputs_and_grads
    sys.path.insert(0, ROOT)
    import bench
    cfg = dict(bench.CFG, batch=80)
    bench_, shard, step, model = _model_and_batch(cfg, gpu)
    ran = []
    real_f, real_b = fused.node_chain_fwd, fused.node_chain_bwd
    fused.node_chain_fwd = lambda *a, **k: (ran.append("f"), real_f(*a, **k))[1]
    fused.node_chain_bwd = lambda *a, **k: (ran.append("b"), real_b(*a, **k))[1]
    try:
        fused.USE_NODE_CHAIN = False
        try:
            ref_out, ref_flat = _outputs_and_grads(bench_, cfg, shard, step, model, True)
        finally:
            fused.USE_NODE_CHAIN = True
        assert not ran, "the chain ran although it was switched off"
        for poison in (False, True):
            del ran[:]
            fused.POISON_DEAD_ROWS = poison
            try:
                out, flat = _outputs_and_grads(bench_, cfg, shard, step, model, True)
            finally:
                fused.POISON_DEAD_ROWS = False
            assert ran.count("f") >= 2 and ran.count("b") >= 2, "the chain did not run: %r" % (ran,)
            for k, v in ref_out.items():
                if v is None:
                    assert out[k] is None
                    continue
                assert bool(th.isfinite(out[k]).all()), k
                s = max(1e-6, float(v.abs().max()))
                assert float((out[k] - v).abs().max()) <= 2e-5 * s, (k, float((out[k] - v).abs().max()), s)
            assert bool(th.isfinite(flat).all())
            for prm, off in zip(step.sync.params, step.sync.offsets):
                a, b = flat[off:off + prm.numel()], ref_flat[off:off + prm.numel()]
                s = float(b.abs().max())
                if s == 0.0:
                    assert float(a.abs().max()) == 0.0
                else:
                    assert float((a - b).abs().max()) <= 5e-5 * s, (off, float((a - b).abs().max()), s)
    finally:
        fused.node_chain_fwd, fused.node_chain_bwd = real_f, real_b
