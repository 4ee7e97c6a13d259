"""``fused.gate_bundle``: the index arrays a step derives from its two 0 / 1 gates -- both row masks, the kept nodes' tile list, the
first layer's kept target rows, the kept edges' ascending tile list, the selectors with dead nodes as -1 -- built in three launches
(``dmp_row_mask_bits_jobs``, ``dmp_kept_rows_jobs``) against the ten single launches they replace: every array equal, bit for bit.
The arrays index the scatter-adds of SubgraphCountingMatching/models/dmpnn.py:92,163 under the ScalarFilter gates of
basemodel.py:1515-1531."""
import numpy as np
import pytest
import torch as th

pytestmark = pytest.mark.gpu


def _t(a):
    return th.from_numpy(np.ascontiguousarray(a))


def _case(n, e, ep, seed, gpu, keep_v=0.4, keep_e=0.45):
    from dualmessagepassing_amd import gatememo
    from dualmessagepassing_amd.graph import GraphIndex
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, n, e).astype(np.int64), rng.integers(0, n, e).astype(np.int64)
    ix = GraphIndex(_t(src).to(gpu), _t(dst).to(gpu), n, _t(rng.random(e) < 0.5).to(gpu), validate=True)
    vg = _t((rng.random(n) < keep_v).astype(np.float32)).to(gpu)
    eg = _t((rng.random(e) < keep_e).astype(np.float32)).to(gpu)
    eg[:ep] = 1.0
    for g in (vg, eg):
        gatememo.mark(g, binary=True, zero_rows=True)
    return ix, vg, eg


@pytest.mark.parametrize("n,e,ep", [(5000, 70000, 32 * 40), (4096, 40001, 0), (73728, 548864, 24576), (33, 64, 32)])
def test_bundle_equals_the_single_launches(n, e, ep, gpu):
    from dualmessagepassing_amd import fused, gatememo
    got = {}
    for on in (False, True):
        ix, vg, eg = _case(n, e, ep, n + e, gpu)
        saved = fused.USE_GATE_BUNDLE
        fused.USE_GATE_BUNDLE = on
        try:
            fused.gate_bundle(ix, vg, eg, want_nodes=True, l0_range=(ep, e), want_ascending=True)
            vm = gatememo.peek(vg, "row_mask")
            planted = on and vm is not None and gatememo.peek(ix, "edge_select_nodes", (vm,)) is not None
            vm, em = fused.gate_row_mask(vg), fused.gate_row_mask(eg)
            nodes = fused.kept_rows(vm, 0, n, tiles=True)
            l0 = fused.kept_rows(em, ep, e)
            asc = fused.kept_rows(em, 0, e, tiles=True)
            sel = ix.edge_select_nodes(vm)
        finally:
            fused.USE_GATE_BUNDLE = saved
        assert planted == on
        th.cuda.synchronize()
        nk, ek = int(nodes[1][0]), int(asc[1][0])
        got[on] = dict(vm=vm.clone(), em=em.clone(), nodes=nodes[0][:(nk + 31) // 32 * 32].clone(), ncnt=nodes[1].clone(),
                       l0=l0[0][:int(l0[1][0])].clone(), l0cnt=l0[1].clone(), asc=asc[0][:(ek + 31) // 32 * 32].clone(), acnt=asc[1].clone(),
                       selA=sel[0].clone(), selB=sel[1].clone(), dstM=sel[2].clone())
    for k in got[False]:
        assert th.equal(got[False][k], got[True][k]), k
    # ... and they are what they say: the kept nodes ascending, padded with -1 to whole tiles
    keep = (_case(n, e, ep, n + e, gpu)[1] != 0).nonzero().view(-1).int()
    assert th.equal(got[True]["nodes"][:keep.numel()], keep) and bool((got[True]["nodes"][keep.numel():] == -1).all())
    assert got[True]["ncnt"].tolist() == [keep.numel(), (keep.numel() + 31) // 32]


def test_bundle_leaves_what_it_is_not_asked_for(gpu):
    from dualmessagepassing_amd import fused, gatememo
    ix, vg, eg = _case(6000, 50000, 3200, 9, gpu)
    fused.gate_bundle(ix, vg, eg, want_nodes=False, l0_range=None, want_ascending=False)
    vm, em = fused.gate_row_mask(vg), fused.gate_row_mask(eg)          # the masks are there ...
    assert vm is not None and em is not None
    assert gatememo.names(ix) == () and gatememo.names(vm) == () and gatememo.names(em) == ()
    ref_v = ((vg.view(-1, 1) != 0) if False else None)
    bits = ((vm.view(-1, 1).to(th.int64) >> th.arange(32, device=gpu)) & 1).reshape(-1)[:6000].float()
    assert th.equal(bits, (vg != 0).float())
    # a dense gate: nothing is built (every consumer takes its unmasked form)
    ix2, vg2, eg2 = _case(6000, 50000, 3200, 10, gpu)
    gatememo.mark(eg2, dense=True)
    fused.gate_bundle(ix2, vg2, eg2, want_nodes=True, l0_range=(3200, 50000), want_ascending=True)
    assert gatememo.peek(vg2, "row_mask") is None and gatememo.names(ix2) == ()


def _tiny(gpu, seed=5):
    """70 nodes (three node tiles, the last ragged), 333 edges (a ragged last tile and a ragged last mask word), of which the first
    64 are the pattern's (the smallest aligned ``l0_range`` start above zero): the pattern's 20 nodes and 64 edges kept, the rest
    under random 0 / 1 gates."""
    from dualmessagepassing_amd import gatememo, ops
    from dualmessagepassing_amd.graph import GraphIndex
    n, e, ep = 70, 333, 64
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, n, e).astype(np.int64), rng.integers(0, n, e).astype(np.int64)
    ix = GraphIndex(_t(src).to(gpu), _t(dst).to(gpu), n, _t(rng.random(e) < 0.5).to(gpu), validate=True)
    vg = _t((rng.random(n) < 0.5).astype(np.float32)).to(gpu)
    eg = _t((rng.random(e) < 0.45).astype(np.float32)).to(gpu)
    vg[:20] = 1.0
    eg[:ep] = 1.0
    for g in (vg, eg):
        gatememo.mark(g, binary=True, zero_rows=True)
    coef = ix.degree_coef(ix.out_deg)
    pool = ops.PoolIndex(th.tensor([ep, 100, 0, e - ep - 100], dtype=th.int64, device=gpu), None, num_rows=e)
    return ix, vg, eg, coef, pool


def _products(ix, vg, eg, coef, pool, H=64):
    """Every index array the step derives from the two gates, by name, as its getter returns it."""
    from dualmessagepassing_amd import fused
    n, e, ep = ix.num_nodes, ix.num_edges, 64
    vm, em = fused.gate_row_mask(vg), fused.gate_row_mask(eg)
    nd = fused.node_rows(ix, vg, H)
    assert vm is not None and em is not None and nd is not None
    got = dict(vmask=vm, emask=em, node_tiles=fused.kept_rows(vm, 0, n, tiles=True), l0_rows=fused.kept_rows(em, ep, e),
                ascending_tiles=fused.ascending_tiles(eg), live_tiles=fused.live_tiles(ix, coef, eg), keep_in_csr=fused.keep_in_csr(ix, eg),
                node_rows=nd, kept_incidence=nd.kept_incidence(ix, eg), kept_incidence_in=nd.kept_incidence(ix, eg, in_only=True),
                masked_slots=fused.masked_slots(ix, coef, eg), pool_weight_sums=fused.pool_weight_sums(pool, eg),
                keep_pool_csr=fused.keep_pool_csr(pool, eg))
    assert all(v is not None for v in got.values()), got
    return got


def _parts(v):
    return list(v) if isinstance(v, tuple) else [v]


def _written(name, v):
    """The entries of product ``v`` its build wrote (lists and CSRs are allocated for the worst case), as host values."""
    if name in ("node_tiles", "ascending_tiles", "live_tiles"):              # tile slot lists: whole tiles, padded with -1
        tiles = int(v[2][0]) if len(v) == 4 else int(v[1][1])
        return [v[0][:32 * tiles].tolist()] + ([v[1][:tiles].tolist(), v[2].tolist(), v[3]] if len(v) == 4 else [v[1].tolist()])
    if name == "l0_rows":
        return [v[0][:int(v[1][0])].tolist(), v[1].tolist()]
    if name in ("keep_in_csr", "keep_pool_csr"):
        return [v[0].tolist(), v[1][:int(v[0][-1])].tolist()]
    if name == "node_rows":
        kept = int(v.rows[1][0])
        return [v.mask.tolist(), v.rows[0][:kept].tolist(), v.rows[1].tolist(), v.tiles[2].tolist(), v.tiles[3], [s.tolist() for s in v.sel], v.prefix]
    return [t.tolist() for t in _parts(v)]


def _all_written(p, ix, coef):
    th.cuda.synchronize()
    out = {k: _written(k, v) for k, v in p.items() if k != "masked_slots" and not k.startswith("kept_incidence")}
    out["masked_slots"] = p["masked_slots"][:32 * int(ix.class_tiles(coef)[2][0])].tolist()        # (the slots of the tiles in use)
    kept = int(p["node_rows"].rows[1][0])
    for k in ("kept_incidence", "kept_incidence_in"):                        # a row per POSITION in the kept nodes' list
        out[k] = [p[k][0][:kept + 1].tolist(), p[k][1][:int(p[k][0][kept])].tolist()]
    return out


def test_every_getter_finds_what_it_built_until_the_gate_changes(gpu):
    """Each product is built once per version of its gate: a second call returns the SAME objects; after an in-place write to
    the edge gate (same values) its products are new objects with the same contents, the node gate's stay."""
    case = _tiny(gpu)
    ix, vg, eg, coef = case[:4]
    first, second = _products(*case), _products(*case)
    for k in first:
        a, b = _parts(first[k]), _parts(second[k])
        assert len(a) == len(b) and all(x is y for x, y in zip(a, b)), k
    assert first["node_rows"].prefix == 0 and first["node_tiles"][0] is first["node_rows"].tiles[0]
    before = _all_written(first, ix, coef)
    eg.mul_(1)
    third = _products(*case)
    for k in ("vmask", "node_tiles", "node_rows"):
        assert all(x is y for x, y in zip(_parts(first[k]), _parts(third[k]))), k
    for k in set(first) - {"vmask", "node_tiles", "node_rows"}:
        assert not any(x is y for x, y in zip(_parts(first[k]), _parts(third[k]))
                       if th.is_tensor(x)), k
    assert _all_written(third, ix, coef) == before


def test_bundle_plants_what_every_getter_then_finds(gpu):
    """With the bundle on, every product it was asked for is in its getter's memo BEFORE the getter is called -- the getter
    returns that very object -- and every getter's result has the bits it has with the bundle off."""
    from dualmessagepassing_amd import fused, gatememo
    got = {}
    for on in (False, True):
        case = _tiny(gpu)
        ix, vg, eg = case[:3]
        n, e, ep = ix.num_nodes, ix.num_edges, 64
        saved = fused.USE_GATE_BUNDLE
        fused.USE_GATE_BUNDLE = on
        try:
            fused.gate_bundle(ix, vg, eg, want_nodes=True, l0_range=(ep, e), want_ascending=True)
            vm, em = gatememo.peek(vg, "row_mask"), gatememo.peek(eg, "row_mask")
            assert (vm is not None) == on and (em is not None) == on
            planted = {}
            if on:
                planted = dict(vmask=vm, emask=em, node_tiles=gatememo.peek(vm, fused.kept_rows_name(0, n, True)),
                               l0_rows=gatememo.peek(em, fused.kept_rows_name(ep, e)), asc=gatememo.peek(em, fused.kept_rows_name(0, e, True)),
                               sel=gatememo.peek(ix, "edge_select_nodes", (vm,)))
                assert all(v is not None for v in planted.values()), planted
            p = _products(*case)
        finally:
            fused.USE_GATE_BUNDLE = saved
        if on:
            assert p["vmask"] is planted["vmask"] and p["emask"] is planted["emask"]
            assert p["node_tiles"] is planted["node_tiles"] and p["l0_rows"] is planted["l0_rows"]
            assert p["ascending_tiles"][0] is planted["asc"][0] and p["node_rows"].tiles[0] is planted["node_tiles"][0]
            assert p["node_rows"].sel is planted["sel"]
        got[on] = _all_written(p, ix, case[3])
    assert got[True] == got[False]
