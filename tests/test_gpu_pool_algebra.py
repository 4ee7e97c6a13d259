"""The pooled last layer's per-graph algebra as three launches (``fused.pool_out``, ``rows_gemm``, ``pool_wgrad``; csrc/dmp_heads.hip).

A last layer that hands out per-graph sums only ends its forward with the second level of three pooled sums, a [G, H] x [H, H]
product, a bias row pass -- and starts its backward with another product, another second-level sum and two parameter gradients:
nine dependent launches on a few thousand rows.  Here: the three kernels against an fp64 restatement in torch (and the second-level
sums against ``pool_rows``, bit for bit), the layer with the route on against the route off, the host condition's fallbacks through
the timer's record names, and the model's step replayed from its recording.

Shapes: 1, 17 and 48 graphs (a tile of one row; two tiles, the second of one row; three full tiles) and, for the gradient kernel,
150 (five workgroups of 32 graphs, the last one ragged), graphs of 0, 40, 150 and 540 rows = 0, 1, 3 and 9 chunks of 64 (none; one; fewer than the four requested together;
more).  The fp64 bound, 2e-5 of the natural scale ``max sum |a||b|``, is the project's bound for such products
(tests/test_gpu_h1w_codes.py); the layer's figures are SURVEY section 8(c)'s and DESIGN.md section 5's."""
import os
import sys

import pytest
import torch as th

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 40, 150, 540)          # rows of a graph -> 0, 1, 3, 9 chunks


def _index(G, flagged, seed, gpu):
    """A pooling index over G graphs in row order, every chunk count of ``SIZES`` drawn (G = 1: three chunks), graph 2 of a
    larger batch empty; ``flagged``: with a reversed-edge flag on about half of the rows."""
    from dualmessagepassing_amd import ops
    gen = th.Generator().manual_seed(seed)
    if G == 1:
        sizes = th.tensor([SIZES[2]])
    else:
        sizes = th.tensor(SIZES)[th.randint(0, 4, (G,), generator=gen)]
        sizes[:4] = th.tensor(SIZES)[th.tensor([3, 1, 0, 2])]
    R = int(sizes.sum())
    flag = (th.rand(R, generator=gen) < 0.5).to(gpu) if flagged else None
    pool = ops.PoolIndex(sizes.to(gpu), flag, num_rows=R)
    assert pool.rows_in_order and pool.num_graphs == G
    return pool, R


def _padded(t, extra=3):
    """``t`` as the leading rows of a buffer with NaN rows behind it (rows past the chunk table must never be read)."""
    buf = th.full((t.size(0) + extra,) + tuple(t.shape[1:]), float("nan"), device=t.device)
    buf[:t.size(0)] = t
    return buf[:t.size(0)]


def _graph_sums64(part, pool, H):
    """fp64: the non-flagged half of a chunk table summed per graph, and the same of the absolute values."""
    gp = pool.gptr.long().cpu()
    ch = (pool.gent.long() >> 1)
    out = th.zeros(pool.num_graphs, H, dtype=th.float64, device=part.device)
    mag = th.zeros_like(out)
    for g in range(pool.num_graphs):
        rows = part[ch[gp[g]:gp[g + 1]], :H].double()
        out[g], mag[g] = rows.sum(0), rows.abs().sum(0)
    return out, mag


def _report(what, got, want, scale, lib_got=None):
    err = float((got.double() - want).abs().max()) if got.numel() else 0.0
    line = "%s: error %.3g, natural scale %.3g, ratio %.3g" % (what, err, scale, err / scale if scale else 0.0)
    if lib_got is not None:
        line += "; the replaced library route: error %.3g" % (float((lib_got.double() - want).abs().max()) if got.numel() else 0.0)
    print(line)
    assert bool(th.isfinite(got).all()), what
    assert err <= 2e-5 * scale, (what, err, scale)


@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("G", [1, 17, 48])
@pytest.mark.parametrize("flagged,with_z,with_x,with_b", [(True, True, True, True), (False, True, False, True), (True, False, True, False),
                                                          (False, False, False, False)])
def test_forward_kernel_against_fp64_and_pool_rows(H, G, flagged, with_z, with_x, with_b, gpu):
    from dualmessagepassing_amd import fused
    pool, R = _index(G, flagged, 11 * G + H, gpu)
    vpool, Rn = _index(G, False, 13 * G + H, gpu)
    gen = th.Generator().manual_seed(G + H)
    h1, z, xn = (th.randn(r, H, generator=gen).to(gpu) for r in (R, R, Rn))
    W2 = (th.randn(H, H, generator=gen) / H ** 0.5).to(gpu)
    b2 = th.randn(H, generator=gen).to(gpu) if with_b else None
    halves = 2 if flagged else 1
    gcnt = fused.pool_weight_sums(pool)
    assert gcnt.shape == (G, halves)
    partH, partZ, partX = (fused.pool_chunk_sums(t, p) for t, p in ((h1, pool), (z, pool), (xn, vpool)))
    want_q, want_zs, want_vs = fused.pool_rows(h1, pool)[:, :H], fused.pool_rows(z, pool)[:, :H], fused.pool_rows(xn, vpool)
    Q64, Qmag = _graph_sums64(partH, pool, H)
    Z64, Zmag = _graph_sums64(partZ, pool, H)
    dirty = []
    for p in (partH, partZ):                    # NaN in the flagged half and behind the table: neither may show
        p = _padded(p)
        if flagged:
            p[:, H:] = float("nan")
        dirty.append(p)
    es, vs, Q = fused.pool_out(dirty[0], dirty[1] if with_z else None, pool, gcnt, W2, b2, _padded(partX) if with_x else None,
                               vpool if with_x else None, want_q=True)
    assert th.equal(Q, want_q)                                         # the second level: pool_rows' bits
    if with_x:
        assert th.equal(vs, want_vs)
    else:
        assert vs is None
    want = Q64 @ W2.double().t()
    mag = Qmag @ W2.double().abs().t()
    lib = want_q @ W2.t()
    if with_z:
        want, mag, lib = want + Z64, mag + Zmag, th.addmm(want_zs, want_q, W2.t())
    if with_b:
        want = want + gcnt[:, :1].double() * b2.double()
        mag = mag + gcnt[:, :1].double() * b2.double().abs()
        lib = lib.addcmul(gcnt[:, :1], b2.view(1, H))
    assert G == 1 or bool((es[2] == 0).all())                          # a graph without chunks: zero sums, zero count
    _report("es [H=%d, G=%d]" % (H, G), es, want, float(mag.max()), lib)


@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("G", [1, 17, 48])
def test_rows_gemm_against_fp64(H, G, gpu):
    from dualmessagepassing_amd import fused
    gen = th.Generator().manual_seed(3 * G + H)
    T = th.randn(G, H, generator=gen).to(gpu)
    W2 = (th.randn(H, H, generator=gen) / H ** 0.5).to(gpu)
    for w_out_in, Wm in ((False, W2), (True, W2.t())):                 # T W2, and T W2^T with the weight in nn.Linear layout
        U = fused.rows_gemm(T, W2, w_out_in)
        want = T.double() @ Wm.double()
        _report("U [H=%d, G=%d, w_out_in=%d]" % (H, G, w_out_in), U, want, float((T.double().abs() @ Wm.double().abs()).max()), T @ Wm)
    wide = th.randn(G, 2 * H, generator=gen).to(gpu)                   # a column block of a wider matrix
    _report("U of a column block", fused.rows_gemm(wide[:, H:], W2, False), wide[:, H:].double() @ W2.double(),
            float((wide[:, H:].double().abs() @ W2.double().abs()).max()))


@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("G", [1, 17, 48, 150])                       # (48, 150: two and five workgroups' partials, the last one ragged)
@pytest.mark.parametrize("flagged", [True, False])
def test_gradient_kernel_against_fp64_and_pool_rows(H, G, flagged, gpu):
    from dualmessagepassing_amd import fused, ops
    pool, R = _index(G, flagged, 17 * G + H, gpu)
    gen = th.Generator().manual_seed(5 * G + H)
    T = th.randn(G, H, generator=gen).to(gpu)
    gcnt = fused.pool_weight_sums(pool)
    for width in ((2 * H,) if flagged else (2 * H, H)):                # the pass's table is [V, 2H]; [V, H] without a flag
        qc = th.randn(pool.num_chunks, width, generator=gen).to(gpu)
        want_q = ops.seg_sum_raw(qc, pool.gptr, pool.gent, G, None, False, rows_shared=False)[:, :H]
        Q64, Qmag = _graph_sums64(qc, pool, H)
        dirty = _padded(qc)
        if width == 2 * H:
            dirty[:, H:] = float("nan")
        with fused.deferred_reductions():                              # as in the layer's backward: one reduction launch at the end
            dW2, db2, Q = fused.pool_wgrad(dirty, pool, T, gcnt, want_q=True)
        assert th.equal(Q, want_q)
        assert dW2.shape == (H, H) and db2.shape == (H,)
        _report("dW2 [H=%d, G=%d]" % (H, G), dW2, T.double().t() @ Q64, float((T.double().abs().t() @ Qmag).max()), T.t() @ want_q)
        cnt = gcnt[:, 0].double()
        _report("db2 [H=%d, G=%d]" % (H, G), db2, cnt @ T.double(), max(float((cnt @ T.double().abs()).max()), 1e-30), gcnt[:, 0] @ T)
        again = fused.pool_wgrad(dirty, pool, T, gcnt)                 # no atomics, a fixed order: the same bits
        assert th.equal(again[0], dW2) and th.equal(again[1], db2)


def test_entries_refuse_null_and_misaligned_arguments(gpu):
    from dualmessagepassing_amd import fused
    from dualmessagepassing_amd._lib import ptr, stream_ptr
    lib = fused._lib.load()
    H, G = 64, 17
    pool, R = _index(G, True, 1, gpu)
    V = pool.num_chunks
    buf = th.zeros(V * 2 * H + G * H + H * H + 64, device=gpu)
    part, W2, b2, es = th.zeros(V, 2 * H, device=gpu), th.zeros(H, H, device=gpu), th.zeros(H, device=gpu), th.zeros(G, H, device=gpu)
    gcnt = th.zeros(G, 2, device=gpu)
    odd = lambda n: buf[1:1 + n]                                        # 4 bytes off a 16-byte boundary
    BAD_ARG = -1                                                        # DMP_ERR_BAD_ARG (include/dmp_hip.h)

    def out(partH=part, W=W2, b=b2, e=es, gp=pool.gptr, px=None, halves=2):
        return lib.dmp_pool_out(ptr(partH), None, V, halves, ptr(gp), ptr(pool.gent), G, ptr(gcnt), ptr(W), ptr(b), ptr(px), V, ptr(pool.gptr),
                                ptr(pool.gent), G, H, ptr(e), None, None, stream_ptr())

    assert out() == 0
    codes = [out(partH=None), out(partH=odd(V * 2 * H)), out(W=None), out(W=odd(H * H)), out(b=odd(H)), out(e=None), out(e=odd(G * H)),
             out(gp=None), out(px=part[:, :H].contiguous()), out(halves=3)]          # (node sums without a destination)
    T = th.zeros(G, H, device=gpu)
    nb = int(lib.dmp_pool_wgrad_blocks(G))
    assert nb == 1 and int(lib.dmp_pool_wgrad_blocks(0)) == 0 and int(lib.dmp_pool_wgrad_blocks(32)) == 1 and int(lib.dmp_pool_wgrad_blocks(65)) == 3
    pp = th.zeros(nb, H * H + H, device=gpu)

    def wg(q=part, t=T, c=gcnt, p=pp, ldq=2 * H):
        return lib.dmp_pool_wgrad(ptr(q), ldq, V, 2, ptr(pool.gptr), ptr(pool.gent), G, ptr(t), H, ptr(c), H, ptr(p), None, stream_ptr())

    assert wg() == 0
    codes += [wg(q=None), wg(q=odd(V * 2 * H)), wg(t=None), wg(t=odd(G * H)), wg(c=None), wg(p=None), wg(p=odd(nb * (H * H + H))), wg(ldq=H - 4)]

    def rg(a=T, W=W2, o=es, lda=H):
        return lib.dmp_rows_gemm(ptr(a), lda, G, H, ptr(W), 0, ptr(o), H, stream_ptr())

    assert rg() == 0
    codes += [rg(a=None), rg(a=odd(G * H)), rg(W=None), rg(o=None), rg(o=odd(G * H)), rg(lda=H + 2)]
    th.cuda.synchronize()
    assert all(c == BAD_ARG for c in codes), codes
    with pytest.raises(fused._lib.DmpError):                           # ... and a width the tiles do not take: an error, no fallback
        fused.rows_gemm(th.zeros(G, 32, device=gpu), th.zeros(32, 32, device=gpu), False)


# ------------------------------------------------------------------------------------------------ the layer
def _layer_case(gpu, H=128, gated=True, in_order=True):
    """bench.py's union of 96 pattern + 96 target graphs (the smallest batch at which the typed and the kept-node paths engage) with
    random 0 / 1 gates marked as ``dmpnn.joint_rep`` marks them, inputs wiped under their zeros, one layer and the pooling indexes."""
    sys.path.insert(0, ROOT)
    import bench
    from dualmessagepassing_amd import gatememo, ops
    from dualmessagepassing_amd.basemodel import _pool_indexes_union
    from dualmessagepassing_amd.collate import collate_device
    from dualmessagepassing_amd.dmpnn import DMPLayer, _joint_gates, _joint_index, prepare_joint
    cfg = dict(bench.CFG, batch=96)
    shard = bench.make_shard(cfg, 3, gpu)
    p, g = shard["p"], shard["g"]
    pattern = collate_device(p["local_src"], p["local_dst"], p["num_nodes"].clone(), p["num_edges"].clone(), p["N"], p["E"],
                             ndata=p["ndata"], edata=dict(p["edata"]), max_nodes=p["max_n"], max_edges=p["max_e"])
    graph = collate_device(g["local_src"], g["local_dst"], g["num_nodes"].clone(), g["num_edges"].clone(), g["N"], g["E"],
                           ndata=g["ndata"], edata=dict(g["edata"]), max_nodes=g["max_n"], max_edges=g["max_e"])
    union = prepare_joint(pattern, graph, H)
    ix, coef = _joint_index(union, H)
    vpool, epool = _pool_indexes_union(pattern, graph, ["node", "edge"], True)
    if not in_order:                     # the same sums over an index built from row keys (a sort: not in row order)
        epool = ops.PoolIndex.from_keys(epool.seg32.long(), epool.num_graphs)
        assert not epool.rows_in_order
    gen = th.Generator().manual_seed(7)
    N, E = ix.num_nodes, ix.num_edges
    vg = eg = None
    if gated:
        v_gate = (th.rand(N - p["N"], generator=gen) < 0.41).float().to(gpu)
        e_gate = (th.rand(E - p["E"], generator=gen) < 0.42).float().to(gpu)
        gatememo.mark(v_gate, binary=True)
        gatememo.mark(e_gate, binary=True)
        vg, eg = _joint_gates(v_gate, e_gate, p["N"], p["E"], th.float32, gpu)
    x, z = th.randn(N, H, generator=gen).to(gpu), th.randn(E, H, generator=gen).to(gpu)
    if gated:
        x, z = x * vg[:, None], z * eg[:, None]
    th.manual_seed(5)
    layer = DMPLayer(H, H, batch_norm=False, act_func="leaky_relu").to(gpu)
    gvs, ges = th.randn(vpool.num_graphs, H, generator=gen).to(gpu), th.randn(epool.num_graphs, H, generator=gen).to(gpu)
    return dict(ix=ix, coef=coef, vg=vg, eg=eg, x=x, z=z, layer=layer, vpool=vpool, epool=epool, gvs=gvs, ges=ges, keep=(ix, union, pattern, graph))


def _run_layer(c, on, residual=True, poison=False, names=None):
    from dualmessagepassing_amd import _lib, fused
    saved = fused.USE_POOL_ALGEBRA, fused.POISON_DEAD_ROWS
    fused.USE_POOL_ALGEBRA, fused.POISON_DEAD_ROWS = on, poison
    _lib.timer.reset()
    _lib.timer.enabled = names is not None
    try:
        x, z = c["x"].clone().requires_grad_(True), c["z"].clone().requires_grad_(True)
        xn, zn, vs, es = fused.fused_dmp_layer(c["ix"], c["coef"], residual, x, z, c["vg"], c["eg"], c["layer"],
                                               pools=(c["vpool"], c["epool"], False))
        assert zn is None and es.shape == c["ges"].shape
        params = list(c["layer"].parameters())
        grads = th.autograd.grad([vs, es], [x, z] + params, [c["gvs"], c["ges"]], allow_unused=True)
        th.cuda.synchronize()
        if names is not None:
            names.extend(n.split("[", 1)[0] for n, recs in _lib.timer.records.items() for _ in recs)
    finally:
        fused.USE_POOL_ALGEBRA, fused.POISON_DEAD_ROWS = saved
        _lib.timer.enabled = False
        _lib.timer.reset()
    res = {"vs": vs.detach(), "es": es.detach(), "dx": grads[0], "dz": grads[1]}
    res.update({"d" + n: g for (n, _), g in zip(c["layer"].named_parameters(), grads[2:])})
    return res


NEW = ("pool_out", "rows_gemm", "pool_wgrad")


def _compare_layer(c, on, off):
    assert set(on) == set(off)
    kept_e = None if c["eg"] is None else c["eg"] != 0
    for k, ref in off.items():
        got = on[k]
        assert (got is None) == (ref is None), k
        if ref is None:
            continue
        if k == "dz" and kept_e is not None:                           # (rows under a zero of the gate: dead, multiplied by that zero further down)
            got, ref = got[kept_e], ref[kept_e]
        if k == "dx" and c["vg"] is not None:
            got, ref = got[c["vg"] != 0], ref[c["vg"] != 0]
        assert bool(th.isfinite(got).all()), k
        if k in ("vs", "dx"):
            assert th.equal(got, ref), k
            continue
        err, top = float((got - ref).abs().max()), float(ref.abs().max())
        print("%s: differs by %.3g, largest entry %.3g" % (k, err, top))
        assert err <= 1e-5 * max(1.0, top), (k, err, top)
        assert err <= 5e-5 * top or top == 0.0, (k, err, top)


@pytest.mark.parametrize("gated,residual,poison", [(True, True, False), (True, True, True), (False, True, False), (True, False, True)])
def test_layer_with_the_route_on_equals_the_route_off(gated, residual, poison, gpu):
    c = _layer_case(gpu, gated=gated)
    n_on, n_off = [], []
    on = _run_layer(c, True, residual, poison, n_on)
    off = _run_layer(c, False, residual, poison, n_off)
    assert all(n_on.count(n) == 1 for n in NEW), n_on
    assert not any(n in n_off for n in NEW)
    assert n_on.count("pool_relu_bwd") == n_off.count("pool_relu_bwd") == 1
    # the second level of three forward sums and of the backward's one: four ``seg_sum`` launches fewer
    assert n_off.count("seg_sum") - n_on.count("seg_sum") == (4 if residual else 3), (n_on.count("seg_sum"), n_off.count("seg_sum"))
    _compare_layer(c, on, off)


@pytest.mark.parametrize("route", ["H32", "not_in_row_order", "switch_off"])
def test_fallbacks_run_the_old_launches(route, gpu):
    from dualmessagepassing_amd import fused
    if route == "H32":                   # a width the kernels do not take: the host condition says no, the layer runs as before
        c = _layer_case(gpu, H=32)
        lay = c["layer"].emlp[2]
        assert not fused.pool_algebra_ok(c["ix"], 32, c["epool"], lay.weight, lay.bias)
        names = []
        _run_layer(c, True, names=names)
        assert not any(n in names for n in NEW), names
        assert names.count("seg_sum") + names.count("seg_sum2") >= 2
        wide = _layer_case(gpu)          # ... and what else the condition reads, on a width they do take
        lay = wide["layer"].emlp[2]
        assert fused.pool_algebra_ok(wide["ix"], 128, wide["epool"], lay.weight, lay.bias)
        assert not fused.pool_algebra_ok(wide["ix"], 128, wide["epool"], lay.weight.t(), lay.bias)               # not contiguous
        assert not fused.pool_algebra_ok(wide["ix"], 128, wide["epool"], lay.weight, lay.bias.detach()[1:])      # misaligned
        return
    c = _layer_case(gpu, in_order=(route != "not_in_row_order"))
    names = []
    if route == "not_in_row_order":
        # (the row-less form needs the gated counts of an index in row order: such a layer hands out rows, the old launches)
        from dualmessagepassing_amd import _lib
        _lib.timer.reset()
        _lib.timer.enabled = True
        try:
            out = fused.fused_dmp_layer(c["ix"], c["coef"], True, c["x"], c["z"], c["vg"], c["eg"], c["layer"], pools=(c["vpool"], c["epool"]))
            th.cuda.synchronize()
            names = [n.split("[", 1)[0] for n, recs in _lib.timer.records.items() for _ in recs]
        finally:
            _lib.timer.enabled = False
            _lib.timer.reset()
        assert out[3] is not None
        lay = c["layer"].emlp[2]
        assert not fused.pool_algebra_ok(c["ix"], 128, c["epool"], lay.weight, lay.bias)
    else:
        _run_layer(c, False, names=names)
        assert names.count("pool_relu_bwd") == 1
    assert not any(n in names for n in NEW), names
    assert names.count("seg_sum") >= 2


# ------------------------------------------------------------------------------------------------ the recorded step
def test_replayed_step_equals_the_eager_step(gpu):
    """bench.py's recordable step at 96 pairs, once eagerly and once replayed from its recording: prediction and flat gradient."""
    from dualmessagepassing_amd import fused
    from dualmessagepassing_amd.dp import StepGraph
    sys.path.insert(0, ROOT)
    import bench
    assert fused.USE_POOL_ALGEBRA
    cfg = dict(bench.CFG, batch=96, graph=True)
    shard = bench.make_shard(cfg, 0, gpu)
    step, model = bench.build_step(cfg, shard, gpu, 1)
    gen = th.Generator().manual_seed(99)
    with th.no_grad():                                          # away from the zero-initialised head
        for p in step.sync.params:
            p.add_((0.05 * th.randn(p.shape, generator=gen)).to(gpu))
    calls = []
    real = fused.pool_wgrad
    fused.pool_wgrad = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        run = StepGraph(lambda: step.front(), max_shapes=1)
        with run.on_stream():
            run()
            th.cuda.synchronize()
            eager, pred = step.sync.flat.detach().clone(), step.last_pred_c.clone()
            step.sync.flat.zero_()
            run()
            th.cuda.synchronize()
            replayed, pred2 = step.sync.flat.detach().clone(), step.last_pred_c.clone()
    finally:
        fused.pool_wgrad = real
    assert calls, "the three-launch route did not run"
    assert run.eager_calls == 1 and run.replays == 1
    assert bool(th.isfinite(eager).all()) and float(eager.abs().max()) > 0 and th.equal(eager, replayed)
    assert bool(th.isfinite(pred).all()) and th.equal(pred, pred2)
