"""The first layer's code weight gradient from the second Linear's backward launch (csrc/dmp_h1w.hip::h1w_k<1|2>,
``fused.bwd_h1_w(codes=...)`` -> ``dmp_bwd_h1_w_codes``): ``XX = [enc^T dPre | (c (.) enc)^T dPre | enc^T dO]`` over the rows of the
tile list inside one embedding table's edge range, against fp64, against ``bwd_h1_w`` without codes (the four other results: the same
bits) and against ``l0_bwd_w``, the launch it replaces; the row range; the model with the switch on and off (gated, without a filter
net, with the dead rows poisoned), replayed from a recording, and on the routes the variant does not take.

Shapes: 203 edge rows in 7 hand-built tiles (padding inside and at the end of tiles, a tile of padding only, a tile across the
range's first row 37, which lies inside a tile and inside a mask word) on 12 workgroups -- five of them without a tile.  The fp64
bound, 2e-5 of a block's natural scale ``max sum |a||b|``, is the project's bound for bf16x6 products."""
import os
import sys
import types

import numpy as np
import pytest
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu_test = pytest.mark.gpu
H, E, K, KPAD, R0 = 128, 203, 10, 12, 37
SLOPE = 1 / 5.5


# ------------------------------------------------------------------------------------------------ the host condition (no GPU)
def test_host_condition_truth_table():
    from dualmessagepassing_amd import fused
    enc = th.zeros(64, KPAD)
    two = [(0, (0, 20), (0, 8)), (1, (20, 64), (8, 40))]

    def l0(k=K, e=enc):
        return types.SimpleNamespace(enc=e, K=k)

    ok = fused.h1w_codes_ok
    assert fused.USE_H1W_CODES and fused.H1W_MAX_CODES == 16
    assert ok(l0(), two, "kept") and ok(l0(), two, "all")
    assert ok(l0(16, th.zeros(64, 16)), two, "kept")
    assert not ok(None, two, "kept")                                   # not the first layer
    assert not ok(l0(), two, "kept", h1w=False)                        # H != 128, exact fp32, 4 GiB arrays: ``h1w_ok`` said no
    assert not ok(l0(), two, None)                                     # no tile list whose rows ``l0_bwd_w`` would have walked
    assert not ok(l0(17, th.zeros(64, 20)), two, "kept")               # more code columns than half the code operand holds
    assert not ok(l0(0), two, "kept")
    assert not ok(l0(), two[1:], "kept")                               # a single table: its launch stays ``l0_bwd_w``'s
    assert not ok(l0(), [(0, (0, 64), (0, 40))], "all")
    assert not ok(l0(), [two[0], (1, (64, 64), (8, 40))], "kept")      # the last table has no edge rows
    assert not ok(l0(e=th.zeros(64, 2 * KPAD)[:, ::2]), two, "kept")   # code columns not contiguous
    assert not ok(l0(e=enc.double()), two, "kept")
    saved = fused.USE_H1W_CODES
    fused.USE_H1W_CODES = False
    try:
        assert not ok(l0(), two, "kept")
    finally:
        fused.USE_H1W_CODES = saved


# ------------------------------------------------------------------------------------------------ the kernel
def _tiles(dev):
    """7 tiles by hand over a strict, ascending subset of the 203 rows; 12 tiles of room (12 workgroups)."""
    ids = [r for r in range(E) if r % 5 != 3 and r not in (36, 38, 100, 202)]
    t = []
    t.append(ids[0:10] + [-1, -1, -1] + ids[10:22] + [-1] * 7)           # padding in the middle and at the end (rows 0 .. 26)
    t.append(ids[22:54])                                                   # a full tile across row 37 (rows 27 .. 69)
    t.append([-1] * 32)                                                    # padding only
    t.append(ids[54:70] + [-1] + ids[70:80] + [-1] * 5)
    t.append(ids[80:112])
    t.append([-1] * 4 + ids[112:130] + [-1] * 10)
    rest = ids[130:]
    assert 0 < len(rest) <= 32 and rest[-1] == E - 2
    t.append(rest + [-1] * (32 - len(rest)))
    assert len(t) == 7 and all(len(x) == 32 for x in t)
    flat = [r for x in t for r in x if r >= 0]
    assert flat == ids and any(r < R0 for r in t[1]) and any(r >= R0 for r in t[1])
    bound = 12
    slot = th.full((bound * 32,), -1, dtype=th.int32)
    slot[:7 * 32] = th.tensor([r for x in t for r in x], dtype=th.int32)
    listed = th.zeros(E, dtype=th.bool)
    listed[ids] = True
    return (slot.to(dev), th.zeros(bound, device=dev), th.tensor([7], dtype=th.int32, device=dev), bound), listed.to(dev)


_CASES = {}


def _case(binary, gpu):
    """Inputs, the launch without codes and the fp64 restatement: made once per code kind, shared by the tests, never changed."""
    if binary in _CASES:
        return _CASES[binary]
    from dualmessagepassing_amd import fused
    gen = th.Generator().manual_seed(11 + int(binary))
    tiles, listed = _tiles(gpu)
    nan = float("nan")
    d_o = th.randn(E, H, generator=gen).to(gpu)
    h1 = th.randn(E, H, generator=gen).to(gpu)
    W2 = (th.randn(H, H, generator=gen) / H ** 0.5).to(gpu)
    coef = (2.0 + 10.0 * th.rand(E, generator=gen)).to(gpu)
    enc = th.zeros(E, KPAD)
    enc[:, :K] = (th.rand(E, K, generator=gen) < 0.5).float() if binary else th.randn(E, K, generator=gen)
    enc[:, K:] = 7.0                                     # the padding columns of a code row are not code columns
    enc = enc.to(gpu)
    enc[~listed, :K] = 0.0                               # (a row outside the list is a gated-out row: its packed codes are zeros)
    d_o[~listed], h1[~listed] = nan, nan
    plain = fused.bwd_h1_w(d_o, W2, h1, tiles, SLOPE, out=th.full((E, H), nan, device=gpu))
    c = dict(tiles=tiles, listed=listed, d_o=d_o, h1=h1, W2=W2, coef=coef, enc=enc, plain=plain)
    _CASES[binary] = c
    return c


def _run(c, rows, residual, gpu):
    from dualmessagepassing_amd import fused
    return fused.bwd_h1_w(c["d_o"], c["W2"], c["h1"], c["tiles"], SLOPE, out=th.full((E, H), float("nan"), device=gpu),
                          codes=dict(enc=c["enc"], K=K, coef_e=c["coef"], rows=rows, residual=residual))


def _want(c, rows, d_pre):
    """fp64 blocks and their natural scales over the listed rows of the range."""
    sel = c["listed"].clone()
    sel[:rows[0]] = False
    sel[rows[1]:] = False
    e = c["enc"][sel, :K].double()
    ce = e * c["coef"][sel].double().view(-1, 1)
    dp, do = d_pre[sel].double(), c["d_o"][sel].double()
    blocks = [(e.t() @ dp, e.abs().t() @ dp.abs()), (ce.t() @ dp, ce.abs().t() @ dp.abs()), (e.t() @ do, e.abs().t() @ do.abs())]
    return [(w, float(s.max()) if s.numel() else 0.0) for w, s in blocks]


def _check_blocks(xx, want, nblocks, what):
    assert xx.shape == (K, nblocks * H)
    for b in range(nblocks):
        w, scale = want[b]
        err = float((xx[:, b * H:(b + 1) * H].double() - w).abs().max())
        print("%s block %d: error %.3g, natural scale %.3g, ratio %.3g" % (what, b, err, scale, err / scale if scale else 0.0))
        assert err <= 2e-5 * scale, (what, b, err, scale)


@gpu_test
@pytest.mark.parametrize("binary", [True, False])
def test_kernel_against_fp64_and_its_parts(binary, gpu):
    from dualmessagepassing_amd import fused
    c = _case(binary, gpu)
    lib = fused._lib.load()
    assert int(lib.dmp_bwd_h1_w_blocks(c["tiles"][3])) == 12 > int(c["tiles"][2][0])    # workgroups without a tile
    assert int(lib.dmp_bwd_h1_w_max_codes()) == fused.H1W_MAX_CODES
    rows = (R0, E)
    dg, db, dbr, dw, xx = _run(c, rows, True, gpu)
    pdg, pdb, pdbr, pdw = c["plain"]
    listed = c["listed"]
    # the four results of the plain launch: the same bits; rows outside the list: never written
    assert th.equal(dg[listed], pdg[listed]) and bool(th.isnan(dg[~listed]).all()) and bool(th.isnan(pdg[~listed]).all())
    assert th.equal(db, pdb) and th.equal(dbr, pdbr) and th.equal(dw, pdw)
    for t in (dg[listed], db, dbr, dw, xx):
        assert bool(th.isfinite(t).all())
    want = _want(c, rows, pdg)
    _check_blocks(xx, want, 3, "fused")
    # the launch it replaces, on the same rows (its own mask from the code rows: the range starts inside a mask word)
    ref = fused.l0_bwd_w(c["enc"], K, c["coef"], pdg, c["d_o"], rows, mask=fused.code_row_mask(c["enc"], K))
    _check_blocks(ref, want, 3, "l0_bwd_w")
    # the same bits on every launch
    again = _run(c, rows, True, gpu)
    assert all(th.equal(a[listed] if a.size(0) == E else a, b[listed] if b.size(0) == E else b) for a, b in zip((dg, db, dbr, dw, xx), again))
    # without the residual gradient: two blocks, unchanged
    dg2, db2, dbr2, dw2, xx2 = _run(c, rows, False, gpu)
    assert xx2.shape == (K, 2 * H) and th.equal(xx2, xx[:, :2 * H])
    assert th.equal(dg2[listed], pdg[listed]) and th.equal(db2, pdb) and th.equal(dbr2, pdbr) and th.equal(dw2, pdw)
    # ``out``: the reduced block lands in the caller's rows
    buf = th.full((2 * K, 3 * H), -3.0, device=gpu)
    from dualmessagepassing_amd.fused import bwd_h1_w
    res = bwd_h1_w(c["d_o"], c["W2"], c["h1"], c["tiles"], SLOPE, out=th.full((E, H), float("nan"), device=gpu),
                   codes=dict(enc=c["enc"], K=K, coef_e=c["coef"], rows=rows, residual=True, out=buf[K:]))
    assert th.equal(buf[K:], xx) and th.equal(res[4], xx) and bool((buf[:K] == -3.0).all())


@gpu_test
@pytest.mark.parametrize("binary", [True, False])
def test_row_range(binary, gpu):
    """Only the rows of the range are summed: the table before row 37, and an empty range (exact zeros)."""
    c = _case(binary, gpu)
    pdg = c["plain"][0]
    xx = _run(c, (0, R0), True, gpu)[4]
    _check_blocks(xx, _want(c, (0, R0), pdg), 3, "rows [0, 37)")
    whole = _run(c, (0, E), True, gpu)[4]
    _check_blocks(whole, _want(c, (0, E), pdg), 3, "rows [0, 203)")
    for rows in ((R0, R0), (0, 0), (E, E)):
        for residual in (True, False):
            z = _run(c, rows, residual, gpu)[4]
            assert z.shape == (K, (3 if residual else 2) * H) and bool((z == 0).all())
    # a range one row short on either side differs from the full one by exactly that row's terms (row 37 and row 201 are listed)
    for rows, row in (((R0 + 1, E), R0), ((R0, E - 2), E - 2)):
        assert bool(c["listed"][row])
        got = _run(c, rows, True, gpu)[4]
        _check_blocks(got, _want(c, rows, pdg), 3, "rows [%d, %d)" % rows)


@gpu_test
def test_entry_refuses_what_the_variant_does_not_cover(gpu):
    from dualmessagepassing_amd import fused
    c = _case(True, gpu)
    wide = th.zeros(E, 20, device=gpu)
    with pytest.raises(fused._lib.DmpError):
        fused.bwd_h1_w(c["d_o"], c["W2"], c["h1"], c["tiles"], SLOPE, codes=dict(enc=wide, K=17, coef_e=c["coef"], rows=(R0, E), residual=True))
    lib = fused._lib.load()
    lib.dmp_dev_set_exact_fp32(1)
    try:
        assert not fused.h1w_ok(c["d_o"], c["h1"], H)
        with pytest.raises(fused._lib.DmpError):
            _run(c, (R0, E), True, gpu)
    finally:
        lib.dmp_dev_set_exact_fp32(0)
    assert not fused.h1w_ok(c["d_o"][:, :64], c["h1"][:, :64], 64)


# ------------------------------------------------------------------------------------------------ the model
def _model(cfg, gpu):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_compact import _model_and_batch
    return _model_and_batch(cfg, gpu)


def _pass(model_and_batch, cfg, on, names=None):
    """One forward and backward of bench.py's model: every output, the flat gradient, the timer's record names."""
    from dualmessagepassing_amd import _lib, fused
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_compact import _outputs_and_grads
    bench_, shard, step, model = model_and_batch
    saved = fused.USE_H1W_CODES
    fused.USE_H1W_CODES = on
    _lib.timer.reset()
    _lib.timer.enabled = names is not None
    try:
        out, flat = _outputs_and_grads(bench_, cfg, shard, step, model, True)
        if names is not None:
            names.extend(n for n, recs in _lib.timer.records.items() for _ in recs)
    finally:
        fused.USE_H1W_CODES = saved
        _lib.timer.enabled = False
        _lib.timer.reset()
    return out, flat


def _count(names, base):
    return sum(1 for n in names if n.split("[", 1)[0] == base)


def _compare(step, on, off, bitwise=False):
    (out1, flat1), (out0, flat0) = on, off
    assert set(out1) == set(out0)
    for k, v in out0.items():                                   # the forward is untouched
        assert (v is None) == (out1[k] is None), k
        if v is not None:
            assert th.equal(out1[k], v), k
    assert bool(th.isfinite(flat1).all())
    if bitwise:
        assert th.equal(flat1, flat0)
        return
    for prm, off_ in zip(step.sync.params, step.sync.offsets):
        a, b = flat1[off_:off_ + prm.numel()], flat0[off_:off_ + prm.numel()]
        s = float(b.abs().max())
        err = float((a - b).abs().max())
        assert err <= 5e-5 * s, (off_, err, s)


@gpu_test
@pytest.mark.parametrize("filt,poison", [("ScalarFilter", False), ("ScalarFilter", True), ("None", False)])
def test_model_with_the_switch_on_and_off(filt, poison, gpu):
    """64 pairs of bench.py's shapes (4,608 node rows), gated over the kept edges' tiles / without a filter net over the identity
    tiles: the outputs bit for bit, every parameter gradient within 5e-5 of its largest entry, and one ``l0_bwd_w`` launch (the
    pattern's) where the two-launch route has two."""
    from dualmessagepassing_amd import fused
    sys.path.insert(0, ROOT)
    import bench
    cfg = dict(bench.CFG, batch=64, filter=filt)
    mb = _model(cfg, gpu)
    saved = fused.POISON_DEAD_ROWS
    fused.POISON_DEAD_ROWS = poison
    try:
        n_on, n_off = [], []
        on = _pass(mb, cfg, True, n_on)
        off = _pass(mb, cfg, False, n_off)
    finally:
        fused.POISON_DEAD_ROWS = saved
    assert _count(n_on, "bwd_h1_w") >= 1 and _count(n_on, "bwd_h1_w") == _count(n_off, "bwd_h1_w")      # the tile-list route ran
    assert _count(n_off, "l0_bwd_w") == 2 and _count(n_on, "l0_bwd_w") == 1
    _compare(mb[2], on, off)


@gpu_test
def test_replayed_step_equals_the_eager_step(gpu):
    """bench.py's recordable step (batch, forward, loss, backward, gradient pack) once eagerly and once replayed from its recording."""
    from dualmessagepassing_amd import fused
    from dualmessagepassing_amd.dp import StepGraph
    sys.path.insert(0, ROOT)
    import bench
    assert fused.USE_H1W_CODES
    cfg = dict(bench.CFG, batch=64, graph=True)
    shard = bench.make_shard(cfg, 0, gpu)
    step, model = bench.build_step(cfg, shard, gpu, 1)
    gen = th.Generator().manual_seed(99)
    with th.no_grad():                                          # away from the zero-initialised head
        for p in step.sync.params:
            p.add_((0.05 * th.randn(p.shape, generator=gen)).to(gpu))
    calls = []
    real = fused.bwd_h1_w
    fused.bwd_h1_w = lambda *a, **k: (calls.append(k.get("codes") is not None), real(*a, **k))[1]
    try:
        run = StepGraph(lambda: step.front(), max_shapes=1)
        with run.on_stream():
            run()
            th.cuda.synchronize()
            eager = step.sync.flat.detach().clone()
            step.sync.flat.zero_()
            run()
            th.cuda.synchronize()
            replayed = step.sync.flat.detach().clone()
    finally:
        fused.bwd_h1_w = real
    assert any(calls), "the fused launch did not run"
    assert run.eager_calls == 1 and run.replays == 1
    assert bool(th.isfinite(eager).all()) and float(eager.abs().max()) > 0 and th.equal(eager, replayed)


@gpu_test
@pytest.mark.parametrize("route", ["hid64", "exact_fp32"])
def test_routes_outside_the_variant_keep_the_two_launches(route, gpu):
    """H = 64 / the exact-fp32 development switch: the host condition says no and the step is the two-launch step, bit for bit."""
    from dualmessagepassing_amd import fused
    sys.path.insert(0, ROOT)
    import bench
    lib = fused._lib.load()
    cfg = dict(bench.CFG, batch=64, hid=64 if route == "hid64" else 128)
    if route == "exact_fp32":
        lib.dmp_dev_set_exact_fp32(1)
    try:
        mb = _model(cfg, gpu)
        n_on, n_off = [], []
        on = _pass(mb, cfg, True, n_on)
        off = _pass(mb, cfg, False, n_off)
    finally:
        lib.dmp_dev_set_exact_fp32(0)
    assert _count(n_on, "l0_bwd_w") == _count(n_off, "l0_bwd_w") == 2
    assert sorted(n_on) == sorted(n_off)
    _compare(mb[2], on, off, bitwise=True)
