"""The first layer's edge MLP forward from the label codes as ONE launch (csrc/dmp_l0mlp.hip: ``fused.out_fwd_typed_codes(first=...)``
-> ``fused.l0_edge_fwd(mlp=...)`` -> ``dmp_l0_edge_mlp_fwd``) against the launches it replaces (``dmp_l0_edge_fwd_*`` per embedding
table, then ``dmp_out_fwd_typed_codes``) and against fp64, on hand-made tile lists.

The arithmetic contract.  The second role runs ``dmp_out_fwd_typed_codes``' piece products in its order with its epilogue order: ``zn``
is ``torch.equal`` to that launch run on the one launch's own ``H1`` over the same tile list.  The first role forms the K-column
product on the matrix pipe (bf16x6) where ``dmp_l0_edge_fwd_*`` uses fp32 multiply-adds, so ``H1`` is NOT bit-identical to theirs: both
are held to the bound ``tests/test_gpu_layer0.py`` applies to this layer's activation, ``2e-5 * max(1, |ref|max)`` against fp64, and
the two errors are printed side by side.  Dead input rows hold NaN; dead output rows must keep their sentinel bit for bit."""
import os
import sys

import pytest
import torch as th

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 128
K = 10               # the shipped code width (rows of Kpad = 12 floats)
KPAD = 12
SLOPE = 1.0 / 5.5
SENT = 7.5
BOUND = 2e-5         # tests/test_gpu_layer0.py::test_layer0_kernels_against_fp64


class _Index:
    """What ``fused.l0_edge_fwd`` reads of a graph index: the node count and the per-edge selectors / coefficients."""

    def __init__(self, num_nodes, sel_a, sel_b, coef_e):
        self.num_nodes, self.num_edges, self._sel = num_nodes, sel_a.numel(), (sel_a, sel_b, coef_e)

    def edge_select(self, coef):
        return self._sel


def _pick(E, n):
    return lambda g: th.randperm(E, generator=g)[:n].sort().values


# name: (E, N, pattern rows, embedding tables, kept rows, tile bound or None (the list's own), residual rows given)
SHAPES = {
    # 20 kept rows of 40: one tile with 12 padding slots, pattern and target rows mixed in it
    "one_tile": (40, 16, 5, 2, _pick(40, 20), None, True),
    # 150 kept of 300: five tiles under a bound of ten -- ten workgroups, five of them with an empty range (return before any barrier)
    "fewer_tiles_than_workgroups": (300, 40, 37, 2, _pick(300, 150), None, True),
    # 200 kept of 300 under a tile bound of ONE: one workgroup walks all seven tiles -- the rings of two and four wrap around
    "one_workgroup": (300, 40, 37, 2, _pick(300, 200), 1, True),
    # no pattern rows at all: code_row0 = 0, no residual operand
    "no_pattern_rows": (100, 24, 0, 2, _pick(100, 70), None, False),
    # one shared table: every row takes the first table's matrices, the rows below code_row0 still take no codes term
    "shared_table": (100, 24, 9, 1, _pick(100, 70), None, True),
    # every row, in order (``fused.identity_tiles``); 100 rows: 28 padding slots in the last tile
    "identity": (100, 24, 9, 2, lambda g: th.arange(100), "identity", True),
}
_CASES = {}


def _case(name):
    """Inputs (NaN in every dead row; anything in the codes' padding columns), weights, the tile list and the fp64 results: made once."""
    if name in _CASES:
        return _CASES[name]
    E, N, n_pat, tables, pick, bound, with_r = SHAPES[name]
    g = th.Generator().manual_seed(len(name) + E)
    kept = pick(g)
    keep = th.zeros(E, dtype=th.bool)
    keep[kept] = True
    r = lambda *s: th.randn(*s, generator=g)
    c = dict(E=E, N=N, n_pat=n_pat, tables=tables, kept=kept, keep=keep, with_r=with_r)
    enc = th.zeros(E, KPAD)
    enc[:, :K] = (th.rand(E, K, generator=g) < 0.5).float()
    enc[:, K:] = 3.0                                              # padding columns: the kernels must not use them
    enc[~keep] = float("nan")
    c["enc"] = enc
    c["W0"] = r(tables * K, H)                                    # the embedding tables (the pattern's over the target's)
    c["Wes"], c["W2t"], c["be"], c["b2"] = r(H, 2 * H) / (2 * H) ** 0.5, r(H, H) / H ** 0.5, r(H), r(H)
    c["coef_e"] = 1.0 / th.randint(1, 8, (E,), generator=g).float()
    # P = XP[:, H:] of [N + 1, 3H] (ldp = 3H, as in the layer); row N is a zero row: the launches of their own cannot take a selector
    # of -1, they read that row instead
    XP = r(N + 1, 3 * H)
    XP[N] = 0.0
    c["selA"] = th.randint(0, N, (E,), generator=g).to(th.int32)
    c["selB"] = th.randint(0, N, (E,), generator=g).to(th.int32)
    c["selA"][kept[::7]] = -1                                     # (a dead node: reads as zeros through the descriptor)
    c["selB"][kept[3::11]] = -1
    live = th.zeros(N + 1, dtype=th.bool)
    live[N] = True
    for sel in (c["selA"], c["selB"]):
        ids = sel[kept].long()
        live[ids[ids >= 0]] = True
    XP[~live] = float("nan")                                      # the rows no kept slot references
    c["XP"] = XP
    R = r(n_pat, H)
    R[~keep[:n_pat]] = float("nan")
    c["R"] = R
    nt = (kept.numel() + 31) // 32
    if bound == "identity":
        c["tiles"] = "identity"
    else:
        b = (E + 31) // 32 if bound is None else bound
        slot = th.full((max(b, nt) * 32,), -1, dtype=th.int32)
        slot[:kept.numel()] = kept.to(th.int32)
        c["tiles"] = (slot, th.zeros(max(b, nt)), th.tensor([nt], dtype=th.int32), b)
    c["M"] = None                                                 # W0 Wes: formed in fp32 on the device (``_dev``), as the layer does
    _CASES[name] = c
    return c


def _dev(c, gpu):
    from dualmessagepassing_amd import fused
    g = lambda t: t.to(gpu)
    XP = g(c["XP"])
    d = dict(enc=g(c["enc"]), W0=g(c["W0"]), Wes=g(c["Wes"]), W2t=g(c["W2t"]), be=g(c["be"]), b2=g(c["b2"]), P=XP[:, H:],
             R=g(c["R"]) if c["with_r"] else None, coef_e=g(c["coef_e"]), selA=g(c["selA"]), selB=g(c["selB"]))
    d["M"] = th.cat([d["W0"][t * K:(t + 1) * K] @ d["Wes"] for t in range(c["tables"])])
    d["tiles"] = fused.identity_tiles(c["E"], gpu) if c["tiles"] == "identity" else tuple(g(t) if th.is_tensor(t) else t for t in c["tiles"])
    return d


def _fp64(c, d):
    """``(H1, zn)`` of the kept rows in fp64 on the CPU, from the fp32 operands the kernels get."""
    keep, n_pat, E = c["keep"], c["n_pat"], c["E"]
    dd = lambda t: t.double().cpu()
    enc, M, P = dd(d["enc"])[keep][:, :K], dd(d["M"]), dd(d["P"])
    rows = th.arange(E)[keep]
    t = ((rows >= n_pat) & (c["tables"] == 2)).long()            # the row's table
    MA = th.stack([M[i * K:(i + 1) * K, :H] for i in range(c["tables"])])[t]      # [kept, K, H]
    MB = th.stack([M[i * K:(i + 1) * K, H:] for i in range(c["tables"])])[t]
    ce = dd(d["coef_e"])[keep].view(-1, 1)
    a, b = c["selA"][keep].long(), c["selB"][keep].long()
    zero = th.zeros(1, dtype=th.float64)
    pa = th.where((a >= 0).view(-1, 1), P[a.clamp(min=0), :H], zero)
    pb = th.where((b >= 0).view(-1, 1), P[b.clamp(min=0), H:2 * H], zero)
    pre = th.einsum("rk,rkh->rh", enc, MA) + ce * th.einsum("rk,rkh->rh", enc, MB) + pa - pb + dd(d["be"])
    h1 = th.nn.functional.leaky_relu(pre, SLOPE)
    zn = h1 @ dd(d["W2t"]) + dd(d["b2"])
    zn = zn + th.where((rows >= n_pat).view(-1, 1), enc @ dd(d["W0"])[-K:], zero)
    if c["with_r"] and n_pat:
        res = th.zeros(E, H, dtype=th.float64)
        res[:n_pat] = dd(d["R"])
        zn = zn + res[keep]
    return h1, zn


def _one_launch(c, d, gpu):
    from dualmessagepassing_amd import fused
    E, N = c["E"], c["N"]
    ix = _Index(N, d["selA"], d["selB"], d["coef_e"])
    h1 = th.full((E, H + 4), SENT, device=gpu)                    # (outputs: column blocks of wider buffers)
    zn = th.full((E, H + 4), SENT, device=gpu)
    assert fused.l0_edge_mlp_ok(H, K, c["tables"], d["enc"], d["P"], d["W2t"], d["R"])
    fused.out_fwd_typed_codes(h1[:, :H], d["W2t"], d["b2"], d["enc"], K, d["W0"][-K:], d["tiles"], prev=d["R"], out=zn[:, 4:],
                              row0=c["n_pat"], first=dict(M=d["M"], tables=c["tables"], split=c["n_pat"], P=d["P"], ldp=d["P"].stride(0),
                                                          bias=d["be"], coef=None, index=ix, slope=SLOPE))
    return h1, zn


def _launches_of_their_own(c, d, gpu):
    """``l0_edge_fwd`` per table over ALL rows of its range (dead rows: NaN codes in, NaN out -- only the kept rows are compared), the
    selectors of -1 pointing at P's zero row."""
    from dualmessagepassing_amd import fused
    E, N, n_pat = c["E"], c["N"], c["n_pat"]
    fix = lambda s: th.where(s < 0, th.full_like(s, N), s)
    ix = _Index(N + 1, fix(d["selA"]), fix(d["selB"]), d["coef_e"])
    h1 = th.full((E, H), SENT, device=gpu)
    ranges = [(0, (0, E))] if c["tables"] == 1 else [(0, (0, n_pat)), (1, (n_pat, E))]
    for t, rows in ranges:
        if rows[1] > rows[0]:
            fused.l0_edge_fwd(d["enc"], K, d["M"][t * K:(t + 1) * K], d["P"], d["P"].stride(0), d["be"], None, ix, SLOPE, rows, h1)
    return h1


def _err(name, what, new, old, ref):
    bound = BOUND * max(1.0, float(ref.abs().max()))
    e_new = float((new.double().cpu() - ref).abs().max())
    e_old = float((old.double().cpu() - ref).abs().max()) if old is not None else float("nan")
    print("%s %s: one launch %.3e  launches of their own %.3e  bound %.3e" % (name, what, e_new, e_old, bound))
    return e_new, e_old, bound


@pytest.mark.parametrize("name", list(SHAPES))
def test_one_launch_against_its_second_half_and_fp64(name, gpu):
    from dualmessagepassing_amd import fused
    c = _case(name)
    d = _dev(c, gpu)
    keep = c["keep"].to(gpu)
    assert d["P"].stride(0) == 3 * H
    h1w, znw = _one_launch(c, d, gpu)
    h1, zn = h1w[:, :H], znw[:, 4:]
    assert bool(th.isfinite(h1[keep]).all()) and bool(th.isfinite(zn[keep]).all()), "a dead row's NaN reached a kept row"
    # dead rows, and the columns beside the outputs: the sentinel, bit for bit
    assert bool((h1[~keep] == SENT).all()) and bool((zn[~keep] == SENT).all()), "a dead row was written"
    assert bool((h1w[:, H:] == SENT).all()) and bool((znw[:, :4] == SENT).all()), "the columns beside an output were written"
    # 1. the second role: dmp_out_fwd_typed_codes on the one launch's own H1 over the same tile list, bit for bit
    zn2 = th.full((c["E"], H), SENT, device=gpu)
    fused.out_fwd_typed_codes(h1.contiguous(), d["W2t"], d["b2"], d["enc"], K, d["W0"][-K:], d["tiles"], prev=d["R"], out=zn2, row0=c["n_pat"])
    assert th.equal(zn[keep], zn2[keep]), "zn differs from dmp_out_fwd_typed_codes on the same H1"
    # 2. the first role against fp64, the launches of their own beside it
    ref_h1, ref_zn = _fp64(c, d)
    old = _launches_of_their_own(c, d, gpu)
    e_new, e_old, bound = _err(name, "H1e", h1[keep], old[keep], ref_h1)
    assert e_old <= bound, ("launches of their own", e_old, bound)
    assert e_new <= bound, ("one launch", e_new, e_old, bound)
    e_new, _, bound = _err(name, "zn", zn[keep], None, ref_zn)
    assert e_new <= bound, ("zn", e_new, bound)
    # repeatability: the same bits on a second launch
    h1b, znb = _one_launch(c, d, gpu)
    assert th.equal(h1b, h1w) and th.equal(znb, znw)


def test_without_biases(gpu):
    """No bias on either Linear (NULL: the kernel loads it through a descriptor of zero records): the bits of zero biases, and fp64."""
    c = _case("one_tile")
    d = _dev(c, gpu)
    keep = c["keep"].to(gpu)
    zeros = th.zeros(H, device=gpu)
    h1w, znw = _one_launch(c, dict(d, be=None, b2=None), gpu)
    h1z, znz = _one_launch(c, dict(d, be=zeros, b2=zeros), gpu)
    assert th.equal(h1w, h1z) and th.equal(znw, znz)
    ref_h1, ref_zn = _fp64(c, dict(d, be=zeros, b2=zeros))
    e, _, bound = _err("no biases", "H1e", h1w[:, :H][keep], None, ref_h1)
    assert e <= bound, (e, bound)
    e, _, bound = _err("no biases", "zn", znw[:, 4:][keep], None, ref_zn)
    assert e <= bound, (e, bound)


def test_fallback_conditions(gpu):
    """The switch, another width, too many code columns or tables, a row stride the descriptors cannot take: the launches of their own."""
    from dualmessagepassing_amd import _lib, fused
    a = th.zeros(64, H, device=gpu)
    enc = th.zeros(64, KPAD, device=gpu)
    assert fused.l0_edge_mlp_ok(H, K, 2, enc, a, None)
    assert fused.l0_edge_mlp_ok(H, 12, 1, enc, a)
    assert not fused.l0_edge_mlp_ok(H, 13, 2, th.zeros(64, 16, device=gpu), a)
    assert not fused.l0_edge_mlp_ok(H, K, 3, enc, a)
    assert not fused.l0_edge_mlp_ok(64, K, 2, enc, th.zeros(64, 64, device=gpu))
    assert not fused.l0_edge_mlp_ok(H, K, 2, th.zeros(64, KPAD + 2, device=gpu)[:, :KPAD], a)
    lib = _lib.load()
    lib.dmp_dev_set_exact_fp32(1)
    try:
        assert not fused.l0_edge_mlp_ok(H, K, 2, enc, a)
    finally:
        lib.dmp_dev_set_exact_fp32(0)
    fused.USE_L0_EDGE_MLP = False
    try:
        assert not fused.l0_edge_mlp_ok(H, K, 2, enc, a)
    finally:
        fused.USE_L0_EDGE_MLP = True


def _compact():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_compact
    return test_gpu_compact


def _first_layer_records(bench_, cfg, shard, step, model):
    """One forward + backward with the HIP-event timer on -> (outputs, flat gradient, {record base name: launches})."""
    from dualmessagepassing_amd import _lib
    _lib.timer.reset()
    _lib.timer.only, _lib.timer.enabled = None, True
    try:
        out, flat = _compact()._outputs_and_grads(bench_, cfg, shard, step, model, True)
        launches = {}
        for k, v in _lib.timer.summary().items():
            launches[k.split("[", 1)[0]] = launches.get(k.split("[", 1)[0], 0) + int(v["launches"])
    finally:
        _lib.timer.enabled = False
        _lib.timer.reset()
    return out, flat, launches


@pytest.mark.parametrize("filt", ["ScalarFilter", "None"])
def test_model_with_the_one_launch_equals_the_model_without_it(filt, gpu):
    """bench.py's model on 8 pairs (under the ScalarFilter gates: over the kept edges' tiles; without a filter net: the identity
    tiles), forward + loss + backward with ``USE_L0_EDGE_MLP`` on against off: all 15 outputs and every parameter gradient at the
    tolerances ``tests/test_gpu_layer0.py`` holds the label-code path's switch to (2e-5 / 2e-4 of ``max(1, |ref|max)``); the timer's
    records say which route ran.  Then the step replayed through ``StepGraph`` twice: the same bits both times."""
    from dualmessagepassing_amd import fused
    from dualmessagepassing_amd.dp import StepGraph
    sys.path.insert(0, ROOT)
    import bench
    cfg = dict(bench.CFG, batch=8, filter=filt)
    bench_, shard, step, model = _compact()._model_and_batch(cfg, gpu)
    fused.USE_L0_EDGE_MLP = False
    try:
        ref_out, ref_flat, rec = _first_layer_records(bench_, cfg, shard, step, model)
    finally:
        fused.USE_L0_EDGE_MLP = True
    assert rec.get("l0_edge_fwd") == 2 and rec.get("out_fwd_typed_codes") == 1, rec     # one per table, then the second Linear
    out, flat, rec = _first_layer_records(bench_, cfg, shard, step, model)
    assert rec.get("l0_edge_fwd") == 1 and "out_fwd_typed_codes" not in rec, rec         # the one launch, under its first half's name
    assert set(out) == set(ref_out)
    for k, v in ref_out.items():
        if v is None:
            assert out[k] is None
            continue
        assert bool(th.isfinite(out[k]).all()), k
        s = max(1.0, float(v.abs().max()))
        e = float((out[k] - v).abs().max())
        print("%s %s: %.3e of %.3e" % (filt, k, e, s))
        assert e <= 2e-5 * s, (k, e, s)
    assert bool(th.isfinite(flat).all())
    for prm, off in zip(step.sync.params, step.sync.offsets):
        a, b = flat[off:off + prm.numel()], ref_flat[off:off + prm.numel()]
        s = max(1.0, float(b.abs().max()))
        assert float((a - b).abs().max()) <= 2e-4 * s, (off, float((a - b).abs().max()), s)
    # replayed: the recording holds the one launch; two replays give the same bits
    step_g, _ = bench.build_step(dict(cfg, graph=True), shard, gpu, 1)
    g = StepGraph(lambda: step_g.front(), optimizer=None, max_shapes=1)
    res = []
    with g.on_stream():
        g()                                                       # eager
        for _ in range(2):
            step_g.sync.flat.fill_(float("nan"))
            g()
            th.cuda.synchronize()
            res.append((step_g.last_pred_c.detach().clone(), step_g.sync.flat.detach().clone()))
        assert g.replays == 2
    assert bool(th.isfinite(res[0][0]).all()) and bool(th.isfinite(res[0][1]).all())
    assert th.equal(res[0][0], res[1][0]) and th.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("how", ["hid64", "exact_fp32"])
def test_unsupported_shapes_run_the_launches_of_their_own(how, gpu):
    """H = 64 and the exact-fp32 development switch: the first layer runs ``l0_edge_fwd`` once per embedding table, as before."""
    from dualmessagepassing_amd import _lib
    sys.path.insert(0, ROOT)
    import bench
    cfg = dict(bench.CFG, batch=8, hid=64) if how == "hid64" else dict(bench.CFG, batch=8)
    lib = _lib.load()
    if how == "exact_fp32":
        lib.dmp_dev_set_exact_fp32(1)
    try:
        bench_, shard, step, model = _compact()._model_and_batch(cfg, gpu)
        out, flat, rec = _first_layer_records(bench_, cfg, shard, step, model)
    finally:
        lib.dmp_dev_set_exact_fp32(0)
    assert rec.get("l0_edge_fwd") == 2, rec
    assert bool(th.isfinite(out["pred_c"]).all()) and bool(th.isfinite(flat).all())
