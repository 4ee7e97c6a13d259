"""Shared by tests/test_gpu_bf16x6_only.py and scripts/bf16x6_probe.py: the bf16x6 kernels that have NO exact-fp32 form (they refuse
``dmp_dev_set_exact_fp32(1)``), each driven through its ``fused.*`` wrapper on hand-made tile lists and compared with fp64.

Three kinds of measurement (``run_only`` returns ``{kernel: {scenario: {output: record}}}``):

* ``ladder``: the sparse ladder of tests/bf16x6_cases.py -- every output element is ONE product of two values whose bf16 pieces are
  known, so each of the six piece products is at least 4 x 2^-21 of it.  ``err`` = the largest elementwise relative error; ``ok`` =
  finite, exactly 0 where fp64 is 0, the dead rows' sentinel bit for bit, and (for the second stage of a chained kernel) the first
  stage's pass-through output ``torch.equal`` to the permuted ladder rows.  160 rows, 128 kept in four 32-slot tiles (the class-tiled
  kernels: two classes with a partial tile each); the 32 dead rows hold NaN on input.
* the adversarial ``scenarios`` of tests/bf16x6_cases.py on 1031 kept rows of 1100: ``err`` of the natural scale ``sum |a||b|``
  (propagated through a chain in fp64), ``bound`` = the order-independent fp32 bound ``sum over the stages of gamma_K + 2^-23``
  (``gamma_K = K u / (1 - K u)``, ``u = 2^-24``, K the stage's contraction length), and where the kernel replaces launches that have an
  exact form, ``route`` = their error under ``dmp_dev_set_exact_fp32(1)`` on the same operands.
* ``tiny`` (magnitudes from 2^-118 up, ``operands``): two pieces are left; ``err`` of the natural scale.

The tile builders are the kernels' own tests' (imported, not copied)."""
import numpy as np
import torch as th

from bf16x6_cases import ladder, ladder_dense, ladder_rows, rel_elem, scenarios
from test_gpu_edge_mlp_fwd import _ascending_tiles, _class_tiles, _Index, _LiveTiles
from test_gpu_node_chain import _tiles

H = 128
SENT = 7.5
NAN = float("nan")
U = 2.0 ** -24
LADDER_ROWS, LADDER_KEPT = 160, 128
ENV_ROWS, ENV_KEPT = 1100, 1031
ENVELOPE = ("normal", "element_binades", "row_binades", "cancel", "small", "huge")


def stage_bound(*ks):
    """sum over the stages of ``gamma_K + 2^-23``: what fp32 arithmetic in ANY order guarantees for a K-term dot product of exact
    piece products (K - 1 additions: below gamma_K), plus two roundings for what the kernel forms around it (a class panel
    ``A + c B``, an epilogue's sum)."""
    return sum(k * U / (1.0 - k * U) + 2.0 ** -23 for k in ks)


def _kept(rows, n_kept, seed):
    g = th.Generator().manual_seed(seed)
    kept = th.randperm(rows, generator=g)[:n_kept].sort().values
    keep = th.zeros(rows, dtype=th.bool)
    keep[kept] = True
    return kept, keep


def _full(keep, vals, fill=NAN):
    """[rows, cols]: ``vals`` in the kept rows, ``fill`` (NaN: nothing of a dead row may be read) in the others"""
    out = th.full((keep.numel(), vals.size(1)), fill, dtype=th.float32)
    out[keep] = vals
    return out


def _sent(rows, cols, gpu):
    return th.full((rows, cols), SENT, device=gpu)


def _perm_pow2(k, rng):
    """[k, k] with one power of two (2^-2 .. 2^2) per row and column: a product with it permutes and scales columns exactly"""
    m = np.zeros((k, k), np.float32)
    m[np.arange(k), rng.permutation(k)] = np.exp2(rng.integers(-2, 3, k)).astype(np.float32)
    return th.from_numpy(m)


def _gpu_tiles(t, gpu):
    return tuple(x.to(gpu) if th.is_tensor(x) else x for x in t)


class _Rec(dict):
    """{scenario: {output: record}} of one kernel"""

    def ladder(self, scenario, output, got, ref64, keep=None, full=None, exact=True):
        """``got`` / ``ref64``: the kept rows (or a whole reduced product); ``full``: the whole output buffer, whose dead rows must hold
        the sentinel; ``exact``: a pass-through stage was bit for bit what it should be"""
        err, ok = rel_elem(got, ref64)
        if full is not None:
            ok = ok and bool((full.cpu()[~keep] == SENT).all())
        self.setdefault(scenario, {})[output] = dict(kind="ladder", err=err, ok=bool(ok and exact))

    def envelope(self, scenario, output, got, ref64, scale64, bound, route=None, keep=None, full=None):
        got, ref64, scale64 = got.double().cpu(), ref64.cpu(), scale64.cpu()
        nz = scale64 > 0
        ok = bool(th.isfinite(got).all())
        if full is not None:
            ok = ok and bool((full.cpu()[~keep] == SENT).all())
        rel = lambda t: float(((t.double().cpu() - ref64).abs()[nz] / scale64[nz]).max()) if bool(nz.any()) else 0.0
        r = dict(kind="tiny" if scenario == "tiny" else "envelope", err=rel(got), bound=bound, ok=ok)
        if route is not None:
            r["route"] = rel(route)
        self.setdefault(scenario, {})[output] = r


def _exact(lib, fn):
    """fn() under the exact-fp32 switch: the replaced launches on the f32-input MFMA"""
    assert not lib.dmp_dev_get_exact_fp32()
    lib.dmp_dev_set_exact_fp32(1)
    try:
        return fn()
    finally:
        lib.dmp_dev_set_exact_fp32(0)


def _cancel_weight(gen, cols=H):
    """[H, cols] whose rows k and k + H/2 are equal: against ``cancel`` (columns k and k + H/2 hold x and -x) every exact result is 0"""
    half = th.randn(H // 2, cols, generator=gen) * 0.1
    return th.cat([half, half], 0)


def operands(rows, h, gen):
    """``bf16x6_cases.scenarios`` with ``tiny`` = magnitudes FROM 2^-118 up (sign(x) max(|x|, 1) 2^-118).  An element there loses at most
    half a bf16 subnormal quantum, 2^-134: 2^-16 of itself, hence of the natural scale.  N(0, 1) 2^-118 also holds elements far below
    2^-118, which lose more of themselves; a 128-term scale averages that out, the 12- to 40-term sums of the code kernels do not (an
    emulation of ``split_pair`` gives 3.5e-5 of a 12-term natural scale, what the kernel gives), and no kernel could do better."""
    out = scenarios(rows, h, gen)
    t = out["tiny"] * 2.0 ** 118
    out["tiny"] = th.sign(t) * t.abs().clamp(min=1.0) * 2.0 ** -118
    return out


def _env_operands(gen):
    """{scenario: [ENV_KEPT, H]} with ``tiny``"""
    return operands(ENV_KEPT, H, gen)


# ---------------------------------------------------------------------------------------------------- csrc/dmp_h1w.hip
def bwd_h1_w(gpu, codes):
    """``dPre = d_o W2`` (slope 1.0), ``dW = d_o^T h1`` and with ``codes`` the block ``[enc^T dPre | (coef enc)^T dPre | enc^T d_o]``"""
    from dualmessagepassing_amd import _lib, fused
    lib = _lib.load()
    rec = _Rec()
    rng = np.random.default_rng(31 + int(codes))
    K, KPAD = 16, 16
    kept, keep = _kept(LADDER_ROWS, LADDER_KEPT, 1)
    T = _tiles(kept, LADDER_ROWS, gpu)

    def launch(d_o, W2, h1, T, rows, enc=None, coef_e=None):
        out = _sent(rows, H, gpu)
        kw = {}
        if codes:
            if enc is None:
                enc, coef_e = th.zeros(rows, KPAD, device=gpu), th.ones(rows, device=gpu)
            kw = dict(codes=dict(enc=enc, K=K, coef_e=coef_e, rows=(0, rows), residual=True))
        return (out,) + tuple(fused.bwd_h1_w(d_o, W2, h1, T, 1.0, out=out, **kw))[1:]

    # the sparse ladder, both products of one launch: with 128 kept rows the one column per row is a permutation of the block
    do_k, h1_k, W2 = ladder_rows(LADDER_KEPT, H, rng), ladder_dense((LADDER_KEPT, H), rng), ladder_dense((H, H), rng)
    res = launch(_full(keep, do_k).to(gpu), W2.to(gpu), _full(keep, h1_k).to(gpu), T, LADDER_ROWS)
    rec.ladder("ladder", "dPre", res[0].cpu()[keep], do_k.double() @ W2.double(), keep, res[0])
    rec.ladder("ladder", "dW", res[3], do_k.double().t() @ h1_k.double())
    if codes:
        # the codes block: dPre a dense ladder bit for bit (W2 a power-of-two permutation), 16 code rows at a time so that each of the
        # [K, 3H] sums is one product; the eight groups cover every kept row
        do_k, W2 = ladder_dense((LADDER_KEPT, H), rng), _perm_pow2(H, rng)
        dpre = do_k @ W2                                                           # exact: one power of two per column
        worst = [(0.0, True)] * 3
        same = True
        for grp in range(LADDER_KEPT // K):
            enc_k = th.zeros(LADDER_KEPT, KPAD)
            enc_k[grp * K:(grp + 1) * K, :K] = _code_block(K, rng)
            coef_k = th.from_numpy(np.exp2(rng.integers(-3, 0, LADDER_KEPT)).astype(np.float32))
            res = launch(_full(keep, do_k).to(gpu), W2.to(gpu), th.ones(LADDER_ROWS, H, device=gpu), T, LADDER_ROWS,
                         _full(keep, enc_k, 0.0).to(gpu), _full(keep, coef_k.view(-1, 1)).view(-1).to(gpu))
            same = same and th.equal(res[0].cpu()[keep], dpre)
            e, ce = enc_k[:, :K].double(), (enc_k[:, :K] * coef_k.view(-1, 1)).double()
            for b, want in enumerate((e.t() @ dpre.double(), ce.t() @ dpre.double(), e.t() @ do_k.double())):
                err, ok = rel_elem(res[4][:, b * H:(b + 1) * H], want)
                worst[b] = (max(worst[b][0], err), worst[b][1] and ok)
        for b, name in enumerate(("enc^T dPre", "(coef enc)^T dPre", "enc^T d_o")):
            rec.setdefault("ladder", {})[name] = dict(kind="ladder", err=worst[b][0], ok=bool(worst[b][1] and same))
    # the adversarial operands; the replaced route: bwd_h1_typed + atb_typed(plain=True) on the f32-input MFMA
    gen = th.Generator().manual_seed(41 + int(codes))
    kept, keep = _kept(ENV_ROWS, ENV_KEPT, 2)
    T = _tiles(kept, ENV_ROWS, gpu)
    W2 = _cancel_weight(gen)
    W2d = W2.double()
    for name, z in _env_operands(gen).items():
        h1_k = th.randn(ENV_KEPT, H, generator=gen)
        enc_k = th.zeros(ENV_KEPT, KPAD)
        enc_k[:, :K] = (th.rand(ENV_KEPT, K, generator=gen) < 0.5).float()
        coef_k = 1.0 / th.randint(1, 8, (ENV_KEPT,), generator=gen).float()
        d_o, h1 = _full(keep, z).to(gpu), _full(keep, h1_k).to(gpu)
        res = launch(d_o, W2.to(gpu), h1, T, ENV_ROWS, _full(keep, enc_k, 0.0).to(gpu), _full(keep, coef_k.view(-1, 1)).view(-1).to(gpu))

        def route():
            dg = fused.bwd_h1_typed(d_o, W2.to(gpu), h1, T, 1.0, out=_sent(ENV_ROWS, H, gpu))[0]
            with _LiveTiles(fused, T):
                return dg, fused.atb_typed(d_o, h1, None, None, gate=None, plain=True)

        rdg, rdw = _exact(lib, route)
        zd = z.double()
        s_pre = zd.abs() @ W2d.abs()
        rec.envelope(name, "dPre", res[0].cpu()[keep], zd @ W2d, s_pre, stage_bound(H), rdg.cpu()[keep], keep, res[0])
        if name != "cancel":                                                       # (single products only)
            rec.envelope(name, "dW", res[3], zd.t() @ h1_k.double(), zd.abs().t() @ h1_k.double().abs(), stage_bound(ENV_KEPT), rdw)
            if codes:
                e, ce = enc_k[:, :K].double(), (enc_k[:, :K] * coef_k.view(-1, 1)).double()
                want = th.cat([e.t() @ (zd @ W2d), ce.t() @ (zd @ W2d), e.t() @ zd], 1)
                scale = th.cat([e.t() @ s_pre, ce.t() @ s_pre, e.t() @ zd.abs()], 1)
                rec.envelope(name, "codes block", res[4], want, scale, stage_bound(H, ENV_KEPT))
    return rec


def _code_block(k, rng):
    """[k, k]: a ladder value per row in column ``pi(row)``"""
    m = np.zeros((k, k), np.float32)
    m[np.arange(k), rng.permutation(k)] = ladder((k,), rng)[0]
    return th.from_numpy(m)


def _class_case(rows, n_kept, seed, coefs):
    """kept rows in two degree classes (a partial tile each at 128 kept), the class tiles and each kept row's coefficient"""
    kept, keep = _kept(rows, n_kept, seed)
    cls = th.zeros(rows, dtype=th.long)
    cls[kept[n_kept * 3 // 8:]] = 1                                               # 48 and 80 of 128: 1.5 and 2.5 tiles
    tiles = _class_tiles(kept, cls, coefs, rows)
    ce = th.tensor(coefs, dtype=th.float64)[cls[keep]].view(-1, 1)
    return kept, keep, cls, tiles, ce


def _graph_index(rows, gpu, seed):
    """A real ``GraphIndex`` over ``rows`` edges (what ``bwd_z_w`` reads of it: the destinations and the reverse flags)"""
    from dualmessagepassing_amd.graph import GraphIndex
    rng = np.random.default_rng(seed)
    n = max(2, rows // 6)
    src, dst = rng.integers(0, n, rows).astype(np.int64), rng.integers(0, n, rows).astype(np.int64)
    return GraphIndex(th.from_numpy(src).to(gpu), th.from_numpy(dst).to(gpu), n, th.from_numpy(rng.random(rows) < 0.5).to(gpu)), n


def bwd_z_w(gpu):
    """``dz = dPre (A + c B)^T`` over the class tiles and ``dWes = [z^T dPre | z^T (c dPre)]`` (no base, ``d_s`` = 0)"""
    from dualmessagepassing_amd import fused
    rec = _Rec()
    rng = np.random.default_rng(51)

    def launch(dpre, z, wes, tiles, ix, n, rows):
        gate = th.ones(rows, device=gpu)
        real = fused.dead_rows_buffer
        fused.dead_rows_buffer = lambda shape, dev: th.full(shape, SENT, dtype=th.float32, device=dev)
        try:
            with _LiveTiles(fused, _gpu_tiles(tiles, gpu)):
                res = fused.bwd_z_w(dpre, z, wes, th.zeros(n, 2 * H, device=gpu), None, None, ix, gate=gate, dead_rows="leave")
        finally:
            fused.dead_rows_buffer = real
        assert res is not None
        return res

    coefs = (0.5, 0.25)                                                           # powers of two: c B and c dPre stay ladder values
    kept, keep, cls, tiles, ce = _class_case(LADDER_ROWS, LADDER_KEPT, 3, coefs)
    ix, n = _graph_index(LADDER_ROWS, gpu, 3)
    dp_k, z_k, L = ladder_rows(LADDER_KEPT, H, rng), ladder_dense((LADDER_KEPT, H), rng), ladder_dense((H, H), rng)
    zero = th.zeros(H, H)
    for half, wes in (("A", th.cat([L.t(), zero], 1)), ("B", th.cat([zero, L.t()], 1))):      # Wes = [A | B], dz = dPre (A + c B)^T
        dz, dw = launch(_full(keep, dp_k).to(gpu), _full(keep, z_k).to(gpu), wes.contiguous().to(gpu), tiles, ix, n, LADDER_ROWS)
        want = dp_k.double() @ L.double()
        rec.ladder("ladder", "dz panel " + half, dz.cpu()[keep], want if half == "A" else ce * want, keep, dz)
    rec.ladder("ladder", "dWes", dw, th.cat([z_k.double().t() @ dp_k.double(), z_k.double().t() @ (ce * dp_k.double())], 1))
    gen = th.Generator().manual_seed(52)
    coefs = (0.5, 1.0 / 3.0)
    kept, keep, cls, tiles, ce = _class_case(ENV_ROWS, ENV_KEPT, 4, coefs)
    ix, n = _graph_index(ENV_ROWS, gpu, 4)
    w = _cancel_weight(gen, 2 * H)                                               # (A^T | B^T): the structure on the contraction index
    wes = th.cat([w[:, :H].t(), w[:, H:].t()], 1).contiguous()
    wd = w.double()
    for name, dp in _env_operands(gen).items():
        z_k = th.randn(ENV_KEPT, H, generator=gen)
        dz, dw = launch(_full(keep, dp).to(gpu), _full(keep, z_k).to(gpu), wes.to(gpu), tiles, ix, n, ENV_ROWS)
        dd, zd = dp.double(), z_k.double()
        rec.envelope(name, "dz", dz.cpu()[keep], dd @ wd[:, :H] + ce * (dd @ wd[:, H:]), dd.abs() @ wd[:, :H].abs() + ce * (dd.abs() @ wd[:, H:].abs()),
                     stage_bound(H), None, keep, dz)
        if name != "cancel":
            rec.envelope(name, "dWes", dw, th.cat([zd.t() @ dd, zd.t() @ (ce * dd)], 1), th.cat([zd.abs().t() @ dd.abs(), zd.abs().t() @ (ce * dd.abs())], 1),
                         stage_bound(ENV_KEPT))
    return rec


def atb2(gpu):
    """``a^T b`` for two pairs of one launch, and the wide form ``[a^T b | a^T (c b)]`` over class tiles"""
    from dualmessagepassing_amd import fused
    rec = _Rec()
    rng = np.random.default_rng(61)
    kept, keep = _kept(LADDER_ROWS, LADDER_KEPT, 5)
    T = _tiles(kept, LADDER_ROWS, gpu)
    a = [ladder_rows(LADDER_KEPT, H, rng)[th.from_numpy(rng.permutation(LADDER_KEPT))] for _ in range(2)]
    b = [ladder_dense((LADDER_KEPT, H), rng) for _ in range(2)]
    dev = lambda t: _full(keep, t).to(gpu)
    assert fused.atb2_ok(dev(a[0]), dev(b[0]), H)
    got = fused.atb2([(dev(a[0]), dev(b[0])), (dev(a[1]), dev(b[1]))], T)
    for j in range(2):
        rec.ladder("ladder", "job %d" % j, got[j], a[j].double().t() @ b[j].double())
    _, keepc, _, tiles, ce = _class_case(LADDER_ROWS, LADDER_KEPT, 5, (0.5, 0.25))
    got = fused.atb2([(_full(keepc, a[0]).to(gpu), _full(keepc, b[0]).to(gpu))], _gpu_tiles(tiles, gpu), wide=True)[0]
    rec.ladder("ladder", "wide", got, th.cat([a[0].double().t() @ b[0].double(), a[0].double().t() @ (ce * b[0].double())], 1))
    gen = th.Generator().manual_seed(62)
    kept, keep = _kept(ENV_ROWS, ENV_KEPT, 6)
    T = _tiles(kept, ENV_ROWS, gpu)
    _, keepc, _, tiles, ce = _class_case(ENV_ROWS, ENV_KEPT, 6, (0.5, 1.0 / 3.0))
    for name, z in _env_operands(gen).items():
        if name == "cancel":
            continue
        d = th.randn(ENV_KEPT, H, generator=gen)
        zd, dd = z.double(), d.double()
        got = fused.atb2([(_full(keep, z).to(gpu), _full(keep, d).to(gpu)), (_full(keep, d).to(gpu), _full(keep, z).to(gpu))], T)
        rec.envelope(name, "job 0", got[0], zd.t() @ dd, zd.abs().t() @ dd.abs(), stage_bound(ENV_KEPT))
        rec.envelope(name, "job 1", got[1], dd.t() @ zd, dd.abs().t() @ zd.abs(), stage_bound(ENV_KEPT))
        got = fused.atb2([(_full(keepc, z).to(gpu), _full(keepc, d).to(gpu))], _gpu_tiles(tiles, gpu), wide=True)[0]
        rec.envelope(name, "wide", got, th.cat([zd.t() @ dd, zd.t() @ (ce * dd)], 1), th.cat([zd.abs().t() @ dd.abs(), zd.abs().t() @ (ce * dd.abs())], 1),
                     stage_bound(ENV_KEPT))
    return rec


# ---------------------------------------------------------------------------------------------------- csrc/dmp_typed.hip: the codes k-group
def out_fwd_typed_codes(gpu):
    """``h1 W2t + enc[:, :K] Wc``: the codes k-group with ``h1`` = 0, then the converse"""
    from dualmessagepassing_amd import _lib, fused
    lib = _lib.load()
    rec = _Rec()
    rng = np.random.default_rng(71)
    K, KPAD = 16, 16
    kept, keep = _kept(LADDER_ROWS, LADDER_KEPT, 7)
    T = _tiles(kept, LADDER_ROWS, gpu)

    def launch(h1, W2t, enc, Wc, T, rows):
        out = _sent(rows, H, gpu)
        assert fused.out_codes_ok(h1, enc, K, Wc)
        fused.out_fwd_typed_codes(h1, W2t, None, enc, K, Wc, T, out=out)
        return out

    enc_k, Wc = ladder_rows(LADDER_KEPT, K, rng), ladder_dense((K, H), rng)
    h1_k, W2t = ladder_rows(LADDER_KEPT, H, rng), ladder_dense((H, H), rng)
    zeros_k = th.zeros(LADDER_KEPT, H)
    out = launch(_full(keep, zeros_k).to(gpu), W2t.to(gpu), _full(keep, enc_k).to(gpu), Wc.to(gpu), T, LADDER_ROWS)
    rec.ladder("ladder", "codes k-group", out.cpu()[keep], enc_k.double() @ Wc.double(), keep, out)
    out = launch(_full(keep, h1_k).to(gpu), W2t.to(gpu), _full(keep, th.zeros(LADDER_KEPT, KPAD)).to(gpu), Wc.to(gpu), T, LADDER_ROWS)
    rec.ladder("ladder", "h1 W2t", out.cpu()[keep], h1_k.double() @ W2t.double(), keep, out)
    # adversarial: both terms at once; the replaced route: smallk_embed + out_fwd_typed on the f32-input MFMA
    gen = th.Generator().manual_seed(72)
    kept, keep = _kept(ENV_ROWS, ENV_KEPT, 8)
    T = _tiles(kept, ENV_ROWS, gpu)
    W2t = _cancel_weight(gen)
    Wc = th.randn(K, H, generator=gen) * 0.1
    for name, z in _env_operands(gen).items():
        magnitude = z.abs().max(1, keepdim=True).values                           # the codes term at the row's own magnitude
        enc_k = (th.rand(ENV_KEPT, K, generator=gen) < 0.5).float() * th.exp2(th.floor(th.log2(magnitude.clamp(min=2.0 ** -126))))
        if name == "cancel":
            enc_k = th.zeros(ENV_KEPT, K)
        h1, enc = _full(keep, z).to(gpu), _full(keep, enc_k).to(gpu)
        out = launch(h1, W2t.to(gpu), enc, Wc.to(gpu), T, ENV_ROWS)

        def route():
            z0 = th.zeros(ENV_ROWS, H, device=gpu)
            z0[keep.to(gpu)] = fused.smallk_embed(enc[keep.to(gpu)][:, :K].contiguous(), Wc.to(gpu))
            o = _sent(ENV_ROWS, H, gpu)
            fused.out_fwd_typed(h1, W2t.to(gpu), None, z0, T, out=o)
            return o

        old = _exact(lib, route)
        zd, ed = z.double(), enc_k.double()
        rec.envelope(name, "out", out.cpu()[keep], zd @ W2t.double() + ed @ Wc.double(), zd.abs() @ W2t.double().abs() + ed.abs() @ Wc.double().abs(),
                     stage_bound(H + K), old.cpu()[keep], keep, out)
    return rec


# ---------------------------------------------------------------------------------------------------- csrc/dmp_edgemlp.hip
def edge_mlp_fwd(gpu):
    """``H1e = z (A + c B)`` (no gathers, no bias, slope 1.0) and ``zn = H1e W2t``"""
    from dualmessagepassing_amd import _lib, fused
    lib = _lib.load()
    rec = _Rec()
    rng = np.random.default_rng(81)

    def launch(z, wes, W2t, tiles, rows, n):
        h1, zn = _sent(rows, H, gpu), _sent(rows, H, gpu)
        P, zb = th.zeros(n, 3 * H, device=gpu), th.zeros(H, device=gpu)
        sel = (th.full((rows,), -1, dtype=th.int32, device=gpu), th.full((rows,), -1, dtype=th.int32, device=gpu))
        assert fused.edge_mlp_fwd_ok(H, z, P[:, H:], W2t)
        fused.edge_mlp_fwd(z, wes, P[:, H:], 3 * H, zb, None, _Index(n, rows), 1.0, W2t, zb, None, _gpu_tiles(tiles, gpu), sel=sel, h1=h1, out=zn)
        return h1, zn

    coefs = (0.5, 0.25)
    kept, keep, cls, tiles, ce = _class_case(LADDER_ROWS, LADDER_KEPT, 9, coefs)
    z_k, L, L2 = ladder_rows(LADDER_KEPT, H, rng), ladder_dense((H, H), rng), ladder_dense((H, H), rng)
    zero = th.zeros(H, H)
    for half, wes in (("A", th.cat([L, zero], 1)), ("B", th.cat([zero, L], 1))):
        h1, zn = launch(_full(keep, z_k).to(gpu), wes.to(gpu), L2.to(gpu), tiles, LADDER_ROWS, 8)
        want = z_k.double() @ L.double()
        rec.ladder("ladder", "H1e panel " + half, h1.cpu()[keep], want if half == "A" else ce * want, keep, h1)
    # the second Linear: the first an exact pass-through (a power-of-two permutation), H1e the permuted ladder rows bit for bit
    Pm = _perm_pow2(H, rng)
    h1, zn = launch(_full(keep, z_k).to(gpu), th.cat([Pm, zero], 1).to(gpu), L2.to(gpu), tiles, LADDER_ROWS, 8)
    through = z_k @ Pm
    rec.ladder("ladder", "zn", zn.cpu()[keep], through.double() @ L2.double(), keep, zn, exact=th.equal(h1.cpu()[keep], through))
    # adversarial; the replaced route: edge_fwd_typed + out_fwd_typed on the f32-input MFMA
    gen = th.Generator().manual_seed(82)
    coefs = (0.5, 1.0 / 3.0)
    kept, keep, cls, tiles, ce = _class_case(ENV_ROWS, ENV_KEPT, 10, coefs)
    asc = _gpu_tiles(_ascending_tiles(kept, ENV_ROWS), gpu)
    wes = _cancel_weight(gen, 2 * H)
    W2t = th.randn(H, H, generator=gen) / H ** 0.5
    wd, w2d = wes.double(), W2t.double()
    for name, z in _env_operands(gen).items():
        if name == "cancel":
            continue                                                               # (a chain: not a single product)
        zg = _full(keep, z).to(gpu)
        h1, zn = launch(zg, wes.to(gpu), W2t.to(gpu), tiles, ENV_ROWS, 8)

        def route():
            P = th.zeros(8, 3 * H, device=gpu)
            sel = (th.full((ENV_ROWS,), -1, dtype=th.int32, device=gpu), th.full((ENV_ROWS,), -1, dtype=th.int32, device=gpu))
            real = fused.dead_rows_buffer
            fused.dead_rows_buffer = lambda shape, dev: th.full(shape, SENT, dtype=th.float32, device=dev)
            try:
                with _LiveTiles(fused, _gpu_tiles(tiles, gpu)):
                    oh1 = fused.edge_fwd_typed(zg, wes.to(gpu), P[:, H:], 3 * H, None, None, _Index(8, ENV_ROWS), 1.0,
                                               dead_gate=th.ones(ENV_ROWS, device=gpu), sel=sel)
            finally:
                fused.dead_rows_buffer = real
            ozn = _sent(ENV_ROWS, H, gpu)
            fused.out_fwd_typed(oh1, W2t.to(gpu), None, None, asc, out=ozn)
            return oh1, ozn

        oh1, ozn = _exact(lib, route)
        zd = z.double()
        r1 = zd @ wd[:, :H] + ce * (zd @ wd[:, H:])
        s1 = zd.abs() @ wd[:, :H].abs() + ce * (zd.abs() @ wd[:, H:].abs())
        rec.envelope(name, "H1e", h1.cpu()[keep], r1, s1, stage_bound(H), oh1.cpu()[keep], keep, h1)
        rec.envelope(name, "zn", zn.cpu()[keep], r1 @ w2d, s1 @ w2d.abs(), stage_bound(H, H), ozn.cpu()[keep], keep, zn)
    return rec


# ---------------------------------------------------------------------------------------------------- csrc/dmp_nodechain.hip
def node_chain(gpu):
    """Both passes of the kept-node chain, every one of its twelve packed panels on the ladder once"""
    from dualmessagepassing_amd import _lib, fused
    lib = _lib.load()
    rec = _Rec()
    rng = np.random.default_rng(91)
    zero = th.zeros(H, H)

    def fwd(x, S, Wx, Bn, W2, T, rows):
        assert fused.node_chain_ok(H, x, S, Bn, Wx, W2)
        pf, _ = fused.node_chain_panels(Bn, Wx, W2)
        H1n, XP, xn = _sent(rows, H, gpu), _sent(rows, 3 * H, gpu), _sent(rows, H, gpu)
        fused.node_chain_fwd(x, S, pf, th.zeros(H, device=gpu), th.zeros(H, device=gpu), False, 1.0, T, H1n, XP[:, H:], xn)
        return H1n, XP[:, H:], xn

    def bwd(dxn, H1, dP, Wx, Bn, W2, T, rows):
        _, pb = fused.node_chain_panels(Bn, Wx, W2)
        dXP = _sent(rows, 3 * H, gpu)
        dXP[:, H:] = dP
        dS, dx = _sent(rows, 2 * H, gpu), _sent(rows, H, gpu)
        with fused.deferred_reductions():
            fused.node_chain_bwd(dxn, H1, dXP[:, H:], pb, False, 1.0, T, dXP[:, :H], dS, dx)
        return dXP[:, :H], dS, dx

    kept, keep = _kept(LADDER_ROWS, LADDER_KEPT, 11)
    T = _tiles(kept, LADDER_ROWS, gpu)
    a_k = ladder_rows(LADDER_KEPT, H, rng)                                        # the sparse streamed operand of every configuration
    L = [ladder_dense((H, H), rng) for _ in range(3)]
    ad = a_k.double()
    dev = lambda t: _full(keep, t).to(gpu)
    zk, zk2 = th.zeros(LADDER_KEPT, H), th.zeros(LADDER_KEPT, 2 * H)
    # forward, first stage: x against Wx0 | Wx1 | Wx2; S_in against Bn_in; S_out against Bn_out
    H1n, P, _ = fwd(dev(a_k), dev(zk2), th.cat(L, 1).to(gpu), th.zeros(2 * H, H, device=gpu), zero.to(gpu), T, LADDER_ROWS)
    rec.ladder("ladder", "H1n of x Wx0", H1n.cpu()[keep], ad @ L[0].double(), keep, H1n)
    rec.ladder("ladder", "P", P.cpu()[keep], th.cat([ad @ L[1].double(), ad @ L[2].double()], 1), keep, P)
    for half, S_k, Bn in (("in", th.cat([a_k, zk], 1), th.cat([L[0], zero], 0)), ("out", th.cat([zk, a_k], 1), th.cat([zero, L[1]], 0))):
        H1n, _, _ = fwd(dev(zk), dev(S_k), th.zeros(H, 3 * H, device=gpu), Bn.to(gpu), zero.to(gpu), T, LADDER_ROWS)
        rec.ladder("ladder", "H1n of S_%s Bn_%s" % (half, half), H1n.cpu()[keep], ad @ L[0 if half == "in" else 1].double(), keep, H1n)
    # forward, second stage: Wx0 a power-of-two permutation, H1n the permuted ladder rows bit for bit, xn = H1n W2^T
    Pm = _perm_pow2(H, rng)
    through = a_k @ Pm
    H1n, _, xn = fwd(dev(a_k), dev(zk2), th.cat([Pm, zero, zero], 1).to(gpu), th.zeros(2 * H, H, device=gpu), L[2].to(gpu), T, LADDER_ROWS)
    rec.ladder("ladder", "xn", xn.cpu()[keep], through.double() @ L[2].double().t(), keep, xn, exact=th.equal(H1n.cpu()[keep], through))
    # backward, first stage: dPn = dxn W2
    ones = th.ones(LADDER_ROWS, H, device=gpu)
    zw, zb = th.zeros(H, 3 * H, device=gpu), th.zeros(2 * H, H, device=gpu)
    dPn, _, _ = bwd(dev(a_k), ones, dev(zk2), zw, zb, L[0].to(gpu), T, LADDER_ROWS)
    rec.ladder("ladder", "dPn", dPn.cpu()[keep], ad @ L[0].double(), keep, dPn)
    # backward, second stage: W2 a permutation, dPn bit for bit; dS = [dPn Bn_in^T | dPn Bn_out^T], dx = dPn Wx0^T
    dPn, dS, dx = bwd(dev(a_k), ones, dev(zk2), th.cat([L[2], zero, zero], 1).to(gpu), th.cat([L[0], L[1]], 0).to(gpu), Pm.to(gpu), T, LADDER_ROWS)
    td = through.double()
    same = th.equal(dPn.cpu()[keep], through)
    rec.ladder("ladder", "dS", dS.cpu()[keep], th.cat([td @ L[0].double().t(), td @ L[1].double().t()], 1), keep, dS, exact=same)
    rec.ladder("ladder", "dx of dPn Wx0^T", dx.cpu()[keep], td @ L[2].double().t(), keep, dx, exact=same)
    # backward: dx of dP's halves against Wx1^T and Wx2^T (dxn = 0: dPn = 0)
    for j in (1, 2):
        dP_k = th.cat([a_k, zk], 1) if j == 1 else th.cat([zk, a_k], 1)
        Wx = th.cat([zero] * j + [L[j]] + [zero] * (2 - j), 1)
        _, _, dx = bwd(dev(zk), ones, dev(dP_k), Wx.to(gpu), zb, zero.to(gpu), T, LADDER_ROWS)
        rec.ladder("ladder", "dx of dP%d Wx%d^T" % (j, j), dx.cpu()[keep], ad @ L[j].double().t(), keep, dx)
    # adversarial; the replaced route: typed_jobs / out_fwd_typed / bwd_h1_typed on the f32-input MFMA
    gen = th.Generator().manual_seed(92)
    kept, keep = _kept(ENV_ROWS, ENV_KEPT, 12)
    T = _tiles(kept, ENV_ROWS, gpu)
    r = lambda *s: th.randn(*s, generator=gen)
    Wx, Bn, W2 = r(H, 3 * H) / (3 * H) ** 0.5, r(2 * H, H) / (3 * H) ** 0.5, r(H, H) / H ** 0.5
    Wxg, Bng, W2g = Wx.to(gpu), Bn.to(gpu), W2.to(gpu)
    Wxd, Bnd, W2d = Wx.double(), Bn.double(), W2.double()
    for name, z in _env_operands(gen).items():
        if name == "cancel":
            continue                                                               # (a chain: not a single product)
        S_k = th.cat([z.flip(1), z.roll(1, 0)], 1)                                 # operands of the row's own magnitudes
        x, S = dev(z), dev(S_k)
        H1n, P, xn = fwd(x, S, Wxg, Bng, W2g, T, ENV_ROWS)

        def route_f():
            oH1, oXP, oxn, T1 = _sent(ENV_ROWS, H, gpu), _sent(ENV_ROWS, 3 * H, gpu), _sent(ENV_ROWS, H, gpu), _sent(ENV_ROWS, H, gpu)
            fused.typed_jobs([dict(a=x, W=Wxg[:, :H], out=oXP[:, :H]), dict(a=S[:, :H], W=Bng[:H], out=T1),
                              dict(a=x, W=Wxg[:, H:2 * H], out=oXP[:, H:2 * H]), dict(a=x, W=Wxg[:, 2 * H:], out=oXP[:, 2 * H:])], T)
            fused.out_fwd_typed(S[:, H:], Bng[H:], None, oXP[:, :H], T, out=oH1, slope=1.0, prev2=T1)
            fused.out_fwd_typed(oH1, W2g, None, None, T, out=oxn, w_in_out=False)
            return oH1, oXP[:, H:], oxn

        oH1, oP, oxn = _exact(lib, route_f)
        zd, sd = z.double(), S_k.double()
        r1 = zd @ Wxd[:, :H] + sd @ Bnd
        s1 = zd.abs() @ Wxd[:, :H].abs() + sd.abs() @ Bnd.abs()
        rec.envelope(name, "H1n", H1n.cpu()[keep], r1, s1, stage_bound(3 * H), oH1.cpu()[keep], keep, H1n)
        rec.envelope(name, "P", P.cpu()[keep], zd @ Wxd[:, H:], zd.abs() @ Wxd[:, H:].abs(), stage_bound(H), oP.cpu()[keep], keep, P)
        rec.envelope(name, "xn", xn.cpu()[keep], r1 @ W2d.t(), s1 @ W2d.t().abs(), stage_bound(3 * H, H), oxn.cpu()[keep], keep, xn)
        # backward on the same operands: dxn = z, dP = S
        ones = th.ones(ENV_ROWS, H, device=gpu)
        dPn, dS, dx = bwd(x, ones, S, Wxg, Bng, W2g, T, ENV_ROWS)

        def route_b():
            oXP = _sent(ENV_ROWS, 3 * H, gpu)
            oXP[:, H:] = S
            oS, oU, odx = _sent(ENV_ROWS, 2 * H, gpu), _sent(ENV_ROWS, 2 * H, gpu), _sent(ENV_ROWS, H, gpu)
            fused.bwd_h1_typed(x, W2g, ones, T, 1.0, out=oXP[:, :H])
            fused.typed_jobs([dict(a=oXP[:, :H], W=Bng[:H], w_in_out=False, out=oS[:, :H]), dict(a=oXP[:, :H], W=Bng[H:], w_in_out=False, out=oS[:, H:]),
                              dict(a=oXP[:, :H], W=Wxg[:, :H], w_in_out=False, out=oU[:, :H]),
                              dict(a=oXP[:, H:2 * H], W=Wxg[:, H:2 * H], w_in_out=False, out=oU[:, H:])], T)
            fused.out_fwd_typed(oXP[:, 2 * H:], Wxg[:, 2 * H:], None, oU[:, :H], T, out=odx, w_in_out=False, prev2=oU[:, H:])
            return oXP[:, :H], oS, odx

        odPn, odS, odx = _exact(lib, route_b)
        rp, sp = zd @ W2d, zd.abs() @ W2d.abs()
        rec.envelope(name, "dPn", dPn.cpu()[keep], rp, sp, stage_bound(H), odPn.cpu()[keep], keep, dPn)
        rec.envelope(name, "dS", dS.cpu()[keep], th.cat([rp @ Bnd[:H].t(), rp @ Bnd[H:].t()], 1),
                     th.cat([sp @ Bnd[:H].t().abs(), sp @ Bnd[H:].t().abs()], 1), stage_bound(H, H), odS.cpu()[keep], keep, dS)
        rec.envelope(name, "dx", dx.cpu()[keep], rp @ Wxd[:, :H].t() + sd @ Wxd[:, H:].t(), sp @ Wxd[:, :H].t().abs() + sd.abs() @ Wxd[:, H:].t().abs(),
                     stage_bound(H, 3 * H), odx.cpu()[keep], keep, dx)
    return rec


# ---------------------------------------------------------------------------------------------------- csrc/dmp_l0node.hip
L0_VK, L0_K0, L0_KP = 16, 12, 16                                                 # 40 code columns: [venc | S0_in | S0_out]
L0_COLS = L0_VK + 2 * L0_K0
L0_SPLIT = 37                                                                    # the second table's first row (inside a tile)


def _l0_node_case(rows, keep, x_k, W, gpu):
    """The case dict of tests/test_gpu_l0_node_mfma.py (its ``_new`` / ``_bwd_new`` drive the wrappers): the kept rows' 40 code columns
    ``x_k``, NaN in the padding columns and in every dead row, the kept nodes' list made by ``fused.kept_rows``"""
    from dualmessagepassing_amd import fused
    venc = _full(keep, x_k[:, :L0_VK])
    S0 = th.full((rows, 2 * L0_KP), NAN)
    S0[keep, :L0_K0] = x_k[:, L0_VK:L0_VK + L0_K0]
    S0[keep, L0_KP:L0_KP + L0_K0] = x_k[:, L0_VK + L0_K0:]
    kg = keep.to(gpu)
    mask = fused.gate_row_mask(kg.float())
    lst, cnt = fused.kept_rows(mask, 0, rows, tiles=True)
    assert int(cnt[0]) == int(keep.sum())
    return dict(n=rows, tables=2, vk=L0_VK, k0=L0_K0, kp=L0_KP, split=L0_SPLIT, first=0, keep=kg, venc=venc.to(gpu), S0=S0.to(gpu),
                W=None if W is None else W.to(gpu), bias=None, mask=mask, rows=(lst, cnt[0:1]))


def _l0_pack(Ws):
    """[tables, .., 3H] from per-table [40, 3H] matrices (the S0 blocks feed H1n alone: their P columns are not part of the product)"""
    from dualmessagepassing_amd import fused
    return th.stack([fused.l0_node_pack(L0_VK, L0_K0, H, w[:L0_VK], w[L0_VK:L0_VK + L0_K0, :H], w[L0_VK + L0_K0:, :H]) for w in Ws])


def _l0_node_ref(x_k, keep, Ws):
    """fp64 ``(H1n, P)`` of the kept rows and their natural scales: a row below the split takes the first table"""
    rows = th.arange(keep.numel())[keep]
    first = (rows < L0_SPLIT).view(-1, 1)
    xd = x_k.double()
    eff = []
    for w in Ws:
        w = w.double().clone()
        w[L0_VK:, H:] = 0.0
        eff.append(w)
    ref = th.where(first, xd @ eff[0], xd @ eff[1])
    scale = th.where(first, xd.abs() @ eff[0].abs(), xd.abs() @ eff[1].abs())
    return ref, scale


def l0_node_fwd_mfma(gpu):
    """``H1n = [venc | S0_in | S0_out] W_t[:, :H]`` (no bias, slope 1.0) and ``P = venc W_t[:, H:]``: the 32x32x16 sequence"""
    from test_gpu_l0_node_mfma import _new
    from dualmessagepassing_amd import fused
    rec = _Rec()
    rng = np.random.default_rng(101)

    def launch(rows, keep, x_k, Ws):
        c = _l0_node_case(rows, keep, x_k, _l0_pack(Ws), gpu)
        assert fused.l0_node_mfma_ok(H, L0_VK, L0_K0, L0_KP, 2, rows, c["venc"], c["S0"])
        h1, P = _new(c, 1.0, _sent(rows, H, gpu), _sent(rows, 2 * H, gpu))
        dead_ok = bool((h1.cpu()[~keep] == SENT).all()) and bool((P.cpu()[~keep] == 0).all())     # (a dead row's P: zeros)
        return h1.cpu()[keep], P.cpu()[keep], dead_ok

    kept, keep = _kept(LADDER_ROWS, LADDER_KEPT, 13)
    x_k = ladder_rows(LADDER_KEPT, L0_COLS, rng)
    Ws = [ladder_dense((L0_COLS, 3 * H), rng) for _ in range(2)]
    h1, P, dead_ok = launch(LADDER_ROWS, keep, x_k, Ws)
    ref, _ = _l0_node_ref(x_k, keep, Ws)
    rec.ladder("ladder", "H1n", h1, ref[:, :H], exact=dead_ok)
    rec.ladder("ladder", "P", P, ref[:, H:], exact=dead_ok)
    gen = th.Generator().manual_seed(102)
    kept, keep = _kept(ENV_ROWS, ENV_KEPT, 14)
    half = th.randn(L0_COLS // 2, 3 * H, generator=gen) * 0.1
    Ws = [th.cat([half, half], 0), th.cat([half, half], 0) * 0.5]                 # rows k and k + 20 equal: "cancel" over the 40 columns
    for name, x_k in operands(ENV_KEPT, L0_COLS, gen).items():
        h1, P, dead_ok = launch(ENV_ROWS, keep, x_k, Ws)
        ref, scale = _l0_node_ref(x_k, keep, Ws)
        rec.envelope(name, "H1n", h1, ref[:, :H], scale[:, :H], stage_bound(L0_COLS))
        if name != "cancel":                                                       # (P takes the venc columns alone: nothing cancels)
            rec.envelope(name, "P", P, ref[:, H:], scale[:, H:], stage_bound(L0_VK))
        rec[name]["H1n"]["ok"] = rec[name]["H1n"]["ok"] and dead_ok
    return rec


def l0_node_codes_bwd(gpu):
    """``Xn[h] = S0_h^T dPn`` per table and ``Yn[b] = venc^T (block b of [dPn | dP_dst | dP_src | dxn])``: the 16x16x32 sequence"""
    from test_gpu_l0_node_mfma import _bwd_new
    rec = _Rec()
    rng = np.random.default_rng(111)

    def want(x_k, keep, dXP_k, dxn_k, absolute=False):
        """fp64 ``(Xn [2, 2 K0, H], Yn [4, VK, H])`` over the kept rows (one venc table, two S0 tables)"""
        rows = th.arange(keep.numel())[keep]
        f = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
        x, blocks = f(x_k), [f(dXP_k[:, b * H:(b + 1) * H]) for b in range(3)] + [f(dxn_k)]
        X = th.zeros(2, 2 * L0_K0, H, dtype=th.float64)
        for t, sel in enumerate((rows < L0_SPLIT, rows >= L0_SPLIT)):
            for h in range(2):
                s = x[sel][:, L0_VK + h * L0_K0:L0_VK + (h + 1) * L0_K0]
                X[h, t * L0_K0:(t + 1) * L0_K0] = s.t() @ blocks[0][sel]
        Y = th.stack([x[:, :L0_VK].t() @ b for b in blocks])
        return X, Y

    def launch(rows, keep, x_k, dXP_k, dxn_k):
        c = _l0_node_case(rows, keep, x_k, None, gpu)
        return tuple(t.cpu() for t in _bwd_new(c, _full(keep, dXP_k).to(gpu), _full(keep, dxn_k).to(gpu), 1))

    # sixteen code rows at a time, a ladder value per code column in a row of its own (the S0 blocks: twelve of the sixteen), so that
    # each sum is one product; the eight groups cover every kept row and slot
    kept, keep = _kept(LADDER_ROWS, LADDER_KEPT, 15)
    dXP_k, dxn_k = ladder_dense((LADDER_KEPT, 3 * H), rng), ladder_dense((LADDER_KEPT, H), rng)
    worst = {"Xn": (0.0, True), "Yn": (0.0, True)}
    for grp in range(LADDER_KEPT // 16):
        x_k = th.zeros(LADDER_KEPT, L0_COLS)
        r0 = grp * 16
        x_k[r0:r0 + 16, :L0_VK] = _code_block(16, rng)
        for h in range(2):
            pick = th.from_numpy(rng.permutation(16)[:L0_K0]).long() + r0
            x_k[pick, L0_VK + h * L0_K0 + th.from_numpy(rng.permutation(L0_K0)).long()] = th.from_numpy(ladder((L0_K0,), rng)[0])
        Xn, Yn = launch(LADDER_ROWS, keep, x_k, dXP_k, dxn_k)
        X64, Y64 = want(x_k, keep, dXP_k, dxn_k)
        for name, got, ref in (("Xn", Xn, X64), ("Yn", Yn, Y64)):
            err, ok = rel_elem(got, ref)
            worst[name] = (max(worst[name][0], err), worst[name][1] and ok)
    for name, (err, ok) in worst.items():
        rec.setdefault("ladder", {})[name] = dict(kind="ladder", err=err, ok=bool(ok))
    gen = th.Generator().manual_seed(112)
    kept, keep = _kept(ENV_ROWS, ENV_KEPT, 16)
    for name, x_k in operands(ENV_KEPT, L0_COLS, gen).items():
        if name == "cancel":
            continue                                                               # (contracted over the rows: nothing cancels)
        dXP_k, dxn_k = th.randn(ENV_KEPT, 3 * H, generator=gen), th.randn(ENV_KEPT, H, generator=gen)
        Xn, Yn = launch(ENV_ROWS, keep, x_k, dXP_k, dxn_k)
        (X64, Y64), (XS, YS) = want(x_k, keep, dXP_k, dxn_k), want(x_k, keep, dXP_k, dxn_k, absolute=True)
        rec.envelope(name, "Xn", Xn, X64, XS, stage_bound(ENV_KEPT))
        rec.envelope(name, "Yn", Yn, Y64, YS, stage_bound(ENV_KEPT))
    return rec


# ---------------------------------------------------------------------------------------------------- csrc/dmp_l0mlp.hip
def l0_edge_mlp(gpu):
    """The one-launch ``l0_edge_fwd(mlp=...)``: ``H1e = enc M_t[:, :H] + coef_e enc M_t[:, H:]`` (no gathers, no bias, slope 1.0) and
    ``zn = H1e W2t + enc Wc``"""
    from test_gpu_l0_edge_mlp import _Index as _CodeIndex
    from dualmessagepassing_amd import fused
    rec = _Rec()
    rng = np.random.default_rng(121)
    K = 12                                                                        # (``dmp_l0_edge_mlp_max_codes``; rows of 12 floats)
    SPLIT = 37

    def launch(rows, keep, T, enc_k, coef_k, M, W2t, Wc, row0):
        enc = _full(keep, enc_k).to(gpu)
        minus = th.full((rows,), -1, dtype=th.int32, device=gpu)
        ix = _CodeIndex(8, minus, minus, _full(keep, coef_k.view(-1, 1)).view(-1).to(gpu))
        P = th.zeros(8, 3 * H, device=gpu)[:, H:]
        h1, zn = _sent(rows, H, gpu), _sent(rows, H, gpu)
        assert fused.l0_edge_mlp_ok(H, K, 2, enc, P, W2t.to(gpu))
        fused.out_fwd_typed_codes(h1, W2t.to(gpu), None, enc, K, Wc.to(gpu), T, prev=None, out=zn, row0=row0,
                                  first=dict(M=M.to(gpu), tables=2, split=SPLIT, P=P, ldp=3 * H, bias=None, coef=None, index=ix, slope=1.0))
        return h1, zn

    def tables(rows, keep, enc_k, coef_k, M, absolute=False):
        """fp64 ``enc M_t[:, :H] + coef enc M_t[:, H:]`` of the kept rows (a row below the split takes the first table)"""
        first = (th.arange(rows)[keep] < SPLIT).view(-1, 1)
        f = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
        e, m, c = f(enc_k), f(M), coef_k.double().view(-1, 1)
        one = lambda t: e @ m[t * K:(t + 1) * K, :H] + c * (e @ m[t * K:(t + 1) * K, H:])
        return th.where(first, one(0), one(1))

    kept, keep = _kept(LADDER_ROWS, LADDER_KEPT, 17)
    T = _tiles(kept, LADDER_ROWS, gpu)
    enc_k = ladder_rows(LADDER_KEPT, K, rng)
    coef_k = th.from_numpy(np.exp2(rng.integers(-3, 0, LADDER_KEPT)).astype(np.float32))      # powers of two: coef enc M stays a ladder product
    L, W2t, Wc = ladder_dense((2 * K, H), rng), ladder_dense((H, H), rng), ladder_dense((K, H), rng)
    zero = th.zeros(2 * K, H)
    for half, M in (("A", th.cat([L, zero], 1)), ("B", th.cat([zero, L], 1))):
        h1, _ = launch(LADDER_ROWS, keep, T, enc_k, coef_k, M, W2t, th.zeros(K, H), 0)
        rec.ladder("ladder", "H1e panel " + half, h1.cpu()[keep], tables(LADDER_ROWS, keep, enc_k, coef_k, M), keep, h1)
    # the codes k-group of the second role: M = 0, so H1e = 0 and zn = enc Wc
    h1, zn = launch(LADDER_ROWS, keep, T, enc_k, coef_k, th.zeros(2 * K, 2 * H), W2t, Wc, 0)
    rec.ladder("ladder", "zn of enc Wc", zn.cpu()[keep], enc_k.double() @ Wc.double(), keep, zn, exact=bool((h1.cpu()[keep] == 0).all()))
    # the second Linear: code column k passes through to column 12 i + k of H1e, scaled by a power of two (bit for bit); eleven launches
    # walk every row of W2t
    worst, ok, same = 0.0, True, True
    for i in range((H + K - 1) // K):
        M = th.zeros(2 * K, 2 * H)
        cols = (th.arange(K) + i * K) % H
        for t in range(2):
            M[t * K + th.arange(K), cols] = th.from_numpy(np.exp2(rng.integers(-2, 3, K)).astype(np.float32))
        h1, zn = launch(LADDER_ROWS, keep, T, enc_k, coef_k, M, W2t, th.zeros(K, H), 0)
        through = tables(LADDER_ROWS, keep, enc_k, coef_k, M).float()             # exact: one power of two per element
        same = same and th.equal(h1.cpu()[keep], through)
        err, good = rel_elem(zn.cpu()[keep], through.double() @ W2t.double())
        worst, ok = max(worst, err), ok and good and bool((zn.cpu()[~keep] == SENT).all())
    rec.setdefault("ladder", {})["zn of H1e W2t"] = dict(kind="ladder", err=worst, ok=bool(ok and same))
    gen = th.Generator().manual_seed(122)
    kept, keep = _kept(ENV_ROWS, ENV_KEPT, 18)
    T = _tiles(kept, ENV_ROWS, gpu)
    half = th.randn(K // 2, 2 * H, generator=gen) * 0.1
    M = th.cat([half, half, half * 0.5, half * 0.5], 0)                            # per table: rows k and k + 6 equal
    W2t, Wc = th.randn(H, H, generator=gen) / H ** 0.5, th.randn(K, H, generator=gen) * 0.1
    for name, enc_k in operands(ENV_KEPT, K, gen).items():
        coef_k = 1.0 / th.randint(1, 8, (ENV_KEPT,), generator=gen).float()
        if name == "tiny":
            # the kernel's operand row is [enc | coef enc] (the coefficient scales the row, not a panel): with a coefficient below 1 the
            # elements the split sees lie BELOW 2^-118, where more than 2^-16 of them is lost (measured with 1/1 .. 1/7: 1.68e-5)
            coef_k = th.ones(ENV_KEPT)
        h1, zn = launch(ENV_ROWS, keep, T, enc_k, coef_k, M, W2t, Wc, 0)
        r1, s1 = tables(ENV_ROWS, keep, enc_k, coef_k, M), tables(ENV_ROWS, keep, enc_k, coef_k, M, absolute=True)
        rec.envelope(name, "H1e", h1.cpu()[keep], r1, s1, stage_bound(2 * K), None, keep, h1)
        if name != "cancel":                                                       # (a chain: not a single product)
            ed = enc_k.double()
            rec.envelope(name, "zn", zn.cpu()[keep], r1 @ W2t.double() + ed @ Wc.double(), s1 @ W2t.double().abs() + ed.abs() @ Wc.double().abs(),
                         stage_bound(2 * K, H + K), None, keep, zn)
    return rec


# ---------------------------------------------------------------------------------------------------- csrc/dmp_lrppool.hip
def lrp_pool(gpu):
    """The LRP pooling product ``out[p] = sum_s row(slot[p, s]) W_s`` and its three gradients (widths 128 / 128)"""
    import util_fp64_lrp as UL
    from dualmessagepassing_amd import lrp
    rec = _Rec()
    rng = np.random.default_rng(131)

    def product(perm, x, z, w, dout):
        x, z, w = (t.to(gpu).requires_grad_(True) for t in (x, z, w))
        assert lrp.USE_POOL_KERNEL and lrp._pool_kernel_ok(perm, x, z, w)
        before = lrp._PermProduct.calls
        out = lrp.perm_product(perm, x, z, w)
        assert lrp._PermProduct.calls == before + 1
        out.backward(dout.to(gpu))
        return out.detach().cpu(), x.grad.cpu(), z.grad.cpu(), w.grad.cpu()

    # the sparse ladder: 96 node and 32 edge rows, row t a ladder value in column t; permutation (t, s) holds row t in slot s alone
    L, N, E = 2, 96, 32
    L2, R = L * L, 128
    slot = th.full((R * L2, L2), N + E, dtype=th.int64)
    t_of = th.arange(R * L2) // L2
    slot[th.arange(R * L2), th.arange(R * L2) % L2] = t_of
    perm = lrp.PermIndex(slot.view(-1).to(gpu), th.zeros(N, dtype=th.int64, device=gpu), th.zeros(N, device=gpu), N, E, L)
    rows = ladder_rows(R, H, rng)
    w = ladder_dense((H, H, L2), rng)
    dout = ladder_dense((R * L2, H), rng)
    got = product(perm, rows[:N], rows[N:], w, dout)
    ref = UL.perm_product_fp64(slot.view(-1), N, E, L, rows[:N], rows[N:], w, dout)
    rec.ladder("ladder", "out", got[0], ref[0])
    rec.ladder("ladder", "d weight", got[3], ref[3])
    # the rows' gradient W_s dout[p]: an upstream row with one ladder value (column t), for the permutations of one slot at a time
    worst, ok = 0.0, True
    for s in range(L2):
        d = th.zeros(R * L2, H)
        mine = th.arange(R * L2)[th.arange(R * L2) % L2 == s]
        d[mine, t_of[mine] % H] = th.from_numpy(ladder((R,), rng)[0])
        got = product(perm, rows[:N], rows[N:], w, d)
        ref = UL.perm_product_fp64(slot.view(-1), N, E, L, rows[:N], rows[N:], w, d)
        for a, b in ((got[1], ref[1]), (got[2], ref[2])):
            err, good = rel_elem(a, b)
            worst, ok = max(worst, err), ok and good
    rec.setdefault("ladder", {})["d rows"] = dict(kind="ladder", err=worst, ok=bool(ok))
    # adversarial: 33 permutations at L 4 (one above a tile of 32)
    name = "P33-w128"
    case = UL.cases()[name]
    perm = lrp.PermIndex.from_graphs(case["graphs"], gpu, case["L"])
    N, E, P, L = perm.num_nodes, perm.num_edges, perm.num_perms, case["L"]
    gen = th.Generator().manual_seed(132)
    _, _, w, _, dout, _ = UL.inputs(name, N, E, P, L, H, H)
    cnt = th.bincount(perm.slot.cpu()[perm.slot.cpu() < N + E], minlength=N + E)
    bounds = (stage_bound(H * L * L), stage_bound(H * int(cnt.max())), stage_bound(H * int(cnt.max())), stage_bound(P))
    for scen, rows in operands(N + E, H, gen).items():
        if scen == "cancel":
            continue                                                               # (sums over slots and permutations: nothing cancels)
        got = product(perm, rows[:N], rows[N:], w, dout)
        ref = UL.perm_product_fp64(perm.slot, N, E, L, rows[:N], rows[N:], w, dout)
        scale = UL.perm_product_fp64(perm.slot, N, E, L, rows[:N].abs(), rows[N:].abs(), w.abs(), dout.abs())
        for what, a, b, s, bound in zip(("out", "d node rows", "d edge rows", "d weight"), got, ref, scale, bounds):
            rec.envelope(scen, what, a, b, s, bound)
    return rec




KERNELS = {
    "bwd_h1_w": lambda gpu: bwd_h1_w(gpu, False),
    "bwd_h1_w_codes": lambda gpu: bwd_h1_w(gpu, True),
    "bwd_z_w": bwd_z_w,
    "atb2": atb2,
    "out_fwd_typed_codes": out_fwd_typed_codes,
    "edge_mlp_fwd": edge_mlp_fwd,
    "l0_edge_mlp": l0_edge_mlp,
    "node_chain": node_chain,
    "l0_node_fwd_mfma": l0_node_fwd_mfma,
    "l0_node_codes_bwd": l0_node_codes_bwd,
    "lrp_pool": lrp_pool,
}


def run_only(gpu, kernels=None):
    """{kernel: {scenario: {output: record}}} (module docstring)"""
    return {name: dict(KERNELS[name](gpu)) for name in (kernels or KERNELS)}
