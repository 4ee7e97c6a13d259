"""Shared by tests/test_gpu_bf16x6.py and scripts/bf16x6_probe.py: every bf16x6 kernel of the library that has an exact-fp32 form, on
adversarial operands and on the sparse "ladder", each run twice -- as shipped (three bf16 pieces per fp32 operand, six piece products on
v_mfma_f32_32x32x16_bf16) and under ``dmp_dev_set_exact_fp32(1)`` (the same kernel on the f32-input MFMA) -- and compared with fp64.
The ladder builders also serve tests/test_bf16x6_ladder_cpu.py (their proof, numpy only) and tests/bf16x6_only_cases.py."""
import numpy as np
import torch as th


def scenarios(rows, h, gen):
    """{name: [rows, h] fp32 operand}.  ``cancel``: columns k and k + h/2 hold x and -x (the weights below repeat with period
    h/2, so every exact product is 0); ``small`` / ``tiny``: values around 2^-100 / 2^-118 -- the third bf16 piece (2^-16 below the value)
    is still a normal bf16 number / lies under bf16's smallest subnormal (2^-133); ``element_binades`` / ``row_binades``: magnitudes from 2^-60 to 2^60 inside a row / row
    by row."""
    base = th.randn(rows, h, generator=gen)
    out = {"normal": base.clone()}
    out["element_binades"] = base * th.exp2(th.randint(-60, 61, (rows, h), generator=gen).float())
    out["row_binades"] = base * th.exp2(th.randint(-60, 61, (rows, 1), generator=gen).float())
    x = base[:, :h // 2]
    out["cancel"] = th.cat([x, -x], 1)
    out["small"] = base * 2.0 ** -100      # the third piece still a normal bf16 number: must be fp32-accurate
    out["tiny"] = base * 2.0 ** -118       # the third piece under bf16's range: two pieces left (2^-16)
    out["huge"] = base * 2.0 ** 100
    return out


LADDER_BOUND = 2.0 ** -21     # of |x y|: the three dropped piece products (2^-24 together), a few fp32 roundings of the accumulator, x 4


def ladder(shape, rng, exponents=None, signs=False):
    """fp32 values ``x = h + m + l`` whose round-to-nearest bf16 split is exactly ``(h, m, l)``: ``h`` = 129..159 / 128 (8 significant
    bits inside (1, 1.25): a negative ``m`` never crosses the binade), ``m`` = +-[1.5, 2) 2^-9 on the 2^-16 grid, ``l`` = +-(48..63) 2^-23
    = +-[1.5, 2) 2^-18, the two signs independent.  Every one of the six piece products of two such values is at least 4.5e-6 of the
    product (tests/test_bf16x6_ladder_cpu.py), so none of them can go missing inside ``LADDER_BOUND``.  ``exponents`` (int array or
    (lo, hi)) / ``signs``: a power-of-two factor and a sign per element, which leave the piece structure as it is.
    Returns ``(x, h, m, l)`` as numpy fp32 arrays."""
    sgn = lambda: rng.integers(0, 2, shape) * 2.0 - 1.0
    h = rng.integers(129, 160, shape) / 128.0
    m = sgn() * rng.integers(192, 256, shape) * 2.0 ** -16
    l = sgn() * rng.integers(48, 64, shape) * 2.0 ** -23
    f = np.ones(shape)
    if exponents is not None:
        e = rng.integers(exponents[0], exponents[1] + 1, shape) if isinstance(exponents, tuple) else np.asarray(exponents)
        f = np.exp2(e.astype(np.float64))
    if signs:
        f = f * sgn()
    h, m, l = h * f, m * f, l * f
    return (h + m + l).astype(np.float32), h.astype(np.float32), m.astype(np.float32), l.astype(np.float32)


def ladder_rows(rows, k, rng):
    """[rows, k] left operand of ``out = A W``: row r is zero except a ladder value in column ``r mod k`` -- with ``rows >= k`` every k
    position (every lane and slot of the piece layout, every row of a packed panel) meets a row, and each output element is ONE product."""
    assert rows >= k
    a = np.zeros((rows, k), np.float32)
    r = np.arange(rows)
    a[r, r % k] = ladder((rows,), rng)[0]
    return th.from_numpy(a)


def ladder_cols(rows, k, rng):
    """[rows, k] left operand of a product contracted over the ROWS (``A^T D``): one block of k rows, one of each tile slot 0 .. 31 in
    turn and spread over the tiles at random, holds a ladder value in column ``pi(row)`` (``pi``: a permutation of the block); every other
    row is zero, so each output element is ONE product whatever ``rows`` is."""
    assert rows >= k and k % 32 == 0
    a = np.zeros((rows, k), np.float32)
    tiles = rows // 32
    if tiles >= k // 32:
        sel = np.concatenate([rng.choice(tiles, k // 32, replace=False) * 32 + s for s in range(32)])
    else:
        sel = rng.choice(rows, k, replace=False)
    a[sel, rng.permutation(k)] = ladder((k,), rng)[0]
    return th.from_numpy(a)


def ladder_dense(shape, rng):
    return th.from_numpy(ladder(shape, rng)[0])


def rel_elem(got, ref64):
    """``(largest |got - ref| / |ref| over ref != 0, whether every element with ref == 0 is exactly 0 and all are finite)``"""
    got = got.double().cpu()
    ref64 = ref64.cpu()
    nz = ref64 != 0
    ok = bool(th.isfinite(got).all()) and bool((got[~nz] == 0).all())
    if not bool(nz.any()):
        return 0.0, ok
    return float(((got - ref64).abs()[nz] / ref64.abs()[nz]).max()), ok


def _rel(got, ref64, scale64):
    """largest |got - ref| / scale over the elements with a non-zero scale"""
    ok = scale64 > 0
    if not bool(ok.any()):
        return 0.0
    return float(((got.double() - ref64).abs()[ok] / scale64[ok]).max())


def _both(lib, fn):
    """fn() as shipped (bf16x6) and under the exact-fp32 switch."""
    assert not lib.dmp_dev_get_exact_fp32()
    x6 = fn()
    lib.dmp_dev_set_exact_fp32(1)
    try:
        ex = fn()
    finally:
        lib.dmp_dev_set_exact_fp32(0)
    return x6, ex


KERNELS = ("edge_fwd_typed", "bwd_z_typed", "atb_typed", "out_fwd", "bwd_h1", "out_fwd_typed", "bwd_h1_typed", "atb_plain", "atb_plain_tiles", "atb_tile_jobs", "typed_jobs")
ROWS = {128: 4099, 64: 1031}          # the last tile partial


def _products(fused, gpu, z, zt, d, wes, ix, coef, ce, n, h):
    """``(name, launch, fp64 result, natural scale)`` of every kernel that has an exact form, each in its identity configuration (zero
    bias, no ``prev``, slope 1.0 or a positive ``h1``, gate 1, all rows in ``identity_tiles``) so that the output IS the product.
    ``z`` [rows, h]: the streamed operand of the products ``z W``; ``zt`` / ``d`` [rows, h]: the operands of ``zt^T d``; ``wes`` [h, 2h] =
    ``[A | B]``."""
    rows = z.size(0)
    zd, ztd, dd, wd = z.double(), zt.double(), d.double(), wes.double()
    tiles = fused.identity_tiles(rows, gpu)
    zeros_p = th.zeros(n, 3 * h, device=gpu)
    ones = th.ones(rows, device=gpu)
    pos = th.ones(rows, h, device=gpu)
    # --- edge_fwd_typed: act(z (A + c B) + P[a] - P[b] + bias) with P = 0, bias = 0, slope 1 (identity)
    ref = zd @ wd[:, :h] + ce[:, None] * (zd @ wd[:, h:])
    scale = zd.abs() @ wd[:, :h].abs() + ce[:, None] * (zd.abs() @ wd[:, h:].abs())
    yield "edge_fwd_typed", (lambda: fused.edge_fwd_typed(z, wes, zeros_p[:, h:], 3 * h, None, coef, ix, slope=1.0)), ref, scale
    # --- bwd_z_typed: dPre (A + c B)^T  (no base, dS = 0).  The operand's structure ("cancel", the ladder's one column per row) must
    # sit on the contraction index: columns of dPre against rows of A^T -> (A^T | B^T) as a Wes
    ds0 = th.zeros(n, 2 * h, device=gpu)
    wes2 = th.cat([wes[:, :h].t().contiguous(), wes[:, h:].t().contiguous()], 1)
    w2d = wes2.double()
    ref2 = zd @ w2d[:, :h].t() + ce[:, None] * (zd @ w2d[:, h:].t())
    scale2 = zd.abs() @ w2d[:, :h].t().abs() + ce[:, None] * (zd.abs() @ w2d[:, h:].t().abs())
    yield "bwd_z_typed", (lambda: fused.bwd_z_typed(z, h, wes2, ds0, None, coef, ix)), ref2, scale2
    # --- atb_typed: [zt^T d | zt^T (c d)] (the contraction runs over the rows)
    ref3 = th.cat([ztd.t() @ dd, ztd.t() @ (dd * ce[:, None])], 1)
    scale3 = th.cat([ztd.abs().t() @ dd.abs(), ztd.abs().t() @ (dd.abs() * ce[:, None])], 1)
    yield "atb_typed", (lambda: fused.atb_typed(zt, d, coef, ix)), ref3, scale3
    # --- out_fwd: prev + gate (z W2^T + b2) with prev = 0, b2 = 0, gate = 1: z W2^T
    w2 = wes[:, :h].t().contiguous()                              # nn.Linear weight [out, in]: W2[j][k] = A[k][j]
    ref4, scale4 = zd @ wd[:, :h], zd.abs() @ wd[:, :h].abs()
    yield "out_fwd", (lambda: fused.out_fwd_mfma(z, w2, None, ones, None)), ref4, scale4
    # --- bwd_h1: act'(H1) (gate z) W2 with H1 > 0 everywhere, gate = 1: z W2, W2 = A^T's storage
    w2b = wes[:, :h].contiguous()                                 # dH1 = dO @ W2 with W2 [out = k, in = j] = A[k][j]
    yield "bwd_h1", (lambda: fused.bwd_h1_mfma(z, w2b, pos, both_halves=False, gate=ones, slope=0.0)[0]), ref4, scale4
    # --- the tile-list kernels of csrc/dmp_typed.hip over every row: z A through the [in, out] and the [out, in] weight reads
    yield "out_fwd_typed", (lambda: fused.out_fwd_typed(z, w2b, None, None, tiles)), ref4, scale4
    yield "bwd_h1_typed", (lambda: fused.bwd_h1_typed(z, w2b, pos, tiles, slope=0.0)[0]), ref4, scale4
    # --- zt^T d alone (H = 128: the bf16-piece LDS image of csrc/dmp_h1w.hip as shipped, csrc/dmp_atb.hip under the switch)
    yield "atb_plain", (lambda: fused.atb_typed(zt, d, coef, ix, plain=True)), ztd.t() @ dd, ztd.abs().t() @ dd.abs()

    def without_atb2(fn):
        """csrc/dmp_atb.hip's own bf16x6 tile-list kernels (at H = 128 the launches prefer csrc/dmp_h1w.hip's ``atb2``)"""
        def run():
            fused.USE_ATB2 = False
            try:
                return fn()
            finally:
                fused.USE_ATB2 = True
        return run

    yield "atb_plain_tiles", without_atb2(lambda: fused.atb_typed(zt, d, coef, ix, plain=True)), ztd.t() @ dd, ztd.abs().t() @ dd.abs()
    yield ("atb_tile_jobs", without_atb2(lambda: fused.atb_rows_multi([(zt, d, None, False)], tiles=tiles)[0][0]), ztd.t() @ dd,
           ztd.abs().t() @ dd.abs())

    def two_jobs():
        out = th.empty(rows, 2 * h, device=gpu)
        fused.typed_jobs([dict(a=z, W=w2b, out=out[:, :h]), dict(a=z, W=w2, w_in_out=False, out=out[:, h:])], tiles)
        return out

    yield "typed_jobs", two_jobs, th.cat([ref4, ref4], 1), th.cat([scale4, scale4], 1)


def run_all(gpu, rows=None, h=128):
    """{scenario: {kernel: (bf16x6 error, exact-fp32 error, finite)}}: of the natural scale for ``scenarios``; for ``"ladder"`` the
    largest ELEMENTWISE relative error of either form on the sparse ladder (each output element one product of two ladder values) and
    whether every result is finite."""
    from dualmessagepassing_amd import _lib, fused
    from dualmessagepassing_amd.graph import GraphIndex
    lib = _lib.load()
    rows = ROWS[h] if rows is None else rows
    gen = th.Generator().manual_seed(20260410)
    rng = np.random.default_rng(5)
    n = max(2, rows // 6)
    src, dst = rng.integers(0, n, rows).astype(np.int64), rng.integers(0, n, rows).astype(np.int64)
    ix = GraphIndex(th.from_numpy(src).to(gpu), th.from_numpy(dst).to(gpu), n, th.from_numpy(rng.random(rows) < 0.5).to(gpu))
    coef = ix.degree_coef(ix.out_deg)
    ce = ix.edge_select(coef)[2].double()                         # coef[dst e]
    half = (th.randn(h // 2, 2 * h, generator=gen) * 0.1)
    wes = th.cat([half, half], 0).to(gpu)                          # rows k and k + h/2 equal: "cancel" has exact result 0
    res = {}
    for name, z_cpu in scenarios(rows, h, gen).items():
        z = z_cpu.to(gpu)
        d = th.randn(rows, h, generator=gen).to(gpu)               # of unit scale
        r = {}
        for kernel, fn, ref, scale in _products(fused, gpu, z, z, d, wes, ix, coef, ce, n, h):
            x6, ex = _both(lib, fn)
            r[kernel] = (_rel(x6, ref, scale), _rel(ex, ref, scale), bool(th.isfinite(x6).all()))
        res[name] = r
    # the sparse ladder: the panel is the ladder matrix itself (a zero B half: A + c B = A in fp32)
    lrng = np.random.default_rng(20260411)
    z = ladder_rows(rows, h, lrng).to(gpu)
    zt = ladder_cols(rows, h, lrng).to(gpu)
    d = ladder_dense((rows, h), lrng).to(gpu)
    lw = th.cat([ladder_dense((h, h), lrng), th.zeros(h, h)], 1).to(gpu)
    r = {}
    for kernel, fn, ref, _ in _products(fused, gpu, z, zt, d, lw, ix, coef, ce, n, h):
        x6, ex = _both(lib, fn)
        (e6, ok6), (e32, ok32) = rel_elem(x6, ref), rel_elem(ex, ref)
        r[kernel] = (e6, e32, ok6 and ok32)
    res["ladder"] = r
    return res


