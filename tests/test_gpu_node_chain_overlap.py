"""The kept-node product chain (csrc/dmp_nodechain.hip) where its pipeline can go wrong: the panel chunks stream through two LDS
buffers per workgroup, several workgroups share a CU, and a workgroup that walks more than one pass carries the stream from a
pass's last chunk to the next pass's first.

Shapes come from the kernel's own sizing: ``T`` tiles per pass and the block cap ``G`` are read off ``dmp_node_chain_blocks``.
* short lists: 1, 33, 65 and 129 kept rows -- one tile with 31 padding slots; a pass boundary inside the list for 2-tile and for
  4-tile passes, the last pass partly padding or past the list's end;
* ``2 T G + 1`` tiles, the last one 5 rows short: some workgroup runs three passes, the last a short one.

Rules of tests/test_gpu_node_chain.py: fp64 on the CPU as the reference; every output within ``1e-5 * max(1, |ref|max)`` or twice the
three-launch chain's own error where that is larger; column sums within ``2e-6`` of the column's sum of magnitudes; NaN in every dead
input row; sentinel-filled outputs whose dead rows stay bit for bit.  Each case's reference is computed once."""
import pytest
import torch as th

pytestmark = pytest.mark.gpu
H = 128
SLOPE = 1.0 / 5.5
SENT = 7.5
SHORT = (1, 33, 65, 129)
_CASES = {}
_SIZING = []


def _sizing():
    """(tiles per pass, block cap) of the kernel, from ``dmp_node_chain_blocks``: ``min(cap, ceil(tiles / T))`` workgroups."""
    if not _SIZING:
        from dualmessagepassing_amd import _lib
        blocks = _lib.load().dmp_node_chain_blocks
        T = 1
        while int(blocks(T + 1)) == 1:
            T += 1
        G = int(blocks(1 << 40))
        assert int(blocks(T * G)) == G and int(blocks(T * (G - 1))) == G - 1
        _SIZING.append((T, G))
    return _SIZING[0]


def _multi_pass_rows():
    T, G = _sizing()
    return (2 * T * G + 1) * 32 - 5


def _tiles(kept, N, gpu):
    """``(slot, tile_scale, num_tiles, bound)`` as ``NodeRows.tiles``: 32 slots per tile, -1 = padding, the tile count on the device."""
    bound = (N + 31) // 32
    slot = th.full((bound * 32,), -1, dtype=th.int32)
    slot[:kept.numel()] = kept.to(th.int32)
    nt = (kept.numel() + 31) // 32
    return slot.to(gpu), th.zeros(bound, device=gpu), th.tensor([nt], dtype=th.int32, device=gpu), bound


def _case(nkept, gpu):
    """Inputs on the device (column blocks of wider buffers, NaN in every dead row), weights, tiles and the fp64 results: made once."""
    if nkept in _CASES:
        return _CASES[nkept]
    T, G = _sizing()
    N = 160 if nkept <= 129 else nkept + 4000 + 37          # (the long list: the bound still reaches the block cap)
    g = th.Generator().manual_seed(1000 + nkept)
    kept = th.randperm(N, generator=g)[:nkept].sort().values
    keep = th.zeros(N, dtype=th.bool)
    keep[kept] = True
    r = lambda *s: th.randn(*s, generator=g)
    c = dict(N=N, kept=kept, keep=keep)
    Wx, Bn, W2 = r(H, 3 * H) / (3 * H) ** 0.5, r(2 * H, H) / (3 * H) ** 0.5, r(H, H) / H ** 0.5
    bn, b2 = r(H), r(H)
    wide = dict(x=r(N, H + 8), S=r(N, 3 * H), dxn=r(N, H + 4), dP=r(N, 3 * H), H1=r(N, H))
    for v in wide.values():
        v[~keep] = float("nan")
    x, S, dxn, dP, H1 = wide["x"][:, 4:4 + H], wide["S"][:, H:], wide["dxn"][:, :H], wide["dP"][:, H:], wide["H1"]
    d = lambda t: t.double()
    k = keep
    dWx, dBn, dW2 = d(Wx), d(Bn), d(W2)
    h1 = th.nn.functional.leaky_relu(d(x[k]) @ dWx[:, :H] + d(S[k]) @ dBn + d(bn), SLOPE)
    c["ref_f"] = dict(H1n=h1, P=d(x[k]) @ dWx[:, H:], xn=d(x[k]) + h1 @ dW2.t() + d(b2), x=d(x[k]))
    dh = d(dxn[k]) @ dW2
    dpn = th.where(d(H1[k]) > 0, dh, SLOPE * dh)
    c["ref_b"] = dict(dPn=dpn, dS=th.cat([dpn @ dBn[:H].t(), dpn @ dBn[H:].t()], 1),
                      dx=d(dxn[k]) + dpn @ dWx[:, :H].t() + d(dP[k]) @ dWx[:, H:].t(), dxn=d(dxn[k]),
                      dbn=dpn.sum(0), db2n=d(dxn[k]).sum(0),
                      dbn_scale=(d(dxn[k]).abs() @ dW2.abs()).sum(0), db2n_scale=d(dxn[k]).abs().sum(0))
    w = {n: v.to(gpu) for n, v in wide.items()}
    c["dev"] = dict(x=w["x"][:, 4:4 + H], S=w["S"][:, H:], dxn=w["dxn"][:, :H], dP=w["dP"][:, H:], H1=w["H1"],
                    Wx=Wx.to(gpu), Bn=Bn.to(gpu), W2=W2.to(gpu), bn=bn.to(gpu), b2=b2.to(gpu))
    c["tiles"] = _tiles(kept, N, gpu)
    assert c["tiles"][3] >= min(T * G, (nkept + 31) // 32)
    _CASES[nkept] = c
    return c


def _check(name, what, got, old, ref, keep):
    """Kept rows against fp64 (the one launch; the three-launch chain where it ran), dead rows bit for bit the sentinel."""
    bound = 1e-5 * max(1.0, float(ref.abs().max()))
    e_new = float((got.cpu()[keep].double() - ref).abs().max())
    e_old = float((old.cpu()[keep].double() - ref).abs().max()) if old is not None else 0.0
    print("%s %s: chain %.3e  three launches %.3e  bound %.3e" % (name, what, e_new, e_old, bound))
    assert bool(th.isfinite(got.cpu()[keep]).all()), what
    assert e_new <= max(bound, 2.0 * e_old), (what, e_new, e_old, bound)
    assert bool((got.cpu()[~keep] == SENT).all()), what + ": a dead row was written"


def _sent(N, w, gpu):
    return th.full((N, w), SENT, device=gpu)


def _forward(c, gpu, residual=True):
    from dualmessagepassing_amd import fused
    v, N = c["dev"], c["N"]
    pf, _ = fused.node_chain_panels(v["Bn"], v["Wx"], v["W2"])
    H1n, XP, xn = _sent(N, H, gpu), _sent(N, 3 * H, gpu), _sent(N, H, gpu)
    fused.node_chain_fwd(v["x"], v["S"], pf, v["bn"], v["b2"], residual, SLOPE, c["tiles"], H1n, XP[:, H:], xn)      # (P: a column block)
    return H1n, XP, xn


def _forward_three(c, gpu):
    from dualmessagepassing_amd import fused
    v, N, T = c["dev"], c["N"], c["tiles"]
    x, S, Wx, Bn = v["x"], v["S"], v["Wx"], v["Bn"]
    oH1, oXP, oxn, T1 = _sent(N, H, gpu), _sent(N, 3 * H, gpu), _sent(N, H, gpu), _sent(N, H, gpu)
    fused.typed_jobs([dict(a=x, W=Wx[:, :H], bias=v["bn"], out=oXP[:, :H]), dict(a=S[:, :H], W=Bn[:H], out=T1),
                      dict(a=x, W=Wx[:, H:2 * H], out=oXP[:, H:2 * H]), dict(a=x, W=Wx[:, 2 * H:], out=oXP[:, 2 * H:])], T)
    fused.out_fwd_typed(S[:, H:], Bn[H:], None, oXP[:, :H], T, out=oH1, slope=SLOPE, prev2=T1)
    fused.out_fwd_typed(oH1, v["W2"], v["b2"], x, T, out=oxn, w_in_out=False)
    return oH1, oXP, oxn


def _backward(c, gpu, with_dx=True, residual=True, partials=None):
    """-> dXP ([dPn | dP]), dS in a wider buffer, dx, the two reduced column sums; ``partials``: a list that takes the partial rows."""
    from dualmessagepassing_amd import fused
    v, N = c["dev"], c["N"]
    _, pb = fused.node_chain_panels(v["Bn"], v["Wx"], v["W2"])
    dXP = _sent(N, 3 * H, gpu)
    dXP[:, H:] = v["dP"]                                                                   # (the kept-incidence sums wrote it)
    dSw, dx = _sent(N, 2 * H + 4, gpu), _sent(N, H, gpu)
    real = fused.reduce_partials
    if partials is not None:
        fused.reduce_partials = lambda part, *a, **k: (partials.append(part), real(part, *a, **k))[1]
    try:
        with fused.deferred_reductions():
            dbn, db2n = fused.node_chain_bwd(v["dxn"], v["H1"], dXP[:, H:], pb, residual, SLOPE, c["tiles"], dXP[:, :H], dSw[:, :2 * H],
                                             dx if with_dx else None)
    finally:
        fused.reduce_partials = real
    return dXP, dSw, dx, dbn, db2n


def _backward_three(c, gpu):
    from dualmessagepassing_amd import fused
    v, N, T = c["dev"], c["N"], c["tiles"]
    dxn, Wx, Bn = v["dxn"], v["Wx"], v["Bn"]
    oXP = _sent(N, 3 * H, gpu)
    oXP[:, H:] = v["dP"]
    oS, oU, odx = _sent(N, 2 * H, gpu), _sent(N, 2 * H, gpu), _sent(N, H, gpu)
    fused.bwd_h1_typed(dxn, v["W2"], v["H1"], T, SLOPE, out=oXP[:, :H])
    fused.typed_jobs([dict(a=oXP[:, :H], W=Bn[:H], w_in_out=False, out=oS[:, :H]), dict(a=oXP[:, :H], W=Bn[H:], w_in_out=False, out=oS[:, H:]),
                      dict(a=oXP[:, :H], W=Wx[:, :H], w_in_out=False, prev=dxn, out=oU[:, :H]),
                      dict(a=oXP[:, H:2 * H], W=Wx[:, H:2 * H], w_in_out=False, out=oU[:, H:])], T)
    fused.out_fwd_typed(oXP[:, 2 * H:], Wx[:, 2 * H:], None, oU[:, :H], T, out=odx, w_in_out=False, prev2=oU[:, H:])
    return oXP, oS, odx


def _same(a, b):
    return th.equal(a.contiguous().view(th.int32), b.contiguous().view(th.int32))           # bit for bit (dead rows of dP hold NaN)


def _check_forward(name, c, gpu, residual):
    keep, ref = c["keep"], c["ref_f"]
    H1n, XP, xn = _forward(c, gpu, residual)
    oH1, oXP, oxn = _forward_three(c, gpu) if residual else (None, None, None)
    _check(name, "H1n", H1n, oH1, ref["H1n"], keep)
    _check(name, "P", XP[:, H:], oXP[:, H:] if residual else None, ref["P"], keep)
    _check(name, "xn", xn, oxn, ref["xn"] if residual else ref["xn"] - ref["x"], keep)
    assert bool((XP[:, :H] == SENT).all()), "the block beside P was written"


def _check_backward(name, c, gpu, with_dx, residual):
    keep, ref, v = c["keep"], c["ref_b"], c["dev"]
    dXP, dSw, dx, dbn, db2n = _backward(c, gpu, with_dx, residual)
    oXP, oS, odx = _backward_three(c, gpu) if residual else (None, None, None)
    _check(name, "dPn", dXP[:, :H], oXP[:, :H] if residual else None, ref["dPn"], keep)
    _check(name, "dS", dSw[:, :2 * H], oS, ref["dS"], keep)
    if with_dx:
        _check(name, "dx", dx, odx, ref["dx"] if residual else ref["dx"] - ref["dxn"], keep)
    else:
        assert bool((dx == SENT).all()), "dx was written although it was not asked for"
    assert bool((dSw[:, 2 * H:] == SENT).all()), "the columns beside dS were written"
    assert _same(dXP[:, H:], v["dP"]), "dP was written"
    for what, got, want, scale in (("dbn", dbn, ref["dbn"], ref["dbn_scale"]), ("db2n", db2n, ref["db2n"], ref["db2n_scale"])):
        err, tol = float((got.cpu().double() - want).abs().max()), 2e-6 * max(1.0, float(scale.max()))
        print("%s %s: chain %.3e  bound %.3e" % (name, what, err, tol))
        assert err <= tol, (what, err, tol)


@pytest.mark.parametrize("nkept", SHORT)
def test_short_tile_lists(nkept, gpu):
    c = _case(nkept, gpu)
    name = "kept%d" % nkept
    _check_forward(name, c, gpu, True)
    _check_backward(name, c, gpu, True, True)
    _check_backward(name, c, gpu, False, True)


@pytest.mark.parametrize("residual", [True, False], ids=["residual", "no_residual"])
@pytest.mark.parametrize("which", ["forward", "backward_dx", "backward_no_dx"])
def test_a_workgroup_of_three_passes(which, residual, gpu):
    T, G = _sizing()
    c = _case(_multi_pass_rows(), gpu)
    tiles = (c["kept"].numel() + 31) // 32
    assert tiles == 2 * T * G + 1 and -(-tiles // G) > 2 * T and c["kept"].numel() % 32 == 27
    if which == "forward":
        _check_forward("three_passes", c, gpu, residual)
    else:
        _check_backward("three_passes", c, gpu, which == "backward_dx", residual)


def test_ten_launches_give_the_same_bits(gpu):
    """Every output and both partial arrays of ten launches on the same inputs, bit for bit those of the first: a chunk buffer
    written before its readers were through shows as differing bits."""
    c = _case(_multi_pass_rows(), gpu)
    first = None
    for i in range(10):
        parts = []
        got = list(_forward(c, gpu)) + list(_backward(c, gpu, partials=parts))
        assert len(parts) == 2
        got += parts
        parts_nodx = []
        nodx = _backward(c, gpu, with_dx=False, partials=parts_nodx)
        got += [nodx[0], nodx[1], nodx[3], nodx[4]] + parts_nodx
        if first is None:
            first = got
            continue
        for j, (a, b) in enumerate(zip(got, first)):
            assert _same(a, b), "launch %d: output %d differs from the first launch's" % (i, j)


def test_empty_tile_list(gpu):
    """No tiles: nothing is written, the partial rows are zero."""
    c = _case(129, gpu)
    N = c["N"]
    empty = dict(c, tiles=_tiles(th.zeros(0, dtype=th.long), N, gpu))
    for t in _forward(empty, gpu):
        assert bool((t == SENT).all())
    for with_dx in (True, False):
        parts = []
        dXP, dSw, dx, dbn, db2n = _backward(empty, gpu, with_dx=with_dx, partials=parts)
        assert bool((dXP[:, :H] == SENT).all()) and bool((dSw == SENT).all()) and bool((dx == SENT).all())
        assert _same(dXP[:, H:], c["dev"]["dP"])
        assert len(parts) == 2 and all(bool((p == 0).all()) for p in parts)
        assert bool((dbn == 0).all()) and bool((db2n == 0).all())
