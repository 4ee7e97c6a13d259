"""The first layer's node side from the label codes on the matrix pipe (csrc/dmp_l0node.hip, ``fused.l0_node_fwd_mfma``):

    H1n[r]             = act([venc | S0_in | S0_out][r] W_t[:, :H] + bn)
    [P_dst | P_src][r] = [venc | S0_in | S0_out][r] W_t[:, H:3H]            t = 0 below the node split, 1 from it on

for the kept node rows in one launch, and the backward's contraction over the same rows (``fused.l0_node_codes_bwd``)

    Xn[h, table rows] = S0_h^T dPn            Yn[b, table rows] = venc^T [dPn | dP_dst | dP_src (| dxn)]

-- against an fp64 restatement and against the launches they replace (``fused.l0_node_fwd`` per table; ``smallk_atb_cols``) on the
same inputs, the dead rows' contract (nothing read, ``H1n`` untouched, ``P`` zeros, zero partials from a workgroup without tiles), the
packed codes of ``dmp_l0_pack`` bit for bit, the route in bench.py's model with the switch on against off, and the replayed step.

Bounds: ``1e-5 max(1, |ref|max)`` per element of a row output, 2e-4 of the largest entry for a summed product (the layer tests'
bounds); the switch in the model: outputs to 2e-5 and parameter gradients to 5e-5 of their largest entry (tests/test_gpu_node_rows.py).
Observed worst cases (MI355X): rows 1.1e-4 against a bound of 8.9e-3 (code sums of 257); summed products 8.9e-6 of a largest entry
of 92 (1e-7)."""
import os
import sys

import pytest
import torch as th

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 128
CODES = [(1, 1), (6, 10), (16, 12), (6, 16), (16, 10), (1, 16)]       # (VK, K0): VK + 2 K0 <= 40, K0 a multiple of 4 and not
KINDS = ["nolist", "all", "none", "ragged", "short", "prefix_at", "prefix_below"]


def _inputs(n, tables, vk, k0, kind, big, gpu, seed):
    """Codes, sums, packed matrices and the kept rows of one case.  ``kind``: how the kept rows are given (``nolist``: no gate at
    all; ``short``: a list of more capacity than rows, its tail pointing at a dead row; ``prefix_*``: the leading rows all kept,
    the prefix handed over AT the split / BELOW it).  ``big``: code sums of that magnitude in some entries (256: one bf16 piece,
    257: two).  Rows outside the kept list and the padding columns hold NaN: none of it may be read."""
    from dualmessagepassing_amd import fused
    gen = th.Generator().manual_seed(seed)
    kp, kvp = (k0 + 3) // 4 * 4 + 4, (vk + 3) // 4 * 4            # Kp padded beyond K0's own rounding
    split = 0 if tables == 1 else min(n - 1, 37)                  # (no multiple of 32)
    first = split if kind == "prefix_at" else (max(split - 5, 0) if kind == "prefix_below" else 0)
    if kind in ("nolist", "all"):
        keep = th.ones(n, dtype=th.bool)
    elif kind == "none":
        keep = th.zeros(n, dtype=th.bool)
    else:
        keep = th.rand(n, generator=gen) < 0.4
        keep[:first] = True
        keep[n - 1] = kind != "short"                             # ("short": the last row is dead, the list's tail points at it)
    venc = (th.rand(n, kvp, generator=gen) < 0.4).float()
    S0 = th.randint(-3, 6, (n, 2 * kp), generator=gen).float()
    if big:
        S0[::3, 0] = float(big)
        S0[1::5, kp + k0 - 1] = -float(big)
    venc[:, vk:] = float("nan")
    S0[:, k0:kp] = float("nan")
    S0[:, kp + k0:] = float("nan")
    venc[~keep] = float("nan")
    S0[~keep] = float("nan")
    W = th.stack([fused.l0_node_pack(vk, k0, H, th.randn(vk, 3 * H, generator=gen), th.randn(k0, H, generator=gen),
                                     th.randn(k0, H, generator=gen)) for _ in range(tables)])
    bias = th.randn(H, generator=gen)
    c = dict(n=n, tables=tables, vk=vk, k0=k0, kp=kp, split=split if tables == 2 else n, first=first, kind=kind, keep=keep.to(gpu),
             venc=venc.to(gpu), S0=S0.to(gpu), W=W.to(gpu), bias=bias.to(gpu), mask=None, rows=None)
    if kind != "nolist":
        c["mask"] = fused.gate_row_mask(c["keep"].float())
        ids = th.nonzero(keep).view(-1).int()
        if kind == "short":
            lst = th.full((n + 64,), n - 1, dtype=th.int32)       # capacity beyond the rows; the tail names the (dead) last row
            lst[:ids.numel()] = ids
            c["rows"] = (lst.to(gpu), th.tensor([ids.numel()], dtype=th.int32, device=gpu))
        else:
            lst, cnt = fused.kept_rows(c["mask"], 0, n, tiles=True)
            assert int(cnt[0]) == ids.numel()
            c["rows"] = (lst, cnt[0:1])
    return c


def _fp64(c, slope):
    n, vk, k0, kp = c["n"], c["vk"], c["k0"], c["kp"]
    keep = c["keep"]
    x = th.cat([c["venc"][:, :vk], c["S0"][:, :k0], c["S0"][:, kp:kp + k0]], 1).double()
    x = th.where(keep.view(-1, 1), x, th.zeros_like(x))
    out = th.zeros(n, 3 * H, dtype=th.float64, device=x.device)
    for t in range(c["tables"]):
        r0, r1 = (0, c["split"]) if t == 0 else (c["split"], n)
        out[r0:r1] = x[r0:r1] @ c["W"][t, :vk + 2 * k0].double()
    pre = out[:, :H] + c["bias"].double()
    return th.where(pre > 0, pre, slope * pre), out[:, H:]


def _new(c, slope, h1=None, P=None):
    from dualmessagepassing_amd import fused
    dev = c["venc"].device
    h1 = th.full((c["n"], H), -7.0, device=dev) if h1 is None else h1
    P = th.full((c["n"], 2 * H), -7.0, device=dev) if P is None else P
    fused.l0_node_fwd_mfma(c["venc"], c["vk"], c["S0"], c["k0"], c["kp"], c["W"], c["split"], c["bias"], slope, c["n"], H, h1, P,
                           mask=c["mask"], rows=c["rows"], prefix=c["first"])
    return h1, P


def _old(c, slope):
    from dualmessagepassing_amd import fused
    dev = c["venc"].device
    h1, P = th.full((c["n"], H), -7.0, device=dev), th.full((c["n"], 2 * H), -7.0, device=dev)
    for t in range(c["tables"]):
        n0, n1 = (0, c["split"]) if t == 0 else (c["split"], c["n"])
        if n1 > n0:
            fused.l0_node_fwd(c["venc"], c["vk"], c["S0"], c["k0"], c["kp"], c["W"][t], c["bias"], slope, c["mask"], n0, n1, H, h1, P,
                              rows=c["rows"], q_begin=min(c["first"], n0))
    return h1, P


def _check(c, slope, tag):
    keep = c["keep"]
    ref_h, ref_p = _fp64(c, slope)
    h1, P = _new(c, slope)
    oh, oP = _old(c, slope)
    assert bool((h1[~keep] == -7.0).all()), tag                        # a dead row's H1n: the sentinel survives
    assert bool((P[~keep] == 0).all()), tag                            # ... its projections: zeros
    assert bool(th.isfinite(h1).all()) and bool(th.isfinite(P).all()), tag      # no NaN of a dead row or a padding column was read
    worst = {}
    if bool(keep.any()):
        for name, got, old, ref in (("H1n", h1, oh, ref_h), ("P", P, oP, ref_p)):
            tol = 1e-5 * max(1.0, float(ref[keep].abs().max()))
            e64, eold = float((got.double() - ref)[keep].abs().max()), float((got - old)[keep].abs().max())
            worst[name] = (e64, eold, tol)
            assert e64 <= tol and eold <= tol, (tag, name, e64, eold, tol)
    assert th.equal(oh[~keep], h1[~keep]) and th.equal(oP[~keep], P[~keep]), tag
    h2, P2 = _new(c, slope)
    assert th.equal(h1, h2) and th.equal(P, P2), tag                   # repeatable
    return worst


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,tables", [(96, 1), (96, 2), (257, 1), (257, 2), (1000, 1), (1000, 2)])
def test_node_side_against_fp64_and_the_launches_per_table(n, tables, kind, gpu):
    worst = {}
    for i, (vk, k0) in enumerate(CODES):
        for slope in (0.0, 1 / 5.5):
            c = _inputs(n, tables, vk, k0, kind, 0, gpu, seed=1000 * n + 10 * i + tables)
            for name, v in _check(c, slope, (n, tables, kind, vk, k0, slope)).items():
                if name not in worst or v[0] / v[2] > worst[name][0] / worst[name][2]:
                    worst[name] = v
    for name, (e64, eold, tol) in worst.items():
        print("%s n=%d tables=%d %s: %.3e against fp64, %.3e against the launches per table, bound %.3e" % (name, n, tables, kind, e64, eold, tol))


@pytest.mark.parametrize("big", [256, 257])
@pytest.mark.parametrize("kind", ["nolist", "ragged"])
def test_code_sums_at_the_edge_of_one_bf16_piece(big, kind, gpu):
    """A code sum of magnitude 256 is one bf16 piece (mid and lo pieces zero), 257 needs two: the kernel runs all six piece products
    and holds the same bound on both sides."""
    for vk, k0 in ((6, 10), (16, 12)):
        for tables in (1, 2):
            c = _inputs(257, tables, vk, k0, kind, big, gpu, seed=big + vk + tables)
            assert float(c["S0"][c["keep"]][:, 0].abs().max()) == big
            for name, (e64, eold, tol) in _check(c, 1 / 5.5, (big, kind, vk, k0, tables)).items():
                print("%s sums of %d, %s, VK=%d K0=%d tables=%d: %.3e against fp64, %.3e against the launches per table, bound %.3e"
                      % (name, big, kind, vk, k0, tables, e64, eold, tol))


def test_more_tiles_than_workgroups_and_no_bias(gpu):
    """40,000 rows without a gate are 1,250 tiles over 512 workgroups (three tiles each, the last ones short); a gated launch over
    the same rows; no bias."""
    for n, kind in ((40000, "nolist"), (40000, "ragged"), (106496, "nolist"), (106496, "ragged")):
        c = _inputs(n, 2, 16, 10, kind, 0, gpu, seed=5)
        c["split"] = 8197
        _check(c, 1 / 5.5, kind)
        c["bias"] = None
        ref_h, _ = _fp64(dict(c, bias=th.zeros(H, device=gpu)), 0.0)
        h1, _ = _new(c, 0.0)
        keep = c["keep"]
        assert float((h1.double() - ref_h)[keep].abs().max()) <= 1e-5 * max(1.0, float(ref_h[keep].abs().max()))


def test_host_condition_and_unsupported_arguments(gpu):
    """What ``l0_node_mfma_ok`` turns away the C entry turns away as well (DMP_ERR_UNSUPPORTED raises), nothing is launched."""
    from dualmessagepassing_amd import _lib, fused
    c = _inputs(96, 1, 6, 10, "nolist", 0, gpu, seed=1)
    assert fused.l0_node_mfma_ok(H, 6, 10, c["kp"], 1, 96, c["venc"], c["S0"])
    lib = _lib.load()
    lib.dmp_dev_set_exact_fp32(1)
    try:
        assert not fused.l0_node_mfma_ok(H, 6, 10, c["kp"], 1, 96, c["venc"], c["S0"])
        with pytest.raises(Exception):
            _new(c, 0.0)
    finally:
        lib.dmp_dev_set_exact_fp32(0)
    odd = dict(c, venc=th.zeros(96, 9, device=gpu)[:, :8])           # a row stride of 36 bytes
    assert not fused.l0_node_mfma_ok(H, 6, 10, c["kp"], 1, 96, odd["venc"], c["S0"])
    with pytest.raises(Exception):
        _new(odd, 0.0)
    h1, P = _new(c, 0.0)
    assert bool(th.isfinite(h1).all())


# ----------------------------------------------------------------------------- the backward's contraction
def _bwd_new(c, dXP, dxn, vtables):
    from dualmessagepassing_amd import fused
    dev = dXP.device
    Xn = th.full((2, c["tables"] * c["k0"], H), float("nan"), device=dev)
    Yn = th.full((3 if dxn is None else 4, vtables * c["vk"], H), float("nan"), device=dev)
    fused.l0_node_codes_bwd(c["venc"], c["vk"], vtables, c["S0"], c["k0"], c["kp"], c["tables"], c["split"], dXP, dxn, c["n"], H, Xn, Yn,
                            rows=c["rows"], prefix=c["first"])
    return Xn, Yn


def _bwd_fp64(c, dXP, dxn, vtables):
    n, vk, k0, kp, keep = c["n"], c["vk"], c["k0"], c["kp"], c["keep"]
    z = lambda t: th.where(keep.view(-1, 1), t, th.zeros_like(t)).double()
    v, si, so = z(c["venc"][:, :vk]), z(c["S0"][:, :k0]), z(c["S0"][:, kp:kp + k0])
    blocks = [z(dXP[:, b * H:(b + 1) * H]) for b in range(3)] + ([] if dxn is None else [z(dxn)])
    X = th.zeros(2, c["tables"] * k0, H, dtype=th.float64, device=dXP.device)
    Y = th.zeros(len(blocks), vtables * vk, H, dtype=th.float64, device=dXP.device)
    for t in range(c["tables"]):
        r0, r1 = (0, c["split"]) if t == 0 else (c["split"], n)
        X[0, t * k0:(t + 1) * k0] = si[r0:r1].t() @ blocks[0][r0:r1]
        X[1, t * k0:(t + 1) * k0] = so[r0:r1].t() @ blocks[0][r0:r1]
        tv = t if vtables == 2 else 0
        for b, d in enumerate(blocks):
            Y[b, tv * vk:(tv + 1) * vk] += v[r0:r1].t() @ d[r0:r1]
    return X, Y


def _bwd_old(c, dXP, dxn, vtables):
    """The launches the kernel replaces (``smallk_atb_cols`` under the mask of a table whose first row is a multiple of 32, else
    ``smallk_atb``) on code rows whose dead rows are zeros, as the layer's are."""
    from dualmessagepassing_amd import fused
    n, vk, k0, kp, keep = c["n"], c["vk"], c["k0"], c["kp"], c["keep"]
    z = lambda t: th.where(keep.view(-1, 1), t, th.zeros_like(t)).contiguous()
    v, si, so = z(c["venc"][:, :vk]), z(c["S0"][:, :k0]), z(c["S0"][:, kp:kp + k0])
    X = th.zeros(2, c["tables"] * k0, H, device=dXP.device)
    Y = th.zeros(3 if dxn is None else 4, vtables * vk, H, device=dXP.device)
    for t in range(c["tables"]):
        r0, r1 = (0, c["split"]) if t == 0 else (c["split"], n)
        if r1 == r0:
            continue
        m = None if c["mask"] is None else c["mask"][r0 // 32:]
        for h, s in enumerate((si, so)):
            X[h, t * k0:(t + 1) * k0] = fused.smallk_atb_cols(s[r0:r1], dXP[r0:r1, :H], None, None, H, mask=m)[0]
        tv = t if vtables == 2 else 0
        Y[:, tv * vk:(tv + 1) * vk] += fused.smallk_atb_cols(v[r0:r1], dXP[r0:r1], None if dxn is None else dxn[r0:r1], None, H, mask=m)
    return X, Y


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,tables,split", [(96, 1, 0), (96, 2, 37), (257, 2, 64), (1000, 1, 0), (1000, 2, 37), (1000, 2, 512)])
def test_backward_products_against_fp64_and_the_two_launches(n, tables, split, kind, gpu):
    """``dmp_l0_node_codes_bwd``: both families of K-column products from one pass over the kept rows; bound 2e-4 of the largest
    entry (the layer tests' bound for a summed product); NaN in every gradient and code row outside the kept list."""
    for i, (vk, k0) in enumerate(CODES):
        for residual, vtables in ((True, 1), (False, tables)):
            c = _inputs(n, tables, vk, k0, kind, 0, gpu, seed=77 * n + 10 * i + tables)
            if tables == 2:
                c["split"] = split
            gen = th.Generator().manual_seed(n + i)
            dXP, dxn = th.randn(n, 3 * H, generator=gen).to(gpu), (th.randn(n, H, generator=gen).to(gpu) if residual else None)
            dXP[~c["keep"]] = float("nan")
            if dxn is not None:
                dxn[~c["keep"]] = float("nan")
            Xn, Yn = _bwd_new(c, dXP, dxn, vtables)
            X64, Y64 = _bwd_fp64(c, dXP, dxn, vtables)
            old = _bwd_old(c, dXP, dxn, vtables) if (tables == 1 or split % 32 == 0 or c["mask"] is None) else None
            for name, got, ref, o in (("Xn", Xn, X64, old and old[0]), ("Yn", Yn, Y64, old and old[1])):
                assert bool(th.isfinite(got).all()), (name, kind, vk, k0)
                tol = 2e-4 * max(1e-30, float(ref.abs().max()))
                e = float((got.double() - ref).abs().max())
                eo = float((got - o).abs().max()) if o is not None else 0.0
                assert e <= tol and eo <= tol, (name, n, tables, split, kind, vk, k0, residual, e, eo, tol)
            if i == 2:
                print("n=%d tables=%d split=%d %s VK=%d K0=%d residual=%s: Xn %.3e Yn %.3e against fp64 (largest entries %.3e, %.3e)"
                      % (n, tables, split, kind, vk, k0, residual, float((Xn.double() - X64).abs().max()), float((Yn.double() - Y64).abs().max()),
                         float(X64.abs().max()), float(Y64.abs().max())))
            X2, Y2 = _bwd_new(c, dXP, dxn, vtables)
            assert th.equal(Xn, X2) and th.equal(Yn, Y2)                 # a fixed order: repeatable


@pytest.mark.parametrize("big", [256, 257])
def test_backward_products_with_code_sums_at_the_edge_of_one_piece(big, gpu):
    c = _inputs(1000, 2, 16, 12, "ragged", big, gpu, seed=big)
    gen = th.Generator().manual_seed(big)
    dXP, dxn = th.randn(1000, 3 * H, generator=gen).to(gpu), th.randn(1000, H, generator=gen).to(gpu)
    Xn, Yn = _bwd_new(c, dXP, dxn, 2)
    X64, Y64 = _bwd_fp64(c, dXP, dxn, 2)
    for name, got, ref in (("Xn", Xn, X64), ("Yn", Yn, Y64)):
        e, s = float((got.double() - ref).abs().max()), float(ref.abs().max())
        print("sums of %d, %s: %.3e of %.3e" % (big, name, e, s))
        assert e <= 2e-4 * s


def test_a_workgroup_without_tiles_writes_zeros(gpu):
    """Nothing kept: every workgroup's partial is zeros (the buffers come uninitialised); 40,000 rows: more tiles than workgroups,
    and the partials of the workgroups past the list's end are zeros as well."""
    from dualmessagepassing_amd import _lib, fused
    from dualmessagepassing_amd.fused import ptr, stream_ptr
    lib = _lib.load()
    for n, kind in ((1000, "none"), (40000, "ragged")):
        c = _inputs(n, 2, 16, 10, kind, 0, gpu, seed=3)
        dXP, dxn = th.randn(n, 3 * H, device=gpu), th.randn(n, H, device=gpu)
        lst, cnt = c["rows"]
        G = int(lib.dmp_l0_node_codes_bwd_blocks(min(lst.numel(), n)))
        pX, pY = th.full((G, 2 * 2 * 10 * H), float("nan"), device=gpu), th.full((G, 4 * 16 * H), float("nan"), device=gpu)
        rc = lib.dmp_l0_node_codes_bwd(ptr(c["venc"]), c["venc"].stride(0), 16, 1, ptr(c["S0"]), c["S0"].stride(0), 10, c["kp"], 2, c["split"],
                                       ptr(dXP), dXP.stride(0), ptr(dxn), dxn.stride(0), ptr(lst), ptr(cnt), lst.numel(), 0, n, H, ptr(pX), ptr(pY),
                                       stream_ptr())
        assert rc == 0
        assert bool(th.isfinite(pX).all()) and bool(th.isfinite(pY).all())
        tiles = (int(cnt[0]) + 31) // 32
        used = 0 if tiles == 0 else (tiles + (tiles + G - 1) // G - 1) // ((tiles + G - 1) // G)
        assert bool((pX[used:] == 0).all()) and bool((pY[used:] == 0).all()) and (kind != "none" or used == 0)


@pytest.mark.parametrize("n,rows_g,k,stacked,gated,pad", [(0, 1, 1, False, False, 0), (5, 0, 10, False, True, 0), (37, 1000, 10, False, True, 3),
                                                          (100, 2571, 8, True, True, 0), (9, 70001, 3, True, False, 5),
                                                          (1200, 548864, 10, False, True, 0), (31, 257, 16, False, True, 1)])
def test_packed_codes_are_the_gated_rows_bit_for_bit(n, rows_g, k, stacked, gated, pad, gpu):
    """``dmp_l0_pack`` / ``dmp_l0_pack_jobs`` (a thread per 16-byte chunk of the output): ``[enc_p ; gate * enc_g]`` zero-padded,
    the second kind of rows in columns K .. 2K-1 when stacked; inputs with a row stride beyond K."""
    from dualmessagepassing_amd import fused
    gen = th.Generator().manual_seed(n + rows_g + k)
    enc_p = th.randn(n, k + pad, generator=gen).to(gpu)[:, :k]
    enc_g = th.randn(rows_g, k + pad, generator=gen).to(gpu)[:, :k]
    gate = (th.rand(rows_g, generator=gen) < 0.6).float().to(gpu) if gated else None
    goff = k if stacked else 0
    ref = th.zeros(n + rows_g, (goff + k + 3) // 4 * 4, device=gpu)
    ref[:n, :k] = enc_p
    ref[n:, goff:goff + k] = enc_g if gate is None else enc_g * gate.view(-1, 1)
    assert th.equal(fused.l0_pack(enc_p, enc_g, gate, stacked), ref)
    if n and rows_g:
        both = fused.l0_pack_many([(enc_p, enc_g, gate, stacked), (enc_g[:7], enc_p, None, False)])
        assert th.equal(both[0], ref)
        assert th.equal(both[1][:7, :k], enc_g[:7]) and th.equal(both[1][7:, :k], enc_p) and bool((both[1][:, k:] == 0).all())


# ----------------------------------------------------------------------------- the route: bench.py's model, the switch on against off
def _compact():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_compact
    return test_gpu_compact


def _records(bench_, cfg, shard, step, model):
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


def _same(step, out, flat, ref_out, ref_flat, tag):
    for k, v in ref_out.items():
        if v is None:
            assert out[k] is None
            continue
        assert bool(th.isfinite(out[k]).all()), (tag, k)
        s = max(1e-6, float(v.abs().max()))
        e = float((out[k] - v).abs().max())
        print("%s %s: %.3e of %.3e" % (tag, k, e, s))
        assert e <= 2e-5 * s, (tag, k, e, s)
    assert bool(th.isfinite(flat).all()), tag
    for prm, off in zip(step.sync.params, step.sync.offsets):
        a, b = flat[off:off + prm.numel()], ref_flat[off:off + prm.numel()]
        s = float(b.abs().max())
        if s == 0.0:
            assert float(a.abs().max()) == 0.0, (tag, off)
        else:
            assert float((a - b).abs().max()) <= 5e-5 * s, (tag, off, float((a - b).abs().max()), s)


@pytest.mark.parametrize("filt,poison", [("ScalarFilter", False), ("ScalarFilter", True), ("None", False)])
def test_model_with_the_switch_on_against_off(filt, poison, gpu):
    """bench.py's model, forward + loss + backward: gated on 64 pairs (4,608 nodes: the kept nodes' list), the same with every dead
    row's buffer poisoned, and on 8 pairs without a filter net (every node row); the timer's record names say which launches ran."""
    from dualmessagepassing_amd import fused
    sys.path.insert(0, ROOT)
    import bench
    cfg = dict(bench.CFG, batch=8 if filt == "None" else 64, filter=filt)
    bench_, shard, step, model = _compact()._model_and_batch(cfg, gpu)
    fused.USE_L0_NODE_MFMA = False
    try:
        ref_out, ref_flat, rec = _records(bench_, cfg, shard, step, model)
    finally:
        fused.USE_L0_NODE_MFMA = True
    assert rec.get("l0_node_fwd") == 2 and "l0_node_mfma" not in rec, rec          # one per table
    assert rec.get("smallk_atb_jobs") == 1 and "l0_node_bwd" not in rec, rec
    fused.POISON_DEAD_ROWS = poison
    try:
        out, flat, rec = _records(bench_, cfg, shard, step, model)
    finally:
        fused.POISON_DEAD_ROWS = False
    assert rec.get("l0_node_mfma") == 1 and "l0_node_fwd" not in rec, rec
    assert rec.get("l0_node_bwd") == 1 and "smallk_atb_jobs" not in rec, rec
    _same(step, out, flat, ref_out, ref_flat, "%s%s" % (filt, " poisoned" if poison else ""))
    out2, flat2, _ = _records(bench_, cfg, shard, step, model)
    assert all(v is None or th.equal(v, out2[k]) for k, v in out.items()) and (poison or th.equal(flat, flat2))      # repeatable


@pytest.mark.parametrize("how", ["hid64", "exact_fp32", "columns", "gate_without_kept_nodes"])
def test_fallbacks_run_the_launches_per_table(how, gpu):
    """H = 64, the exact-fp32 development switch, more code columns per block than the k-groups hold, and a node gate without the
    kept-node path (8 pairs: 576 nodes, below its 4,096): ``l0_node_fwd`` per table and the two backward launches."""
    from dualmessagepassing_amd import _lib, fused
    sys.path.insert(0, ROOT)
    import bench
    cfg = dict(bench.CFG, batch=8 if how == "gate_without_kept_nodes" else 64, filter="None" if how in ("hid64", "columns") else "ScalarFilter")
    if how == "hid64":
        cfg["hid"] = 64
    lib = _lib.load()
    saved = fused.L0_NODE_MFMA_MAX_CODES
    if how == "exact_fp32":
        lib.dmp_dev_set_exact_fp32(1)
    if how == "columns":
        fused.L0_NODE_MFMA_MAX_CODES = 4
    try:
        bench_, shard, step, model = _compact()._model_and_batch(cfg, gpu)
        out, flat, rec = _records(bench_, cfg, shard, step, model)
    finally:
        lib.dmp_dev_set_exact_fp32(0)
        fused.L0_NODE_MFMA_MAX_CODES = saved
    assert rec.get("l0_node_fwd") == 2 and "l0_node_mfma" not in rec, rec
    assert rec.get("smallk_atb_jobs") == 1 and "l0_node_bwd" not in rec, rec
    assert bool(th.isfinite(out["pred_c"]).all()) and bool(th.isfinite(flat).all())


def test_replayed_step_equals_its_eager_step(gpu):
    """``dp.StepGraph`` on bench.py's step: the recording holds the one launch (its tile count is read on the device), and a replay
    gives the bits of the eager step."""
    from dualmessagepassing_amd.dp import StepGraph
    sys.path.insert(0, ROOT)
    import bench
    cfg = dict(bench.CFG, batch=64)
    shard = bench.make_shard(cfg, 0, gpu)
    step, _ = bench.build_step(dict(cfg, graph=True), shard, gpu, 1)
    gen = th.Generator().manual_seed(7)
    with th.no_grad():
        for prm in step.sync.params:
            prm.add_((0.05 * th.randn(prm.shape, generator=gen)).to(gpu))
    g = StepGraph(lambda: step.front(), optimizer=None, max_shapes=1)
    res = []
    with g.on_stream():
        for _ in range(3):                                            # eager, recorded + replayed, replayed
            step.sync.flat.fill_(float("nan"))
            g()
            th.cuda.synchronize()
            res.append((step.last_pred_c.detach().clone(), step.sync.flat.detach().clone()))
        assert g.replays == 2
    assert bool(th.isfinite(res[0][0]).all()) and bool(th.isfinite(res[0][1]).all())
    for r in res[1:]:
        assert th.equal(res[0][0], r[0]) and th.equal(res[0][1], r[1])
