"""Training-mode BatchNorm + activation (csrc/dmp_bn.hip through ``ops.batch_norm_act``) and its tensor-op stand-in for the
widths the kernels refuse (``ops.masked_batch_norm``) against the float64 restatement ``util_fp64.batch_norm_fp64``.

Every admitted width (4 .. 1024) with and without the affine parameters, row counts around the rows a workgroup takes per pass,
no activation, relu and a leaky slope; two consecutive calls, so the running averages accumulate; 70001 and 10858 rows; batches
padded to a capacity with live counts 1, 2, cap - 1, cap and the clamped 0 and cap + 7, +-1e6 in the padding; row 0 as an outlier
at 50 standard deviations (the statistics kernel shifts every column by a value taken from the input's rows); and, through the C entry points,
row strides above the width with a sentinel in the gap columns, and the host-side refusals.

Compared: the output, ``running_mean``, ``running_var`` (unbiased), ``num_batches_tracked``, dx, dgamma, dbeta; the padding rows
of the output and of dx are exact zeros.  The upstream gradient is zeroed where the value before the activation is within
1e-4 of zero (``test_fp64_refs_cpu.py`` bounds the share).  Tolerances: output and running statistics 1e-5, gradients 5e-5, of
max(1, max |ref|); the 70001-row and the outlier cases pass within that or within four times the distance of the float32
tensor ops from float64.  Every case asserts the path it took."""
import pytest
import torch as th

import util_fp64 as U

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = -1, -2
EPS = 1e-5


def _spy(monkeypatch):
    from dualmessagepassing_amd import _lib
    lib = _lib.load()
    seen = {"dmp_bn_train_fwd_rows": 0, "dmp_bn_train_bwd_rows": 0}
    for name in seen:
        real = getattr(lib, name)

        def call(*a, _real=real, _name=name):
            seen[_name] += 1
            return _real(*a)

        monkeypatch.setattr(lib, name, call)
    return seen


def _module(C, affine, momentum, gamma, beta, mean, var, gpu):
    bn = th.nn.BatchNorm1d(C, affine=affine, momentum=momentum, eps=EPS)
    with th.no_grad():
        bn.running_mean.copy_(mean)
        bn.running_var.copy_(var)
        if affine:
            bn.weight.copy_(gamma)
            bn.bias.copy_(beta)
    return bn.to(gpu)


def _compare(got, ref, band, what, live):
    """got / ref: dicts with y, mean, var, dx, dgamma, dbeta; ``band``: the float32 restatement's dict or None."""
    for k, tol in (("y", 1e-5), ("mean", 1e-5), ("var", 1e-5), ("dx", 5e-5), ("dgamma", 5e-5), ("dbeta", 5e-5)):
        if ref[k] is None:
            assert got[k] is None
        elif band is None:
            U.close(got[k], ref[k], tol, what + k)
        else:
            U.within_band(got[k], ref[k], band[k], tol, "bn %s%s" % (what, k))
    assert not bool(got["y"][live:].any()) and not bool(got["dx"][live:].any()), what + "padding rows are not exact zeros"


@pytest.mark.parametrize("case", sorted(U.bn_cases()))
def test_batch_norm_act_matches_fp64(case, gpu, monkeypatch):
    from dualmessagepassing_amd import ops
    c = U.bn_cases()[case]
    C, affine = c["C"], c["affine"]
    seen = _spy(monkeypatch)
    for run, (R, n, slope) in enumerate(c["runs"]):
        x, dy, gamma, beta, mean, var = U.bn_inputs(case, run)
        live = U.bn_live(R, n)
        if not affine:
            gamma = beta = None
        ref = U.bn_reference(x, dy, gamma, beta, mean, var, c["momentum"], EPS, live, slope)
        bn = _module(C, affine, c["momentum"], gamma, beta, mean, var, gpu)
        xg = x.to(gpu).requires_grad_(True)
        rows_dev = None if n is None else th.tensor([n], dtype=th.int64, device=gpu)
        assert ops.batch_norm_act_ok(bn, xg)
        for _ in range(2):
            y = ops.batch_norm_act(bn, xg, slope, rows_dev)
        grads = th.autograd.grad(y, [xg] + list(bn.parameters()), th.where(ref["safe"], dy, th.zeros(())).to(gpu))
        assert seen == {"dmp_bn_train_fwd_rows": 2 * (run + 1), "dmp_bn_train_bwd_rows": run + 1}, "the HIP path was not taken"
        assert int(bn.num_batches_tracked) == 2
        got = dict(y=y.detach(), mean=bn.running_mean, var=bn.running_var, dx=grads[0], dgamma=grads[1] if affine else None,
                   dbeta=grads[2] if affine else None)
        band = None
        if c["band"]:
            band = U.bn_reference(x, dy, gamma, beta, mean, var, c["momentum"], EPS, live, slope, dtype=th.float32, safe=ref["safe"])
        _compare(got, ref, band, "%s R%d n%s slope%s " % (case, R, n, slope), live)


# ------------------------------------------------------------------------------------------------- through the C entry points

def _lib():
    from dualmessagepassing_amd import _lib as L
    return L, L.load()


def _strided(t, ld, gpu, fill=7.0):
    buf = th.full((t.size(0), ld), fill, device=gpu)
    buf[:, :t.size(1)] = t.to(gpu)
    return buf


@pytest.mark.parametrize("C,R,lds,slope", [(64, 37, (72, 68, 80, 76), 1.0 / 5.5), (256, 10, (260, 512, 264, 256), None), (4, 300, (8, 4, 12, 16), 0.0)],
                         ids=["C64", "C256", "C4"])
def test_entry_points_with_row_strides_above_the_width(C, R, lds, slope, gpu):
    """ldx, ldo (the output is the backward's y: ldy), lddy and the ld of dx all differ from C; every buffer is allocated at its
    full stride and the gap columns keep their fill."""
    L, lib = _lib()
    ldx, ldy, lddy, ldd = lds
    g = th.Generator().manual_seed(C + R)
    x, dy = th.randn(R, C, generator=g) * 3.0 + th.randn(C, generator=g) * 5.0, th.randn(R, C, generator=g)
    gamma, beta, mean, var = th.rand(C, generator=g) + 0.5, th.randn(C, generator=g), th.randn(C, generator=g), th.rand(C, generator=g) + 0.5
    ref = U.bn_reference(x, dy, gamma, beta, mean, var, 0.1, EPS, R, slope, steps=1)
    xg, dyg = _strided(x, ldx, gpu), _strided(th.where(ref["safe"], dy, th.zeros(())), lddy, gpu)
    out, dx = th.full((R, ldy), 7.0, device=gpu), th.full((R, ldd), 7.0, device=gpu)
    gg, bg, rm, rv = gamma.to(gpu), beta.to(gpu), mean.to(gpu), var.to(gpu)
    nb = int(lib.dmp_bn_partial_rows(R, C))
    assert nb >= 1
    partial, stats = th.empty(nb, 2 * C, device=gpu), th.empty(4 * C, device=gpu)
    act, sl = int(slope is not None), float(slope or 0.0)
    assert lib.dmp_bn_train_fwd_rows(xg.data_ptr(), ldx, R, None, C, gg.data_ptr(), bg.data_ptr(), EPS, 0.1, rm.data_ptr(), rv.data_ptr(),
                                     act, sl, partial.data_ptr(), stats.data_ptr(), out.data_ptr(), ldy, L.stream_ptr()) == 0
    assert lib.dmp_bn_train_bwd_rows(xg.data_ptr(), ldx, out.data_ptr(), ldy, dyg.data_ptr(), lddy, R, None, C, gg.data_ptr(), act, sl,
                                     partial.data_ptr(), stats.data_ptr(), dx.data_ptr(), ldd, L.stream_ptr()) == 0
    th.cuda.synchronize()
    got = dict(y=out[:, :C], mean=rm, var=rv, dx=dx[:, :C], dgamma=stats[3 * C:], dbeta=stats[2 * C:3 * C])
    _compare(got, ref, None, "C%d strided " % C, R)
    for buf, ld in ((out, ldy), (dx, ldd), (xg, ldx), (dyg, lddy)):
        assert ld == C or bool((buf[:, C:] == 7.0).all()), "a gap column was written"


@pytest.mark.parametrize("bad", [dict(C=12), dict(C=2048), dict(off=4), dict(ldx=66), dict(ldo=70), dict(slope=1.5), dict(slope=-0.1)],
                         ids=["C12", "C2048", "misaligned", "ldx%4", "ldo%4", "slope>1", "slope<0"])
def test_entry_point_refusals_return_unsupported_and_launch_nothing(bad, gpu):
    L, lib = _lib()
    a = dict(C=64, off=0, ldx=None, ldo=None, slope=0.5)
    a.update(bad)
    C, R = a["C"], 8
    ldx, ldo = a["ldx"] or C, a["ldo"] or C
    x, out, dy, dx = (th.full((R * max(ldx, ldo) + 4,), 7.0, device=gpu) for _ in range(4))
    gamma, partial, stats = th.ones(C, device=gpu), th.full((2 * C,), 7.0, device=gpu), th.full((4 * C,), 7.0, device=gpu)
    assert lib.dmp_bn_partial_rows(R, C) == (0 if "C" in bad else 1)
    assert lib.dmp_bn_train_fwd_rows(x.data_ptr() + a["off"], ldx, R, None, C, gamma.data_ptr(), gamma.data_ptr(), EPS, 0.1, None, None, 1,
                                     a["slope"], partial.data_ptr(), stats.data_ptr(), out.data_ptr(), ldo, L.stream_ptr()) == UNSUPPORTED
    assert lib.dmp_bn_train_bwd_rows(x.data_ptr() + a["off"], ldx, out.data_ptr(), ldo, dy.data_ptr(), ldo, R, None, C, gamma.data_ptr(), 1,
                                     a["slope"], partial.data_ptr(), stats.data_ptr(), dx.data_ptr(), ldo, L.stream_ptr()) == UNSUPPORTED
    th.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (out, dx, partial, stats))


# ------------------------------------------------------------------------------------------------------ masked_batch_norm

@pytest.mark.parametrize("cap,n,momentum", U.MASKED_BN_RUNS)
def test_masked_batch_norm_matches_fp64_and_the_kernels_at_the_next_width(cap, n, momentum, gpu, monkeypatch):
    """Width 50 goes through ``apply_mlp`` to ``masked_batch_norm`` (tensor ops, asserted); the same rows at width 64, the next one the
    kernels admit, go to the kernels, which must agree on the shared columns (for ``momentum=None`` the kernels are not admitted either)."""
    from dualmessagepassing_amd import ops
    x, dy, gamma, beta, mean, var = U.masked_bn_inputs(cap, n)
    live = U.bn_live(cap, n)
    seen = _spy(monkeypatch)
    masked = []
    real = ops.masked_batch_norm
    monkeypatch.setattr(ops, "masked_batch_norm", lambda *a: (masked.append(1), real(*a))[1])
    rows_dev = th.tensor([n], dtype=th.int64, device=gpu)
    res = {}
    for C in (50, 64):
        cut = [t[..., :C] for t in (x, dy, gamma, beta, mean, var)]
        ref = U.bn_reference(*cut, momentum, EPS, live, None)
        bn = _module(C, True, momentum, *cut[2:], gpu)
        seq = th.nn.Sequential(bn)
        xg = cut[0].contiguous().to(gpu).requires_grad_(True)
        before = (len(masked), dict(seen))
        for _ in range(2):
            y = ops.apply_mlp(seq, xg, rows_dev)
        grads = th.autograd.grad(y, [xg, bn.weight, bn.bias], cut[1].contiguous().to(gpu))
        hip = C == 64 and momentum is not None
        assert len(masked) - before[0] == (0 if hip else 2), "the path taken at width %d" % C
        assert seen["dmp_bn_train_fwd_rows"] - before[1]["dmp_bn_train_fwd_rows"] == (2 if hip else 0)
        assert int(bn.num_batches_tracked) == 2
        res[C] = dict(y=y.detach(), mean=bn.running_mean, var=bn.running_var, dx=grads[0], dgamma=grads[1], dbeta=grads[2])
        _compare(res[C], ref, None, "width %d n%d momentum %s " % (C, n, momentum), live)
    for k in res[50]:
        err, scale = U.dist(res[50][k], res[64][k][..., :50])
        assert err <= 2 * {"y": 1e-5, "mean": 1e-5, "var": 1e-5}.get(k, 5e-5) * scale, (k, err, scale)
