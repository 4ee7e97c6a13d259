"""The pooled prediction heads (csrc/dmp_heads.hip: ``dmp_heads_forward``, ``dmp_heads_backward``, ``dmp_heads_blend`` through
``pred._PooledHeadsHIP``) and the count loss (``dmp_count_loss`` through ``harness.count_loss``) against the float64
restatements of ``util_fp64``.

Heads: both widths, relu and two leaky slopes, B on the edges of the forward's 16-row tiles (15, 16, 17), of the weight
gradient's groups of four rows (B % 4 != 0) and of its 256-row prefetch (255, 256, 257), B = 1 and B past 1024; one and two
heads (two is ``DMP_HEADS_MAX``; three are refused on the host); the blend absent, given and taken from the target sizes by the
blend kernel; bias factors L and 1; ``sums`` as a column slice whose stride the op passes to the kernels, and one it has to
copy; sizes up to 512.  The blended count is compared on all rows; the gradients by ``sums`` and by all eight parameters per
head are taken with the cotangent zeroed on the rows the reference finds unsafe (a hidden pre-activation within 1e-5 max |pre|
of zero; ``test_fp64_refs_cpu.py`` bounds their share).  Every case asserts the launches it made.

Count loss: n on both sides of the workgroup's 1024 threads and far past it, the three criteria, slopes 1, 0.01 and 0, a block
of entries exactly on the kinks (pred = 0, d = 0, |d| = 1), where torch's conventions are the expected value.

Tolerances: heads forward 1e-5 and gradients 1e-4, loss and dpred 1e-5, of max(1, max |ref|); the heads at B >= 1024 and the loss
at n = 65537 pass within that or within four times the distance of the fp32 tensor ops from float64 (``util_fp64.within_band``)."""
import ctypes

import pytest
import torch as th

import util_fp64 as U

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = -1, -2


def _spy(monkeypatch, *names):
    """Counts the calls of the named C entry points; the forward's records the row strides it was given."""
    from dualmessagepassing_amd import _lib
    lib = _lib.load()
    seen = {n: [] for n in names}
    for name in names:
        real = getattr(lib, name)

        def call(*a, _real=real, _name=name):
            seen[_name].append([(a[1][i].ld_ps, a[1][i].ld_gs) for i in range(a[2])] if _name == "dmp_heads_forward" else 1)
            return _real(*a)

        monkeypatch.setattr(lib, name, call)
    return seen


def _product(c, d, safe, gpu):
    """The op on the device copies of a case's inputs: (y, d wide per head, parameter gradients per head)."""
    from dualmessagepassing_amd.pred import _PooledHeadsHIP
    H, B, c0 = c["H"], c["B"], d["c0"]
    params = [[t.to(gpu).requires_grad_(True) for t in head] for head in d["params"]]
    wide = [t.to(gpu).requires_grad_(True) for t in d["wide"]]
    flat = []
    for i in range(c["heads"]):
        blend = "len" if c["blend"] == "len" else (None if d["blends"][i] is None else d["blends"][i].to(gpu))
        flat += [wide[i][:, c0:c0 + H], d["pl"][i].to(gpu), d["gl"][i].to(gpu), d["scale_p"], d["scale_g"], blend] + params[i]
    y = _PooledHeadsHIP.apply(c["heads"], c["slope"], *flat)
    (y * (d["cot"] * safe.view(-1, 1)).to(gpu)).sum().backward()
    return y.detach(), [w.grad for w in wide], [[t.grad for t in head] for head in params]


@pytest.mark.parametrize("case", sorted(U.heads_cases()))
def test_heads_match_fp64(case, gpu, monkeypatch):
    c = U.heads_cases()[case]
    d = U.heads_inputs(case)
    H, n = c["H"], c["heads"]
    ref = U.heads_reference(c, d)
    seen = _spy(monkeypatch, "dmp_heads_forward", "dmp_heads_backward", "dmp_heads_blend")
    y, dwide, dparams = _product(c, d, ref["safe"], gpu)
    width = d["wide"][0].size(1)
    assert seen["dmp_heads_forward"] == [[(width if c["stride"] == "pass" else H,) * 2] * n], "the stride the kernels were given"
    assert len(seen["dmp_heads_backward"]) == 1 and len(seen["dmp_heads_blend"]) == int(c["blend"] == "len")
    yard = U.heads_reference(c, d, dtype=th.float32, device=gpu, safe=ref["safe"]) if c["band"] else None

    if yard is None:
        U.close(y, ref["y"], 1e-5, "y")
        for i in range(n):
            U.close(dwide[i], ref["dwide"][i], 1e-4, "dsums%d" % i)
            for j, name in enumerate(U.HEAD_PARAMS):
                U.close(dparams[i][j], ref["dparams"][i][j], 1e-4, "d%s%d" % (name, i))
        return
    U.within_band(y, ref["y"], yard["y"], 1e-5, "heads %s y" % case)
    rows = []
    for i in range(n):                                           # every gradient is asserted; the worst one is printed
        for name, a, b, f in [("sums", dwide[i], ref["dwide"][i], yard["dwide"][i])] + [
                (name, dparams[i][j], ref["dparams"][i][j], yard["dparams"][i][j]) for j, name in enumerate(U.HEAD_PARAMS)]:
            assert bool(th.isfinite(a).all()), name
            err, scale = U.dist(a, b)
            yerr, _ = U.dist(f, b)
            rows.append((err / scale, yerr / scale, scale, "d%s%d" % (name, i)))
            assert err <= max(1e-4 * scale, 4.0 * yerr), "d%s%d: %g against fp64, the fp32 tensor ops %g (scale %g)" % (name, i, err, yerr, scale)
    print("FP64BAND heads %s worst-grad(%s) kernel %.3g yardstick %.3g (x scale %.3g)" % ((case, max(rows)[3]) + max(rows)[:3]))


@pytest.mark.parametrize("B", [257, 1024])
def test_heads_are_bitwise_reproducible(B, gpu):
    name = sorted(k for k, c in U.heads_cases().items() if c["B"] == B and c["blend"] == "len" and c["lmax"] is None)[0]
    c = U.heads_cases()[name]
    d = U.heads_inputs(name)
    safe = th.ones(B, dtype=th.bool)
    y0, w0, p0 = _product(c, d, safe, gpu)
    y1, w1, p1 = _product(c, d, safe, gpu)
    assert th.equal(y0, y1)
    for a, b in zip(w0 + [t for h in p0 for t in h], w1 + [t for h in p1 for t in h]):
        assert th.equal(a, b)


def test_more_heads_than_the_maximum_are_refused_on_the_host(gpu):
    from dualmessagepassing_amd import _abi, _lib
    lib = _lib.load()
    H, B, n = 64, 4, U.HEADS_MAX + 1
    buf = lambda *shape: th.full(shape, 7.0, device=gpu)
    W, IO = (_abi.dmp_head_weights * n)(), (_abi.dmp_head_io * n)()
    keep = []
    for i in range(n):
        prm = [buf(H, H), buf(H), buf(H, H), buf(H), buf(H, 4 * H + 4), buf(H), buf(1, H + 4), buf(1)]
        io = dict(ps=buf(B, H), gs=buf(B, H), pl=buf(B), gl=buf(B), F=buf(B, 4 * H + 4), Y1S=buf(B, H + 4), y=buf(B))
        for name, t in zip(U.HEAD_PARAMS, prm):
            setattr(W[i], name, t.data_ptr())
        for name, t in io.items():
            setattr(IO[i], name, t.data_ptr())
        IO[i].ld_ps = IO[i].ld_gs = H
        IO[i].scale_p = IO[i].scale_g = 1.0
        keep.append((prm, io))
    assert lib.dmp_heads_forward(W, IO, n, B, H, 0.0, _lib.stream_ptr()) == BAD_ARG
    out, ws = buf(B), [buf(B) for _ in range(n)]
    ptrs = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    assert lib.dmp_heads_blend(ptrs([k[1]["y"] for k in keep]), ptrs([k[1]["gl"] for k in keep]), ptrs(ws), n, B, out.data_ptr(),
                               _lib.stream_ptr()) == BAD_ARG
    th.cuda.synchronize()
    assert all(bool((k[1]["y"] == 7.0).all()) for k in keep) and bool((out == 7.0).all())       # nothing was launched
    assert lib.dmp_heads_forward(W, IO, U.HEADS_MAX, B, 96, 0.0, _lib.stream_ptr()) == UNSUPPORTED
    assert lib.dmp_heads_forward(W, IO, U.HEADS_MAX, B, H, 1.5, _lib.stream_ptr()) == UNSUPPORTED


# --------------------------------------------------------------------------------------------------------------- count loss

def _criterion(pred, target, kind, slope):
    import torch.nn.functional as F
    p = pred.detach().clone().requires_grad_(True)
    loss = {"MSE": F.mse_loss, "MAE": F.l1_loss, "SMSE": F.smooth_l1_loss}[kind](F.leaky_relu(p, slope), target)
    loss.backward()
    return loss.detach(), p.grad


@pytest.mark.parametrize("case", sorted(U.count_loss_cases()))
def test_count_loss_matches_fp64_on_and_off_the_kinks(case, gpu, monkeypatch):
    from dualmessagepassing_amd import harness
    n, kind, slope, band = U.count_loss_cases()[case]
    pred, target = U.count_loss_inputs(case)
    loss0, dp0 = U.count_loss_fp64(pred, target, kind, slope)
    seen = _spy(monkeypatch, "dmp_count_loss")
    pg, tg = pred.to(gpu).requires_grad_(True), target.to(gpu)
    loss = harness.count_loss(pg, tg, kind, slope)
    loss.backward()
    assert len(seen["dmp_count_loss"]) == 1 and loss.shape == ()
    if band:
        ly, dy = _criterion(pg, tg, kind, slope)
        U.within_band(loss.detach(), loss0, ly, 1e-5, "count-loss %s loss" % case)
        U.within_band(pg.grad, dp0, dy, 1e-5, "count-loss %s dpred" % case)
    else:
        U.close(loss.detach(), loss0, 1e-5, "loss")
        U.close(pg.grad, dp0, 1e-5, "dpred")
    # the same bits from a second launch, and from 1-D views of both
    again = pred.to(gpu).requires_grad_(True)
    loss1 = harness.count_loss(again, tg, kind, slope)
    loss1.backward()
    flat = pred.to(gpu).view(-1).requires_grad_(True)
    loss2 = harness.count_loss(flat, tg.view(-1), kind, slope)
    loss2.backward()
    assert len(seen["dmp_count_loss"]) == 3
    assert th.equal(loss1, loss) and th.equal(again.grad, pg.grad)
    assert th.equal(loss2, loss) and flat.grad.shape == (n,) and th.equal(flat.grad.view(n, 1), pg.grad)


@pytest.mark.parametrize("bad,code", [(dict(n=0), BAD_ARG), (dict(kind=3), BAD_ARG), (dict(kind=-1), BAD_ARG), (dict(slope=-0.01), UNSUPPORTED),
                                      (dict(slope=1.5), UNSUPPORTED), (dict(slope=float("nan")), UNSUPPORTED),
                                      (dict(n=(1 << 22) + 1), UNSUPPORTED)],
                         ids=["n0", "kind3", "kind-1", "slope<0", "slope>1", "slope-nan", "n>2^22"])
def test_count_loss_refusals_return_a_code_and_launch_nothing(bad, code, gpu):
    from dualmessagepassing_amd import _lib
    lib = _lib.load()
    a = dict(n=8, kind=0, slope=0.5)
    a.update(bad)
    pred, target = th.zeros(8, device=gpu), th.zeros(8, device=gpu)
    loss, dpred = th.full((1,), 7.0, device=gpu), th.full((8,), 7.0, device=gpu)
    assert lib.dmp_count_loss(pred.data_ptr(), target.data_ptr(), a["n"], a["kind"], a["slope"], loss.data_ptr(), dpred.data_ptr(),
                              _lib.stream_ptr()) == code
    th.cuda.synchronize()
    assert float(loss) == 7.0 and bool((dpred == 7.0).all())
