"""The relational conv's kernels (csrc/dmp_relconv.hip) against the float64 per-edge restatement of ``util_fp64.relconv_fp64``
at the branches ``test_gpu_unc_rel.py`` does not reach: bias x self-loop in all four combinations with and without tanh and
basis weights; widths above 256 (two and three column passes of the 64-lane group) and below 4; the LDS edge (R P 4 = 64 KiB:
one row per backward workgroup, on the kernels) and the next R up (on the tensor ops); N = 1 with self-loop edges; repeated
(u, v, t); all edges of one type; N one more than the rows per workgroup for every lane-group size; a norm that requires a
gradient (falls back, ``dnorm`` matches); edge types outside [0, R) contribute nothing, forward and backward; bitwise
repeatability.  Tolerances are those of ``test_gpu_unc_rel.py``: out 2e-5, dx 1e-4, parameter gradients 2e-4; at width 516 /
513 the fp32 tensor ops run beside the kernels and the kernels pass within those figures or within four times the tensor ops'
own distance from fp64 (both printed; DESIGN.md section 5 has the table)."""
import pytest
import torch as th

import util_fp64 as U

pytestmark = pytest.mark.gpu


def _spy(monkeypatch):
    from dualmessagepassing_amd import unc_rel
    calls = []
    real = unc_rel._RelAgg.apply
    monkeypatch.setattr(unc_rel._RelAgg, "apply", lambda *a: (calls.append(1), real(*a))[1])
    return calls


def _run(m, x, w_out, src, dst, et, norm, gpu):
    from dualmessagepassing_amd.graph import BatchedGraph
    m.zero_grad(set_to_none=True)
    xg = x.to(gpu).requires_grad_(True)
    out = m(BatchedGraph(src.to(gpu), dst.to(gpu), x.size(0)), xg, et.to(gpu), None if norm is None else norm.to(gpu))
    (out * w_out.to(gpu)).sum().backward()
    return out.detach(), xg.grad, {k: v.grad.clone() for k, v in m.named_parameters()}


@pytest.mark.parametrize("case", sorted(U.relconv_cases()))
def test_relconv_matches_fp64(case, gpu, monkeypatch):
    from dualmessagepassing_amd import _lib, unc_rel
    c = U.relconv_cases()[case]
    calls = _spy(monkeypatch)
    m, x, w_out = U.relconv_make(c)
    src, dst, et, norm = U.relconv_graph(c, U.stable_seed(case))
    norm = norm if c["norm"] else None
    ref, xd, p = U.relconv_fp64(m, x, src, dst, et, norm, c["act"])
    (ref * w_out.double()).sum().backward()
    m = m.to(gpu)
    out, dx, grads = _run(m, x, w_out, src, dst, et, norm, gpu)
    assert bool(_lib.load().dmp_relconv_supported(c["R"], unc_rel.padded_width(c["width"]))) == c["hip"]
    assert len(calls) == int(c["hip"]), "the case did not take the path it names"
    assert sorted(grads) == sorted(p)
    if not c["band"]:
        U.close(out, ref, 2e-5, "out")
        U.close(dx, xd.grad, 1e-4, "dx")
        for k, gk in grads.items():
            U.close(gk, p[k].grad, 2e-4, "grad " + k)
        return
    monkeypatch.setattr(_lib.load(), "dmp_relconv_supported", lambda R, P: 0)       # the same layer on the fp32 tensor ops
    out2, dx2, grads2 = _run(m, x, w_out, src, dst, et, norm, gpu)
    assert len(calls) == 1
    U.within_band(out, ref, out2, 2e-5, "relconv %s out" % case)
    U.within_band(dx, xd.grad, dx2, 1e-4, "relconv %s dx" % case)
    for k, gk in grads.items():
        U.within_band(gk, p[k].grad, grads2[k], 2e-4, "relconv %s grad %s" % (case, k))


def test_lds_edge_sits_at_64_kib():
    from dualmessagepassing_amd import _lib
    lib = _lib.load()
    e, o, q = (U.relconv_cases()[n] for n in ("lds-edge", "lds-over", "lds-edge-p4"))
    assert e["R"] * e["width"] * 4 == 65536 and o["R"] == e["R"] + 1 and q["R"] * 4 * 4 == 65536
    assert lib.dmp_relconv_supported(e["R"], e["width"]) and not lib.dmp_relconv_supported(o["R"], o["width"])
    assert lib.dmp_relconv_supported(4096, 4) and not lib.dmp_relconv_supported(4097, 4)


def test_a_norm_that_requires_a_gradient_falls_back_and_dnorm_matches(gpu, monkeypatch):
    from dualmessagepassing_amd.graph import BatchedGraph
    c = U.relconv_cases()["b1-l1-a1-full"]
    calls = _spy(monkeypatch)
    m, x, w_out = U.relconv_make(c)
    src, dst, et, norm = U.relconv_graph(c, 9)
    nd = norm.double().requires_grad_(True)
    ref, xd, p = U.relconv_fp64(m, x, src, dst, et, nd, True)     # the reference reads norm.detach(): restate with the leaf
    W = p["weight"]
    msg = th.bmm(xd[src].unsqueeze(1), W[et]).squeeze(1) * nd
    ref = th.tanh(th.zeros(c["N"], c["width"], dtype=th.float64).index_add(0, dst, msg) + p["h_bias"] + xd @ p["loop_weight"])
    (ref * w_out.double()).sum().backward()
    m = m.to(gpu)
    ng = norm.to(gpu).requires_grad_(True)
    xg = x.to(gpu).requires_grad_(True)
    out = m(BatchedGraph(src.to(gpu), dst.to(gpu), c["N"]), xg, et.to(gpu), ng)
    (out * w_out.to(gpu)).sum().backward()
    assert not calls, "a norm with a gradient must take the tensor ops"
    U.close(out, ref, 2e-5, "out")
    U.close(ng.grad, nd.grad, 1e-4, "dnorm")
    U.close(xg.grad, xd.grad, 1e-4, "dx")
    for k, q in m.named_parameters():
        U.close(q.grad, p[k].grad, 2e-4, "grad " + k)


@pytest.mark.parametrize("H,R,loop,act,with_norm", [(50, 5, 1, 1, True), (64, 3, 0, 0, False), (300, 2, 1, 0, True)])
def test_edge_types_outside_the_range_contribute_nothing(H, R, loop, act, with_norm, gpu):
    """Through ``_RelAgg`` (the kernels' own entry): types -1 and R mixed into a valid graph give the result of the graph
    without those edges, forward (out) and backward (dY, dbias).  The endpoints stay valid."""
    from dualmessagepassing_amd.graph import BatchedGraph
    from dualmessagepassing_amd.unc_rel import _RelAgg, padded_width
    N, E = 77, 600
    P = padded_width(H)
    gen = th.Generator().manual_seed(H + R)
    src, dst = th.randint(0, N, (E,), generator=gen), th.randint(0, N, (E,), generator=gen)
    et = th.randint(0, R, (E,), generator=gen)
    et[::5] = -1
    et[2::7] = R
    et[3::31] = R + 1000
    norm = th.rand(E, generator=gen) + 0.1 if with_norm else None
    Y = th.randn(N, (R + loop) * P, generator=gen)
    bias = th.rand(H, generator=gen) - 0.5
    w_out = th.randn(N, H, generator=gen)
    keep = (et >= 0) & (et < R)
    assert 0 < int(keep.sum()) < E

    Yd, bd = Y.double().requires_grad_(True), bias.double().requires_grad_(True)
    ref = U.relagg_fp64(Yd, bd, src[keep], dst[keep], et[keep], None if norm is None else norm.double()[keep], N, R, loop, H, P, act)
    (ref * w_out.double()).sum().backward()

    def run(s, d, t, n):
        Yg, bg = Y.to(gpu).requires_grad_(True), bias.to(gpu).requires_grad_(True)
        ix = BatchedGraph(s.to(gpu), d.to(gpu), N).index()
        out = _RelAgg.apply(Yg, bg, ix, t.to(gpu), None if n is None else n.to(gpu), R, loop, H, P, act)
        (out * w_out.to(gpu)).sum().backward()
        return out.detach(), Yg.grad, bg.grad

    out, dY, db = run(src, dst, et, norm)
    U.close(out, ref, 2e-5, "out")
    U.close(dY, Yd.grad, 1e-4, "dY")
    U.close(db, bd.grad, 2e-4, "dbias")
    # the padding columns of every block carry no gradient
    assert P == H or float(dY.view(N, R + loop, P)[:, :, H:].abs().max()) == 0.0
    out2, dY2, db2 = run(src[keep], dst[keep], et[keep], None if norm is None else norm[keep])
    assert th.equal(out, out2) and th.equal(dY, dY2) and th.equal(db, db2)      # same CSR order of the kept edges: same sums


@pytest.mark.parametrize("case", ["w300-nobias-noloop", "lds-edge"])
def test_two_runs_are_bitwise_equal(case, gpu, monkeypatch):
    c = U.relconv_cases()[case]
    calls = _spy(monkeypatch)
    m, x, w_out = U.relconv_make(c)
    src, dst, et, norm = U.relconv_graph(c, U.stable_seed(case))
    m = m.to(gpu)
    a = _run(m, x, w_out, src, dst, et, norm, gpu)
    b = _run(m, x, w_out, src, dst, et, norm, gpu)
    assert len(calls) == 2
    assert th.equal(a[0], b[0]) and th.equal(a[1], b[1])
    for k in a[2]:
        assert th.equal(a[2][k], b[2][k]), k
