"""The sparsemax attention kernels (csrc/dmp_attn.hip) against fp64 beyond one query tile.

The forward carries 16 query rows per workgroup, the backward rows kernel 8 (dh >= 16) or 16, and both recover
(tile, head, pair) from the block index; tests/test_gpu_attn.py compares values at Lq <= 9, one tile.  Here:

* the sweep of tests/util_fp64_attn.py (Lq 16 / 17 / 40 / 130 x Lk 3 / 70 / 2049 x every head width x 1 and 3 heads,
  2 or 3 pairs): every output, tau and supp included, against ``reference`` pinned to the kernel's own support sizes,
  which ``admissible`` holds to fp64's up to the keys inside the rounding window.  No row is excluded for being near its
  threshold; the condition that makes the pin unambiguous is asserted on the fp64 side of every case;
* one-sided and absent masks, empty batches and empty query sets, non-contiguous and unaligned inputs, reproducibility
  and every output written at three tiles on both sides of the LDS score cache;
* DotAttention, the three attention heads and MemDotAttention at 40 query rows, the HIP route forced, against a deep
  copy of the module run in double on the CPU, at seeds whose double run has no key in any row's window.
Tolerances: tau and O 1e-5, dQ / dK / dV 1e-4 (tests/test_gpu_attn.py's); modules 1e-4 / 2e-4 (its fixture tests')."""
import copy

import pytest
import torch as th

import util_fp64_attn as U

pytestmark = pytest.mark.gpu


def _run(case, dev, q=None, k=None, v=None, dout=None):
    """The kernels on ``case`` (or on the given device tensors in its place) -> (o, tau, supp, dq, dk, dv)."""
    from dualmessagepassing_amd.attn import SparsemaxAttention
    leaves = [x.float().to(dev).requires_grad_(True) if y is None else y for x, y in ((case.q, q), (case.k, k), (case.v, v))]
    qm, km = (None if m is None else m.to(dev) for m in (case.qm, case.km))
    o, tau, supp = SparsemaxAttention.apply(leaves[0], leaves[1], leaves[2], qm, km, case.nh, case.scale)
    o.backward(case.dout.float().to(dev) if dout is None else dout)
    th.cuda.synchronize()
    return (o, tau, supp) + tuple(x.grad for x in leaves)


# ----------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("Lq,Lk,dh,nh", U.SWEEP)
def test_kernels_match_pinned_fp64(Lq, Lk, dh, nh, gpu):
    from dualmessagepassing_amd import attn
    assert dh in attn.KERNEL_DH and set(U.DHS) == set(attn.KERNEL_DH)
    case = U.sweep_case(Lq, Lk, dh, nh)
    assert attn.kernel_ok(case.q.float().to(gpu), case.k.float().to(gpu), case.v.float().to(gpu), nh)
    U.check_outputs(_run(case, gpu), case, "Lq %d Lk %d dh %d nh %d" % (Lq, Lk, dh, nh))


MASK_SEED = 7


@pytest.mark.parametrize("qmask,kmask", [(False, True), (True, False), (False, False)], ids=["no-qmask", "no-kmask", "no-masks"])
def test_one_sided_masks(qmask, kmask, gpu):
    case = U.make_case(3, 40, 70, 3, 16, MASK_SEED, qmask=qmask, kmask=kmask)
    U.check_outputs(_run(case, gpu), case, "masks q %s k %s" % (qmask, kmask))


# ----------------------------------------------------------------------------- empty shapes
@pytest.mark.parametrize("B,Lq", [(0, 5), (3, 0), (0, 0)])
def test_empty_shapes(B, Lq, gpu):
    """No pair, or no query row, against Lk = 6 keys: the shapes and dtypes of the tensor route, exact zeros in dK and dV
    where there is no query row, nothing raises."""
    from dualmessagepassing_amd import attn
    g = th.Generator().manual_seed(B * 10 + Lq)
    q, k, v = th.randn(B, Lq, 32, generator=g), th.randn(B, 6, 32, generator=g), th.randn(B, 6, 32, generator=g)
    qm, km = th.rand(B, Lq, generator=g) > 0.3, th.rand(B, 6, generator=g) > 0.3
    for masks in ((qm, km), (None, None)):
        got, want = [], []
        for dev, out in ((gpu, got), ("cpu", want)):
            x = [t.clone().to(dev).requires_grad_(True) for t in (q, k, v)]
            if dev == "cpu":
                o = attn.attention_tensor(*x, *masks, 4, 0.5)
            else:
                assert attn.kernel_ok(*x, 4)
                o = attn.sparsemax_attention(*x, *(None if m is None else m.to(dev) for m in masks), 4, 0.5)
            (o * 2.0).sum().backward()
            out.extend([o] + [t.grad for t in x])
        th.cuda.synchronize()
        for a, b, what in zip(got, want, ("O", "dQ", "dK", "dV")):
            assert a is not None and a.shape == b.shape and a.dtype == b.dtype, (what, a.shape if a is not None else None, b.shape)
            assert th.equal(a.cpu(), b), what                                  # empty, or exact zeros
        if B > 0:
            assert got[2].numel() and float(got[2].abs().max()) == 0.0 and float(got[3].abs().max()) == 0.0


# ----------------------------------------------------------------------------- layout
LAYOUT_SEED = 11


def _offset(x, dev):
    """A contiguous fp32 copy of ``x`` that starts 4 bytes into a larger buffer."""
    buf = th.empty(x.numel() + 1, dtype=th.float32, device=dev)
    view = buf[1:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def test_non_contiguous_inputs(gpu):
    """q a column slice of a wider tensor, k the transpose of a sequence-first tensor, v a [B, nh, L, dh] layout transposed
    and reshaped back: the same bits as on contiguous copies, gradients at the leaves included."""
    case = U.make_case(3, 40, 70, 3, 16, LAYOUT_SEED)
    B, Lq, D = case.q.shape
    Lk, nh = case.k.size(1), case.nh
    plain = _run(case, gpu)
    U.check_outputs(plain, case, "contiguous")
    wide = th.randn(B, Lq, D + 24, device=gpu)
    wide[..., 8:8 + D] = case.q.float().to(gpu)
    wide.requires_grad_(True)
    seq_first = case.k.float().to(gpu).transpose(0, 1).contiguous().requires_grad_(True)
    by_head = case.v.float().to(gpu).view(B, Lk, nh, -1).permute(0, 2, 1, 3).contiguous().requires_grad_(True)
    q, k, v = wide[..., 8:8 + D], seq_first.transpose(0, 1), by_head.permute(0, 2, 1, 3).reshape(B, Lk, D)
    assert not q.is_contiguous() and not k.is_contiguous()
    from dualmessagepassing_amd.attn import SparsemaxAttention, kernel_ok
    assert kernel_ok(q, k, v, nh)
    o, tau, supp = SparsemaxAttention.apply(q, k, v, case.qm.to(gpu), case.km.to(gpu), nh, case.scale)
    o.backward(case.dout.float().to(gpu))
    th.cuda.synchronize()
    dq, dk, dv = wide.grad[..., 8:8 + D], seq_first.grad.transpose(0, 1), by_head.grad.permute(0, 2, 1, 3).reshape(B, Lk, D)
    for a, b, what in zip((o, tau, supp, dq, dk, dv), plain, ("O", "tau", "supp", "dQ", "dK", "dV")):
        assert th.equal(a, b), what
    assert float(wide.grad[..., :8].abs().max()) == 0.0 and float(wide.grad[..., 8 + D:].abs().max()) == 0.0


def test_unaligned_inputs(gpu):
    """q, k, v and dO contiguous at a 4-byte offset into a larger buffer (the kernels load float4): the kernel route takes
    them, with the same bits as on aligned copies."""
    from dualmessagepassing_amd import attn
    case = U.make_case(3, 40, 70, 3, 16, LAYOUT_SEED)
    plain = _run(case, gpu)
    q, k, v = (_offset(x.float().to(gpu), gpu).requires_grad_(True) for x in (case.q, case.k, case.v))
    assert attn.kernel_ok(q, k, v, case.nh)
    got = _run(case, gpu, q, k, v, _offset(case.dout.float().to(gpu), gpu))
    for a, b, what in zip(got, plain, ("O", "tau", "supp", "dQ", "dK", "dV")):
        assert th.equal(a, b), what
    U.check_outputs(got, case, "unaligned")
    out = attn.sparsemax_attention(q, k, v, case.qm.to(gpu), case.km.to(gpu), case.nh, case.scale)
    assert th.equal(out, plain[0])


# ----------------------------------------------------------------------------- reproducible, every output written
@pytest.mark.parametrize("Lk,dh", [(2048, 64), (2048, 4), (2049, 16), (2049, 8)])
def test_three_tiles_reproducible_and_written(Lk, dh, gpu, monkeypatch):
    """Lq = 40 (3 forward tiles, the last with two empty waves), 3 heads, the last key count the LDS score cache holds and
    the first it does not, output buffers poisoned: nothing of O, tau, supp, dQ, dK, dV is left unwritten, two runs agree
    bit for bit, and the values are fp64's."""
    from dualmessagepassing_amd import fused
    monkeypatch.setattr(fused, "POISON_DEAD_ROWS", True)
    case = U.make_case(2, 40, Lk, 3, dh, 100 + Lk + dh)
    a, b = _run(case, gpu), _run(case, gpu)
    for x, y, what in zip(a, b, ("O", "tau", "supp", "dQ", "dK", "dV")):
        assert not (th.isnan(x).any() if x.dtype.is_floating_point else (x == -1).any()), what
        assert th.equal(x, y), what
    U.check_outputs(a, case, "poisoned Lk %d dh %d" % (Lk, dh))


# ----------------------------------------------------------------------------- modules at production-like lengths
def prefix_mask(lengths, L):
    return th.arange(L).view(1, L) < th.tensor(lengths).view(-1, 1)


def build_module(kind, seed):
    """-> (module, float inputs that take gradients, call(module, inputs) -> tuple of outputs); CPU, fp32."""
    from dualmessagepassing_amd import pred
    th.manual_seed(seed)
    B, Lg, Lp = 3, 40, 9
    g_mask, p_mask = prefix_mask([40, 23, 1], Lg), prefix_mask([9, 4, 1], Lp)
    if kind.startswith("dot_"):
        nh, dh = (4, 4) if kind.endswith("h4") else (2, 16)
        D = 16
        net = pred.DotAttention(D, D, D, nh * dh, num_heads=nh, scale=1 / dh ** 0.5)
        query = th.randn(B, Lg, D) * g_mask.unsqueeze(-1)
        if kind.startswith("dot_self"):
            return net, [query], lambda m, x, to: (m(x[0], x[0], x[0], query_mask=to(g_mask), key_mask=to(g_mask)),)
        key, value = th.randn(B, Lp, D) * p_mask.unsqueeze(-1), th.randn(B, Lp, D) * p_mask.unsqueeze(-1)
        return net, [query, key, value], lambda m, x, to: (m(x[0], x[1], x[2], query_mask=to(g_mask), key_mask=to(p_mask)),)
    if kind == "memdot":
        net = pred.MemDotAttention(12, 20, 20, 16, 16, num_heads=4, scale=1.0, mem_len=4, mem_init="mean", pre_lnorm=True)
        k_mask = prefix_mask([15, 6, 1], 15)
        x = [th.randn(B, Lg, 12) * g_mask.unsqueeze(-1), th.randn(B, 15, 20) * k_mask.unsqueeze(-1), th.randn(B, 15, 20) * k_mask.unsqueeze(-1)]
        return net, x, lambda m, x, to: (m(x[0], x[1], x[2], query_mask=to(g_mask), key_mask=to(k_mask)),)
    cls = {"head_sum": pred.SumAttnPredictNet, "head_mean": pred.MeanAttnPredictNet, "head_max": pred.MaxAttnPredictNet}[kind]
    net = cls(16, 16, num_heads=4, infer_steps=3, return_weights=True)
    with th.no_grad():                           # the last Linears start at zero: the outputs and every gradient but theirs would be 0
        for lin in (net.pred_fc2, net.weight_fc2):
            lin.weight.normal_(0.0, 0.3)
            lin.bias.normal_(0.0, 0.3)
    x = [th.randn(B, Lp, 16) * p_mask.unsqueeze(-1), th.randn(B, Lg, 16) * g_mask.unsqueeze(-1)]
    return net, x, lambda m, x, to: m(x[0], to(p_mask), x[1], to(g_mask))


def run_module(net, inputs, call, dev, dtype, weights=None):
    """-> (outputs, input gradients, parameter gradients by name, the output weights of the loss)."""
    net = copy.deepcopy(net).to(device=dev, dtype=dtype)
    x = [t.to(device=dev, dtype=dtype).requires_grad_(True) for t in inputs]
    outs = call(net, x, lambda m: m.to(dev))
    if weights is None:
        g = th.Generator().manual_seed(1)
        weights = [th.randn(o.shape, generator=g, dtype=th.float64) for o in outs]
    sum((o * w.to(device=dev, dtype=dtype)).sum() for o, w in zip(outs, weights)).backward()
    return outs, [t.grad for t in x], {k: p.grad for k, p in net.named_parameters()}, weights


def double_run(kind, seed, monkeypatch):
    """The module in double on the CPU (tensor route); -> its run, the number of sparsemax rows computed, and how many of
    them have a live key inside the window of the row's threshold."""
    from dualmessagepassing_amd import attn, pred
    net, inputs, call = build_module(kind, seed)
    orig = attn.sparsemax
    seen = [0, 0]

    def spy(s, dim=-1):
        p = orig(s, dim)
        assert dim == 2 and s.dtype == th.float64
        live = s > -1e29                                                         # attention_tensor fills masked keys with -1e30
        some = live.any(dim=2)
        tau = (s - p).masked_fill(p == 0, float("inf")).amin(dim=2, keepdim=True)       # s - p on the support
        gap = (s - tau).abs().masked_fill(~live, float("inf")).amin(dim=2)
        big = th.clamp_min(s.abs().masked_fill(~live, 0.0).amax(dim=2), 1.0)
        seen[0] += int(some.sum())
        seen[1] += int(((gap < U.WINDOW * big) & some).sum())
        return p
    def sizes(p_mask, g_mask):                   # PredictNet._size_features, which is fp32 whatever the module's dtype
        pl, gl = p_mask.sum(dim=1).double().unsqueeze(1), g_mask.sum(dim=1).double().unsqueeze(1)
        return th.cat([pl, gl, pl.reciprocal(), gl.reciprocal()], dim=1)
    with monkeypatch.context() as m:
        m.setattr(attn, "sparsemax", spy)
        m.setattr(pred.PredictNet, "_size_features", staticmethod(sizes))
        ref = run_module(net, inputs, call, "cpu", th.float64)
    return (net, inputs, call), ref, seen


# seeds at which the double run has no key in any row's window (asserted; the heads compute 2,880 sparsemax rows, of which
# one to seven have a window key at most seeds)
MODULE_SEEDS = {"dot_cross_h4": 0, "dot_cross_h2": 0, "dot_self_h4": 0, "dot_self_h2": 0, "head_sum": 19, "head_mean": 19,
                "head_max": 19, "memdot": 2}


@pytest.mark.parametrize("kind", sorted(MODULE_SEEDS))
def test_module_matches_double_at_forty_rows(kind, gpu, monkeypatch):
    from dualmessagepassing_amd import attn, mem
    (net, inputs, call), ref, (rows, window) = double_run(kind, MODULE_SEEDS[kind], monkeypatch)
    assert rows > 0 and window == 0, "%s: %d of %d sparsemax rows of the double run have a key in the window (choose another seed)" % (
        kind, window, rows)

    def no(*a, **k):
        raise AssertionError("a tensor-op path ran where the HIP kernels should")
    with monkeypatch.context() as m:
        m.setattr(attn, "attention_tensor", no)
        m.setattr(mem, "memory_tensor", no)
        got = run_module(net, inputs, call, gpu, th.float32, ref[3])
        th.cuda.synchronize()
    worst = {}
    for name, tol, a, b in ([("out %d" % i, 1e-4, x, y) for i, (x, y) in enumerate(zip(got[0], ref[0]))]
                            + [("input grad %d" % i, 2e-4, x, y) for i, (x, y) in enumerate(zip(got[1], ref[1]))]
                            + [("grad " + k, 2e-4, got[2][k], ref[2][k]) for k in ref[2]]):
        assert (a is None) == (b is None), name
        if b is None:
            continue
        err = U._err(a, b.detach())
        worst[name.split()[0]] = max(worst.get(name.split()[0], 0.0), err)
        assert err <= tol, "%s %s: err %g > %g" % (kind, name, err, tol)
    print("%s: %d sparsemax rows, none with a window key; worst err %s" % (kind, rows, " ".join("%s %.2e" % kv for kv in sorted(worst.items()))))
