"""The float64 restatement of AdamW (``util_fp64_adamw``) against the authority, ``torch.optim.AdamW`` on float64 CPU parameters:
three tensors whose gradients come and go (``grad = None``), a changed learning rate, AMSGrad on and off, weight decay 0 and
0.1, two pairs of betas.  Parameters, moments and step counts after EVERY step, to 1e-13 relative (both sides round in double,
in a different order).  Plus the conditions on the gradients that ``test_gpu_adamw_fp64.py`` relies on."""
import pytest
import torch as th

import util_fp64_adamw as UA

SIZES = (5, 130, 9)
# which tensors have a gradient at each step: tensor 1 joins at the third step, each tensor sits out three of the nine
LIVE_AT = [(0,), (0, 2), (0, 1, 2), (0, 1), (1, 2), (0, 1, 2), (2,), (0, 1, 2), (1,)]
REL = 1e-13


def _rel(a, ref, floor=None):
    """max over the elements of |a - ref| / max(|ref|, floor)."""
    den = ref.abs() if floor is None else th.maximum(ref.abs(), floor)
    err = (a - ref).abs()
    ok = err <= REL * den
    return bool(ok.all()), float((err / den.clamp_min(1e-300)).max())


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9)])
@pytest.mark.parametrize("weight_decay", [0.0, 0.1])
@pytest.mark.parametrize("amsgrad", [False, True])
def test_restatement_and_bookkeeper_reproduce_torch_adamw_in_double(amsgrad, weight_decay, betas):
    lr, eps = 3e-3, 1e-8
    ps = [th.nn.Parameter(UA.parameter(n, 3 + i).double()) for i, n in enumerate(SIZES)]
    opt = th.optim.AdamW(ps, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, foreach=False)
    book = UA.Bookkeeper(len(SIZES))
    mine = [dict(p=p.detach().clone(), m=th.zeros_like(p), v=th.zeros_like(p), vmax=th.zeros_like(p) if amsgrad else None)
            for p in ps]
    for it, live in enumerate(LIVE_AT):
        if it == 4:
            lr = 1e-3
            opt.param_groups[0]["lr"] = lr
        grads = {}
        for i, p in enumerate(ps):
            p.grad = None
            if i in live:
                grads[i] = UA.gradient(SIZES[i], 17 + i, it, spike=it == 2).double()
                p.grad = grads[i].clone()
        opt.step()
        counts = book.advance(live)
        for i, (p, s) in enumerate(zip(ps, mine)):
            if counts[i]:
                s["m"], s["v"], s["vmax"] = UA.moments(s["m"], s["v"], s["vmax"], grads[i], *betas)
                s["p"] = UA.update(s["p"], s["m"], s["vmax"] if amsgrad else s["v"], lr, betas[0], betas[1], eps, weight_decay,
                                   counts[i])
            st = opt.state[p]
            assert (int(st["step"]) if st else 0) == book.steps[i], (it, i)
            ok, worst = _rel(s["p"], p.detach())
            assert ok, ("parameter", it, i, worst)
            if st:
                g_last = grads[i].abs() if i in grads else None
                ok, worst = _rel(s["m"], st["exp_avg"], floor=g_last)          # m' cancels: measured against max(|m'|, |g|)
                assert ok, ("exp_avg", it, i, worst)
                ok, worst = _rel(s["v"], st["exp_avg_sq"])
                assert ok, ("exp_avg_sq", it, i, worst)
                assert ("max_exp_avg_sq" in st) == amsgrad
                if amsgrad:
                    ok, worst = _rel(s["vmax"], st["max_exp_avg_sq"])
                    assert ok, ("max_exp_avg_sq", it, i, worst)
    assert book.steps == [6, 6, 6] and book.taken == 9


def test_update_takes_one_count_per_element():
    """``update`` with a tensor of counts is ``update`` with each count on its elements (a flat buffer of several tensors)."""
    n = 12
    p, g = UA.parameter(n, 1), UA.gradient(n, 1, 0)
    m, v, _ = UA.moments(th.zeros(n), th.zeros(n), None, g, 0.9, 0.99)
    steps = th.tensor([1] * 4 + [3] * 4 + [100000] * 4)
    both = UA.update(p, m, v, 3e-3, 0.9, 0.99, 1e-8, 1e-2, steps)
    for k in (1, 3, 100000):
        sel = steps == k
        assert th.equal(both[sel], UA.update(p[sel], m[sel], v[sel], 3e-3, 0.9, 0.99, 1e-8, 1e-2, k))
    # at step 100,000 both corrections are exactly 1 in double: beta^step underflows
    assert 0.9 ** 100000 == 0.0 and 0.99 ** 100000 == 0.0


def test_bookkeeper_shared_count_and_veto_word():
    """One shared count (a flat buffer without per-tensor counts): a tensor that joins late is updated at the buffer's count.
    A vetoed step advances no count; the veto word's four entries."""
    shared, own = UA.Bookkeeper(3, shared=True), UA.Bookkeeper(3)
    assert shared.advance((0,)) == [1, 0, 0] and own.advance((0,)) == [1, 0, 0]
    assert shared.advance((0, 2)) == [2, 0, 2] and own.advance((0, 2)) == [2, 0, 1]
    assert shared.advance(()) == [0, 0, 0] and shared.taken == 3          # a step without a live tensor is still a step
    g = UA.Bookkeeper(2, start=7)
    assert g.advance(None, flags=6, mask=2) == [0, 0] and g.word == [0, 6, 1, 1] and g.taken == 7
    assert g.advance(None, flags=2, mask=2) == [0, 0] and g.word == [0, 6, 1, 2]
    assert g.advance((1,), flags=5, mask=2) == [0, 8] and g.word == [0, 7, 0, 2] and g.taken == 8 and g.steps == [7, 8]
    assert g.advance(None, flags=0, mask=2) == [8, 9] and g.word == [0, 7, 0, 2]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025])
def test_gradients_of_the_gpu_cases(n):
    """What the GPU cases rely on: classes fixed over the steps, both signs and exact zeros present once the tensor is large
    enough, nothing non-zero below 5e-13 (so g^2 >= 2.5e-25 and v' >= (1 - beta2) g^2 >= 2.5e-27 are normal fp32 numbers), and
    -- the point of the 1e-8 and 1e-6 classes -- at step 1 sqrt(v') / sqrt(bc2) within a factor 10 of eps, for eps = 1e-8 on the
    1e-8 elements and for eps = 1e-6 on the 1e-6 elements; otherwise the placement of eps is not being tested."""
    cls = UA.grad_classes(n, n)
    for it in range(8):
        g = UA.gradient(n, n, it, spike=it == 2)
        assert g.dtype == th.float32 and bool(((g == 0) == (cls == 0)).all())
        nz = g[g != 0].abs().double()
        assert nz.numel() == 0 or float(nz.min()) >= 5e-13
        mag = th.tensor(UA.MAGNITUDES, dtype=th.float64)[cls] * (10.0 if it == 2 else 1.0)
        assert bool((g.abs().double() >= 0.5 * mag * (1 - 1e-6)).all()) and bool((g.abs().double() <= 1.5 * mag * (1 + 1e-6)).all())
    if n >= 1023:
        g = UA.gradient(n, n, 0)
        assert bool((g > 0).any()) and bool((g < 0).any()) and bool((g == 0).any())
        assert sorted(set(cls.tolist())) == list(range(len(UA.MAGNITUDES)))
        for magnitude, eps, beta2 in ((1e-8, 1e-8, 0.99), (1e-6, 1e-6, 0.9)):
            lo, hi = UA.near_eps(g, cls, magnitude, eps, beta2)
            assert 0.1 <= lo and hi <= 10.0, (magnitude, lo, hi)
