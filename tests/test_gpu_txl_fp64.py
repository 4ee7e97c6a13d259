"""``txl.rel_attention`` on the kernels of csrc/dmp_txl.hip against an fp64 restatement of the reference's attention
(models/txl.py:95-177 without a mask), over the edge shapes of the unmasked ``rel_shift`` and the admitted sizes.

Yardstick (``util_fp64.within_band``): the project's figures -- forward 1e-5, gradients 1e-4 of the array's scale -- or four
times the distance of the fp32 tensor-op path from the same fp64 result.  Every output and all six gradients are checked;
``dR`` and the two bias gradients, which the kernels reduce over the sequences, also against per-sequence launches summed
by hand."""
import pytest
import torch as th

from util_fp64 import within_band

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("q", "k", "v", "r", "r_w_bias", "r_r_bias")

SHAPES = [
    (1, 1, 1, 1, 16),        # one entry: shift(BD)[0, 0] = BD[0, 0]
    (3, 2, 2, 1, 16),        # the zero diagonal only
    (3, 3, 3, 2, 16),        # the first wrapped entry: S[0, 2] takes BD[1, 0]
    (5, 4, 8, 4, 32),
    (2, 5, 7, 1, 64),        # m neither 0 nor q
    (3, 64, 64, 4, 32),
    (2, 64, 128, 1, 128),    # the driver's default with a full memory
    (130, 8, 8, 4, 16),      # more sequences than backward workgroups per head
]


def attention_fp64(q, k, v, r, bw, br, scale):
    """The reference's computation in double, its rel_shift by pad and reshape."""
    q, k, v, r, bw, br = (t.double() for t in (q, k, v, r, bw, br))
    N, ql, nh, dh = q.shape
    kl = k.size(1)
    ac = th.einsum("bind,bjnd->bijn", q + bw, k)
    bd = th.einsum("bind,jnd->bijn", q + br, r)
    bd = th.cat([bd.new_zeros(N, ql, 1, nh), bd], dim=2).view(N, kl + 1, ql, nh)[:, 1:].reshape(N, ql, kl, nh)
    p = th.softmax((ac + bd) * scale, dim=2)
    return th.einsum("bijn,bjnd->bind", p, v).reshape(N, ql, nh * dh)


def _inputs(N, q, k, nh, dh, seed):
    """Unit-variance rows and biases of 0.5: scores of standard deviation about 1.5 at scale 1 / sqrt(dh) -- a softmax that
    is neither flat nor one-hot."""
    g = th.Generator().manual_seed(seed)
    return [th.randn(N, q, nh, dh, generator=g), th.randn(N, k, nh, dh, generator=g), th.randn(N, k, nh, dh, generator=g),
            th.randn(k, nh, dh, generator=g), 0.5 * th.randn(nh, dh, generator=g), 0.5 * th.randn(nh, dh, generator=g)]


def _run(fn, args, w, dtype=th.float32):
    xs = [a.to(DEV, dtype).requires_grad_(True) for a in args]
    o = fn(*xs)
    (o * w.to(dtype)).sum().backward()
    return [o.detach()] + [x.grad for x in xs]


@pytest.mark.parametrize("N,q,k,nh,dh", SHAPES)
def test_rel_attention_against_fp64(N, q, k, nh, dh):
    from dualmessagepassing_amd import txl
    args = _inputs(N, q, k, nh, dh, seed=N * 1000 + q * 10 + k)
    scale = dh ** -0.5
    w = th.randn(N, q, nh * dh, generator=th.Generator().manual_seed(3)).to(DEV)
    assert txl.kernel_ok(*[a.to(DEV) for a in args])
    got = _run(lambda *x: txl.rel_attention(*x, scale), args, w)
    yard = _run(lambda *x: txl.rel_attention_tensor(*x, scale), args, w)
    ref = _run(lambda *x: attention_fp64(*x, scale), args, w, th.float64)
    within_band(got[0], ref[0], yard[0], 1e-5, "o %s" % ((N, q, k, nh, dh),))
    for name, a, b, c in zip(NAMES, got[1:], ref[1:], yard[1:]):
        assert a.shape == b.shape
        within_band(a, b, c, 1e-4, "d%s %s" % (name, (N, q, k, nh, dh)))


def test_the_softmax_of_the_test_inputs_is_neither_flat_nor_one_hot():
    q, k, v, r, bw, br = (t.double() for t in _inputs(2, 64, 128, 1, 128, seed=1))
    ac = th.einsum("bind,bjnd->bijn", q + bw, k) * 128 ** -0.5
    p = th.softmax(ac, dim=2)
    assert 3.0 / 128 < float(p.max(dim=2).values.mean()) < 0.7


def test_reduced_gradients_equal_single_sequence_launches_summed_by_hand():
    """dR, d r_w_bias and d r_r_bias of N = 5 sequences against the five N = 1 launches summed in double.  Bound: the kernels'
    fixed-order sum makes N - 1 fp32 additions per element, each within 2^-24 of the running sum, which the sum of the
    terms' magnitudes bounds."""
    from dualmessagepassing_amd import txl
    N, q, k, nh, dh = 5, 4, 8, 4, 32
    args = _inputs(N, q, k, nh, dh, seed=11)
    scale = dh ** -0.5
    w = th.randn(N, q, nh * dh, generator=th.Generator().manual_seed(3)).to(DEV)
    full = _run(lambda *x: txl.rel_attention(*x, scale), args, w)
    singles = []
    for n in range(N):
        one = [a[n:n + 1] for a in args[:3]] + args[3:]
        singles.append(_run(lambda *x: txl.rel_attention(*x, scale), one, w[n:n + 1]))
    for idx in (4, 5, 6):                 # r, r_w_bias, r_r_bias
        terms = th.stack([s[idx].double() for s in singles])
        bound = (N - 1) * 2.0 ** -24 * 1.001 * terms.abs().sum(0)
        err = (full[idx].double() - terms.sum(0)).abs()
        assert bool((err <= bound + 1e-30).all()), (NAMES[idx - 1], float(err.max()), float(bound.max()))
    for idx in (0, 1, 2, 3):              # o, dq, dk, dv: per sequence, the same bits
        assert th.equal(full[idx], th.cat([s[idx] for s in singles])), idx
