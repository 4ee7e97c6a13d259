"""``txl.rel_attention`` on the kernels of csrc/dmp_txl.hip against an fp64 restatement of the reference's attention
(models/txl.py:95-177 without a mask), over the edge shapes of the unmasked ``rel_shift``, the admitted maxima, ragged sizes
between them (q and k no multiple of the kernels' 16 x 16 ownership, of 4, of 32 or of 64) and scores beyond the range of
``expf``.

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
    # ragged sizes: a thread's 4 x 8 entries partly inside the tile, a partial second softmax half, the remainders of the
    # tile products, the row pair of the 32-wide chunk at q % 32 != 0
    (3, 17, 17, 2, 16),      # q = k one past a 16-block, m = 0
    (2, 16, 17, 1, 32),      # m = 1, k % 4 = 1
    (3, 37, 101, 2, 32),     # partial second softmax half, two rows per thread with q % 32 = 5
    (2, 63, 127, 1, 64),     # one short of both maxima, k % 4 = 3, two head-width chunks
    (2, 33, 97, 4, 128),     # four chunks, row 32 alone in the second row slot
    (2, 20, 128, 1, 16),     # m = 108 > q: most of a row comes from the wrap
    (2, 64, 65, 2, 16),      # the second softmax half holds one lane
    (2, 49, 49, 1, 64),      # a lone segment shorter than 64
    (70, 37, 101, 4, 32),    # more sequences than backward workgroups per head (64) at a ragged shape: the tiles' padding
                             # still holds the previous sequence
]
OVERFLOW = 89.0              # expf of a larger float32 is inf: a softmax without the row-maximum shift overflows


def scores_fp64(q, k, r, bw, br, scale):
    """The scaled scores [N, q, k, nh] in double, the reference's rel_shift by pad and reshape."""
    q, k, r, bw, br = (t.double() for t in (q, k, r, bw, br))
    N, ql, nh, dh = q.shape
    kl = k.size(1)
    ac = th.einsum("bind,bjnd->bijn", q + bw, k)
    bd = th.einsum("bind,jnd->bijn", q + br, r)
    bd = th.cat([bd.new_zeros(N, ql, 1, nh), bd], dim=2).view(N, kl + 1, ql, nh)[:, 1:].reshape(N, ql, kl, nh)
    return (ac + bd) * scale


def attention_fp64(q, k, v, r, bw, br, scale):
    """The reference's computation in double."""
    N, ql, nh, dh = q.shape
    p = th.softmax(scores_fp64(q, k, r, bw, br, scale), dim=2)
    return th.einsum("bijn,bjnd->bind", p, v.double()).reshape(N, ql, nh * dh)


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


def _against_fp64(args, scale, tag):
    """The kernels and the fp32 tensor ops against fp64: the output and all six gradients under the band."""
    from dualmessagepassing_amd import txl
    N, q = args[0].shape[:2]
    w = th.randn(N, q, args[0].size(2) * args[0].size(3), generator=th.Generator().manual_seed(3)).to(DEV)
    assert txl.kernel_ok(*[a.to(DEV) for a in args])
    got = _run(lambda *x: txl.rel_attention(*x, scale), args, w)
    yard = _run(lambda *x: txl.rel_attention_tensor(*x, scale), args, w)
    ref = _run(lambda *x: attention_fp64(*x, scale), args, w, th.float64)
    within_band(got[0], ref[0], yard[0], 1e-5, "o %s" % (tag,))
    for name, a, b, c in zip(NAMES, got[1:], ref[1:], yard[1:]):
        assert a.shape == b.shape
        within_band(a, b, c, 1e-4, "d%s %s" % (name, tag))


@pytest.mark.parametrize("N,q,k,nh,dh", SHAPES)
def test_rel_attention_against_fp64(N, q, k, nh, dh):
    _against_fp64(_inputs(N, q, k, nh, dh, seed=N * 1000 + q * 10 + k), dh ** -0.5, (N, q, k, nh, dh))


def test_scores_beyond_the_range_of_expf_against_fp64():
    """The queries times 30 at a ragged shape.  Condition (asserted, in double): at least half of the (sequence, head, row)
    softmax rows have a largest scaled score above 89, where expf overflows unless the row maximum is taken off first -- in
    the forward, and in the backward that recomputes P from the stored maximum.  Same band as every other case; every output
    and gradient finite (``within_band`` asserts it)."""
    N, q, k, nh, dh = 2, 37, 101, 2, 32
    args = _inputs(N, q, k, nh, dh, seed=N * 1000 + q * 10 + k)
    args[0] = args[0] * 30.0
    scale = dh ** -0.5
    top = scores_fp64(args[0], args[1], *args[3:], scale).amax(dim=2)           # [N, q, nh]
    share = float((top > OVERFLOW).double().mean())
    print("TXLOVERFLOW rows above %g: %.3f of %d, largest score %.1f" % (OVERFLOW, share, top.numel(), float(top.max())))
    assert share >= 0.5, share
    _against_fp64(args, scale, "30 q " + str((N, q, k, nh, dh)))


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
