"""The "ladder" operands of tests/bf16x6_cases.py, proved on the CPU (numpy only): values x = h + m + l whose bf16 split (round to
nearest even, as ``split_pair`` of csrc/dmp_mfma_common.h makes it) is exactly (h, m, l), so that each of the six piece products of
``mfma_x6`` is individually and deterministically visible in a product x y:

  (a) the values are exact in fp32 and the emulated split returns (h, m, l) -- with a power-of-two factor and a sign as well;
  (b) the emulated six-product sum, accumulated in fp32 in ``mfma_x6``'s order, is within 2^-21 |x y| of the fp64 product;
  (c) with any ONE of the six products left out EVERY pair is off by at least 4 x 2^-21 |x y|: a GPU test that holds a kernel to
      2^-21 on these operands cannot pass with a piece product missing, doubled in another's place or read from a wrong slot.

2^-21 is derived: the three dropped second-order products are at most 2^-24 of |x y| together, the accumulator takes a few fp32
roundings (2^-24 each), and a factor 4 is left for the matrix unit's internal order of accumulation."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bf16x6_cases import LADDER_BOUND, ladder  # noqa: E402

PAIRS = 200000
# mfma_x6's order (csrc/dmp_mfma_common.h): (piece of a, piece of b), the small terms first
ORDER = (("lo", "hi"), ("hi", "lo"), ("mid", "mid"), ("mid", "hi"), ("hi", "mid"), ("hi", "hi"))


def bf16_rne(x):
    """fp32 -> the nearest bf16 value (ties to even), as fp32: what v_cvt_pk_bf16_f32 returns for finite values"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split(x):
    """``split_pair``: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid), the differences in fp32"""
    x = x.astype(np.float32)
    hi = bf16_rne(x)
    r = (x - hi).astype(np.float32)
    mid = bf16_rne(r)
    s = (r - mid).astype(np.float32)
    return dict(hi=hi, mid=mid, lo=bf16_rne(s))


def six_products(a, b, leave_out=None):
    """sum of the piece products in ``mfma_x6``'s order, every addition rounded to fp32 (a piece product itself is exact: 8 x 8 bits)"""
    acc = np.zeros(a["hi"].shape, np.float32)
    for i, (p, q) in enumerate(ORDER):
        if i != leave_out:
            acc = (acc + (a[p] * b[q]).astype(np.float32)).astype(np.float32)
    return acc


@pytest.fixture(scope="module")
def pairs():
    rng = np.random.default_rng(20260411)
    return ladder((PAIRS,), rng), ladder((PAIRS,), rng)


def test_the_builder_is_exact_and_the_split_returns_its_pieces(pairs):
    for x, h, m, l in pairs:
        assert x.dtype == np.float32
        assert np.array_equal(x.astype(np.float64), h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64))
        assert float(h.min()) > 1.0 and float(h.max()) < 1.25
        assert np.array_equal(np.abs(m) * 2.0 ** 16, np.round(np.abs(m) * 2.0 ** 16))
        assert float(np.abs(m).min()) >= 1.5 * 2.0 ** -9 and float(np.abs(m).max()) < 2.0 ** -8
        assert float(np.abs(l).min()) >= 1.5 * 2.0 ** -18 and float(np.abs(l).max()) < 2.0 ** -17
        for sm in (-1, 1):
            for sl in (-1, 1):
                assert bool(((np.sign(m) == sm) & (np.sign(l) == sl)).any())      # independent signs: all four combinations
        s = split(x)
        assert np.array_equal(s["hi"], h) and np.array_equal(s["mid"], m) and np.array_equal(s["lo"], l)


def test_a_power_of_two_factor_and_a_sign_leave_the_pieces_as_they_are():
    rng = np.random.default_rng(3)
    x, h, m, l = ladder((PAIRS // 2,), rng, exponents=(-100, 100), signs=True)
    assert bool((x < 0).any()) and bool((x > 0).any())
    assert float(np.abs(x).min()) < 2.0 ** -90 and float(np.abs(x).max()) > 2.0 ** 90
    assert np.array_equal(x.astype(np.float64), h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64))
    s = split(x)
    assert np.array_equal(s["hi"], h) and np.array_equal(s["mid"], m) and np.array_equal(s["lo"], l)


def test_the_six_product_sum_is_within_the_bound(pairs):
    (x, _, _, _), (y, _, _, _) = pairs
    ref = x.astype(np.float64) * y.astype(np.float64)
    got = six_products(split(x), split(y)).astype(np.float64)
    err = np.abs(got - ref) / np.abs(ref)
    print("six products: largest relative error %.3g (bound %.3g)" % (err.max(), LADDER_BOUND))
    assert LADDER_BOUND == 2.0 ** -21
    assert float(err.max()) <= LADDER_BOUND


@pytest.mark.parametrize("leave_out", range(6), ids=["%s_x_%s" % pq for pq in ORDER])
def test_every_single_omission_is_four_bounds_off_on_every_pair(leave_out, pairs):
    (x, _, _, _), (y, _, _, _) = pairs
    ref = x.astype(np.float64) * y.astype(np.float64)
    got = six_products(split(x), split(y), leave_out=leave_out).astype(np.float64)
    err = np.abs(got - ref) / np.abs(ref)
    print("without %s x %s: smallest relative error %.3g (4 x bound %.3g)" % (ORDER[leave_out] + (err.min(), 4 * LADDER_BOUND)))
    assert float(err.min()) >= 4.0 * LADDER_BOUND


def test_one_product_doubled_in_anothers_place_is_caught(pairs):
    """``mid x mid`` issued twice in place of ``hi x lo`` (the hand-copy fault of a six-MFMA sequence).  The two products overlap in
    magnitude (8.6e-6 .. 1.5e-5 against 5.8e-6 .. 9.3e-6), so where their signs agree one may stand in for the other; where the signs
    differ -- half of the pairs, the signs being independent -- the two errors add up, and every such pair is four bounds off.  A
    kernel's ladder test sees thousands of pairs per lane."""
    (x, _, _, _), (y, _, _, _) = pairs
    a, b = split(x), split(y)
    ref = x.astype(np.float64) * y.astype(np.float64)
    got = (six_products(a, b, leave_out=1) + (a["mid"] * b["mid"]).astype(np.float32)).astype(np.float64)
    err = np.abs(got - ref) / np.abs(ref)
    differ = np.sign(a["mid"] * b["mid"]) != np.sign(b["lo"])
    assert 0.45 * PAIRS < int(differ.sum()) < 0.55 * PAIRS
    assert float(err[differ].min()) >= 4.0 * LADDER_BOUND
    print("mid x mid in place of hi x lo: %.1f %% of all pairs four bounds off" % (100.0 * float((err >= 4.0 * LADDER_BOUND).mean())))
