"""``gatememo``: where the index arrays derived from a 0 / 1 gate hang and when they are stale -- the owner rule, the flags and the
memo, on plain CPU tensors.  (The gates are the ScalarFilter gates of SubgraphCountingMatching/models/basemodel.py:1515-1531.)"""
import weakref

import torch as th

from dualmessagepassing_amd import gatememo as gm


def _counting(value):
    calls = []

    def build():
        calls.append(1)
        return value() if callable(value) else value
    return build, calls


def test_owner_is_the_base_of_a_whole_view_only():
    g = th.ones(8)
    assert gm.owner(g) is g
    assert gm.owner(g.view(-1, 1)) is g
    assert gm.owner(g.reshape(-1)) is g
    part = g[:4]                               # same address, fewer elements: it says something else than its base
    assert gm.owner(part) is part
    assert gm.owner(g[4:]) is not g
    box = object()
    assert gm.owner(box) is box


def test_hit_and_miss():
    g, k1, k2 = th.ones(8), object(), object()
    build, calls = _counting(lambda: [len(calls)])
    a = gm.memo(g, "x", (k1,), build)
    assert gm.memo(g, "x", (k1,), build) is a and len(calls) == 1
    assert gm.peek(g, "x", (k1,)) is a and gm.peek(g, "x", (k2,)) is None and gm.peek(g, "x") is None and gm.peek(g, "y", (k1,)) is None
    # another key object under the same name: rebuilt, and the entry replaced
    b = gm.memo(g, "x", (k2,), build)
    assert b is not a and len(calls) == 2
    assert gm.peek(g, "x", (k1,)) is None and gm.peek(g, "x", (k2,)) is b
    # keys are compared by identity, not by value
    t1, t2 = th.zeros(3), th.zeros(3)
    c = gm.memo(g, "t", (t1,), build)
    assert gm.memo(g, "t", (t2,), build) is not c and len(calls) == 4
    # a tuple name: two entries of a kind side by side
    p, q = gm.memo(g, ("rows", 0, 8), (), build), gm.memo(g, ("rows", 0, 4), (), build)
    assert gm.peek(g, ("rows", 0, 8)) is p and gm.peek(g, ("rows", 0, 4)) is q and p is not q
    # a new version of the holder: every entry is gone, whatever its name
    other = gm.memo(g, "other", (), build)
    n = len(calls)
    g.mul_(1)
    assert gm.peek(g, "other") is None and gm.peek(g, "x", (k2,)) is None and gm.peek(g, ("rows", 0, 8)) is None
    assert gm.memo(g, "x", (k2,), build) is not b and len(calls) == n + 1
    assert gm.peek(g, "other") is None and other is not None
    # ``plant``: a value built elsewhere lands where ``memo`` finds it
    v = [7]
    assert gm.plant(g, "planted", (k1,), v) is v and gm.memo(g, "planted", (k1,), build) is v and len(calls) == n + 1


def test_a_built_none_is_a_value_like_any_other():
    g = th.ones(8)
    build, calls = _counting(None)
    assert gm.memo(g, "n", (), build) is None and gm.memo(g, "n", (), build) is None and len(calls) == 1


def test_views_share_the_memo():
    g = th.ones(8)
    build, calls = _counting(lambda: [1])
    a = gm.memo(g.view(-1, 1), "x", (), build)
    assert gm.memo(g.reshape(-1), "x", (), build) is a and gm.peek(g, "x") is a and len(calls) == 1
    assert gm.peek(g[:4], "x") is None          # a slice has a memo of its own


def test_flags():
    g = th.ones(8)
    assert not gm.flag(g, "binary") and gm.flag(g, "ones_prefix") == 0 and not gm.skips_rows(g)
    gm.mark(g, binary=True, ones_prefix=3)
    assert gm.flag(g.view(-1, 1), "binary") and gm.flag(g.reshape(-1), "ones_prefix") == 3 and not gm.flag(g, "zero_rows")
    assert not gm.flag(g[:4], "binary")
    assert gm.skips_rows(g) and gm.skips_rows(g.view(-1, 1)) and not gm.skips_rows(g[:4])
    gm.mark(g.view(-1, 1), zero_rows=True)      # marked through a whole view: on the owner, the earlier marks stay
    assert gm.flag(g, "zero_rows") and gm.flag(g, "binary")
    g.mul_(1)                                   # flags are statements of the gate's maker: a new version keeps them
    assert gm.flag(g, "binary")
    gm.mark(g, dense=True)
    assert gm.flag(g, "binary") and not gm.skips_rows(g)


def test_no_entry_keeps_its_holder_alive():
    g, key = th.ones(8), th.zeros(2)
    gm.mark(g, binary=True)
    gm.memo(g.view(-1, 1), ("x", 1), (key,), lambda: (th.zeros(4), key))
    ref = weakref.ref(g)
    del g
    assert ref() is None                         # (no gc.collect(): freed by its reference count)


def test_a_holder_that_refuses_attributes_gets_the_value_built_every_time():
    class Slotted:
        __slots__ = ()

    h = Slotted()
    build, calls = _counting(lambda: [1])
    a, b = gm.memo(h, "x", (), build), gm.memo(h, "x", (), build)
    assert a == [1] and b == [1] and a is not b and len(calls) == 2 and gm.peek(h, "x") is None
