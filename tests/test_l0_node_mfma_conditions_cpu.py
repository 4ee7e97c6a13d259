"""``fused.l0_node_mfma_ok``: when the first layer's node side runs as one launch on the matrix pipe (csrc/dmp_l0node.hip) and when
it keeps ``l0_node_fwd``'s launch per table -- the host condition over its fallback list, on CPU tensors and stand-ins."""
import itertools
import types

import torch as th


def _rows(n, ld, ptr=0):
    """A stand-in for a [n, ld] fp32 array at address ``ptr`` (no memory behind it: the condition asks for strides and addresses)."""
    return types.SimpleNamespace(stride=lambda d: (ld, 1)[d], data_ptr=lambda: ptr, size=lambda d: (n, ld)[d])


def test_the_route_and_every_fallback():
    from dualmessagepassing_amd import fused
    N = 73728
    venc, S0 = th.zeros(64, 16), th.zeros(64, 24)
    ok = lambda **kw: fused.l0_node_mfma_ok(**dict(dict(H=128, VK=16, K0=10, Kp=12, tables=2, N=N, venc=venc, S0=S0, exact_fp32=0), **kw))
    assert ok() and ok(tables=1) and ok(VK=1, K0=1, Kp=4) and ok(VK=16, K0=12) and ok(VK=6, K0=16, Kp=16, S0=th.zeros(4, 32))
    assert not ok(H=64) and not ok(H=256)                                       # H != 128
    assert not ok(exact_fp32=1)                                                 # DMP_EXACT_FP32=1
    assert not ok(VK=16, K0=13, Kp=16, S0=th.zeros(4, 32))                      # VK + 2 K0 > L0_NODE_MAX_COLS
    assert not ok(VK=17, K0=4, Kp=4, venc=th.zeros(4, 20))                      # a block wider than a k-group
    assert not ok(VK=4, K0=17, Kp=20, S0=th.zeros(4, 40))
    assert not ok(tables=3) and not ok(tables=0)                                # more than two tables
    assert not ok(venc=None)                                                    # no node codes
    # arrays the descriptors cannot address: rows that are no whole 16 bytes, an unaligned base, a stride of 16 KiB, 4 GiB
    assert not ok(venc=th.zeros(64, 18)[:, :16]) and not ok(S0=th.zeros(64, 26)[:, :24])
    assert not ok(venc=_rows(64, 16, ptr=8)) and not ok(S0=_rows(64, 24, ptr=4))
    assert not ok(Kp=10, S0=th.zeros(64, 20)) and not ok(Kp=12, S0=th.zeros(64, 20))
    assert ok(venc=_rows(N, 4092)) and not ok(venc=_rows(N, 4096))
    big = ((1 << 32) - 65536) // (512 * 4)                                      # code rows of 2 KiB
    assert ok(N=big - 1, venc=_rows(big, 512)) and not ok(N=big, venc=_rows(big, 512))
    assert ok(N=big - 1, S0=_rows(big, 512)) and not ok(N=big, S0=_rows(big, 512))
    rows_p = ((1 << 32) - 65536) // (256 * 4)                                   # the [N, 2H] projections
    assert ok(N=rows_p - 1) and not ok(N=rows_p)


def test_the_switch_takes_the_route_out():
    from dualmessagepassing_amd import fused
    venc, S0 = th.zeros(64, 16), th.zeros(64, 24)
    saved = fused.USE_L0_NODE_MFMA
    try:
        for on, (vk, k0) in itertools.product((True, False), ((16, 10), (1, 1), (16, 12))):
            fused.USE_L0_NODE_MFMA = on
            assert fused.l0_node_mfma_ok(128, vk, k0, 12, 2, 4096, venc, S0, exact_fp32=0) == on
    finally:
        fused.USE_L0_NODE_MFMA = saved
    assert fused.USE_L0_NODE_MFMA                                               # on by default
    assert fused.L0_NODE_MFMA_MAX_CODES == 16 and 16 + 2 * 12 == fused.L0_NODE_MAX_COLS


def test_the_backward_route_adds_its_gradient_rows():
    """``fused.l0_node_bwd_ok``: the forward's condition, a venc table for all rows or one per table, gradient rows of whole 8 bytes."""
    from dualmessagepassing_amd import fused
    venc, S0 = th.zeros(64, 16), th.zeros(64, 24)
    dXP, dxn = th.zeros(64, 384), th.zeros(64, 128)
    ok = lambda **kw: fused.l0_node_bwd_ok(**dict(dict(H=128, VK=16, K0=10, Kp=12, tables=2, vtables=1, N=64, venc=venc, S0=S0, dXP=dXP, dxn=dxn,
                                                       exact_fp32=0), **kw))
    assert ok() and ok(dxn=None) and ok(vtables=2) and ok(tables=1)
    assert not ok(H=64) and not ok(exact_fp32=1) and not ok(K0=13, Kp=16, S0=th.zeros(4, 32)) and not ok(tables=3) and not ok(venc=None)
    assert not ok(tables=1, vtables=2) and not ok(vtables=0) and not ok(dXP=None)
    assert not ok(dXP=th.zeros(64, 385)[:, :384]) and not ok(dxn=th.zeros(64, 129)[:, :128])          # rows of an odd number of floats
    assert not ok(dXP=th.zeros(64, 256)) and not ok(dxn=th.zeros(128, 64).t())                          # too narrow, a transposed view
    assert not ok(dXP=_rows(64, 384, ptr=4)) and not ok(dXP=_rows(64, 4096)) and ok(dXP=_rows(64, 4094))
    big = ((1 << 32) - 65536) // (384 * 4)
    assert ok(N=big - 1) and not ok(N=big)
    saved = fused.USE_L0_NODE_MFMA
    fused.USE_L0_NODE_MFMA = False
    try:
        assert not ok()
    finally:
        fused.USE_L0_NODE_MFMA = saved
