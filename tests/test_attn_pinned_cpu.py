"""tests/util_fp64_attn.py without a GPU: the fp64 restatement, the condition on the sweep's inputs, and the stand-in
experiment that shows what pinning the support buys.

Stand-in: the fp32 tensor route (``attn.attention_tensor`` in float on the CPU) plays the kernel; its support sizes are
read off its own sparsemax.  It passes exactly what tests/test_gpu_attn_fp64.py asserts of the kernels
(``check_outputs``).  Then one row's size is moved by one:

* outside the window (a row whose window is empty): ``admissible`` refuses it;
* inside the window (the row's one window key joins or leaves the support; the stand-in then computes on that piece, as
  a kernel whose rounding decided the key the other way would): accepted, and every output stays within the strict
  figures of the pinned reference.  Measured at case (Lq 130, Lk 70, dh 4, nh 3), row (b 0, i 34, h 2), support size 4,
  whose window key is inside fp64's support and leaves it: against fp64's own support tau 2.25e-5, O 3.66e-4,
  dQ 7.38e-2, dK 2.70e-2, dV 1.17e-4 (dQ and dK hundreds of times over 1e-4, and tau and O over 1e-5 as well: the window
  is as wide as _case's exclusion rule, not as narrow as fp32 rounding); against the pinned reference tau 9.27e-8,
  O 4.67e-7, dQ 1.04e-7, dK 5.67e-8, dV 1.51e-7, the figures of the unmoved run.
Both negatives were tried against a broken checker: with ``reference`` ignoring ``supp`` the inside-the-window test fails
on its pinned comparison with the unpinned figures above; with ``admissible`` answering True everywhere the
outside-the-window test fails because the refusal it expects is not the one raised."""
import pytest
import torch as th

import util_fp64_attn as U
from dualmessagepassing_amd import attn

EXPERIMENT = (130, 70, 4, 3)


def _sized(x, dim, force):
    """``attn.sparsemax`` with the support size of the rows where ``force`` > 0 set to it, unclamped on the support."""
    x = x.transpose(dim, -1)
    z = x - x.max(dim=-1, keepdim=True)[0]
    zs, order = th.sort(z, dim=-1, descending=True, stable=True)
    k = th.arange(1, z.size(-1) + 1, dtype=z.dtype)
    cs = zs.cumsum(dim=-1)
    size = (1.0 + k * zs > cs).sum(dim=-1, keepdim=True)
    size = th.where(force.unsqueeze(-1) > 0, force.unsqueeze(-1), size)
    tau = (cs.gather(-1, size - 1) - 1.0) / size.to(z.dtype)
    rank = th.empty_like(order).scatter_(-1, order, th.arange(z.size(-1)).expand_as(order).contiguous())
    return th.where(rank < size, z - tau, th.zeros((), dtype=z.dtype)).transpose(dim, -1), size.squeeze(-1)


def _standin(case, monkeypatch, force=None):
    """(o, tau, supp, dq, dk, dv) of the fp32 tensor route; ``force`` [B, Lq, nh]: support sizes to impose where > 0."""
    seen = {}
    orig = attn.sparsemax

    def spy(x, dim=-1):
        if force is None:
            p = orig(x, dim)
            size = (p > 0).sum(dim=dim)
        else:
            p, size = _sized(x, dim, force)
        seen["s"], seen["size"] = x.detach(), size
        return p
    q, k, v = (x.float().requires_grad_(True) for x in (case.q, case.k, case.v))
    with monkeypatch.context() as m:
        m.setattr(attn, "sparsemax", spy)
        o = attn.attention_tensor(q, k, v, case.qm, case.km, case.nh, case.scale)
    o.backward(case.dout.float())
    rows = case.win.rows
    supp = th.where(rows, seen["size"], th.zeros((), dtype=th.int64))
    zs = th.sort(seen["s"], dim=2, descending=True)[0]
    top = th.arange(zs.size(2)).view(1, 1, -1, 1) < supp.unsqueeze(2)
    tau = th.where(rows, ((zs * top).sum(dim=2) - 1.0) / supp.clamp_min(1).float(), th.zeros(()))
    return o, tau, supp.int(), q.grad, k.grad, v.grad


def test_sweep_is_the_kernels_widths():
    assert U.DHS == attn.KERNEL_DH


@pytest.mark.parametrize("key", [(17, 3, 4, 3), (40, 70, 16, 3), (130, 2049, 8, 1)], ids=str)
def test_reference_is_the_tensor_route_in_double(key):
    c = U.sweep_case(*key)
    ref = U.reference(c.q, c.k, c.v, c.qm, c.km, c.nh, c.scale, c.dout)
    q, k, v = (x.clone().requires_grad_(True) for x in (c.q, c.k, c.v))
    o = attn.attention_tensor(q, k, v, c.qm, c.km, c.nh, c.scale)
    o.backward(c.dout)
    for got, want, what in ((ref.o, o.detach(), "O"), (ref.dq, q.grad, "dQ"), (ref.dk, k.grad, "dK"), (ref.dv, v.grad, "dV")):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), what
    assert th.equal(ref.c, c.win.c64)
    assert float((ref.tau - c.win.tau64).abs().max()) <= 1e-12 * max(1.0, float(ref.tau.abs().max()))
    # the restated special rows: masked queries and the all-masked pair
    assert int(ref.c[~c.qm].abs().max()) == 0 and int(ref.c[1].abs().max()) == 0
    assert bool((ref.c[0][c.qm[0]] > 0).all())


@pytest.mark.parametrize("B,Lq", [(0, 5), (3, 0), (0, 0)])
def test_tensor_route_takes_empty_shapes(B, Lq):
    q, k, v = (th.randn(B, L, 32, requires_grad=True) for L in (Lq, 6, 6))
    o = attn.sparsemax_attention(q, k, v, th.ones(B, Lq, dtype=th.bool), th.ones(B, 6, dtype=th.bool), 4, 0.5)
    o.sum().backward()
    assert o.shape == q.shape and all(t.grad.shape == t.shape and not t.grad.abs().sum() for t in (q, k, v))


def test_window_condition_holds_over_the_sweep():
    """No window with more than one key, window rows at most 10 % of a case and 1 % of the sweep: from fp64 alone.  The
    tied key rows sit inside the support, all three together, in some row of every case."""
    rows = window = 0
    for key in U.SWEEP:
        case = U.sweep_case(*key)
        nwin, n = U.case_conditions(case, str(key))
        rows, window = rows + n, window + nwin
        src, copies = U.tied_keys(key[1])
        live = [b for b in range(case.k.size(0)) if b != 1 and (key[1] > 3 or b == 0)]      # the pairs with both copies
        assert all(th.equal(case.k[b, j], case.k[b, src]) for j in copies for b in live), key
        S64 = U._analyse(case.q[live], case.k[live], case.qm[live], case.km[live], case.nh, case.scale)[3]
        assert bool(S64[:, :, src].any()) and all(th.equal(S64[:, :, j], S64[:, :, src]) for j in copies), key
    print("sweep: %d of %d rows with a key in the window" % (window, rows))
    assert window <= U.SWEEP_CAP * rows, (window, rows)
    assert window > 0                                      # the pin has work to do
    masked = {Lq: U.masked_query_rows(Lq) for Lq in U.LQS}
    assert masked[16] == [11] and masked[17] == [11] and all(len(masked[Lq]) == (Lq - 2) // 8 for Lq in (40, 130))


@pytest.mark.parametrize("key", [(16, 3, 8, 1), (17, 70, 32, 3), (40, 2049, 4, 3), EXPERIMENT], ids=str)
def test_fp32_stand_in_passes_the_gpu_assertions(key, monkeypatch):
    U.check_outputs(_standin(U.sweep_case(*key), monkeypatch), U.sweep_case(*key), "stand-in %s" % (key,))


def test_a_size_moved_outside_the_window_is_refused(monkeypatch):
    case = U.sweep_case(*EXPERIMENT)
    got = list(_standin(case, monkeypatch))
    b, i, h = ((case.win.nW == 0) & case.win.rows & (case.win.c64 > 1)).nonzero()[7].tolist()
    for step in (1, -1):
        moved = got[2].clone()
        moved[b, i, h] += step
        with pytest.raises(AssertionError, match="support size fp64 does not admit"):
            U.check_outputs(got[:2] + [moved] + got[3:], case, "moved by %d" % step)


def test_a_size_moved_inside_the_window_needs_the_pin(monkeypatch):
    case = U.sweep_case(*EXPERIMENT)
    win = case.win
    b, i, h = (win.nW > 0).nonzero()[0].tolist()
    print("row (b %d, i %d, h %d): c64 %d, window key %s the support" % (b, i, h, int(win.c64[b, i, h]), "in" if int(win.nWin[b, i, h]) else "outside"))
    plain = _standin(case, monkeypatch)
    assert int(plain[2][b, i, h]) == int(win.c64[b, i, h])           # fp32 on its own decides this row as fp64 does
    force = th.zeros_like(win.c64)
    force[b, i, h] = win.c64[b, i, h] + (-1 if int(win.nWin[b, i, h]) else 1)
    got = _standin(case, monkeypatch, force)
    assert int(got[2][b, i, h]) == int(force[b, i, h]) and int((got[2] != plain[2]).sum()) == 1
    fig = U.check_outputs(got, case, "moved inside the window, pinned")
    assert fig["differ"] == 1
    loose = U.errors(got, case, pinned=False)
    print("moved inside the window, fp64's own support: " + " ".join("%s %.2e" % kv for kv in loose.items()))
    assert min(loose["dQ"], loose["dK"]) > 100 * U.TOL_GRAD, loose
    with pytest.raises(AssertionError, match="err"):
        U.check_outputs(got, case, "moved inside the window, not pinned", pinned=False)
