"""fp64 restatement of the sparsemax attention (csrc/dmp_attn.hip) with the support pinned per row, the inputs of the
sweep beyond one query tile, and the assertions that tests/test_gpu_attn_fp64.py and tests/test_attn_pinned_cpu.py share.
Plain torch in double on the CPU; nothing here imports the kernels.

Per row (b, i, h) with at least one live key: z_j the fp64 score, (c64, tau64, S64) the fp64 support size, threshold and
set by the sort rule of ``attn.sparsemax``, and the window W = live keys with |z_j - tau64| < 1e-4 * max(1, max_j |z_j|):
the keys that fp32 rounding may move in or out of the support (the rule of test_gpu_attn.py::_case, which masks such rows
out; here no row leaves).  sparsemax is piecewise linear in the scores and the pieces are the supports, so a computation
that decides a window key the other way is on the neighbouring piece: its outputs are continuous there (the key's weight
is within the window of 0), its gradients are not.  ``reference(..., supp=c)`` therefore takes the support as the c largest
fp64 scores and evaluates that piece's formulas unclamped; ``admissible`` bounds how c may differ from c64: by window keys
only.  With at most one key per window "the c largest" is unambiguous."""
import collections
import functools
import zlib

import torch as th

WINDOW = 1e-4
CASE_CAP, SWEEP_CAP = 0.10, 0.01          # rows with a non-empty window: share of a case's rows / of the whole sweep's
TOL_FWD, TOL_GRAD = 1e-5, 1e-4            # the project's figures (tests/test_gpu_attn.py), scale max(1, |ref|max)

Rows = collections.namedtuple("Rows", "rows c64 tau64 nW nWin")       # [B, Lq, nh] each; rows = live query, some live key
Ref = collections.namedtuple("Ref", "o tau c dq dk dv win")


def _heads(x, nh):
    return x.view(x.size(0), x.size(1), nh, x.size(2) // nh)


def _live(m, B, L):
    return th.ones(B, L, dtype=th.bool) if m is None else m.reshape(B, L) != 0


def _analyse(q, k, qmask, kmask, nh, scale):
    """-> z [B, Lq, Lk, nh] (raw scores), rank [B, Lq, Lk, nh] (0 = largest live score), W, S64 (same shape), Rows."""
    B, Lq, _ = q.shape
    Lk = k.size(1)
    z = th.einsum("bind,bjnd->bijn", _heads(q, nh), _heads(k, nh)) * scale
    klive = _live(kmask, B, Lk)
    some = klive.any(dim=1).view(B, 1, 1, 1)
    lv = klive.view(B, 1, Lk, 1)
    zm = th.where(some, z.masked_fill(~lv, float("-inf")), th.zeros(()).double())      # pairs without a live key: placeholder
    zs, order = th.sort(zm, dim=2, descending=True, stable=True)
    rank = th.empty_like(order).scatter_(2, order, th.arange(Lk).view(1, 1, Lk, 1).expand_as(order).contiguous())
    mx = zs[:, :, :1]
    zs = zs - mx
    cs = zs.cumsum(dim=2)
    kk = th.arange(1, Lk + 1, dtype=th.float64).view(1, 1, Lk, 1)
    c64 = (1.0 + kk * zs > cs).sum(dim=2)                                                # >= 1
    tau64 = ((cs.gather(2, (c64 - 1).unsqueeze(2)) - 1.0) / c64.unsqueeze(2).double() + mx).squeeze(2)
    rows = (_live(qmask, B, Lq).view(B, Lq, 1) & some.view(B, 1, 1)).expand(B, Lq, nh)
    big = th.clamp_min(z.abs().masked_fill(~lv, 0.0).amax(dim=2), 1.0)
    W = lv & rows.unsqueeze(2) & ((z - tau64.unsqueeze(2)).abs() < WINDOW * big.unsqueeze(2))
    S64 = (rank < c64.unsqueeze(2)) & rows.unsqueeze(2)
    zero = th.zeros((), dtype=th.int64)
    win = Rows(rows, th.where(rows, c64, zero), th.where(rows, tau64, th.zeros(()).double()), W.sum(dim=2), (W & S64).sum(dim=2))
    return z, rank, W, S64, win


def reference(q, k, v, qmask, kmask, nh, scale, dout, supp=None):
    """q [B, Lq, nh * dh], k / v [B, Lk, nh * dh], dout like q, all double; masks [B, L] (nonzero = live) or None;
    ``supp`` [B, Lq, nh] support sizes (None = fp64's own) -> Ref(o, tau, c, dq, dk, dv, win).  Rows with a masked query:
    zeros, c = 0; rows whose keys are all masked: 1 / Lk on every padded position, no score gradient, tau = 0, c = 0."""
    B, Lq, D = q.shape
    Lk = k.size(1)
    z, rank, _, _, win = _analyse(q, k, qmask, kmask, nh, scale)
    rows = win.rows
    c = win.c64 if supp is None else th.where(rows, supp.detach().cpu().to(th.int64), th.zeros((), dtype=th.int64))
    S = ((rank < c.unsqueeze(2)) & rows.unsqueeze(2)).double()
    cd = c.clamp_min(1).double()
    tau = th.where(rows, ((z * S).sum(dim=2) - 1.0) / cd, th.zeros(()).double())
    p = (z - tau.unsqueeze(2)) * S                                                      # not clamped: the pinned piece
    qlive = _live(qmask, B, Lq)
    uniform = qlive.view(B, Lq, 1, 1) & ~_live(kmask, B, Lk).any(dim=1).view(B, 1, 1, 1)
    p = th.where(uniform, th.full((), 1.0 / Lk, dtype=th.float64), p)
    qh, kh, vh = _heads(q, nh), _heads(k, nh), _heads(v, nh)
    o = th.einsum("bijn,bjnd->bind", p, vh).reshape(B, Lq, D)
    g = _heads(dout, nh) * qlive.view(B, Lq, 1, 1)                                      # masked query rows pass no gradient
    dp = th.einsum("bind,bjnd->bijn", g, vh)
    delta = (dp * S).sum(dim=2) / cd
    ds = (dp - delta.unsqueeze(2)) * S
    dq = scale * th.einsum("bijn,bjnd->bind", ds, kh).reshape(B, Lq, D)
    dk = scale * th.einsum("bijn,bind->bjnd", ds, qh).reshape(B, Lk, D)
    dv = th.einsum("bijn,bind->bjnd", p, g).reshape(B, Lk, D)
    return Ref(o, tau, c, dq, dk, dv, win)


def admissible(c, c64, nW, nWin):
    """The size c differs from fp64's only by keys inside the window: c64 - |W n S64| <= c <= c64 + |W \\ S64|
    (elementwise; an empty window therefore requires c == c64)."""
    return (c64 - nWin <= c) & (c <= c64 + (nW - nWin))


# ----------------------------------------------------------------------------- the sweep's inputs
LQS = (16, 17, 40, 130)      # one forward tile; one row into the second; 3 forward tiles, the last with waves 2 and 3 empty
LKS = (3, 70, 2049)          # (5 backward tiles at dh >= 16); many tiles.  Below one key step, past one, past the LDS cache
DHS = (4, 8, 16, 32, 64)     # == attn.KERNEL_DH (asserted in the tests)
NHS = (1, 3)
SWEEP = [(Lq, Lk, dh, nh) for Lk in LKS for Lq in LQS for dh in DHS for nh in NHS]
# seeds moved off the crc of the shape until the fp64 reference alone meets the window condition (case_conditions)
# and the tied keys sit inside some row's support (tests/test_attn_pinned_cpu.py::test_window_condition_holds_over_the_sweep):
# at the third the crc seed puts the three tied keys on one row's threshold (a window of 3), at the first two no support holds them
SALT = {(17, 2049, 4, 1): 1, (40, 2049, 4, 1): 1, (130, 2049, 32, 3): 1}


def batch(Lk):
    return 2 if Lk > 1000 else 3


def masked_query_rows(Lq):
    """Rows masked in every pair: one in every block of 8 rows after the first (8 = the backward rows kernel's tile at
    dh >= 16, so every later forward tile of 16 and every later backward tile of 8 or 16 holds one), at a position that
    moves through the waves; never the last row, which stays live (a block that is the last row alone has none)."""
    out = []
    for t in range(1, (Lq + 7) // 8):
        i = 8 * t + (3 * t) % 8
        if i >= Lq - 1:
            i = 8 * t
        if i < Lq - 1:
            out.append(i)
    return out


def tied_keys(Lk):
    """(source, copies): the key rows ``copies`` are bit-for-bit copies of the live key row ``source``."""
    return (1, (0, 2)) if Lk == 3 else (Lk // 2, (Lk // 2 - 1, Lk - 1))


def make_inputs(B, Lq, Lk, nh, dh, seed, qmask=True, kmask=True):
    """The generator of test_gpu_attn.py::_case (fp32-representable doubles, non-prefix key masks, pair 1 all-masked,
    masked query rows) without its near-threshold exclusion, plus: ``masked_query_rows`` and the first row of pair 0
    masked, the last row live; two key rows copied from a live third whose length is doubled (pairs 0 and 2), so that
    the three tied scores are the row's largest, inside the support, wherever they are positive; the pair's last query
    row is that key row itself.  At Lk == 3 only pair 0 carries both copies (three equal keys: uniform weights), the
    other pairs one."""
    g = th.Generator().manual_seed(seed)
    D = nh * dh
    q = th.randn(B, Lq, D, generator=g, dtype=th.float64) * 2.0
    k = th.randn(B, Lk, D, generator=g, dtype=th.float64)
    v = th.randn(B, Lk, D, generator=g, dtype=th.float64)
    km = th.rand(B, Lk, generator=g) > 0.3
    qm = th.rand(B, Lq, generator=g) > 0.2
    src, copies = tied_keys(Lk)
    if Lk > 3:
        k[:, src] *= 2.0
    for b in range(B):
        for j in copies if (Lk > 3 or b == 0) else copies[:1]:
            k[b, j] = k[b, src]
            km[b, j] = True
        if Lk > 3 or b == 0:
            q[b, -1] = k[b, src]                     # the last row (always live) looks along the tied keys
    km[:, src] = True
    if B > 1:
        km[1] = False
    qm[:, masked_query_rows(Lq)] = False
    qm[0, 0] = False
    qm[:, -1] = True
    q, k, v = q.float().double(), k.float().double(), v.float().double()
    dout = th.randn(B, Lq, D, generator=g, dtype=th.float64).float().double()
    return q, k, v, (qm if qmask else None), (km if kmask else None), 1.0 / dh ** 0.5, dout


Case = collections.namedtuple("Case", "q k v qm km nh scale dout win")


def make_case(B, Lq, Lk, nh, dh, seed, qmask=True, kmask=True):
    q, k, v, qm, km, scale, dout = make_inputs(B, Lq, Lk, nh, dh, seed, qmask, kmask)
    return Case(q, k, v, qm, km, nh, scale, dout, _analyse(q, k, qm, km, nh, scale)[4])


@functools.lru_cache(maxsize=None)
def sweep_case(Lq, Lk, dh, nh):
    key = (Lq, Lk, dh, nh)
    return make_case(batch(Lk), Lq, Lk, nh, dh, zlib.crc32(repr(key).encode()) + SALT.get(key, 0))


def case_conditions(case, what=""):
    """The condition on the inputs, from the fp64 reference alone: no window holds more than one key, rows with a
    non-empty window are at most CASE_CAP of the case's rows.  -> (window rows, rows)."""
    win = case.win
    n = int(win.rows.sum())
    assert n > 0, what
    assert int(win.nW.max()) <= 1, "%s: a window holds %d keys (choose another seed)" % (what, int(win.nW.max()))
    nwin = int((win.nW > 0).sum())
    assert nwin <= CASE_CAP * n, "%s: %d of %d rows have a key in the window (choose another seed)" % (what, nwin, n)
    return nwin, n


# ----------------------------------------------------------------------------- the assertions
def _err(got, ref):
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert not th.isnan(got).any()
    if not ref.numel():
        return 0.0
    return float((got - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def errors(got, case, pinned=True):
    """Worst error of each output of ``got`` against ``reference`` (pinned to got's support sizes, or fp64's own),
    over max(1, |ref|max)."""
    o, tau, supp, dq, dk, dv = (x.detach().cpu() for x in got)
    ref = reference(case.q, case.k, case.v, case.qm, case.km, case.nh, case.scale, case.dout, supp=supp if pinned else None)
    return {"tau": _err(tau, ref.tau), "O": _err(o, ref.o), "dQ": _err(dq, ref.dq), "dK": _err(dk, ref.dk), "dV": _err(dv, ref.dv)}


def check_outputs(got, case, what, pinned=True):
    """``got`` = (o, tau, supp, dq, dk, dv) of an fp32 computation of ``case``: supp admissible (equal to c64 on every
    empty-window row, 0 on rows with a masked query or no live key), then tau and O within 1e-5 and dQ, dK, dV within
    1e-4 of ``reference`` pinned to supp; masked query rows exactly zero in O and dQ.  -> the figures, printed.
    ``pinned=False`` compares with fp64's own support instead (what the stand-in experiment shows to be too strict)."""
    o, tau, supp, dq, dk, dv = (x.detach().cpu() for x in got)
    win = case.win
    nwin, n = case_conditions(case, what)
    c = supp.to(th.int64)
    assert c.shape == win.c64.shape, (what, c.shape)
    assert int(c[~win.rows].abs().max() if (~win.rows).any() else 0) == 0, what + ": supp != 0 on a row without a support"
    ok = admissible(c, win.c64, win.nW, win.nWin) | ~win.rows
    assert bool(ok.all()), "%s: %d rows with a support size fp64 does not admit (first %s: %d, fp64 %d, window %d)" % (
        what, int((~ok).sum()), tuple(ok.logical_not().nonzero()[0].tolist()), int(c[~ok][0]), int(win.c64[~ok][0]), int(win.nW[~ok][0]))
    assert th.equal(c[win.nW == 0], win.c64[win.nW == 0]), what
    differ = int((c != win.c64).sum())
    fig = errors(got, case, pinned)
    print("%s: err tau %.2e O %.2e dQ %.2e dK %.2e dV %.2e; %d of %d rows with a window key, %d decided unlike fp64" % (
        what, fig["tau"], fig["O"], fig["dQ"], fig["dK"], fig["dV"], nwin, n, differ))
    for name, tol in (("tau", TOL_FWD), ("O", TOL_FWD), ("dQ", TOL_GRAD), ("dK", TOL_GRAD), ("dV", TOL_GRAD)):
        assert fig[name] <= tol, "%s: %s err %g > %g" % (what, name, fig[name], tol)
    if case.qm is not None and bool((~case.qm).any()):
        assert float(o[~case.qm].abs().max()) == 0.0 and float(dq[~case.qm].abs().max()) == 0.0, what + ": masked query rows"
    if case.km is not None:
        dead = ~case.km.any(dim=1)
        if bool(dead.any()):
            assert int(supp[dead].abs().max()) == 0, what + ": supp on an all-masked pair"
    fig.update(window_rows=nwin, rows=n, differ=differ)
    return fig
