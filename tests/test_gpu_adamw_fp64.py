"""Every route of ``dp.FlatAdamW`` into ``adamw_kernel`` (csrc/dmp_fused.hip) -- ``dmp_adamw_step`` / ``_skip`` (host step count),
``_dev`` (device count), ``_guarded`` (veto word) and ``_segments`` (one count per tensor of a flat buffer) -- against the float64
restatement of ``util_fp64_adamw`` (tied to ``torch.optim.AdamW`` in double by test_adamw_ref_cpu.py), stage by stage after
EVERY step: the buffers are read before and after ``opt.step()`` and, with u = 2^-24,

* ``m'``     within  2 * 4u (|m| + |g|)  of ``moments`` of the pre-step buffers.  Four roundings in ``m + b1c * (g - m)``: the
  constant b1c = (float)(1 - beta1), the difference, the product, the sum (the library is built without contraction: no FMA);
  the first three act on a term of at most |g| + |m|, the last on |m'| <= |m| + |g|;
* ``v'``     within  2 * 6u v'_ref.  Six roundings in ``v * beta2 + b2c * g * g``: two constants, three products, one sum, all
  terms non-negative.  (No single term carries more than four of them -- constant, product, product, sum -- so 6 is the
  count of the expression, not the sharpest figure.);
* ``vmax'``  bitwise  max(vmax, v') of the kernel's own v', in fp32;
* ``p'``     within  2 * (3u |p| + 8u |upd|)  of ``update`` evaluated from the KERNEL'S OWN m' and v' / vmax' (a rounding in
  the moments is not charged twice), upd = lr / bc1 * m' / (sqrt(d) / sqrt(bc2) + eps).  On p: the constant
  (float)(1 - lr wd), the product, the final difference = 3.  On upd the longest chain is 8: the constant step_size =
  (float)(lr / bc1); sqrt, the constant (float)(1 / sqrt(bc2)), their product and the sum with eps (the rounding of eps itself
  touches only the eps term, which has one rounding fewer behind it); the quotient; the product with step_size; the final
  difference.  sqrt and the quotient are correctly rounded (no fast-math);
* elements that are to be left alone (skipped ranges, dead tensors, vetoed steps, the padding floats of a flat buffer): all
  four buffers bitwise as before;
* the device state (``state["dev"]``, ``state["dev_seg"]``, the signs and values of ``seg_tab``, the veto word) exactly what
  ``util_fp64_adamw.Bookkeeper`` says, which never reads the device.

The factors are counts of roundings in the code, the outer 2 is slack for the second-order terms; none is a measured number.
Each test prints the worst observed share of its bounds (``ADAMW64 ...``).

Pinned here too: a dead run that ends a buffer whose length is no multiple of 4 is left alone to its very end (the tail gap is
``(pos, numel)`` and the entry points accept a last bound equal to n); runs that do not start on a multiple of 4 are refused;
``eps = 0`` is refused on the flat buffer of ``flatten_parameters()`` (its padding would compute 0 / 0) and admitted on a
plain parameter; a step in which NO tensor of a flat buffer has a gradient leaves all of them alone."""
import pytest
import torch as th

import util_fp64_adamw as UA

pytestmark = pytest.mark.gpu

U = UA.U32
HYPER = {"A": dict(lr=3e-3, weight_decay=1e-2, betas=(0.9, 0.99), eps=1e-8),
         "B": dict(lr=1e-2, weight_decay=0.0, betas=(0.5, 0.9), eps=1e-6)}
ROUTES = ("skip", "dev", "guarded")
SMALL = (1, 3, 4, 5, 1023, 1025)
BIG = 2048 * 256 * 4 + 5          # the first size whose last elements are reached on the kernel's SECOND grid-stride trip, with a partial tail


def _bits(t):
    return t.contiguous().view(th.int32)


class Rig:
    """One ``FlatAdamW`` on one buffer ``p`` that holds the tensors ``layout`` = [(offset, numel), ...]; ``step()`` runs one
    optimizer step and holds every stage and the device state to the restatement and the bookkeeper."""

    def __init__(self, p, opt, route, layout, book, word=None, mask=0):
        self.p, self.opt, self.route, self.layout, self.book = p, opt, route, layout, book
        self.word, self.mask = word, mask
        self.worst = {"m": 0.0, "v": 0.0, "p": 0.0}
        self.touched = 0

    @property
    def group(self):
        return self.opt.param_groups[0]

    def _snap(self):
        st = self.opt.state.get(self.p, {})
        zero = th.zeros(self.p.numel())
        out = {"p": self.p.detach().cpu().clone(), "g": self.p.grad.detach().cpu().clone().view(-1)}
        for name, key in (("m", "exp_avg"), ("v", "exp_avg_sq"), ("vmax", "max_exp_avg_sq")):
            out[name] = st[key].detach().cpu().clone().view(-1) if key in st else zero
        out["p"] = out["p"].view(-1)
        return out

    def _hold(self, err, bound, what, it):
        ratio = th.where(bound > 0, err / bound.clamp_min(1e-300), th.where(err > 0, th.full_like(err, float("inf")), th.zeros_like(err)))
        worst = float(ratio.max()) if ratio.numel() else 0.0
        self.worst[what] = max(self.worst[what], worst)
        assert worst <= 1.0, "%s' at step %d: %.3g of its bound at element %d" % (what, it, worst, int(ratio.argmax()))

    def step(self, live=None, flags=None, it=0):
        """``live``: the tensors of the layout that the optimizer was told (by the caller) to update, None = all."""
        g, ams = self.group, self.group["amsgrad"]
        b1, b2 = g["betas"]
        lr, eps, wd = float(g["lr"]), g["eps"], g["weight_decay"]
        if flags is not None:
            self.word[0] = int(flags)
        pre = self._snap()
        self.opt.step()
        post = self._snap()
        counts = self.book.advance(live, flags, self.mask) if self.word is not None else self.book.advance(live)
        step_e = th.zeros(self.p.numel(), dtype=th.int64)
        for (off, n), c in zip(self.layout, counts):
            step_e[off:off + n] = c
        sel = step_e > 0
        for name in ("p", "m", "v", "vmax"):                                   # left alone: bitwise as before
            assert th.equal(_bits(post[name])[~sel], _bits(pre[name])[~sel]), (name, "rewritten where it is to be left alone", it)
        assert th.equal(post["g"], pre["g"])
        if ams or "max_exp_avg_sq" in self.opt.state.get(self.p, {}):
            assert ams and "max_exp_avg_sq" in self.opt.state[self.p]
        if bool(sel.any()):
            if bool(sel.all()):
                sel = slice(None)
            self.touched += int(step_e[sel].numel())
            p0, m0, v0, gg = (pre[k][sel].double() for k in ("p", "m", "v", "g"))
            m1, v1 = post["m"][sel].double(), post["v"][sel].double()
            mr, vr, _ = UA.moments(m0, v0, None, gg, b1, b2)
            self._hold((m1 - mr).abs(), 2 * 4 * U * (m0.abs() + gg.abs()), "m", it)
            self._hold((v1 - vr).abs(), 2 * 6 * U * vr, "v", it)
            d = v1
            if ams:
                want = th.maximum(pre["vmax"][sel], post["v"][sel])             # fp32, of the kernel's own v'
                assert th.equal(_bits(post["vmax"][sel]), _bits(want)), ("vmax'", it)
                d = post["vmax"][sel].double()
            pr = UA.update(p0, m1, d, lr, b1, b2, eps, wd, step_e[sel])
            upd = UA.update(th.zeros_like(p0), m1, d, lr, b1, b2, eps, wd, step_e[sel]).abs()
            self._hold((post["p"][sel].double() - pr).abs(), 2 * (3 * U * p0.abs() + 8 * U * upd), "p", it)
        self._device_state(counts, lr, b1, b2)
        return counts

    def _device_state(self, counts, lr, b1, b2):
        st = self.opt.state[self.p]
        if self.word is not None:
            assert self.word.tolist() == self.book.word
        if self.route == "skip":
            assert "dev" not in st and "dev_seg" not in st and st["step"] == self.book.taken
        elif self.route in ("dev", "guarded"):
            assert "dev_seg" not in st and st["dev"].tolist() == [float(self.book.taken), lr]
        else:
            assert "dev" not in st and st["dev_seg"].tolist() == [float(self.book.taken), lr] + [float(s) for s in self.book.steps]
            tab = st["seg_tab"].cpu().double().view(-1, 2)
            c = th.tensor(counts, dtype=th.float64)
            dead = c == 0
            assert bool((tab[dead, 0] < 0).all()) and bool((tab[~dead, 0] > 0).all())
            if bool((~dead).any()):                                            # one fp32 rounding of a double: within 2u
                want0 = lr / (1.0 - th.pow(th.tensor(b1, dtype=th.float64), c[~dead]))
                want1 = 1.0 / (1.0 - th.pow(th.tensor(b2, dtype=th.float64), c[~dead])).sqrt()
                assert bool(((tab[~dead, 0] - want0).abs() <= 2 * U * want0).all())
                assert bool(((tab[~dead, 1] - want1).abs() <= 2 * U * want1).all())

    def report(self, what):
        assert self.touched > 0, "no element was ever updated: nothing was checked"
        print("ADAMW64 %s: worst share of the bound  m' %.3f  v' %.3f  p' %.3f  (%d element-steps)"
              % (what, self.worst["m"], self.worst["v"], self.worst["p"], self.touched))


def _optimizer(p, route, hyper, amsgrad, gpu, mask=1):
    from dualmessagepassing_amd.dp import FlatAdamW
    opt = FlatAdamW([p], amsgrad=amsgrad, capturable=route == "dev", **hyper)
    word = None
    if route == "guarded":
        word = th.zeros(4, dtype=th.int32, device=gpu)
        opt.set_veto(word, mask)
    return opt, word


def _plain(n, route, hyper, amsgrad, gpu, pieces=None, mask=1, start=0):
    """A plain parameter [n] (no per-tensor segments).  ``pieces``: [(offset, numel), ...] that hand-set live runs treat as
    tensors -- they share the buffer's one step count."""
    p = th.nn.Parameter(UA.parameter(n, n).to(gpu))
    opt, word = _optimizer(p, route, hyper, amsgrad, gpu, mask)
    layout = pieces if pieces is not None else [(0, n)]
    return Rig(p, opt, route, layout, UA.Bookkeeper(len(layout), shared=True, start=start), word, mask)


def _schedule(rig, n, steps, gpu, flags=None):
    """The plain schedule: a x10 spike at the third step (AMSGrad's maximum is the older value afterwards), the learning rate
    divided by 3 through ``param_groups`` before the fifth."""
    for it in range(steps):
        if it == 4:
            rig.group["lr"] = rig.group["lr"] / 3.0
        rig.p.grad = UA.gradient(n, n, it, spike=it == 2).to(gpu)
        rig.step(None, None if flags is None else flags[it], it)


@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("hyper", ["A", "B"])
@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("route", ROUTES)
def test_plain_parameter_every_stage(route, n, hyper, amsgrad, gpu):
    rig = _plain(n, route, dict(HYPER[hyper]), amsgrad, gpu)
    _schedule(rig, n, 6, gpu, flags=[0] * 6 if route == "guarded" else None)
    assert rig.book.taken == 6
    rig.report("%s n %d %s amsgrad %d" % (route, n, hyper, amsgrad))


@pytest.mark.parametrize("route", ROUTES)
def test_second_grid_stride_trip_and_its_partial_tail(route, gpu):
    """2,097,152 + 5 elements: the launch is capped at 2048 workgroups x 256 lanes x 4 floats, so the last five elements are
    one full group and one group of a single float on the second trip of the kernel's loop."""
    rig = _plain(BIG, route, dict(HYPER["A"]), True, gpu)
    _schedule(rig, BIG, 2, gpu, flags=[0, 0] if route == "guarded" else None)
    tail = rig.p.grad[-5:].cpu()
    assert int((tail != 0).sum()) >= 4                                        # (their update is visible: the stage checks bind)
    rig.report("%s n %d" % (route, BIG))


@pytest.mark.parametrize("route", ROUTES + ("segments",))
def test_state_loaded_at_step_100000(route, gpu):
    """``load_state_dict`` of a state at step 100,000 (beta1^step underflows: both corrections are exactly 1), then two steps."""
    from dualmessagepassing_amd.dp import FlatAdamW
    hyper = dict(HYPER["A"])
    if route == "segments":
        sync, master, layout = _flat(gpu, _sizes(5), 9)
        first = FlatAdamW([master], amsgrad=True, **hyper)
        _feed(sync, master, layout, None, 0, gpu)
        first.step()
        sd = first.state_dict()
        assert sd["state"][0]["seg_steps"] == [1] * 5
        sd["state"][0]["step"] = 100000
        sd["state"][0]["seg_steps"] = [100000] * 5
        opt = FlatAdamW([master], amsgrad=True, **hyper)
        opt.load_state_dict(sd)
        rig = Rig(master, opt, route, layout, UA.Bookkeeper(5, start=100000))
        for it in (1, 2):
            live = None if it == 1 else (0, 2, 4)
            _feed(sync, master, layout, live, it, gpu)
            rig.step(live, None, it)
        assert rig.book.steps == [100002, 100001, 100002, 100001, 100002]
    else:
        n = 1025
        rig0 = _plain(n, route, hyper, True, gpu)
        _schedule(rig0, n, 1, gpu, flags=[0] if route == "guarded" else None)
        sd = rig0.opt.state_dict()
        sd["state"][0]["step"] = 100000
        opt, word = _optimizer(rig0.p, route, hyper, True, gpu)
        opt.load_state_dict(sd)
        rig = Rig(rig0.p, opt, route, [(0, n)], UA.Bookkeeper(1, shared=True, start=100000), word, 1)
        for it in (1, 2):
            rig.p.grad = UA.gradient(n, n, it, spike=it == 2).to(gpu)
            rig.step(None, 0 if route == "guarded" else None, it)
        assert rig.book.taken == 100002
    rig.report("%s loaded at 100000" % route)


# ------------------------------------------------------------------------------------------------ skip ranges (hand-set runs)

def _pieces(gaps):
    """A buffer laid out in 4-float pieces of 4, 8 or 12 floats, live (L) and dead (D) alternating, with ``gaps`` dead pieces:
    1: L D (the gap ends the buffer), 16: D L ... D L (a gap opens it), 17: L D ... L D."""
    kinds = {1: "LD", 16: "DL" * 16, 17: "LD" * 17}[gaps]
    pieces, off = [], 0
    for k in range(len(kinds)):
        n = 4 * (1 + k % 3)
        pieces.append((off, n))
        off += n
    return pieces, [k for k, c in enumerate(kinds) if c == "L"], off


@pytest.mark.parametrize("route,gaps", [(r, g) for r in ROUTES for g in (1, 16)] + [("skip", 17)])
def test_live_runs_leave_the_gaps_alone(route, gaps, gpu):
    """``_dmp_live_runs`` with 1, 16 (one launch, skip ranges) and 17 gaps (the host-count route: one launch per live run); a step
    with every piece live in between."""
    pieces, live, n = _pieces(gaps)
    rig = _plain(n, route, dict(HYPER["A"]), True, gpu, pieces=pieces)
    for it in range(3):
        some = it != 1
        rig.p._dmp_live_runs = [pieces[k] for k in live] if some else None
        rig.p.grad = UA.gradient(n, n, it, spike=it == 2).to(gpu)
        rig.step(live if some else None, 0 if route == "guarded" else None, it)
    rig.report("%s %d gaps" % (route, gaps))


@pytest.mark.parametrize("route", ["dev", "guarded"])
def test_seventeen_gaps_are_refused_on_the_device_count_routes(route, gpu):
    pieces, live, n = _pieces(17)
    rig = _plain(n, route, dict(HYPER["A"]), True, gpu, pieces=pieces)
    rig.p._dmp_live_runs = [pieces[k] for k in live]
    rig.p.grad = UA.gradient(n, n, 0).to(gpu)
    before = rig.p.detach().clone()
    with pytest.raises(ValueError, match="more than 16 gaps"):
        rig.opt.step()
    assert th.equal(rig.p.detach(), before)


@pytest.mark.parametrize("route", ROUTES)
def test_a_dead_run_that_ends_an_unaligned_buffer_is_left_alone_to_the_end(route, gpu):
    """1030 floats, the first 1024 live: the tail gap is (1024, 1030) and floats 1028 and 1029 -- the partial group of 4 -- stay
    as they are (the gap used to end at 1028).  A run that does not start on a multiple of 4 is refused."""
    from dualmessagepassing_amd._lib import DmpError
    n = 1030
    pieces = [(0, 1024), (1024, 6)]
    rig = _plain(n, route, dict(HYPER["A"]), True, gpu, pieces=pieces)
    for it in range(2):
        rig.p._dmp_live_runs = [pieces[0]]
        rig.p.grad = UA.gradient(n, n, it).to(gpu)
        rig.step((0,), 0 if route == "guarded" else None, it)
    rig.report("%s tail gap to numel" % route)
    rig.p._dmp_live_runs = [(0, 1022)]
    with pytest.raises(DmpError, match="DMP_ERR_BAD_ARG"):
        rig.opt.step()


# ---------------------------------------------------------------------------------------------------------------- guarded

def test_guarded_drops_flagged_steps_only(gpu):
    """Mask 2.  The first two steps are dropped (flags 2, then 6 = a bit inside and a bit outside the mask): the first COUNTED
    step is the third, at count 1, and ``word[3] == 2``.  Flags outside the mask alone (5) let the step go ahead."""
    n = 1025
    rig = _plain(n, "guarded", dict(HYPER["A"]), True, gpu, mask=2)
    flags = [2, 6, 0, 5, 0, 2, 1]
    seen = []
    for it, f in enumerate(flags):
        if it == 4:
            rig.group["lr"] = 1e-3
        rig.p.grad = UA.gradient(n, n, it, spike=it == 2).to(gpu)
        seen.append(rig.step(None, f, it)[0])
        if it == 1:
            assert rig.word.tolist() == [0, 6, 1, 2]
    assert seen == [0, 0, 1, 2, 3, 0, 4] and rig.word.tolist() == [0, 7, 0, 3]
    rig.opt.sync_state()
    assert rig.opt.state[rig.p]["step"] == 4
    rig.report("guarded flags")


# --------------------------------------------------------------------------------------------------------------- segments

def _sizes(P, tiny=False):
    """Tensor sizes, none a multiple of 4 (every tensor is followed by padding floats)."""
    cycle = (1, 2, 3, 5) if tiny else (1, 2, 3, 5, 185, 130)
    return [cycle[i % len(cycle)] for i in range(P)]


def _flat(gpu, sizes, seed):
    from dualmessagepassing_amd.dp import FlatGradSync

    class Bag(th.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = th.nn.ParameterList([th.nn.Parameter(UA.parameter(n, seed + i)) for i, n in enumerate(sizes)])

    sync = FlatGradSync(Bag().to(gpu))
    master = sync.flatten_parameters()
    layout = list(zip(sync.offsets, sizes))
    pad = _padding(master, layout)
    assert int(pad.sum()) > 0 and bool((master.detach().cpu()[pad] == 0).all())
    return sync, master, layout


def _padding(master, layout):
    pad = th.ones(master.numel(), dtype=th.bool)
    for off, n in layout:
        pad[off:off + n] = False
    return pad


def _feed(sync, master, layout, live, it, gpu, spike=False):
    """Fresh gradients for the live tensors (None: all), packed into the flat gradient as a training step does."""
    flat = UA.gradient(master.numel(), 31, it, spike=spike).to(gpu)
    sync.detach_grads()
    for i in (range(len(layout)) if live is None else live):
        off, n = layout[i]
        sync.params[i].grad = flat[off:off + n].view_as(sync.params[i])
    sync.pack()
    assert master.grad is sync.flat
    some = live is not None and len(live) < len(layout)                        # (the host-side set; None when nothing is missing)
    assert master._dmp_live_params == (tuple(live) if some else None)


def _padding_is_zero(sync, rig):
    st, pad = rig.opt.state[rig.p], _padding(rig.p, rig.layout)
    for t in (rig.p, st["exp_avg"], st["exp_avg_sq"]) + ((st["max_exp_avg_sq"],) if "max_exp_avg_sq" in st else ()):
        assert bool((_bits(t.detach().cpu())[pad] == 0).all())


def _live_schedule(P):
    """All; two of three; the LAST tensor alone (tensor 64 of 65: the second live word); all but the last; another two of three;
    none; all."""
    return [None, tuple(i for i in range(P) if i % 3 != 0), (P - 1,), tuple(range(P - 1)),
            tuple(i for i in range(P) if i % 3 != 1), (), None]


@pytest.mark.parametrize("P,hyper,amsgrad", [(1, "A", True), (1, "B", False), (65, "A", True), (65, "B", False), (65, "A", False),
                                             (1024, "A", True), (1024, "B", False)])
def test_segments_keep_one_count_per_tensor(P, hyper, amsgrad, gpu):
    from dualmessagepassing_amd.dp import FlatAdamW
    sync, master, layout = _flat(gpu, _sizes(P, tiny=P >= 1024), P)
    opt = FlatAdamW([master], amsgrad=amsgrad, **HYPER[hyper])
    rig = Rig(master, opt, "segments", layout, UA.Bookkeeper(P))
    for it, live in enumerate(_live_schedule(P)):
        if it == 4:
            rig.group["lr"] = rig.group["lr"] / 3.0
        _feed(sync, master, layout, live, it, gpu, spike=it == 2)
        rig.step(live, None, it)
        _padding_is_zero(sync, rig)
    assert rig.book.taken == 7
    opt.sync_state()
    assert opt.state[master]["seg_steps"] == rig.book.steps and opt.state[master]["step"] == 7
    rig.report("segments P %d %s amsgrad %d" % (P, hyper, amsgrad))


@pytest.mark.parametrize("hyper,amsgrad", [("A", True), ("B", False)])
def test_1025_tensors_fall_back_to_one_shared_count_and_live_runs(hyper, amsgrad, gpu):
    """Above ``DMP_ADAMW_MAX_SEGMENTS`` tensors there are no per-tensor counts: the documented fallback is the buffer's one
    count and the live runs (more than 16 gaps: one launch per run).  A step in which no tensor has a gradient leaves every
    tensor alone."""
    from dualmessagepassing_amd import _abi
    from dualmessagepassing_amd.dp import FlatAdamW
    P = _abi.DMP_ADAMW_MAX_SEGMENTS + 1
    sync, master, layout = _flat(gpu, _sizes(P, tiny=True), P)
    opt = FlatAdamW([master], amsgrad=amsgrad, **HYPER[hyper])
    rig = Rig(master, opt, "skip", layout, UA.Bookkeeper(P, shared=True))
    for it, live in enumerate(_live_schedule(P)):
        if it == 4:
            rig.group["lr"] = rig.group["lr"] / 3.0
        _feed(sync, master, layout, live, it, gpu, spike=it == 2)
        counts = rig.step(live, None, it)
        assert "dev_seg" not in opt.state[master] and "seg_tab" not in opt.state[master]
        if it == 2:
            assert counts[P - 1] == 3 and sum(counts) == 3                     # the buffer's count, not the tensor's own
        _padding_is_zero(sync, rig)
    rig.report("fallback P %d %s amsgrad %d" % (P, hyper, amsgrad))


def test_segments_read_the_summed_live_indicators_from_the_device(gpu):
    """``master._dmp_live_dev``: 0 = dead, anything else (1, or 2 = live on two ranks) = live, whatever the host-side set says
    -- every tensor HAS a gradient in the buffer here, the dead ones must not be touched all the same."""
    from dualmessagepassing_amd.dp import FlatAdamW
    P = 9
    sync, master, layout = _flat(gpu, _sizes(P), 5)
    opt = FlatAdamW([master], amsgrad=True, **HYPER["A"])
    rig = Rig(master, opt, "segments", layout, UA.Bookkeeper(P))
    for it, ind in enumerate([[0, 1, 2, 0, 1, 2, 0, 1, 2], [2, 0, 0, 1, 1, 0, 2, 2, 0], [1] * 9, [0] * 9, [0, 0, 0, 0, 0, 0, 0, 0, 2]]):
        _feed(sync, master, layout, None, it, gpu, spike=it == 2)
        master._dmp_live_dev = th.tensor(ind, dtype=th.float32, device=gpu)
        rig.step(tuple(i for i, x in enumerate(ind) if x), None, it)
        _padding_is_zero(sync, rig)
    assert rig.book.steps == [2, 2, 2, 2, 3, 2, 2, 3, 3]
    rig.report("segments live_dev")


def test_a_veto_on_the_segment_route_advances_no_count_and_rewrites_nothing(gpu):
    from dualmessagepassing_amd.dp import FlatAdamW
    P = 7
    sync, master, layout = _flat(gpu, _sizes(P), 7)
    word = th.zeros(4, dtype=th.int32, device=gpu)
    opt = FlatAdamW([master], amsgrad=True, **HYPER["A"]).set_veto(word, 1)
    rig = Rig(master, opt, "segments", layout, UA.Bookkeeper(P), word, 1)
    lives = [None, (0, 2, 4, 6), (1, 3, 5), None, None, (0, 1, 2)]
    for it, (live, f) in enumerate(zip(lives, [0, 1, 2, 3, 1, 0])):
        if it == 2:
            rig.group["lr"] = 1e-3
        _feed(sync, master, layout, live, it, gpu, spike=it == 2)
        rig.step(live, f, it)
        _padding_is_zero(sync, rig)
    assert rig.book.steps == [2, 3, 2, 2, 1, 2, 1] and rig.book.taken == 3 and word.tolist() == [0, 3, 0, 3]
    rig.report("segments veto")


# ----------------------------------------------------------------------------------------------------------------- eps = 0

def test_eps_zero_is_refused_on_a_flat_buffer_and_admitted_on_a_plain_parameter(gpu):
    """On the flat buffer the padding floats (m' = d = 0 for ever) would compute 0 / 0 and put NaN into the parameter buffer,
    where the per-tensor optimizer has no such element: refused before anything is written, on the segment route and on the
    fallback alike.  A plain parameter has no padding: eps = 0 is torch's update there."""
    from dualmessagepassing_amd.dp import FlatAdamW
    for P in (3, 1025):
        sync, master, layout = _flat(gpu, _sizes(P, tiny=True), 3)
        opt = FlatAdamW([master], amsgrad=True, **dict(HYPER["A"], eps=0.0))
        _feed(sync, master, layout, None, 0, gpu)
        before = master.detach().clone()
        with pytest.raises(ValueError, match="eps = 0"):
            opt.step()
        assert th.equal(master.detach(), before) and not opt.state[master]
    n = 1025
    rig = _plain(n, "skip", dict(HYPER["A"], eps=0.0), True, gpu)
    for it in range(2):
        g = UA.gradient(n, n, it)
        rig.p.grad = th.where(g == 0, th.ones_like(g), g).to(gpu)              # (a zero gradient at eps = 0 is 0 / 0 in torch too)
        rig.step(None, None, it)
    assert bool(th.isfinite(rig.p.detach()).all())
    rig.report("plain eps 0")
