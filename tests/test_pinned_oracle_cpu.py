"""The oracle's branch pin (``dmp_oracle.PIN``) and the branch reader's checks (tests/util_branches.py), on the CPU.

The stand-in for a product is the fp32 oracle whose pre-activations carry an error of 2e-6 of the tensor's largest value
(the size of a re-association of the sums): enough to put some units on the other side of the kink than the fp64 run,
which moves gradients by percents -- and by nothing measurable once the fp64 run is pinned to the stand-in's branches."""
import numpy as np
import pytest
import torch as th

import dmp_oracle as O
from util_branches import branch_masks, kinked_probes
from util_flips import TAU
from util_graphs import er_batch


def _case(batch, n, m, h, act, dtype):
    """2 layers, gates, residual; the tensors of test_gpu_dmplayer's rep-net cases, in ``dtype``, as fresh leaves."""
    rng = np.random.default_rng(n * h + batch)
    src, dst, rev, N, _, _ = er_batch(batch, n, m, rng)
    E = len(src)
    gen = th.Generator().manual_seed(h + n)
    layers = [O.random_dmp_params(h, h, gen, act) for _ in range(2)]
    v0, e0 = th.randn(N, h, generator=gen), th.randn(E, h, generator=gen)
    wv, we = th.randn(N, h, generator=gen), th.randn(E, h, generator=gen)
    vg, eg = (th.rand(N, 1, generator=gen) < 0.7).float(), (th.rand(E, 1, generator=gen) < 0.7).float()
    c = dict(src=th.from_numpy(src), dst=th.from_numpy(dst), rev=th.from_numpy(rev), N=N, act=act,
             layers=[{k: v.to(dtype).requires_grad_(True) for k, v in p.items()} for p in layers],
             v=v0.to(dtype).requires_grad_(True), e=e0.to(dtype).requires_grad_(True), wv=wv.to(dtype), we=we.to(dtype),
             vg=vg.to(dtype), eg=eg.to(dtype))
    c["live"] = [vg.view(-1) != 0, eg.view(-1) != 0] * 2
    return c


def _run(c, masks=None, probe=False):
    """Forward + backward of the oracle on the case -> (outputs + gradients by name, probes)."""
    O.PROBE = [] if probe else None
    try:
        fwd = lambda: O.dmpnn_graph_rep(c["layers"], c["src"], c["dst"], c["rev"], O.out_degrees(c["src"], c["N"]), c["v"], c["e"],
                                        c["vg"], c["eg"], True, c["act"])
        if masks is None:
            a, b = fwd()
        else:
            with O.pinned(masks):
                a, b = fwd()
        probes = O.PROBE
    finally:
        O.PROBE = None
    leaves = [("dv", c["v"]), ("de", c["e"])] + [("%d.%s" % (i, k), p) for i, l in enumerate(c["layers"]) for k, p in l.items()]
    grads = th.autograd.grad((a * c["wv"]).sum() + (b * c["we"]).sum(), [t for _, t in leaves])
    out = {"v_rep": a.detach(), "e_rep": b.detach()}
    out.update({k: g for (k, _), g in zip(leaves, grads)})
    return out, probes


def _worst(got, ref):
    """{name: |got - ref|max / max(1, |ref|max)} over the gradients."""
    return {k: float((got[k].double() - ref[k].double()).abs().max()) / max(1.0, float(ref[k].abs().max()))
            for k in ref if k not in ("v_rep", "e_rep")}


def _strict(got, ref, what):
    for k, e in _worst(got, ref).items():
        tol = 1e-4 if k in ("dv", "de") else 2e-4
        assert e <= tol, "%s %s: %g (tolerance %g)" % (what, k, e, tol)


@pytest.mark.parametrize("act", ["relu", "leaky_relu"])
@pytest.mark.parametrize("batch,n,m,h", [(8, 16, 40, 32), (3, 5, 7, 20)])
def test_pinning_the_oracle_to_its_own_branches_changes_nothing(batch, n, m, h, act):
    c = _case(batch, n, m, h, act, th.float64)
    free, probes = _run(c, probe=True)
    probes = kinked_probes(probes)
    assert [s for s, _ in probes] == ["nmlp", "emlp", "nmlp", "emlp"]
    own, _ = _run(c, [p > 0 for _, p in probes])
    for k in free:
        assert th.equal(own[k], free[k]), k


def test_a_wrong_count_or_shape_of_masks_raises():
    c = _case(3, 5, 7, 20, "leaky_relu", th.float64)
    _, probes = _run(c, probe=True)
    masks = [p > 0 for _, p in kinked_probes(probes)]
    with pytest.raises(ValueError, match="only 3 branch masks"):
        _run(c, masks[:3])
    with pytest.raises(ValueError, match="5 branch masks pinned"):
        _run(c, masks + masks[:1])
    with pytest.raises(ValueError, match="site 1"):
        _run(c, [masks[0], masks[1][:-1]] + masks[2:])
    with pytest.raises(ValueError, match="site 0"):
        _run(c, [masks[0].float()] + masks[1:])
    assert O.PIN is None                                          # a failed run leaves no pin behind
    c["act"] = "tanh"                                             # a smooth activation takes no entry
    _run(c, [])
    with pytest.raises(ValueError, match="1 branch masks pinned"):
        _run(c, masks[:1])


@pytest.mark.parametrize("act", ["relu", "leaky_relu"])
def test_pinned_to_a_stand_in_products_branches_the_strict_rule_holds(act, monkeypatch):
    """(32, 64, 256, 64), 2.4 M units.  The stand-in differs from fp64 in >= 10 branches, all inside the window; unpinned
    that breaks 2e-4; pinned, every parameter gradient holds 2e-4 and dv / de hold 1e-4; and ONE pinned unit flipped, on a
    live row and far from the kink, is seen."""
    shape = (32, 64, 256, 64)
    c64 = _case(*shape, act, th.float64)
    free, probes = _run(c64, probe=True)
    probes = kinked_probes(probes)
    # the stand-in: fp32, every pre-activation off by 2e-6 of its tensor's largest value, up or down; it keeps its hidden rows
    gen = th.Generator().manual_seed(7)
    hidden, plain = [], O.act_at

    def noisy(site, pre, fn):
        out = plain(site, pre + (th.randint(0, 2, pre.shape, generator=gen) * 2 - 1) * (2e-6 * float(pre.detach().abs().max())), fn)
        hidden.append((site, out.detach()))
        return out
    monkeypatch.setattr(O, "act_at", noisy)
    stand_in, _ = _run(_case(*shape, act, th.float32))
    monkeypatch.setattr(O, "act_at", plain)
    masks, differing = branch_masks(hidden, probes, c64["live"], O.activation(act), 1e-4, "stand-in " + act)
    # the stand-in writes every row, so its branches can be counted over all of them: dozens differ, most in rows under a
    # zero gate (tiny inputs), where they move no gradient; the few on live rows do all of the damage below
    total = 0
    for (_, rows), (_, pre) in zip(hidden, probes):
        differ = (rows > 0) != (pre > 0)
        assert not bool((differ & (pre.abs() > TAU * max(1.0, float(pre.abs().max())))).any())
        total += int(differ.sum())
    print("branches differing from fp64: %d, on live rows %s" % (total, differing))
    assert total >= 10 and sum(differing) >= 3, (total, differing)
    worst = _worst(stand_in, free)
    print("unpinned: worst %g (%s)" % (max(worst.values()), max(worst, key=worst.get)))
    assert max(worst.values()) > 2e-4
    pinned, _ = _run(c64, masks)
    for k in ("v_rep", "e_rep"):
        assert th.equal(pinned[k], free[k]), k                    # the pin leaves the forward value alone
    worst = _worst(stand_in, pinned)
    print("pinned: worst %g (%s)" % (max(worst.values()), max(worst, key=worst.get)))
    _strict(stand_in, pinned, "pinned")
    # one wrong derivative among 2.4 M: the last node site, the first live unit whose |pre64| is above the median
    site = 2
    pre = probes[site][1].abs()
    far = (pre > pre[c64["live"][site]].median()) & c64["live"][site].view(-1, 1)
    r, col = (int(i) for i in far.nonzero()[0])
    flipped = [m.clone() for m in masks]
    flipped[site][r, col] = not bool(flipped[site][r, col])
    wrong, _ = _run(c64, flipped)
    with pytest.raises(AssertionError, match="one unit flipped"):
        _strict(stand_in, wrong, "one unit flipped")
