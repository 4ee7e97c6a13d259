"""The derivative branches the PRODUCT took at its ReLU / LeakyReLU sites, read from what it keeps for its own backward.

A pre-activation within fp32 rounding of zero may land on the other side of the kink in the product than in the oracle
(other association of the sums).  Both are right: each differentiates the piecewise-linear function it evaluated.  So a
gradient test does not need an exception for such units -- it needs the oracle to differentiate the SAME pieces:

  1. run the product forward; ``fused_hidden`` / ``modular_hidden`` / ``head_hidden`` return the post-activation hidden rows
     per site, in the oracle's site order (``hidden > 0`` is the rule the product's backward applies to them);
  2. ``branch_masks`` checks them against the oracle's recorded pre-activations (``dmp_oracle.PROBE``) on the live rows --
     a branch may differ only within ``util_flips.TAU`` of the kink, the hidden values are ``act(pre)`` to the forward
     tolerance, the window holds few units -- and hands out the masks;
  3. the oracle runs under ``dmp_oracle.pinned(masks)``; its gradients are compared at the strict tolerance, everywhere.

A site whose hidden rows the product's route does not keep RAISES (``MissingHiddenRows``); nothing here ever falls back to
the oracle's own branch.  Rows under a zero of a 0 / 1 gate are dead in the product (unwritten, NaN under
``fused.POISON_DEAD_ROWS``): their mask is ``hidden > 0`` like any other (False for NaN) and irrelevant -- the gate multiplies
their gradient by zero -- and ``live`` keeps them out of the checks."""
import torch as th

from util_flips import TAU

WINDOW_SHARE = 5e-4     # the reference's own units inside the window: at most max(3, this share of the live units) per site


class MissingHiddenRows(AssertionError):
    pass


def _nodes(outputs):
    """Every autograd node below ``outputs``, in the order the forward created them."""
    seen, stack = set(), [t.grad_fn for t in outputs if th.is_tensor(t) and t.grad_fn is not None]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        stack.extend(f for f, _ in fn.next_functions)
    return sorted(seen, key=lambda f: f._sequence_nr())


def fused_hidden(outputs, sides=None):
    """Hidden rows of every ``_FusedDMPLayer`` node below ``outputs`` (tensors of the product, before ``backward()``):
    ``[(site, rows), ...]`` with, per layer, the node MLP's ``H1n`` and then the edge MLP's ``H1e``.
    ``sides = ((Np, Ep), (Ng, Eg))``: the pattern and the target went through the layers as ONE union graph (pattern rows
    first, ``collate.union_graphs``) or one after the other; the result lists all pattern sites, then all target sites, as
    ``model_oracle.model_forward`` evaluates them."""
    layers = [f for f in _nodes(outputs) if type(f).__name__ == "_FusedDMPLayerBackward"]
    if not layers:
        raise MissingHiddenRows("nmlp / emlp: no _FusedDMPLayer node below these outputs")
    out = [[] for _ in (sides or (None,))]
    for f in layers:
        H1n, H1e = f.saved_tensors[3], f.saved_tensors[4]
        for site, rows in (("nmlp", H1n), ("emlp", H1e)):
            if rows is None or rows.dim() != 2:
                raise MissingHiddenRows("%s: a fused layer keeps no [rows, H] hidden buffer for it" % site)
        if sides is None:
            out[0] += [("nmlp", H1n), ("emlp", H1e)]
            continue
        (np_, ep_), (ng_, eg_) = sides
        if (H1n.size(0), H1e.size(0)) == (np_ + ng_, ep_ + eg_):
            out[0] += [("p nmlp", H1n[:np_]), ("p emlp", H1e[:ep_])]
            out[1] += [("g nmlp", H1n[np_:]), ("g emlp", H1e[ep_:])]
        elif (H1n.size(0), H1e.size(0)) == (np_, ep_) and (np_, ep_) != (ng_, eg_):
            out[0] += [("p nmlp", H1n), ("p emlp", H1e)]
        elif (H1n.size(0), H1e.size(0)) == (ng_, eg_) and (np_, ep_) != (ng_, eg_):
            out[1] += [("g nmlp", H1n), ("g emlp", H1e)]
        else:
            raise MissingHiddenRows("nmlp / emlp: hidden buffers of %d / %d rows belong to neither side nor to their union" % (
                H1n.size(0), H1e.size(0)))
    return [s for side in out for s in side]


def _kinked(module):
    return type(module) in (th.nn.ReLU, th.nn.LeakyReLU)


class modular_hidden:
    """The same for layers that run their MLPs module by module (``DMPLayer.forward``, UNC's ``DualGraphConv``)::

        with modular_hidden(layers) as rec:
            out = forward(...)
        hidden = rec.rows(out)

    Per layer and MLP (``nmlp``, then ``emlp``) with a ReLU / LeakyReLU inside: the output of that activation module where the
    route calls it (forward hook), else the output the fused Linear + activation node (``ops._LinearNN``) keeps for its
    backward, found below ``out`` by the first Linear's weight."""

    def __init__(self, layers):
        self.layers, self.calls, self.handles = list(layers), {}, []

    def __enter__(self):
        for layer in self.layers:
            for mlp in (layer.nmlp, layer.emlp):
                for m in mlp:
                    if _kinked(m):
                        self.handles.append(m.register_forward_hook(lambda mod, inp, out: self.calls.setdefault(mod, []).append(out)))
        return self

    def __exit__(self, *exc):
        for h in self.handles:
            h.remove()
        return False

    def rows(self, outputs):
        kept = {}
        for f in _nodes(outputs):
            if type(f).__name__ == "_LinearNNBackward" and f.saved_tensors[2] is not None:
                kept.setdefault(f.saved_tensors[1].data_ptr(), []).append(f.saved_tensors[2])
        out = []
        for i, layer in enumerate(self.layers):
            for site in ("nmlp", "emlp"):
                mlp = getattr(layer, site)
                for j, m in enumerate(mlp):
                    if not _kinked(m):
                        continue
                    found = list(self.calls.get(m, []))
                    if not found and j > 0 and isinstance(mlp[j - 1], th.nn.Linear):
                        found = kept.get(mlp[j - 1].weight.data_ptr(), [])
                    if len(found) != 1:
                        raise MissingHiddenRows("layer %d %s: %d hidden buffers kept on this route (one expected)" % (i, site, len(found)))
                    out.append((site, found[0].detach()))
        return out


def head_hidden(pred):
    """Hidden rows ``act(pred_fc1(.))`` [B, h] of the pooled count heads below ``pred`` (node head, then edge head)."""
    out = []
    for f in _nodes([pred]):
        if type(f).__name__ == "_PooledHeadsHIPBackward":
            for k in f.keep:                                     # (sums, pl, gl, F, Y1S, blend, parameters)
                out.append(("pred_fc1", k[4][:, :k[6][0].size(0)]))
        elif type(f).__name__ == "_PooledHeadBackward":
            out.append(("pred_fc1", f.saved_tensors[3][:, :f.saved_tensors[4].size(0)]))
    if not out:
        raise MissingHiddenRows("pred_fc1: no pooled-head node below the prediction keeps its hidden rows")
    return out


def kinked_probes(probes):
    """The entries of ``dmp_oracle.PROBE`` that are pre-activations of a ReLU / LeakyReLU (a smooth site records one column of inf)."""
    return [(s, p) for s, p in probes if not (p.dim() == 2 and p.size(1) == 1 and bool(th.isinf(p).all()))]


def branch_masks(hidden, probes, live, act, fwd_tol, what):
    """bool masks ``hidden > 0`` per site (on the CPU), after three checks on the live rows of every site against the
    REFERENCE's pre-activations ``probes`` (``kinked_probes`` of an unpinned oracle run, same site order):

    * a branch differs from the reference's only where ``|pre| <= TAU * max(1, |pre|max)``;
    * ``hidden == act(pre)`` within ``fwd_tol * max(1, |act(pre)|max)``;
    * the reference's own units inside that window number at most ``max(3, WINDOW_SHARE * live units)``.

    ``live``: per site a bool [rows] tensor or None (every row is live).  ``act``: the reference's activation function.
    Prints the counts per site and returns ``(masks, differing)``: ``differing[i]`` = live units on the other branch."""
    assert len(hidden) == len(probes) == len(live), "%s: %d sites kept, %d probed, %d live lists" % (what, len(hidden), len(probes), len(live))
    masks, differing = [], []
    for i, ((site, rows), (osite, pre), lv) in enumerate(zip(hidden, probes, live)):
        name = "%s site %d (%s / %s)" % (what, i, site, osite)
        pre = pre.detach().double()
        rows = rows.detach().to(pre.device)
        assert tuple(rows.shape) == tuple(pre.shape), "%s: hidden rows %s, pre-activation %s" % (name, tuple(rows.shape), tuple(pre.shape))
        mask = rows > 0
        masks.append(mask.cpu())
        lv = th.ones(pre.size(0), dtype=th.bool, device=pre.device) if lv is None else lv.to(pre.device).view(-1).bool()
        assert lv.numel() == pre.size(0), name
        units = int(lv.sum()) * pre.size(1)
        if units == 0:
            differing.append(0)
            print("%s: no live rows" % name)
            continue
        lpre, lrows, lmask = pre[lv], rows[lv].double(), mask[lv]
        assert bool(th.isfinite(lrows).all()), "%s: a live hidden row is not finite" % name
        window = lpre.abs() <= TAU * max(1.0, float(pre.abs().max()))
        differ = lmask != (lpre > 0)
        n_win, n_diff, n_out = int(window.sum()), int(differ.sum()), int((differ & ~window).sum())
        ref = act(lpre)
        err, scale = float((lrows - ref).abs().max()), max(1.0, float(ref.abs().max()))
        print("%s: %d live units, %d in the window, %d branches differ from the reference, hidden err %.3g (scale %.3g)" % (
            name, units, n_win, n_diff, err, scale))
        assert n_out == 0, "%s: %d branches differ outside the rounding window, e.g. pre %g" % (
            name, n_out, float(lpre[differ & ~window][0]))
        assert err <= fwd_tol * scale, "%s: hidden rows off by %g (scale %g, tolerance %g)" % (name, err, scale, fwd_tol)
        assert n_win <= max(3, WINDOW_SHARE * units), "%s: %d of %d live units inside the window" % (name, n_win, units)
        differing.append(n_diff)
    return masks, differing
