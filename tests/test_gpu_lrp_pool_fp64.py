"""The pool kernels (csrc/dmp_lrppool.hip, ``lrp.USE_POOL_KERNEL``) against the float64 loop restatement of ``util_fp64_lrp``
(checked against the reference's formulation in test_lrp_pool_cpu.py), on hand-made batches: an isolated node, a path, a
5-clique, a star of 9 (504 permutations of one node at L 4), duplicate and reversed-flag edges; L 1, 3, 4, 6; widths 64 / 128
in all four pairs; 0, 1, 31, 33 and a few hundred permutations; an index at a capacity.

* product and gradients within the band of ``util_fp64.within_band`` (1e-5 the product, 1e-4 the gradients: the figures of the
  TXL and heads modules for fp32-accurate products; the yardstick is the gather / dense-product route on the same inputs);
* two runs bit-equal; ``perm_pool`` with bias and relu equal on both routes (rtol 1e-5 / atol 1e-6, the figure of
  ``test_capacity_tail_adds_nothing``), the index at a capacity included;
* forward + backward of ``perm_pool`` at 4116 permutations allocate less than ONE [P * L*L, in] matrix (the other route
  allocates two);
* a recorded DMPLRP step at hid 64 replays on the kernels and ends where the eager run ends."""
import copy

import numpy as np
import pytest
import torch as th

import util_fp64 as U
import util_fp64_lrp as UL

pytestmark = pytest.mark.gpu

CASES = UL.cases()
_MEMO = {}


def _index(name, gpu):
    """(PermIndex on the GPU, (N, E, P)) of a case; "capacity": the hand-made batch of test_gpu_lrp_index.py at L 3, padded
    by 37 permutations."""
    from dualmessagepassing_amd.lrp import PermIndex
    if name == "capacity":
        from test_gpu_lrp_index import _hand_batch
        exact = PermIndex.from_batched(_hand_batch(gpu, True), 3)
        perm = PermIndex.from_batched(_hand_batch(gpu, True), 3, capacity=exact.num_perms + 37)
        assert perm.live is not None and perm.num_perms == exact.num_perms + 37
    else:
        perm = PermIndex.from_graphs(CASES[name]["graphs"], gpu, CASES[name]["L"])
    return perm, (perm.num_nodes, perm.num_edges, perm.num_perms)


def _shape(name):
    return (3, 64, 64) if name == "capacity" else (CASES[name]["L"], CASES[name]["fin"], CASES[name]["hid"])


def _reference(name, gpu):
    """The case's index, inputs and fp64 results: computed once, shared by the tests, never written to."""
    if name not in _MEMO:
        perm, (N, E, P) = _index(name, gpu)
        L, fin, hid = _shape(name)
        x, z, w, _, dout, _ = UL.inputs(name, N, E, P, L, fin, hid)
        _MEMO[name] = (perm, (x, z, w, dout), UL.perm_product_fp64(perm.slot, N, E, L, x, z, w, dout))
    return _MEMO[name]


def _product(perm, tensors, gpu, kernel, monkeypatch):
    from dualmessagepassing_amd import lrp
    monkeypatch.setattr(lrp, "USE_POOL_KERNEL", kernel)
    x, z, w, dout = (t.to(gpu) for t in tensors)
    x, z, w = (t.requires_grad_(True) for t in (x, z, w))
    before = lrp._PermProduct.calls
    out = lrp.perm_product(perm, x, z, w)
    assert lrp._PermProduct.calls - before == int(kernel), "the route taken"
    out.backward(dout)
    return out.detach(), x.grad, z.grad, w.grad


NAMES = sorted(CASES) + ["capacity"]
WHAT = (("out", 1e-5), ("d node_feat", 1e-4), ("d edge_feat", 1e-4), ("d weight", 1e-4))


@pytest.mark.parametrize("name", NAMES)
def test_product_and_gradients_against_fp64_and_twice_the_same(name, gpu, monkeypatch):
    perm, tensors, ref = _reference(name, gpu)
    got = _product(perm, tensors, gpu, True, monkeypatch)
    if perm.num_perms:
        yard = _product(perm, tensors, gpu, False, monkeypatch)
    else:
        yard = tuple(th.zeros_like(t) for t in got)          # no permutation: zeros on any route
    for a, r, y, (what, tol) in zip(got, ref, yard, WHAT):
        assert tuple(a.shape) == tuple(r.shape), what
        U.within_band(a, r, y, tol, "%s %s" % (name, what))
    again = _product(perm, tensors, gpu, True, monkeypatch)
    for a, b, (what, _) in zip(got, again, WHAT):
        assert th.equal(a, b), what + ": two runs differ"
    if perm.num_perms:
        assert float(got[0].abs().max()) > 0.1 and float(got[3].abs().max()) > 0.1


def _pooled(perm, name, gpu, kernel, monkeypatch):
    """``perm_pool`` with bias and relu, and every gradient.  The inputs are ``small``: rtol 1e-5 / atol 1e-6 has an absolute
    floor, and an fp32 sum of n terms carries about sqrt(n) 2^-24 of its largest partial sum whatever the order (n up to
    in L*L = 2048 here, hundreds of permutations in the weight gradient: 3e-6 of it), so the two routes can only be held to
    1e-6 in entries that all but cancel where the partial sums stay below ~0.3 -- products of size 0.1 sqrt(L), upstream
    factors of 0.02."""
    from dualmessagepassing_amd import lrp
    monkeypatch.setattr(lrp, "USE_POOL_KERNEL", kernel)
    L, fin, hid = _shape(name)
    x, z, w, b, _, coef = (t.to(gpu) for t in UL.inputs(name, perm.num_nodes, perm.num_edges, perm.num_perms, L, fin, hid, small=True))
    x, z, w, b = (t.requires_grad_(True) for t in (x, z, w, b))
    before = lrp._PermProduct.calls
    out = lrp.perm_pool(perm, x, z, w, b, th.relu)
    assert lrp._PermProduct.calls - before == int(kernel)
    (out * coef).sum().backward()
    return out.detach(), x.grad, z.grad, w.grad, b.grad


@pytest.mark.parametrize("name", [n for n in NAMES if not n.startswith("P0-")])
def test_perm_pool_is_the_same_on_both_routes(name, gpu, monkeypatch):
    perm, _ = _index(name, gpu)
    runs = [_pooled(perm, name, gpu, kernel, monkeypatch) for kernel in (True, False)]
    if name == "capacity":          # ... and the exact index on the kernels: the tail adds nothing
        from dualmessagepassing_amd.lrp import PermIndex
        from test_gpu_lrp_index import _hand_batch
        runs.append(_pooled(PermIndex.from_batched(_hand_batch(gpu, True), 3), name, gpu, True, monkeypatch))
    for other in runs[1:]:
        for a, b, what in zip(runs[0], other, ("out", "dx", "dz", "dw", "db")):
            assert th.allclose(a, b, rtol=1e-5, atol=1e-6), (name, what, float((a - b).abs().max()))
    # (a tail that reached d bias would add 37 upstream terms of size 0.02 to it: 1e-6 sees that)
    assert float(runs[0][3].abs().max()) > 1e-3 and float(runs[0][4].abs().max()) > 1e-3


def test_no_slot_row_buffer_in_either_pass(gpu, monkeypatch):
    from dualmessagepassing_amd import _lib, lrp
    L, fin, hid = 4, 64, 64
    L2 = L * L
    perm = lrp.PermIndex.from_graphs(UL.stars24(28 * 147), gpu, L)
    N, E, P = perm.num_nodes, perm.num_edges, perm.num_perms
    assert P == 4116 and perm._key_csr is None
    bound = P * L2 * fin * 4                                  # one slot-row matrix
    # what the route may allocate, by arithmetic: five [P, hid] arrays at a time (product, + bias, relu and gradients of
    # them), the workspace (bf16 planes of the panels + the weight gradient's partials), the key CSR (offsets and permutations:
    # int32; six int64 [P L*L] arrays while the keys are sorted: keys, sorted keys, order, the sort's scratch, the quotient),
    # the [N + E, in] gradients and the weight's twice
    lib = _lib.load()
    legit = (5 * P * hid * 4 + 4 * int(lib.dmp_lrp_pool_workspace_words(P, fin, hid, L))
             + (4 + 8) * ((N + E) * L2 + 1) + 4 * P * L2 + 6 * 8 * P * L2
             + 2 * (N + E) * fin * 4 + 2 * fin * hid * L2 * 4)
    assert legit < 0.75 * bound, (legit, bound)
    x, z, w, b, _, coef = (t.to(gpu) for t in UL.inputs("memory", N, E, P, L, fin, hid))
    x, z, w, b = (t.requires_grad_(True) for t in (x, z, w, b))

    def rise(kernel):
        monkeypatch.setattr(lrp, "USE_POOL_KERNEL", kernel)
        for t in (x, z, w, b):
            t.grad = None
        th.cuda.synchronize()
        th.cuda.reset_peak_memory_stats()
        before = th.cuda.memory_allocated()
        out = lrp.perm_pool(perm, x, z, w, b, th.relu)
        (out * coef).sum().backward()
        th.cuda.synchronize()
        return th.cuda.max_memory_allocated() - before

    new = rise(True)
    print("peak rise on the kernels %d B, one slot-row matrix %d B, allowance by arithmetic %d B" % (new, bound, legit))
    assert new < bound, (new, bound)
    assert new <= legit, (new, legit)
    assert rise(False) >= 2 * bound                           # the other route: the rows and their gradient


def test_recorded_dmplrp_step_replays_on_the_kernels(gpu):
    from dualmessagepassing_amd import lrp
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.dp import FlatAdamW, FlatGradSync
    from dualmessagepassing_amd.harness import GraphedTrainStep, train_epoch
    from test_gpu_lrp_index import _pairs
    assert lrp.USE_POOL_KERNEL is True
    view = _pairs().lrp()
    orders = [np.random.default_rng(ep).permutation(len(view)) for ep in range(3)]
    th.manual_seed(7)
    base = build_model(**view.model_config(hid_dim=64, layers=2)).to(gpu)
    finals, steps = [], None
    for graphed in (False, True):
        model = copy.deepcopy(base)
        sync = FlatGradSync(model)
        opt = FlatAdamW([sync.flatten_parameters()], lr=2e-3, weight_decay=1e-5, amsgrad=True, capturable=graphed)
        start = sync.master.detach().clone()
        step = GraphedTrainStep(model, opt, sync, max_shapes=4) if graphed else None
        trace = []
        calls = lrp._PermProduct.calls
        ctx = step.steps.on_stream() if graphed else None
        if ctx is not None:
            ctx.__enter__()
        try:
            for order in orders:
                train_epoch(model, opt, view, 8, gpu, sync=sync, neg_slp=0.01, order=order, trace=trace, graph=step)
        finally:
            if ctx is not None:
                ctx.__exit__(None, None, None)
        th.cuda.synchronize()
        # two layers on two sides per step that ran (eager) or was recorded
        assert lrp._PermProduct.calls - calls >= 4, "the kernel route was not taken"
        finals.append((sync.master.detach().clone(), th.stack([t[0] for t in trace]).cpu(), sync.master.grad.detach().clone()))
        if graphed:
            steps = step.steps
    assert steps.replays >= 3 and steps.replays + steps.eager_calls == 6, (steps.replays, steps.eager_calls)
    (p0, l0, g0), (p1, l1, g1) = finals
    assert th.allclose(l0, l1, rtol=1e-5, atol=1e-6), (l0, l1)
    assert th.allclose(p0, p1, rtol=1e-5, atol=1e-6), float((p0 - p1).abs().max())
    assert th.allclose(g0, g1, rtol=1e-5, atol=1e-6), float((g0 - g1).abs().max())
    assert float((p0 - start).abs().max()) > 1e-4
