"""The device-built permutation index (csrc/dmp_lrp.hip, ``PermIndex.from_batched``) and the LRP / DMPLRP training path on it.

* the index of every ``lrp_layer_*`` / ``lrp_model_*`` fixture equals the one read from the reference's own matrices, and the
  one ``from_graphs`` enumerates on a hand-made batch (empty graph, single node, degrees 0 .. 4 with parallel, antiparallel
  and reversed edges, a node of 9 neighbours) for L = 1 .. 6, with and without an ``is_reversed`` frame: ``torch.equal``;
* the neighbour cap (32 on the kernels, 33 through the host build), capacities above and below the total, two runs bit-equal;
* ``model(pattern, graph)`` reproduces the model fixtures (tolerances of tests/test_gpu_lrp.py: 2e-4 / 3e-4);
* ``train_epoch`` / ``evaluate_epoch`` / ``fit`` / ``evaluate_run`` over ``PairDataset.lrp()``, against a hand loop on the
  8-argument form with ``from_graphs`` indexes (loss per step rtol 1e-5 / atol 1e-6);
* a recorded DMPLRP step replays batches whose permutation totals differ and ends where the eager run ends (rtol 1e-5 /
  atol 1e-6, as tests/test_gpu_mem.py)."""
import copy
import json
import os

import numpy as np
import pytest
import torch as th

from conftest import golden_files, load_golden
from test_gpu_lrp import _close, _graph, _sparse, _t

pytestmark = pytest.mark.gpu


def _same(a, b):
    assert a.seq_len == b.seq_len and a.num_nodes == b.num_nodes and a.num_edges == b.num_edges and a.num_perms == b.num_perms
    assert th.equal(a.sizes, b.sizes), "sizes"
    assert th.equal(a.scale, b.scale), "scale"
    assert a.slot.dtype == th.int64 and th.equal(a.slot, b.slot), "slot"


def _kernels_only(monkeypatch):
    from dualmessagepassing_amd.lrp import PermIndex

    def refuse(*a, **k):
        raise AssertionError("the host build was taken")
    monkeypatch.setattr(PermIndex, "_build_host", classmethod(refuse))


# ----------------------------------------------------------------------------- the reference's own matrices
@pytest.mark.parametrize("path", golden_files("lrp_layer_") + golden_files("lrp_model_"))
def test_index_equals_the_reference_matrices(path, gpu, monkeypatch):
    from dualmessagepassing_amd.lrp import PermIndex
    _kernels_only(monkeypatch)
    d = load_golden(path)
    if "lrp_model_" in path:
        L = int({str(k): str(v) for k, v in zip(d["config_keys"], d["config_vals"])}.get("lrp_seq_len", 4))
        sides = [("p", "p_"), ("g", "g_")]
    else:
        L = int(dict(zip(d["kw_keys"].tolist(), d["kw_vals"].tolist())).get("lrp_seq_len", 4))
        sides = [("g", "")]
    assert sides
    for t, pre in sides:
        ref = PermIndex.from_sparse(_sparse(d, pre + "pool", gpu), _sparse(d, pre + "n2p", gpu), _sparse(d, pre + "e2p", gpu), L)
        got = PermIndex.from_batched(_graph(d, t, gpu), L)
        _same(got, ref)
        assert int(got.status.item()) == 0 and got.live is None
        _same(PermIndex.from_batched(_graph(d, t, gpu), L, total=ref.num_perms), ref)
        with pytest.raises(ValueError, match="total"):
            PermIndex.from_batched(_graph(d, t, gpu), L, total=ref.num_perms + 1)


# ----------------------------------------------------------------------------- a hand-made batch against from_graphs
def _hand_graphs():
    """(src, dst, n, is_reversed) with local ids: no node; one node; five nodes with out-degrees 0 .. 4 (node 0's only
    out-edge is a reversed one; 2 -> 1 twice, the later edge wins; 1 -> 2 / 2 -> 1 antiparallel); twelve nodes, node 0 with
    nine distinct neighbours."""
    z = np.zeros(0, np.int64)
    g5 = [(4, 0), (2, 1), (4, 1), (3, 0), (0, 4), (4, 2), (3, 1), (2, 0), (1, 2), (4, 3), (3, 2), (2, 1)]
    r5 = [False, False, False, False, True, False, False, False, False, False, False, False]
    g12 = [(0, k) for k in (5, 1, 9, 3, 7, 2, 8, 4, 6)] + [(10, 11), (11, 10), (5, 0), (3, 7), (0, 5), (7, 3), (6, 0), (9, 10)]
    r12 = [False] * 9 + [False, False, False, False, False, True, True, False]
    out = [(z, z, 0, np.zeros(0, bool)), (z, z, 1, np.zeros(0, bool))]
    for edges, rev, n in ((g5, r5, 5), (g12, r12, 12)):
        s, t = (np.array(x, np.int64) for x in zip(*edges))
        out.append((s, t, n, np.array(rev, bool)))
    return out


def _hand_batch(gpu, with_rev, graphs=None):
    from dualmessagepassing_amd.graph import BatchedGraph
    graphs = graphs or _hand_graphs()
    offs = np.concatenate([[0], np.cumsum([g[2] for g in graphs])])
    src = np.concatenate([g[0] + o for g, o in zip(graphs, offs)])
    dst = np.concatenate([g[1] + o for g, o in zip(graphs, offs)])
    g = BatchedGraph(_t(src).to(gpu), _t(dst).to(gpu), int(offs[-1]), _t(np.array([g[2] for g in graphs], np.int64)).to(gpu),
                     _t(np.array([len(g[0]) for g in graphs], np.int64)).to(gpu))
    if with_rev:
        g.edata["is_reversed"] = _t(np.concatenate([g_[3] for g_ in graphs])).to(gpu)
    return g


_REFS = {}


def _hand_ref(gpu, L, with_rev):
    from dualmessagepassing_amd.lrp import PermIndex
    if (L, with_rev) not in _REFS:
        graphs = [g if with_rev else g[:3] for g in _hand_graphs()]
        _REFS[(L, with_rev)] = PermIndex.from_graphs(graphs, gpu, L)
    return _REFS[(L, with_rev)]


@pytest.mark.parametrize("with_rev", [True, False])
@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 6])
def test_index_equals_the_enumeration_on_a_hand_made_batch(L, with_rev, gpu, monkeypatch):
    from dualmessagepassing_amd.lrp import PermIndex
    _kernels_only(monkeypatch)
    ref = _hand_ref(gpu, L, with_rev)
    g = _hand_batch(gpu, with_rev)
    got = PermIndex.from_batched(g, L)
    _same(got, ref)
    assert PermIndex.from_batched(g, L) is got                          # one index per graph object and seq_len
    sizes = got.sizes.cpu().tolist()
    assert sizes[0] == 1 and sizes[1] == 1                              # the single node; node 0 of the third graph
    nine = 1
    for k in range(min(L - 1, 9)):
        nine *= 9 - k
    assert sizes[6] == nine
    sums = PermIndex.from_batched(_hand_batch(gpu, with_rev), L, pooling="sum")
    assert th.equal(sums.slot, ref.slot) and th.equal(sums.scale, th.ones_like(ref.scale))


def test_self_loop_is_refused(gpu):
    from dualmessagepassing_amd.lrp import PermIndex
    graphs = _hand_graphs()
    s, t, n, r = graphs[2]
    graphs[2] = (np.append(s, 3), np.append(t, 3), n, np.append(r, False))
    with pytest.raises(ValueError, match="self-loop"):
        PermIndex.from_batched(_hand_batch(gpu, True, graphs), 4)
    graphs[2] = (graphs[2][0], graphs[2][1], n, np.append(r, True))     # as a reversed edge it is no neighbour
    _same(PermIndex.from_batched(_hand_batch(gpu, True, graphs), 4), PermIndex.from_graphs(graphs, gpu, 4))


# ----------------------------------------------------------------------------- the neighbour cap
def _star(k):
    extra = [(1, 0), (2, 1), (1, 2)]
    s, t = (np.array(x, np.int64) for x in zip(*([(0, j) for j in range(k, 0, -1)] + extra)))
    return (s, t, k + 1, np.zeros(len(s), bool))


def test_star_at_the_neighbour_cap_runs_on_the_kernels(gpu, monkeypatch):
    from dualmessagepassing_amd.lrp import PermIndex
    graphs = [_star(32), _hand_graphs()[2]]
    ref = PermIndex.from_graphs(graphs, gpu, 3)
    assert int(ref.sizes[0]) == 992
    _kernels_only(monkeypatch)
    _same(PermIndex.from_batched(_hand_batch(gpu, True, graphs), 3), ref)


def test_star_above_the_neighbour_cap_takes_the_host_build(gpu):
    from dualmessagepassing_amd.lrp import PermIndex
    graphs = [_hand_graphs()[2], _star(33)]
    ref = PermIndex.from_graphs(graphs, gpu, 3)
    assert int(ref.sizes[5]) == 33 * 32
    _same(PermIndex.from_batched(_hand_batch(gpu, True, graphs), 3), ref)          # decided from the status word
    hinted = _hand_batch(gpu, True, graphs)
    hinted.lrp_max_degree = 33                                                     # decided from the dataset's degrees
    _same(PermIndex.from_batched(hinted, 3, total=ref.num_perms), ref)
    _same(PermIndex.from_batched(_hand_batch(gpu, True), 7), PermIndex.from_graphs(_hand_graphs(), gpu, 7))    # L out of range


# ----------------------------------------------------------------------------- capacity
def test_capacity_above_and_below_the_total(gpu, monkeypatch):
    from dualmessagepassing_amd import _abi
    from dualmessagepassing_amd.lrp import PermIndex
    _kernels_only(monkeypatch)
    L = 4
    ref = _hand_ref(gpu, L, True)
    P, zero = ref.num_perms, ref.num_nodes + ref.num_edges
    runs = []
    for _ in range(2):
        big = PermIndex.from_batched(_hand_batch(gpu, True), L, capacity=P + 7)
        assert big.num_perms == P + 7 and big.slot.numel() == (P + 7) * L * L
        assert th.equal(big.slot[:P * L * L], ref.slot) and bool((big.slot[P * L * L:] == zero).all())
        assert th.equal(big.sizes, ref.sizes) and th.equal(big.scale, ref.scale)
        assert int(big.status.item()) == 0
        assert th.equal(big.live, (th.arange(P + 7, device=gpu) < P).float())
        runs.append(big)
    assert th.equal(runs[0].slot, runs[1].slot) and th.equal(runs[0].sizes, runs[1].sizes) and th.equal(runs[0].scale, runs[1].scale)
    small = PermIndex.from_batched(_hand_batch(gpu, True), L, capacity=P - 1)
    assert small.num_perms == P - 1 and int(small.status.item()) == _abi.DMP_LRP_DROPPED
    assert th.equal(small.slot, ref.slot[:(P - 1) * L * L])
    hinted = _hand_batch(gpu, True)
    hinted.lrp_max_degree = 9                                           # the recorded step's form: nothing is read back
    none = PermIndex.from_batched(hinted, L, capacity=0)
    assert none.num_perms == 0 and none.slot.numel() == 0 and int(none.status.item()) == _abi.DMP_LRP_DROPPED


def test_capacity_tail_adds_nothing(gpu):
    """``perm_pool`` over an index at a capacity: outputs and every gradient are those of the exact index (the products run
    at another row count, so to rounding: rtol 1e-5 / atol 1e-6 of fp32 sums of a few hundred terms of size ~1; a tail that
    reached the bias gradient would add 37 terms of that size)."""
    from dualmessagepassing_amd.lrp import PermIndex, perm_pool
    L, hid = 3, 8
    exact = PermIndex.from_batched(_hand_batch(gpu, True), L)
    padded = PermIndex.from_batched(_hand_batch(gpu, True), L, capacity=exact.num_perms + 37)
    gen = th.Generator().manual_seed(1)
    outs = []
    for perm in (exact, padded):
        x = th.randn(exact.num_nodes, hid, generator=gen.manual_seed(1)).to(gpu).requires_grad_(True)
        z = th.randn(exact.num_edges, hid, generator=gen).to(gpu).requires_grad_(True)
        w = th.randn(hid, hid, L * L, generator=gen).to(gpu).requires_grad_(True)
        b = th.randn(hid, generator=gen).to(gpu).requires_grad_(True)
        coef = th.randn(exact.num_nodes, hid, generator=gen).to(gpu)
        out = perm_pool(perm, x, z, w, b, th.relu)
        (out * coef).sum().backward()
        outs.append((out.detach(), x.grad, z.grad, w.grad, b.grad))
    for a, b_, name in zip(outs[0], outs[1], ("out", "dx", "dz", "dw", "db")):
        assert th.allclose(a, b_, rtol=1e-5, atol=1e-6), (name, float((a - b_).abs().max()))
    assert float(outs[0][4].abs().max()) > 0


# ----------------------------------------------------------------------------- model(pattern, graph)
@pytest.mark.parametrize("path", golden_files("lrp_model_"))
def test_two_argument_call_reproduces_the_model_fixtures(path, gpu, monkeypatch):
    from dualmessagepassing_amd.basemodel import build_model
    _kernels_only(monkeypatch)
    d = load_golden(path)
    config = {str(k): eval(str(v)) for k, v in zip(d["config_keys"], d["config_vals"])}
    model = build_model(**config)
    model.load_state_dict({k[3:]: _t(v) for k, v in d.items() if k.startswith("sd.")}, strict=True)
    model.to(gpu)
    out = model(_graph(d, "p", gpu), _graph(d, "g", gpu))
    for k in ("p_v_rep", "p_e_rep", "g_v_rep", "g_e_rep", "pred_c"):
        _close(out[k], d["out." + k], 2e-4, k)
    out["pred_c"].sum().backward()
    n = 0
    for k, p in model.named_parameters():
        if "grad." + k in d:
            _close(p.grad, d["grad." + k], 3e-4, "grad " + k)
            n += 1
        else:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
    assert n > 10


# ----------------------------------------------------------------------------- the loop
def _pairs():
    from dualmessagepassing_amd.harness import SyntheticPairs
    return SyntheticPairs(16, 3, 3, 8, 16, 3, 3)


def _host_side(ds, idx, key):
    return [(ds.samples[i][key]["src"], ds.samples[i][key]["dst"], ds.samples[i][key]["num_nodes"], ds.samples[i][key]["rev"]) for i in idx]


@pytest.mark.parametrize("rep_net", ["LRP", "DMPLRP"])
def test_train_epoch_equals_a_hand_loop_on_the_eight_argument_form(rep_net, gpu):
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.dp import FlatAdamW, FlatGradSync
    from dualmessagepassing_amd.harness import count_loss, evaluate_epoch, train_epoch
    from dualmessagepassing_amd.lrp import PermIndex
    ds = _pairs()
    view = ds.lrp()
    th.manual_seed(3)
    base = build_model(**view.model_config(hid_dim=16, layers=2, rep_net=rep_net)).to(gpu)
    assert type(base).__name__ == rep_net

    def setup():
        model = copy.deepcopy(base)
        sync = FlatGradSync(model)
        return model, sync, FlatAdamW([sync.flatten_parameters()], lr=2e-3, weight_decay=1e-5, amsgrad=True)

    model, sync, opt = setup()
    start = sync.master.detach().clone()
    trace = []
    for _ in range(2):
        res = train_epoch(model, opt, view, 8, gpu, sync=sync, neg_slp=0.01, trace=trace)
        assert np.isfinite(res["bp_loss"]) and np.isfinite(res["eval_metric"])
    got = th.stack([t[0] for t in trace]).cpu()

    hand, hsync, hopt = setup()
    hand.train()
    want = []
    for _ in range(2):
        for i in range(0, len(ds), 8):
            idx = np.arange(i, i + 8)
            pattern, graph, counts, _w = ds.batchify(idx, gpu)
            hsync.detach_grads()
            out = hand(pattern, PermIndex.from_graphs(_host_side(ds, idx, "pattern"), gpu, 4), None, None,
                       graph, PermIndex.from_graphs(_host_side(ds, idx, "graph"), gpu, 4))
            loss = count_loss(out["pred_c"], counts, "MSE", 0.01)
            loss.backward()
            hsync.pack()
            hsync.sync()
            th.nn.utils.clip_grad_norm_(hsync.params, 8.0)
            hopt.step()
            want.append(loss.detach())
    want = th.stack(want).cpu()
    assert got.shape == want.shape == (4,) and float(want.max()) > 0.1
    assert th.allclose(got, want, rtol=1e-5, atol=1e-6), (got, want)
    assert float((sync.master.detach() - start).abs().max()) > 1e-4          # it trained

    ev = evaluate_epoch(model, view, 8, gpu)
    assert all(np.isfinite(ev[k]) for k in ("MAE", "MSE", "AUC")), {k: ev[k] for k in ("MAE", "MSE", "AUC")}

    # matching terms: the shared GraphAdjModelV2.forward hands out pred_v
    th.manual_seed(3)
    mbase = build_model(**view.model_config(hid_dim=16, layers=2, rep_net=rep_net, pred_return_weights="node")).to(gpu)
    losses = []
    for w in (0.0, 1.0):
        m = copy.deepcopy(mbase)
        msync = FlatGradSync(m)
        mopt = FlatAdamW([msync.flatten_parameters()], lr=2e-3, weight_decay=1e-5, amsgrad=True)
        mtrace = []
        train_epoch(m, mopt, view, 8, gpu, sync=msync, neg_slp=0.01, match_loss_w=w, match_reg_w=0.5 * w, match_weights=("node",), trace=mtrace)
        losses.append(th.stack([t[0] for t in mtrace]).cpu())
    assert bool(th.isfinite(losses[1]).all()) and float((losses[1] - losses[0]).abs().max()) > 1e-3, losses


def test_fit_then_evaluate_run(tmp_path, gpu):
    from dualmessagepassing_amd import dataio
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.dp import FlatGradSync
    from dualmessagepassing_amd.harness import evaluate_run, fit
    view = _pairs().lrp(3)
    train, dev = view.subset(range(12)), view.subset(range(12, 16))
    th.manual_seed(0)
    config = view.model_config(hid_dim=16, layers=2)
    model = build_model(**config).to(gpu)
    sync = FlatGradSync(model)
    opt = th.optim.AdamW(sync.params, lr=2e-3, weight_decay=1e-5, amsgrad=True)
    run = os.path.join(tmp_path, "run")
    hist = fit(model, opt, train, dev, 2, 8, gpu, save_dir=run, config=config, sync=sync)
    assert len(hist) == 2 and all(np.isfinite(h["train"]["bp_loss"]) and np.isfinite(h["dev"]["MAE"]) for h in hist)
    saved = dataio.load_config(os.path.join(run, "config.json"))
    assert saved["rep_net"] == "DMPLRP" and saved["lrp_seq_len"] == 3
    res = evaluate_run(run, {"dev": dev, "train": train}, gpu, batch_size=8, stamp="t")      # strict load inside
    for split, part in (("dev", dev), ("train", train)):
        assert np.isfinite(res[split]["MAE"])
        doc = json.load(open(os.path.join(run, "eval_%s_results_t.json" % split)))
        assert len(doc["prediction"]["pred_c"]) == len(part)
    layer = next(iter(build_model(**saved).g_rep_net["DMPLRP"]))
    assert layer.lrp_seq_len == 3 and layer.lrp_weight.shape[-1] == 9


# ----------------------------------------------------------------------------- the recorded step
def test_recorded_dmplrp_step_replays_batches_of_different_totals(gpu):
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.dp import FlatAdamW, FlatGradSync
    from dualmessagepassing_amd.harness import GraphedTrainStep, train_epoch
    view = _pairs().lrp()
    orders = [np.random.default_rng(ep).permutation(len(view)) for ep in range(3)]
    totals = {tuple(int(t) for t in view.perm_counts[o[i:i + 8]].sum(axis=0)) for o in orders for i in (0, 8)}
    assert len(totals) >= 5                                               # six batches, (almost) every one another total
    th.manual_seed(7)
    base = build_model(**view.model_config(hid_dim=16, layers=2)).to(gpu)
    finals, steps = [], None
    for graphed in (False, True):
        model = copy.deepcopy(base)
        sync = FlatGradSync(model)
        opt = FlatAdamW([sync.flatten_parameters()], lr=2e-3, weight_decay=1e-5, amsgrad=True, capturable=graphed)
        start = sync.master.detach().clone()
        step = GraphedTrainStep(model, opt, sync, max_shapes=4) if graphed else None
        trace = []
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
        finals.append((sync.master.detach().clone(), th.stack([t[0] for t in trace]).cpu()))
        if graphed:
            steps = step.steps
    assert steps.replays >= 3 and len(steps._graphs) <= 4 and steps.replays + steps.eager_calls == 6, (steps.replays, steps.eager_calls)
    (p0, l0), (p1, l1) = finals
    assert th.allclose(l0, l1, rtol=1e-5, atol=1e-6), (l0, l1)
    assert th.allclose(p0, p1, rtol=1e-5, atol=1e-6), float((p0 - p1).abs().max())
    assert float((p0 - start).abs().max()) > 1e-4


def test_padded_ragged_batches_replay_and_train_like_the_exact_shapes(gpu):
    """A ragged set: the recorded step pads its batches with inert pairs (every node of an inert ring graph has exactly
    one permutation: counted in closed form) and builds the indexes at a capacity level.  Against the eager run on the
    exact shapes: the packed gradient of the first step (same parameters, same pairs) within 1e-5 of its largest entry --
    fp32 sums of some 10^3 terms whose order changes with the row counts of the padded products --, and every epoch's loss
    within 2e-3 (the bound of tests/test_gpu_ragged_replay.py).  The parameters themselves are no stable measure here:
    AdamW moves a parameter whose gradient is rounding noise by up to lr per step, whatever the gradient's size."""
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.dp import FlatAdamW, FlatGradSync
    from dualmessagepassing_amd.harness import GraphedTrainStep, SmallLikePairs, train_epoch
    view = SmallLikePairs(64, seed=5, threads=4).lrp()
    B, epochs = 16, 3
    th.manual_seed(0)
    base = build_model(**view.model_config(hid_dim=16, layers=2)).to(gpu)
    finals, steps = [], None
    for graphed in (False, True):
        model = copy.deepcopy(base)
        sync = FlatGradSync(model)
        opt = FlatAdamW([sync.flatten_parameters()], lr=2e-4, weight_decay=1e-5, amsgrad=True, capturable=graphed)
        step = GraphedTrainStep(model, opt, sync, max_shapes=4) if graphed else None
        losses = []
        ctx = step.steps.on_stream() if graphed else None
        if ctx is not None:
            ctx.__enter__()
        try:
            train_epoch(model, opt, view, B, gpu, sync=sync, neg_slp=0.01, order=np.arange(B), graph=step)
            th.cuda.synchronize()
            first = sync.master.grad.detach().clone()
            for ep in range(epochs):
                r = train_epoch(model, opt, view, B, gpu, sync=sync, neg_slp=0.01, order=np.random.default_rng(ep).permutation(len(view)), graph=step)
                losses.append(r["bp_loss"])
        finally:
            if ctx is not None:
                ctx.__exit__(None, None, None)
        th.cuda.synchronize()
        finals.append((first, losses))
        if graphed:
            steps = step.steps
    assert steps.replays >= 3 and len(steps._graphs) <= 4, (steps.replays, steps.eager_calls)
    (g0, l0), (g1, l1) = finals
    scale = float(g0.abs().max())
    print("first-step gradient: largest entry %g, largest difference %g" % (scale, float((g0 - g1).abs().max())))
    assert scale > 1e-3 and float((g0 - g1).abs().max()) <= 1e-5 * scale, float((g0 - g1).abs().max()) / scale
    for a, b in zip(l0, l1):
        assert np.isfinite(a) and abs(a - b) <= 2e-3 * max(1.0, abs(a)), (l0, l1)
