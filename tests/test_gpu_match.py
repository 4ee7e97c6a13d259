"""The matching half of the training step and of the evaluation on the MI355X:

* ``dmp_match_loss`` (csrc/dmp_match.hip, through ``harness.match_terms``) against ``harness.match_terms_tensor`` in fp64 --
  the definition tests/test_match_cpu.py holds to the reference's ``_match_terms`` -- at 1e-5 relative to max(1, |ref|),
  over one element, a row length that is no multiple of four, a row stride larger than the row, more rows than one
  workgroup takes and a row longer than one wave's chunk; bitwise repeatable; every output element written; the tensor
  ops where the kernel refuses; an upstream gradient other than 1;
* ``collate.subiso_weights`` on subisomorphism rows padded to a capacity;
* a recorded step with matching terms (``GraphedTrainStep(match_weights=...)``) replays and trains like the eager step:
  per-step losses within 2e-3 and final parameters within 2e-4 of their scale, the figures tests/test_gpu_ragged_replay.py
  holds the count-only replay to (padded against exact shapes, re-associated sums);
* ``evaluate_epoch(match_weights=...)`` / ``evaluate_run`` against the reference's own ``evaluate_epoch``
  (tests/golden/match/, scripts/make_golden_match.py): integers exact, floats at 1e-4 (SURVEY §8(c)'s figure for
  full-model outputs, in its form |d| <= tol * max(1, |ref|) per element), the AUC exact.
"""
import copy
import itertools
import json
import os

import numpy as np
import pytest
import torch as th

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu
TOL = 1e-5
SHAPES = [(1, 1), (3, 7), (5, 64), (65, 513), (4, 4100)]


def _close(got, ref, tol, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs() - tol * ref.abs().clamp(min=1.0)
    assert bool((err <= 0).all()), "%s: worst excess %g over tol %g" % (what, float(err.max()), tol)


def make_inputs(B, Lc, dev, seed, front=0, inert=False, stride=0):
    """``pred`` [B, Lc] fp32 (a slice of a wider tensor with ``stride`` extra columns), int64 weights up to 1e4, a
    pre-padding mask with interior holes whose longest row leaves ``front`` columns unused (row 0: that longest row --
    fully live for front 0; row 1: no live column), ``pred_c`` of both signs, pair weights with zeros (``inert``; row 0, the
    longest, is inert in every second case so that the window is shorter than the longest row)."""
    g = th.Generator().manual_seed(seed)
    sizes = th.randint(0, Lc - front + 1, (B,), generator=g)
    sizes[0] = Lc - front
    if B > 1:
        sizes[1] = 0
    if B > 2:
        sizes[2] = max(1, (Lc - front) // 2)                       # row 2: live, and real in every case
    mask = th.arange(Lc).view(1, -1) >= (Lc - sizes).view(-1, 1)
    holes = th.rand(B, Lc, generator=g) < 0.2
    holes[0] = False                                               # row 0 keeps every position of its range
    mask = mask & ~holes
    wide = th.randn(B, Lc + stride, generator=g) * 3.0
    weights = th.randint(0, 10001, (B, Lc), generator=g)
    weights[:, ::2] = th.randint(0, 4, (B, (Lc + 1) // 2), generator=g)      # small weights too: the criteria's inner branches
    pred_c = th.randn(B, 1, generator=g)
    pw = None
    if inert:
        pw = (th.rand(B, generator=g) < 0.6).float()
        pw[0] = float(seed % 2)
        if B > 2:
            pw[2] = 1.0
    wide = wide.to(dev)
    return wide[:, :Lc], weights.to(dev), mask.to(dev), pred_c.to(dev), (None if pw is None else pw.to(dev))


def run_terms(fn, pred, weights, mask, pred_c, coef, bp, pw, dtype, upstream=1.0):
    p = pred.detach().to(dtype).requires_grad_(True)
    c = pred_c.detach().to(dtype).requires_grad_(True)
    total, loss, reg = fn(p, weights, mask, c, coef, bp, None if pw is None else pw.to(dtype))
    (total * upstream).backward()
    return total.detach(), loss.detach(), reg.detach(), p.grad, c.grad


CASES = [(B, Lc, bp, slope, inert) for (B, Lc), bp, slope, inert in
         itertools.product(SHAPES, ("MSE", "MAE", "SMSE"), (0.0, 0.01, 1.0), (False, True))]


@pytest.mark.parametrize("B,Lc,bp,slope,inert", CASES)
def test_kernel_matches_the_fp64_definition(gpu, B, Lc, bp, slope, inert):
    from dualmessagepassing_amd import harness
    seed = 7 * B + Lc + int(100 * slope) + len(bp)
    front = 0 if Lc < 4 or seed % 3 == 0 else min(Lc - 1, 5)                 # capacity columns in front in two cases of three
    stride = 3 if Lc == 64 else (1 if seed % 2 else 0)                       # (5, 64): rows no longer 16-byte aligned
    pred, weights, mask, pred_c, pw = make_inputs(B, Lc, gpu, seed, front, inert, stride)
    coef = th.tensor([slope, 0.7, 0.3], device=gpu)
    got = run_terms(harness.match_terms, pred, weights, mask, pred_c, coef, bp, pw, th.float32)
    ref = run_terms(harness.match_terms_tensor, pred, weights, mask, pred_c, coef.double(), bp, pw, th.float64)
    assert got[0].dtype == th.float32 and got[3].shape == (B, Lc) and got[4].shape == (B, 1)
    for name, a, b in zip(("total", "loss", "reg", "dpred", "dpred_c"), got, ref):
        _close(a, b, TOL, "%s %s" % (name, (B, Lc, bp, slope, inert, front)))
    # outside the window and on inert pairs: exact zeros
    real = th.ones(B, dtype=th.bool, device=gpu) if pw is None else pw != 0
    assert bool((got[3][~real] == 0).all()) and bool((got[4][~real] == 0).all())
    assert bool((got[3][ref[3] == 0] == 0).all())
    if B > 2:
        assert bool((ref[3] != 0).any()) and bool((ref[4] != 0).any())


def test_two_runs_are_bitwise_equal_and_every_element_is_written(gpu, monkeypatch):
    from dualmessagepassing_amd import fused, harness
    pred, weights, mask, pred_c, pw = make_inputs(65, 513, gpu, 5, front=9, inert=True, stride=1)
    coef = th.tensor([0.01, 1.0, 0.01], device=gpu)
    monkeypatch.setattr(fused, "POISON_DEAD_ROWS", False)
    a = run_terms(harness.match_terms, pred, weights, mask, pred_c, coef, "MSE", pw, th.float32)
    b = run_terms(harness.match_terms, pred, weights, mask, pred_c, coef, "MSE", pw, th.float32)
    monkeypatch.setattr(fused, "POISON_DEAD_ROWS", True)         # the output buffers start as NaN (DMP_POISON_DEAD_ROWS=1)
    c = run_terms(harness.match_terms, pred, weights, mask, pred_c, coef, "MSE", pw, th.float32)
    for x, y, z in zip(a, b, c):
        assert th.equal(x, y) and th.equal(x, z) and bool(th.isfinite(z).all())
    # no real pair at all: zeros, also under the poison
    none = run_terms(harness.match_terms, pred, weights, mask, pred_c, coef, "MSE", th.zeros(65, device=gpu), th.float32)
    for t in none:
        assert bool((t == 0).all())


def test_unsupported_shapes_fall_back_to_the_tensor_ops(gpu, monkeypatch):
    from dualmessagepassing_amd import _lib, harness
    lib = _lib.load()
    assert lib.dmp_match_loss_workspace_words(1 << 16, 1 << 15) == 0 and lib.dmp_match_loss_workspace_words(3, 7) > 0
    buf = th.zeros(64, device=gpu)
    p = buf.data_ptr()
    rc = lib.dmp_match_loss(p, 1 << 15, p, p, p, None, p, 1 << 16, 1 << 15, 0, p, p, p, p, _lib.stream_ptr())
    assert rc == -2, rc                                          # DMP_ERR_UNSUPPORTED, before any pointer is touched
    pred, weights, mask, pred_c, pw = make_inputs(5, 64, gpu, 3, front=2, inert=True)
    coef = th.tensor([0.01, 1.0, 0.5], device=gpu)
    want = run_terms(harness.match_terms_tensor, pred, weights, mask, pred_c, coef, "SMSE", pw, th.float32)

    def refuse(*a):
        raise AssertionError("the kernel was launched for a shape it refuses")

    monkeypatch.setattr(lib, "dmp_match_loss_workspace_words", lambda B, Lc: 0)
    monkeypatch.setattr(lib, "dmp_match_loss", refuse)
    got = run_terms(harness.match_terms, pred, weights, mask, pred_c, coef, "SMSE", pw, th.float32)
    for x, y in zip(got, want):
        assert th.equal(x, y)


def test_upstream_gradient_scales_the_seeds(gpu):
    from dualmessagepassing_amd import harness
    pred, weights, mask, pred_c, pw = make_inputs(5, 64, gpu, 8, front=4, inert=True, stride=4)
    coef = (0.01, 1.0, 0.25)                                      # three Python numbers
    got = run_terms(harness.match_terms, pred, weights, mask, pred_c, coef, "MSE", pw, th.float32, upstream=-2.5)
    ref = run_terms(harness.match_terms_tensor, pred, weights, mask, pred_c, coef, "MSE", pw, th.float64, upstream=-2.5)
    one = run_terms(harness.match_terms, pred, weights, mask, pred_c, coef, "MSE", pw, th.float32)
    for name, a, b in zip(("total", "loss", "reg", "dpred", "dpred_c"), got, ref):
        _close(a, b, TOL, name)
    assert th.equal(got[3], one[3] * -2.5) and bool((one[3] != 0).any())


# ----------------------------------------------------------------------------- datasets with subisomorphism rows
def ragged_pairs(num, seed):
    """Ragged (pattern, graph) pairs with their exact subisomorphism rows: patterns of 3 .. 4 nodes, graphs of 8, 12 or 16
    nodes with three edges per node.  Few distinct sizes on purpose: a Sum head adds its bias once per PADDED position
    (pred.py:93-156), so a batch's predictions depend on its padded length, and a padded batch (the dataset's longest rows)
    equals the exact-shape batch only when that batch holds a largest graph on every side -- which 16 pairs drawn from
    these sizes do (``_train_both`` asserts it for the orders it uses)."""
    from dualmessagepassing_amd import harness
    rng = np.random.default_rng(seed)
    shape = dict(p_nodes=4, p_edges=5, g_nodes=16, g_edges=48, n_vlabels=2, n_elabels=1)      # (about half of the pairs have matches)
    samples = []
    for _ in range(num):
        pn = int(rng.integers(3, 5)); pe = int(rng.integers(pn - 1, 6))
        gn = int(rng.choice([8, 12, 16])); ge = 3 * gn
        pu, pv = harness._er_edges(pn, pe, rng)
        gu, gv = harness._er_edges(gn, ge, rng)
        pvl, gvl = rng.integers(0, 2, pn), rng.integers(0, 2, gn)
        pel, gel = np.zeros(pe, np.int64), np.zeros(ge, np.int64)
        sub = harness.enumerate_subisomorphisms(pu, pv, pvl, pel, gu, gv, gvl, gel)
        samples.append({"pattern": harness.PairDataset._with_rev(pu, pv, pvl, pel, shape["p_edges"], 1),
                        "graph": harness.PairDataset._with_rev(gu, gv, gvl, gel, shape["g_edges"], 1),
                        "counts": len(sub), "subisomorphisms": sub})
    return harness.PairDataset(samples, shape)


@pytest.fixture(scope="module")
def ragged():
    return ragged_pairs(96, seed=21)


def test_subiso_weights_on_rows_padded_to_the_capacity(gpu, ragged):
    from dualmessagepassing_amd.collate import subiso_weights
    idx = np.arange(16, 32)
    assert sum(ragged.samples[i]["counts"] for i in idx) > 0
    want_n, want_e = ragged.batchify(idx, gpu, return_weights=("node", "edge"))[3]
    cap = ragged.sub_capacity(16)
    meta, tensors = ragged.batch_arrays(idx, gpu, subs=cap)
    assert int(tensors[-1][-1]) < cap                            # this batch leaves part of the capacity unused
    tensors[-2][int(tensors[-1][-1]):] = 3                       # whatever the tail holds, it belongs to no sample
    pattern, graph = ragged.graphs_from_arrays(meta, tensors)
    got_n, got_e = subiso_weights(pattern, graph, tensors[-2], tensors[-1], ("node", "edge"), work_hint=cap)
    assert th.equal(got_n, want_n) and th.equal(got_e, want_e) and int(want_n.sum()) > 0 and int(want_e.sum()) > 0
    # a padded batch: the real pairs' rows at the dataset's row length, zeros for the inert pairs
    pad = ragged.pad_buckets(16, levels=4)
    meta, tensors = ragged.batch_arrays(idx, gpu, pad=pad, subs=cap)
    pattern, graph = ragged.graphs_from_arrays(meta, tensors)
    pad_n, pad_e = subiso_weights(pattern, graph, tensors[-2], tensors[-1], ("node", "edge"), work_hint=cap)
    assert pad_n.shape == (32, pad["graph"][0]) and pad_e.shape == (32, pad["graph"][1])
    assert th.equal(pad_n[:16, -want_n.size(1):], want_n) and th.equal(pad_e[:16, -want_e.size(1):], want_e)
    assert int(pad_n.sum()) == int(want_n.sum()) and int(pad_e.sum()) == int(want_e.sum())


# ----------------------------------------------------------------------------- the recorded step
def _train_both(ds, gpu, pad, epochs=3, B=16, max_shapes=4):
    """The same run twice from deep copies of one model: ``train_epoch`` eagerly, and through a recorded step with both
    matching terms; annealed slope and regulariser weight.  -> (per-step losses, final flat parameters) of both, the step."""
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.dp import FlatAdamW, FlatGradSync
    from dualmessagepassing_amd.harness import GraphedTrainStep, RunSchedule, train_epoch
    th.manual_seed(0)
    base = build_model(**ds.model_config(hid_dim=16, layers=2, pred_return_weights="node,edge"))
    with th.no_grad():          # the heads' last layers start as zeros: let the matching terms see their inputs
        for head in base.pred_net.values():
            for lin in (head.pred_fc2, head.weight_fc2):
                lin.weight.uniform_(-0.3, 0.3)
                lin.bias.uniform_(-0.1, 0.1)
    config = {"train_batch_size": B, "train_epochs": epochs, "lr": 2e-4, "weight_decay": 1e-5, "scheduler": "constant",
              "neg_pred_slp": "anneal_cosine$1.0$0.01", "match_loss_w": 1.0, "match_reg_w": "anneal_cosine$0.01$0.0", "rep_reg_w": 0.0}
    orders = [np.random.default_rng(ep).permutation(len(ds)) for ep in range(epochs)]
    for order in orders:        # every batch holds a largest graph on every side (see ``ragged_pairs``)
        for k in range(0, len(ds), B):
            for key in ("pattern", "graph"):
                for size in (lambda g: g["num_nodes"], lambda g: len(g["src"])):
                    assert max(size(ds.samples[i][key]) for i in order[k:k + B]) == max(size(x[key]) for x in ds.samples)
    runs, step = [], None
    for graphed in (False, True):
        model = copy.deepcopy(base).to(gpu)
        sync = FlatGradSync(model)
        opt = FlatAdamW([sync.flatten_parameters()], lr=2e-4, weight_decay=1e-5, amsgrad=True, capturable=True)
        sched = RunSchedule(config, len(ds))
        if graphed:
            step = GraphedTrainStep(model, opt, sync, match_weights=("node", "edge"), pad=pad, max_shapes=max_shapes)
        trace = []
        ctx = step.steps.on_stream() if graphed else None
        if ctx is not None:
            ctx.__enter__()
        try:
            for ep in range(epochs):
                train_epoch(model, opt, ds, B, gpu, sync=sync, order=orders[ep], schedule=sched,
                            epoch=ep, match_weights=("node", "edge"), trace=trace, graph=step if graphed else None)
        finally:
            if ctx is not None:
                ctx.__exit__(None, None, None)
        th.cuda.synchronize()
        runs.append((np.array([float(a) for a, _ in trace]), sync.master.detach().clone()))
    return runs, step


def _assert_same_run(runs, step, n_steps, max_shapes):
    (l0, p0), (l1, p1) = runs
    assert len(l0) == len(l1) == n_steps
    assert step.steps.eager_calls <= max_shapes and step.steps.replays >= n_steps - 2 * max_shapes, (step.steps.eager_calls, step.steps.replays)
    worst = np.abs(l0 - l1) / np.maximum(1.0, np.abs(l0))
    print("per-step loss deviation:", np.round(worst, 6).tolist())
    scale = float(p0.abs().max())
    print("parameter deviation / scale:", float((p0 - p1).abs().max()) / scale)
    assert worst.max() <= 2e-3, worst.tolist()
    assert float((p0 - p1).abs().max()) <= 2e-4 * scale, float((p0 - p1).abs().max()) / scale


def test_recorded_matching_step_replays_on_ragged_batches(gpu, ragged):
    runs, step = _train_both(ragged, gpu, pad="auto")
    assert step._pad_spec, "the ragged dataset was not padded"
    _assert_same_run(runs, step, 18, 4)


def test_recorded_matching_step_replays_on_uniform_batches(gpu):
    """Uniform graphs, no padding: the subisomorphism rows differ in length from batch to batch, and only their fixed
    capacity makes the step's shape repeat."""
    from dualmessagepassing_amd.harness import SyntheticPairs
    ds = SyntheticPairs(96, 4, 4, 12, 36, 2, 1, seed=5)
    assert len({x["subisomorphisms"].size for x in ds.samples}) > 4
    runs, step = _train_both(ds, gpu, pad="auto")
    assert not step._pad_spec
    _assert_same_run(runs, step, 18, 4)
    assert step.steps.eager_calls == 1 and step.steps.replays == 17


def test_fit_replays_a_matching_run(gpu, ragged, monkeypatch):
    from dualmessagepassing_amd import harness
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.dp import FlatAdamW, FlatGradSync
    made = []

    class Recording(harness.GraphedTrainStep):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(harness, "GraphedTrainStep", Recording)
    th.manual_seed(0)
    model = build_model(**ragged.model_config(hid_dim=16, layers=2, pred_return_weights="node")).to(gpu)
    sync = FlatGradSync(model)
    opt = FlatAdamW([sync.flatten_parameters()], lr=2e-4, weight_decay=1e-5, amsgrad=True, capturable=True)
    train, dev = ragged.subset(range(80)), ragged.subset(range(80, 96))
    hist = harness.fit(model, opt, train, dev, 2, 16, gpu, sync=sync, seed=1, graph=True, match_weights="node", match_loss_w=1.0)
    assert len(made) == 1 and made[0].match_weights == ("node",)
    assert made[0].steps.replays >= 10 - 2 * 4 and made[0].steps.replays > 0, (made[0].steps.replays, made[0].steps.eager_calls)
    assert all(np.isfinite(h["train"]["bp_loss"]) for h in hist)


# ----------------------------------------------------------------------------- evaluation
def _fixture_run(name, gpu):
    """A fixture of scripts/make_golden_match.py -> (fixture, PairDataset, model with its state_dict, config)."""
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.harness import PairDataset
    d = load_golden(os.path.join(GOLDEN, "match", name + ".npz"))
    ne, nel = int(d["rev_max_ne"]), int(d["rev_max_nel"])
    samples = []
    for i in range(int(d["n"])):
        g = lambda k: d["%d.%s" % (i, k)]
        samples.append({"id": str(d["ids"][i]), "pattern": PairDataset._with_rev(g("pu"), g("pv"), g("pvl"), g("pel"), ne, nel),
                        "graph": PairDataset._with_rev(g("gu"), g("gv"), g("gvl"), g("gel"), ne, nel), "counts": len(g("sub")),
                        "subisomorphisms": np.asarray(g("sub"), np.int64).reshape(-1, len(g("pvl")))})
    config = json.loads(str(d["config_json"]))
    model = build_model(config)
    model.load_state_dict({k[3:]: th.from_numpy(np.asarray(v)) for k, v in d.items() if k.startswith("sd.")}, strict=True)
    return d, PairDataset(samples, {}), model.to(gpu), config


def _assert_matches_fixture(res, d, which):
    rt = lambda got, key: _close(th.as_tensor(np.asarray(got, np.float64)), th.as_tensor(np.asarray(d[key], np.float64)), 1e-4, key)
    assert np.array_equal(res["counts"].numpy(), d["counts"])
    _close(res["pred"], th.from_numpy(np.maximum(d["pred_c"], 0.0)), 1e-4, "relu(pred_c)")
    for k in ("MAE", "MSE", "RMSE"):
        rt(res[k], k)
    assert res["AUC"] == float(d["AUC"])                         # signs only: exact
    for pk, wk, ek, mk in (("pred_v", "node_weights", "NED", "MNED"), ("pred_e", "edge_weights", "EED", "MEED")):
        if pk[-1] not in which:
            assert pk not in res and ek not in res
            continue
        assert np.array_equal(res[wk].numpy(), d[wk]) and d[wk].size > 0 and d[wk].max() > 0          # integers: exact
        assert res[pk].shape == d[pk].shape
        rt(res[pk].numpy(), pk)
        rt(res[ek].numpy(), ek)
        rt(res[mk], mk)


@pytest.mark.parametrize("name,which", [("eval_dmpnn_node", "v"), ("eval_dmpnn_node_edge", "ve")])
def test_evaluate_epoch_matches_the_reference(gpu, name, which):
    from dualmessagepassing_amd import harness
    d, ds, model, _ = _fixture_run(name, gpu)
    plain = harness.evaluate_epoch(model, ds, int(d["batch"]), gpu)
    res = harness.evaluate_epoch(model, ds, int(d["batch"]), gpu, match_weights=str(d["match_weights"]))
    _assert_matches_fixture(res, d, which)
    for k in ("MAE", "MSE", "eval_metric", "RMSE", "AUC"):      # the count metrics do not depend on match_weights
        assert plain[k] == res[k]
    assert th.equal(plain["pred"], res["pred"]) and "NED" not in plain and "pred_v" not in plain


def test_evaluate_run_writes_the_matching_fields(gpu, tmp_path):
    from dualmessagepassing_amd import dataio, harness
    d, ds, model, config = _fixture_run("eval_dmpnn_node_edge", gpu)
    run = str(tmp_path)
    dataio.save_config(dict(config, match_weights=str(d["match_weights"]), eval_metric="MAE", eval_batch_size=int(d["batch"])),
                       os.path.join(run, "config.json"))
    th.save(model.state_dict(), dataio.checkpoint_path(run, 0))
    out = harness.evaluate_run(run, {"dev": ds}, gpu, epoch=0, stamp="t")
    np.testing.assert_allclose(out["dev"]["MAE"], float(d["MAE"]), rtol=1e-4)
    with open(os.path.join(run, "eval_dev_results_t.json")) as f:
        doc = json.load(f)
    assert doc["data"]["id"] == [str(x) for x in d["ids"]] and doc["data"]["counts"] == d["counts"].tolist()
    assert doc["data"]["node_weights"] == d["node_weights"].tolist() and doc["data"]["edge_weights"] == d["edge_weights"].tolist()
    for part, k in (("prediction", "pred_c"), ("prediction", "pred_v"), ("prediction", "pred_e"), ("error", "NED"), ("error", "EED")):
        assert len(doc[part][k]) == len(d[k]), k
    for k in ("MAE", "MSE", "RMSE", "MNED", "MEED"):
        np.testing.assert_allclose(doc["error"][k], float(d[k]), rtol=1e-4, err_msg=k)
    assert doc["error"]["AUC"] == float(d["AUC"])
    # told otherwise: the count fields alone
    harness.evaluate_run(run, {"dev": ds}, gpu, epoch=0, stamp="c", match_weights=())
    with open(os.path.join(run, "eval_dev_results_c.json")) as f:
        doc = json.load(f)
    assert "pred_v" not in doc["prediction"] and "NED" not in doc["error"] and "RMSE" in doc["error"]
