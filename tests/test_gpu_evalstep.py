"""The recorded evaluation pass on the GPU: ``dmp_eval_terms`` against a float64 restatement and against ``eval_terms_tensor`` on
the same device inputs, then ``evaluate_epoch(graph=GraphedEvalStep)`` against the eager pass -- on a uniform dataset (bit
for bit), on its resident view, on a ragged dataset (padded batches, SURVEY 8(c)'s 2e-4), between two training steps (no
stale state in a recording), with matching heads, through one object for two datasets, and inside ``fit``."""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch as th

import util_resident
from conftest import ROOT

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")


# ----------------------------------------------------------------------------- the kernel
def _pair_weights(layout, n):
    if layout == "null":
        return None
    i = th.arange(n)
    return {"ones": th.ones(n), "prefix": (i < (n + 1) // 2).float(), "interleaved": (i % 2 == 0).float(), "zeros": th.zeros(n)}[layout]


def _inputs(n, layout, heads, Lc, extra, seed):
    g = th.Generator().manual_seed(seed)
    pred_c, target = th.randn(n, 1, generator=g) * 3, th.randint(0, 6, (n, 1), generator=g).float()
    made = []
    for k in range(2):
        if k >= heads:
            made.append(None)
            continue
        store = th.randn(n, Lc + extra, generator=g) * 2
        w = th.randint(0, 5, (n, Lc), generator=g)
        w[0, 0] = 2 ** 24 + 1              # a weight fp32 has to round
        made.append((store, w))
    return pred_c, target, _pair_weights(layout, n), made


def _on(gpu, pred_c, target, pw, made, Lc):
    heads = [None if m is None else (m[0].to(gpu)[:, :Lc], m[1].to(gpu)) for m in made]       # a view: row stride Lc + extra
    return pred_c.to(gpu), target.to(gpu), (None if pw is None else pw.to(gpu).view(-1, 1)), heads


def _run(fn, gpu, args, cursor, cap, launches=2):
    from dualmessagepassing_amd.harness import EvalBuffers
    pred_c, target, pw, heads = args
    buf = EvalBuffers(cap, gpu)
    buf.rows.fill_(NAN)
    buf.cursor.fill_(cursor)
    for _ in range(launches):
        assert fn(pred_c, target, heads, buf, pair_weights=pw) is buf.sums
    return buf


def _restate(pred_c, target, pw, made, Lc, launches):
    """float64 on the host: compacted rows and sums of ``launches`` identical batches."""
    real = th.ones(pred_c.numel(), dtype=th.bool) if pw is None else pw.view(-1) != 0
    p = th.relu(pred_c.view(-1))
    e = (p - target.view(-1))[real].double()                       # formed in fp32, as the product forms it
    a = e.abs()
    sums = th.stack([real.sum().double(), a.sum(), (e * e).sum(), th.where(a < 1, 0.5 * e * e, a - 0.5).sum()]) * launches
    errs = [None if m is None else (th.relu(m[0][:, :Lc].double()) - m[1].double()).abs().sum(dim=1)[real] for m in made]
    return p[real], target.view(-1)[real], errs, sums


def _check(buf, ref, n, Lc, cursor, cap, launches, exact_only=False):
    pred, target, errs, sums = ref
    real = pred.numel()
    rows = buf.rows.cpu()
    end = cursor + launches * real
    assert buf.cursor.item() == end and buf.overflow.item() == int(end > cap)
    written = th.arange(cap)
    written = (written >= cursor) & (written < end)
    for k, want in enumerate([pred, target] + errs):
        col = rows[k]
        if want is None:
            assert col.isnan().all()
            continue
        assert col[~written].isnan().all() and not col[written].isnan().any()
        want = want.repeat(launches)[:max(0, min(end, cap) - cursor)]
        if k < 2:
            assert th.equal(col[written], want)
        else:                              # the terms are non-negative: a row's sum of absolute terms is its value
            assert ((col[written].double() - want).abs() <= (Lc + 2) * U * want).all()
    got = buf.sums.cpu()
    assert got[0].item() == sums[0].item() == launches * real
    assert ((got - sums).abs() <= n * 2.0 ** -52 * sums).all(), (got, sums)


@pytest.fixture
def routes(monkeypatch):
    """``(kernel route, tensor route)``: while the first runs, a fall through to the tensor ops is an error."""
    from dualmessagepassing_amd import harness
    tensor_route = harness.eval_terms_tensor

    def kernel_route(*a, **kw):
        with monkeypatch.context() as m:
            m.setattr(harness, "eval_terms_tensor", lambda *a, **kw: pytest.fail("the kernel refused a batch it covers"))
            return harness.eval_terms(*a, **kw)
    return kernel_route, tensor_route


def _case(gpu, routes, n, layout, heads, Lc, extra, cursor, seed):
    kernel, tensor = routes
    host = _inputs(n, layout, heads, Lc, extra, seed)
    args = _on(gpu, *host, Lc)
    real = n if host[2] is None else int(host[2].sum())
    cap = cursor + 2 * real + 3
    a, b = _run(kernel, gpu, args, cursor, cap), _run(kernel, gpu, args, cursor, cap)
    _check(a, _restate(*host, Lc, 2), n, Lc, cursor, cap, 2)
    assert th.equal(a.rows.view(th.int32), b.rows.view(th.int32)) and th.equal(a.sums, b.sums)          # a bitwise repeat
    # the tensor route on the same device inputs, its row sums in float64 (the heads' predictions widened; pred_c stays fp32:
    # the error terms are formed in fp32 on both routes) -- the bounds of the restatement apply as they stand
    wide = args[:3] + ([None if h is None else (h[0].double(), h[1]) for h in args[3]],)
    c = _run(tensor, gpu, wide, cursor, cap)
    assert th.equal(a.rows[:2].view(th.int32), c.rows[:2].view(th.int32)) and th.equal(a.cursor, c.cursor) and th.equal(a.overflow, c.overflow)
    ea, ec = a.rows[2:].double(), c.rows[2:].double()
    assert th.equal(ea.isnan(), ec.isnan())
    live = ~ea.isnan()
    assert ((ea[live] - ec[live]).abs() <= (Lc + 2) * U * ec[live]).all()
    assert ((a.sums - c.sums).abs() <= n * 2.0 ** -52 * c.sums).all()
    return host, args, real


NS = (1, 63, 64, 65, 255, 256, 257, 1025)
LAYOUTS = ("ones", "prefix", "interleaved", "zeros", "null")
LCS = (1, 3, 64, 65, 257)


@pytest.mark.parametrize("n", NS)
def test_kernel_over_batch_sizes_and_weight_layouts(gpu, routes, n):
    for j, layout in enumerate(LAYOUTS):
        k = NS.index(n) + j
        _case(gpu, routes, n, layout, heads=k % 3, Lc=LCS[k % 5], extra=3 * (k % 2), cursor=7 * ((k // 2) % 2), seed=1000 * n + j)


@pytest.mark.parametrize("Lc", LCS)
def test_kernel_over_row_lengths_strides_and_heads(gpu, routes, Lc):
    for extra in (0, 3):
        for heads in (0, 1, 2):
            for cursor, layout in ((0, "interleaved"), (7, "null")):
                _case(gpu, routes, 257 if Lc < 257 else 65, layout, heads, Lc, extra, cursor, seed=Lc + extra + heads)


@pytest.mark.parametrize("layout", ["interleaved", "null"])
def test_kernel_at_the_end_of_the_buffers(gpu, routes, layout):
    kernel, tensor = routes
    n, Lc = 257, 5
    host = _inputs(n, layout, 2, Lc, 3, seed=5)
    args = _on(gpu, *host, Lc)
    real = n if host[2] is None else int(host[2].sum())
    ref = _restate(*host, Lc, 1)
    for route in (kernel, tensor):
        for cursor in (0, 7):
            fit = _run(route, gpu, args, cursor, cursor + real, launches=1)            # an exact fit: no flag
            _check(fit, ref, n, Lc, cursor, cursor + real, 1)
            assert fit.overflow.item() == 0
            short = _run(route, gpu, args, cursor, cursor + real - 1, launches=1)      # one row short: the flag, the rows below cap
            _check(short, ref, n, Lc, cursor, cursor + real - 1, 1)
            assert short.overflow.item() == 1 and short.cursor.item() == cursor + real
            assert th.equal(short.rows[:, cursor:].view(th.int32), fit.rows[:, cursor:cursor + real - 1].view(th.int32))
    # storage right behind the buffers stays as it was: the buffers as the first rows of a larger allocation
    from dualmessagepassing_amd.harness import EvalBuffers
    buf = EvalBuffers(real - 1, gpu)
    big = th.full((4, 2 * real), NAN, device=gpu)
    buf.rows = big[:, :real - 1]                                    # columns behind cap belong to the same rows of ``big``
    # (row stride 2 * real: the kernel addresses each row by its own pointer)
    buf.pred, buf.target, buf.err = buf.rows[0], buf.rows[1], (buf.rows[2], buf.rows[3])
    kernel(args[0], args[1], args[3], buf, pair_weights=args[2])
    assert buf.overflow.item() == 1 and big[:, real - 1:].isnan().all() and not big[:, :real - 1].isnan().any()


# ----------------------------------------------------------------------------- end to end
def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


@functools.lru_cache(maxsize=None)
def _uniform():
    from dualmessagepassing_amd.harness import SyntheticPairs
    return SyntheticPairs(44, 4, 4, 12, 36, 2, 1, seed=5)


def _model(gpu, ds, weights=False, seed=0):
    """The bench's DMPNN configuration at the dataset's sizes, the heads' zero-initialised last layers given values."""
    from dualmessagepassing_amd.basemodel import build_model
    bench = _bench()
    s = ds.shape
    cfg = dict(bench.CFG, p_nodes=s["p_nodes"], p_edges=s["p_edges"], g_nodes=s["g_nodes"], g_edges=s["g_edges"],
               p_labels=max(s["n_vlabels"], s["n_elabels"]), g_labels=max(s["n_vlabels"], s["n_elabels"]))
    config = bench.model_config(cfg)
    if weights:
        config["pred_return_weights"] = "node,edge"
    th.manual_seed(seed)
    model = build_model(**config)
    with th.no_grad():
        for head in model.pred_net.values():
            for lin in [head.pred_fc2] + ([head.weight_fc2] if weights else []):
                lin.weight.uniform_(-0.3, 0.3)
                lin.bias.uniform_(0.0, 0.5)
    return model.to(gpu)


def _same_pass(got, eager):
    assert th.equal(got["pred"], eager["pred"]) and th.equal(got["counts"], eager["counts"])
    assert got["AUC"] == eager["AUC"] or (got["AUC"] != got["AUC"] and eager["AUC"] != eager["AUC"])
    n = len(eager["pred"])
    for k in ("MAE", "MSE", "eval_metric"):
        assert abs(got[k] - eager[k]) <= n * U * max(1.0, abs(eager[k])), (k, got[k], eager[k])


def test_recorded_pass_is_the_eager_pass_on_a_uniform_dataset_and_its_resident_view(gpu):
    from dualmessagepassing_amd.harness import GraphedEvalStep, evaluate_epoch
    ds = _uniform()
    model = _model(gpu, ds)
    eager = evaluate_epoch(model, ds, 8, gpu)
    assert (eager["pred"] > 0).any()
    batches = -(-len(ds) // 8)
    step = GraphedEvalStep(model)
    got = evaluate_epoch(model, ds, 8, gpu, graph=step)
    assert not step._pad_spec                                   # uniform: no padding
    _same_pass(got, eager)
    # full batches: one eager call, one recording, then replays; the short last batch runs eagerly
    assert step.steps.replays >= batches - 2, (step.steps.replays, step.steps.eager_calls)
    scalars = evaluate_epoch(model, ds, 8, gpu, graph=step, collect=False)
    assert set(scalars) == {"MAE", "MSE", "RMSE", "eval_metric"} and all(scalars[k] == got[k] for k in scalars)
    view = ds.resident(gpu)
    sent, replays = view.uploads, step.steps.replays
    again = evaluate_epoch(model, view, 8, gpu, graph=step)
    _same_pass(again, eager)
    assert view.uploads == sent + batches and step.steps.replays >= replays + batches - 1


def test_recorded_pass_on_padded_batches_leaves_the_inert_pairs_out(gpu):
    from dualmessagepassing_amd.harness import GraphedEvalStep, evaluate_epoch
    ds = util_resident.ragged_pairs()
    model = _model(gpu, ds)
    eager = evaluate_epoch(model, ds, 16, gpu)
    step = GraphedEvalStep(model)
    got = evaluate_epoch(model, ds, 16, gpu, graph=step)
    assert step._pad_spec and step.steps.replays >= 1           # ragged: every batch padded to one of four levels
    assert len(got["pred"]) == len(ds) and th.equal(got["counts"], eager["counts"])       # no inert pair anywhere
    assert step.buffers.sums[0].item() == len(ds) == step.buffers.cursor.item()
    scale = max(1.0, float(eager["pred"].abs().max()))
    assert float((got["pred"] - eager["pred"]).abs().max()) <= 2e-4 * scale


def test_a_recording_follows_the_parameters_between_training_steps(gpu):
    from dualmessagepassing_amd.dp import FlatAdamW, FlatGradSync
    from dualmessagepassing_amd.harness import GraphedEvalStep, GraphedTrainStep, evaluate_epoch
    ds = _uniform()
    model = _model(gpu, ds, seed=1)
    sync = FlatGradSync(model)
    opt = FlatAdamW([sync.flatten_parameters()], lr=1e-2, weight_decay=1e-5, amsgrad=True, capturable=True)
    train = GraphedTrainStep(model, opt, sync)
    step = GraphedEvalStep(model, steps_like=train.steps)
    assert step.steps.stream is train.steps.stream
    with train.steps.on_stream():
        first = evaluate_epoch(model, ds, 8, gpu, graph=step)
        replays = step.steps.replays
        for k in range(2):
            train(ds, np.arange(8 * k, 8 * k + 8), gpu, neg_slp=0.01)
        second = evaluate_epoch(model, ds, 8, gpu, graph=step)
        assert step.steps.replays >= replays + len(ds) // 8              # every full batch a replay now
        eager = evaluate_epoch(model, ds, 8, gpu)
    assert not th.equal(first["pred"], second["pred"])
    _same_pass(second, eager)


def test_one_step_object_takes_two_datasets_of_different_length(gpu):
    from dualmessagepassing_amd.harness import GraphedEvalStep, evaluate_epoch
    ds = _uniform()
    short = ds.subset(range(5, 25))
    model = _model(gpu, ds)
    step = GraphedEvalStep(model)
    for d in (short, ds, short):
        _same_pass(evaluate_epoch(model, d, 8, gpu, graph=step), evaluate_epoch(model, d, 8, gpu))
        assert step.buffers.overflow.item() == 0
    assert step.buffers.cap == len(ds) and step.steps.replays >= 1


def test_recorded_pass_with_matching_heads(gpu):
    from dualmessagepassing_amd.harness import GraphedEvalStep, evaluate_epoch
    ds = _uniform()
    model = _model(gpu, ds, weights=True)
    want = ("node", "edge")
    eager = evaluate_epoch(model, ds, 8, gpu, match_weights=want)
    step = GraphedEvalStep(model, match_weights=want)
    got = evaluate_epoch(model, ds, 8, gpu, graph=step)
    _same_pass(got, eager)
    assert step.steps.replays >= len(ds) // 8 - 2
    for key, mean, Lc in (("NED", "MNED", ds.shape["g_nodes"]), ("EED", "MEED", 2 * ds.shape["g_edges"])):
        assert float(eager[key].abs().sum()) > 0
        assert ((got[key] - eager[key]).abs() <= (Lc + 2) * U * eager[key]).all(), key
        assert abs(got[mean] - eager[mean]) <= ((Lc + 2) * U + len(ds) * U) * max(1.0, eager[mean])
    for k in ("pred_v", "pred_e", "node_weights", "edge_weights"):
        assert k in eager and k not in got


def test_fit_with_a_recorded_dev_pass_trains_the_same_model(gpu, tmp_path):
    from dualmessagepassing_amd import dataio, harness
    from dualmessagepassing_amd.dp import FlatAdamW, FlatGradSync
    ds = _uniform()
    train, dev = ds.subset(range(32)), ds.subset(range(32, 44))
    base = _model(gpu, ds, seed=2)
    hist, made = {}, []
    real = harness.GraphedEvalStep

    class Counting(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    for mode in ("eager-dev", "recorded-dev"):
        model = copy.deepcopy(base)
        sync = FlatGradSync(model)
        opt = FlatAdamW([sync.flatten_parameters()], lr=1e-3, weight_decay=1e-5, amsgrad=True, capturable=True)
        harness.GraphedEvalStep = Counting
        try:
            hist[mode] = harness.fit(model, opt, train, dev, 2, 8, gpu, sync=sync, seed=1, graph=True, save_dir=str(tmp_path / mode),
                                     **({"eval_graph": True} if mode == "recorded-dev" else {}))
        finally:
            harness.GraphedEvalStep = real
    assert len(made) == 1 and made[0].steps.replays >= 1          # the recorded dev pass ran, on fit's own step object
    for a, b in zip(hist["eager-dev"], hist["recorded-dev"]):
        assert a["train"] == b["train"]
        for k in ("MAE", "MSE"):
            assert abs(a["dev"][k] - b["dev"][k]) <= len(dev) * U * max(1.0, abs(a["dev"][k])), (k, a["dev"], b["dev"])
    for epoch in range(2):         # evaluation does not touch the parameters
        s0, s1 = (th.load(dataio.checkpoint_path(str(tmp_path / mode), epoch), map_location="cpu") for mode in hist)
        assert s0.keys() == s1.keys() and all(th.equal(s0[k], s1[k]) for k in s0)


def test_refusals_on_the_gpu(gpu):
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.harness import GraphedEvalStep
    ds = _uniform()
    seq = build_model(ds.model_config(hid_dim=64, rep_net="CNN", rep_cnn_batch_norm=False)).to(gpu)
    with pytest.raises(ValueError, match="edge-sequence"):
        GraphedEvalStep(seq)
