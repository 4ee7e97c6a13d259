"""The recorded evaluation pass without a GPU: the new ABI entry (header, export table, ``_abi``), ``eval_terms_tensor``
against plain Python loops in float64, and ``evaluate_epoch(graph=GraphedEvalStep)`` against the eager pass on a CPU device.
No model of the package runs on a CPU (the collate is a kernel already), so the end-to-end half uses a stand-in: a
``PairDataset`` whose ``graphs_from_arrays`` hands the batch's size vectors over as they are, a model in tensor ops on those,
and a tensor-op ``subiso_weights``; everything between them -- ``batch_arrays``, padding, pair weights, the step, the
buffers, ``eval_terms``, the metrics -- is the product's."""
import ctypes
import math
import os
import types

import numpy as np
import pytest
import torch

import util_header
import util_resident
from conftest import ROOT

U = 2.0 ** -24


def test_the_header_the_library_and_the_binding_declare_the_entry():
    from dualmessagepassing_amd import _abi, _lib
    h = util_header.read(os.path.join(ROOT, "include", "dmp_hip.h"))
    assert "dmp_eval_terms" in h.functions and "dmp_eval_terms" in _abi.SIGNATURES
    res, args = h.signature(_abi, "dmp_eval_terms")
    got_res, got_args = _abi.SIGNATURES["dmp_eval_terms"]
    assert got_res is res is ctypes.c_int
    assert len(got_args) == len(args) == 21 and all(g is w for g, w in zip(got_args, args))
    assert _abi.ABI_VERSION == h.defines["DMP_ABI_VERSION"] == 97          # an entry was added, no signature changed
    lib = _lib.load()
    none = [None, None, None, 4, None, 0, None, 0, None, None, 0, None, 0, None, None, 8, None, None, None, None, None]
    assert lib.dmp_eval_terms(*none) == -1
    big = [64, 64, None, (1 << 22) + 1, None, 0, None, 0, None, None, 0, None, 0, None, 64, 8, 64, 64, 64, 64, None]
    assert lib.dmp_eval_terms(*big) == -2                                  # refused on the host, before any launch


# ---------------------------------------------------------------- eval_terms_tensor against loops
def _layouts(n):
    return {"ones": [1.0] * n, "prefix": [1.0] * (n // 2) + [0.0] * (n - n // 2), "interleaved": [float(i % 2 == 0) for i in range(n)],
            "zeros": [0.0] * n}


def _loops(pred_c, target, pw, heads, cursor, cap, sentinel):
    """Plain Python in float64: the rows of a buffer of ``cap`` rows that started as ``sentinel``."""
    pred_out, target_out = [sentinel] * cap, [sentinel] * cap
    errs = [[sentinel] * cap for _ in heads]
    sums, row = [0.0, 0.0, 0.0, 0.0], cursor
    for i in range(len(pred_c)):
        if pw is not None and pw[i] == 0:
            continue
        p = max(float(pred_c[i]), 0.0)
        if row < cap:
            pred_out[row], target_out[row] = p, float(target[i])
            for k, (hp, hw) in enumerate(heads):
                errs[k][row] = sum(abs(max(float(x), 0.0) - float(w)) for x, w in zip(hp[i], hw[i]))
        e = float(np.float32(np.float32(p) - np.float32(target[i])))
        sums[0] += 1
        sums[1] += abs(e)
        sums[2] += e * e
        sums[3] += 0.5 * e * e if abs(e) < 1 else abs(e) - 0.5
        row += 1
    return pred_out, target_out, errs, sums, row


def _filled(cap, value, cursor):
    from dualmessagepassing_amd.harness import EvalBuffers
    buf = EvalBuffers(cap, "cpu")
    buf.rows.fill_(value)
    buf.cursor.fill_(cursor)
    return buf


def _same(got, want, sentinel, tol=None):
    for g, w in zip(got.tolist(), want):
        if w == sentinel:
            assert g == sentinel
        elif tol is None:
            assert g == w
        else:
            assert abs(g - w) <= tol(w), (g, w)


@pytest.mark.parametrize("Lc", [1, 7])
@pytest.mark.parametrize("n", [1, 5, 64])
def test_eval_terms_tensor_is_the_loops(n, Lc):
    from dualmessagepassing_amd.harness import eval_terms_tensor
    g = torch.Generator().manual_seed(100 * n + Lc)
    pred_c, target = torch.randn(n, 1, generator=g) * 3, torch.randint(0, 5, (n, 1), generator=g).float()
    heads = [(torch.randn(n, Lc, generator=g) * 2, torch.randint(0, 4, (n, Lc), generator=g)) for _ in range(2)]
    for name, pw in _layouts(n).items():
        for cursor in (0, 3):
            real = int(sum(pw))
            for cap in {cursor + real, cursor + real + 2, max(cursor + real - 1, cursor)}:       # exact fit, room, one row short
                buf = _filled(cap, -7.0, cursor)
                out = eval_terms_tensor(pred_c, target, heads, buf, pair_weights=torch.tensor(pw).view(n, 1))
                assert out is buf.sums
                want = _loops(pred_c.view(-1).tolist(), target.view(-1).tolist(), pw, [(a.tolist(), b.tolist()) for a, b in heads], cursor, cap, -7.0)
                _same(buf.pred, want[0], -7.0)
                _same(buf.target, want[1], -7.0)
                for k in (0, 1):       # fp32 row sums against float64: the terms' roundings and Lc - 1 additions
                    _same(buf.err[k], want[2][k], -7.0, tol=lambda w: (Lc + 2) * U * abs(w))
                assert buf.sums[0].item() == want[3][0] == real
                for k in (1, 2, 3):
                    assert abs(buf.sums[k].item() - want[3][k]) <= n * 2.0 ** -52 * want[3][k]
                assert buf.cursor.item() == want[4] == cursor + real           # the cursor advances past cap as well
                assert buf.overflow.item() == int(cursor + real > cap), (name, cursor, cap)
    # pair_weights None is the all-ones layout; one head only; two batches in a row accumulate
    buf, ref = _filled(2 * n + 1, -7.0, 1), _filled(2 * n + 1, -7.0, 1)
    for b in (buf, buf):
        eval_terms_tensor(pred_c, target, [None, heads[1]], b)
    for _ in range(2):
        eval_terms_tensor(pred_c, target, [None, heads[1]], ref, pair_weights=torch.ones(n))
    assert torch.equal(buf.rows, ref.rows) and torch.equal(buf.sums, ref.sums) and buf.cursor.item() == 2 * n + 1
    assert torch.equal(buf.err[0], torch.full((2 * n + 1,), -7.0)) and torch.equal(buf.pred[1:n + 1], buf.pred[n + 1:])
    assert buf.overflow.item() == 0


def test_eval_terms_on_a_cpu_device_is_the_tensor_route():
    from dualmessagepassing_amd.harness import eval_terms, eval_terms_tensor
    pred_c, target = torch.tensor([1.5, -2.0, 0.25]), torch.tensor([1.0, 0.0, 3.0])
    a, b = _filled(4, 0.0, 0), _filled(4, 0.0, 0)
    eval_terms(pred_c, target, (), a)
    eval_terms_tensor(pred_c, target, (), b)
    assert torch.equal(a.rows, b.rows) and torch.equal(a.sums, b.sums) and a.cursor.item() == 3
    assert a.sums.tolist() == [3.0, 0.5 + 0.0 + 2.75, 0.25 + 2.75 ** 2, 0.125 + 2.25]
    with pytest.raises(ValueError):
        eval_terms(pred_c, target, (None, None, None), a)


# ---------------------------------------------------------------- the step on a CPU device
class _CpuPairs:
    """Mixed into ``PairDataset``: the batch's arrays handed over as they are (the product's collate is a kernel)."""

    @classmethod
    def graphs_from_arrays(cls, meta, tensors):
        out = []
        for side, (n, e, max_n, max_e) in enumerate(meta[:2]):
            src, dst, nn_, ne_, nid, vlabel, eid, elabel, rev = tensors[side * 9:(side + 1) * 9]
            out.append(types.SimpleNamespace(num_nodes=nn_, num_edges=ne_, max_nodes=max_n, max_edges=max_e))
        return tuple(out)


def _cpu_pairs(ds):
    from dualmessagepassing_amd.harness import PairDataset
    cls = type("CpuPairs", (_CpuPairs, PairDataset), {})
    return cls(ds.samples, ds.shape)


def _cpu_subiso_weights(pattern, graph, sub_flat, sample_ptr, which, validate=True, work_hint=0):
    """How often each target node occurs in a pair's subisomorphism rows, [B, max nodes] int64 (node) and the same numbers
    doubled over [B, max edges] (edge): a stand-in with the product's shapes."""
    B = graph.num_nodes.numel()
    pos = torch.arange(sub_flat.numel())
    pair = torch.bucketize(pos, sample_ptr[1:], right=True)
    live = pos < sample_ptr[-1]
    node = torch.zeros(B, graph.max_nodes, dtype=torch.int64)
    node.index_put_((pair[live], sub_flat[live]), torch.ones(int(live.sum()), dtype=torch.int64), accumulate=True)
    edge = torch.zeros(B, graph.max_edges, dtype=torch.int64)
    width = min(graph.max_nodes, graph.max_edges)
    edge[:, :width] = 2 * node[:, :width]
    edge *= torch.arange(graph.max_edges).view(1, -1) < graph.num_edges.view(-1, 1)       # nothing behind a pair's last edge
    return (node if "node" in which else None), (edge if "edge" in which else None)


class _Model(torch.nn.Module):
    """pred_c from the pairs' sizes (both signs), per-position predictions that are zero behind a graph's last node / edge."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([0.37, -1.3, 0.21]))
        self.gate_capacity = 5

    def forward(self, pattern, graph):
        assert self.gate_capacity is None and not self.training and not torch.is_grad_enabled()
        pn, gn, ge = pattern.num_nodes.float(), graph.num_nodes.float(), graph.num_edges.float()
        pred_c = (self.w[0] * gn * ge / pn + self.w[1] * pn + self.w[2]).view(-1, 1)
        out = {"pred_c": pred_c}
        for key, mk, sizes, L in (("pred_v", "g_v_mask", graph.num_nodes, graph.max_nodes), ("pred_e", "g_e_mask", graph.num_edges, graph.max_edges)):
            cols = torch.arange(L).view(1, -1)
            out[mk] = cols < sizes.view(-1, 1)
            out[key] = torch.where(out[mk], 0.1 * pred_c + 0.45 * cols - 0.6, torch.zeros(()))
        return out

    refine_node_weights = refine_edge_weights = staticmethod(lambda w, use_max=False: w)


@pytest.fixture
def cpu_route(monkeypatch):
    from dualmessagepassing_amd import harness
    monkeypatch.setattr(harness, "subiso_weights", _cpu_subiso_weights)
    return harness


def _mean_bound(n, value):
    """The worst case of the eager route's fp32 mean over n terms (the recorded route's fp64 sum is the tighter one)."""
    return n * U * max(1.0, abs(value))


@pytest.mark.parametrize("pad", ["auto", None])
@pytest.mark.parametrize("match", [(), ("node", "edge")])
def test_the_step_on_a_cpu_device_gives_the_eager_pass(cpu_route, match, pad):
    harness = cpu_route
    ds, model = _cpu_pairs(util_resident.tiny_pairs()), _Model()
    eager = harness.evaluate_epoch(model, ds, 2, "cpu", match_weights=match or None)
    step = harness.GraphedEvalStep(model, match_weights=match, pad=pad)
    got = harness.evaluate_epoch(model, ds, 2, "cpu", graph=step)
    assert model.gate_capacity == 5
    assert (step._pad_spec not in (None, False)) == (pad == "auto")          # four pairs of four sizes: padded with "auto"
    assert torch.equal(got["pred"], eager["pred"]) and torch.equal(got["counts"], eager["counts"])
    assert (got["pred"] == 0).any() and (got["pred"] > 0).any()
    for k in ("MAE", "MSE", "eval_metric"):
        assert abs(got[k] - eager[k]) <= _mean_bound(len(ds), eager[k])
    assert got["RMSE"] == got["MSE"] ** 0.5 and got["AUC"] == eager["AUC"]
    assert step.buffers.sums[0].item() == len(ds) == step.buffers.cursor.item()
    for key, mean, L in (("NED", "MNED", max(x["graph"]["num_nodes"] for x in ds.samples)),
                         ("EED", "MEED", max(len(x["graph"]["src"]) for x in ds.samples))):
        assert (key in got) == (key in eager) == bool(match)
        if match:
            assert eager[key].abs().sum() > 0
            # a row's sum of absolute terms is the row's value itself
            assert ((got[key] - eager[key]).abs() <= (L + 2) * U * eager[key].abs()).all()
            assert abs(got[mean] - eager[mean]) <= (L + 2) * U * eager[mean] + _mean_bound(len(ds), eager[mean])
    for k in ("pred_v", "pred_e", "node_weights", "edge_weights"):
        assert k not in got
    scalars = harness.evaluate_epoch(model, ds, 2, "cpu", graph=step, collect=False)
    assert set(scalars) == {"MAE", "MSE", "RMSE", "eval_metric"} and all(scalars[k] == got[k] for k in scalars)


def test_one_step_object_takes_datasets_of_different_length(cpu_route):
    harness = cpu_route
    ds, model = _cpu_pairs(util_resident.tiny_pairs()), _Model()
    short = _cpu_pairs(ds.subset([3, 1]))
    step = harness.GraphedEvalStep(model)
    for d in (short, ds, short):
        got, eager = harness.evaluate_epoch(model, d, 2, "cpu", graph=step), harness.evaluate_epoch(model, d, 2, "cpu")
        assert torch.equal(got["pred"], eager["pred"]) and torch.equal(got["counts"], eager["counts"]) and len(got["pred"]) == len(d)
        assert step.buffers.overflow.item() == 0
    assert step.buffers.cap == len(ds)            # grown once, then kept for the shorter pass


def test_the_refusals(cpu_route, monkeypatch):
    harness = cpu_route
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.seqmodel import EdgeSeqModel
    base = util_resident.tiny_pairs()
    seq = build_model(base.model_config(hid_dim=8, layers=1, rep_net="CNN"))
    assert isinstance(seq, EdgeSeqModel)
    with pytest.raises(ValueError, match="edge-sequence"):
        harness.GraphedEvalStep(seq)
    with pytest.raises(ValueError, match="eval_metric"):
        harness.GraphedEvalStep(_Model(), eval_metric="nope")
    ds, model = _cpu_pairs(base), _Model()
    step = harness.GraphedEvalStep(model)
    with pytest.raises(ValueError, match="another model"):
        harness.evaluate_epoch(_Model(), ds, 2, "cpu", graph=step)
    with pytest.raises(ValueError, match="match_weights"):
        harness.evaluate_epoch(model, ds, 2, "cpu", graph=step, match_weights=("node",))
    with pytest.raises(RuntimeError, match="begin"):
        harness.GraphedEvalStep(model)(ds, np.arange(2), "cpu")
    # an LRP view outside the device index build, as GraphedTrainStep refuses it
    view = base.lrp(4)
    monkeypatch.setattr(view, "max_degree", 10 ** 6)
    with pytest.raises(ValueError, match="device index build"):
        harness.evaluate_epoch(model, view, 2, "cpu", graph=harness.GraphedEvalStep(model))
    # a pass that loses a batch: the cursor does not reach len(dataset)
    calls = []
    real_call = harness.GraphedEvalStep.__call__
    monkeypatch.setattr(harness.GraphedEvalStep, "__call__",
                        lambda self, *a: calls.append(1) if len(calls) == 0 else real_call(self, *a))
    with pytest.raises(RuntimeError, match="result rows"):
        harness.evaluate_epoch(model, ds, 2, "cpu", graph=step)
    monkeypatch.setattr(harness.GraphedEvalStep, "__call__", real_call)
    # result buffers one row short: the overflow word
    step.begin(len(ds), "cpu")
    step.buffers.cap -= 1
    for i in (0, 2):
        step(ds, np.arange(i, i + 2), "cpu")
    with pytest.raises(RuntimeError, match="result buffers"):
        step.results(len(ds))


def test_stepgraph_takes_a_stream_and_fit_an_eval_graph_flag():
    import inspect
    from dualmessagepassing_amd import dp, harness
    assert inspect.signature(dp.StepGraph.__init__).parameters["stream"].default is None
    marker = object()
    assert dp.StepGraph(lambda: None, stream=marker)._stream is marker
    assert inspect.signature(harness.fit).parameters["eval_graph"].default is False
    sig = inspect.signature(harness.evaluate_epoch).parameters
    assert sig["graph"].default is None and sig["collect"].default is True
    assert math.isclose(U, 2.0 ** -24)
