"""The device-resident dataset view on the GPU (``PairDataset.resident``, ``dmp_collate_resident``): every batch of the case
list equals the host path's tensor by tensor; every output element is written, the same way twice; above the slot limit the
host path answers; a recorded training run and an evaluation on the view are the runs on the plain dataset."""
import copy

import numpy as np
import pytest
import torch as th

import util_resident

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def views(gpu):
    made = {}

    def get(name):
        if name not in made:
            ds, cases = util_resident.cases(name)
            made[name] = (ds, ds.resident(gpu), cases)
        return made[name]
    return get


def _assert_same_batch(got, ref, what):
    (meta, tensors), (meta_ref, tensors_ref) = got, ref
    assert meta == meta_ref, (what, meta, meta_ref)
    assert len(tensors) == len(tensors_ref), what
    for k, (g, r) in enumerate(zip(tensors, tensors_ref)):
        assert g.dtype == r.dtype and g.shape == r.shape and g.device == r.device, (what, k, g.dtype, r.dtype, g.shape, r.shape)
        if g.dtype == th.bool:                       # the flags byte for byte: any non-zero byte reads as True
            g, r = g.view(th.uint8), r.view(th.uint8)
        assert th.equal(g, r), (what, k)


@pytest.mark.parametrize("name", ["ragged", "tiny", "subset"])
def test_every_batch_of_the_case_list_is_the_host_paths(gpu, views, name):
    from dualmessagepassing_amd.harness import PairDataset
    ds, view, cases = views(name)
    assert type(view).graphs_from_arrays.__func__ is PairDataset.graphs_from_arrays.__func__
    assert view.samples is ds.samples and view.shape is ds.shape and len(view) == len(ds)
    assert view.pad_buckets(16) == ds.pad_buckets(16) and view.sub_capacity(16) == ds.sub_capacity(16) and view.model_config() == ds.model_config()
    elements = sum(np.asarray(x[k][f]).size for x in ds.samples for k in util_resident.SIDES for f in ("src", "dst", "vlabel", "elabel", "eid", "rev"))
    elements += sum(x["subisomorphisms"].size for x in ds.samples) + 6 * (len(ds) + 1)
    assert 0 < view.nbytes < 8 * elements                        # narrower than the int64 arrays the host path uploads
    sent = view.uploads
    for what, indices, pad, subs in cases:
        got = view.batch_arrays(np.asarray(indices), gpu, pad=pad, subs=subs)
        _assert_same_batch(got, ds.batch_arrays(indices, gpu, pad=pad, subs=subs), what)
    assert view.uploads == sent + len(cases)                     # one plan per batch, nothing else goes up


def test_a_subset_of_the_view_is_resident_too(gpu, views):
    ds, view, _ = views("ragged")
    part = view.subset(range(10, 30))
    assert type(part) is type(view) and len(part) == 20 and part.nbytes < view.nbytes
    _assert_same_batch(part.batch_arrays(list(range(16)), gpu), ds.subset(range(10, 30)).batch_arrays(list(range(16)), gpu), "subset of the view")


def _short_padded_batch(views):
    ds, view, cases = views("ragged")
    what, indices, pad, subs = next(c for c in cases if c[0] == "pad-short+subs")
    return ds, view, indices, pad, subs


def test_every_output_element_is_written(gpu, views):
    """Case 2's short batch with ``subs``, through the binding into buffers that hold a sentinel byte in every position."""
    ds, view, indices, pad, subs = _short_padded_batch(views)
    meta, plan, info = view.plan(indices, pad=pad, subs=subs)
    out = view.alloc_outputs(info, True, subs)
    for t in out:
        t.view(th.uint8).fill_(0xA5)
    view.launch(th.from_numpy(plan).to(gpu), info, out, True, subs)
    _assert_same_batch((meta, out), ds.batch_arrays(indices, gpu, pad=pad, subs=subs), "sentinel")


def test_two_calls_give_bitwise_equal_outputs(gpu, views):
    ds, view, indices, pad, subs = _short_padded_batch(views)
    a = view.batch_arrays(indices, gpu, pad=pad, subs=subs)
    b = view.batch_arrays(indices, gpu, pad=pad, subs=subs)
    _assert_same_batch(a, b, "second call")
    assert all(x.data_ptr() != y.data_ptr() for x, y in zip(a[1], b[1]) if x.numel())


def test_above_the_slot_limit_the_host_path_answers(gpu, views):
    from dualmessagepassing_amd import _abi, _lib
    ds, view, _ = views("tiny")
    indices = np.arange(_abi.DMP_RESIDENT_MAX_SLOTS + 1) % len(ds)
    sent = view.uploads
    got = view.batch_arrays(indices, gpu)
    assert view.uploads == sent                                  # no plan went up: the host path built the batch
    _assert_same_batch(got, ds.batch_arrays(indices, gpu), "above the limit")
    at = indices[:-1]                                            # the limit itself is the kernel's
    _assert_same_batch(view.batch_arrays(at, gpu), ds.batch_arrays(at, gpu), "at the limit")
    assert view.uploads == sent + 1
    meta, plan, info = view.plan(indices)
    with pytest.raises(_lib.DmpError, match="DMP_ERR_UNSUPPORTED"):          # the entry point refuses before it launches
        view.launch(th.from_numpy(plan).to(gpu), info, view.alloc_outputs(info, False), False)
    # a batch for another device and an empty batch are the host path's too
    assert view.batch_arrays([0, 1], "cpu")[1][0].device.type == "cpu"


# ----------------------------------------------------------------------------- training and evaluation
def _base_model(ds):
    from dualmessagepassing_amd.basemodel import build_model
    th.manual_seed(0)
    base = build_model(**ds.model_config(hid_dim=16, layers=2, pred_return_weights="node,edge"))
    with th.no_grad():          # the heads' last layers start as zeros: let the matching terms see their inputs
        for head in base.pred_net.values():
            for lin in (head.pred_fc2, head.weight_fc2):
                lin.weight.uniform_(-0.3, 0.3)
                lin.bias.uniform_(-0.1, 0.1)
    return base


def _train(ds, base, gpu, epochs=2, B=16):
    from dualmessagepassing_amd.dp import FlatAdamW, FlatGradSync
    from dualmessagepassing_amd.harness import GraphedTrainStep, train_epoch
    model = copy.deepcopy(base).to(gpu)
    sync = FlatGradSync(model)
    opt = FlatAdamW([sync.flatten_parameters()], lr=2e-4, weight_decay=1e-5, amsgrad=True, capturable=True)
    step = GraphedTrainStep(model, opt, sync, max_shapes=4, match_weights=("node", "edge"))
    losses = []
    with step.steps.on_stream():
        for ep in range(epochs):
            r = train_epoch(model, opt, ds, B, gpu, sync=sync, neg_slp=0.01, match_loss_w=1.0, match_reg_w=0.01,
                            order=np.random.default_rng(ep).permutation(len(ds)), match_weights=("node", "edge"), graph=step)
            losses.append(r["bp_loss"])
    th.cuda.synchronize()
    return losses, sync.master.detach().clone(), step, model


def _assert_trains_like_the_plain_dataset(ds, view, gpu, epochs=2):
    """The recorded run on ``view`` against the same run on ``ds``: bit for bit where the run on ``ds`` repeats itself bit for bit,
    else under the rule tests/test_gpu_ragged_replay.py applies between its two runs (parameters within 2e-4 of their largest
    magnitude, epoch losses within 2e-3 relative, absolute below 1).  -> the model trained on the view."""
    base = _base_model(ds)
    (l0, p0, _, _), (l1, p1, _, _) = _train(ds, base, gpu, epochs), _train(ds, base, gpu, epochs)
    sent = view.uploads
    l2, p2, step, model = _train(view, base, gpu, epochs)
    assert step._pad_spec and step.steps.replays > 0, (step.steps.replays, step.steps.eager_calls)
    assert view.uploads >= sent + epochs * (len(ds) // 16)
    exact = th.equal(p0, p1) and l0 == l1
    print("plain run repeats bit for bit:", exact, " losses", l0, l2, " parameter deviation", float((p0 - p2).abs().max()))
    if exact:
        assert th.equal(p0, p2) and l0 == l2, (l0, l2, float((p0 - p2).abs().max()))
    else:
        scale = float(p0.abs().max())
        assert float((p0 - p2).abs().max()) <= 2e-4 * scale, float((p0 - p2).abs().max()) / scale
        for a, b in zip(l0, l2):
            assert abs(a - b) <= 2e-3 * max(1.0, abs(a)), (l0, l2)
    return model


def test_a_recorded_matching_run_on_a_dataset_without_rows(gpu):
    """``SmallLikePairs`` keeps no subisomorphism rows: ``sub_capacity`` is 0, the recorded matching step takes an EMPTY
    ``sub_flat`` (no device address) and an all-zero ``sample_ptr`` -- on the view as on the plain dataset."""
    from dualmessagepassing_amd.harness import SmallLikePairs
    ds = SmallLikePairs(32, seed=7, threads=4)
    assert ds.sub_capacity(16) == 0
    view = ds.resident(gpu)
    meta, tensors = view.batch_arrays(np.arange(16), gpu, pad=ds.pad_buckets(16), subs=0)
    assert tensors[-2].shape == (0,) and tensors[-2].dtype == th.int64 and tensors[-1].shape == (33,) and not tensors[-1].any()
    _assert_trains_like_the_plain_dataset(ds, view, gpu)


def test_a_recorded_run_on_the_view_is_the_run_on_the_plain_dataset(gpu, views):
    """Two epochs at batch 16 through ``GraphedTrainStep(max_shapes=4, match_weights=("node", "edge"))``.  The batches are bit
    identical (the tests above), so where the plain run repeats itself bit for bit the view's run must equal it bit for bit;
    otherwise the rule of tests/test_gpu_ragged_replay.py between its two runs holds: parameters within 2e-4 of their largest
    magnitude, epoch losses within 2e-3 relative (absolute below 1).  Then ``evaluate_epoch`` with matching on both: equal."""
    from dualmessagepassing_amd.harness import evaluate_epoch
    ds, view, _ = views("ragged")
    model = _assert_trains_like_the_plain_dataset(ds, view, gpu)
    want = ("node", "edge")
    e0, e1 = evaluate_epoch(model, ds, 16, gpu, match_weights=want), evaluate_epoch(model, ds, 16, gpu, match_weights=want)
    e2 = evaluate_epoch(model, view, 16, gpu, match_weights=want)
    assert set(e2) == set(e0) and {"MNED", "MEED", "pred_v", "pred_e", "node_weights", "edge_weights"} <= set(e0)
    same = lambda a, b: (th.equal(a, b) if th.is_tensor(a) else (a == b or (a != a and b != b)))
    # the evaluation sums in a fixed order: the plain dataset's repeats itself bit for bit, and the view's batches are the
    # plain dataset's, so nothing but equality is asked for (no tolerance of this test's own)
    assert all(same(e0[k], e1[k]) for k in e0), [k for k in e0 if not same(e0[k], e1[k])]
    for k in e0:
        assert same(e0[k], e2[k]), k
