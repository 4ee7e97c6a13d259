"""The device-resident dataset view without a GPU: the new ABI entries (header against ``_abi``), the plan builder
(``resident.resident_plan``) executed by a numpy restatement of the kernel against ``PairDataset.batch_arrays`` on the CPU over
the whole case list, the host path's ``ValueError``s, and the refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch as th

import util_header
import util_resident
from conftest import ROOT


def test_the_header_and_the_binding_declare_the_same_resident_entries():
    from dualmessagepassing_amd import _abi
    h = util_header.read(os.path.join(ROOT, "include", "dmp_hip.h"))
    assert "dmp_collate_resident" in h.functions and "dmp_collate_resident" in _abi.SIGNATURES
    res, args = h.signature(_abi, "dmp_collate_resident")
    got_res, got_args = _abi.SIGNATURES["dmp_collate_resident"]
    assert got_res is res is ctypes.c_int
    assert len(got_args) == len(args) and all(g is w for g, w in zip(got_args, args))
    assert got_args[0] is ctypes.POINTER(_abi.dmp_resident_side) and got_args[7] is ctypes.POINTER(_abi.dmp_resident_batch)
    for name in ("dmp_resident_side", "dmp_resident_batch"):
        assert [(f, t) for f, t, *_ in getattr(_abi, name)._fields_] == h.fields(_abi, name)
    assert _abi.DMP_RESIDENT_MAX_SLOTS == h.defines["DMP_RESIDENT_MAX_SLOTS"] >= 2 * 1024
    assert _abi.ABI_VERSION == h.defines["DMP_ABI_VERSION"] == 97          # entries were added, no signature changed


def test_the_library_exports_the_entry_and_refuses_bad_arguments_on_the_host():
    from dualmessagepassing_amd import _abi, _lib
    lib = _lib.load()
    sides, batch = (_abi.dmp_resident_side * 2)(), (_abi.dmp_resident_batch * 2)()
    assert lib.dmp_collate_resident(None, None, None, None, None, 4, 2, None, None, None, None, 0, 0, None, None) == -1
    assert lib.dmp_collate_resident(sides, 64, None, None, 64, 0, 0, batch, 64, None, None, 0, 0, None, None) == -1        # no slot
    assert lib.dmp_collate_resident(sides, 64, None, None, 64, 4, 5, batch, 64, None, None, 0, 0, None, None) == -1        # real > slots
    assert lib.dmp_collate_resident(sides, 64, None, None, 64, 4, 2, batch, 64, None, 64, 8, 0, None, None) == -1          # half a tail
    # above the slot limit: refused before the (null) arrays of the sides are looked at
    assert lib.dmp_collate_resident(sides, 64, None, None, 64, _abi.DMP_RESIDENT_MAX_SLOTS + 1, 2, batch, 64, None, None, 0, 0, None, None) == -2


def _host(ds, indices, pad, subs):
    return ds.batch_arrays(indices, "cpu", pad=pad, subs=subs)


@pytest.mark.parametrize("name", ["ragged", "tiny", "subset"])
def test_an_executed_plan_is_the_host_paths_batch(name):
    from dualmessagepassing_amd.resident import resident_plan, resident_store
    ds, cases = util_resident.cases(name)
    store, sizes = resident_store(ds.samples)
    for what, indices, pad, subs in cases:
        meta_ref, ref = _host(ds, indices, pad, subs)
        meta, plan, info = resident_plan(sizes, indices, pad=pad, subs=subs, n_vlabels=ds.shape["n_vlabels"], n_elabels=ds.shape["n_elabels"])
        assert meta == meta_ref and all(type(v) is int for m in meta for v in m), (what, meta, meta_ref)
        assert plan.dtype == np.int64 and plan.ndim == 1 and plan.flags["C_CONTIGUOUS"] and len(plan) == 4 + 6 * info["slots"] + 5
        got = util_resident.run_plan(store, plan, info, pad is not None, subs)
        assert len(got) == len(ref), what
        for k, (g, r) in enumerate(zip(got, ref)):
            g = th.from_numpy(np.ascontiguousarray(g))
            assert g.dtype == r.dtype and g.shape == r.shape and th.equal(g, r), (what, k)


def test_the_case_list_reaches_the_first_and_the_last_capacity_level():
    """A guard on the case list itself (host path and test utility only: it says nothing about the view)."""
    ds, cases = util_resident.cases("ragged")
    level = {what: util_resident.level_of(_host(ds, indices, pad, subs)[0], pad) for what, indices, pad, subs in cases if pad is not None}
    assert level["pad-level1"] == 1 and level["pad-level4"] == 4, level
    assert ds.sub_capacity(16) > 0 and any(x["counts"] == 0 for x in ds.samples)


def test_the_store_is_narrow_and_counts_convert_as_torch_converts():
    from dualmessagepassing_amd.resident import resident_store
    ds = util_resident.ragged_pairs()
    store, sizes = resident_store(ds.samples)
    for key in util_resident.SIDES:
        assert all(store[key][k].dtype == np.int32 for k in ("src", "dst", "vlabel", "elabel", "eid")) and store[key]["rev"].dtype == np.uint8
        assert store[key]["node_ptr"][-1] == sizes[key][0].sum() == len(store[key]["vlabel"])
        assert store[key]["edge_ptr"][-1] == sizes[key][1].sum() == len(store[key]["src"])
    assert store["counts"].dtype == np.float32
    assert th.equal(th.from_numpy(store["counts"]), th.tensor([x["counts"] for x in ds.samples], dtype=th.float32))
    big = [dict(ds.samples[0], counts=2 ** 24 + 1)]          # not a float32: rounded as torch rounds it
    assert th.equal(th.from_numpy(resident_store(big)[0]["counts"]), th.tensor([2 ** 24 + 1], dtype=th.float32))
    assert store["sub_ptr"][-1] == len(store["subs"]) == sum(x["subisomorphisms"].size for x in ds.samples)


def test_the_host_paths_value_errors_are_raised_by_the_plan():
    from dualmessagepassing_amd.resident import resident_plan, resident_store
    ds = util_resident.ragged_pairs()
    _, sizes = resident_store(ds.samples)
    order = util_resident.by_size(ds)
    tight = dict(ds.pad_buckets(16, levels=4))
    tight["graph"] = (tight["graph"][0], 40)                 # a layout for smaller graphs than these: the largest fit no level
    busiest = sorted(range(len(ds)), key=lambda i: -ds.samples[i]["subisomorphisms"].size)[:4]
    for indices, pad, subs, text in ((list(range(17)), ds.pad_buckets(16, levels=4), None, "more pairs than the padding"),
                                     (order[-16:], tight, None, "does not fit 16 graphs"),
                                     (busiest, None, ds.samples[busiest[0]]["subisomorphisms"].size, "subisomorphism rows take")):
        with pytest.raises(ValueError, match=text) as ref:
            _host(ds, indices, pad, subs)
        with pytest.raises(ValueError, match=text) as got:
            resident_plan(sizes, indices, pad=pad, subs=subs, n_vlabels=16, n_elabels=16)
        assert str(got.value) == str(ref.value)
    # a batch of (nearly) empty graphs: an inert graph would have to be larger than the dataset's largest
    tiny = util_resident.tiny_pairs()
    _, tsizes = resident_store(tiny.samples)
    wide = tiny.pad_buckets(1, levels=1)                     # one real + one inert pair: the edgeless pattern leaves the inert one more edges than the largest has
    with pytest.raises(ValueError, match="an inert graph would exceed") as ref:
        _host(tiny, [0], wide, None)
    with pytest.raises(ValueError, match="an inert graph would exceed") as got:
        resident_plan(tsizes, [0], pad=wide)
    assert str(got.value) == str(ref.value)
    with pytest.raises(IndexError):
        resident_plan(tsizes, [4])


def test_the_views_that_carry_more_than_arrays_refuse():
    ds = util_resident.tiny_pairs()
    with pytest.raises(NotImplementedError):
        ds.lrp(2).resident("cuda")
    with pytest.raises(NotImplementedError):
        ds.edge_seq().resident("cuda")


def test_a_value_beyond_the_storage_type_is_a_value_error():
    from dualmessagepassing_amd.harness import PairDataset
    from dualmessagepassing_amd.resident import resident_store
    ds = util_resident.tiny_pairs()
    for field, value in (("eid", 2 ** 31), ("vlabel", -2 ** 31 - 1), ("rev", 2)):
        g = dict(ds.samples[3]["graph"])
        g[field] = np.asarray(g[field]).astype(np.int64).copy()
        g[field][0] = value
        samples = ds.samples[:3] + [dict(ds.samples[3], graph=g)]
        with pytest.raises(ValueError, match="graph." + field):
            resident_store(samples)
        with pytest.raises(ValueError, match="graph." + field):        # raised when the view is built, before any device is touched
            PairDataset(samples, ds.shape).resident("cuda")
    rows = dict(ds.samples[3], subisomorphisms=ds.samples[3]["subisomorphisms"] + 2 ** 31)
    with pytest.raises(ValueError, match="subisomorphisms"):
        resident_store([rows])
    assert resident_store(ds.samples[:3] + [dict(ds.samples[3], graph=dict(ds.samples[3]["graph"], eid=ds.samples[3]["graph"]["eid"] * 0 + 2 ** 31 - 1))])
