"""The memory heads (Sum / Mean / Max MemAttnPredictNet and DIAMNet, pred.py:648-1328) on the CPU: construction through
``build_model`` for every rep-net, the defaults, the refused mem_init values, the reference's state_dict keys and seeded
initial values, and the tensor-op path of the memory initialisation against the reference's own runs
(tests/golden/mem/*.npz, scripts/make_golden_mem.py).
Tolerances: the memory 1e-6, MemDotAttention 1e-5, heads 1e-4, parameter gradients 2e-4 (relative to max(1, |ref|max))."""
import glob
import os
import zlib

import numpy as np
import pytest
import torch as th

from conftest import GOLDEN, load_golden

MEM = os.path.join(GOLDEN, "mem")
HEADS = ("SumMemAttnPredictNet", "MeanMemAttnPredictNet", "MaxMemAttnPredictNet", "DIAMNet")
REP_NETS = ("DMPNN", "CompGCN", "RGCN", "RGIN", "LRP", "DMPLRP")
VOCAB = dict(max_ngv=16, max_ngvl=4, max_nge=32, max_ngel=4, max_npv=8, max_npvl=4, max_npe=16, max_npel=4)


def _files(prefix):
    return sorted(glob.glob(os.path.join(MEM, prefix + "*.npz")))


def _id(p):
    return os.path.basename(p)[:-4]


def _t(a):
    return th.from_numpy(np.asarray(a))


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % (2 ** 31)


def _close(got, ref, tol, what):
    got, ref = got.detach().double(), _t(ref).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = max(1.0, float(ref.abs().max())) if ref.numel() else 1.0
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    assert err <= tol * scale, "%s: max err %g (scale %g)" % (what, err, scale)


def _config(d, prefix="config"):
    return {str(k): eval(str(v)) for k, v in zip(d[prefix + "_keys"], d[prefix + "_vals"])}


def _sd(d, prefix):
    return {k[len(prefix):]: _t(v) for k, v in d.items() if k.startswith(prefix)}


def _heads(model):
    if isinstance(model.pred_net, th.nn.ModuleDict):
        return [h for h in model.pred_net.values() if h is not None]
    return [model.pred_net]


# ----------------------------------------------------------------------------- construction
@pytest.mark.parametrize("rep_net", REP_NETS)
@pytest.mark.parametrize("head", HEADS)
def test_build_model_constructs_memory_heads(rep_net, head):
    from dualmessagepassing_amd.basemodel import build_model
    model = build_model(rep_net=rep_net, pred_net=head, hid_dim=16, pred_hid_dim=16, pred_num_heads=4, pred_infer_steps=3,
                        pred_mem_len=3, **VOCAB)
    heads = _heads(model)
    assert heads
    for h in heads:
        assert type(h).__name__ == head and not h.poolable()
        assert h.num_heads == 4 and h.infer_steps == 3 and h.mem_len == 3
        if head == "DIAMNet":
            assert [k for k, _ in h.named_children()] == ["act", "drop", "p_fc", "g_fc", "pred_fc2", "mem_layer", "p_attn",
                                                          "g_attn", "m_attn", "pred_fc1"]
            assert h.pred_fc1.in_features == 16 * 3 + 4
        else:
            assert [k for k, _ in h.p_attn.named_parameters()] == [
                "weight_v", "weight_o", "weight_q", "weight_k", "g_net.weight", "g_net.bias", "q_layer_norm.weight",
                "q_layer_norm.bias", "k_layer_norm.weight", "k_layer_norm.bias", "v_layer_norm.weight", "v_layer_norm.bias",
                "proj_k.weight", "proj_k.bias", "proj_v.weight", "proj_v.bias"]
            assert h.p_attn.scale == 1.0 and h.p_attn.pre_lnorm


def test_memory_head_defaults():
    from dualmessagepassing_amd.basemodel import build_model
    want = {"SumMemAttnPredictNet": "sum", "MeanMemAttnPredictNet": "mean", "MaxMemAttnPredictNet": "max", "DIAMNet": "mean"}
    for head, mem_init in want.items():
        # pred_mem_init reaches DIAMNet only: the memory-attention heads keep their class default
        model = build_model(rep_net="DMPNN", pred_net=head, hid_dim=16, pred_hid_dim=16, **VOCAB)
        h = model.pred_net["v"]
        assert (h.num_heads, h.infer_steps, h.mem_len, h.mem_init) == (4, 1, 4, mem_init)
        model = build_model(rep_net="DMPNN", pred_net=head, hid_dim=16, pred_hid_dim=16, pred_mem_init="circular_max", **VOCAB)
        assert model.pred_net["v"].mem_init == ("circular_max" if head == "DIAMNet" else mem_init)


@pytest.mark.parametrize("mem_init", ["attn", "lstm", "circular_attn", "circular_lstm"])
def test_attn_and_lstm_memory_init_raise(mem_init):
    from dualmessagepassing_amd import pred
    from dualmessagepassing_amd.basemodel import build_model
    with pytest.raises(NotImplementedError, match="not built"):
        build_model(rep_net="DMPNN", pred_net="DIAMNet", hid_dim=16, pred_hid_dim=16, pred_mem_init=mem_init, **VOCAB)
    with pytest.raises(NotImplementedError, match="not built"):
        pred.SumMemAttnPredictNet(16, 16, num_heads=4, mem_init=mem_init)
    with pytest.raises(ValueError):
        pred.DIAMNet(16, 16, mem_init="median")


def test_diamnet_return_weights_needs_mem_len_4():
    from dualmessagepassing_amd import pred
    with pytest.raises(ValueError, match="mem_len == 4"):
        pred.DIAMNet(16, 16, num_heads=4, mem_len=3, return_weights=True)
    pred.DIAMNet(16, 16, num_heads=4, mem_len=3, return_weights=False)
    assert pred.DIAMNet(16, 16, num_heads=4, mem_len=4, return_weights=True).weight_fc1.in_features == 16 * 4 + 2


def test_dot_attention_default_has_no_layer_norm():
    from dualmessagepassing_amd.pred import DotAttention
    a = DotAttention(8, 8, 8, 8, num_heads=2)
    assert not a.pre_lnorm and not any("layer_norm" in k for k in a.state_dict())


def test_memory_on_cpu_takes_the_tensor_path(monkeypatch):
    from dualmessagepassing_amd import mem
    x = th.randn(2, 5, 8)
    m = th.ones(2, 5, dtype=th.bool)
    assert not mem.kernel_ok([x])
    monkeypatch.setattr(mem.MemInit, "apply", lambda *a: pytest.fail("kernel path on the CPU"))
    (y,), mm = mem.memory_init([x], m, 2, "mean")
    assert y.shape == (2, 2, 8) and mm.dtype == th.bool


# ----------------------------------------------------------------------------- the memory initialisation
@pytest.mark.parametrize("path", _files("initmem_"), ids=_id)
def test_memory_tensor_path_matches_reference(path):
    from dualmessagepassing_amd.mem import memory_init
    d = load_golden(path)
    M, mode, mask = int(d["M"]), str(d["mode"]), _t(d["mask"])
    for cls, inclusive in (("memattn", False), ("diam", True)):
        x = _t(d["x"]).clone().requires_grad_(True)
        (m,), mm = memory_init([x], mask, M, mode, inclusive_end=inclusive)
        (m * _t(d[cls + ".w"])).sum().backward()
        _close(m, d[cls + ".mem"], 1e-6, cls + " memory")
        assert th.equal(mm, _t(d[cls + ".mem_mask"])), cls + " memory mask"
        _close(x.grad, d[cls + ".dx"], 1e-6, cls + " dx")


def test_memory_of_two_tensors_shares_the_windows():
    from dualmessagepassing_amd.mem import memory_init
    d = load_golden(_files("initmem_circular_max_m4_mixed")[0])
    x = _t(d["x"])
    (a, b), mm = memory_init([x, -x], _t(d["mask"]), 4, "circular_max")
    (c,), mm1 = memory_init([x], _t(d["mask"]), 4, "circular_max")
    (e,), _ = memory_init([-x], _t(d["mask"]), 4, "circular_max")
    assert th.equal(a, c) and th.equal(b, e) and th.equal(mm, mm1)


@pytest.mark.parametrize("path", _files("memattn_"), ids=_id)
def test_mem_dot_attention_tensor_path_matches_reference(path):
    from dualmessagepassing_amd.pred import MemDotAttention
    d = load_golden(path)
    dq, dk, hid, nh = int(d["dq"]), int(d["dk"]), int(d["hid"]), int(d["nh"])
    attn = MemDotAttention(dq, dk, dk, hid, hid, num_heads=nh, scale=1.0, mem_len=int(d["M"]), mem_init=str(d["mode"]),
                           pre_lnorm=True)
    attn.load_state_dict(_sd(d, "p."), strict=True)
    assert [k for k, _ in attn.named_parameters()] == [k[2:] for k in d if k.startswith("p.")]
    query, key, value = (_t(d[k]).clone().requires_grad_(True) for k in ("query", "key", "value"))
    out = attn(query, key, value, query_mask=_t(d["qmask"]), key_mask=_t(d["kmask"]))
    (out * _t(d["w"])).sum().backward()
    _close(out, d["out"], 1e-5, "out")
    for k, t in (("dquery", query), ("dkey", key), ("dvalue", value)):
        _close(t.grad, d[k], 1e-4, k)
    for k, p in attn.named_parameters():
        _close(p.grad, d["g." + k], 2e-4, "grad " + k)


# ----------------------------------------------------------------------------- the four heads standalone
def _head_from(d, tag):
    from dualmessagepassing_amd import pred
    th.manual_seed(_seed("memhead", tag[len("head_"):]))
    kw = dict(num_heads=int(d["nh"]), infer_steps=int(d["steps"]), mem_len=int(d["M"]), act_func="relu", dropout=0.0,
              return_weights=bool(d["rw"]))
    if str(d["mem_init"]):
        kw["mem_init"] = str(d["mem_init"])
    return getattr(pred, str(d["cls"]))(d["p_rep"].shape[-1], int(d["hid"]), **kw)


@pytest.mark.parametrize("path", _files("head_"), ids=_id)
def test_head_seeded_init_equals_reference(path):
    d = load_golden(path)
    head = _head_from(d, _id(path))
    ref = _sd(d, "sd_init.")
    got = head.state_dict()
    assert list(got) == list(ref)
    for k in ref:
        assert th.equal(got[k], ref[k]), k


def _load_head(d, path):
    head = _head_from(d, _id(path))
    head.load_state_dict(dict(_sd(d, "sd_init."), **_sd(d, "sd.")), strict=True)
    return head


def run_head(head, d, dev=None):
    dev = dev or th.device("cpu")
    p_rep = _t(d["p_rep"]).to(dev).requires_grad_(True)
    g_rep = _t(d["g_rep"]).to(dev).requires_grad_(True)
    y, w = head(p_rep, _t(d["p_mask"]).to(dev), g_rep, _t(d["g_mask"]).to(dev))
    loss = y.sum()
    if bool(d["rw"]):
        _close(w.cpu(), d["weights"], 1e-4, "weights")
        loss = loss + (w * _t(d["ww"]).to(dev)).sum()
    else:
        assert w is None
    loss.backward()
    _close(y.cpu(), d["y"], 1e-4, "count")
    _close(p_rep.grad.cpu(), d["dp_rep"], 2e-4, "dp_rep")
    _close(g_rep.grad.cpu(), d["dg_rep"], 2e-4, "dg_rep")
    for k, p in head.named_parameters():
        if "g." + k not in d:                 # unused without return_weights (DIAMNet's p_fc, g_fc, m_attn)
            assert p.grad is None, k
            continue
        _close(p.grad.cpu(), d["g." + k], 2e-4, "grad " + k)


@pytest.mark.parametrize("path", _files("head_"), ids=_id)
def test_head_tensor_path_matches_reference(path):
    d = load_golden(path)
    run_head(_load_head(d, path), d)


# ----------------------------------------------------------------------------- full models
def _pad(rows, sizes, L):
    """pre_pad batchify (utils/dl.py:51-81): the rows of graph i land in [i, L - size_i:]."""
    out = rows.new_zeros((len(sizes), L, rows.size(1)))
    off = 0
    for i, n in enumerate(sizes):
        out[i, L - n:] = rows[off:off + n]
        off += n
    return out


def _model_from(d, key):
    from dualmessagepassing_amd.basemodel import build_model
    th.manual_seed(_seed("mem-model", key))
    return build_model(**_config(d))


def model_state(d):
    return dict(_sd(d, "sd_init."), **_sd(d, "sd."))


@pytest.mark.parametrize("path", _files("model_"), ids=_id)
def test_model_seeded_init_and_strict_load(path):
    d = load_golden(path)
    model = _model_from(d, _id(path).split("_")[1])
    ref = _sd(d, "sd_init.")
    got = model.state_dict()
    assert list(got) == list(ref)
    for k in ref:
        assert th.equal(got[k], ref[k]), k
    missing, unexpected = model.load_state_dict(model_state(d), strict=True)
    assert not missing and not unexpected


@pytest.mark.parametrize("path", _files("model_"), ids=_id)
def test_model_heads_on_reference_reps(path):
    """``get_subiso_pred`` (the padded path the memory heads take) on the reference's own representations: count,
    matching weights and every gradient of the heads' parameters."""
    d = load_golden(path)
    model = _model_from(d, _id(path).split("_")[1])
    model.load_state_dict(model_state(d), strict=True)
    bnn = {t: [int(x) for x in d[t + "_bnn"]] for t in "pg"}
    bne = {t: [int(x) for x in d[t + "_bne"]] for t in "pg"}
    pads, masks = {}, {}
    for t in "pg":
        for kind, sizes in (("v", bnn[t]), ("e", bne[t])):
            if "out.%s_%s_rep" % (t, kind) not in d:
                continue
            m = _t(d["out.%s_%s_mask" % (t, kind)])
            rows = _pad(_t(d["out.%s_%s_rep" % (t, kind)]), sizes, m.size(1))
            pads[t + kind] = rows.masked_fill(~m.unsqueeze(-1), 0)
            masks[t + kind] = m
    if "pe" in pads:
        pred_c, (pred_v, pred_e) = model.get_subiso_pred(pads["pv"], masks["pv"], pads["pe"], masks["pe"], pads["gv"], masks["gv"],
                                                        pads["ge"], masks["ge"])
    else:
        pred_c, (pred_v, pred_e) = model.get_subiso_pred(pads["pv"], masks["pv"], pads["gv"], masks["gv"])
    _close(pred_c, d["out.pred_c"], 1e-4, "pred_c")
    total = pred_c.sum()
    for k, v in (("pred_v", pred_v), ("pred_e", pred_e)):
        if "out." + k in d:
            _close(v, d["out." + k], 1e-4, k)
            total = total + v.sum()
        else:
            assert v is None
    total.backward()
    n = 0
    for k, p in model.named_parameters():
        if k.startswith("pred_net"):
            _close(p.grad, d["grad." + k], 2e-4, "grad " + k)
            n += 1
    assert n > 0


@pytest.mark.parametrize("path", _files("expand_"), ids=_id)
def test_expand_with_diamnet(path):
    from dualmessagepassing_amd.basemodel import build_model
    d = load_golden(path)
    config = _config(d)
    grow = {str(k): int(v) for k, v in zip(d["grow_keys"], d["grow_vals"])}
    model = build_model(**config)
    model.load_state_dict(_sd(d, "sd."), strict=True)
    model.expand(**dict(config, **grow))
    ref = _sd(d, "sd_after.")
    got = model.state_dict()
    assert sorted(got) == sorted(ref)
    assert any(".mem_layer." in k for k in ref) and any(".m_attn." in k for k in ref)
    for k in ref:
        assert got[k].shape == ref[k].shape and th.equal(got[k], ref[k]), k
