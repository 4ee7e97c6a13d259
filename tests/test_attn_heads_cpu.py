"""The attention prediction heads (Sum / Mean / Max AttnPredictNet, pred.py:490-643) on the CPU: construction through
``build_model`` for every rep-net, the reference's state_dict keys and seeded initial values, and the tensor-op path of the
sparsemax attention against the reference's own runs (tests/golden/attn/*.npz, scripts/make_golden_attn.py).
Tolerances: single ops 1e-5, stacked attention / heads 1e-4, parameter gradients 2e-4 (relative to max(1, |ref|max))."""
import glob
import os
import zlib

import numpy as np
import pytest
import torch as th

from conftest import GOLDEN, load_golden

ATTN = os.path.join(GOLDEN, "attn")
HEADS = ("SumAttnPredictNet", "MeanAttnPredictNet", "MaxAttnPredictNet")
REP_NETS = ("DMPNN", "CompGCN", "RGCN", "RGIN", "LRP", "DMPLRP")
VOCAB = dict(max_ngv=16, max_ngvl=4, max_nge=32, max_ngel=4, max_npv=8, max_npvl=4, max_npe=16, max_npel=4)


def _files(prefix):
    return sorted(glob.glob(os.path.join(ATTN, prefix + "*.npz")))


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


# ----------------------------------------------------------------------------- construction
@pytest.mark.parametrize("rep_net", REP_NETS)
@pytest.mark.parametrize("head", HEADS)
def test_build_model_constructs_attention_heads(rep_net, head):
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.pred import BaseAttnPredictNet
    model = build_model(rep_net=rep_net, pred_net=head, hid_dim=16, pred_hid_dim=16, pred_num_heads=4, pred_infer_steps=3, **VOCAB)
    heads = [h for h in model.pred_net.values() if h is not None] if isinstance(model.pred_net, th.nn.ModuleDict) else [model.pred_net]
    assert heads
    for h in heads:
        assert type(h).__name__ == head and isinstance(h, BaseAttnPredictNet)
        assert h.num_heads == 4 and h.infer_steps == 3 and not h.poolable()
        assert [k for k, _ in h.p_attn.named_parameters()] == ["weight_v", "weight_o", "weight_q", "weight_k", "g_net.weight",
                                                                "g_net.bias"]


def test_attention_head_defaults():
    from dualmessagepassing_amd.basemodel import build_model
    model = build_model(rep_net="DMPNN", pred_net="SumAttnPredictNet", hid_dim=16, pred_hid_dim=16, **VOCAB)
    assert model.pred_net["v"].num_heads == 4 and model.pred_net["v"].infer_steps == 1


def test_pooling_heads_unchanged():
    from dualmessagepassing_amd.basemodel import build_model
    for head in ("SumPredictNet", "MeanPredictNet", "MaxPredictNet"):
        model = build_model(rep_net="DMPNN", pred_net=head, hid_dim=16, pred_hid_dim=16, **VOCAB)
        assert not any(k.startswith("pred_net.v.p_attn") for k in model.state_dict())
        assert model.pred_net["v"].poolable() == (head != "MaxPredictNet")


def test_hidden_not_divisible_by_heads_raises():
    from dualmessagepassing_amd.basemodel import build_model
    with pytest.raises(ValueError):
        build_model(rep_net="DMPNN", pred_net="SumAttnPredictNet", hid_dim=16, pred_hid_dim=18, pred_num_heads=4, **VOCAB)


def test_kernel_head_widths_match_the_library():
    """The head widths the Python layer sends to the kernels are the ones the library takes (dmp_attn_supported_dh)."""
    from dualmessagepassing_amd import _lib
    from dualmessagepassing_amd.attn import KERNEL_DH
    lib = _lib.load()
    assert [d for d in range(1, 129) if lib.dmp_attn_supported_dh(d)] == list(KERNEL_DH)


def test_attention_on_cpu_takes_the_tensor_path():
    from dualmessagepassing_amd import attn
    q = th.randn(2, 3, 16)
    assert not attn.kernel_ok(q, q, q, 4)
    out = attn.sparsemax_attention(q, q, q, None, None, 4, 0.5)
    assert th.equal(out, attn.attention_tensor(q, q, q, None, None, 4, 0.5))


# ----------------------------------------------------------------------------- sparsemax and the attention core
@pytest.mark.parametrize("path", _files("sparsemax_"), ids=_id)
def test_sparsemax_matches_reference(path):
    from dualmessagepassing_amd.act import map_activation_str_to_layer
    d = load_golden(path)
    x = _t(d["x"]).clone().requires_grad_(True)
    km = _t(d["kmask"])
    B, _, Lk, _ = x.shape
    sm = map_activation_str_to_layer("sparsemax")
    sm_dim = sm.dim
    try:
        sm.dim = 2
        y = sm(x.masked_fill(km.view(B, 1, Lk, 1) == 0, -1e30))
    finally:
        sm.dim = sm_dim
    (y * _t(d["w"])).sum().backward()
    _close(y, d["y"], 1e-6, "sparsemax")
    _close(x.grad, d["dx"], 1e-5, "d scores")
    assert th.allclose(y.sum(2), th.ones(()), atol=1e-5)


@pytest.mark.parametrize("path", _files("dotattn_"), ids=_id)
def test_dot_attention_tensor_path_matches_reference(path):
    from dualmessagepassing_amd.pred import DotAttention
    d = load_golden(path)
    nh, dh = int(d["nh"]), int(d["dh"])
    query = _t(d["query"]).clone().requires_grad_(True)
    D = query.size(-1)
    attn = DotAttention(D, D, D, nh * dh, num_heads=nh, scale=1 / dh ** 0.5)
    attn.load_state_dict(_sd(d, "p."), strict=True)
    if bool(d["self"]):
        key = value = query
    else:
        key = _t(d["key"]).clone().requires_grad_(True)
        value = _t(d["value"]).clone().requires_grad_(True)
    out = attn(query, key, value, query_mask=_t(d["qmask"]), key_mask=_t(d["kmask"]))
    (out * _t(d["w"])).sum().backward()
    _close(out, d["out"], 1e-5, "out")
    _close(query.grad, d["dquery"], 1e-4, "dquery")
    if not bool(d["self"]):
        _close(key.grad, d["dkey"], 1e-4, "dkey")
        _close(value.grad, d["dvalue"], 1e-4, "dvalue")
    for k, p in attn.named_parameters():
        _close(p.grad, d["g." + k], 2e-4, "grad " + k)


# ----------------------------------------------------------------------------- the three heads standalone
HEAD_CLS = {"sum": "SumAttnPredictNet", "mean": "MeanAttnPredictNet", "max": "MaxAttnPredictNet"}


def _head_from(d, tag):
    from dualmessagepassing_amd import pred
    cls = getattr(pred, HEAD_CLS[tag.split("_")[1]])
    th.manual_seed(_seed("head", tag[len("head_"):]))
    D = d["p_rep"].shape[-1]
    return cls(D, int(d["hid"]), num_heads=int(d["nh"]), infer_steps=int(d["steps"]), act_func="relu", dropout=0.0,
               return_weights=bool(d["rw"]))


@pytest.mark.parametrize("path", _files("head_"), ids=_id)
def test_head_seeded_init_equals_reference(path):
    d = load_golden(path)
    head = _head_from(d, _id(path))
    ref = _sd(d, "sd_init.")
    got = head.state_dict()
    assert list(got) == list(ref)
    for k in ref:
        assert th.equal(got[k], ref[k]), k


@pytest.mark.parametrize("path", _files("head_"), ids=_id)
def test_head_tensor_path_matches_reference(path):
    d = load_golden(path)
    head = _head_from(d, _id(path))
    head.load_state_dict(_sd(d, "sd."), strict=True)
    p_rep = _t(d["p_rep"]).clone().requires_grad_(True)
    g_rep = _t(d["g_rep"]).clone().requires_grad_(True)
    y, w = head(p_rep, _t(d["p_mask"]), g_rep, _t(d["g_mask"]))
    loss = y.sum()
    if bool(d["rw"]):
        _close(w, d["weights"], 1e-4, "weights")
        loss = loss + (w * _t(d["ww"])).sum()
    else:
        assert w is None
    loss.backward()
    _close(y, d["y"], 1e-4, "count")
    _close(p_rep.grad, d["dp_rep"], 2e-4, "dp_rep")
    _close(g_rep.grad, d["dg_rep"], 2e-4, "dg_rep")
    for k, p in head.named_parameters():
        _close(p.grad, d["g." + k], 2e-4, "grad " + k)


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
    th.manual_seed(_seed("attn-model", key))
    return build_model(**_config(d))


@pytest.mark.parametrize("path", _files("model_"), ids=_id)
def test_model_seeded_init_and_strict_load(path):
    d = load_golden(path)
    model = _model_from(d, _id(path).split("_")[1])
    ref = _sd(d, "sd_init.")
    got = model.state_dict()
    assert list(got) == list(ref)
    for k in ref:
        assert th.equal(got[k], ref[k]), k
    missing, unexpected = model.load_state_dict(_sd(d, "sd."), strict=True)
    assert not missing and not unexpected


@pytest.mark.parametrize("path", _files("model_"), ids=_id)
def test_model_heads_on_reference_reps(path):
    """``get_subiso_pred`` (the padded path the attention heads take) on the reference's own representations: count,
    matching weights and every gradient of the heads' parameters."""
    d = load_golden(path)
    model = _model_from(d, _id(path).split("_")[1])
    model.load_state_dict(_sd(d, "sd."), strict=True)
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
def test_expand_with_attention_head(path):
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
    assert any(".p_attn." in k for k in ref)
    for k in ref:
        assert got[k].shape == ref[k].shape and th.equal(got[k], ref[k]), k
