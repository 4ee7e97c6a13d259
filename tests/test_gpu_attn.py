"""The sparsemax attention kernels (csrc/dmp_attn.hip) and the attention prediction heads on the GPU.

* kernel forward / backward against an fp64 restatement (``attn.attention_tensor`` in double) over odd and long key
  counts (both sides of the LDS score cache's 2048), Lq != Lk, non-prefix key masks, all-masked rows, masked query
  rows, 1 and 4 heads and every head width of ``attn.KERNEL_DH``.  Rows whose fp64 scores come within a relative 1e-4 of
  their threshold (a key that fp32 rounding may move in or out of the support) are taken out by their query mask;
* bitwise reproducibility, every output written (DMP_POISON_DEAD_ROWS), the dispatch to the tensor-op path;
* the fixtures of scripts/make_golden_attn.py (the reference's own runs) through the HIP path: DotAttention, the three
  heads standalone, and the DMPNN / RGIN models with attention heads (OutputDict, pred_v / pred_e, parameter gradients);
* a recorded training step (harness.GraphedTrainStep) of DMPNN + SumAttnPredictNet replays what the eager step computes.
Tolerances: forward 1e-5, gradients 1e-4 (fp64 restatement); fixtures as tests/test_gpu_fullmodel.py."""
import copy
import glob
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch as th

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu
ATTN = os.path.join(GOLDEN, "attn")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INLINE = os.environ.get("DMP_ATTN_TESTS_INLINE") == "1"
inner = pytest.mark.skipif(not INLINE, reason="runs in a child process started by its test_* wrapper")
outer = pytest.mark.skipif(INLINE, reason="wrapper: the child process runs the inner case")


def _t(a):
    return th.from_numpy(np.asarray(a))


def _close(got, ref, tol, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu() if th.is_tensor(ref) else _t(ref).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not th.isnan(got).any(), what
    scale = max(1.0, float(ref.abs().max())) if ref.numel() else 1.0
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    assert err <= tol * scale, "%s: max err %g (scale %g)" % (what, err, scale)


# ----------------------------------------------------------------------------- kernels against fp64
def _case(B, Lq, Lk, nh, dh, seed):
    """Inputs with non-prefix key masks, one all-masked pair (B > 1), masked query rows; rows near a kink masked out."""
    from dualmessagepassing_amd.attn import sparsemax
    g = th.Generator().manual_seed(seed)
    D = nh * dh
    q = th.randn(B, Lq, D, generator=g, dtype=th.float64) * 2.0
    k = th.randn(B, Lk, D, generator=g, dtype=th.float64)
    v = th.randn(B, Lk, D, generator=g, dtype=th.float64)
    km = th.rand(B, Lk, generator=g) > 0.3
    km[:, Lk // 2] = True
    if B > 1:
        km[1] = False
    qm = th.rand(B, Lq, generator=g) > 0.2
    qm[0, 0] = False
    qm[0, -1] = True
    q, k, v = q.float().double(), k.float().double(), v.float().double()        # fp32-representable inputs
    scale = 1.0 / dh ** 0.5
    s = th.einsum("bind,bjnd->bijn", q.view(B, Lq, nh, dh), k.view(B, Lk, nh, dh)) * scale
    s = s.masked_fill(km.view(B, 1, Lk, 1) == 0, -1e30)
    p = sparsemax(s, dim=2)
    live = km.view(B, 1, Lk, 1).expand_as(s)
    tau = (s - p).masked_fill(p == 0, float("inf")).amin(dim=2, keepdim=True)    # s - p on the support
    gap = (s - tau).abs().masked_fill(~live, float("inf")).amin(dim=2)             # [B, Lq, nh]
    ref = th.maximum(s.masked_fill(~live, 0).abs().amax(dim=2), th.ones(()))
    near = ((gap < 1e-4 * ref) & km.any(dim=1).view(B, 1, 1)).any(dim=2)             # [B, Lq]
    qm = qm & ~near
    return q, k, v, qm, km, scale


def _run(q, k, v, qm, km, nh, scale, dev, dout):
    from dualmessagepassing_amd.attn import SparsemaxAttention
    qg, kg, vg = (x.float().to(dev).requires_grad_(True) for x in (q, k, v))
    o, tau, supp = SparsemaxAttention.apply(qg, kg, vg, qm.to(dev), km.to(dev), nh, scale)
    o.backward(dout.float().to(dev))
    th.cuda.synchronize()
    return o, tau, supp, qg.grad, kg.grad, vg.grad


def _ref(q, k, v, qm, km, nh, scale, dout):
    from dualmessagepassing_amd.attn import attention_tensor
    qd, kd, vd = (x.clone().requires_grad_(True) for x in (q, k, v))
    o = attention_tensor(qd, kd, vd, qm, km, nh, scale)
    o.backward(dout)
    return o, qd.grad, kd.grad, vd.grad


def _shape(Lk):
    return (1, 5) if Lk > 1000 else (3, 7 if Lk != 7 else 9)


@pytest.mark.parametrize("Lk", [1, 3, 17, 64, 512, 2049, 8192])
@pytest.mark.parametrize("dh", [4, 8, 16, 32, 64])
@pytest.mark.parametrize("nh", [1, 4])
def test_kernel_matches_fp64(Lk, dh, nh, gpu):
    B, Lq = _shape(Lk)
    q, k, v, qm, km, scale = _case(B, Lq, Lk, nh, dh, zlib.crc32(repr((Lk, dh, nh)).encode()))
    dout = th.randn(q.shape, generator=th.Generator().manual_seed(Lk + dh), dtype=th.float64).float().double()
    o, tau, supp, dq, dk, dv = _run(q, k, v, qm, km, nh, scale, gpu, dout)
    ro, rdq, rdk, rdv = _ref(q, k, v, qm, km, nh, scale, dout)
    _close(o, ro, 1e-5, "O")
    _close(dq, rdq, 1e-4, "dQ")
    _close(dk, rdk, 1e-4, "dK")
    _close(dv, rdv, 1e-4, "dV")
    # rows with every key masked: support size 0; masked query rows: zeros
    if B > 1:
        assert int(supp[1].abs().max()) == 0
    if (~qm).any():
        assert float(o[~qm.to(gpu)].abs().max()) == 0.0


def test_kernel_is_bitwise_reproducible(gpu):
    for Lk, dh, nh in ((512, 16, 4), (2049, 32, 1)):
        B, Lq = (4, 64) if Lk < 1000 else (1, 9)
        q, k, v, qm, km, scale = _case(B, Lq, Lk, nh, dh, 5)
        dout = th.randn(q.shape, generator=th.Generator().manual_seed(1), dtype=th.float64)
        a = _run(q, k, v, qm, km, nh, scale, gpu, dout)
        b = _run(q, k, v, qm, km, nh, scale, gpu, dout)
        for x, y in zip(a, b):
            assert th.equal(x, y)


def test_every_output_is_written(gpu, monkeypatch):
    from dualmessagepassing_amd import fused
    monkeypatch.setattr(fused, "POISON_DEAD_ROWS", True)
    for Lk, dh in ((17, 16), (2049, 8)):
        B, Lq = _shape(Lk)
        q, k, v, qm, km, scale = _case(B, Lq, Lk, 4, dh, 9)
        dout = th.randn(q.shape, dtype=th.float64)
        for x in _run(q, k, v, qm, km, 4, scale, gpu, dout):
            assert not (th.isnan(x).any() if x.dtype.is_floating_point else (x == -1).any())


def test_dispatch_kernel_or_tensor_path(gpu, monkeypatch):
    """Head widths in KERNEL_DH take the kernels, also from contiguous views that start 4 bytes into a larger buffer (the
    kernels load float4: SparsemaxAttention copies those); other widths and non-fp32 inputs take the tensor-op path."""
    from dualmessagepassing_amd import attn
    calls = []
    orig = attn.attention_tensor
    monkeypatch.setattr(attn, "attention_tensor", lambda *a: (calls.append(1), orig(*a))[1])
    for dh, dtype, want_kernel, offset in ((16, th.float32, True, 0), (4, th.float32, True, 0), (12, th.float32, False, 0),
                                           (2, th.float32, False, 0), (16, th.float64, False, 0), (16, th.float32, True, 1)):
        q = th.randn(2 * 5 * 4 * dh + offset, device=gpu, dtype=dtype)[offset:].view(2, 5, 4 * dh)
        k = th.randn(2 * 6 * 4 * dh + offset, device=gpu, dtype=dtype)[offset:].view(2, 6, 4 * dh)
        assert q.data_ptr() % 16 == 4 * offset and k.data_ptr() % 16 == 4 * offset and q.is_contiguous() and k.is_contiguous()
        assert attn.kernel_ok(q, k, k, 4) == want_kernel
        n = len(calls)
        out = attn.sparsemax_attention(q, k, k, None, None, 4, 0.5)
        assert (len(calls) == n) == want_kernel
        ref = orig(q.double().cpu(), k.double().cpu(), k.double().cpu(), None, None, 4, 0.5)
        _close(out, ref, 1e-5, "dh %d" % dh)
    assert not attn.kernel_ok(q.cpu().float(), k.cpu().float(), k.cpu().float(), 4)


# ----------------------------------------------------------------------------- the reference's fixtures on the HIP path
@pytest.fixture
def kernels_only(monkeypatch):
    """Fail instead of taking the tensor-op path."""
    from dualmessagepassing_amd import attn

    def no(*a, **k):
        raise AssertionError("the tensor-op attention path ran where the HIP kernels should")
    monkeypatch.setattr(attn, "attention_tensor", no)


def _sd(d, prefix):
    return {k[len(prefix):]: _t(v) for k, v in d.items() if k.startswith(prefix)}


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(ATTN, "dotattn_*.npz"))), ids=lambda p: os.path.basename(p)[:-4])
def test_dot_attention_fixture_on_gpu(path, gpu, kernels_only):
    from dualmessagepassing_amd.pred import DotAttention
    d = load_golden(path)
    nh, dh = int(d["nh"]), int(d["dh"])
    query = _t(d["query"]).to(gpu).requires_grad_(True)
    D = query.size(-1)
    attn = DotAttention(D, D, D, nh * dh, num_heads=nh, scale=1 / dh ** 0.5)
    attn.load_state_dict(_sd(d, "p."), strict=True)
    attn.to(gpu)
    key = value = query
    if not bool(d["self"]):
        key = _t(d["key"]).to(gpu).requires_grad_(True)
        value = _t(d["value"]).to(gpu).requires_grad_(True)
    out = attn(query, key, value, query_mask=_t(d["qmask"]).to(gpu), key_mask=_t(d["kmask"]).to(gpu))
    (out * _t(d["w"]).to(gpu)).sum().backward()
    _close(out, d["out"], 1e-5, "out")
    _close(query.grad, d["dquery"], 1e-4, "dquery")
    if not bool(d["self"]):
        _close(key.grad, d["dkey"], 1e-4, "dkey")
        _close(value.grad, d["dvalue"], 1e-4, "dvalue")
    for k, p in attn.named_parameters():
        _close(p.grad, d["g." + k], 2e-4, "grad " + k)


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(ATTN, "head_*.npz"))), ids=lambda p: os.path.basename(p)[:-4])
def test_head_fixture_on_gpu(path, gpu, kernels_only):
    from dualmessagepassing_amd import pred
    d = load_golden(path)
    cls = getattr(pred, {"sum": "SumAttnPredictNet", "mean": "MeanAttnPredictNet", "max": "MaxAttnPredictNet"}[
        os.path.basename(path).split("_")[1]])
    D = d["p_rep"].shape[-1]
    head = cls(D, int(d["hid"]), num_heads=int(d["nh"]), infer_steps=int(d["steps"]), return_weights=bool(d["rw"]))
    head.load_state_dict(_sd(d, "sd."), strict=True)
    head.to(gpu)
    p_rep = _t(d["p_rep"]).to(gpu).requires_grad_(True)
    g_rep = _t(d["g_rep"]).to(gpu).requires_grad_(True)
    y, w = head(p_rep, _t(d["p_mask"]).to(gpu), g_rep, _t(d["g_mask"]).to(gpu))
    loss = y.sum()
    if bool(d["rw"]):
        _close(w, d["weights"], 1e-4, "weights")
        loss = loss + (w * _t(d["ww"]).to(gpu)).sum()
    loss.backward()
    _close(y, d["y"], 1e-4, "count")
    _close(p_rep.grad, d["dp_rep"], 2e-4, "dp_rep")
    _close(g_rep.grad, d["dg_rep"], 2e-4, "dg_rep")
    for k, p in head.named_parameters():
        _close(p.grad, d["g." + k], 2e-4, "grad " + k)


def _graph(d, t, dev):
    from dualmessagepassing_amd.graph import BatchedGraph
    g = BatchedGraph(_t(d[t + "_src"]).to(dev), _t(d[t + "_dst"]).to(dev), int(d[t + "_num_nodes"]),
                     _t(d[t + "_bnn"]).to(dev), _t(d[t + "_bne"]).to(dev))
    for k, v in d.items():
        if k.startswith(t + "_ndata."):
            g.ndata[k.split(".", 1)[1]] = _t(v).to(dev)
        if k.startswith(t + "_edata."):
            g.edata[k.split(".", 1)[1]] = _t(v).to(dev)
    return g


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(ATTN, "model_*.npz"))), ids=lambda p: os.path.basename(p)[:-4])
def test_model_fixture_on_gpu(path, gpu, kernels_only):
    from dualmessagepassing_amd.basemodel import build_model
    d = load_golden(path)
    config = {str(k): eval(str(v)) for k, v in zip(d["config_keys"], d["config_vals"])}
    model = build_model(**config)
    missing, unexpected = model.load_state_dict(_sd(d, "sd."), strict=True)
    assert not missing and not unexpected
    model.to(gpu)
    out = model(_graph(d, "p", gpu), _graph(d, "g", gpu))
    for k in ("p_v_mask", "p_e_mask", "g_v_mask", "g_e_mask"):
        if "out." + k in d:
            assert th.equal(out[k].cpu(), _t(d["out." + k])), k
    for k in ("p_v_emb", "p_e_emb", "g_v_emb", "g_e_emb"):
        if "out." + k in d:
            _close(out[k], d["out." + k], 1e-5, k)
    for k in ("p_v_rep", "p_e_rep", "g_v_rep", "g_e_rep", "pred_c"):
        if "out." + k in d:
            _close(out[k], d["out." + k], 1e-4, k)
    total = out["pred_c"].sum()
    for k in ("pred_v", "pred_e"):
        if "out." + k in d:
            _close(out[k], d["out." + k], 1e-4, k)
            total = total + out[k].sum()
        else:
            assert out[k] is None
    total.backward()
    for k, p in model.named_parameters():
        if "grad." + k in d:
            _close(p.grad, d["grad." + k], 2e-4, "grad " + k)


# ----------------------------------------------------------------------------- recorded training step
def _isolated(node):
    env = dict(os.environ, DMP_ATTN_TESTS_INLINE="1")
    r = subprocess.run([sys.executable, "-X", "faulthandler", "-m", "pytest", "%s::%s" % (os.path.abspath(__file__), node), "-q", "-x",
                        "-p", "no:cacheprovider"], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-25:])
    assert r.returncode == 0 and " passed" in r.stdout, "child exited with %s:\n%s" % (r.returncode, tail)


@outer
def test_graphed_training_with_attention_head(gpu):
    _isolated("test_inner_graphed_training_with_attention_head")


@inner
def test_inner_graphed_training_with_attention_head(gpu):
    """Two epochs of count-loss training of DMPNN + SumAttnPredictNet (4 heads, 3 inference steps: the padded,
    non-poolable head path), eager vs HIP-graph replay from the same initial state: same losses, same parameters."""
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.dp import FlatAdamW, FlatGradSync
    from dualmessagepassing_amd.harness import GraphedTrainStep, SyntheticPairs, train_epoch
    ds = SyntheticPairs(56, 3, 2, 8, 16, 2, 1, seed=11)
    th.manual_seed(5)
    base = build_model(**ds.model_config(hid_dim=64, layers=2, pred_net="SumAttnPredictNet", pred_num_heads=4,
                                         pred_infer_steps=3)).to(gpu)
    runs = []
    for graphed in (False, True):
        model = copy.deepcopy(base)
        sync = FlatGradSync(model)
        master = sync.flatten_parameters()
        start = master.detach().clone()
        opt = FlatAdamW([master], lr=2e-3, weight_decay=1e-5, amsgrad=True, capturable=graphed)
        step = GraphedTrainStep(model, opt, sync) if graphed else None
        trace = []
        for epoch in range(2):
            train_epoch(model, opt, ds, 16, gpu, sync=sync, neg_slp=0.01, order=np.random.default_rng(epoch).permutation(len(ds)),
                        trace=trace, graph=step)
        th.cuda.synchronize()
        runs.append((th.stack([t[0] for t in trace]).cpu(), master.detach().clone(), step))
    (l0, p0, _), (l1, p1, step) = runs
    assert step.steps.replays >= 2 * 4 - 4, (step.steps.replays, step.steps.eager_calls)
    assert th.allclose(l0, l1, rtol=1e-5, atol=1e-6), (l0 - l1).abs().max()
    assert float((p0 - p1).abs().max()) <= 1e-5 * float(p0.abs().max()), float((p0 - p1).abs().max())
    assert float((p0 - start).abs().max()) > 1e-3
